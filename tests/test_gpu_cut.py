"""The block cut (bz2_rle.hip k_cut_tab + k_cut) steered to the edge of its
table.  k_cut_tab tabulates, for block k and e < 128, the first chunk start at
or past (k + 1) * nblockMAX + e; the walk reads entry e_k = W_k - k *
nblockMAX, which grows by each cut's overshoot (0..4) and so reaches the
table's upper edge only after 31 blocks with a heavy chunk across almost every
target.  tests/cut_model.py (pinned to libbz2 by test_cut_model_cpu.py) builds
such streams and says which entry every block reads; each case's aim is
asserted on the model before the stream goes to the GPU:
  (a) the last full block reads e = 120..127 and wants offset e + 4 -- from
      124 on beyond the recorded offsets -- with 1 B .. 8 KB of text after
      that start, the row's two tiles just reaching and just missing the end
  (b) the same on a middle block       (c) e = 128.. (no table entry)
  (d) no chunk start left: the stream ends inside the chunk that crosses the
      last target, or exactly at the target
  (e) 35 blocks of overshoot patterns  (f) batches with several streams
  (g) (a), (c), (d) again with STARCH_CUT_TAB=0, the walk that searches the
      text for every block, in a child process (the variable is read once)
Every stream must equal libbz2's byte for byte: the C restatement
(oracle_lib.bz2) and, where built, the reference library itself.  Level 1
throughout (31 blocks of 100 KB is the smallest input that gets there)."""
import concurrent.futures
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests import cut_model as cm, oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_refs = {}


def _reference(name):
    if name not in _refs:
        level, items, aim, blocks = cm.case(name)
        data = cm.to_bytes(items)
        want = oracle_lib.bz2(data, level)
        if oracle_lib.ref() is not None:
            assert oracle_lib.ref_bz2(data, level) == want, name
        _refs[name] = want
    return _refs[name]


@pytest.fixture(scope="module")
def refs():
    """Every case's libbz2 stream, computed once (the library calls run side by side)."""
    for name in cm.CASES:
        cm.case(name)
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        list(ex.map(_reference, cm.CASES))
    return _refs


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(cm.CASES))
def test_cut_matches_libbz2(ctx, refs, name):
    level, items, aim, blocks = cm.case(name)          # asserts the e_k the case aims at
    if name[0] in "ab":
        assert blocks[aim["k"]].e == aim["e"] in cm.EDGE_E
    got = ctx.bz2_compress(cm.to_bytes(items), level)
    assert got == refs[name]


@pytest.mark.parametrize("level,names", [(1, cm.BATCH_L1), (9, cm.BATCH_L9)], ids=["level1", "level9"])
def test_cut_batch_of_streams(ctx, refs, level, names):
    """Several streams in one launch: slot0[s] is non-zero, the rows of all
    streams share the table, and a stream whose last block reads the table's
    edge stands in the middle.  (A call has one level: the level-9 stream, 3
    blocks with small e, gets a batch of its own.)"""
    import torch
    pieces = []
    for n in names:
        lv, items, aim, blocks = cm.case(n)
        assert lv == level
        pieces.append(cm.to_bytes(items))
    if level == 1:
        mid = cm.case(names[2])
        assert mid[2]["e"] == 125 and mid[2]["d"] == 129 and mid[2]["k"] == len(mid[3]) - 2
        assert len({len(p) for p in pieces}) == 4 and len(pieces[1]) < 4096
    blob = b"".join(pieces)
    offs, lens, o = [], [], 0
    for p in pieces:
        offs.append(o); lens.append(len(p)); o += len(p)
    d_in = torch.frombuffer(bytearray(blob + b"\0" * 64), dtype=torch.uint8).cuda()
    cap = len(blob) + len(blob) // 50 + 4096 * len(pieces)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    oo, ol = ctx.bz2_compress_many_device(d_in.data_ptr(), offs, lens, level, d_out.data_ptr(), cap)
    out = d_out.cpu().numpy().tobytes()
    for n, a, k in zip(names, oo, ol):
        assert out[a:a + k] == refs[n], n


def _child(out_path):
    import starch_amd
    c = starch_amd.Starch(0)
    res = {}
    for name in cm.SEARCH_ONLY:
        level, items, aim, blocks = cm.case(name)
        res[name] = hashlib.sha256(c.bz2_compress(cm.to_bytes(items), level)).hexdigest()
    c.close()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_search_only_walk_matches_libbz2(refs, tmp_path):
    """STARCH_CUT_TAB=0: no table, every block's end searched in the text.
    Both walks must equal libbz2 (stronger than equalling each other)."""
    assert {n[0] for n in cm.SEARCH_ONLY} == {"a", "c", "d"}
    out = str(tmp_path / "search_only.json")
    env = dict(os.environ, STARCH_CUT_TAB="0")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_cut", out], cwd=ROOT, env=env, capture_output=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    got = json.load(open(out))
    assert sorted(got) == sorted(cm.SEARCH_ONLY)
    bad = [n for n in cm.SEARCH_ONLY if got[n] != hashlib.sha256(refs[n]).hexdigest()]
    assert not bad, bad


if __name__ == "__main__":
    _child(sys.argv[1])
