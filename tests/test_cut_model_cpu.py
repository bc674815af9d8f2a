"""tests/cut_model.py against libbz2 itself (no GPU, none of this project's
encoder): the model's block boundaries must reproduce the library's combined
CRC.  The input is split at the model's boundaries; each piece, compressed
alone, is one block whose CRC stands in the 4 bytes after the block magic;
folded as the library folds them (bz:compress.c:627-628) they must give the
combined CRC in the footer of the whole input's stream.  A boundary off by a
byte anywhere changes two block CRCs and so the fold.

Python's bz2.compress hands the input over with BZ_RUN and finishes with an
empty BZ_FINISH call (final_joins=False); the reference build's harness,
where present, gives everything to one BZ_FINISH call (final_joins=True)."""
import bz2
import hashlib

import numpy as np
import pytest

from tests import corpus, cut_model as cm, oracle_lib

BLOCK_MAGIC = bytes.fromhex("314159265359")
FOOTER_MAGIC = 0x177245385090


def footer_crc(stream):
    """The combined CRC: the 32 bits after the 48-bit footer magic, which ends
    0..7 padding bits before the stream's last byte ends."""
    v = int.from_bytes(stream[-11:], "big")
    hits = [(v >> s) & 0xFFFFFFFF for s in range(8) if (v >> (s + 32)) & 0xFFFFFFFFFFFF == FOOTER_MAGIC]
    assert len(hits) == 1, hits
    return hits[0]


_piece_crc = {}


def block_crc(piece, level, compress):
    key = (level, compress, hashlib.sha1(piece).digest())
    if key not in _piece_crc:
        s = compress(piece, level)
        assert s[:4] == b"BZh%d" % level and s[4:10] == BLOCK_MAGIC
        crc = int.from_bytes(s[10:14], "big")
        assert footer_crc(s) == crc, "the piece is not a single block"
        _piece_crc[key] = crc
    return _piece_crc[key]


def fold(data, blocks, level, compress):
    """compress: block -> the call that turns its piece into one block"""
    assert blocks[0].beg == 0 and blocks[-1].end == len(data)
    c = 0
    for a, b in zip(blocks, blocks[1:]):
        assert a.end == b.beg
    for b in blocks:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ block_crc(data[b.beg:b.end], level, compress(b))
    return c


def check_against_libbz2(items, level):
    data = cm.to_bytes(items)
    mx = cm.nblock_max(level)
    run = cm.cut(items, level, final_joins=False)
    for k, b in enumerate(run[:-1]):
        assert mx <= b.n <= mx + 4 and b.w == k * mx + b.e
    assert fold(data, run, level, lambda b: bz2.compress) == footer_crc(bz2.compress(data, level))
    if oracle_lib.ref() is not None:
        fin = cm.cut(items, level, final_joins=True)
        # (a block that a final byte joined is one block only under the same one-call finish)
        same = set(run)
        assert fold(data, fin, level, lambda b: bz2.compress if b in same else oracle_lib.ref_bz2) == \
            footer_crc(oracle_lib.ref_bz2(data, level))
    return run


@pytest.mark.parametrize("name", list(cm.CASES))
def test_generated_inputs_cut_where_libbz2_cuts(name):
    level, items, aim, blocks = cm.case(name)          # checks the aimed-at e_k on the model
    check_against_libbz2(items, level)


def test_edge_cases_aim_where_they_say():
    """The targeted table entries, asserted: (a) and (b) look up e = 120..127
    and want offset e + 4 (not recorded from 128 on); (a) sees both values of
    to_end at e >= 124; (c) walks through e = 128, 129, 132, 140; (d) has no
    chunk start at or past the last target."""
    seen = set()
    for name in cm.CASES:
        level, items, aim, blocks = cm.case(name)
        es = cm.e_seq(cm.cut(items, level, final_joins=False))
        if name[0] in "ab":
            assert aim["e"] in cm.EDGE_E and aim["d"] == aim["e"] + 4 == es[aim["k"] + 1]
            assert (aim["d"] >= cm.CUT_E) == (aim["e"] >= 124)
            if name[0] == "a":
                assert aim["k"] == len(es) - 2
                seen.add((aim["e"] >= 124, aim["to_end"]))
            else:
                assert len(es) - 1 - aim["k"] >= 10 and aim["to_end"] is False
        if name[0] == "d" and aim["d"] is None:
            assert aim["k"] == len(es) - 1 and aim["to_end"] is True
    assert {(True, True), (True, False)} <= seen
    past = set(cm.e_seq(cm.case("c_past_4x36_mixed")[3])) | set(cm.e_seq(cm.case("c_past_129")[3]))
    assert {128, 129, 132, 140} <= past
    for name in ("e_all4", "e_all0", "e_cycle", "e_random"):
        assert len(cm.case(name)[3]) == 36
    assert len(cm.case("f_level9_3blocks")[3]) == 4 and max(cm.e_seq(cm.case("f_level9_3blocks")[3])) < 16


def test_parent_rule_wrong_on_the_edge_rows():
    """What the (a) rows are about, shown on the model: the first chunk start
    at or past T0 + e lies at offset 128 or more -- beyond what a row records
    -- while the two scanned tiles reach the stream's end and text follows
    that start.  'Nothing recorded and the tiles reach the end' therefore
    does not mean 'no chunk start left'."""
    n = 0
    for name in cm.CASES:
        level, items, aim, blocks = cm.case(name)
        if name[0] == "a" and aim["e"] >= 124 and aim["to_end"]:
            nxt = cm.cut(items, level, final_joins=False)[aim["k"] + 1]
            assert nxt.e >= cm.CUT_E and nxt.end - nxt.beg >= 1 and nxt.end == blocks[-1].end
            n += 1
    assert n >= 12


@pytest.mark.parametrize("gen", ["exact_max_bs1", "max_plus_one_bs1", "runs_cross_cut_bs1", "multiblock_text_bs1"])
def test_corpus_edge_inputs(gen):
    fn, level = corpus.LARGE_GENERATORS[gen]
    data = fn()
    items = cm.from_bytes(data)
    assert cm.to_bytes(items) == data
    check_against_libbz2(items, level)


@pytest.mark.parametrize("run", [1, 3, 4, 254, 255, 256, 509, 510, 511, 600])
def test_runs_at_a_boundary(run):
    """A run of `run` bytes beginning 0..6 bytes below the first block's
    target, with text or nothing after it (the final single byte included)."""
    mx = cm.nblock_max(1)
    rng = np.random.RandomState(run)
    for below in range(7):
        for after in (0, 1, 50):
            items = [cm.filler(rng, mx - below), (cm.HEAVY, run)] + ([cm.filler(rng, after)] if after else [])
            check_against_libbz2(items, 1)


def test_final_single_byte_joins_only_with_the_finishing_call():
    mx = cm.nblock_max(1)
    items = [cm.filler(np.random.RandomState(5), mx + 1)]
    assert [b.n for b in cm.cut(items, 1, final_joins=False)] == [mx, 1]
    assert [b.n for b in cm.cut(items, 1, final_joins=True)] == [mx + 1]
    check_against_libbz2(items, 1)
    items = [cm.filler(np.random.RandomState(6), mx - 5), (cm.HEAVY, 256)]      # the run's 256th byte
    assert [b.n for b in cm.cut(items, 1, final_joins=False)] == [mx, 1]
    assert [b.n for b in cm.cut(items, 1, final_joins=True)] == [mx + 1]
    check_against_libbz2(items, 1)


def test_offsets_match_a_byte_walk():
    """Offsets.w_at (the tile arithmetic of the to_end checks) against a plain
    per-byte walk of the chunk positions."""
    rng = np.random.RandomState(9)
    items = [cm.filler(rng, 300), (cm.HEAVY, 700), cm.filler(rng, 5), (0x20, 3), (cm.HEAVY, 4), (0x20, 255),
             cm.filler(rng, 9000), (cm.HEAVY, 5000), cm.filler(rng, 10)]
    data = cm.to_bytes(items)
    assert cm.to_bytes(cm.from_bytes(data)) == data
    w, t, walk = 0, 0, []
    for i, c in enumerate(data):
        t = (t + 1) % 255 if i and data[i - 1] == c else 0
        walk.append(w)
        w += 1 if t < 3 else (2 if t == 3 else 0)
    off = cm.Offsets(items)
    assert off.wend == w and off.length == len(data)
    for pos in list(range(0, 1400)) + list(range(0, len(data), 97)) + [len(data) - 1]:
        assert off.w_at(pos) == walk[pos], pos
    assert sum(b.n for b in cm.cut(items, 1)) == w
