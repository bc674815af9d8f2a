"""CPU: the starchcat planner (starch_cat_plan, starch_amd.cat_plan), the
copy-only cat that needs no GPU (starch_amd.cat_host) and the starchcat
command's --plan and copy-only forms.  Nothing here opens a GPU context.

Archives are put together without a GPU, as in tests/test_extract_index.py:
segment texts from the oracle's transform, bzip2 streams from the oracle's
compressor, the index from starch_amd.build_index.  The expected result of a
copy-only cat is assembled the same way from the same oracle streams.
"""
import os
import subprocess

import pytest

import starch_amd
from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STARCHCAT = os.path.join(ROOT, "starch_amd", "_build", "starchcat")
HIGH = b"chr\xe9"                     # a byte >= 0x80: after every ASCII name by memcmp


def _chrom_bed(name, n, seed):
    out, pos = [], seed
    for i in range(n):
        pos += 1 + (i * 7 + seed) % 90
        out.append(name + b"\t%d\t%d\tid%d\n" % (pos, pos + 1 + (i % 5) * 10, i))
    return b"".join(out)


def _pieces(chroms, level=9, seed=3):
    """[(name, line count, text, bzip2 stream)] for one stream per listed chromosome (repeats allowed)."""
    out = []
    for k, name in enumerate(chroms):
        _, osegs = oracle_lib.transform(_chrom_bed(name, 40 + 5 * k, seed + k))
        assert len(osegs) == 1 and osegs[0][0] == name
        _, lines, text = osegs[0]
        out.append((name, lines, text, oracle_lib.bz2(text, level)))
    return out


def _assemble(pieces, note=None, level=9, base_counts=False, tag=0):
    """An archive of the pieces in the given order; CRC / blocks / base counts are tags the index carries."""
    segs, off = [], 4
    for k, (name, lines, text, st) in enumerate(pieces):
        h = sum(name) * 131 + len(text) + tag
        segs.append(starch_amd.Segment(lines, len(text), off, len(st), len(name), 1, 0x9E3779B9 ^ h, 0,
                                       1000 + h, 2000 + h))
        off += len(st)
    blob = starch_amd.MAGIC + b"".join(p[3] for p in pieces)
    return blob + starch_amd.build_index(segs, [p[0] for p in pieces], off, note=note, level=level,
                                         base_counts=base_counts)


def _three():
    return [_assemble(_pieces([b"chr1", b"chr3"], seed=1)),
            _assemble(_pieces([b"chr10", b"chr2"], seed=11)),
            _assemble(_pieces([b"chr3", b"chrX", b"chr3"], seed=21))]


def test_plan_groups_runs_and_order():
    plan = starch_amd.cat_plan(_three())
    assert [p[0] for p in plan] == [b"chr1", b"chr10", b"chr2", b"chr3", b"chrX"]
    assert plan[3] == (b"chr3", "merge", [(0, 1), (2, 0), (2, 2)])
    assert plan[0] == (b"chr1", "copy", [(0, 0)])
    assert plan[1] == (b"chr10", "copy", [(1, 0)])
    assert plan[2] == (b"chr2", "copy", [(1, 1)])
    assert plan[4] == (b"chrX", "copy", [(2, 1)])


def test_plan_orders_names_by_memcmp():
    names = [HIGH, b"chr10", b"chrX", b"chr1", b"chr", b"chr1\x7f", b"chr1\x80"]
    plan = starch_amd.cat_plan([_assemble(_pieces(names))])
    got = [p[0] for p in plan]
    assert got == sorted(names) == [b"chr", b"chr1", b"chr10", b"chr1\x7f", b"chr1\x80", b"chrX", HIGH]
    assert all(p[1] == "copy" for p in plan)
    # the same names spread over inputs, in another order
    plan2 = starch_amd.cat_plan([_assemble(_pieces(names[:3])), _assemble(_pieces(names[3:]))])
    assert [p[0] for p in plan2] == got


def test_plan_level_and_base_counts_turn_copies_into_merges():
    a9 = _assemble(_pieces([b"chr1", b"chr2"]))
    a5 = _assemble(_pieces([b"chr3", b"chr4"], level=5), level=5)
    plan = starch_amd.cat_plan([a9, a5], level=9)
    assert [(p[0], p[1]) for p in plan] == [(b"chr1", "copy"), (b"chr2", "copy"), (b"chr3", "merge"), (b"chr4", "merge")]
    plan = starch_amd.cat_plan([a9, a5], level=5)
    assert [(p[0], p[1]) for p in plan] == [(b"chr1", "merge"), (b"chr2", "merge"), (b"chr3", "copy"), (b"chr4", "copy")]
    with_counts = _assemble(_pieces([b"chr5"]), base_counts=True)
    plan = starch_amd.cat_plan([a9, with_counts], base_counts=True)
    assert [(p[0], p[1]) for p in plan] == [(b"chr1", "merge"), (b"chr2", "merge"), (b"chr5", "copy")]
    plan = starch_amd.cat_plan([a9, with_counts], base_counts=False)
    assert all(p[1] == "copy" for p in plan)


@pytest.mark.parametrize("base_counts_in,base_counts_out", [(False, False), (True, False), (True, True)])
def test_copy_only_cat_without_a_gpu(base_counts_in, base_counts_out):
    note = "café \"cat 7\"\ttab €"
    pa = _pieces([b"chrX", b"chr1", HIGH], seed=2)          # not in sorted order inside the input
    pb = _pieces([b"chr2", b"chr10"], seed=12)
    a = _assemble(pa, note="first", base_counts=base_counts_in, tag=1)
    b = _assemble(pb, note=None, base_counts=base_counts_in, tag=2)
    got = starch_amd.cat_host([a, b], note=note, level=9, base_counts=base_counts_out)
    # the same oracle streams in group order, each with the tag of its own input
    order = sorted(pa + pb, key=lambda p: p[0])
    assert [p[0] for p in order] == [b"chr1", b"chr10", b"chr2", b"chrX", HIGH]
    segs, off = [], 4
    for p in order:
        h = sum(p[0]) * 131 + len(p[2]) + (1 if p in pa else 2)
        segs.append(starch_amd.Segment(p[1], len(p[2]), off, len(p[3]), len(p[0]), 1, 0x9E3779B9 ^ h, 0, 1000 + h, 2000 + h))
        off += len(p[3])
    want = starch_amd.MAGIC + b"".join(p[3] for p in order) + starch_amd.build_index(
        segs, [p[0] for p in order], off, note=note, level=9, base_counts=base_counts_out)
    assert got == want
    info, entries = starch_amd.list_archive(got)
    assert info["note"] == note and [e["chromosome"] for e in entries] == [p[0] for p in order]
    assert all(("uniqueBaseCount" in e) == base_counts_out for e in entries)
    # one input alone: a normalised copy
    assert starch_amd.cat_host([a], note="first", base_counts=base_counts_in) == _assemble(
        sorted(pa, key=lambda p: p[0]), note="first", base_counts=base_counts_in, tag=1)


def test_merge_group_needs_a_context():
    with pytest.raises(starch_amd.StarchError) as e:
        starch_amd.cat_host(_three())
    assert e.value.code == -2
    a9 = _assemble(_pieces([b"chr1"]))
    with pytest.raises(starch_amd.StarchError) as e:
        starch_amd.cat_host([a9], level=5)
    assert e.value.code == -2
    with pytest.raises(starch_amd.StarchError) as e:
        starch_amd.cat_host([a9], base_counts=True)
    assert e.value.code == -2


def test_errors():
    good = _assemble(_pieces([b"chr1", b"chr2"]))
    for call in (starch_amd.cat_plan, starch_amd.cat_host):
        with pytest.raises(starch_amd.StarchError) as e:
            call([])
        assert e.value.code == -2, "zero archives"
        gz = good.replace(b'"compressionFormat":"bzip2"', b'"compressionFormat":"gzip"')   # (the index starts where it did)
        assert len(gz) == len(good) - 1 and starch_amd.list_archive(gz)[0]["compressionFormat"] == "gzip"
        with pytest.raises(starch_amd.StarchError) as e:
            call([good, gz])
        assert e.value.code == -2, "gzip index"
        with pytest.raises(starch_amd.StarchError) as e:
            call([good, good[:-1]])
        assert e.value.code == -12, "truncated footer"
        with pytest.raises(starch_amd.StarchError) as e:
            call([good[:20]])
        assert e.value.code == -12, "too short"
        # a stream reaching past the index offset
        p = _pieces([b"chr7"])
        seg = starch_amd.Segment(p[0][1], len(p[0][2]), 4, len(p[0][3]) + 1, 4, 1, 0, 0, 0, 0)
        past = starch_amd.MAGIC + p[0][3] + starch_amd.build_index([seg], [b"chr7"], 4 + len(p[0][3]))
        with pytest.raises(starch_amd.StarchError) as e:
            call([past, good])
        assert e.value.code == -12, "stream past the index offset"


def test_plan_sizing_and_short_capacity():
    import ctypes
    L = starch_amd.load()
    arch = _three()
    ptrs = (ctypes.c_char_p * 3)(*arch)
    lens = (ctypes.c_uint64 * 3)(*[len(a) for a in arch])
    ng, nr, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    assert L.starch_cat_plan(ptrs, lens, 3, None, None, 0, ctypes.byref(ng), None, 0, ctypes.byref(nr), None, 0,
                             ctypes.byref(nb)) == 0
    assert (ng.value, nr.value, nb.value) == (5, 7, len(b"chr1chr10chr2chr3chrX"))
    groups = (starch_amd.CatGroup * 5)()
    runs = (starch_amd.CatRun * 7)()
    assert L.starch_cat_plan(ptrs, lens, 3, None, groups, 4, ctypes.byref(ng), runs, 7, ctypes.byref(nr), None, 0,
                             ctypes.byref(nb)) == -3
    assert L.starch_cat_plan(ptrs, lens, 3, None, groups, 5, ctypes.byref(ng), runs, 7, ctypes.byref(nr), None, 0,
                             ctypes.byref(nb)) == 0
    assert [g.n_runs for g in groups] == [1, 1, 1, 3, 1] and groups[3].first_run == 3 and groups[3].merge == 1
    idx = [starch_amd.list_archive(a)[1] for a in arch]
    assert groups[3].lines == sum(idx[i][e]["uncompressedLineCount"] for i, e in [(0, 1), (2, 0), (2, 2)])
    assert groups[3].text_bytes == sum(idx[i][e]["transformedBytes"] for i, e in [(0, 1), (2, 0), (2, 2)])
    o = starch_amd.Options()
    L.starch_options_init(ctypes.byref(o))
    for field, bad in (("emit_index", 0), ("reference_compat", 1), ("compression_method", 1), ("block_size_100k", 0)):
        L.starch_options_init(ctypes.byref(o))
        setattr(o, field, bad)
        assert L.starch_cat_plan(ptrs, lens, 3, ctypes.byref(o), None, 0, ctypes.byref(ng), None, 0, ctypes.byref(nr),
                                 None, 0, ctypes.byref(nb)) == -2, field


def _run(args, **kw):
    return subprocess.run([STARCHCAT] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, **kw)


def test_starchcat_plan_and_copy_only(tmp_path):
    arch = _three()
    paths = []
    for k, a in enumerate(arch):
        paths.append(str(tmp_path / ("in%d.starch" % k)))
        with open(paths[-1], "wb") as f:
            f.write(a)
    r = _run(["--plan"] + paths)
    assert r.returncode == 0, r.stderr
    assert r.stdout == (b"chr1\tcopy\t0:0\nchr10\tcopy\t1:0\nchr2\tcopy\t1:1\nchr3\tmerge\t0:1,2:0,2:2\n"
                        b"chrX\tcopy\t2:1\n")
    # copy-only: the first two inputs share no chromosome
    r = _run(["--note", "two inputs", paths[0], paths[1]])
    assert r.returncode == 0, r.stderr
    assert r.stdout == starch_amd.cat_host(arch[:2], note="two inputs")
    r = _run(["--bzip2-level", "9", "--note", "two inputs", paths[1], paths[0]])
    assert r.returncode == 0 and r.stdout == starch_amd.cat_host(arch[1::-1], note="two inputs")
    r = _run([paths[0], str(tmp_path / "missing.starch")])
    assert r.returncode != 0 and r.stdout == b""
    r = _run(["--level", "10", paths[0]])
    assert r.returncode != 0 and r.stdout == b""
