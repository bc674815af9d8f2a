"""bigWig / bigBed files read on the host: the writer of tests/bbi_writer.py
against the oracle of tests/bbi_oracle.py on every case of tests/bbi_cases.py,
starch_bbi_info on good and malformed files, the region's choice of blocks, and
the Python interface.  Nothing here opens a GPU."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import pytest

from tests import bbi_cases as cases
from tests import bbi_oracle as oracle
from tests import bbi_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- writer against oracle ----------------------------------------------------------------
def test_oracle_reads_a_hand_written_file():
    sec = W.wig_section(1, [(5, 9, 0.5), (9, 12, 1234567.0)], type_=1)
    data = W.write("bigwig", [(b"chrA", 100), (b"chrB", 200)], [W.Block(sec, W.wig_box(sec))])
    info = oracle.read(data)
    assert info["kind"] == "bigwig" and info["chroms"] == [(b"chrA", 100), (b"chrB", 200)] and info["ubs"] == len(sec)
    assert [b[0] for b in info["blocks"]] == [(1, 5, 1, 12)]
    assert oracle.expected(data) == (b"chrB\t5\t9\tid-1\t0.5\nchrB\t9\t12\tid-2\t1.23457e+06\n", 1)
    assert oracle.expected(data, bedgraph=True)[0] == b"chrB\t5\t9\t0.5\nchrB\t9\t12\t1.23457e+06\n"
    recs = [(0, 0, 0, b""), (0, 0, 4, b"n\t1")]
    data = W.write("bigbed", [(b"c", 9)], [W.Block(W.bed_block(recs), W.bed_box(recs))], ubs=0)
    assert oracle.expected(data) == (b"c\t0\t0\nc\t0\t4\tn\t1\n", 1)


@pytest.mark.parametrize("name", sorted(cases.good()))
def test_writer_and_oracle_agree_on_every_good_case(name):
    kind, data, regions = cases.good()[name]
    info = oracle.read(data)
    assert info["kind"] == kind
    for k, (box, off, size) in enumerate(info["blocks"]):
        p = oracle.payload(data, info, k)
        if info["ubs"]:
            assert len(p) <= info["ubs"] and struct.unpack(">I", data[off + size - 4:off + size])[0] == zlib.adler32(p)
    whole, n = oracle.expected(data)
    assert n == len(info["blocks"]) and whole.count(b"\n") >= 1
    for rg in regions:
        part, nsel = oracle.expected(data, region=rg)
        assert part.count(b"\n") <= whole.count(b"\n") and nsel <= n


def test_cases_reach_what_they_are_for():
    g = cases.good()
    info = oracle.read(g["three_sections"][1])
    recs = [oracle.records(g["three_sections"][1], info, k) for k in range(3)]
    assert sorted(len(r) for r in recs) == [1, 12, 1024]
    fixed = [r for r in recs if len(r) == 12][0]
    assert fixed[0][1] < (1 << 31) <= fixed[-1][1]                       # the fixedStep starts cross 2^31
    for how, btype in (("stored", 0), ("fixed", 1), ("dynamic", 2)):
        data = g["deflate_" + how][1]
        for _, off, size in oracle.read(data)["blocks"]:
            assert (data[off + 2] >> 1) & 3 == btype                     # BTYPE of the first (only) deflate block
    info = oracle.read(g["exact_ubs"][1])
    assert max(len(oracle.payload(g["exact_ubs"][1], info, k)) for k in range(3)) == info["ubs"]
    assert oracle.read(g["uncompressed"][1])["ubs"] == 0
    assert len(oracle.read(g["many_blocks"][1])["blocks"]) == 1100 > 4 * 256
    info = oracle.read(g["sizing_walk"][1])
    assert info["ubs"] == cases.BIG_UBS > 1000 * max(len(oracle.payload(g["sizing_walk"][1], info, k)) for k in range(5))
    assert len(g["sizing_walk"][1]) < 16384
    info = oracle.read(g["adler_sizes"][1])
    assert [len(oracle.payload(g["adler_sizes"][1], info, k)) for k in range(4)] == [5551, 5552, 5553, 13]
    out = oracle.expected(g["g_values"][1])[0]
    for word in (b"\t0\n", b"\t-0\n", b"\t1\n", b"\t0.1\n", b"\t1e-05\n", b"\t123457\n", b"\t1.23457e+06\n", b"\t1.4013e-45\n",
                 b"\t3.40282e+38\n", b"\tinf\n", b"\tnan\n"):
        assert word in out, word
    out = oracle.expected(g["bed_framing"][1])[0]
    assert out.startswith(b"chr1\t0\t0\nchr1\t0\t0\t" + b"r" * 63 + b"\n") and b"\t" + b"v" * 1024 + b"\n" in out
    srt = oracle.sort_bed(oracle.expected(g["bed_ties"][1])[0])
    assert srt != oracle.expected(g["bed_ties"][1])[0]                   # the sort must act
    # both trees of deep_trees are three levels deep
    data = g["deep_trees"][1]
    info = oracle.read(data)
    for root, leaf, inner in ((info["cto"] + 32, 13, 13), (info["fio"] + 48, 32, 24)):
        depth, off = 1, root
        while data[off] == 0:
            off = struct.unpack_from("<Q", data, off + 4 + inner - 8)[0]
            depth += 1
        assert depth >= 3
    assert [n for n, _ in info["chroms"]][:3] == [b"chr1", b"chr10", b"chr2"]
    sel = [oracle.expected(g["regions"][1], region=rg) for rg in g["regions"][2]]
    assert all(n < 6 for _, n in sel) and sel[6] == (b"", 0) and sel[8] == (b"", 0)
    assert sel[2][1] == 1 and sel[3][1] == 2 and sel[4][1] == 2 and sel[5][1] == 1       # inside one block; across a block border


@pytest.mark.parametrize("name", sorted(cases.bad()))
def test_oracle_refuses_every_bad_case(name):
    kind, data = cases.bad()[name]
    with pytest.raises((oracle.Malformed, zlib.error)):
        oracle.expected(data)


# ---- starch_bbi_info ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.good()))
def test_bbi_info_agrees_with_the_oracle(name):
    import starch_amd
    kind, data, regions = cases.good()[name]
    want = oracle.read(data)
    got = starch_amd.bbi_info(data)
    assert (got["kind"], got["version"], got["uncompress_buf_size"], got["chroms"], got["n_blocks"]) == \
           (kind, want["version"], want["ubs"], want["chroms"], len(want["blocks"]))
    assert (got["chrom_tree_offset"], got["full_data_offset"], got["full_index_offset"], got["zoom_levels"]) == \
           (want["cto"], want["fdo"], want["fio"], want["zooms"])
    assert [((b["start_chrom"], b["start_base"], b["end_chrom"], b["end_base"]), b["data_offset"], b["data_size"]) for b in got["blocks"]] == want["blocks"]
    for rg in regions:
        assert [b["index"] for b in starch_amd.bbi_info(data, region=rg)["blocks"]] == oracle.selected(want, rg), rg


@pytest.mark.parametrize("name", sorted(cases.malformed()))
def test_bbi_info_refuses_malformed_files_with_a_reason(name):
    import starch_amd
    data, word = cases.malformed()[name]
    with pytest.raises(oracle.Malformed):
        oracle.read(data)
    with pytest.raises(starch_amd.StarchError) as e:
        starch_amd.bbi_info(data)
    assert e.value.code == -12 and "bbi: " in str(e.value) and word in str(e.value), str(e.value)


def test_a_chain_of_overlapping_nodes_costs_no_more_than_the_file(tmp_path):
    """The walk's memory is bounded by the file's bytes: 12,000 inner nodes that each claim the rest of the
    file are refused at the second one, not after a stack of millions of child offsets has grown (about
    1 GiB for this file).  Peak memory is a property of a process, so a fresh one measures it: its peak
    after a good file is read, and again after the chain is refused."""
    data = cases.node_chain()
    assert len(data) == 336144
    (tmp_path / "chain.bw").write_bytes(data)
    (tmp_path / "good.bw").write_bytes(cases.good()["deep_trees"][1])
    script = ("import resource, sys, starch_amd\n"
              "peak = lambda: resource.getrusage(resource.RUSAGE_SELF).ru_maxrss\n"
              "starch_amd.bbi_info(open(sys.argv[1], 'rb').read())\n"
              "before = peak()\n"
              "try:\n"
              "    starch_amd.bbi_info(open(sys.argv[2], 'rb').read())\n"
              "except starch_amd.StarchError as e:\n"
              "    print(e.code, peak() - before, e)\n")
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "good.bw"), str(tmp_path / "chain.bw")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    code, grown_kib, reason = r.stdout.decode().split(" ", 2)
    assert int(code) == -12 and "the R-tree: its nodes overlap" in reason
    assert int(grown_kib) < 16 * 1024, grown_kib          # the file has a third of a MiB


def test_bbi_info_on_short_and_empty_inputs_and_a_forced_kind():
    import starch_amd
    data = cases.good()["three_sections"][1]
    for cut in (0, 1, 3, 4, 63, 64, 65, 100, len(data) // 2, len(data) - 1):
        with pytest.raises(starch_amd.StarchError) as e:
            starch_amd.bbi_info(data[:cut])
        assert e.value.code == -12, cut
    L = starch_amd.load()
    h, err = starch_amd.BbiHeader(), ctypes.create_string_buffer(256)
    o = starch_amd.BbiQuery(kind=2)
    assert L.starch_bbi_info(data, len(data), ctypes.byref(o), ctypes.byref(h), None, 0, None, 0, None, None, 0, err, 256) == -12
    assert b"not the kind that was asked for" in err.value
    o = starch_amd.BbiQuery(kind=1)
    assert L.starch_bbi_info(data, len(data), ctypes.byref(o), ctypes.byref(h), None, 0, None, 0, None, None, 0, err, 256) == 0
    assert h.n_blocks == 3 and h.n_chroms == 5
    sizes = (ctypes.c_uint32 * 2)()
    assert L.starch_bbi_info(data, len(data), None, ctypes.byref(h), sizes, 2, None, 0, None, None, 0, None, 0) == -3   # a short buffer


# ---- the library and the Python interface ---------------------------------------------------
def test_symbol_declarations_and_header():
    import starch_amd
    L = starch_amd.load()
    f = L.starch_bbi_info
    assert f.restype is ctypes.c_int and len(f.argtypes) == 13
    assert ctypes.sizeof(starch_amd.BbiQuery) == 40 and starch_amd.BbiQuery.chrom.offset == 8
    assert ctypes.sizeof(starch_amd.BbiHeader) == 24 + 7 * 8 and ctypes.sizeof(starch_amd.BbiBlock) == 32
    for name in ("bbi_info", "BBI_KINDS", "BbiQuery", "BbiHeader", "BbiBlock"):
        assert name in starch_amd.__all__
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    for word in ("unverified against UCSC's tools", "big-endian bigWig/bigBed is not supported", "0x78CA8C91", "0x2468ACE0",
                 "a node\n * reached twice is an error"):
        assert word in header, word


def test_bad_arguments():
    import starch_amd
    L = starch_amd.load()
    data = cases.good()["three_sections"][1]
    h = starch_amd.BbiHeader()
    assert L.starch_bbi_info(data, len(data), None, None, None, 0, None, 0, None, None, 0, None, 0) == -2       # no header to fill
    assert L.starch_bbi_info(None, 5, None, ctypes.byref(h), None, 0, None, 0, None, None, 0, None, 0) == -2    # bytes announced, none given
    for q in (starch_amd.BbiQuery(kind=3), starch_amd.BbiQuery(region=1), starch_amd.BbiQuery(region=3, chrom=b"c", chrom_len=1),
              starch_amd.BbiQuery(region=2, chrom=b"c", chrom_len=1, start=5, end=5)):
        assert L.starch_bbi_info(data, len(data), ctypes.byref(q), ctypes.byref(h), None, 0, None, 0, None, None, 0, None, 0) == -2
