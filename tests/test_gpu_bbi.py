"""GPU: bigwig2bed and bigbed2bed (Starch.bbi2bed, bbi2bed_device, compress_bbi, the
two commands).

Every comparison is equality of whole outputs against tests/bbi_oracle.py on the
files of tests/bbi_cases.py: unsorted output is the oracle's lines in block
order (bigWig as chrom, start, end, value), sorted output the same lines in
sort-bed's order.  The uncompressed cases come first: they run the record
kernels without the zlib stage."""
import os
import subprocess

import pytest

from tests import bbi_cases as cases
from tests import bbi_expect as expect
from tests import bbi_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
GOOD = sorted(cases.good(), key=lambda n: ("uncompressed" not in n, n))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", GOOD)
def test_good_files_give_the_oracles_lines(ctx, name):
    kind, data, regions = cases.good()[name]
    for rg in regions:
        want = expect.expected_text(data, rg)
        assert ctx.bbi2bed(data, region=rg, sort=False) == want, rg
        st = ctx.bbi_stats()
        assert st["lines_out"] == want.count(b"\n") and st["blocks"] == len(oracle.selected(oracle.read(data), rg)) and not st["sorted"]
        assert st["kind"] == (1 if kind == "bigwig" else 2) and st["compressed"] == (oracle.read(data)["ubs"] != 0)
        assert ctx.bbi2bed(data, region=rg) == oracle.sort_bed(want), rg
        assert ctx.bbi2bed(data, region=rg, kind=kind) == oracle.sort_bed(want), rg


def test_orders_of_ties_and_of_chromosome_names(ctx):
    data = cases.good()["bed_ties"][1]
    got = ctx.bbi2bed(data).split(b"\n")[:-1]
    keys = [(l.split(b"\t")[0], int(l.split(b"\t")[1]), int(l.split(b"\t")[2])) for l in got]
    assert keys == sorted(keys) and len(got) == 342
    assert got[0] == b"chr1\t100\t151\tm299" and got[-1] == b"chr2\t5\t6\tx"
    data = cases.good()["deep_trees"][1]                                       # chr1 < chr10 < chr2 as bytes, ids 0, 1, 2
    names = [l.split(b"\t")[0] for l in ctx.bbi2bed(data).split(b"\n")[:-1]]
    assert names == sorted(names) and names.index(b"chr10") < names.index(b"chr2")
    assert ctx.bbi_stats()["sorted"] == 1


def test_region_edges(ctx):
    data = cases.good()["regions"][1]
    for rg, lines in (((b"chr1", 799, 801), 2), ((b"chr2", 95, 96), 1), (b"chr9", 0), ((b"chr1", 5000, 6000), 0), (b"chr3", 0)):
        want = expect.expected_text(data, rg)
        assert want.count(b"\n") == lines
        assert ctx.bbi2bed(data, region=rg, sort=False) == want, rg
        assert ctx.bbi2bed(data, region=rg) == oracle.sort_bed(want), rg
    st_all = ctx.bbi2bed(data, sort=False) and ctx.bbi_stats()
    ctx.bbi2bed(data, region=(b"chr1", 450, 700), sort=False)
    st = ctx.bbi_stats()
    assert st["blocks"] == 1 and st["uploaded_bytes"] < st_all["uploaded_bytes"] and st["records"] == 10 and st["lines_out"] == 7


def test_wave_records_and_the_sizing_walk_are_counted(ctx):
    ctx.bbi2bed(cases.good()["bed_framing"][1], sort=False)
    assert ctx.bbi_stats()["wave_records"] == 2                                # rests of 1024 and 3000 bytes
    ctx.bbi2bed(cases.good()["sizing_walk"][1], sort=False)
    assert ctx.bbi_stats()["sized"] == 1
    ctx.bbi2bed(cases.good()["exact_ubs"][1], sort=False)
    assert ctx.bbi_stats()["sized"] == 0


def test_compress_bbi_and_the_device_entry(ctx):
    import torch
    for name in ("three_sections", "bed_ties"):
        data = cases.good()[name][1]
        want = oracle.sort_bed(expect.expected_text(data))
        arch = ctx.compress_bbi(data)
        assert ctx.unstarch(arch) == want
        assert arch == ctx.compress(want)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        assert ctx.bbi2bed_device(t.data_ptr(), len(data)) == len(want)
        assert ctx._output() == want
    data = cases.good()["regions"][1]
    assert ctx.unstarch(ctx.compress_bbi(data, region=b"chr2")) == oracle.sort_bed(expect.expected_text(data, b"chr2"))


@pytest.mark.parametrize("name", sorted(cases.bad()))
def test_bad_blocks_are_refused_and_nothing_is_written(ctx, name):
    import starch_amd
    kind, data = cases.bad()[name]
    block = dict(expect.RECORD_BAD, **expect.ZLIB_BAD)[name]
    tool = "bigwig2bed" if kind == "bigwig" else "bigbed2bed"
    for sort in (False, True):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.bbi2bed(data, sort=sort)
        assert e.value.code == -12 and "%s: block %d: " % (tool, block) in str(e.value), str(e.value)
        with pytest.raises(starch_amd.StarchError) as e:                      # no output is left behind
            ctx._output()
        assert e.value.code == -4
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.compress_bbi(data)
    assert e.value.code == -12
    good = cases.good()["g_values"][1]                                         # the context serves a good call afterwards
    assert ctx.bbi2bed(good, sort=False) == expect.expected_text(good)


def test_a_file_of_the_other_kind_and_bad_arguments(ctx):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bbi2bed(cases.good()["bed_ties"][1], kind="bigwig")
    assert e.value.code == -12 and "bbi: the file is a bigBed" in str(e.value)
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bbi2bed(cases.malformed()["bad_magic"][0])
    assert e.value.code == -12 and "bad magic" in str(e.value)
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bbi2bed(cases.good()["regions"][1], region=(b"chr1", 5, 5))
    assert e.value.code == -2


# ---- the commands -----------------------------------------------------------------------------
def _cli(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_commands(ctx, tmp_path):
    wig, bed = cases.good()["regions"][1], cases.good()["bed_ties"][1]
    (tmp_path / "a.bw").write_bytes(wig)
    (tmp_path / "a.bb").write_bytes(bed)
    bw, bb = os.path.join(BUILD, "bigwig2bed"), os.path.join(BUILD, "bigbed2bed")
    r = _cli([bw, "--do-not-sort", "--region", "chr1:450-700", str(tmp_path / "a.bw")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == expect.expected_text(wig, (b"chr1", 450, 700))
    r = _cli([bb, str(tmp_path / "a.bb")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == oracle.sort_bed(expect.expected_text(bed))
    r = _cli([bb, "--output=starch", "--region", "chr2", str(tmp_path / "a.bb")])
    assert (r.returncode, r.stderr) == (0, b"") and ctx.unstarch(r.stdout) == oracle.sort_bed(expect.expected_text(bed, b"chr2"))
    # the other kind of file, stdin and a bad region: exit status 2 before a GPU is opened (none is visible to the child)
    blind = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args in ([bw, str(tmp_path / "a.bb")], [bb, str(tmp_path / "a.bw")], [bw, "-"], [bw], [bw, "--region", "chr1:9-3", str(tmp_path / "a.bw")]):
        r = _cli(args, env=blind, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    (tmp_path / "bad.bb").write_bytes(cases.bad()["bed_newline"][1])
    r = _cli([bb, str(tmp_path / "bad.bb")])
    assert r.returncode == 22 and r.stdout == b"" and b"bigbed2bed: block 1: " in r.stderr
