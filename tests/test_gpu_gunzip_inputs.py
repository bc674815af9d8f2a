"""GPU: gzip and BGZF inputs of the BED commands.  Every host entry point that
reads text recognises a gzip input (1f 8b 08) and inflates it in HBM; the same
text given plain, as BGZF and as one generic gzip member must give byte-identical
outputs.  Plain starch3 (Starch.compress) takes its bytes as they are."""
import gzip
import os
import random
import subprocess

import pytest

from tests import align_oracle, corpus
from tests import deflate_writer as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def forms(text):
    """plain, BGZF (several members) and one generic gzip member"""
    return [text, dw.bgzf_file(text, block=3000), gzip.compress(text, 6)]


@pytest.fixture(scope="module")
def beds(ctx):
    lines = corpus.multi_chrom_bed(3, 400, seed=21, kind="bed6").splitlines(keepends=True)
    random.Random(4).shuffle(lines)
    raw = b"".join(lines)
    other = corpus.multi_chrom_bed(3, 300, seed=22, kind="bed6")
    return {"raw": raw, "a": ctx.sort_bed(raw), "b": ctx.sort_bed(other)}


def same(outputs):
    assert all(o == outputs[0] for o in outputs[1:])
    return outputs[0]


def test_sort_bed_sort_check_and_compress_sorted(ctx, beds):
    out = same([ctx.sort_bed(f) for f in forms(beds["raw"])])
    assert out == beds["a"] and out != beds["raw"]
    s = ctx.gunzip_stats()
    assert s["members"] == 1 and not s["is_bgzf"] and s["bytes_out"] == len(beds["raw"])
    assert same([ctx.sort_check(f) for f in forms(beds["raw"])]) != 0
    assert same([ctx.sort_check(f) for f in forms(beds["a"])]) == 0
    same([ctx.compress_sorted(f) for f in forms(beds["raw"])])


def test_bedops_merge_plain_and_bgzf(ctx, beds):
    a, b = forms(beds["a"]), forms(beds["b"])
    want = ctx.bedops("merge", [a[0], b[0]])
    assert want
    assert ctx.bedops("merge", [a[0], b[1]]) == want
    assert ctx.bedops("merge", [a[1], b[2]]) == want
    assert ctx.bedops("merge", [a[2], b[0]]) == want


@pytest.mark.parametrize("tool", ("bedmap", "map_elements", "map_scores", "closest_features"))
def test_two_input_tools(ctx, beds, tool):
    a, b = forms(beds["a"]), forms(beds["b"])
    f = getattr(ctx, tool)
    want = f(a[0], b[0])
    assert want
    for fa, fb in ((0, 1), (0, 2), (1, 0), (2, 0), (1, 2)):
        assert f(a[fa], b[fb]) == want, (fa, fb)


def test_convert_vcf_and_gff(ctx):
    from tests import convert_oracle as oracle
    vcf = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + \
        b"".join(b"chr%d\t%d\t.\tAC\tA,GT,ACG\t9\tq\tDP=%d\n" % (k % 3, 900 - k, k) for k in range(600))
    gff = b"##gff-version 3\n" + b"".join(
        oracle.G.replace(b"11\t20", b"%d\t%d" % (700 - k, 705 - k)) + b"ID=a%d\n" % k for k in range(500))
    for fmt, data in (("vcf", vcf), ("gff", gff)):
        out = same([ctx.convert(f, fmt) for f in forms(data)])
        assert out.count(b"\n") >= 500
        same([ctx.compress_converted(f, fmt) for f in forms(data)])


def test_align2bed_sam(ctx):
    sam = b"@HD\tVN:1.6\n" + b"".join(
        align_oracle.sam_row(b"r%d" % k, 0, b"chr%d" % (k % 2), 5000 - 3 * k, b"10M2D5M") + b"\n" for k in range(400))
    out = same([ctx.align2bed(f, "sam") for f in forms(sam)])
    assert out.count(b"\n") == 400


def _run(cmd, *args):
    return subprocess.run([os.path.join(BUILD, cmd)] + list(args), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


def test_commands_take_gzip_files(ctx, beds, tmp_path):
    bed_gz, vcf_gz, gen_gz = tmp_path / "x.bed.gz", tmp_path / "x.vcf.gz", tmp_path / "x.gz"
    bed_gz.write_bytes(dw.bgzf_file(beds["raw"], block=4000))
    vcf = b"##fileformat=VCFv4.2\n" + b"".join(b"chr1\t%d\t.\tA\tG\t9\tq\tDP=1\n" % (300 - k) for k in range(200))
    vcf_gz.write_bytes(dw.bgzf_file(vcf, block=1000))
    gen_gz.write_bytes(gzip.compress(beds["raw"]))
    r = _run("sort-bed", str(bed_gz))
    assert r.returncode == 0 and r.stdout == beds["a"], r.stderr
    r = _run("convert2bed", "--input=vcf", str(vcf_gz))
    assert r.returncode == 0 and r.stdout == ctx.convert(vcf, "vcf"), r.stderr
    r = _run("starch-zcat", str(bed_gz), str(gen_gz))
    assert r.returncode == 0 and r.stdout == beds["raw"] * 2, r.stderr
    bad = tmp_path / "bad.gz"
    z = bytearray(dw.bgzf_file(beds["raw"], block=4000))
    z[40] ^= 0x55
    bad.write_bytes(bytes(z))
    r = _run("starch-zcat", str(bad))
    assert r.returncode == 22 and r.stdout == b"" and b"gunzip: member 0 at byte 0" in r.stderr, r.stderr


def test_corrupt_bgzf_to_bedops_is_a_data_error(ctx, beds):
    import starch_amd
    z = bytearray(dw.bgzf_file(beds["b"], block=3000))
    _, members = starch_amd.gunzip_plan(bytes(z))
    z[members[2]["in_off"] + 30] ^= 0xFF
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bedops("merge", [beds["a"], bytes(z)])
    assert e.value.code == -12 and "gunzip: member 2 at byte %d" % members[2]["in_off"] in str(e.value)
    assert "line" not in str(e.value)
    assert ctx.bedops("merge", [beds["a"], beds["b"]])


def test_plain_starch3_takes_gzip_bytes_as_text(ctx, beds):
    # starch_encode_host is not a recogniser: its contract is byte identity with the reference on arbitrary
    # bytes.  These bytes begin 1f 8b 08, so every recognising entry point takes them for gzip, and they are
    # BED lines all the same (a chromosome name is any bytes): the archive must be the CPU oracle's, stream
    # for stream, as tests/test_gpu_parity.py and smoke() compare archives.
    import starch_amd
    from tests import oracle_lib
    odd = b"\x1f\x8b\x08"
    data = b"".join(odd + b"\t%d\t%d\tid%d\n" % (10 * k, 10 * k + 7, k) for k in range(300)) + beds["a"]
    assert starch_amd.is_gzip(data)
    _, osegs = oracle_lib.transform(data)
    assert len(osegs) >= 2 and osegs[0][0] == odd and osegs[0][1] == 300
    idx, streams = starch_amd.parse_archive(ctx.compress(data))
    assert len(streams) == len(osegs)
    for st, (chr_, lines, text), meta in zip(streams, osegs, idx["streams"]):
        assert meta["chromosome"].encode("latin-1") == chr_ and meta["uncompressedLineCount"] == lines
        assert st == oracle_lib.bz2(text, 9), chr_
    with pytest.raises(starch_amd.StarchError) as e:      # the same bytes to a recogniser: a data error of the inflater
        ctx.sort_bed(data)
    assert e.value.code == -12 and "gunzip: member 0 at byte 0" in str(e.value)
