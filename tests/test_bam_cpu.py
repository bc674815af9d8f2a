"""CPU-side checks of bam2bed: the oracle of tests/bam_oracle.py against its
hand-written table, and the parts of the command, the library and the Python
interface that open no GPU."""
import ctypes
import os
import random
import re
import struct
import subprocess
import zlib

import pytest

from tests import align_oracle
from tests import bam_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help", "bam2bed.txt")


def _run(cmd, *args, **kw):
    return subprocess.run([os.path.join(ROOT, "starch_amd", "_build", cmd)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


# ---- the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracle_gives_the_hand_written_sam_lines(case):
    rec, want = oracle.TABLE[case]
    data = oracle.bam(b"", oracle.REFS, [rec])
    assert oracle.sam_text(data) == want + b"\n"


def test_table_reaches_every_tag_type_and_special_column():
    lines = b"\n".join(want for _, want in oracle.TABLE)
    types = {t[1] for rec, _ in oracle.TABLE for t in rec.get("tags", [])}
    assert types == set("AcCsSiIfZHB")
    assert {t[2][0] for rec, _ in oracle.TABLE for t in rec.get("tags", []) if t[1] == "B"} == set("cCsSiIf")
    for word in (b"\t=\t", b"\t-2147483648\t", b"\t-5\t", b"2M10N2M", b"CG:B:I,32", b":f:0\t", b":f:-0\t", b":f:1e-05", b":f:123456\t",
                 b":f:1e+06", b":f:1.4013e-45", b":f:inf", b":f:-inf", b":f:nan", b"\tNAN\t*", b"\t*\t*"):
        assert word in lines, word
    for op in oracle.OPS:
        assert bytes([op]) in oracle.TABLE[4][1].split(b"\t")[5]


def test_header_text_lines_and_the_whole_table_through_sam2bed_rules():
    recs = [rec for rec, _ in oracle.TABLE]
    for text, head in ((b"", b""), (b"@HD\tVN:1.6\n@CO\tx\n", b"@HD\tVN:1.6\n@CO\tx\n"), (b"@HD\tVN:1.6\n@CO\tx", b"@HD\tVN:1.6\n@CO\tx\n"),
                       (b"@CO\ta\n\0\0\0", b"@CO\ta\n"), (b"\n@CO\ta", b"\n@CO\ta\n")):
        data = oracle.bam(text, oracle.REFS, recs)
        assert oracle.sam_text(data) == head + b"".join(want + b"\n" for _, want in oracle.TABLE)
        kept = oracle.expected(data, keep_header=True)
        assert kept.count(b"_header\t") == head.count(b"\n")
    plain = oracle.expected(data)
    assert plain.count(b"\n") == len(recs) - 1 and b"chr1\t6\t22\tr001\t99\t+\t30\t8M2I4M1D3M\t=\t37\t39\t" in plain
    assert b"_unmapped\t0\t1\tun\t4\t+\t0\t*\t" in oracle.expected(data, all_reads=True)
    assert b"chr1\t10\t12\tlong\t0\t+\nchr1\t22\t24\tlong\t0\t+\n" in oracle.expected(data, split=True, reduced=True)
    assert oracle.record_offsets(data)[0] == len(oracle.header(text, oracle.REFS))


def test_random_bam_is_well_formed_and_bgzf_round_trips():
    rng = random.Random(20261021)
    data, recs = oracle.random_bam(rng, 200)
    assert len(oracle.record_offsets(data)) == 200
    text = oracle.sam_text(data)
    assert text.count(b"\n") == 200 + oracle.TEXT.count(b"\n")
    assert oracle.expected(data, all_reads=True).count(b"\n") == 200
    assert 0 < oracle.expected(data).count(b"\n") < 200
    offs = oracle.record_offsets(data)
    for kw in (dict(), dict(cuts=offs), dict(cuts=[o + 2 for o in offs]), dict(level=0), dict(eof=False)):
        z = oracle.bgzf(data, **kw)
        out, p, members = b"", 0, 0
        while p < len(z):
            assert z[p:p + 4] == b"\x1f\x8b\x08\x04" and z[p + 12:p + 16] == b"BC\x02\0"
            size = struct.unpack_from("<H", z, p + 16)[0] + 1
            piece = zlib.decompress(z[p + 18:p + size - 8], -15)
            assert struct.unpack_from("<II", z, p + size - 8) == (zlib.crc32(piece), len(piece))
            out, p, members = out + piece, p + size, members + 1
        assert out == data
        if "cuts" in kw:
            assert members >= 200
    assert zlib.decompress(oracle.gzip_member(data), 31) == data


# ---- the command ----------------------------------------------------------------------------
def test_help_is_the_golden_and_opens_no_gpu():
    r = _run("bam2bed", "--help")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == open(GOLDEN, "rb").read()
    for word in (b"USAGE: bam2bed [--output=bed|starch] [--do-not-sort] [--keep-header] [--split] [--split-with-deletions]",
                 b"--all-reads", b"--reduced", b"--device N", b"Not supported: --max-mem, --sort-tmpdir, --zero-indexed, --do-not-split.",
                 b"unverified against samtools\n  or BEDOPS (*)", b"C's %g of the float32", b"inf, -inf\n    and nan", b"CG:B:I",
                 b"samtools view -h"):
        assert word in r.stdout, word
    r = _run("bam2bed", "--version")
    assert r.returncode == 0 and r.stdout.startswith(b"bam2bed\n  version: ") and r.stderr == b""


def test_usage_errors_and_unsupported_options():
    missing = os.path.join(ROOT, "no", "such", "file.bam")
    for args in (["--max-mem=2G", missing], ["--max-mem", "2G", missing], ["--sort-tmpdir=/tmp", missing], ["--zero-indexed", missing],
                 ["--do-not-split", missing], ["--frobnicate", missing], ["-x", missing], ["--input=bam", missing], ["--output=bam", missing],
                 ["--output"], ["--output=starch", "--do-not-sort", missing], [missing, missing]):
        r = _run("bam2bed", *args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: bam2bed" in r.stderr, args


def test_missing_input_and_missing_gpu():
    missing = os.path.join(ROOT, "no", "such", "file.bam")
    for args in ([missing], ["--split-with-deletions", "--all-reads", "--reduced", "--keep-header", "--do-not-sort", missing],
                 ["--output=STARCH", "--device", "0", missing]):
        r = _run("bam2bed", *args, stdin=subprocess.DEVNULL)
        assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b"", args
    for args in (["-"], ["--output=starch"], ["--split", GOLDEN]):
        r = _run("bam2bed", *args, stdin=subprocess.DEVNULL)
        assert r.returncode == 22 and r.stdout == b"", args
        assert r.stderr == b"Error: no GPU context (HIP device error)\n", args


def test_convert2bed_still_refuses_bam_and_the_old_surface_is_unchanged():
    import starch_amd
    r = _run("convert2bed", "--input=bam", GOLDEN, stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"Error: ")
    assert starch_amd.ALIGN_FORMATS == {"sam": 0, "psl": 1, "rmsk": 2}
    with pytest.raises(ValueError):
        starch_amd._align_options("bam", False, False, False, False, False, True)
    L = starch_amd.load()
    opt = starch_amd.AlignOptions(format=3)
    assert L.starch_align_host(ctypes.c_void_p(1), b"", 0, ctypes.byref(opt)) == -2


# ---- the library and the Python interface ---------------------------------------------------
def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_bam_host", "starch_bam_device", "starch_bam_encode_host", "starch_bam_get_stats", "starch_bam_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    O = starch_amd.BamOptions           # six u32
    assert ctypes.sizeof(O) == 24
    assert [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 8, 12, 16, 20]
    S = starch_amd.BamStats             # eleven u64, six floats
    assert ctypes.sizeof(S) == 112
    assert S.sorted.offset == 80 and S.ms_inflate.offset == 88 and S.ms_total.offset == 108
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    section = header[header.index("bam2bed: BAM records to BED, read through BGZF"):]
    assert header.index("sam2bed, psl2bed, rmsk2bed: SAM, PSL and RepeatMasker .out to BED") < len(header) - len(section)
    for word in ("unverified against samtools or BEDOPS are marked (*)", "(*) infinities and NaNs", "no\n * floating-point instruction",
                 "bam2bed: record N: <what is wrong>", "[t * T, (t + 1) * T) of the inflated file"):
        assert word in section, word
    body = re.search(r"typedef struct \{([^}]*)\} starch_bam_stats;", header).group(1)
    fields = re.findall(r"\b(?:input_|inflated_|references|header_|records|unmapped_|tiles|wave_|lines_|output_|sorted|ms_)\w*",
                        re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in S._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_bam_options;", header).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in O._fields_]
    for m in ("bam2bed", "bam2bed_device", "compress_bam", "bam_stats"):
        assert callable(getattr(starch_amd.Starch, m))
    for name in ("bam_constants", "BamOptions", "BamStats"):
        assert name in starch_amd.__all__


def test_constants():
    import starch_amd
    T, block, W = starch_amd.bam_constants()
    assert T == 16384 and 3 * T <= 48 * 1024            # the LDS budget of the framing: 16 bits per byte beside the tile
    assert block >= 64 and block % 64 == 0 and block == starch_amd.align_constants()[0]
    assert 64 <= W <= 65536 and W % 64 == 0
    for text in oracle.E_SHORT, oracle.E_PAST, oracle.E_COUNTS, oracle.E_NAME, oracle.E_REF, oracle.E_CIGAR, oracle.E_TAGTYPE, oracle.E_TAGS:
        assert ('"%s"' % text) in open(os.path.join(ROOT, "starch_amd", "csrc", "bed_bam.hip")).read()


def test_bad_arguments_are_refused_before_a_device_is_touched():
    import starch_amd
    L = starch_amd.load()
    opt = starch_amd.BamOptions()
    assert L.starch_bam_host(None, b"", 0, ctypes.byref(opt)) == -2            # a NULL context
    assert L.starch_bam_device(None, None, 0, ctypes.byref(opt)) == -2
    assert L.starch_bam_encode_host(None, b"", 0, ctypes.byref(opt), None) == -2
    assert L.starch_bam_get_stats(None, None) == -2
    fake = ctypes.c_void_p(1)            # never dereferenced: the options are refused first
    assert L.starch_bam_host(fake, b"", 0, None) == -2
    assert L.starch_bam_device(fake, None, 0, None) == -2
    assert L.starch_bam_encode_host(fake, b"", 0, None, None) == -2
    for kw in (dict(split_deletions=1), dict(split_deletions=1, all_reads=1, reduced=1, keep_header=1)):
        opt = starch_amd.BamOptions(**kw)
        assert L.starch_bam_host(fake, b"", 0, ctypes.byref(opt)) == -2, kw
        assert L.starch_bam_device(fake, None, 0, ctypes.byref(opt)) == -2, kw
        assert L.starch_bam_encode_host(fake, b"", 0, ctypes.byref(opt), None) == -2, kw
    opt = starch_amd.BamOptions(no_sort=1)
    assert L.starch_bam_encode_host(fake, b"", 0, ctypes.byref(opt), None) == -2   # an archive needs the sort
    opt = starch_amd.BamOptions()
    assert L.starch_bam_host(fake, None, 5, ctypes.byref(opt)) == -2               # bytes announced, none given
    o = starch_amd._bam_options(True, True, False, True, False, False)
    assert (o.split, o.split_deletions, o.all_reads, o.reduced, o.keep_header, o.no_sort) == (1, 1, 0, 1, 0, 1)
