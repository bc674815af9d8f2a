"""CPU-side checks of convert2bed: the oracle of tests/convert_oracle.py against
its hand-written table, and the parts of the `convert2bed` command and of the
Python interface that open no GPU."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import convert_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERT = os.path.join(ROOT, "starch_amd", "_build", "convert2bed")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help", "convert2bed.txt")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _run(*args, **kw):
    return subprocess.run([CONVERT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracle_gives_the_hand_written_table(case):
    fmt, kw, data, want = oracle.TABLE[case]
    try:
        got = oracle.convert(fmt, data, **kw)
    except oracle.ConvertError as e:
        got = (e.line, e.text)
    assert got == want


def test_table_reaches_every_error_text_and_format():
    texts = {v for k, v in vars(oracle).items() if k.startswith("E_")}
    seen = {want[1] for _, _, _, want in oracle.TABLE if isinstance(want, tuple)}
    assert seen == texts
    assert {fmt for fmt, _, _, _ in oracle.TABLE} == set(oracle.FORMATS)
    assert {kw.get("vcf_class") for fmt, kw, _, _ in oracle.TABLE if fmt == "vcf"} >= {"all", "snvs", "insertions", "deletions"}


def test_oracle_invariants_on_random_inputs():
    rng = random.Random(20261020)
    for fmt in oracle.FORMATS:
        for _ in range(20):
            data = oracle.random_input(fmt, rng, rng.randint(0, 60))
            lines, hdr, rec, dec = oracle.counts(fmt, data)
            assert lines == data.count(b"\n") and hdr + rec + dec == lines
            plain = oracle.convert(fmt, data)
            kept = oracle.convert(fmt, data, keep_header=True)
            assert plain.count(b"\n") == rec and kept.count(b"\n") == rec + hdr
            assert [r for r in kept.split(b"\n") if not r.startswith(b"_header\t")] == plain.split(b"\n")
            assert oracle.sort_bed(plain).count(b"\n") == rec
            if fmt == "vcf":   # every allele lands in exactly one class
                alleles = sum(r.split(b"\t")[4].count(b",") + 1 for r in oracle.lines_of(data) if r and not r.startswith(b"#"))
                assert sum(oracle.convert(fmt, data, vcf_class=c).count(b"\n") for c in ("snvs", "insertions", "deletions")) == alleles


def test_help_is_the_golden_and_opens_no_gpu():
    r = _run("--help")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == open(GOLDEN, "rb").read()
    for word in (b"--input=gff|gtf|vcf|wig", b"--output=bed|starch", b"--do-not-sort", b"--keep-header", b"--snvs", b"--insertions",
                 b"--deletions", b"unverified against a\n  BEDOPS binary", b"zero_length_insertion=True", b"REF-length rule",
                 b"BEDOPS' rule has changed\n         between releases", b"refuses a record without gene_id", b"prints it with %f",
                 b"Not supported: --input=bam|sam|psl|rmsk, --multisplit, --zero-indexed, --do-not-split,\n  --max-mem, --sort-tmpdir"):
        assert word in r.stdout, word
    r = _run("--version")
    assert r.returncode == 0 and r.stdout.startswith(b"convert2bed\n  version: ") and r.stderr == b""


def test_usage_errors_and_unsupported_options():
    missing = os.path.join(ROOT, "no", "such", "file.gff")
    for args in (["--input=bam", missing], ["--input=sam", missing], ["--input=psl", missing], ["--input=rmsk", missing],
                 ["--input=bed", missing],
                 ["--input=gff", "--multisplit=x", missing], ["--input=gff", "--multisplit", missing],
                 ["--input=gff", "--zero-indexed", missing],
                 ["--input=gff", "--do-not-split", missing],
                 ["--input=gff", "--max-mem=2G", missing], ["--input=gff", "--max-mem", "2G", missing],
                 ["--input=gff", "--sort-tmpdir=/tmp", missing],
                 ["--input=gff", "--frobnicate", missing],          # unknown
                 ["--input=gff", "-x", missing],
                 [missing],                                          # no --input
                 [],
                 ["--input"],
                 ["--input=gff", "--input=gtf", missing],
                 ["--input=gff", "--output=bam", missing],
                 ["--input=gff", "--output=starch", "--do-not-sort", missing],
                 ["--input=gff", "--snvs", missing],                 # a class without vcf
                 ["--input=wig", "--deletions", missing],
                 ["--input=vcf", "--snvs", "--insertions", missing],
                 ["--input=vcf", "--deletions", "--deletions", missing],
                 ["--input=gff", missing, missing]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: convert2bed" in r.stderr, args


def test_missing_input_and_missing_gpu():
    missing = os.path.join(ROOT, "no", "such", "file.gff")
    for args in (["--input=gff", missing], ["--input=VCF", "--snvs", "--keep-header", "--do-not-sort", missing],
                 ["--input=Wig", "--output=STARCH", "--device", "0", missing]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b"", args
    for args in (["--input=gtf", "-"], ["--input=wig", "--output=starch"], ["--input=vcf", "--insertions", GOLDEN]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 22 and r.stdout == b"", args
        assert r.stderr == b"Error: no GPU context (HIP device error)\n", args


def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_convert_host", "starch_convert_device", "starch_convert_encode_host", "starch_convert_get_stats",
                 "starch_convert_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    O = starch_amd.ConvertOptions       # four u32
    assert ctypes.sizeof(O) == 16
    assert (O.format.offset, O.vcf_class.offset, O.keep_header.offset, O.no_sort.offset) == (0, 4, 8, 12)
    S = starch_amd.ConvertStats         # eight u64, five floats, padded to 8
    assert ctypes.sizeof(S) == 88
    assert S.sorted.offset == 56 and S.ms_frame.offset == 64 and S.ms_total.offset == 80
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    section = header[header.index("convert2bed: GFF3, GTF, VCF and WIG to BED"):]
    assert "unverified against a BEDOPS binary" in section
    body = re.search(r"typedef struct \{([^}]*)\} starch_convert_stats;", header).group(1)
    fields = re.findall(r"\b(?:input_|header_|data_|declarations|lines_|output_|sorted|ms_)\w*", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in S._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_convert_options;", header).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in O._fields_]
    for name, value in list(starch_amd.CONVERT_FORMATS.items()) + [("vcf_" + k, v) for k, v in starch_amd.VCF_CLASSES.items()]:
        macro = "STARCH_VCF_" + name[4:].upper() if name.startswith("vcf_") else "STARCH_CONVERT_" + name.upper()
        assert re.search(r"#define %s %d\n" % (macro, value), header), macro
    T, W = starch_amd.convert_constants()
    assert T >= 64 and T % 64 == 0 and W == starch_amd.sort_constants()[1]
    for m in ("convert", "convert_device", "compress_converted", "convert_stats"):
        assert callable(getattr(starch_amd.Starch, m))


def test_bad_arguments_are_refused_before_a_device_is_touched():
    import starch_amd
    L = starch_amd.load()
    opt = starch_amd.ConvertOptions()
    assert L.starch_convert_host(None, b"", 0, ctypes.byref(opt)) == -2          # a NULL context
    assert L.starch_convert_device(None, None, 0, ctypes.byref(opt)) == -2
    assert L.starch_convert_encode_host(None, b"", 0, ctypes.byref(opt), None) == -2
    assert L.starch_convert_get_stats(None, None) == -2
    fake = ctypes.c_void_p(1)            # never dereferenced: the options are refused first
    assert L.starch_convert_host(fake, b"", 0, None) == -2
    for fmt, cls in ((4, 0), (0xffffffff, 0), (2, 4), (0, 1), (1, 2), (3, 3)):
        opt = starch_amd.ConvertOptions(format=fmt, vcf_class=cls)
        assert L.starch_convert_host(fake, b"", 0, ctypes.byref(opt)) == -2, (fmt, cls)
        assert L.starch_convert_device(fake, None, 0, ctypes.byref(opt)) == -2, (fmt, cls)
        assert L.starch_convert_encode_host(fake, b"", 0, ctypes.byref(opt), None) == -2, (fmt, cls)
    opt = starch_amd.ConvertOptions(format=0, no_sort=1)
    assert L.starch_convert_encode_host(fake, b"", 0, ctypes.byref(opt), None) == -2   # an archive needs the sort
    with pytest.raises(ValueError):
        starch_amd._convert_options("bam", "all", False, True)
    with pytest.raises(ValueError):
        starch_amd._convert_options("vcf", "mnps", False, True)
