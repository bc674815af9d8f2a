"""CPU-side checks of sam2bed, psl2bed and rmsk2bed: the oracle of
tests/align_oracle.py against its hand-written table, and the parts of the three
commands and of the Python interface that open no GPU."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import align_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMANDS = ("sam2bed", "psl2bed", "rmsk2bed")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _golden(cmd):
    return os.path.join(ROOT, "tests", "golden", "cli_help", cmd + ".txt")


def _run(cmd, *args, **kw):
    return subprocess.run([os.path.join(ROOT, "starch_amd", "_build", cmd)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracle_gives_the_hand_written_table(case):
    fmt, kw, data, want = oracle.TABLE[case]
    try:
        got = oracle.convert(fmt, data, **kw)
    except oracle.ConvertError as e:
        got = (e.line, e.text)
    assert got == want


def test_table_reaches_every_error_text_format_and_option():
    texts = {v for k, v in vars(oracle).items() if k.startswith("E_")}
    seen = {want[1] for _, _, _, want in oracle.TABLE if isinstance(want, tuple)}
    assert seen == texts
    assert {fmt for fmt, _, _, _ in oracle.TABLE} == set(oracle.FORMATS)
    options = set()
    for fmt, kw, _, _ in oracle.TABLE:
        options |= {(fmt, k) for k in kw}
    assert options == {("sam", "split"), ("sam", "split_deletions"), ("sam", "all_reads"), ("sam", "reduced"), ("sam", "keep_header"),
                       ("psl", "split"), ("psl", "keep_header"), ("rmsk", "keep_header")}
    cigars = b"".join(data for fmt, _, data, want in oracle.TABLE if fmt == "sam" and not isinstance(want, tuple))
    for op in b"MIDNSHP=X*":
        assert bytes([op]) in cigars


def test_oracle_invariants_on_random_inputs():
    rng = random.Random(20261020)
    for fmt in oracle.FORMATS:
        for _ in range(20):
            data = oracle.random_input(fmt, rng, rng.randint(0, 60))
            lines, hdr, rec, unmapped = oracle.counts(fmt, data)
            assert lines == data.count(b"\n") and hdr + rec == lines
            plain = oracle.convert(fmt, data)
            kept = oracle.convert(fmt, data, keep_header=True)
            assert plain.count(b"\n") == rec - unmapped and kept.count(b"\n") == rec - unmapped + hdr
            assert [r for r in kept.split(b"\n") if not r.startswith(b"_header\t")] == plain.split(b"\n")
            assert oracle.sort_bed(plain).count(b"\n") == rec - unmapped
            if fmt == "sam":
                assert oracle.sam(data, all_reads=True).count(b"\n") == rec
                assert oracle.sam(data, all_reads=True).count(b"_unmapped\t0\t1\t") == unmapped
                split = oracle.sam(data, split=True)
                assert split.count(b"\n") >= plain.count(b"\n")
                assert oracle.sam(data, split=True, split_deletions=True).count(b"\n") >= split.count(b"\n")
                assert [r.split(b"\t")[:6] for r in plain.split(b"\n")[:-1]] == \
                       [r.split(b"\t") for r in oracle.sam(data, reduced=True).split(b"\n")[:-1]]
            if fmt == "psl":
                blocks = sum(int(r.split(b"\t")[17]) for r in oracle.lines_of(data) if r.count(b"\t") == 20)
                assert oracle.psl(data, split=True).count(b"\n") == blocks


@pytest.mark.parametrize("cmd", COMMANDS)
def test_help_is_the_golden_and_opens_no_gpu(cmd):
    r = _run(cmd, "--help")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == open(_golden(cmd), "rb").read()
    words = {"sam2bed": (b"--split-with-deletions", b"--all-reads", b"--reduced", b"--split ", b"eleven fields", b"per-piece name"),
             "psl2bed": (b"--split ", b"copied unread", b"line of dashes"),
             "rmsk2bed": (b"C becomes -", b"copied unread")}[cmd]
    for word in words + (b"USAGE: " + cmd.encode() + b" [--output=bed|starch] [--do-not-sort] [--keep-header]", b"--device N",
                         b"--max-mem, --sort-tmpdir, --zero-indexed, --do-not-split.", b"Not supported: ",
                         b"modelled on BEDOPS' convert2bed", b"unverified\n  against a BEDOPS binary", b"Known or possible differences"):
        assert word in r.stdout, word
    r = _run(cmd, "--version")
    assert r.returncode == 0 and r.stdout.startswith(cmd.encode() + b"\n  version: ") and r.stderr == b""


@pytest.mark.parametrize("cmd", COMMANDS)
def test_usage_errors_and_unsupported_options(cmd):
    missing = os.path.join(ROOT, "no", "such", "file.txt")
    cases = [["--max-mem=2G", missing], ["--max-mem", "2G", missing], ["--sort-tmpdir=/tmp", missing], ["--zero-indexed", missing],
             ["--do-not-split", missing], ["--frobnicate", missing], ["-x", missing], ["--input=sam", missing],
             ["--output=bam", missing], ["--output"], ["--output=starch", "--do-not-sort", missing], [missing, missing]]
    if cmd != "sam2bed":
        cases += [["--split-with-deletions", missing], ["--all-reads", missing], ["--reduced", missing]]
    if cmd == "rmsk2bed":
        cases += [["--split", missing]]
    for args in cases:
        r = _run(cmd, *args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: " + cmd.encode() in r.stderr, args


@pytest.mark.parametrize("cmd", COMMANDS)
def test_missing_input_and_missing_gpu(cmd):
    missing = os.path.join(ROOT, "no", "such", "file.txt")
    options = {"sam2bed": ["--split-with-deletions", "--all-reads", "--reduced"], "psl2bed": ["--split"], "rmsk2bed": []}[cmd]
    for args in ([missing], options + ["--keep-header", "--do-not-sort", missing], ["--output=STARCH", "--device", "0", missing]):
        r = _run(cmd, *args, stdin=subprocess.DEVNULL)
        assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b"", args
    for args in (["-"], ["--output=starch"], options + [_golden(cmd)]):
        r = _run(cmd, *args, stdin=subprocess.DEVNULL)
        assert r.returncode == 22 and r.stdout == b"", args
        assert r.stderr == b"Error: no GPU context (HIP device error)\n", args


def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_align_host", "starch_align_device", "starch_align_encode_host", "starch_align_get_stats",
                 "starch_align_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    O = starch_amd.AlignOptions         # seven u32
    assert ctypes.sizeof(O) == 28
    assert [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 8, 12, 16, 20, 24]
    S = starch_amd.AlignStats           # eight u64, five floats, padded to 8
    assert ctypes.sizeof(S) == 88
    assert S.sorted.offset == 56 and S.ms_frame.offset == 64 and S.ms_total.offset == 80
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    section = header[header.index("sam2bed, psl2bed, rmsk2bed: SAM, PSL and RepeatMasker .out to BED"):]
    assert header.index("convert2bed: GFF3, GTF, VCF and WIG to BED") < len(header) - len(section)   # after convert2bed's
    assert "unverified against a BEDOPS binary" in section
    for word in ("BEDOPS needs\n *         eleven fields", "per-piece name", "copied unread"):
        assert word in section, word
    body = re.search(r"typedef struct \{([^}]*)\} starch_align_stats;", header).group(1)
    fields = re.findall(r"\b(?:input_|header_|records|unmapped_|lines_|output_|sorted|ms_)\w*", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in S._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_align_options;", header).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in O._fields_]
    assert list(starch_amd.ALIGN_FORMATS) == list(oracle.FORMATS)
    for name, value in starch_amd.ALIGN_FORMATS.items():
        assert re.search(r"#define STARCH_ALIGN_%s %d\n" % (name.upper(), value), header), name
    T, W = starch_amd.align_constants()
    assert T >= 64 and T % 64 == 0 and W == starch_amd.sort_constants()[1]
    for m in ("align2bed", "align2bed_device", "compress_aligned", "align_stats"):
        assert callable(getattr(starch_amd.Starch, m))
    for name in ("align_constants", "ALIGN_FORMATS", "AlignOptions", "AlignStats"):
        assert name in starch_amd.__all__


def test_bad_arguments_are_refused_before_a_device_is_touched():
    import starch_amd
    L = starch_amd.load()
    opt = starch_amd.AlignOptions()
    assert L.starch_align_host(None, b"", 0, ctypes.byref(opt)) == -2            # a NULL context
    assert L.starch_align_device(None, None, 0, ctypes.byref(opt)) == -2
    assert L.starch_align_encode_host(None, b"", 0, ctypes.byref(opt), None) == -2
    assert L.starch_align_get_stats(None, None) == -2
    fake = ctypes.c_void_p(1)            # never dereferenced: the options are refused first
    assert L.starch_align_host(fake, b"", 0, None) == -2
    bad = [dict(format=3), dict(format=0xffffffff), dict(format=0, split_deletions=1),
           dict(format=1, reduced=1), dict(format=1, all_reads=1), dict(format=1, split=1, split_deletions=1),
           dict(format=2, split=1), dict(format=2, split=1, split_deletions=1), dict(format=2, reduced=1), dict(format=2, all_reads=1)]
    for kw in bad:
        opt = starch_amd.AlignOptions(**kw)
        assert L.starch_align_host(fake, b"", 0, ctypes.byref(opt)) == -2, kw
        assert L.starch_align_device(fake, None, 0, ctypes.byref(opt)) == -2, kw
        assert L.starch_align_encode_host(fake, b"", 0, ctypes.byref(opt), None) == -2, kw
    for fmt in range(3):
        opt = starch_amd.AlignOptions(format=fmt, no_sort=1)
        assert L.starch_align_encode_host(fake, b"", 0, ctypes.byref(opt), None) == -2   # an archive needs the sort
    with pytest.raises(ValueError):
        starch_amd._align_options("bam", False, False, False, False, False, True)
