"""CPU-side checks of closest-features: the oracle of tests/closest_oracle.py
against the hand-written table and its own invariants, and the parts of the
`closest-features` command and of the Python interface that open no GPU."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import closest_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSEST = os.path.join(ROOT, "starch_amd", "_build", "closest-features")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help", "closest-features.txt")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _run(*args, **kw):
    return subprocess.run([CLOSEST] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


def random_bed(rng, chroms, lines, limit=300, lengths=(1, 5, 40, 120)):
    rows = []
    for _ in range(lines):
        s = rng.randrange(0, limit - 1)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths)))))
    return b"".join(b"%s\t%d\t%d\n" % r for r in sorted(rows))


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracle_gives_the_hand_written_table(case):
    ref, query, kw, want = oracle.TABLE[case]
    assert oracle.closest(ref, query, **kw) == want


def test_oracle_invariants_on_random_cases():
    rng = random.Random(20261020)
    zero = na = 0
    for _ in range(200):
        chroms = [b"chr1", b"chr10", b"chr2"][:rng.randint(1, 3)]
        ref = random_bed(rng, chroms, rng.randint(0, 30))
        query = random_bed(rng, chroms[:rng.randint(1, len(chroms))], rng.randint(0, 40))
        no_overlaps = rng.random() < 0.4
        both = oracle.closest(ref, query, dist=True, no_overlaps=no_overlaps, no_ref=True).split(b"\n")[:-1]
        one = oracle.closest(ref, query, dist=True, no_overlaps=no_overlaps, no_ref=True, closest=True).split(b"\n")[:-1]
        assert len(both) == len(one) == ref.count(b"\n")
        for pair, single in zip(both, one):
            le, ld, re_, rd = pair.split(b"|")
            assert (le == b"NA") == (ld == b"NA") and (re_ == b"NA") == (rd == b"NA")
            if ld != b"NA":
                assert int(ld) <= 0 and not (no_overlaps and int(ld) == 0)
            if rd != b"NA":
                assert int(rd) >= 0 and not (no_overlaps and int(rd) == 0)
            assert single in (le + b"|" + ld, re_ + b"|" + rd)          # closest equals one of the two
            if ld != b"NA" and rd != b"NA":
                assert abs(int(single.split(b"|")[1])) == min(-int(ld), int(rd))
            zero += b"0" in (ld, rd)
            na += b"NA" in (ld, rd)
    assert zero > 300 and na > 100, (zero, na)   # the cases reach overlaps and missing sides


def test_help_is_the_golden_and_opens_no_gpu():
    r = _run("--help")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == open(GOLDEN, "rb").read()
    for word in (b"--closest", b"--shortest", b"--dist", b"--no-overlaps", b"--no-ref", b"--delim S",
                 b"unverified against a BEDOPS binary", b"Not supported: --center, --chrom, --ec, --header"):
        assert word in r.stdout, word
    r = _run("--version")
    assert r.returncode == 0 and r.stdout.startswith(b"closest-features\n  version: ") and r.stderr == b""


def test_usage_errors_and_unsupported_options():
    missing = os.path.join(ROOT, "no", "such", "file.bed")
    for args in (["--center", missing, missing],             # not supported
                 ["--chrom", "chr1", missing, missing],
                 ["--ec", missing, missing],
                 ["--header", missing, missing],
                 ["--nearest", missing, missing],            # unknown
                 ["--delim", "", missing, missing],
                 ["--delim", "123456789", missing, missing],
                 ["--delim", "a", "--delim", "b", missing, missing],
                 [],                                          # no files
                 ["--dist", missing],                         # no query
                 [missing, missing, missing],
                 ["--dist", "-", "-"]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: closest-features" in r.stderr, args
    r = _run("--closest", "--dist", "--no-overlaps", "--no-ref", "--delim", "\t", missing, missing)
    assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b""
    r = _run("--shortest", "-", missing, stdin=subprocess.DEVNULL)
    assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b""


def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_closest_host", "starch_closest_device", "starch_closest_get_stats", "starch_closest_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    # starch_closest_options: five u32, 8 x char
    O = starch_amd.ClosestOptions
    assert ctypes.sizeof(O) == 28
    assert (O.closest.offset, O.dist.offset, O.no_overlaps.offset, O.no_ref.offset, O.delim_len.offset, O.delim.offset) == \
        (0, 4, 8, 12, 16, 20)
    # starch_closest_stats: eight u64, six floats
    S = starch_amd.ClosestStats
    assert ctypes.sizeof(S) == 88
    assert S.left_na.offset == 32 and S.output_bytes.offset == 56 and S.ms_decode.offset == 64 and S.ms_total.offset == 84
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    assert "unverified\n * against a BEDOPS binary" in header[header.index("closest-features: nearest"):]
    body = re.search(r"typedef struct \{([^}]*)\} starch_closest_stats;", header).group(1)
    fields = re.findall(r"\b(?:n_|stops_|left_|right_|lines_|output_|ms_)\w+", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in S._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_closest_options;", header).group(1)
    fields = re.findall(r"(\w+)(?:\[8\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in O._fields_]
    T, F = starch_amd.closest_constants()
    assert T >= 64 and T % 64 == 0 and F >= 2
    for m in ("closest_features", "closest_device", "closest_stats"):
        assert callable(getattr(starch_amd.Starch, m))
    # a NULL context is refused before anything touches a device
    one, opt = starch_amd.SetopInput(), starch_amd.ClosestOptions()
    opt.delim_len, opt.delim = 1, b"|"
    offs = (ctypes.c_uint64 * 3)(0, 0, 0)
    assert L.starch_closest_host(None, ctypes.byref(one), ctypes.byref(one), ctypes.byref(opt)) == -2
    assert L.starch_closest_device(None, None, offs, ctypes.byref(opt)) == -2
    assert L.starch_closest_get_stats(None, None) == -2
