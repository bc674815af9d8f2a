"""CPU-side checks of bedmap: the two oracles of tests/map_oracle.py against each
other and against the hand-written table, and the parts of the `bedmap` command
and of the Python interface that open no GPU."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import map_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEDMAP = os.path.join(ROOT, "starch_amd", "_build", "bedmap")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _run(*args, **kw):
    return subprocess.run([BEDMAP] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


def random_bed(rng, chroms, lines, limit=300, lengths=(1, 5, 40, 120)):
    rows = []
    for _ in range(lines):
        s = rng.randrange(0, limit - 1)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths)))))
    return b"".join(b"%s\t%d\t%d\n" % r for r in sorted(rows))


def test_oracles_agree_on_random_cases():
    rng = random.Random(20261019)
    mapped = nested = 0
    for _ in range(200):
        chroms = [b"chr1", b"chr10", b"chr2"][:rng.randint(1, 3)]
        ref = random_bed(rng, chroms, rng.randint(0, 30))
        mp = None if rng.random() < 0.2 else random_bed(rng, chroms[:rng.randint(1, len(chroms))], rng.randint(0, 40))
        kw = dict(cols=oracle.COLS, range=rng.choice((0, 0, 1, 7, 1000)), skip_unmapped=rng.random() < 0.3)
        a, b = oracle.pairs(ref, mp, **kw), oracle.bitmap(ref, mp, **kw)
        assert a == b, (ref, mp, kw)
        for ln in a.split(b"\n")[:-1]:
            f = ln.split(b"|")
            mapped += f[1] != b"0"
            nested += f[2] != f[3]
    assert mapped > 500 and nested > 200, (mapped, nested)   # the cases reach overlaps, and overlaps of overlaps


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracles_give_the_hand_written_table(case):
    ref, mp, kw, want = oracle.TABLE[case]
    assert oracle.pairs(ref, mp, **kw) == want
    assert oracle.bitmap(ref, mp, **kw) == want


def test_help_opens_no_gpu():
    r = _run("--help")
    assert r.returncode == 0 and r.stderr == b""
    assert b"USAGE: bedmap [--echo] [--count] [--bases] [--bases-uniq] [--indicator] [--echo-ref-size]" in r.stdout
    for word in (b"--range N", b"--delim S", b"--skip-unmapped", b"unverified against a BEDOPS binary", b"Not supported"):
        assert word in r.stdout, word
    r = _run("--version")
    assert r.returncode == 0 and r.stdout.startswith(b"bedmap\n  version: ")


def test_usage_errors_and_unsupported_options():
    missing = os.path.join(ROOT, "no", "such", "file.bed")
    for args in (["--count", "--count", missing],            # a repeated option
                 ["--echo", "--range", "1", "--range", "2", missing],
                 ["--bp-ovr", "5", missing],                  # unsupported
                 ["--sum", missing],
                 ["--echo-map", missing],
                 ["--fraction-ref", "0.5", missing],
                 ["--exact", missing],
                 ["--bases-uniq-f", missing],
                 ["--delim", "", missing],
                 ["--delim", "123456789", missing],
                 ["--range", "-1", missing],
                 ["--count"],                                 # no reference
                 ["--count", missing, missing, missing],
                 ["--count", "-", "-"]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: bedmap" in r.stderr, args
    r = _run("--bp-ovr", "1", "--count", missing)             # the default criterion is accepted
    assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b""


def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_map_host", "starch_map_device", "starch_map_get_stats", "starch_map_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    # starch_map_options: u32, 8 x u8, (pad), u64, u32, u32, 8 x char
    O = starch_amd.MapOptions
    assert ctypes.sizeof(O) == 40
    assert (O.ncols.offset, O.cols.offset, O.range.offset, O.skip_unmapped.offset, O.delim_len.offset, O.delim.offset) == \
        (0, 4, 16, 24, 28, 32)
    # starch_map_stats: seven u64, six floats
    assert ctypes.sizeof(starch_amd.MapStats) == 80
    assert starch_amd.MapStats.output_bytes.offset == 48 and starch_amd.MapStats.ms_total.offset == 76
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    for name, code in starch_amd.MAPCOLS.items():
        assert re.search(r"#define STARCH_MAP_%s %d\n" % (name.upper(), code), header), name
    body = re.search(r"typedef struct \{([^}]*)\} starch_map_stats;", header).group(1)
    fields = re.findall(r"\b(?:n_|map_|stops_|lines_|output_|ms_)\w+", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in starch_amd.MapStats._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_map_options;", header).group(1)
    fields = re.findall(r"(\w+)(?:\[8\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in O._fields_]
    T, W = starch_amd.map_constants()
    assert T >= 64 and T % 64 == 0 and W >= 0
    for m in ("bedmap", "bedmap_device", "map_stats"):
        assert callable(getattr(starch_amd.Starch, m))
    # a NULL context is refused before anything touches a device
    one, opt = starch_amd.SetopInput(), starch_amd.MapOptions()
    offs = (ctypes.c_uint64 * 2)(0, 0)
    assert L.starch_map_host(None, ctypes.byref(one), None, ctypes.byref(opt)) == -2
    assert L.starch_map_device(None, None, offs, 1, ctypes.byref(opt)) == -2
    assert L.starch_map_get_stats(None, None) == -2
