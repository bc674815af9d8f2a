"""CPU-side checks of bedmap-elements: the two oracles of tests/mapel_oracle.py
against each other and the hand-written table, and the parts of the
`bedmap-elements` command and of the Python interface that open no GPU."""
import ctypes
import decimal
import os
import random
import re
import subprocess

import pytest

from tests import mapel_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPEL = os.path.join(ROOT, "starch_amd", "_build", "bedmap-elements")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help", "bedmap-elements.txt")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _run(*args, **kw):
    return subprocess.run([MAPEL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


def random_bed(rng, chroms, lines, limit=120, lengths=(1, 2, 5, 20, 90)):
    rows = []
    for k in range(lines):
        s = rng.randrange(0, limit - 1)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths))), k, rng.randrange(1000)))
    return b"".join(b"%s\t%d\t%d\tn%d\t%d\n" % r for r in sorted(rows))


def random_criterion(rng):
    kind = rng.choice(oracle.CRITERIA)
    if kind == "exact":
        return (kind,)
    if kind in ("bp_ovr", "range"):
        return (kind, rng.choice((1, 2, 3, 10, 50)) - (kind == "range" and rng.random() < 0.3))
    return (kind, rng.choice(("1", "1.0", "0.5", ".25", "0.1", "0.333333333", "0.75", "0.000000001")))


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracles_give_the_hand_written_table(case):
    ref, mp, kw, want = oracle.TABLE[case]
    assert oracle.mapel(ref, mp, **kw) == want
    assert oracle.mapel(ref, mp, finder=oracle.hits_sweep, **kw) == want


def test_the_table_covers_every_column_and_criterion():
    cols, crits = set(), set()
    for _, _, kw, _ in oracle.TABLE:
        cols.update(kw.get("cols", ("echo", "echo_map")))
        crits.add(kw.get("criterion", ("bp_ovr", 1))[0])
    assert cols == set(oracle.COLS) and crits == set(oracle.CRITERIA)
    assert len(oracle.TABLE) >= 20


def test_oracles_agree_on_random_cases():
    rng = random.Random(20261020)
    hits = empty = 0
    seen = set()
    for _ in range(400):
        chroms = [b"chr1", b"chr10", b"chr2"][:rng.randint(1, 3)]
        ref = random_bed(rng, chroms, rng.randint(0, 25))
        mp = None if rng.random() < 0.15 else random_bed(rng, chroms[:rng.randint(1, len(chroms))], rng.randint(0, 40))
        crit = random_criterion(rng)
        cols = rng.sample(oracle.COLS, rng.randint(1, len(oracle.COLS)))
        kw = dict(cols=cols, criterion=crit, skip_unmapped=rng.random() < 0.3)
        a = oracle.mapel(ref, mp, **kw)
        assert a == oracle.mapel(ref, mp, finder=oracle.hits_sweep, **kw), (crit, cols)
        rr = oracle.parse(ref)
        lists = oracle.hits_brute(rr, rr if mp is None else oracle.parse(mp), crit)
        assert lists == oracle.hits_sweep(rr, rr if mp is None else oracle.parse(mp), crit)
        hits += sum(map(len, lists))
        empty += sum(not h for h in lists)
        seen.add(crit[0])
    assert hits > 2000 and empty > 500 and seen == set(oracle.CRITERIA), (hits, empty)


def test_help_is_the_golden_and_opens_no_gpu():
    r = _run("--help")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == open(GOLDEN, "rb").read()
    for word in (b"--echo-map-score", b"--echo-overlap-size", b"--echo-map-range", b"--fraction-either F", b"--exact",
                 b"--multidelim S", b"unverified\n  against a BEDOPS binary", b"Not supported: --echo-map-id-uniq",
                 b"With no column option: --echo --echo-map."):
        assert word in r.stdout, word
    r = _run("--version")
    assert r.returncode == 0 and r.stdout.startswith(b"bedmap-elements\n  version: ") and r.stderr == b""


def test_refused_options_exit_2_before_a_gpu_is_opened():
    missing = os.path.join(ROOT, "no", "such", "file.bed")
    refused = [["--echo-map-id-uniq"], ["--sum"], ["--mean"], ["--min"], ["--max"], ["--median"], ["--bases"], ["--bases-uniq"],
               ["--bases-uniq-f"], ["--chrom", "chr1"], ["--ec"], ["--header"], ["--prec", "3"], ["--sci"], ["--faster"],
               ["--sweep-all"],
               ["--bp-ovr", "2", "--exact"], ["--range", "5", "--fraction-ref", "0.5"], ["--exact", "--exact"],   # two criteria
               ["--fraction-map", "0.5", "--fraction-both", "0.5"], ["--bp-ovr", "1", "--bp-ovr", "1"],
               ["--fraction-ref", "0"], ["--fraction-ref", "0.0"], ["--fraction-ref", "1.01"], ["--fraction-map", "5e-1"],
               ["--fraction-both", "0.1234567891"], ["--fraction-either", ""], ["--fraction-either", "."],
               ["--fraction-ref", "-0.5"], ["--fraction-ref", "2"], ["--fraction-ref", "0.5x"],
               ["--bp-ovr", "0"], ["--bp-ovr", "x"], ["--range", "-1"],
               ["--echo", "--echo"], ["--echo-map", "--echo-map"],
               ["--delim", ""], ["--multidelim", "123456789"], ["--multidelim", "a", "--multidelim", "b"]]
    for args in refused:
        r = _run(*(args + [missing, missing]), stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: bedmap-elements" in r.stderr, args
    for args in ([], [missing, missing, missing], ["--count", "-", "-"]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
    # accepted command lines get as far as the missing file
    for args in (["--fraction-ref", "0.5"], ["--fraction-map", ".5"], ["--fraction-both", "0.500000000"],
                 ["--fraction-either", "1"], ["--fraction-ref", "1.0"], ["--bp-ovr", "7"], ["--range", "0"], ["--exact"],
                 ["--echo", "--count", "--indicator", "--echo-ref-size", "--echo-ref-name", "--echo-ref-row-id", "--echo-map",
                  "--echo-map-id", "--echo-map-score", "--echo-map-size", "--echo-overlap-size", "--echo-map-range",
                  "--delim", "\t", "--multidelim", ",", "--skip-unmapped"]):
        r = _run(*(args + [missing, missing]), stdin=subprocess.DEVNULL)
        assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b"", args


def test_fraction_parsing():
    import starch_amd
    F = starch_amd.mapel_fraction
    assert F("0.5") == (5, 1) and F(".5") == (5, 1) and F("0.500000000") == (500000000, 9)
    assert F("1") == (1, 0) and F("1.0") == (10, 1) and F(".25") == (25, 2) and F("1.") == (1, 0)
    assert F(decimal.Decimal("0.5")) == (5, 1) and F(decimal.Decimal("5E-1")) == (5, 1) and F(b"0.75") == (75, 2)
    for bad in ("0", "0.0", "1.01", "5e-1", "0.1234567891", "", ".", "-0.5", "2", " 0.5", "0.5 ", "0,5", 0.5, 1, None,
                decimal.Decimal("0"), decimal.Decimal("1.5"), decimal.Decimal("NaN"), decimal.Decimal("1E-10")):
        with pytest.raises(ValueError):
            F(bad)
    O = starch_amd._mapel_options
    o = O(("echo",), ("fraction_both", "0.25"), False, b"|", b";")
    assert (o.criterion, o.frac_num, o.frac_digits, o.n, o.range) == (4, 25, 2, 0, 0)
    o = O(("echo",), ("bp_ovr", 7), True, b"|", b";;")
    assert (o.criterion, o.n, o.skip_unmapped, o.multidelim_len, o.multidelim) == (0, 7, 1, 2, b";;")
    assert O(("echo",), ("exact",), False, b"|", b";").criterion == 6 and O(("echo",), "exact", False, b"|", b";").criterion == 6
    for bad in (("fraction_ref", 0.5), ("fraction_ref",), ("exact", 1), ("nearest", 1), ()):
        with pytest.raises(ValueError):
            O(("echo",), bad, False, b"|", b";")
    with pytest.raises(ValueError):
        O(("bases",), ("bp_ovr", 1), False, b"|", b";")


def test_the_size_limits_arithmetic():
    # the refusals compare 64-bit sums: fewer than 2^32 lines of fewer than 2^32 hits each cannot wrap 2^64
    assert (2 ** 32 - 1) * (2 ** 32 - 1) < 2 ** 64
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    block = header[header.index("bedmap-elements: the map lines"):]
    assert "2^32 hits or more in all, or 2^40 output bytes or more, is STARCH_ERR_ARG" in block
    src = open(os.path.join(ROOT, "starch_amd", "csrc", "bed_mapel.hip")).read()
    assert "T >= (1ull << 32)" in src
    assert src.index("T >= (1ull << 32)") < src.index("b_H.as<uint32_t>(T)")            # decided before the hit list
    # the 2^40 refusal is the shared format tail's: asked for here, and decided there before the output is sized
    call = re.search(r'format_tail\([^;]*"bedmap-elements", true\);', src)
    assert call and call.start() < src.index("hipLaunchKernelGGL(k_me_write_line")
    common = open(os.path.join(ROOT, "starch_amd", "csrc", "common.hpp")).read()
    tail = common[common.index("inline FormatTail format_tail("):]
    assert tail.index("limit && tot[0] >= (1ull << 40)") < tail.index("out.as<uint8_t>(tot[0] + 64)")


def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_mapel_host", "starch_mapel_device", "starch_mapel_get_stats", "starch_mapel_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    O = starch_amd.MapelOptions
    assert ctypes.sizeof(O) == 80
    assert [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 16, 20, 24, 32, 40, 48, 52, 56, 60, 68]
    S = starch_amd.MapelStats
    assert ctypes.sizeof(S) == 88
    assert S.hits.offset == 24 and S.walk_steps.offset == 40 and S.output_bytes.offset == 56 and S.ms_total.offset == 84
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    block = header[header.index("bedmap-elements: the map lines"):]
    assert "unverified against a BEDOPS binary" in block and "80 bytes, every field naturally aligned" in block
    for words in ("scores are copied, not reformatted", "there is no --echo-map-id-uniq",
                  "ECHO_MAP_RANGE is empty when there are no hits"):
        assert words in re.sub(r"\s*\n \* ", " ", block), words
    body = re.search(r"typedef struct \{([^}]*)\} starch_mapel_stats;", header).group(1)
    fields = re.findall(r"\b(?:n_|hits|heavy_|walk_|lines_|output_|ms_)\w*", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in S._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_mapel_options;", header).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in O._fields_]
    cols = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"#define STARCH_MAPEL_(?!CRIT_)(\w+) (\d+)", header))
    crit = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"#define STARCH_MAPEL_CRIT_(\w+) (\d+)", header))
    assert cols == starch_amd.MAPEL_COLS and crit == starch_amd.MAPEL_CRITERIA
    assert tuple(starch_amd.MAPEL_COLS) == oracle.COLS and tuple(starch_amd.MAPEL_CRITERIA) == oracle.CRITERIA
    T, F, heavy, bound = starch_amd.mapel_constants()
    assert T >= 64 and T % 64 == 0 and F >= 2 and heavy >= 64 and bound >= 2 * F
    assert F == starch_amd.closest_constants()[1]
    for m in ("map_elements", "map_elements_device", "mapel_stats"):
        assert callable(getattr(starch_amd.Starch, m))


def test_argument_errors_touch_no_device():
    import starch_amd
    L = starch_amd.load()
    one = starch_amd.SetopInput()
    opt = starch_amd._mapel_options(("echo", "echo_map"), ("bp_ovr", 1), False, b"|", b";")
    offs = (ctypes.c_uint64 * 3)(0, 0, 0)
    # a NULL context is refused before anything touches a device
    assert L.starch_mapel_host(None, ctypes.byref(one), ctypes.byref(one), ctypes.byref(opt)) == -2
    assert L.starch_mapel_device(None, None, offs, 2, ctypes.byref(opt)) == -2
    assert L.starch_mapel_get_stats(None, None) == -2
    fake = ctypes.c_void_p(1)            # never dereferenced: the options are checked first

    def rc(o):
        return L.starch_mapel_host(fake, ctypes.byref(one), None, ctypes.byref(o))

    def options(**kw):
        o = starch_amd._mapel_options(("echo", "echo_map"), ("bp_ovr", 1), False, b"|", b";")
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    assert L.starch_mapel_host(fake, ctypes.byref(one), None, None) == -2
    assert L.starch_mapel_host(fake, None, None, ctypes.byref(opt)) == -2
    for kw in (dict(ncols=0), dict(ncols=13), dict(delim_len=0), dict(delim_len=9), dict(multidelim_len=0),
               dict(multidelim_len=9), dict(criterion=7), dict(n=0), dict(range=5),                    # bp_ovr with a range
               dict(frac_num=5), dict(frac_digits=1),
               dict(criterion=1, n=1), dict(criterion=6, n=1),                                       # a second criterion
               dict(criterion=2, n=0, frac_num=0, frac_digits=1), dict(criterion=2, n=0, frac_num=11, frac_digits=1),
               dict(criterion=2, n=0, frac_num=1, frac_digits=10), dict(criterion=3, n=1, frac_num=5, frac_digits=1),
               dict(criterion=4, n=0, range=3, frac_num=5, frac_digits=1)):
        assert rc(options(**kw)) == -2, kw
    o = options()
    o.cols[1] = 0                                                                                # a column twice
    assert rc(o) == -2
    o.cols[1] = 12                                                                               # an unknown column
    assert rc(o) == -2
