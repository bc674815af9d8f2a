"""CPU-side checks of bedmap-scores: tests/mapscore_oracle.py over both hit
finders and against its hand-written table, and the parts of the
`bedmap-scores` command and of the Python interface that open no GPU."""
import ctypes
import decimal
import os
import random
import re
import subprocess

import pytest

from tests import mapscore_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
MAPSC = os.path.join(BUILD, "bedmap-scores")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
SCORES = (b"0", b"1", b"-1", b"+7", b"-.5", b"3.", b"0.5", b"1.5", b"2.5", b"12.25", b"-0.000000001", b"999999999.999999999",
          b"-999999999.999999999", b"000000001.000000001", b".125", b"42")


def _run(*args, **kw):
    return subprocess.run([MAPSC] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=NO_GPU, **kw)


def random_bed(rng, chroms, lines, limit=120, lengths=(1, 2, 5, 20, 90)):
    rows = []
    for k in range(lines):
        s = rng.randrange(0, limit - 1)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths))), k, rng.choice(SCORES)))
    return b"".join(b"%s\t%d\t%d\tn%d\t%s\n" % r for r in sorted(rows))


def random_criterion(rng):
    kind = rng.choice(oracle.CRITERIA)
    if kind == "exact":
        return (kind,)
    if kind in ("bp_ovr", "range"):
        return (kind, rng.choice((1, 2, 3, 10, 50)))
    return (kind, rng.choice(("1", "0.5", ".25", "0.1", "0.333333333", "0.000000001")))


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_both_hit_finders_give_the_hand_written_table(case):
    ref, mp, kw, want = oracle.TABLE[case]
    assert oracle.mapsc(ref, mp, **kw) == want
    assert oracle.mapsc(ref, mp, finder=oracle.hits_sweep, **kw) == want


def test_the_table_covers_every_column_and_criterion():
    cols, crits, precs, kths = set(), set(), set(), set()
    for _, _, kw, _ in oracle.TABLE:
        cols.update(kw.get("cols", ("echo", "mean")))
        crits.add(kw.get("criterion", ("bp_ovr", 1))[0])
        precs.add(kw.get("prec", 6))
        kths.add(kw.get("kth"))
    assert cols == set(oracle.COLS) and crits == set(oracle.CRITERIA)
    assert {0, 6, 9} <= precs and {"1", "0.5", "0.000000001"} <= kths
    assert len(oracle.TABLE) >= 20
    text = b"".join(mp or b"" for _, mp, _, _ in oracle.TABLE)
    for score in (b"\t+7\n", b"\t-.5\n", b"\t3.\n", b"\t000000001.000000001\n"):
        assert score in text, score


def test_the_oracle_formats_and_parses_exactly():
    F = oracle.Fraction
    assert [oracle.fmt(F(k, 2), 0) for k in (1, 3, 5, -1, -3, -5)] == [b"0", b"2", b"2", b"0", b"-2", b"-2"]
    assert oracle.fmt(F(-4, 10 ** 7), 6) == b"0.000000" and oracle.fmt(F(-6, 10 ** 7), 6) == b"-0.000001"
    assert oracle.fmt(5 * 10 ** 12, 9) == b"5000000000000.000000000" and oracle.fmt(F(19, 6), 9) == b"3.166666667"
    ok = {b"+7": 7 * 10 ** 9, b"-.5": -5 * 10 ** 8, b"3.": 3 * 10 ** 9, b"000000001.000000001": 10 ** 9 + 1, b"0": 0, b"-0.0": 0,
          b"999999999.999999999": 10 ** 18 - 1}
    for text, want in ok.items():
        assert oracle.units([b"c", b"1", b"2", b"x", text]) == want, text
    for text in (b"", b".", b"+", b"-", b"1e3", b"nan", b"inf", b"1.0000000001", b"1234567890", b" 1", b"1 ", b"--1", b"1.2.3", b"0x1"):
        assert oracle.units([b"c", b"1", b"2", b"x", text]) is None, text
    assert oracle.units([b"c", b"1", b"2", b"x"]) is None


def test_hit_finders_agree_on_random_cases():
    rng = random.Random(20261021)
    nan = numbers = 0
    seen = set()
    for _ in range(300):
        chroms = [b"chr1", b"chr10", b"chr2"][:rng.randint(1, 3)]
        ref = random_bed(rng, chroms, rng.randint(0, 25))
        mp = None if rng.random() < 0.15 else random_bed(rng, chroms[:rng.randint(1, len(chroms))], rng.randint(0, 40))
        crit = random_criterion(rng)
        cols = rng.sample(oracle.COLS, rng.randint(1, len(oracle.COLS)))
        kw = dict(cols=cols, criterion=crit, prec=rng.randint(0, 9), skip_unmapped=rng.random() < 0.3,
                  kth=rng.choice(("1", "0.5", "0.9", "0.000000001")) if "kth" in cols else None)
        a = oracle.mapsc(ref, mp, **kw)
        assert a == oracle.mapsc(ref, mp, finder=oracle.hits_sweep, **kw), (crit, cols)
        nan += a.count(b"NAN")
        numbers += a.count(b".")
        seen.add(crit[0])
    assert nan > 300 and numbers > 1000 and seen == set(oracle.CRITERIA), (nan, numbers)


def test_help_is_the_golden_and_opens_no_gpu():
    r = _run("--help")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == open(os.path.join(GOLDEN, "bedmap-scores.txt"), "rb").read()
    for word in (b"--sum", b"--mean", b"--median", b"--kth F", b"--min-element", b"--max-element", b"--prec P",
                 b"unverified\n  against a BEDOPS binary", b"Known differences: scores are exact decimals",
                 b"ties to even", b"no negative zero", b"ties go to map order", b"Not supported: --stdev, --variance, --cv, --mad",
                 b"With no column option: --echo --mean."):
        assert word in r.stdout, word
    r = _run("--version")
    assert r.returncode == 0 and r.stdout.startswith(b"bedmap-scores\n  version: ") and r.stderr == b""


def test_bedmap_elements_help_is_still_its_golden():
    r = subprocess.run([os.path.join(BUILD, "bedmap-elements"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60, env=NO_GPU)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLDEN, "bedmap-elements.txt"), "rb").read()


def test_refused_options_exit_2_before_a_gpu_is_opened():
    missing = os.path.join(ROOT, "no", "such", "file.bed")
    refused = [["--stdev"], ["--variance"], ["--cv"], ["--mad"], ["--mad", "2"], ["--tmean", "0.1", "0.1"], ["--wmean"],
               ["--echo-map-id-uniq"], ["--echo-map"], ["--echo-map-id"], ["--echo-map-score"], ["--echo-map-range"],
               ["--bases"], ["--bases-uniq"], ["--bases-uniq-f"], ["--chrom", "chr1"], ["--ec"], ["--header"], ["--sci"],
               ["--faster"], ["--sweep-all"], ["--multidelim", ";"],
               ["--bp-ovr", "2", "--exact"], ["--range", "5", "--fraction-ref", "0.5"], ["--exact", "--exact"],   # two criteria
               ["--fraction-map", "0.5", "--fraction-both", "0.5"], ["--bp-ovr", "1", "--bp-ovr", "1"],
               ["--fraction-ref", "0"], ["--fraction-ref", "1.01"], ["--fraction-map", "5e-1"], ["--fraction-both", "0.1234567891"],
               ["--bp-ovr", "0"], ["--bp-ovr", "x"], ["--range", "-1"],
               ["--echo", "--echo"], ["--mean", "--mean"], ["--sum", "--count", "--sum"], ["--kth", "0.5", "--kth", "0.6"],
               ["--min-element", "--min-element"], ["--min", "--max", "--min"],
               ["--kth", "0"], ["--kth", "1.5"], ["--kth", "5e-1"], ["--kth", ""], ["--kth", "0.1234567891"], ["--kth", "-0.5"],
               ["--prec", "10"], ["--prec", "-1"], ["--prec", "x"], ["--prec", ""], ["--prec", "3", "--prec", "3"],
               ["--delim", ""], ["--delim", "123456789"], ["--delim", "a", "--delim", "b"], ["--skip-unmapped", "--skip-unmapped"]]
    for args in refused:
        r = _run(*(args + [missing, missing]), stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
        assert r.stderr.startswith(b"Error: ") and b"USAGE: bedmap-scores" in r.stderr, args
    for args in ([], [missing, missing, missing], ["--count", "-", "-"]):
        r = _run(*args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", args
    # accepted command lines get as far as the missing file
    for args in ([], ["--mean"], ["--fraction-ref", "0.5"], ["--fraction-either", "1"], ["--bp-ovr", "7"], ["--range", "0"],
                 ["--exact"], ["--prec", "0"], ["--prec", "9"], ["--kth", "1"], ["--kth", ".000000001"], ["--kth", "1.0"],
                 ["--echo", "--count", "--indicator", "--sum", "--mean", "--min", "--max", "--median", "--kth", "0.5",
                  "--min-element", "--max-element", "--prec", "3", "--delim", "\t", "--skip-unmapped"]):
        r = _run(*(args + [missing, missing]), stdin=subprocess.DEVNULL)
        assert r.returncode == 61 and b"does not exist" in r.stderr and r.stdout == b"", args


def test_python_options():
    import starch_amd
    O = starch_amd._mapsc_options
    o = O(("echo", "mean"), ("bp_ovr", 1), 6, None, False, b"|")
    assert (o.ncols, list(o.cols[:2]), o.criterion, o.n, o.prec, o.kth_num, o.kth_digits, o.delim_len, o.delim) == \
        (2, [0, 4], 0, 1, 6, 0, 0, 1, b"|")
    o = O(("kth",), ("fraction_both", "0.25"), 0, decimal.Decimal("0.5"), True, b"<=>")
    assert (o.criterion, o.frac_num, o.frac_digits, o.n, o.kth_num, o.kth_digits, o.prec, o.skip_unmapped, o.delim) == \
        (4, 25, 2, 0, 5, 1, 0, 1, b"<=>")
    assert O(("kth",), "exact", 9, "0.000000001", False, b"|").kth_digits == 9
    for bad in (0.5, 1, "0", "1.5", "5e-1", "0.1234567891", decimal.Decimal("NaN")):     # kth is an exact decimal in (0, 1]
        with pytest.raises(ValueError):
            O(("kth",), ("bp_ovr", 1), 6, bad, False, b"|")
    for prec in (1.0, "3", None, True, -1):
        with pytest.raises(ValueError):
            O(("sum",), ("bp_ovr", 1), prec, None, False, b"|")
    with pytest.raises(ValueError):
        O(("echo_map",), ("bp_ovr", 1), 6, None, False, b"|")
    with pytest.raises(ValueError):
        O(("sum",), ("fraction_ref", 0.5), 6, None, False, b"|")


def test_ctypes_declarations_match_the_header():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_mapsc_host", "starch_mapsc_device", "starch_mapsc_get_stats", "starch_mapsc_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    O = starch_amd.MapscOptions
    assert ctypes.sizeof(O) == 80
    assert [n for n, _ in O._fields_] == ["ncols", "cols", "criterion", "frac_digits", "n", "range", "frac_num", "kth_num",
                                          "kth_digits", "prec", "skip_unmapped", "delim_len", "delim"]
    assert [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 16, 20, 24, 32, 40, 48, 56, 60, 64, 68, 72]
    S = starch_amd.MapscStats
    assert ctypes.sizeof(S) == 104
    assert S.hits.offset == 24 and S.straddling.offset == 32 and S.output_bytes.offset == 64 and S.ms_total.offset == 96
    header = open(os.path.join(ROOT, "include", "starch_amd.h")).read()
    block = header[header.index("bedmap-scores: statistics of the scores"):header.index("---- convert2bed")]
    flat = re.sub(r"\s*\n \* ", " ", block)
    for words in ("unverified against a BEDOPS binary", "80 bytes, every field naturally aligned",
                  "scores are exact decimals, not strtod doubles", "ties to even, not printf of a double",
                  "there is no negative zero", "element ties go to map order", "KTH is defined as above",
                  "--stdev, --variance, --cv, --mad, --tmean, --wmean and --echo-map-id-uniq are not supported",
                  "2^32 hits or more in all, or 2^40 output bytes or more, is STARCH_ERR_ARG"):
        assert words in flat, words
    body = re.search(r"typedef struct \{([^}]*)\} starch_mapsc_stats;", header).group(1)
    fields = re.findall(r"\b(?:n_|hits|straddling|sorted_|radix_|lines_|output_|ms_)\w*", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in S._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} starch_mapsc_options;", header).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in O._fields_]
    cols = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"#define STARCH_MAPSC_(\w+) (\d+)", header))
    assert cols == starch_amd.MAPSC_COLS and tuple(starch_amd.MAPSC_COLS) == oracle.COLS
    assert tuple(starch_amd.MAPEL_CRITERIA) == oracle.CRITERIA
    tile, wave = starch_amd.mapsc_constants()
    assert tile >= 256 and tile % 64 == 0 and wave == starch_amd.sort_constants()[1]
    for m in ("map_scores", "map_scores_device", "mapsc_stats"):
        assert callable(getattr(starch_amd.Starch, m))
    for name in ("mapsc_constants", "MAPSC_COLS", "MapscOptions", "MapscStats"):
        assert name in starch_amd.__all__


def test_the_size_limits_are_decided_before_the_buffers():
    # bedmap-scores takes its hit list, and with it the 2^32 refusal, from bedmap-elements' stages
    src = open(os.path.join(ROOT, "starch_amd", "csrc", "bed_mapel.hip")).read()
    hits = src[src.index("int MapelWorkspace::hits("):src.index("void MapelWorkspace::run(")]
    assert hits.index("T >= (1ull << 32)") < hits.index("b_H.as<uint32_t>(T)")
    assert '": result too large (2^32 hits or more)"' in hits
    src = open(os.path.join(ROOT, "starch_amd", "csrc", "bed_mapscore.hip")).read()
    assert "hitter.hits(sorter, lines, \"bedmap-scores\"" in src
    # the 2^40 refusal is the shared format tail's: asked for here, and decided there before the output is sized
    call = re.search(r'format_tail\([^;]*"bedmap-scores", true\);', src)
    assert call and call.start() < src.index("hipLaunchKernelGGL(k_ms_write")
    common = open(os.path.join(ROOT, "starch_amd", "csrc", "common.hpp")).read()
    tail = common[common.index("inline FormatTail format_tail("):]
    assert tail.index("limit && tot[0] >= (1ull << 40)") < tail.index("out.as<uint8_t>(tot[0] + 64)")


def test_argument_errors_touch_no_device():
    import starch_amd
    L = starch_amd.load()
    one = starch_amd.SetopInput()
    opt = starch_amd._mapsc_options(("echo", "mean"), ("bp_ovr", 1), 6, None, False, b"|")
    offs = (ctypes.c_uint64 * 3)(0, 0, 0)
    # a NULL context is refused before anything touches a device
    assert L.starch_mapsc_host(None, ctypes.byref(one), ctypes.byref(one), ctypes.byref(opt)) == -2
    assert L.starch_mapsc_device(None, None, offs, 2, ctypes.byref(opt)) == -2
    assert L.starch_mapsc_get_stats(None, None) == -2
    fake = ctypes.c_void_p(1)            # never dereferenced: the options are checked first

    def rc(o):
        return L.starch_mapsc_host(fake, ctypes.byref(one), None, ctypes.byref(o))

    def options(cols=("echo", "mean"), kth=None, **kw):
        o = starch_amd._mapsc_options(cols, ("bp_ovr", 1), 6, kth, False, b"|")
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    assert L.starch_mapsc_host(fake, ctypes.byref(one), None, None) == -2
    assert L.starch_mapsc_host(fake, None, None, ctypes.byref(opt)) == -2
    assert L.starch_mapsc_device(fake, None, None, 2, ctypes.byref(opt)) == -2
    assert L.starch_mapsc_device(fake, None, offs, 3, ctypes.byref(opt)) == -2
    for kw in (dict(ncols=0), dict(ncols=13), dict(delim_len=0), dict(delim_len=9), dict(prec=10), dict(prec=2 ** 32 - 1),
               dict(kth_num=5), dict(kth_digits=1), dict(kth_num=5, kth_digits=1),                  # a stray kth
               dict(criterion=7), dict(n=0), dict(range=5), dict(frac_num=5), dict(frac_digits=1),
               dict(criterion=1, n=1), dict(criterion=6, n=1),                                      # a second criterion
               dict(criterion=2, n=0, frac_num=11, frac_digits=1), dict(criterion=2, n=0, frac_num=1, frac_digits=10)):
        assert rc(options(**kw)) == -2, kw
    for kw in (dict(kth_num=0), dict(kth_num=11, kth_digits=1), dict(kth_num=1, kth_digits=10), dict(kth_num=2, kth_digits=0)):
        assert rc(options(cols=("kth",), kth="0.5", **kw)) == -2, kw                                 # a bad kth
    assert rc(options(cols=("kth",))) == -2                                                      # KTH without a kth
    o = options()
    o.cols[1] = 0                                                                                # a column twice
    assert rc(o) == -2
    o.cols[1] = 11                                                                               # an unknown column
    assert rc(o) == -2
