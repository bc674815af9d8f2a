"""GPU: bedmap-scores (Starch.map_scores, map_scores_device, the bedmap-scores
command).

Every comparison is equality of whole outputs against tests/mapscore_oracle.py
or literal bytes; there are no tolerances.  TILE is the number of contiguous
hits of the hit list that one workgroup of the segmented reduction takes, WAVE
the bytes from which a copied line is left to a whole wave; both are read from
mapsc_constants().  The layouts around TILE have thousands of lines, so their
expected outputs take the hit lists from the oracle's sweep, which
tests/test_mapscore_cpu.py holds against the brute force.
"""
import os
import random
import subprocess

import pytest

from tests import mapscore_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPSC = os.path.join(ROOT, "starch_amd", "_build", "bedmap-scores")
CRITS = (("bp_ovr", 1), ("bp_ovr", 3), ("range", 7), ("fraction_ref", "0.5"), ("fraction_map", "0.25"),
         ("fraction_both", "0.1"), ("fraction_either", "0.75"), ("exact",))
BIG = 10 ** 18 - 1                       # 999999999.999999999 in units

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def K():
    import starch_amd
    return starch_amd.mapsc_constants()


def dec(u, plain=True):
    """The score of u units as text; not plain: a '+' or no trailing zeros now and then"""
    q, r = divmod(abs(u), 10 ** 9)
    t = b"%d.%09d" % (q, r)
    if not plain:
        t = (t.rstrip(b"0"), t, t.rstrip(b"0").rstrip(b"."), t[1:] if q == 0 and r else t)[abs(u) % 4]
    return (b"-" if u < 0 else b"" if plain or u % 3 else b"+") + t


def rscore(rng):
    u = rng.choice((rng.randrange(-BIG, BIG + 1), rng.randrange(-5000, 5000) * 10 ** 8, rng.randrange(-300, 300),
                    rng.randrange(-10 ** 12, 10 ** 12)))
    return dec(u, plain=False)


def bed(rows, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % ((chrom,) + tuple(r) if len(r) == 2 else tuple(r)) for r in rows)


def random_bed(rng, chroms, lines, limit=300, lengths=(1, 2, 7, 40, 200)):
    rows = []
    for k in range(lines):
        s = rng.randrange(0, limit - 2)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths))), k, rscore(rng)))
    return b"".join(b"%s\t%d\t%d\tn%d\t%s\n" % r for r in sorted(rows))


def layout(counts, score):
    """Disjoint reference lines, line k with counts[k] map lines inside it; score(k, t) is the text of its t-th"""
    w = 2 * max(max(counts), 1) + 4
    ref = b"".join(b"chr1\t%d\t%d\tr%d\n" % (k * w, k * w + w // 2, k) for k in range(len(counts)))
    mp = b"".join(b"chr1\t%d\t%d\tm%d\t%s\n" % (k * w + t, k * w + t + 1, t, score(k, t))
                  for k, c in enumerate(counts) for t in range(c))
    return ref, mp


def check(ctx, ref, mp=None, finder=oracle.hits_brute, **kw):
    got = ctx.map_scores(ref, mp, **kw)
    assert got == oracle.mapsc(ref, mp, finder=finder, **kw), kw
    return got


def consistent(s):
    """sorted_hits and radix_passes of the last call: the radix stage ran over all hits, or not at all"""
    return (s["sorted_hits"] == 0 and s["radix_passes"] == 0) or (s["sorted_hits"] == s["hits"] > 0 and s["radix_passes"] >= 1)


@pytest.fixture(scope="module")
def pair():
    rng = random.Random(1)
    return random_bed(rng, [b"chr1", b"chr2"], 400), random_bed(rng, [b"chr1", b"chr2", b"chr3"], 500)


# ---- 1. table, criteria, columns --------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_hand_written_table(ctx, case):
    ref, mp, kw, want = oracle.TABLE[case]
    assert ctx.map_scores(ref, mp, **kw) == want


@pytest.mark.parametrize("crit", CRITS, ids=lambda c: "-".join(map(str, c)))
def test_every_criterion_with_every_column(ctx, pair, crit):
    r, m = pair
    for col in oracle.COLS:
        check(ctx, r, m, cols=(col,), criterion=crit, kth="0.3" if col == "kth" else None)
    check(ctx, r, m, cols=oracle.COLS, criterion=crit, kth="0.5")
    check(ctx, r, m, cols=oracle.COLS[::-1], criterion=crit, kth="1", prec=0, skip_unmapped=True, delim=b"<=delim>")
    check(ctx, r, None, cols=("count", "sum", "median", "max_element"), criterion=crit, prec=9)
    s = ctx.mapsc_stats()
    assert (s["n_ref"], s["n_map"], s["lines_out"]) == (400, 400, 400) and consistent(s)
    assert all(s[k] >= 0 for k in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_reduce", "ms_format")) and s["ms_total"] > 0


def test_shapes(ctx):
    a, q = bed([(1, 5), (9, 12)]), b"chr1\t3\t10\tx\t1.5\nchr1\t20\t30\ty\t2\n"
    assert ctx.map_scores(b"", q) == b""
    s = ctx.mapsc_stats()
    assert (s["n_ref"], s["n_map"], s["hits"], s["lines_out"], s["output_bytes"]) == (0, 2, 0, 0, 0)
    assert ctx.map_scores(b"", b"") == b"" and ctx.map_scores(b"") == b""
    assert ctx.map_scores(a, b"") == b"chr1\t1\t5|NAN\nchr1\t9\t12|NAN\n"
    assert ctx.map_scores(a, q) == b"chr1\t1\t5|1.500000\nchr1\t9\t12|1.500000\n"
    for x, y in ((a[:-1], q), (a, q[:-1]), (a[:-1], q[:-1])):   # a last line without '\n': the score ends at the line
        assert ctx.map_scores(x, y, cols=("echo", "sum", "min_element"), prec=1) == \
            b"chr1\t1\t5|1.5|chr1\t3\t10\tx\t1.5\nchr1\t9\t12|1.5|chr1\t3\t10\tx\t1.5\n"
    got = ctx.map_scores(a, q, cols=("count", "mean"), criterion=("bp_ovr", 2), skip_unmapped=True)
    assert got == b"1|1.500000\n"
    s = ctx.mapsc_stats()
    assert (s["hits"], s["lines_out"], s["output_bytes"], s["straddling"]) == (1, 1, len(got), 0)


def test_random_dense_cases(ctx):
    names = [b"c", b"ch", b"chr", b"chr1"]
    for seed in range(100):
        rng = random.Random(9000 + seed)
        ref = random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(1, 80))
        mp = None if seed % 9 == 0 else random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(0, 80))
        cols = rng.sample(oracle.COLS, rng.randint(1, len(oracle.COLS)))
        kw = dict(cols=cols, criterion=rng.choice(CRITS), prec=rng.randint(0, 9), skip_unmapped=rng.random() < 0.3,
                  kth=rng.choice(("1", "0.5", "0.25", "0.9", "0.000000001")) if "kth" in cols else None)
        assert ctx.map_scores(ref, mp, **kw) == oracle.mapsc(ref, mp, **kw), (seed, kw)
        assert consistent(ctx.mapsc_stats())


# ---- 2. the segmented reduction around its tile ----------------------------------------------------------------------
def _layouts(total, tile):
    rest = total % tile
    yield "one segment", [total]
    yield "segments of a tile", [tile] * (total // tile) + ([rest] if rest else [])
    yield "segments of one", [1] * total
    head = [tile - 3, 3] if total >= tile else [total - 3, 3]
    yield "ends at a tile's last hit", head + ([1, 1, total - tile - 2] if total > tile + 2 else [total - tile] * (total > tile))
    yield "lines without hits between", [0, 5, 0, 0, total - 5 - min(70, total - 5), 0] + [1, 0] * min(70, total - 5) + [0, 0]
    yield "a wave of one-hit segments", [100] + [1] * 130 + [total - 230 - 64 - 7] + [1] * 64 + [7]
    yield "around the wave", [63, 64, 65, 1, 511, 1, 512, 513] + [total - 1730]


@pytest.mark.parametrize("which", ("TILE-1", "TILE", "TILE+1", "3*TILE+5"))
def test_hits_around_the_tile(ctx, K, which):
    tile = K[0]
    total = {"TILE-1": tile - 1, "TILE": tile, "TILE+1": tile + 1, "3*TILE+5": 3 * tile + 5}[which]
    rng = random.Random(total)
    cols = ("count", "sum", "mean", "min", "max", "median", "kth", "min_element", "max_element")
    for name, counts in _layouts(total, tile):
        assert sum(counts) == total and min(counts) >= 0, (name, counts)
        ref, mp = layout(counts, lambda k, t: rscore(rng))
        check(ctx, ref, mp, finder=oracle.hits_sweep, cols=cols, kth="0.1", prec=rng.randint(0, 9))
        s = ctx.mapsc_stats()
        assert s["hits"] == total and consistent(s), name
        assert s["straddling"] == oracle.straddling(ref, mp, ("bp_ovr", 1), tile, finder=oracle.hits_sweep), name
        if name == "one segment":
            assert s["straddling"] == (1 if total > tile else 0)
        if name == "segments of a tile":
            assert s["straddling"] == 0
        check(ctx, ref, mp, finder=oracle.hits_sweep, cols=("sum", "max"), prec=9)        # without the sort and the elements
        assert ctx.mapsc_stats()["sorted_hits"] == 0


def test_sums_beyond_64_bits(ctx):
    # 5000 hits of 999999999.999999999 are about 5 * 10^21 units: more than 2^64, and several tiles
    ref, mp = layout([5000], lambda k, t: dec(BIG))
    assert ctx.map_scores(ref, mp, cols=("sum", "mean", "count"), prec=9) == b"4999999999999.999995000|999999999.999999999|5000\n"
    ref, mp = layout([5000, 3], lambda k, t: dec(-BIG))
    assert ctx.map_scores(ref, mp, cols=("sum", "mean"), prec=0) == b"-5000000000000|-1000000000\n-3000000000|-1000000000\n"
    # mixed signs that cancel to exactly 0, and to one unit
    ref, mp = layout([5000, 4999], lambda k, t: dec(BIG if t % 2 else -BIG))
    assert ctx.map_scores(ref, mp, cols=("sum", "mean", "min", "max"), prec=9) == \
        b"0.000000000|0.000000000|-999999999.999999999|999999999.999999999\n" \
        b"-999999999.999999999|-200040.008001600|-999999999.999999999|999999999.999999999\n"
    check(ctx, ref, mp, finder=oracle.hits_sweep, cols=("sum", "mean", "median"), prec=6)


def test_mean_of_a_prime_number_of_hits(ctx, K):
    rng = random.Random(5)
    for n in (7, 2053):                                                             # 2053 is prime and more than a tile of 2048
        ref, mp = layout([n, 3], lambda k, t: rscore(rng))
        check(ctx, ref, mp, finder=oracle.hits_sweep, cols=("mean", "sum", "count"), prec=9)
    ref, mp = layout([7], lambda k, t: b"1" if t == 0 else b"0")
    assert ctx.map_scores(ref, mp, cols=("mean",), prec=9) == b"0.142857143\n"


# ---- 3. the order statistics ---------------------------------------------------------------------------------------------
def test_order_statistics_of_hits_already_in_order(ctx):
    cols = ("median", "kth", "count")
    for name, score in (("equal", lambda k, t: b"2.5"), ("ascending", lambda k, t: dec((t - 40) * 10 ** 8 + k)),
                        ("equal per line", lambda k, t: dec(-k))):
        ref, mp = layout([1, 100, 0, 77, 2], score)
        for kth in ("0.000000001", "0.5", "1"):
            check(ctx, ref, mp, cols=cols, kth=kth)
            s = ctx.mapsc_stats()
            assert consistent(s), name
            if name != "equal per line":        # there the key falls from one line to the next, but (line, key) never does
                assert (s["sorted_hits"], s["radix_passes"]) == (0, 0), name
    ref, mp = layout([1, 100, 0, 77, 2], lambda k, t: dec(-t))
    check(ctx, ref, mp, cols=cols, kth="0.5")
    s = ctx.mapsc_stats()
    assert consistent(s) and s["sorted_hits"] == s["hits"] == 180 and s["radix_passes"] >= 1


def test_order_statistics_by_key_byte(ctx):
    rng = random.Random(8)
    top = [k * 2 ** 56 for k in range(-13, 14)]                 # differ in the top byte of the key alone
    low = list(range(256))                                      # in the lowest byte alone
    near = [-2, -1, 0, 1, 2, -10 ** 9, 10 ** 9, -BIG, BIG]      # negative next to positive
    for name, values, passes in (("top", top, 1), ("low", low, 1), ("near", near, None)):
        vals = values[:]
        rng.shuffle(vals)
        ref, mp = layout([len(vals)], lambda k, t: dec(vals[t]))
        for kth in ("0.000000001", "1", "0.5"):                # k = 1, k = n, the middle
            got = check(ctx, ref, mp, cols=("kth", "median", "min", "max"), kth=kth, prec=9)
            s = ctx.mapsc_stats()
            assert consistent(s) and s["sorted_hits"] == len(vals), name
            if passes:
                assert s["radix_passes"] == passes, name      # one line, one byte that varies
        w = sorted(vals)
        assert got.split(b"|")[0] == oracle.fmt(oracle.Fraction(w[(len(w) + 1) // 2 - 1], 10 ** 9), 9)
    # several lines: every line's k-th is its own
    counts = [5, 1, 64, 0, 2, 300]
    ref, mp = layout(counts, lambda k, t: dec(rng.choice(top + low + near)))
    for kth in ("0.000000001", "1", "0.37"):
        check(ctx, ref, mp, cols=("count", "kth", "median"), kth=kth, prec=9)


def test_long_element_lines_and_ties(ctx, K):
    wave = K[1]
    rng = random.Random(3)
    rows = []
    for t in range(40):
        tail = b"x" * rng.choice((0, 10, wave - 30, wave - 1, wave, wave + 1, 3 * wave + 7))
        rows.append(b"chr1\t%d\t%d\tm%d\t%s\t%s\n" % (t, t + 1, t, rng.choice((b"1", b"1.0", b"+1", b"2", b"2.000", b"-3", b"-3.0")), tail))
    mp = b"".join(rows)
    ref = b"chr1\t0\t10\nchr1\t0\t40\tall\t" + b"r" * (2 * wave) + b"\nchr1\t5\t25\tmid\nchr1\t39\t40\nchr1\t50\t60\n"
    got = check(ctx, ref, mp, cols=("min_element", "echo", "max_element", "count"))
    first = got.split(b"\n")[1].split(b"|")             # the line that covers every map line
    assert first[0].split(b"\t")[4] in (b"-3", b"-3.0") and first[2].split(b"\t")[4] in (b"2", b"2.000")
    check(ctx, ref, mp, cols=("max_element", "min_element"), skip_unmapped=True, delim=b"\t")
    check(ctx, mp, None, cols=("echo", "min_element", "max_element"), criterion=("range", 3))


def test_every_mix_of_short_and_long_copies(ctx, K):
    import itertools
    from tests import wave_lines
    W = K[1]
    # the echoed line, the min element and the max element W - 1, W or W + 1 bytes long: every mix with a long one
    mixes = [s for s in itertools.product((W - 1, W, W + 1), repeat=3) if max(s) >= W]
    assert len(mixes) == 26
    ref, mp = [], []
    for k in range(8 * len(mixes)):
        e, lo, hi = mixes[k % len(mixes)]
        ref.append(wave_lines.line(k, e, width=9))
        mp.append(wave_lines.line(k, lo, off=1, width=1, score=b"1"))
        mp.append(wave_lines.line(k, hi, off=3, width=1, score=b"2"))
    check(ctx, b"".join(ref), b"".join(mp), cols=("echo", "min_element", "max_element"))
    check(ctx, b"".join(ref), b"".join(mp), cols=("max_element", "sum", "echo", "min_element"), delim=b"<=>")


def test_copies_left_to_the_wave(ctx, K):
    from tests import wave_lines
    # the echo and both elements long at lanes 0 and 63 of the first wave and lane 0 of the third, then none at all
    for r, m in wave_lines.wave_pairs(K[1]):
        check(ctx, r, m, cols=("echo", "min_element", "max_element"))
        check(ctx, r, m, cols=("count", "max_element", "echo"), skip_unmapped=True)


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------
def _refused(ctx, ref, mp, code, *words, **kw):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.map_scores(ref, mp, **kw)
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    assert ctx.map_scores(bed([(1, 2)]), b"chr1\t1\t6\tx\t-.5\n") == b"chr1\t1\t2|-0.500000\n"   # works again


def test_errors(ctx):
    import starch_amd
    good = b"chr1\t500\t600\ta\t1\nchr1\t700\t800\tb\t2\n"
    lo = b"chr1\t1\t2\ta\t1\nchr1\t3\t4\tb\t1\nchr1\t2\t9\tc\t1\nchr1\t0\t1\td\t1\n"
    _refused(ctx, lo, good, -12, "bedmap-scores: input 0, line 3:", "sort-bed")
    _refused(ctx, good, lo, -12, "bedmap-scores: input 1, line 3:", "sort-bed")
    _refused(ctx, good, b"chr1\t1\t2\tx\t1\nchr1\t5\t5\tx\t1\n", -12, "input 1, line 2:", "stop")
    _refused(ctx, lo, b"chr1\t1\t2\nchr1\t5\n", -12, "input 1, line 2:", "fewer than three")   # malformed goes first
    # hits that lack column 5: the lowest such hit line is named; the same lines as non-hits are accepted
    mp = b"chr1\t1\t5\ta\t1\nchr1\t20\t30\nchr1\t40\t50\tc\nchr1\t60\t70\td\t\nchr1\t80\t90\te\t7\n"
    near, far = bed([(2, 3), (25, 26), (45, 46), (65, 66)]), bed([(2, 3), (85, 86)])
    for cols in (("sum",), ("count", "median"), ("kth",), ("min_element",), ("echo", "mean")):
        _refused(ctx, near, mp, -12, "bedmap-scores: input 1, line 2:", "column 5", cols=cols, kth="0.5" if "kth" in cols else None)
    _refused(ctx, bed([(2, 3), (45, 46), (65, 66)]), mp, -12, "input 1, line 3:", cols=("max",))
    _refused(ctx, bed([(65, 66)]), mp, -12, "input 1, line 4:", cols=("max",))
    _refused(ctx, mp, None, -12, "bedmap-scores: input 0, line 2:", cols=("sum",))
    assert ctx.map_scores(far, mp, cols=("sum", "count"), prec=0) == b"1|1\n7|1\n"
    assert ctx.map_scores(near, mp, cols=("echo", "count", "indicator")) == oracle.mapsc(near, mp, cols=("echo", "count", "indicator"))
    with pytest.raises(oracle.BadScore) as e:
        oracle.mapsc(near, mp, cols=("sum",))
    assert e.value.line == 2
    # scores outside the grammar
    for text in (b"1e3", b"nan", b"1.0000000001", b"1234567890", b"inf", b"", b".", b"+", b"1 ", b"0x10", b"1,5", b"--1"):
        mp = b"chr1\t1\t5\ta\t1\nchr1\t10\t20\tb\t" + text + b"\tmore\nchr1\t30\t40\tc\t" + text + b"\nchr1\t50\t60\td\t4\n"
        _refused(ctx, bed([(2, 3), (15, 16), (35, 36)]), mp, -12, "bedmap-scores: input 1, line 2:", cols=("mean",))
        _refused(ctx, bed([(2, 3), (35, 36)]), mp, -12, "bedmap-scores: input 1, line 3:", cols=("min",))
        assert ctx.map_scores(bed([(2, 3), (55, 56)]), mp, cols=("sum",), prec=0) == b"1\n4\n"        # they are no hits
        assert ctx.map_scores(bed([(2, 3), (15, 16), (35, 36)]), mp, cols=("echo", "count")) == \
            b"chr1\t2\t3|1\nchr1\t15\t16|1\nchr1\t35\t36|1\n"                                      # no score is looked at
    for kw in (dict(delim=b""), dict(delim=b"123456789"), dict(cols=()), dict(cols=("echo", "echo")), dict(criterion=("bp_ovr", 0)),
               dict(prec=10), dict(cols=("kth",)), dict(kth="0.5"), dict(cols=oracle.COLS + ("echo", "count"), kth="0.5")):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.map_scores(good, good, **kw)
        assert e.value.code == -2, kw
    assert ctx.map_scores(bed([(1, 2)]), b"chr1\t1\t6\tx\t-.5\n") == b"chr1\t1\t2|-0.500000\n"


# ---- 5. archives, device entry, command, the sibling commands ---------------------------------------------------------------
def test_archives(ctx, pair):
    r, m = pair
    ar, am = ctx.compress(r), ctx.compress(m)
    assert ar[:4] == b"\xca\x5c\xad\x1a"
    kw = dict(cols=("echo", "count", "mean", "median", "max_element"), criterion=("fraction_either", "0.5"), prec=3)
    want = check(ctx, r, m, **kw)
    assert ctx.map_scores(ar, m, **kw) == ctx.map_scores(r, am, **kw) == ctx.map_scores(ar, am, **kw) == want
    assert ctx.map_scores(ar, None, **kw) == oracle.mapsc(r, None, **kw)


def test_device_entry(ctx, pair):
    import torch
    r, m = pair
    kw = dict(cols=("count", "sum", "kth", "min_element"), criterion=("range", 11), kth="0.9", prec=9)
    want = check(ctx, r, m, **kw)
    blob = r[:-1] + m                                          # the reference without its final newline
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    k = ctx.map_scores_device(dev.data_ptr(), [0, len(r) - 1, len(blob)], **kw)
    assert k == len(want) and ctx.output_device_ptr() != 0 and ctx._output() == want
    k = ctx.map_scores_device(dev.data_ptr(), [0, len(r) - 1], **kw)      # the reference as its own map
    assert ctx._output() == oracle.mapsc(r, None, **kw) and k == len(ctx._output())
    k = ctx.map_scores_device(dev.data_ptr(), [0, len(r) - 1, len(r) - 1], **kw)      # an empty map
    assert ctx._output() == oracle.mapsc(r, b"", **kw)


def test_command(ctx, pair, tmp_path):
    r, m = pair
    fr, fm, fs = tmp_path / "ref.bed", tmp_path / "map.bed", tmp_path / "map.starch"
    fr.write_bytes(r)
    fm.write_bytes(m)
    fs.write_bytes(ctx.compress(m))

    def run(args, **kw):
        return subprocess.run([MAPSC] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)
    p = run([str(fr), str(fm)])
    assert p.returncode == 0 and p.stdout == oracle.mapsc(r, m)                      # --echo --mean
    p = run(["--mean", str(fr), str(fm)])
    assert p.returncode == 0 and p.stdout == oracle.mapsc(r, m, cols=("mean",))
    want = oracle.mapsc(r, m, cols=("count", "sum", "median", "kth", "max_element"), criterion=("fraction_map", ".5"), kth="0.25",
                        prec=2, skip_unmapped=True, delim=b"\t")
    p = run(["--count", "--sum", "--median", "--kth", "0.25", "--max-element", "--fraction-map", ".5", "--prec", "2",
             "--skip-unmapped", "--delim", "\t", "-", str(fs)], input=r)
    assert p.returncode == 0 and p.stdout == want
    p = run(["--exact", "--indicator", "--min", "--max", "--min-element", "--prec", "0", str(fm)])
    assert p.returncode == 0 and p.stdout == oracle.mapsc(m, None, cols=("indicator", "min", "max", "min_element"),
                                                          criterion=("exact",), prec=0)
    fu = tmp_path / "unsorted.bed"
    fu.write_bytes(b"chr1\t5\t6\tx\t1\nchr1\t1\t2\tx\t1\n")
    p = run(["--count", str(fr), str(fu)])
    assert p.returncode == 22 and p.stdout == b"" and b"bedmap-scores: input 1, line 2:" in p.stderr
    fn = tmp_path / "noscore.bed"
    fn.write_bytes(b"chr1\t0\t1000000\tx\t1e3\n")
    p = run(["--sum", str(fr), str(fn)])
    assert p.returncode == 22 and p.stdout == b"" and b"bedmap-scores: input 1, line 1:" in p.stderr
    p = run(["--count", str(fr), str(fn)])
    assert p.returncode == 0 and p.stdout == oracle.mapsc(r, fn.read_bytes(), cols=("count",))


def test_counts_agree_with_the_sibling_commands(ctx, pair):
    r, m = pair
    cols = ("echo", "count", "indicator")
    assert ctx.map_scores(r, m, cols=("count",)) == ctx.map_elements(r, m, cols=("count",)) == ctx.bedmap(r, m, cols=("count",))
    for n in (0, 1, 25):
        assert ctx.map_scores(r, m, cols=cols, criterion=("range", n)) == ctx.map_elements(r, m, cols=cols, criterion=("range", n)) \
            == ctx.bedmap(r, m, cols=cols, range=n)
    for crit in CRITS:
        assert ctx.map_scores(r, m, cols=cols, criterion=crit, skip_unmapped=True) == \
            ctx.map_elements(r, m, cols=cols, criterion=crit, skip_unmapped=True)
    assert ctx.map_scores(r, cols=("count",), skip_unmapped=True) == ctx.bedmap(r, cols=("count",), skip_unmapped=True)
