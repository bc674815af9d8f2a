"""GPU: closest-features (Starch.closest_features, closest_device, the
closest-features command).

Every comparison is equality of whole outputs against tests/closest_oracle.py or
literal bytes.  T is the number of reference lines per query workgroup, F the
fan-out of the hierarchy of maxima over the query stops.
"""
import itertools
import os
import random
import subprocess

import pytest

from tests import closest_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSEST = os.path.join(ROOT, "starch_amd", "_build", "closest-features")
FLAGS = ("closest", "dist", "no_overlaps", "no_ref")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def TF():
    import starch_amd
    return starch_amd.closest_constants()


def bed(rows, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % ((chrom,) + tuple(r) if len(r) == 2 else tuple(r)) for r in rows)


def check(ctx, ref, query, **kw):
    got = ctx.closest_features(ref, query, **kw)
    assert got == oracle.closest(ref, query, **kw), kw
    return got


def check_modes(ctx, ref, query):
    """Both searches on each side: default and no_overlaps, with the distances."""
    check(ctx, ref, query, dist=True)
    check(ctx, ref, query, dist=True, no_overlaps=True)


def random_bed(rng, chroms, lines, limit=300, lengths=(1, 2, 7, 40, 200)):
    rows = []
    for _ in range(lines):
        s = rng.randrange(0, limit - 2)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths)))))
    return bed(sorted(rows))


# ---- 1. table and shapes ---------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_hand_written_table(ctx, case):
    ref, query, kw, want = oracle.TABLE[case]
    assert ctx.closest_features(ref, query, **kw) == want


def test_shapes(ctx):
    a, q = bed([(1, 5), (9, 12)]), bed([(4, 10), (20, 30)])
    assert ctx.closest_features(b"", q, dist=True) == b""
    s = ctx.closest_stats()
    assert (s["n_ref"], s["n_query"], s["lines_out"], s["output_bytes"]) == (0, 2, 0, 0)
    assert ctx.closest_features(a, b"", dist=True) == b"chr1\t1\t5|NA|NA|NA|NA\nchr1\t9\t12|NA|NA|NA|NA\n"
    assert ctx.closest_features(b"", b"") == b""
    assert ctx.closest_features(a, q) == b"chr1\t1\t5|NA|chr1\t4\t10\nchr1\t9\t12|chr1\t4\t10|chr1\t20\t30\n"
    # a last line without '\n', in either input: the inputs must not fuse
    want = oracle.closest(a, q, dist=True)
    assert ctx.closest_features(a[:-1], q, dist=True) == ctx.closest_features(a, q[:-1], dist=True) == want
    assert ctx.closest_features(a[:-1], q[:-1], dist=True) == want
    # extra columns are echoed verbatim from both inputs, empty and space-holding fields too
    wide_r = b"chr1\t1\t5\tname\t0\t+\nchr1\t9\t12\t\t\nchr2\t3\t4\tx y  z\t\n"
    wide_q = b"chr1\t2\t3\t\t\t.\nchr1\t30\t40\ta b\t\nchr2\t1\t2\t  \n"
    assert ctx.closest_features(wide_r, wide_q, dist=True) == \
        b"chr1\t1\t5\tname\t0\t+|NA|NA|chr1\t2\t3\t\t\t.|0\n" \
        b"chr1\t9\t12\t\t|chr1\t2\t3\t\t\t.|-7|chr1\t30\t40\ta b\t|19\n" \
        b"chr2\t3\t4\tx y  z\t|chr2\t1\t2\t  |-2|NA|NA\n"
    check_modes(ctx, wide_r, wide_q)
    check_modes(ctx, wide_q, wide_r)
    # lines long enough for the whole-wave copy, among short ones, as reference, left and right element
    tail = bytes(range(48, 123)) * 9
    long_q = b"chr1\t9\t12\t" + tail + b"\n" + b"chr1\t10\t13\tshort\n" + b"chr1\t50\t60\t" + tail[::-1] + b"\n"
    long_r = bed([(1, 5)]) + b"chr1\t20\t30\t" + tail + b"\n" + bed([(31, 40), (70, 80)])
    for kw in (dict(dist=True), dict(dist=True, no_overlaps=True), dict(closest=True), dict(no_ref=True)):
        check(ctx, long_r, long_q, **kw)
        check(ctx, long_q, long_q, **kw)
    check(ctx, a, q, dist=True, delim=b"\t")
    check(ctx, a, q, dist=True, delim=b"<=delim>")                       # 8 bytes


def test_lines_left_to_the_wave(ctx):
    import starch_amd
    from tests import wave_lines
    W = starch_amd.sort_constants()[1]
    # long reference lines and right elements at lanes 0 and 63 of the first wave and lane 0 of the
    # third (the left elements one lane on), then no long line at all
    for r, q in wave_lines.wave_pairs(W):
        for kw in (dict(dist=True), dict(dist=True, delim=b"<=>"), dict(closest=True, delim=b"<=>"), dict(no_ref=True)):
            check(ctx, r, q, **kw)


def test_every_combination_of_the_flags(ctx):
    rng = random.Random(1)
    r = random_bed(rng, [b"chr1", b"chr2"], 400)
    q = random_bed(rng, [b"chr1", b"chr2", b"chr3"], 500)
    for bits in itertools.product((False, True), repeat=4):
        check(ctx, r, q, **dict(zip(FLAGS, bits)))


def test_stats(ctx):
    rng = random.Random(2)
    r = random_bed(rng, [b"chr1", b"chr2", b"chr4"], 500)
    q = random_bed(rng, [b"chr1", b"chr3"], 300, lengths=(1, 2, 7))
    for no_overlaps in (False, True):
        for closest in (False, True):
            got = check(ctx, r, q, dist=True, no_overlaps=no_overlaps, closest=closest)
            s = ctx.closest_stats()
            assert (s["n_ref"], s["n_query"], s["n_chromosomes"]) == (500, 300, 4)
            assert s["lines_out"] == 500 == got.count(b"\n") and s["output_bytes"] == len(got)
            sides = oracle.sides(r, q, no_overlaps)
            assert s["left_na"] == sum(lt is None for lt, _ in sides) > 0
            assert s["right_na"] == sum(rt is None for _, rt in sides) > 0
            assert s["stops_sorted"] in (0, 1)
            assert all(s[k] >= 0 for k in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_format")) and s["ms_total"] > 0


# ---- 2. reference tiles --------------------------------------------------------------------
def test_tile_sizes(ctx, TF):
    T = TF[0]
    rng = random.Random(3)
    q = random_bed(rng, [b"chr1"], 900, limit=4000)
    for n in (T - 1, T, T + 1, 3 * T + 137):
        check_modes(ctx, random_bed(rng, [b"chr1"], n, limit=4000), q)
        assert ctx.closest_stats()["n_ref"] == n


def test_chromosome_change_at_and_inside_a_tile(ctx, TF):
    T = TF[0]
    rng = random.Random(4)
    q = random_bed(rng, [b"chr1", b"chr2", b"chr3", b"chr4"], 1200, limit=2000)
    for n1 in (T, T // 2 + 3, T - 1):                    # the change at a tile boundary, inside a tile, one line before
        r = random_bed(rng, [b"chr1"], n1, limit=2000) + random_bed(rng, [b"chr2"], T + 9, limit=2000)
        check_modes(ctx, r, q)
    one = bed([(1000, 1200)], b"chr2")
    check_modes(ctx, random_bed(rng, [b"chr1"], T - 1, limit=2000) + one + random_bed(rng, [b"chr3"], T + 5, limit=2000), q)


# ---- 3. the hierarchy ---------------------------------------------------------------------------
def test_one_long_line_ahead_of_short_ones(ctx, TF):
    F = TF[1]
    for n in (F - 1, F, F + 1, F * F - 1, F * F, F * F + 1, F * F * F + 1):
        short = [(10 + 4 * i, 12 + 4 * i) for i in range(n)]             # disjoint, gaps of 2
        big = 4 * n + 100
        q = bed([(0, big)] + short)
        # in the gaps the only overlapping left candidate is the first line; on a short line it is that line
        # or the one before; past `big` the largest stop is the first line's again
        pos = sorted(set([10, 11, 12, 13, 14, big - 1, big, big + 5] +
                         [10 + 4 * i + d for i in (0, 1, F - 2, F - 1, F, F + 1, n // 2, n - 2, n - 1) if 0 <= i < n
                          for d in (0, 1, 2, 3)]))
        r = bed(sorted([(p, p + 1) for p in pos] + [(12, big + 9)]))
        got = check(ctx, r, q, dist=True)
        assert ctx.closest_stats()["stops_sorted"] == 1
        assert b"chr1\t12\t13|chr1\t0\t%d|0|" % big in got               # a gap: the long line, through every level
        check(ctx, r, q, dist=True, no_overlaps=True)
        assert ctx.closest_stats()["stops_sorted"] == 1
        check(ctx, r, q, closest=True)


def test_answer_at_every_place_of_a_tile(ctx, TF):
    F = TF[1]
    n = 3 * F * F + 5
    # stops fall from line to line, so that nothing overlaps a late reference line but the one line made long
    for k in (0, 1, F - 1, F, F + F // 2, 2 * F - 1, F * F - 1, F * F, F * F + F // 2, n - 1):
        rows = [(i, 5 * n + 1 - i) for i in range(n)]                    # nested: every stop below the one before
        rows[k] = (k, 9 * n)
        q = bed(rows)
        r = bed([(n + 3, 7 * n), (6 * n, 6 * n + 1), (9 * n, 9 * n + 2)])
        got = check(ctx, r, q, dist=True)
        assert b"chr1\t%d\t%d|chr1\t%d\t%d|0|NA|NA\n" % (6 * n, 6 * n + 1, k, 9 * n) in got
        check(ctx, r, q, dist=True, no_overlaps=True)
    # no stop reaches the reference line: the last of the lines with the largest stop, wherever it lies
    for k in (0, F - 1, F, 2 * F + 1, F * F, n - 1):
        rows = [(i, n + 1) for i in range(n)]
        for j in range(0, k + 1, max(1, k // 3)):
            rows[j] = (j, n + 2)
        rows[k] = (k, n + 2)
        r = bed([(2 * n, 2 * n + 1)])
        got = check(ctx, r, bed(rows), dist=True)
        assert got == b"chr1\t%d\t%d|chr1\t%d\t%d|%d|NA|NA\n" % (2 * n, 2 * n + 1, k, n + 2, -(n - 1))
        check(ctx, r, bed(rows), dist=True, no_overlaps=True)


def test_a_chromosome_before_shares_the_tile(ctx, TF):
    F = TF[1]
    # chr1's stops are far above chr2's: a tile of maxima that spans both must not answer for chr2
    for n1 in (1, F - 1, F, F + 1, F * F + 3):
        q = bed([(i, 10 ** 9 + i) for i in range(n1)], b"chr1") + bed([(5 * i, 5 * i + 2) for i in range(2 * F + 3)], b"chr2")
        r = bed([(3, 4), (8, 9), (5 * F + 1, 5 * F + 2), (5 * F + 3, 5 * F + 4), (10 ** 6, 10 ** 6 + 1)], b"chr2")
        check_modes(ctx, r, q)
        check_modes(ctx, bed([(1, 10 ** 9 + 7)], b"chr1") + r, q)


# ---- 4. ties ------------------------------------------------------------------------------------------
def test_ties(ctx):
    r = bed([(100, 200)])
    flat = bed([(10, 90), (20, 90), (30, 90), (210, 250), (210, 260), (210, 270)])       # equal stops, not nested
    nested = bed([(5, 95), (10, 90), (20, 90), (30, 90), (40, 60)])                      # equal stops under a longer line
    for q in (flat, nested):
        check_modes(ctx, r, q)
        check(ctx, r, q, closest=True, dist=True)
    assert ctx.closest_features(r, flat, dist=True) == b"chr1\t100\t200|chr1\t30\t90|-11|chr1\t210\t250|11\n"
    assert ctx.closest_features(r, nested, dist=True, no_overlaps=True) == b"chr1\t100\t200|chr1\t5\t95|-6|NA|NA\n"
    # equal stops, the earlier line is the longer: the last one still wins
    q = bed([(10, 90), (50, 90), (60, 70)])
    assert ctx.closest_features(r, q, dist=True, no_overlaps=True) == b"chr1\t100\t200|chr1\t50\t90|-11|NA|NA\n"
    assert ctx.closest_features(r, q, dist=True) == b"chr1\t100\t200|chr1\t50\t90|-11|NA|NA\n"
    # duplicated query lines carry a fourth column that tells them apart
    dup = b"chr1\t10\t90\ta\nchr1\t10\t90\tb\nchr1\t150\t160\tc\nchr1\t150\t160\td\nchr1\t300\t400\te\nchr1\t300\t400\tf\n"
    assert ctx.closest_features(r, dup, no_overlaps=True) == b"chr1\t100\t200|chr1\t10\t90\tb|chr1\t300\t400\te\n"
    assert ctx.closest_features(r, dup) == b"chr1\t100\t200|chr1\t10\t90\tb|chr1\t150\t160\tc\n"
    dup2 = b"chr1\t50\t150\ta\nchr1\t50\t150\tb\nchr1\t60\t120\tc\n"
    assert ctx.closest_features(r, dup2, dist=True) == b"chr1\t100\t200|chr1\t60\t120\tc|0|NA|NA\n"
    check_modes(ctx, r, dup)
    check_modes(ctx, r, dup2)
    # query lines equal to the reference line are right candidates
    eq = b"chr1\t90\t100\tx\nchr1\t100\t200\ty\nchr1\t100\t200\tz\nchr1\t200\t210\tw\n"
    assert ctx.closest_features(r, eq, dist=True) == b"chr1\t100\t200|chr1\t90\t100\tx|-1|chr1\t100\t200\ty|0\n"
    assert ctx.closest_features(r, eq, dist=True, no_overlaps=True) == b"chr1\t100\t200|chr1\t90\t100\tx|-1|chr1\t200\t210\tw|1\n"
    # equal starts with different stops around (s, e)
    around = bed([(100, 101), (100, 199), (100, 200), (100, 201), (100, 900)])
    assert ctx.closest_features(r, around, dist=True) == b"chr1\t100\t200|chr1\t100\t199|0|chr1\t100\t200|0\n"
    check_modes(ctx, r, around)
    check_modes(ctx, bed([(100, 150), (100, 200), (100, 201), (100, 950)]), around)


# ---- 5. chromosomes -----------------------------------------------------------------------------------------
def test_chromosomes(ctx):
    rng = random.Random(6)
    # query chromosomes the reference lacks before, between and after; reference chromosomes the query lacks
    r = random_bed(rng, [b"chr10", b"chr2", b"chr4", b"chrM"], 600)
    q = random_bed(rng, [b"chr1", b"chr10", b"chr2", b"chr20", b"chr3", b"chr4", b"chrX", b"chrY"], 900)
    got = check(ctx, r, q, dist=True)
    assert b"|NA|NA|NA|NA\n" in got and ctx.closest_stats()["n_chromosomes"] == 9
    check(ctx, r, q, dist=True, no_overlaps=True)
    check_modes(ctx, q, r)
    names = [b"c", b"ch", b"chr", b"chr1", b"chr11", b"chr1_x"]       # prefixes of each other
    check_modes(ctx, random_bed(rng, names, 300), random_bed(rng, names[::2], 300))
    check_modes(ctx, random_bed(rng, names[1::2], 300), random_bed(rng, names, 300))
    # the first and last reference line of a chromosome with all candidates on one side
    q2 = bed([(100, 110), (120, 130), (140, 150)], b"chr1") + bed([(100, 110), (120, 130)], b"chr2")
    r2 = bed([(1, 2), (500, 600)], b"chr1") + bed([(1, 100), (130, 131)], b"chr2")
    assert ctx.closest_features(r2, q2, dist=True) == \
        b"chr1\t1\t2|NA|NA|chr1\t100\t110|99\nchr1\t500\t600|chr1\t140\t150|-351|NA|NA\n" \
        b"chr2\t1\t100|NA|NA|chr2\t100\t110|1\nchr2\t130\t131|chr2\t120\t130|-1|NA|NA\n"
    check_modes(ctx, r2, q2)


# ---- 6. wide coordinates ------------------------------------------------------------------------------------------
def test_wide_coordinates(ctx):
    rng = random.Random(8)
    base = 2 ** 62
    q = bed(sorted((base + s, base + s + rng.choice((1, 30, 2000))) for s in (rng.randrange(0, 100000) for _ in range(900))))
    r = bed(sorted((base + s, base + s + rng.choice((1, 300, 50000))) for s in (rng.randrange(0, 100000) for _ in range(300))))
    check_modes(ctx, r, q)
    top = 2 ** 63 - 1
    assert ctx.closest_features(bed([(top - 1, top)]), bed([(0, 1)]), dist=True) == \
        b"chr1\t%d\t%d|chr1\t0\t1|-%d|NA|NA\n" % (top - 1, top, top - 1)
    assert ctx.closest_features(bed([(0, 1)]), bed([(top - 1, top)]), dist=True, closest=True) == \
        b"chr1\t0\t1|chr1\t%d\t%d|%d\n" % (top - 1, top, top - 1)
    two = bed([(0, 2), (top - 2, top)])
    check_modes(ctx, bed([(2 ** 62, 2 ** 62 + 1)]), two)
    check(ctx, bed([(2 ** 62, 2 ** 62 + 1)]), two, dist=True, closest=True)
    check_modes(ctx, two, bed([(2 ** 62, 2 ** 62 + 1), (2 ** 62, top)]))


# ---- 7. random ------------------------------------------------------------------------------------------------------
def _random_flags(rng):
    return {k: rng.random() < 0.4 for k in FLAGS}


def test_random_dense_cases(ctx):
    names = [b"c", b"ch", b"chr", b"chr1"]
    for seed in range(300):
        rng = random.Random(5000 + seed)
        ref = random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(1, 80))
        query = random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(0, 80))
        kw = _random_flags(rng)
        assert ctx.closest_features(ref, query, **kw) == oracle.closest(ref, query, **kw), (seed, kw)


def test_random_wide_cases(ctx):
    for seed in range(40):
        rng = random.Random(6000 + seed)
        lim = rng.choice((5000, 10 ** 9, 2 ** 40))
        lens = (1, 7, lim // 50, lim // 3)
        ref = random_bed(rng, [b"chr1", b"chr2"], rng.randint(1, 200), limit=lim, lengths=lens)
        query = random_bed(rng, [b"chr1", b"chr2", b"chr3"], rng.randint(0, 200), limit=lim, lengths=lens)
        kw = _random_flags(rng)
        assert ctx.closest_features(ref, query, **kw) == oracle.closest(ref, query, **kw), (seed, kw)


# ---- 8. archives ------------------------------------------------------------------------------------------------------
def test_archives(ctx):
    import starch_amd
    rng = random.Random(9)
    r = random_bed(rng, [b"chr1", b"chr10", b"chr2"], 400)
    q = random_bed(rng, [b"chr1", b"chr2", b"chrX"], 300)
    ar, aq = ctx.compress(r), ctx.compress(q)
    assert ar[:4] == b"\xca\x5c\xad\x1a"
    want = check(ctx, r, q, dist=True)
    assert ctx.closest_features(ar, q, dist=True) == want
    assert ctx.closest_features(r, aq, dist=True) == want
    assert ctx.closest_features(ar, aq, dist=True) == want
    ctx.set_compression_method(starch_amd.K_GZIP)
    try:
        gz = ctx.compress(q)
    finally:
        ctx.set_compression_method(starch_amd.K_BZIP2)
    for pair in ((r, gz), (gz, r)):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.closest_features(*pair)
        assert e.value.code == -2 and "gzip" in str(e.value)
    assert ctx.closest_features(ar, aq, dist=True) == want


# ---- 9. errors ------------------------------------------------------------------------------------------------------------
def _refused(ctx, ref, query, code, *words):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.closest_features(ref, query, dist=True)
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    assert ctx.closest_features(bed([(1, 2)]), bed([(5, 6)]), dist=True) == b"chr1\t1\t2|NA|NA|chr1\t5\t6|4\n"   # works again


def test_errors(ctx):
    hi, lo = bed([(500, 600), (700, 800)]), bed([(1, 2), (3, 4), (2, 9), (0, 1)])
    _refused(ctx, lo, hi, -12, "closest-features: input 0, line 3:", "sort-bed")           # unsorted reference
    _refused(ctx, hi, lo, -12, "closest-features: input 1, line 3:", "sort-bed")           # unsorted query
    _refused(ctx, bed([(1, 2)], b"chr2") + bed([(1, 2)], b"chr10"), hi, -12, "input 0, line 2:", "sort-bed")
    _refused(ctx, hi, bed([(1, 2), (5, 5)]), -12, "input 1, line 2:", "stop")
    _refused(ctx, bed([(1, 2), (9, 7)]), hi, -12, "input 0, line 2:", "stop")
    # a malformed line in the query goes ahead of an order error in the reference
    _refused(ctx, lo, b"chr1\t1\t2\nchr1\t5\n", -12, "input 1, line 2:", "fewer than three")
    _refused(ctx, b"chr1\t1\t2\n\nchr1\t5\t6\n", hi, -12, "input 0, line 2:", "empty line")
    _refused(ctx, b"", b"chr1\t1\tx\n", -12, "input 1, line 1:", "stop")                    # checked though nothing refers to it


def test_argument_errors(ctx):
    import ctypes
    import starch_amd
    a = bed([(1, 2)])
    for kw in (dict(delim=b""), dict(delim=b"123456789")):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.closest_features(a, a, **kw)
        assert e.value.code == -2, kw
    L = starch_amd.load()
    one, opt = starch_amd.SetopInput(a, len(a)), starch_amd.ClosestOptions()
    opt.delim_len, opt.delim = 1, b"|"
    for flag in FLAGS:
        setattr(opt, flag, 2)                                  # a flag other than 0 or 1
        assert L.starch_closest_host(ctx._h, ctypes.byref(one), ctypes.byref(one), ctypes.byref(opt)) == -2, flag
        setattr(opt, flag, 0)
    assert L.starch_closest_host(ctx._h, ctypes.byref(one), ctypes.byref(one), None) == -2
    assert L.starch_closest_host(ctx._h, None, ctypes.byref(one), ctypes.byref(opt)) == -2
    assert L.starch_closest_host(ctx._h, ctypes.byref(one), None, ctypes.byref(opt)) == -2
    assert L.starch_closest_device(ctx._h, None, None, ctypes.byref(opt)) == -2
    offs = (ctypes.c_uint64 * 3)(0, 5, 3)                     # decreasing
    assert L.starch_closest_device(ctx._h, None, offs, ctypes.byref(opt)) == -2
    assert L.starch_closest_host(ctx._h, ctypes.byref(one), ctypes.byref(one), ctypes.byref(opt)) == 0
    assert ctx._output() == b"chr1\t1\t2|NA|chr1\t1\t2\n"


# ---- 10. device entry and chaining ------------------------------------------------------------------------------------------
def test_device_entry_and_chaining(ctx):
    import torch
    rng = random.Random(10)
    r = random_bed(rng, [b"chr1", b"chr2"], 700)
    q = random_bed(rng, [b"chr1", b"chr2", b"chr3"], 900)
    want = check(ctx, r, q, dist=True)
    blob = r[:-1] + q                                          # the reference without its final newline
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    k = ctx.closest_device(dev.data_ptr(), [0, len(r) - 1, len(blob)], dist=True)
    assert k == len(want) and ctx.output_device_ptr() != 0 and ctx._output() == want
    k = ctx.closest_device(dev.data_ptr(), [0, len(r) - 1, len(r) - 1], dist=True)      # an empty query
    assert ctx._output() == oracle.closest(r, b"", dist=True) and k == len(ctx._output())
    # bytes left in HBM by sort_bed serve as reference and as query
    rows = q.split(b"\n")[:-1]
    rng.shuffle(rows)
    shuffled = torch.frombuffer(bytearray(b"\n".join(rows) + b"\n"), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    n = ctx.sort_bed_device(shuffled.data_ptr(), shuffled.numel())
    assert n == len(q)
    ctx.closest_device(ctx.output_device_ptr(), [0, n, n], closest=True)
    assert ctx._output() == oracle.closest(q, b"", closest=True)
    both = torch.frombuffer(bytearray(q + q), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    ctx.closest_device(both.data_ptr(), [0, n, 2 * n], dist=True, no_overlaps=True)
    assert ctx._output() == oracle.closest(q, q, dist=True, no_overlaps=True)
    with pytest.raises(ValueError):
        ctx.closest_device(dev.data_ptr(), [0, len(blob)])


# ---- 11. command ---------------------------------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_command(ctx, tmp_path):
    rng = random.Random(11)
    r = random_bed(rng, [b"chr1", b"chr2"], 500)
    q = random_bed(rng, [b"chr1", b"chr3"], 400)
    fr, fq, fs = tmp_path / "ref.bed", tmp_path / "query.bed", tmp_path / "query.starch"
    fr.write_bytes(r)
    fq.write_bytes(q)
    fs.write_bytes(ctx.compress(q))
    want = oracle.closest(r, q, dist=True, closest=True)
    p = _run([CLOSEST, "--dist", "--closest", str(fr), str(fq)])
    assert p.returncode == 0 and p.stdout == want
    p = _run([CLOSEST, "--shortest", "--dist", str(fr), str(fs)])
    assert p.returncode == 0 and p.stdout == want
    p = _run([CLOSEST, "--dist", "--closest", "-", str(fq)], input=r)
    assert p.returncode == 0 and p.stdout == want
    p = _run([CLOSEST, "--no-overlaps", "--no-ref", "--delim", "\t", str(fr), str(fq)])
    assert p.returncode == 0 and p.stdout == oracle.closest(r, q, no_overlaps=True, no_ref=True, delim=b"\t")
    fu = tmp_path / "unsorted.bed"
    fu.write_bytes(bed([(5, 6), (1, 2)]))
    p = _run([CLOSEST, "--dist", str(fr), str(fu)])
    assert p.returncode == 22 and p.stdout == b"" and b"closest-features: input 1, line 2:" in p.stderr
