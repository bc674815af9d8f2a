"""GPU: bedops' element-of, not-element-of, partition, chop and everything
(Starch.bedops and its wrappers, starch_bedops_device, the bedops command).

Every comparison is equality of whole outputs against tests/bedops2_oracle.py:
the bitmap oracle where the coordinates are below 4096, the integer oracle
otherwise.  R is the number of runs per tile of element-of's range maximum, X
the number of pieces per workgroup of chop's expansion.
"""
import ctypes
import os
import random
import subprocess
import time

import pytest

from tests import bedops2_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEDOPS = os.path.join(ROOT, "starch_amd", "_build", "bedops")
OPS = oracle.OPS
THRESHOLDS = (1, 7, "1%", "50%", "100%")
CHOPS = ((1, 1, False), (5, 5, False), (5, 2, False), (5, 9, True), (4096, 4096, False))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def RX():
    import starch_amd
    return starch_amd.bedops_constants()


def bed(rows, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % ((chrom,) + tuple(r) if len(r) == 2 else tuple(r)) for r in rows)


def call(ctx, op, inputs, threshold="100%", width=1, stagger=None, exclude_short=False):
    return ctx.bedops(op, inputs, threshold=threshold, chop=width, stagger=stagger, exclude_short=exclude_short)


def variants(op):
    """keyword sets that exercise op"""
    if "element" in op:
        return [{"threshold": t} for t in THRESHOLDS]
    if op == "chop":
        return [{"width": w, "stagger": g, "exclude_short": x} for w, g, x in CHOPS]
    return [{}]


def check(ctx, inputs, ref, ops=OPS):
    for op in ops:
        for kw in variants(op):
            assert call(ctx, op, inputs, **kw) == ref(op, inputs, **kw), (op, kw)


def _random_input(rng, chroms, lines, tag, limit=4096, lengths=(1, 2, 7, 40, 600)):
    rows = []
    for _ in range(lines):
        s = rng.randrange(0, limit - 2)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit - 1, s + rng.choice(lengths)))))
    rows.sort()
    return b"".join(b"%s\t%d\t%d\t%s%d\n" % (r + (tag, n)) for n, r in enumerate(rows))


# ---- 1. hand tables and shapes ----------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_hand_written_table(ctx, case):
    op, inputs, kw, want = oracle.TABLE[case]
    assert call(ctx, op, inputs, **kw) == want


def test_shapes(ctx):
    a, c = bed([(1, 5), (9, 12)]), bed([(4, 10), (20, 30)])
    for op in OPS:
        assert call(ctx, op, [b"", b""]) == b"", op
    check(ctx, [a, b"", c], oracle.bitmap)                  # empty inputs among three
    check(ctx, [b"", a, c], oracle.bitmap)
    check(ctx, [a, c, b""], oracle.bitmap)
    assert ctx.element_of(b"", a, c) == b"" and ctx.not_element_of(a, b"", b"") == a
    # no final newline, then another input: the two lines must not fuse, and the echo gets its newline
    open_end = b"chr1\t1\t5\tp\nchr1\t9\t12\tq"
    check(ctx, [open_end, c], oracle.bitmap)
    check(ctx, [c, open_end], oracle.bitmap)
    assert ctx.everything(open_end, c) == b"chr1\t1\t5\tp\nchr1\t4\t10\nchr1\t9\t12\tq\nchr1\t20\t30\n"
    assert ctx.element_of(open_end, c, threshold=1) == b"chr1\t1\t5\tp\nchr1\t9\t12\tq\n"
    # extra columns: kept by -e, -n and -u, ignored by -p and -w
    wide = b"chr1\t1\t5\tname\t0\t+\nchr1\t9\t12\t\t\nchr2\t3\t4\tx y z\n"
    check(ctx, [wide, c], oracle.bitmap)
    assert ctx.element_of(wide, c, threshold=1) == b"chr1\t1\t5\tname\t0\t+\nchr1\t9\t12\t\t\n"
    assert ctx.not_element_of(wide, c, threshold=1) == b"chr2\t3\t4\tx y z\n"
    assert ctx.everything(wide) == wide
    assert ctx.partition(wide) == bed([(1, 5), (9, 12)]) + bed([(3, 4)], b"chr2")
    assert ctx.chop(wide, width=3) == bed([(1, 4), (4, 5), (9, 12)]) + bed([(3, 4)], b"chr2")
    # one chromosome ends at the position where the next starts
    two = bed([(0, 10), (5, 20)]) + bed([(20, 30), (25, 40)], b"chr2")
    other = bed([(15, 20)]) + bed([(20, 22)], b"chr2")
    check(ctx, [two, other], oracle.bitmap)
    assert ctx.partition(two) == bed([(0, 5), (5, 10), (10, 20)]) + bed([(20, 25), (25, 30), (30, 40)], b"chr2")
    assert ctx.chop(two, width=100) == bed([(0, 20)]) + bed([(20, 40)], b"chr2")
    # stats of the last call
    got = ctx.partition(a, wide, c)
    s = ctx.setop_stats()
    assert s["lines_out"] == got.count(b"\n") and s["output_bytes"] == len(got)
    assert s["n_inputs"] == 3 and s["n_lines"] == 7 and s["n_chromosomes"] == 2 and s["runs_merged"] == 0
    with pytest.raises(ValueError):
        ctx.setop("union", [a])
    with pytest.raises(ValueError):
        ctx.bedops("union", [a])


# ---- 2. random inputs against the bitmap oracle ---------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_random_cases(ctx, seed):
    rng = random.Random(2000 + seed)
    chroms = [b"chr1", b"chr10", b"chr2"]
    inputs = [_random_input(rng, chroms, rng.randint(500, 2000), b"i%d." % k,
                            lengths=((1, 2, 7), (1, 2, 7, 40), (1, 7, 40, 600))[seed]) for k in range(3)]
    check(ctx, inputs, oracle.bitmap)
    for t in THRESHOLDS:     # -e plus -n is input 0
        e, n = ctx.element_of(*inputs, threshold=t), ctx.not_element_of(*inputs, threshold=t)
        assert sorted((e + n).split(b"\n")) == sorted(inputs[0].split(b"\n")), t


# ---- 3. element-of: the range query ----------------------------------------------------------------
def _spanned(R, long_at=None, long_len=9):
    """3R+137 runs of 3 bases, 10 apart, from 100 on; run long_at has long_len bases instead"""
    n = 3 * R + 137
    rows = [(100 + 10 * i, 100 + 10 * i + (long_len if i == long_at else 3)) for i in range(n)]
    return rows, n


def test_element_of_range_maximum(ctx, RX):
    R = RX[0]
    n = 3 * R + 137
    # the line starts inside run 0 (2 of its 3 bases) and ends inside the last run (1 base)
    ref = b"chr1\t101\t%d\tspan\n" % (100 + 10 * (n - 1) + 1)
    decoy = bed([(0, 10 ** 6)], b"chr10")                 # overlapping coordinates on another chromosome
    for long_at in (R + R // 2, 2 * R, 2 * R - 1, R, R - 1, n - 2, 1):   # middle, first and last of a tile
        rows, _ = _spanned(R, long_at)
        others = [bed(rows), decoy]
        for t, want in ((9, ref), (10, b""), (4, ref), (3, ref)):
            assert ctx.element_of(ref, *others, threshold=t) == want == oracle.integers("element_of", [ref] + others,
                                                                                         threshold=t), (long_at, t)
        assert ctx.not_element_of(ref, *others, threshold=10) == ref
    # only a partial edge run qualifies: the first run is long, the line takes 6 of its bases
    rows, _ = _spanned(R)
    rows[0] = (90, 107)
    assert ctx.element_of(ref, bed(rows), threshold=6) == ref
    assert ctx.element_of(ref, bed(rows), threshold=7) == b""
    rows, _ = _spanned(R)
    rows[-1] = (rows[-1][0], rows[-1][0] + 50)             # the last run: 1 base inside the line
    assert ctx.element_of(ref, bed(rows), threshold=4) == b""
    assert ctx.element_of(ref, bed(rows), threshold=3) == ref
    # no run qualifies by one base
    rows, _ = _spanned(R)
    assert ctx.element_of(ref, bed(rows), threshold=4) == b"" and ctx.element_of(ref, bed(rows), threshold=3) == ref
    # percent: ov * 100 == p * len exactly, and one base short
    length = 25 * 20                                       # a line of 500 bases, a middle run of 20: 4%
    line = b"chr1\t100\t%d\n" % (100 + length)
    rows = [(100 + 10 * i, 100 + 10 * i + 3) for i in range(length // 10) if i not in (18, 19)]
    rows[17] = (270, 290)
    u = bed(rows)
    assert oracle.integers("element_of", [line, u], threshold="4%") == line
    assert ctx.element_of(line, u, threshold="4%") == line
    rows[17] = (270, 289)
    assert ctx.element_of(line, bed(rows), threshold="4%") == b""
    assert ctx.not_element_of(line, bed(rows), threshold="4%") == line
    many_ref, many_u = ref, bed(_spanned(R, 2 * R, 9)[0])
    span = int(ref.split(b"\t")[2]) - 101
    assert span * 1 > 900                                  # 9 bases are below 1% of the line
    assert ctx.element_of(many_ref, many_u, threshold="1%") == b"" == oracle.integers("element_of", [many_ref, many_u],
                                                                                      threshold="1%")


@pytest.mark.parametrize("p", (1, 3))
def test_element_of_percent_boundary_on_the_spanning_line(ctx, RX, p):
    """The line that spans 3R+137 runs, 100*m bases long: a run of m*p bases
    that lies between its two edge runs, so in a whole tile of the range
    maximum, is exactly p percent of it; one base less is not."""
    R = RX[0]
    n = 3 * R + 137
    m = (10 * n) // (100 - p) + 2                          # 100*m bases hold n runs 10 apart with one of them m*p long
    for long_at in (R + R // 2, 2 * R, 2 * R - 1):          # middle, first and last run of a tile
        for short in (0, 1):
            rows, cur = [], 100
            for i in range(n):
                length = m * p - short if i == long_at else 3
                rows.append((cur, cur + length))
                cur += length + 7
            start = rows[0][0] + 1                         # 2 bases of the first run
            ref = b"chr1\t%d\t%d\tspan\n" % (start, start + 100 * m)
            assert start + 100 * m > rows[-1][1] and m * p > 3
            u = [bed(rows), bed([(0, 10 ** 7)], b"chr10")]
            t = "%d%%" % p
            e, ne = ctx.element_of(ref, *u, threshold=t), ctx.not_element_of(ref, *u, threshold=t)
            assert e == oracle.integers("element_of", [ref] + u, threshold=t), (long_at, short)
            assert ne == oracle.integers("not_element_of", [ref] + u, threshold=t), (long_at, short)
            assert (e, ne) == ((b"", ref) if short else (ref, b"")), (long_at, short)
            # the same boundary in bases
            assert ctx.element_of(ref, *u, threshold=m * p) == (b"" if short else ref)
            assert ctx.element_of(ref, *u, threshold=m * p - 1) == ref


def test_element_of_near_2_63(ctx):
    top = 2 ** 63 - 1
    ref = b"chr1\t0\t%d\tall\n" % top
    same, shorter = bed([(0, top)]), bed([(0, top - 1)])
    assert ctx.element_of(ref, same) == ref
    assert ctx.element_of(ref, shorter) == b"" and ctx.not_element_of(ref, shorter) == ref
    assert ctx.element_of(ref, shorter, threshold="99%") == ref
    assert ctx.element_of(ref, shorter, threshold=top - 1) == ref and ctx.element_of(ref, shorter, threshold=top) == b""
    for t in ("100%", "99%", "1%", 1, top):
        for u in (same, shorter):
            assert ctx.element_of(ref, u, threshold=t) == oracle.integers("element_of", [ref, u], threshold=t)


def test_element_of_chromosomes_and_joined_runs(ctx):
    ref = bed([(100, 200)]) + bed([(100, 200)], b"chr10") + bed([(100, 200)], b"chr2")
    # a run on chr10 does not count for chr1
    u = bed([(0, 1000)], b"chr10")
    assert ctx.element_of(ref, u) == bed([(100, 200)], b"chr10")
    assert ctx.not_element_of(ref, u) == bed([(100, 200)]) + bed([(100, 200)], b"chr2")
    # abutting lines from two different inputs form one run; alone neither is enough
    left, right = bed([(90, 150)]) + bed([(100, 150)], b"chr2"), bed([(150, 210)]) + bed([(151, 200)], b"chr2")
    assert ctx.element_of(ref, left, right) == bed([(100, 200)])
    assert ctx.element_of(ref, right, left) == bed([(100, 200)])
    assert ctx.element_of(ref, left) == b"" and ctx.element_of(ref, right, threshold="50%") == bed([(100, 200)])
    check(ctx, [ref, left, right, u], oracle.bitmap, ops=("element_of", "not_element_of"))
    # the other inputs interleave, so merging them together needs their lines ordered first
    rng = random.Random(33)
    others = [_random_input(rng, [b"chr1", b"chr10", b"chr2"], 700, b"o") for _ in range(4)]
    big = _random_input(rng, [b"chr1", b"chr10", b"chr2", b"chr3"], 900, b"r", lengths=(40, 600))
    check(ctx, [big] + others, oracle.bitmap, ops=("element_of", "not_element_of"))


# ---- 4. partition ------------------------------------------------------------------------------------
def test_partition(ctx):
    dup = bed([(5, 9), (5, 9), (5, 9)])
    assert ctx.partition(dup) == bed([(5, 9)]) == ctx.partition(dup, dup, dup)      # one piece from three inputs
    nested = bed([(0, 100), (10, 90), (20, 80), (50, 60)])
    assert ctx.partition(nested) == bed([(0, 10), (10, 20), (20, 50), (50, 60), (60, 80), (80, 90), (90, 100)])
    abut = bed([(0, 10), (10, 20), (20, 30)])
    assert ctx.partition(abut) == abut and ctx.merge(abut) == bed([(0, 30)])
    gap = bed([(0, 10), (12, 20)])
    assert ctx.partition(gap, bed([(5, 8)])) == bed([(0, 5), (5, 8), (8, 10), (12, 20)])
    # more than 2 x 4096 ends, wide coordinates, several chromosomes
    rng = random.Random(44)
    rows = []
    for c in (b"chr1", b"chr2", b"chrX"):
        for _ in range(1700):
            s = rng.randrange(0, 10 ** 12)
            rows.append((c, s, s + rng.choice((1, 1000, 10 ** 9, 10 ** 11))))
    rows.sort()
    x = [bed(rows[0::2]), bed(rows[1::2])]
    assert 2 * len(rows) > 2 * 4096
    got = ctx.partition(*x)
    assert got == oracle.integers("partition", x)
    assert ctx.setop_stats()["groups"] > 4096
    assert ctx.merge(got) == ctx.merge(*x)
    assert ctx.sort_check(got) == 0
    small = [_random_input(rng, [b"chr1", b"chr2"], 900, b"s") for _ in range(2)]
    p = ctx.partition(*small)
    assert ctx.merge(p) == ctx.merge(*small) and ctx.sort_check(p) == 0


# ---- 5. chop -----------------------------------------------------------------------------------------
def test_chop_expansion_windows(ctx, RX):
    X = RX[1]
    w = 7
    long_run = (0, w * (3 * X + 5) - 3)                       # 3X+5 pieces, the last one short
    base = long_run[1] + 10
    ones = [(base + 10 * i, base + 10 * i + w) for i in range(2 * X)]
    first = bed([long_run] + ones)
    got = ctx.chop(first, width=w)
    assert got == oracle.integers("chop", [first], width=w)
    assert got.count(b"\n") == 3 * X + 5 + 2 * X == ctx.setop_stats()["lines_out"]
    shifted = [(10 * i, 10 * i + w) for i in range(2 * X)]
    off = 10 * 2 * X + 10
    last = bed(shifted + [(off, off + long_run[1])])
    assert ctx.chop(last, width=w) == oracle.integers("chop", [last], width=w)
    # with -x the short tail goes, and runs shorter than w leave no piece between the others
    mixed = bed([(0, 3), (10, 10 + 2 * w), (100, 104)] + [(200 + 10 * i, 203 + 10 * i) for i in range(2 * X)] +
                [(10 ** 6, 10 ** 6 + w * X + 1)])
    for x in (False, True):
        for g in (None, 3, 20):
            assert ctx.chop(mixed, width=w, stagger=g, exclude_short=x) == \
                oracle.integers("chop", [mixed], width=w, stagger=g, exclude_short=x), (x, g)
    assert ctx.chop(mixed, width=w, exclude_short=True).count(b"\n") == 2 + X


def test_chop_shapes(ctx):
    a = bed([(0, 4)])
    assert ctx.chop(a, width=10) == a and ctx.chop(a, width=10, exclude_short=True) == b""
    assert ctx.chop(a, width=4, exclude_short=True) == a
    b = bed([(0, 12)])
    assert ctx.chop(b, width=5, stagger=2) == bed([(0, 5), (2, 7), (4, 9), (6, 11), (8, 12), (10, 12)])   # g < w
    assert ctx.chop(b, width=2, stagger=5) == bed([(0, 2), (5, 7), (10, 12)])                             # g > w
    assert ctx.chop(b, width=2, stagger=50) == bed([(0, 2)])                                              # g > the run
    assert ctx.chop(b, width=2, stagger=0) == ctx.chop(b, width=2)
    # nothing wraps at the top of the range
    top = 2 ** 63 - 1
    for k in (0, 1, 5):
        x = bed([(top - k - 9, top - k)])
        for w, g in ((2 ** 63 - 1, None), (2 ** 64 - 1, 4), (2 ** 62, 2 ** 63), (4, 2 ** 64 - 1), (3, 3)):
            for ex in (False, True):
                assert ctx.chop(x, width=w, stagger=g, exclude_short=ex) == \
                    oracle.integers("chop", [x], width=w, stagger=g, exclude_short=ex), (k, w, g, ex)
    # w at least the longest run: merge
    rng = random.Random(55)
    inputs = [_random_input(rng, [b"chr1", b"chr2"], 800, b"c") for _ in range(2)]
    assert ctx.chop(*inputs, width=4096) == ctx.merge(*inputs)


def test_chop_too_large_is_refused(ctx):
    import starch_amd
    t0 = time.monotonic()
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.chop(bed([(0, 2 ** 40)]))
    assert e.value.code == -2 and "result too large" in str(e.value)
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.chop(bed([(0, 2 ** 63 - 1)]) + bed([(0, 2 ** 63 - 1)], b"chr2"), width=1)   # the counts' sum must not wrap
    assert e.value.code == -2 and "result too large" in str(e.value)
    assert time.monotonic() - t0 < 5
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    assert ctx.chop(bed([(0, 2)])) == bed([(0, 1), (1, 2)])                 # the context works again


# ---- 6. everything -------------------------------------------------------------------------------------
def test_everything(ctx):
    rng = random.Random(66)
    inputs = [_random_input(rng, [b"chr1", b"chr10", b"chr2"], n, b"e%d." % k) for k, n in enumerate((900, 1, 1500))]
    got = ctx.everything(*inputs)
    assert got == ctx.sort_bed(b"".join(inputs)) == oracle.integers("everything", inputs)
    # ties across inputs come in input order
    same = b"chr1\t5\t9\t"
    tied = [same + b"a\n" + same + b"b\n", same + b"c\n", b"chr1\t5\t8\tfirst\n" + same + b"d\n"]
    assert ctx.everything(*tied) == b"chr1\t5\t8\tfirst\n" + same + b"a\n" + same + b"b\n" + same + b"c\n" + same + b"d\n"
    # inputs already in order one after the other
    assert ctx.everything(bed([(1, 2), (3, 4)]), bed([(5, 6)], b"chr2")) == bed([(1, 2), (3, 4)]) + bed([(5, 6)], b"chr2")
    # a long line goes through the wave copy
    long_line = b"chr1\t2\t3\t" + b"x" * 1000 + b"\n"
    assert ctx.everything(bed([(5, 6)]), long_line) == long_line + bed([(5, 6)])
    assert ctx.element_of(long_line + bed([(5, 6)]), bed([(0, 4)])) == long_line


# ---- 7. errors -------------------------------------------------------------------------------------------
def _refused(ctx, op, inputs, code, *words):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        call(ctx, op, inputs)
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (op, w, str(e.value))
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4


@pytest.mark.parametrize("op", OPS)
def test_errors(ctx, op):
    hi, lo = bed([(500, 600), (700, 800)]), bed([(1, 2), (3, 4), (2, 9), (0, 1)])
    _refused(ctx, op, [hi, lo], -12, "bedops: input 1, line 3:", "sort-bed")
    _refused(ctx, op, [hi, bed([(1, 2), (5, 5)])], -12, "input 1, line 2:", "stop")
    # a malformed line in input 2 goes ahead of an order error in input 1
    _refused(ctx, op, [hi, lo, b"chr1\t1\t2\nchr1\t5\n"], -12, "input 2, line 2:", "fewer than three")
    _refused(ctx, op, [hi, hi, b"track name=x\nchr1\t1\t2\n"], -12, "input 2, line 1:", "track")
    good = bed([(1, 2)])
    assert ctx.everything(good) == good                     # the context works again


def test_argument_errors(ctx):
    import starch_amd
    L = starch_amd.load()
    two = (starch_amd.SetopInput * 2)()

    def opts(op, threshold=100, pct=1, chop=1):
        o = starch_amd.BedopsOptions()
        o.op, o.threshold, o.threshold_is_percent, o.chop = op, threshold, pct, chop
        return ctypes.byref(o)

    for o in (opts(5, 0, 0), opts(5, 0, 1), opts(6, 101, 1), opts(8, chop=0), opts(10), opts(-1), None):
        assert L.starch_bedops_host(ctx._h, o, two, 2) == -2
    assert L.starch_bedops_host(ctx._h, opts(5), two, 1) == -2
    assert L.starch_bedops_host(ctx._h, opts(9), None, 1) == -2
    assert L.starch_bedops_host(ctx._h, opts(9), two, 0) == -2
    assert L.starch_bedops_host(ctx._h, opts(5, 101, 0), two, 2) == 0        # 101 bases is a threshold
    assert L.starch_setop_host(ctx._h, 5, two, 1) == -2
    a = bed([(1, 2)])
    for bad in ({"threshold": 0}, {"threshold": "0%"}, {"threshold": "101%"}):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.element_of(a, a, **bad)
        assert e.value.code == -2
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.element_of(a)
    assert e.value.code == -2
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.chop(a, width=0)
    assert e.value.code == -2


# ---- 8. device entry and chaining ---------------------------------------------------------------------------
def test_device_entry_and_chaining(ctx):
    import torch
    rng = random.Random(88)
    inputs = [_random_input(rng, [b"chr1", b"chr2"], n, b"d") for n in (900, 0, 1500)]
    inputs[0] = inputs[0][:-1]                                # no final newline
    blob = b"".join(inputs)
    offs = [0]
    for b in inputs:
        offs.append(offs[-1] + len(b))
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    for op in OPS:
        for kw in variants(op)[1:3] or [{}]:
            want = call(ctx, op, inputs, **kw)
            assert want == oracle.bitmap(op, inputs, **kw)
            k = ctx.bedops_device(op, dev.data_ptr(), offs, threshold=kw.get("threshold", "100%"), chop=kw.get("width", 1),
                                  stagger=kw.get("stagger"), exclude_short=kw.get("exclude_short", False))
            assert k == len(want) and ctx._output() == want, (op, kw)
    # an archive as an input gives the same bytes as its BED
    arch = ctx.compress(inputs[2])
    assert arch[:4] == b"\xca\x5c\xad\x1a"
    for op in OPS:
        kw = variants(op)[-2] if len(variants(op)) > 1 else {}
        want = call(ctx, op, [inputs[0], inputs[2]], **kw)
        assert call(ctx, op, [inputs[0], arch], **kw) == want != b"", op
        assert ctx.setop_stats()["archives_decoded"] == 1
    # partition and chop outputs are valid input for the encoder
    for out in (ctx.partition(*inputs), ctx.chop(*inputs, width=100, stagger=40)):
        assert out and ctx.sort_check(out) == 0
        assert ctx.unstarch(ctx.compress(out)) == out
    # ops 0 to 4 through the new entry are the old ones
    import starch_amd
    for op in starch_amd.SETOPS:
        assert ctx.bedops(op, inputs) == ctx.setop(op, inputs), op
        assert ctx.bedops_device(op, dev.data_ptr(), offs) == len(ctx.setop(op, inputs))


# ---- 9. command -------------------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_command(ctx, tmp_path):
    rng = random.Random(99)
    a = _random_input(rng, [b"chr1", b"chr2"], 800, b"a", lengths=(7, 40, 600))
    b = _random_input(rng, [b"chr1", b"chr3"], 600, b"b")
    fa, fb, fs = tmp_path / "a.bed", tmp_path / "b.bed", tmp_path / "b.starch"
    fa.write_bytes(a)
    fb.write_bytes(b)
    fs.write_bytes(ctx.compress(b))
    r = _run([BEDOPS, "-e", "1", str(fa), str(fs)])
    assert r.returncode == 0 and r.stdout == ctx.element_of(a, b, threshold=1) == oracle.bitmap("element_of", [a, b], threshold=1)
    r = _run([BEDOPS, "-n", "50%", "-", str(fb)], input=a)
    assert r.returncode == 0 and r.stdout == ctx.not_element_of(a, b, threshold="50%")
    r = _run([BEDOPS, "-e", str(fa), str(fb)])                 # the default, 100%
    assert r.returncode == 0 and r.stdout == ctx.element_of(a, b) == oracle.bitmap("element_of", [a, b])
    r = _run([BEDOPS, "-p", str(fa), str(fb)])
    assert r.returncode == 0 and r.stdout == ctx.partition(a, b)
    r = _run([BEDOPS, "-w", "100", "--stagger", "40", "-x", str(fa), str(fb)])
    assert r.returncode == 0 and r.stdout == ctx.chop(a, b, width=100, stagger=40, exclude_short=True) != b""
    r = _run([BEDOPS, "-u", str(fa), str(fb)])
    assert r.returncode == 0 and r.stdout == ctx.everything(a, b)
    r = _run([BEDOPS, "--stagger", "40", "-m", str(fa)])
    assert r.returncode == 1 and r.stdout == b"" and b"USAGE" in r.stderr
    fu = tmp_path / "unsorted.bed"
    fu.write_bytes(bed([(5, 6), (1, 2)]))
    r = _run([BEDOPS, "-u", str(fa), str(fu)])
    assert r.returncode == 22 and r.stdout == b"" and b"input 1, line 2:" in r.stderr
