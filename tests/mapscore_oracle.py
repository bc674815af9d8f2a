"""Plain-Python oracle of bedmap-scores (include/starch_amd.h has the
definition).  The hit lists are those of tests/mapel_oracle.py (hits_brute, or
hits_sweep as the cross-check); every column is computed with Python integers
and fractions.Fraction, and rounding is round() of a Fraction, which is ties to
even.  TABLE holds cases whose expected bytes were typed by hand."""
import re
from fractions import Fraction

from tests.mapel_oracle import CRITERIA, hits_brute, hits_sweep, parse  # noqa: F401  (re-exported for the tests)

COLS = ("echo", "count", "indicator", "sum", "mean", "min", "max", "median", "kth", "min_element", "max_element")
SCORE_COLS = COLS[3:]
UNIT = 10 ** 9
GRAMMAR = re.compile(rb"[+-]?(?:[0-9]{1,9}(?:\.[0-9]{0,9})?|\.[0-9]{1,9})")


class BadScore(Exception):
    """A hit has no column 5 or one that is no score; line: the map line from 1."""
    def __init__(self, line):
        super().__init__("map line %d" % line)
        self.line = line


def units(fields):
    """The score of a parsed line as a count of 10^-9 units, or None."""
    if len(fields) < 5 or not GRAMMAR.fullmatch(fields[4]):
        return None
    return int(Fraction(fields[4].decode()) * UNIT)     # exact: at most 9 digits after the point


def fmt(x, prec):
    """x (a Fraction or int) with prec decimals: nearest, ties to even, no negative zero."""
    m = round(Fraction(x) * 10 ** prec)
    q, r = divmod(abs(m), 10 ** prec)
    return (b"-" if m < 0 else b"") + b"%d" % q + (b".%0*d" % (prec, r) if prec else b"")


def mapsc(ref, map=None, cols=("echo", "mean"), criterion=("bp_ovr", 1), prec=6, kth=None, skip_unmapped=False, delim=b"|",
          finder=hits_brute):
    """The bytes Starch.map_scores gives; BadScore for the lowest hit without a valid score when a score column is asked for."""
    criterion = (criterion,) if isinstance(criterion, str) else tuple(criterion)
    rrows = parse(ref)
    mrows = rrows if map is None else parse(map)
    hits = finder(rrows, mrows, criterion)
    scores = [units(row[3]) for row in mrows]
    if any(c in SCORE_COLS for c in cols):
        bad = [j for hs in hits for j in hs if scores[j] is None]
        if bad:
            raise BadScore(min(bad) + 1)
    out = []
    for (_, _, _, _, line), hs in zip(rrows, hits):
        if skip_unmapped and not hs:
            continue
        n = len(hs)
        v = [Fraction(scores[j], UNIT) for j in hs] if any(c in SCORE_COLS for c in cols) else []
        w = sorted(v)
        vals = []
        for col in cols:
            if col == "echo":
                vals.append(line)
            elif col == "count":
                vals.append(b"%d" % n)
            elif col == "indicator":
                vals.append(b"1" if n else b"0")
            elif n == 0:
                vals.append(b"NAN")
            elif col == "sum":
                vals.append(fmt(sum(v), prec))
            elif col == "mean":
                vals.append(fmt(sum(v) / n, prec))
            elif col == "min":
                vals.append(fmt(w[0], prec))
            elif col == "max":
                vals.append(fmt(w[-1], prec))
            elif col == "median":
                vals.append(fmt(w[n // 2] if n % 2 else (w[n // 2 - 1] + w[n // 2]) / 2, prec))
            elif col == "kth":
                k = -((-Fraction(str(kth)) * n) // 1)          # ceil(f * n)
                vals.append(fmt(w[int(k) - 1], prec))
            elif col == "min_element":
                vals.append(mrows[hs[v.index(w[0])]][4])        # index(): the first in map order
            elif col == "max_element":
                vals.append(mrows[hs[v.index(w[-1])]][4])
            else:
                raise ValueError(col)
        out.append(delim.join(vals) + b"\n")
    return b"".join(out)


def straddling(ref, map, criterion, tile, finder=hits_brute):
    """Reference lines whose hits lie in more than one tile of `tile` hits of the hit list."""
    rrows = parse(ref)
    hits = finder(rrows, rrows if map is None else parse(map), tuple(criterion))
    at = count = 0
    for hs in hits:
        if hs and at // tile != (at + len(hs) - 1) // tile:
            count += 1
        at += len(hs)
    return count


# ---- cases typed by hand: (ref, map or None, keyword arguments, expected bytes) -------------------------
R1 = b"chr1\t10\t20\tr1\nchr1\t30\t40\tr2\nchr2\t5\t9\tr3\n"
# under the default criterion r1 has a, b, c (7, -0.5, 3), r2 has b, r3 has nothing
M1 = b"chr1\t0\t12\ta\t+7\nchr1\t15\t35\tb\t-.5\nchr1\t19\t20\tc\t3.\nchr1\t40\t50\td\t4\nchr2\t1\t5\te\t5\nchr3\t1\t9\tf\t6\n"
R3 = b"chr1\t0\t10\nchr1\t10\t20\nchr1\t20\t30\n"


def one_each(*scores):
    """A map with one line under each line of R3"""
    return b"".join(b"chr1\t%d\t%d\tx\t%s\n" % (10 * k, 10 * k + 5, s) for k, s in enumerate(scores))


def under_first(*scores):
    """A map whose lines all lie under the first line of R3"""
    return b"".join(b"chr1\t%d\t%d\tm%d\t%s\n" % (k, k + 1, k, s) for k, s in enumerate(scores))


TABLE = [
    # the default columns, criterion and precision: 9.5 / 3
    (R1, M1, {}, b"chr1\t10\t20\tr1|3.166667\nchr1\t30\t40\tr2|-0.500000\nchr2\t5\t9\tr3|NAN\n"),
    # prec 0: 9.5 is a tie and goes to 10, -0.5 is a tie and goes to 0, which carries no sign
    (R1, M1, dict(cols=("count", "indicator", "sum", "min", "max"), prec=0),
     b"3|1|10|0|7\n1|1|0|0|0\n0|0|NAN|NAN|NAN\n"),
    # prec 9; an odd median; kth 0.5 of three is the second
    (R1, M1, dict(cols=("mean", "median", "kth"), prec=9, kth="0.5"),
     b"3.166666667|3.000000000|3.000000000\n-0.500000000|-0.500000000|-0.500000000\nNAN|NAN|NAN\n"),
    (R1, M1, dict(cols=("kth",), kth="1"), b"7.000000\n-0.500000\nNAN\n"),
    (R1, M1, dict(cols=("kth",), kth="0.000000001", prec=1), b"-0.5\n-0.5\nNAN\n"),
    # the element columns are whole map lines
    (R1, M1, dict(cols=("min_element", "max_element")),
     b"chr1\t15\t35\tb\t-.5|chr1\t0\t12\ta\t+7\nchr1\t15\t35\tb\t-.5|chr1\t15\t35\tb\t-.5\nNAN|NAN\n"),
    # skip_unmapped and another delimiter
    (R1, M1, dict(cols=("count", "sum"), skip_unmapped=True, delim=b"\t"), b"3\t9.500000\n1\t-0.500000\n"),
    # the ties 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    (R3, one_each(b"0.5", b"1.5", b"2.5"), dict(cols=("sum",), prec=0), b"0\n2\n2\n"),
    (R3, one_each(b"-0.5", b"-1.5", b"-2.5"), dict(cols=("mean",), prec=0), b"0\n-2\n-2\n"),
    # a negative result that rounds to zero, and one that does not
    (R3, one_each(b"-0.0000004", b"-0.0000006", b"-.000000001"), dict(cols=("max",), prec=6),
     b"0.000000\n-0.000001\n0.000000\n"),
    # the longest score
    (R3, one_each(b"000000001.000000001", b"999999999.999999999", b"-999999999.999999999"), dict(cols=("sum",), prec=9),
     b"1.000000001\n999999999.999999999\n-999999999.999999999\n"),
    (R3, one_each(b"000000001.000000001", b"999999999.999999999", b"-999999999.999999999"), dict(cols=("min",), prec=6),
     b"1.000000\n1000000000.000000\n-1000000000.000000\n"),
    # even medians: (1 + 2) / 2 is a tie at prec 0; (2 + 3) / 2 of four values; values out of order in the map
    (R3, under_first(b"2", b"1"), dict(cols=("median",), prec=0), b"2\nNAN\nNAN\n"),
    (R3, under_first(b"10", b"3", b"1", b"2"), dict(cols=("median", "kth"), prec=6, kth="0.75"),
     b"2.500000|3.000000\nNAN|NAN\nNAN|NAN\n"),
    # element ties go to map order
    (R3, under_first(b"5", b"5.0", b"+5", b"4", b"4.000"), dict(cols=("min_element", "max_element", "count")),
     b"chr1\t3\t4\tm3\t4|chr1\t0\t1\tm0\t5|5\nNAN|NAN|0\nNAN|NAN|0\n"),
    # every criterion (the hits are those of tests/mapel_oracle.py's table)
    (R1, M1, dict(cols=("count", "sum"), criterion=("bp_ovr", 2)), b"2|6.500000\n1|-0.500000\n0|NAN\n"),
    (R1, M1, dict(cols=("count", "sum"), criterion=("range", 1)), b"3|9.500000\n2|3.500000\n1|5.000000\n"),
    (R1, M1, dict(cols=("count", "sum"), criterion=("fraction_ref", "0.5")), b"1|-0.500000\n1|-0.500000\n0|NAN\n"),
    (R1, M1, dict(cols=("count", "sum"), criterion=("fraction_map", "0.25")), b"2|2.500000\n1|-0.500000\n0|NAN\n"),
    (R1, M1, dict(cols=("count", "sum"), criterion=("fraction_both", "0.25")), b"1|-0.500000\n1|-0.500000\n0|NAN\n"),
    (R1, M1, dict(cols=("count", "sum"), criterion=("fraction_either", "0.25")), b"2|2.500000\n1|-0.500000\n0|NAN\n"),
    (R1, b"chr1\t10\t19\tx\t9\nchr1\t10\t20\ty\t1\nchr1\t10\t20\tz\t2\nchr1\t10\t21\tw\t9\nchr1\t30\t40\tv\t.25\n",
     dict(cols=("count", "sum"), criterion=("exact",)), b"2|3.000000\n1|0.250000\n0|NAN\n"),
    # the reference as its own map
    (b"chr1\t1\t10\tp\t1\nchr1\t5\t6\tq\t2\nchr1\t10\t12\tr\t-3\n", None, dict(cols=("echo", "sum", "mean"), prec=1),
     b"chr1\t1\t10\tp\t1|3.0|1.5\nchr1\t5\t6\tq\t2|3.0|1.5\nchr1\t10\t12\tr\t-3|-3.0|-3.0\n"),
    # scores are not looked at when no column needs them, nor on lines that are no hits
    (R1, b"chr1\t0\t12\ta\t1e3\nchr1\t15\t35\tb\n", dict(cols=("echo", "count", "indicator")),
     b"chr1\t10\t20\tr1|2|1\nchr1\t30\t40\tr2|1|1\nchr2\t5\t9\tr3|0|0\n"),
    (R1, b"chr1\t0\t5\ta\tnan\nchr1\t15\t35\tb\t2\nchr1\t50\t60\tc\n", dict(cols=("sum",), prec=0), b"2\n2\nNAN\n"),
    # an empty map, an empty reference
    (R1, b"", dict(cols=("indicator", "sum", "max_element")), b"0|NAN|NAN\n0|NAN|NAN\n0|NAN|NAN\n"),
    (b"", M1, {}, b""),
]
