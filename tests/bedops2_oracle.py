"""Plain-Python oracles for bedops' element-of, not-element-of, partition, chop
and everything as include/starch_amd.h defines them.  They take nothing from
the code under test, and for every op there are two that share no method:

  bitmap(op, inputs, **kw)    coordinates below 4096: per-base numpy arrays per
                              chromosome (the union as a bool array, the longest
                              run of set bases inside a line's slice; a cover
                              count and a boundary mark per base; numpy ranges
                              over the union's runs; two stable bucket passes, by
                              stop and by start).
  integers(op, inputs, **kw)  any coordinates: sorted boundary lists with
                              bisected depths for partition, explicit loops over
                              merged runs for chop and element-of, and
                              sorted(..., key=(chrom, start, stop, input, line))
                              for everything.

inputs: a list of bytes, BED text.  kw: threshold (an int of bases, or a str
"7" / "50%"), width, stagger (None: width), exclude_short.  Both return the
expected output bytes.  TABLE holds hand-written expectations.
"""
import bisect

import numpy as np

OPS = ("element_of", "not_element_of", "partition", "chop", "everything")
LIMIT = 4096


def lines(bed):
    """[(chrom, start, stop, the whole line without '\\n'), ...]; a last line without newline is a line."""
    out = []
    for ln in bed.split(b"\n"):
        if ln == b"":
            continue
        f = ln.split(b"\t")
        out.append((f[0], int(f[1]), int(f[2]), ln))
    return out


def bed3(rows):
    return b"".join(b"%s\t%d\t%d\n" % r for r in rows)


def threshold_of(t):
    """(value, is percent)"""
    if isinstance(t, int):
        return t, False
    return (int(t[:-1]), True) if t.endswith("%") else (int(t), False)


def selected(ov, length, t):
    v, pct = threshold_of(t)
    return ov * 100 >= v * length if pct else ov >= v     # Python integers: exact


def _chroms(parsed):
    return sorted({c for p in parsed for c, _, _, _ in p})


# ---- per-base arrays --------------------------------------------------------------------
def _union_map(parsed, c):
    m = np.zeros(LIMIT + 1, dtype=bool)
    for p in parsed:
        for cc, s, e, _ in p:
            if cc == c:
                assert 0 <= s < e <= LIMIT
                m[s:e] = True
    return m


def _runs_of(m):
    d = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    return [(int(a), int(b)) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]


def _bitmap_element(inputs, threshold, invert):
    parsed = [lines(b) for b in inputs]
    maps = {}
    out = []
    for c, s, e, raw in parsed[0]:
        if c not in maps:
            maps[c] = _union_map(parsed[1:], c)
        inside = _runs_of(maps[c][s:e])              # the union's runs clipped to the line
        ov = max((b - a for a, b in inside), default=0)
        if selected(ov, e - s, threshold) != invert:
            out.append(raw + b"\n")
    return b"".join(out)


def _bitmap_partition(inputs):
    parsed = [lines(b) for b in inputs]
    rows = []
    for c in _chroms(parsed):
        cover = np.zeros(LIMIT + 2, dtype=np.int64)
        edge = np.zeros(LIMIT + 2, dtype=bool)
        for p in parsed:
            for cc, s, e, _ in p:
                if cc == c:
                    assert 0 <= s < e <= LIMIT
                    cover[s:e] += 1
                    edge[s] = edge[e] = True
        at = np.flatnonzero(edge)
        for p, q in zip(at[:-1], at[1:]):
            if cover[p] > 0:
                rows.append((c, int(p), int(q)))
    return bed3(rows)


def _bitmap_chop(inputs, width, stagger, exclude_short):
    parsed = [lines(b) for b in inputs]
    g = width if stagger is None else stagger
    rows = []
    for c in _chroms(parsed):
        for a, b in _runs_of(_union_map(parsed, c)):
            starts = np.arange(a, b, g, dtype=np.int64)
            stops = np.minimum(starts + width, b)
            for s, e in zip(starts, stops):
                if not (exclude_short and e - s < width):
                    rows.append((c, int(s), int(e)))
    return bed3(rows)


def _bitmap_everything(inputs):
    parsed = [lines(b) for b in inputs]
    out = []
    for c in _chroms(parsed):
        # two stable bucket passes, by stop and then by start, over the lines in (input, line) order
        by_stop = [[] for _ in range(LIMIT + 1)]
        for p in parsed:
            for cc, s, e, raw in p:
                if cc == c:
                    assert 0 <= s < e <= LIMIT
                    by_stop[e].append((s, raw))
        by_start = [[] for _ in range(LIMIT + 1)]
        for cell in by_stop:
            for s, raw in cell:
                by_start[s].append(raw)
        for cell in by_start:
            for raw in cell:
                out.append(raw + b"\n")
    return b"".join(out)


def bitmap(op, inputs, threshold="100%", width=1, stagger=None, exclude_short=False):
    if op == "element_of":
        return _bitmap_element(inputs, threshold, False)
    if op == "not_element_of":
        return _bitmap_element(inputs, threshold, True)
    if op == "partition":
        return _bitmap_partition(inputs)
    if op == "chop":
        return _bitmap_chop(inputs, width, stagger, exclude_short)
    if op == "everything":
        return _bitmap_everything(inputs)
    raise ValueError(op)


# ---- integers ---------------------------------------------------------------------------
def merged_runs(parsed):
    """{chrom: [(a, b), ...]}: the maximal runs of the union of the inputs, abutting ones joined."""
    by = {}
    for p in parsed:
        for c, s, e, _ in p:
            by.setdefault(c, []).append((s, e))
    runs = {}
    for c, iv in by.items():
        iv.sort()
        cur = []
        for s, e in iv:
            if cur and s <= cur[-1][1]:
                if e > cur[-1][1]:
                    cur[-1][1] = e
            else:
                cur.append([s, e])
        runs[c] = [(a, b) for a, b in cur]
    return runs


def _int_element(inputs, threshold, invert):
    parsed = [lines(b) for b in inputs]
    runs = merged_runs(parsed[1:])
    out = []
    for c, s, e, raw in parsed[0]:
        ov = 0
        for a, b in runs.get(c, ()):
            ov = max(ov, min(b, e) - max(a, s))       # negative when they do not overlap
        if selected(ov, e - s, threshold) != invert:
            out.append(raw + b"\n")
    return b"".join(out)


def _int_partition(inputs):
    parsed = [lines(b) for b in inputs]
    rows = []
    for c in _chroms(parsed):
        starts = sorted(s for p in parsed for cc, s, _, _ in p if cc == c)
        stops = sorted(e for p in parsed for cc, _, e, _ in p if cc == c)
        points = sorted(set(starts) | set(stops))
        for p, q in zip(points[:-1], points[1:]):
            # lines with start <= p and stop > p: they cover [p, q), since no start or stop lies between
            if bisect.bisect_right(starts, p) - bisect.bisect_right(stops, p) > 0:
                rows.append((c, p, q))
    return bed3(rows)


def _int_chop(inputs, width, stagger, exclude_short):
    parsed = [lines(b) for b in inputs]
    g = width if stagger is None else stagger
    runs = merged_runs(parsed)
    rows = []
    for c in sorted(runs):
        for a, b in runs[c]:
            k = 0
            while a + k * g < b:
                s = a + k * g
                if not (exclude_short and b - s < width):
                    rows.append((c, s, min(s + width, b)))
                k += 1
    return bed3(rows)


def _int_everything(inputs):
    keyed = []
    for k, b in enumerate(inputs):
        for n, (c, s, e, raw) in enumerate(lines(b)):
            keyed.append((c, s, e, k, n, raw))
    return b"".join(r[5] + b"\n" for r in sorted(keyed, key=lambda r: r[:5]))


def integers(op, inputs, threshold="100%", width=1, stagger=None, exclude_short=False):
    if op == "element_of":
        return _int_element(inputs, threshold, False)
    if op == "not_element_of":
        return _int_element(inputs, threshold, True)
    if op == "partition":
        return _int_partition(inputs)
    if op == "chop":
        return _int_chop(inputs, width, stagger, exclude_short)
    if op == "everything":
        return _int_everything(inputs)
    raise ValueError(op)


# ---- hand-written expectations: (op, inputs, keyword arguments, expected output) ----------------
def _b(*iv, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % (chrom, s, t) for s, t in iv)


_REF = b"chr1\t0\t10\ta\nchr1\t20\t30\tb\t9\nchr1\t40\t60\tc\nchr2\t5\t6\td\n"
_OTH = [_b((0, 4), (4, 10), (25, 30), (38, 47), (50, 60)), _b((28, 29)) + _b((0, 100), chrom=b"chr10")]
TABLE = [
    # 0-4 and 4-10 abut: one run covers line a; b is half covered; c meets two runs of 7 and 10; d none
    ("element_of", [_REF] + _OTH, {}, b"chr1\t0\t10\ta\n"),
    ("not_element_of", [_REF] + _OTH, {}, b"chr1\t20\t30\tb\t9\nchr1\t40\t60\tc\nchr2\t5\t6\td\n"),
    ("element_of", [_REF] + _OTH, {"threshold": "50%"}, b"chr1\t0\t10\ta\nchr1\t20\t30\tb\t9\nchr1\t40\t60\tc\n"),
    ("element_of", [_REF] + _OTH, {"threshold": "51%"}, b"chr1\t0\t10\ta\n"),
    ("element_of", [_REF] + _OTH, {"threshold": 8}, b"chr1\t0\t10\ta\nchr1\t40\t60\tc\n"),
    ("not_element_of", [_REF] + _OTH, {"threshold": 1}, b"chr2\t5\t6\td\n"),
    ("element_of", [_REF, b"", b""], {"threshold": 1}, b""),
    ("partition", [_b((0, 10), (5, 15), (5, 15), (20, 30)), _b((10, 12), (15, 20))], {},
     _b((0, 5), (5, 10), (10, 12), (12, 15), (15, 20), (20, 30))),
    ("partition", [_b((0, 100), (10, 20), (30, 40)), _b((1, 2), chrom=b"chr2")], {},
     _b((0, 10), (10, 20), (20, 30), (30, 40), (40, 100)) + _b((1, 2), chrom=b"chr2")),
    ("partition", [_b((0, 5), (7, 9))], {}, _b((0, 5), (7, 9))),
    ("chop", [_b((0, 10), (10, 12), (20, 23))], {"width": 5}, _b((0, 5), (5, 10), (10, 12), (20, 23))),
    ("chop", [_b((0, 10), (10, 12), (20, 23))], {"width": 5, "exclude_short": True}, _b((0, 5), (5, 10))),
    ("chop", [_b((0, 12))], {"width": 5, "stagger": 2}, _b((0, 5), (2, 7), (4, 9), (6, 11), (8, 12), (10, 12))),
    ("chop", [_b((0, 12))], {"width": 5, "stagger": 2, "exclude_short": True}, _b((0, 5), (2, 7), (4, 9), (6, 11))),
    ("chop", [_b((0, 12)), _b((3, 4), chrom=b"chr2")], {"width": 5, "stagger": 9}, _b((0, 5), (9, 12)) + _b((3, 4), chrom=b"chr2")),
    ("chop", [_b((7, 9))], {}, _b((7, 8), (8, 9))),
    ("everything", [b"chr1\t5\t9\tx\nchr2\t1\t2\n", b"chr1\t1\t2\nchr1\t5\t9\ty\nchr10\t3\t4\tz"], {},
     b"chr1\t1\t2\nchr1\t5\t9\tx\nchr1\t5\t9\ty\nchr10\t3\t4\tz\nchr2\t1\t2\n"),
    ("everything", [b"chr1\t5\t9\tsecond", b"chr1\t5\t8\nchr1\t5\t9\tthird\n", b""], {},
     b"chr1\t5\t8\nchr1\t5\t9\tsecond\nchr1\t5\t9\tthird\n"),
]
