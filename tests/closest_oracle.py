"""A plain-Python oracle for closest-features as include/starch_amd.h defines it.
It takes nothing from the code under test and shares no method with it: a double
loop over reference and query lines builds both candidate lists, and max / min
with the tie rules pick from them.

closest(ref, query, ...) takes BED text (bytes) and returns the expected output
bytes; sides(ref, query, no_overlaps) returns per reference line the pair
(left, right) before `closest` chooses, each None or (query line bytes, dist).
TABLE holds hand-written cases: (ref, query, keyword arguments, expected bytes).
"""


def parse(bed):
    """[(whole line, chrom, start, stop), ...] (a last line without newline is a line)."""
    out = []
    for ln in bed.split(b"\n"):
        if ln == b"":
            continue
        f = ln.split(b"\t")
        out.append((ln, f[0], int(f[1]), int(f[2])))
    return out


def dist(s, e, a, b):
    if a < e and b > s:
        return 0
    if b <= s:
        return -(s - b + 1)
    assert a >= e
    return a - e + 1


def sides(ref, query, no_overlaps=False):
    Q = parse(query)
    out = []
    for _, c, s, e in parse(ref):
        left, right = [], []          # (dist, position in the query, line)
        for k, (line, qc, a, b) in enumerate(Q):
            if qc != c:
                continue
            d = dist(s, e, a, b)
            if no_overlaps and d == 0:
                continue
            if (a, b) < (s, e):
                assert d <= 0
                left.append((d, k, line))
            else:
                assert d >= 0
                right.append((d, k, line))
        lt = max(left, key=lambda t: (t[0], t[1])) if left else None        # the greatest dist, then the last
        rt = min(right, key=lambda t: (t[0], t[1])) if right else None      # the least dist, then the first
        out.append((lt and (lt[2], lt[0]), rt and (rt[2], rt[0])))
    return out


def closest(ref, query, closest=False, dist=False, no_overlaps=False, no_ref=False, delim=b"|"):
    out = []
    for (line, _, _, _), (lt, rt) in zip(parse(ref), sides(ref, query, no_overlaps)):
        if closest:
            if lt is None or rt is None:
                els = [lt if lt is not None else rt]
            else:
                els = [lt if abs(lt[1]) <= abs(rt[1]) else rt]
        else:
            els = [lt, rt]
        fields = [] if no_ref else [line]
        for el in els:
            fields.append(b"NA" if el is None else el[0])
            if dist:
                fields.append(b"NA" if el is None else b"%d" % el[1])
        out.append(delim.join(fields) + b"\n")
    return b"".join(out)


def _b(*rows):
    return b"".join(b"chr1\t%d\t%d\n" % r for r in rows)


D = dict(dist=True)
TABLE = [
    # 0: one element on each side, at a distance
    (_b((100, 200)), _b((10, 50), (300, 400)), D, b"chr1\t100\t200|chr1\t10\t50|-51|chr1\t300\t400|101\n"),
    # 1: abutting on both sides: -1 and +1
    (_b((100, 200)), _b((50, 100), (200, 250)), D, b"chr1\t100\t200|chr1\t50\t100|-1|chr1\t200\t250|1\n"),
    # 2: a query line equal to the reference line is a right candidate
    (_b((100, 200)), _b((100, 200)), D, b"chr1\t100\t200|NA|NA|chr1\t100\t200|0\n"),
    # 3: overlapping on both sides: both at 0
    (_b((100, 200)), _b((90, 110), (150, 300)), D, b"chr1\t100\t200|chr1\t90\t110|0|chr1\t150\t300|0\n"),
    # 4: NA on the left
    (_b((100, 200)), _b((500, 600)), D, b"chr1\t100\t200|NA|NA|chr1\t500\t600|301\n"),
    # 5: NA on the right
    (_b((100, 200)), _b((1, 2)), D, b"chr1\t100\t200|chr1\t1\t2|-99|NA|NA\n"),
    # 6: NA on both sides: the query has another chromosome only, or nothing at all
    (_b((100, 200)), b"chr2\t100\t200\n", D, b"chr1\t100\t200|NA|NA|NA|NA\n"),
    (_b((100, 200)), b"", {}, b"chr1\t100\t200|NA|NA\n"),
    # 8: without dist
    (_b((100, 200)), _b((10, 50), (300, 400)), {}, b"chr1\t100\t200|chr1\t10\t50|chr1\t300\t400\n"),
    # 9: closest: the right one is nearer
    (_b((100, 200)), _b((10, 50), (210, 400)), dict(closest=True, dist=True), b"chr1\t100\t200|chr1\t210\t400|11\n"),
    # 10: closest: a tie goes to the left
    (_b((100, 200)), _b((10, 90), (210, 400)), dict(closest=True, dist=True), b"chr1\t100\t200|chr1\t10\t90|-11\n"),
    # 11: closest with one side NA, and with both
    (_b((100, 200)), _b((300, 400)), dict(closest=True, dist=True), b"chr1\t100\t200|chr1\t300\t400|101\n"),
    (_b((100, 200)), b"", dict(closest=True, dist=True), b"chr1\t100\t200|NA|NA\n"),
    # 13: no_overlaps removes the overlapping lines from both sides
    (_b((100, 200)), _b((10, 50), (90, 110), (150, 300), (200, 201)), dict(no_overlaps=True, dist=True),
     b"chr1\t100\t200|chr1\t10\t50|-51|chr1\t200\t201|1\n"),
    # 14: no_ref, and a delimiter of its own
    (_b((100, 200)), _b((10, 50), (300, 400)), dict(no_ref=True, dist=True, delim=b"\t"),
     b"chr1\t10\t50\t-51\tchr1\t300\t400\t101\n"),
    (_b((100, 200)), _b((10, 50), (300, 400)), dict(no_ref=True, closest=True), b"chr1\t10\t50\n"),
    # 16: the left tie goes to the last, the right tie to the first; a long early line beats nearer starts
    (_b((100, 200)), _b((10, 90), (20, 90), (30, 80), (210, 220), (210, 230)), D,
     b"chr1\t100\t200|chr1\t20\t90|-11|chr1\t210\t220|11\n"),
    (_b((100, 200)), _b((0, 101), (10, 90), (20, 95)), D, b"chr1\t100\t200|chr1\t0\t101|0|NA|NA\n"),
    # 18: equal starts: a shorter line is left, a longer one right
    (_b((100, 200)), _b((100, 150), (100, 250)), D, b"chr1\t100\t200|chr1\t100\t150|0|chr1\t100\t250|0\n"),
    # 19: two reference lines, every column of both inputs echoed
    (b"chr1\t5\t6\tr1\nchr2\t7\t9\tr2\t+\n", b"chr1\t1\t2\tq1\t.\nchr2\t20\t30\tq2\n", D,
     b"chr1\t5\t6\tr1|chr1\t1\t2\tq1\t.|-4|NA|NA\nchr2\t7\t9\tr2\t+|NA|NA|chr2\t20\t30\tq2|12\n"),
]
