"""Plain-Python oracles of bedmap-elements (include/starch_amd.h has the
definition): a brute force over all pairs and a sweep that keeps the active map
lines.  Both use integers and fractions.Fraction for the criteria.  TABLE holds
cases whose expected bytes were typed by hand."""
from fractions import Fraction

U64 = 2 ** 64 - 1
COLS = ("echo", "count", "indicator", "echo_ref_size", "echo_ref_name", "echo_ref_row_id", "echo_map", "echo_map_id",
        "echo_map_score", "echo_map_size", "echo_overlap_size", "echo_map_range")
CRITERIA = ("bp_ovr", "range", "fraction_ref", "fraction_map", "fraction_both", "fraction_either", "exact")


class MissingColumn(Exception):
    """A hit lacks the column echo_map_id or echo_map_score asks for; line: the map line from 1."""
    def __init__(self, line):
        super().__init__("map line %d" % line)
        self.line = line


def parse(bed):
    """[(chrom, start, stop, fields, line without its newline)]"""
    rows = []
    for ln in bytes(bed).split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            rows.append((f[0], int(f[1]), int(f[2]), f, ln))
    return rows


def window(s, e, criterion):
    r = int(criterion[1]) if criterion[0] == "range" else 0
    return max(0, s - r), min(U64, e + r)


def is_hit(criterion, s, e, sp, ep, a, b):
    """Whether the map line [a, b) is a hit of the reference line [s, e) with window [sp, ep)."""
    if not (a < ep and b > sp):
        return False
    ov = min(b, ep) - max(a, sp)
    kind = criterion[0]
    if kind == "bp_ovr":
        return ov >= int(criterion[1])
    if kind == "range":
        return True
    if kind == "exact":
        return a == s and b == e
    f = Fraction(str(criterion[1]))
    ref, mp = Fraction(ov, e - s) >= f, Fraction(ov, b - a) >= f
    return {"fraction_ref": ref, "fraction_map": mp, "fraction_both": ref and mp, "fraction_either": ref or mp}[kind]


def hits_brute(ref, mp, criterion):
    """Per reference row the indices of its hits, in map order: every pair is tried."""
    out = []
    for c, s, e, _, _ in ref:
        sp, ep = window(s, e, criterion)
        out.append([j for j, (mc, a, b, _, _) in enumerate(mp) if mc == c and is_hit(criterion, s, e, sp, ep, a, b)])
    return out


def hits_sweep(ref, mp, criterion):
    """The same by a sweep per chromosome: map lines enter when they start below
    the largest window end so far and leave for good when they end at or before
    the window start, which never decreases."""
    by_chrom = {}
    for j, row in enumerate(mp):
        by_chrom.setdefault(row[0], []).append(j)
    out, state = [], {}
    for c, s, e, _, _ in ref:
        sp, ep = window(s, e, criterion)
        st = state.setdefault(c, {"next": 0, "active": [], "emax": 0})
        ids = by_chrom.get(c, [])
        st["emax"] = max(st["emax"], ep)
        while st["next"] < len(ids) and mp[ids[st["next"]]][1] < st["emax"]:
            st["active"].append(ids[st["next"]])
            st["next"] += 1
        st["active"] = [j for j in st["active"] if mp[j][2] > sp]
        out.append([j for j in st["active"] if mp[j][1] < ep and is_hit(criterion, s, e, sp, ep, mp[j][1], mp[j][2])])
    return out


def mapel(ref, map=None, cols=("echo", "echo_map"), criterion=("bp_ovr", 1), skip_unmapped=False, delim=b"|",
          multidelim=b";", finder=hits_brute):
    """The bytes Starch.map_elements gives; MissingColumn for the lowest hit that lacks a column asked for."""
    criterion = (criterion,) if isinstance(criterion, str) else tuple(criterion)
    rrows = parse(ref)
    mrows = rrows if map is None else parse(map)
    hits = finder(rrows, mrows, criterion)
    need = max([{"echo_map_id": 4, "echo_map_score": 5}.get(c, 0) for c in cols])
    bad = [j for hs in hits for j in hs if len(mrows[j][3]) < need]
    if bad:
        raise MissingColumn(min(bad) + 1)
    out = []
    for i, ((c, s, e, _, line), hs) in enumerate(zip(rrows, hits)):
        if skip_unmapped and not hs:
            continue
        sp, ep = window(s, e, criterion)
        vals = []
        for col in cols:
            if col == "echo":
                vals.append(line)
            elif col == "count":
                vals.append(b"%d" % len(hs))
            elif col == "indicator":
                vals.append(b"1" if hs else b"0")
            elif col == "echo_ref_size":
                vals.append(b"%d" % (e - s))
            elif col == "echo_ref_name":
                vals.append(b"%s:%d-%d" % (c, s, e))
            elif col == "echo_ref_row_id":
                vals.append(b"id-%d" % (i + 1))
            elif col == "echo_map":
                vals.append(multidelim.join(mrows[j][4] for j in hs))
            elif col == "echo_map_id":
                vals.append(multidelim.join(mrows[j][3][3] for j in hs))
            elif col == "echo_map_score":
                vals.append(multidelim.join(mrows[j][3][4] for j in hs))
            elif col == "echo_map_size":
                vals.append(multidelim.join(b"%d" % (mrows[j][2] - mrows[j][1]) for j in hs))
            elif col == "echo_overlap_size":
                vals.append(multidelim.join(b"%d" % (min(mrows[j][2], ep) - max(mrows[j][1], sp)) for j in hs))
            elif col == "echo_map_range":
                vals.append(b"%s\t%d\t%d" % (c, min(mrows[j][1] for j in hs), max(mrows[j][2] for j in hs)) if hs else b"")
            else:
                raise ValueError(col)
        out.append(delim.join(vals) + b"\n")
    return b"".join(out)


# ---- cases typed by hand: (ref, map or None, keyword arguments, expected bytes) -------------------------
R1 = b"chr1\t10\t20\tr1\nchr1\t30\t40\tr2\nchr2\t5\t9\tr3\n"
M1 = b"chr1\t0\t12\ta\t1.5\nchr1\t15\t35\tb\t2\nchr1\t19\t20\tc\t03\nchr1\t40\t50\td\t4\nchr2\t1\t5\te\t5\nchr3\t1\t9\tf\t6\n"
TABLE = [
    # the default columns and criterion; a chromosome with no hit, one the reference lacks
    (R1, M1, {},
     b"chr1\t10\t20\tr1|chr1\t0\t12\ta\t1.5;chr1\t15\t35\tb\t2;chr1\t19\t20\tc\t03\n"
     b"chr1\t30\t40\tr2|chr1\t15\t35\tb\t2\n"
     b"chr2\t5\t9\tr3|\n"),
    # every per-line column
    (R1, M1, dict(cols=("count", "indicator", "echo_ref_size", "echo_ref_name", "echo_ref_row_id")),
     b"3|1|10|chr1:10-20|id-1\n1|1|10|chr1:30-40|id-2\n0|0|4|chr2:5-9|id-3\n"),
    # every list column; scores are copied byte for byte
    (R1, M1, dict(cols=("echo_map_id", "echo_map_score", "echo_map_size", "echo_overlap_size", "echo_map_range")),
     b"a;b;c|1.5;2;03|12;20;1|2;5;1|chr1\t0\t35\n"
     b"b|2|20|5|chr1\t15\t35\n"
     b"||||\n"),
    # skip_unmapped, other delimiters
    (R1, M1, dict(cols=("echo_ref_row_id", "echo_map_id"), skip_unmapped=True, delim=b"\t", multidelim=b", "),
     b"id-1\ta, b, c\nid-2\tb\n"),
    # bp_ovr at its boundary: ov of a, b, c is 2, 5, 1
    (R1, M1, dict(cols=("echo_map_id",), criterion=("bp_ovr", 2)), b"a;b\nb\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("bp_ovr", 3)), b"b\nb\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("bp_ovr", 5)), b"b\nb\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("bp_ovr", 6)), b"\n\n\n"),
    # range: abutting lines come in at 1; the overlap is with the window; never below 0
    (R1, M1, dict(cols=("echo_map_id", "echo_overlap_size"), criterion=("range", 1)),
     b"a;b;c|3;6;1\nb;d|6;1\ne|1\n"),
    (R1, M1, dict(cols=("echo_map_id", "echo_overlap_size"), criterion=("range", 100)),
     b"a;b;c;d|12;20;1;10\na;b;c;d|12;20;1;10\ne|4\n"),
    # fraction_ref on a reference line of 10 bases: ov is 2, 5, 1
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_ref", "0.5")), b"b\nb\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_ref", "0.500000001")), b"\n\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_ref", ".2")), b"a;b\nb\n\n"),
    # fraction_map: a 2/12, b 5/20, c 1/1
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_map", "0.25")), b"b;c\nb\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_map", "0.26")), b"c\n\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_map", "1")), b"c\n\n\n"),
    # both and either at 0.25: ref a .2 b .5 c .1; map a .1666 b .25 c 1
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_both", "0.25")), b"b\nb\n\n"),
    (R1, M1, dict(cols=("echo_map_id",), criterion=("fraction_either", "0.25")), b"b;c\nb\n\n"),
    # exact
    (R1, b"chr1\t10\t19\tx\nchr1\t10\t20\ty\nchr1\t10\t20\tz\nchr1\t10\t21\tw\nchr1\t30\t40\tv\n",
     dict(cols=("count", "echo_map_id"), criterion=("exact",)), b"2|y;z\n1|v\n0|\n"),
    # the reference as its own map: every line hits itself
    (b"chr1\t1\t10\tp\nchr1\t5\t6\tq\nchr1\t10\t12\tr\n", None, dict(cols=("echo_ref_row_id", "echo_map_id", "echo_map_range")),
     b"id-1|p;q|chr1\t1\t10\nid-2|p;q|chr1\t1\t10\nid-3|r|chr1\t10\t12\n"),
    # no hits at all, an empty map, an empty reference
    (R1, b"chr1\t20\t30\tn\n", dict(cols=("count", "echo_map", "echo_map_range")), b"0||\n0||\n0||\n"),
    (R1, b"", dict(cols=("indicator",)), b"0\n0\n0\n"),
    (b"", M1, {}, b""),
]
