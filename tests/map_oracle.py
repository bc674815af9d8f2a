"""Two plain-Python oracles for bedmap as include/starch_amd.h defines it.  They
take nothing from the code under test and share no method with it:

  pairs(ref, map, ...)   any coordinates: a double loop over reference and map
                         lines; BASES_UNIQ from the union of the clipped map
                         lines, merged in a sorted list.
  bitmap(ref, map, ...)  coordinates below 4096: one numpy depth array per
                         chromosome; BASES is the sum of the depth over the
                         window, BASES_UNIQ the number of its non-zero entries,
                         COUNT comes from the pairs.

Both take BED text (bytes) and return the expected output bytes.  Values are
reduced modulo 2^64 as the header says.  TABLE holds hand-written cases.
"""
import numpy as np

COLS = ("echo", "count", "bases", "bases_uniq", "indicator", "echo_ref_size")
LIMIT = 4096
M64 = (1 << 64) - 1


def parse(bed):
    """[(whole line, chrom, start, stop), ...] (a last line without newline is a line)."""
    out = []
    for ln in bed.split(b"\n"):
        if ln == b"":
            continue
        f = ln.split(b"\t")
        out.append((ln, f[0], int(f[1]), int(f[2])))
    return out


def _window(s, e, rng):
    return max(0, s - rng), min(e + rng, M64)


def _by_chrom(lines):
    out = {}
    for _, c, a, b in lines:
        out.setdefault(c, []).append((a, b))
    return out


def _emit(rows, cols, skip_unmapped, delim):
    """rows: one dict per reference line, keyed by column name."""
    out = []
    for r in rows:
        if skip_unmapped and r["count"] == 0:
            continue
        out.append(delim.join(r[c] if c == "echo" else b"%d" % (r[c] & M64) for c in cols) + b"\n")
    return b"".join(out)


def pairs(ref, map=None, cols=("echo", "count"), range=0, skip_unmapped=False, delim=b"|"):
    R = parse(ref)
    M = _by_chrom(R if map is None else parse(map))
    rows = []
    for line, c, s, e in R:
        ws, we = _window(s, e, range)
        count = bases = 0
        pieces = []
        for a, b in M.get(c, ()):
            if a < we and b > ws:
                count += 1
                lo, hi = max(a, ws), min(b, we)
                bases += hi - lo
                pieces.append((lo, hi))
        uniq, end = 0, None
        for lo, hi in sorted(pieces):
            if end is None or lo > end:
                uniq += hi - lo
                end = hi
            elif hi > end:
                uniq += hi - end
                end = hi
        rows.append({"echo": line, "count": count, "bases": bases, "bases_uniq": uniq, "indicator": 1 if count else 0,
                     "echo_ref_size": e - s})
    return _emit(rows, cols, skip_unmapped, delim)


def bitmap(ref, map=None, cols=("echo", "count"), range=0, skip_unmapped=False, delim=b"|"):
    R = parse(ref)
    M = _by_chrom(R if map is None else parse(map))
    depth = {}
    for mc, ivs in M.items():
        d = depth[mc] = np.zeros(LIMIT, dtype=np.int64)
        for a, b in ivs:
            assert b <= LIMIT
            d[a:b] += 1
    rows = []
    for line, c, s, e in R:
        ws, we = _window(s, e, range)
        d = depth.get(c)
        seen = d[ws:min(we, LIMIT)] if d is not None else np.zeros(0, dtype=np.int64)
        count = sum(1 for a, b in M.get(c, ()) if a < we and b > ws)
        rows.append({"echo": line, "count": count, "bases": int(seen.sum()), "bases_uniq": int(np.count_nonzero(seen)),
                     "indicator": 1 if count else 0, "echo_ref_size": e - s})
    return _emit(rows, cols, skip_unmapped, delim)


# (ref, map or None, keyword arguments, expected bytes), worked out by hand
TABLE = [
    # one reference line over three map lines, two of them overlapping each other
    (b"chr1\t10\t20\n", b"chr1\t0\t12\nchr1\t11\t15\nchr1\t18\t30\nchr1\t20\t40\n",
     dict(cols=COLS), b"chr1\t10\t20|3|8|7|1|10\n"),
    # nested map lines: 5..25 holds 8..12; bases counts both, bases_uniq once
    (b"chr1\t10\t20\tname\t7\n", b"chr1\t5\t25\nchr1\t8\t12\n",
     dict(cols=("count", "bases", "bases_uniq", "echo")), b"2|12|10|chr1\t10\t20\tname\t7\n"),
    # abutting on both sides: nothing overlaps; with range 1 both do, one base each
    (b"chr1\t10\t20\n", b"chr1\t0\t10\nchr1\t20\t30\n", dict(cols=("count", "bases", "indicator")), b"0|0|0\n"),
    (b"chr1\t10\t20\n", b"chr1\t0\t10\nchr1\t20\t30\n", dict(cols=("count", "bases", "echo_ref_size"), range=1), b"2|2|10\n"),
    # the window clamps at 0
    (b"chr1\t3\t5\n", b"chr1\t0\t1\nchr1\t104\t200\nchr1\t105\t300\n", dict(cols=("count", "bases_uniq"), range=100),
     b"2|2\n"),
    # chromosomes: chr10 sorts before chr2; chr3 is not in the map, chrX not in the reference
    (b"chr1\t0\t5\nchr10\t0\t5\nchr2\t0\t5\nchr3\t0\t5\n", b"chr1\t1\t2\nchr2\t0\t9\nchr2\t4\t5\nchrX\t0\t5\n",
     dict(cols=("echo", "count", "bases"), delim=b"::"),
     b"chr1\t0\t5::1::1\nchr10\t0\t5::0::0\nchr2\t0\t5::2::6\nchr3\t0\t5::0::0\n"),
    # skip_unmapped, and a reference mapped onto itself
    (b"chr1\t0\t5\nchr1\t7\t9\nchr2\t1\t2\n", b"chr1\t8\t20\n", dict(cols=("echo", "count"), skip_unmapped=True),
     b"chr1\t7\t9|1\n"),
    (b"chr1\t0\t5\nchr1\t3\t9\nchr1\t9\t12\n", None, dict(cols=("count", "bases", "bases_uniq")), b"2|7|5\n2|8|6\n1|3|3\n"),
]
