"""Two plain-Python oracles for the bedops set operations (merge, intersect,
difference, symmdiff, complement) as include/starch_amd.h defines them.  They
take nothing from the code under test and share no method with it or with
each other:

  bitmap(op, inputs)  coordinates below 4096: one numpy bool array per input
                      and chromosome, the op as a boolean expression over
                      them, the runs of True written as BED3.
  sweep(op, inputs)   any coordinates: a dict from (chrom, position) to
                      per-input deltas, walked in order with a per-input depth
                      list (not a weighted sum).

inputs: a list of bytes, BED text; both return the expected BED3 bytes.
"""
import functools

import numpy as np

OPS = ("merge", "intersect", "difference", "symmdiff", "complement")
LIMIT = 4096


@functools.lru_cache(maxsize=512)
def parse(bed):
    """((chrom bytes, start, stop), ...) of BED text (a last line without newline is a line)."""
    out = []
    for ln in bed.split(b"\n"):
        if ln == b"":
            continue
        f = ln.split(b"\t")
        out.append((f[0], int(f[1]), int(f[2])))
    return tuple(out)


def bed3(rows):
    return b"".join(b"%s\t%d\t%d\n" % r for r in rows)


def _holds(op, covered):
    """The set definition for one base: covered[k] is whether input k covers it."""
    n = sum(covered)
    if op == "merge":
        return n >= 1
    if op == "intersect":
        return n == len(covered)
    if op == "difference":
        return covered[0] and n == 1
    if op == "symmdiff":
        return n == 1
    raise ValueError(op)


def bitmap(op, inputs):
    parsed = [parse(b) for b in inputs]
    chroms = sorted({c for p in parsed for c, _, _ in p})
    rows = []
    for c in chroms:
        maps = []
        for p in parsed:
            m = np.zeros(LIMIT + 1, dtype=bool)
            for cc, s, t in p:
                if cc == c:
                    assert 0 <= s < t <= LIMIT
                    m[s:t] = True
            maps.append(m)
        stack = np.stack(maps)
        count = stack.sum(axis=0)
        if op == "merge":
            r = count >= 1
        elif op == "intersect":
            r = count == len(maps)
        elif op == "difference":
            r = stack[0] & (count == 1)
        elif op == "symmdiff":
            r = count == 1
        elif op == "complement":
            union = count >= 1
            on = np.flatnonzero(union)
            r = ~union
            r[:on[0]] = False       # clipped to the union's first and last set base
            r[on[-1]:] = False
        else:
            raise ValueError(op)
        d = np.diff(np.concatenate(([0], r.astype(np.int8), [0])))
        for s, t in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            rows.append((c, int(s), int(t)))
    return bed3(rows)


def sweep(op, inputs):
    parsed = [parse(b) for b in inputs]
    n = len(parsed)
    delta = {}
    for k, p in enumerate(parsed):
        for c, s, t in p:
            delta.setdefault((c, s), [0] * n)[k] += 1
            delta.setdefault((c, t), [0] * n)[k] -= 1
    rows = []
    depth = [0] * n
    cur_chrom, run_start = None, None
    keys = sorted(delta)
    for i, (c, pos) in enumerate(keys):
        if c != cur_chrom:
            assert run_start is None and not any(depth)
            cur_chrom = c
        for k in range(n):
            depth[k] += delta[(c, pos)][k]
        last_of_chrom = i + 1 == len(keys) or keys[i + 1][0] != c
        covered = [d > 0 for d in depth]
        if op == "complement":
            on = not any(covered) and not last_of_chrom   # inside [smallest start, largest stop)
        else:
            on = _holds(op, covered)
        if on and run_start is None:
            run_start = pos
        elif not on and run_start is not None:
            rows.append((c, run_start, pos))
            run_start = None
    return bed3(rows)


def _b(*iv, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % (chrom, s, t) for s, t in iv)


_SAME = _b((100, 200))
# hand-written expectations: (inputs, {op: expected output})
TABLE = [
    ([_b((0, 10), (10, 20)), _b((20, 30))],
     {"merge": _b((0, 30)), "intersect": b"", "symmdiff": _b((0, 30)), "difference": _b((0, 20)), "complement": b""}),
    ([_b((0, 30)), _b((10, 20))],
     {"difference": _b((0, 10), (20, 30)), "intersect": _b((10, 20)), "symmdiff": _b((0, 10), (20, 30)),
      "complement": b"", "merge": _b((0, 30))}),
    ([_b((5, 8)), _b((20, 25)), _b((1, 2), chrom=b"chr2")],
     {"complement": _b((8, 20)), "merge": _b((5, 8), (20, 25)) + _b((1, 2), chrom=b"chr2")}),
    ([_SAME, _SAME, _SAME],
     {"intersect": _SAME, "merge": _SAME, "symmdiff": b"", "difference": b""}),
    ([_b((1, 5), (7, 9)) + _b((3, 6), chrom=b"chr2"), _b((2, 4), chrom=b"chr10") + _b((4, 8), chrom=b"chr2")],
     {"difference": _b((1, 5), (7, 9)) + _b((3, 4), chrom=b"chr2"),
      "merge": _b((1, 5), (7, 9)) + _b((2, 4), chrom=b"chr10") + _b((3, 8), chrom=b"chr2")}),
]
