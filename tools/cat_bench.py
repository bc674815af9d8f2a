"""starchcat against the route it replaces, host bytes to host bytes on one GPU
(DESIGN.md §6): 1/8 of cfg2 dealt line by line into two archives, then

  cat       Starch.cat of the two archives (every chromosome is a merge);
  old       unstarch of each archive plus compress of the merged BED (the
            host-side merge of the two BEDs, which that route also needs, is
            left out);
  copy      cat of two archives holding 12 different chromosomes each (every
            chromosome is a copy: no GPU work).

Median of --reps after one warm-up; one JSON line on stdout.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import starch_amd  # noqa: E402


def src_stamp():
    d = os.path.join(ROOT, "starch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp", ".cpp")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 1), [round(x, 1) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=12_500_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = starch_amd.Starch(0)
    bed = starch_amd.gen_bed(0, a.lines)
    lines = bed.split(b"\n")[:-1]
    halves = [b"\n".join(lines[k::2]) + b"\n" for k in (0, 1)]
    del lines
    arch = [ctx.compress(h) for h in halves]
    want = ctx.compress(bed)
    got = ctx.cat(arch)
    assert got == want, "cat differs from compress(merged BED)"
    stats = ctx.cat_stats()
    res = {"stamp": src_stamp(), "lines": a.lines, "bed_bytes": len(bed), "archive_bytes": len(got),
           "input_archive_bytes": [len(x) for x in arch], "cat_stats": stats}
    res["cat_ms"], res["cat_all"] = timed(lambda: ctx.cat(arch), a.reps)

    def old():
        for x in arch:
            ctx.unstarch(x)
        ctx.compress(bed)
    res["old_ms"], res["old_all"] = timed(old, a.reps)
    twelve = [ctx.compress(starch_amd.gen_bed(0, a.lines // 2, chroms=list(range(k, k + 12)))) for k in (0, 12)]
    plan = starch_amd.cat_plan(twelve)
    assert len(plan) == 24 and all(p[1] == "copy" for p in plan)
    res["copy_ms"], res["copy_all"] = timed(lambda: ctx.cat(twelve), a.reps)
    res["copy_stats"] = ctx.cat_stats()
    res["copy_archive_bytes"] = [len(x) for x in twelve]
    res["copy_host_only_ms"], _ = timed(lambda: starch_amd.cat_host(twelve), a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
