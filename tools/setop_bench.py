"""The bedops set operations on one GPU, device bytes in (DESIGN.md "bedops set
operations"): two inputs of the cfg2 generator's BED3 (gen_bed kind 0, two
seeds, --lines each; both come out in sort-bed order) lie back to back in HBM,
and starch_setop_device runs each of the five ops over them: --warmup runs,
then --reps timed with a host clock around the call (it ends in a stream
synchronise).

Per op one JSON line on stdout: the median, minimum and maximum call time, the
median of every stage time of starch_setop_stats over the same runs
(device-event milliseconds), the counts of the last run, GB/s of input, and
the time a plain copy of the input (read once, written once) would take at
--copy-gb-s, for scale.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starch_amd  # noqa: E402

STAGES = ("ms_parse", "ms_merge", "ms_sort", "ms_sweep", "ms_format")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=12_500_000, help="lines per input")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seeds", type=int, nargs=2, default=[20261015, 20261019])
    ap.add_argument("--copy-gb-s", type=float, default=4000.0, help="HBM copy rate assumed for the copy bound")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("setop_bench: no GPU")
    sizes = [sum(starch_amd.gen_bed_sizes(0, a.lines, seed=s)) for s in a.seeds]
    host = torch.empty(sum(sizes), dtype=torch.uint8)
    offs = [0]
    for s, sz in zip(a.seeds, sizes):
        k = starch_amd.gen_bed(0, a.lines, seed=s, into=ctypes.c_void_p(host.data_ptr() + offs[-1]))
        assert k == sz
        offs.append(offs[-1] + sz)
    dev = host.to("cuda")
    torch.cuda.synchronize()
    del host
    n = offs[-1]
    ctx = starch_amd.Starch(0)
    for op in starch_amd.SETOPS:
        for _ in range(a.warmup):
            ctx.setop_device(op, dev.data_ptr(), offs)
        t, stats = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.setop_device(op, dev.data_ptr(), offs)
            t.append((time.perf_counter() - t0) * 1e3)
            stats.append(ctx.setop_stats())
        med = statistics.median(t)
        last = stats[-1]
        res = {"op": op, "lines_per_input": a.lines, "input_bytes": n, "tile_lines": starch_amd.setop_constants(),
               "warmup": a.warmup, "reps": a.reps,
               "call_ms_median": round(med, 2), "call_ms_min": round(min(t), 2), "call_ms_max": round(max(t), 2),
               "stage_ms_median": {s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
               "input_gb_s": round(n / med / 1e6, 2),
               "copy_bound_ms": round(2 * n / a.copy_gb_s / 1e6, 3),
               "counts": {k: last[k] for k in ("n_lines", "n_chromosomes", "runs_merged", "groups", "lines_out",
                                               "output_bytes", "radix_passes")}}
        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
