"""bedmap-elements on one GPU, device bytes in (DESIGN.md "bedmap-elements"): a
generated sorted reference against a generated sorted map, both the cfg2
generator's BED3 (gen_bed kind 0, two seeds, --lines each; both come out in
sort-bed order), back to back in HBM.  starch_mapel_device runs over them with
--cols and --criterion: --warmup runs, then --reps timed with a host clock
around the call (it ends in a stream synchronise).  --nested puts one line in
front of the map that covers all of chr1, so that every reference line of chr1
has a hit that lies far ahead of its others in the map.

One JSON line on stdout: the median, minimum and maximum call time, the median
of every stage time of starch_mapel_stats over the same runs (device-event
milliseconds), the counts of the last run, and GB/s of input.
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

STAGES = ("ms_parse", "ms_build", "ms_query", "ms_format")
COVER = b"chr1\t0\t2000000000\n"


def criterion_of(text):
    """bp_ovr:N, range:N, fraction_ref:F (and _map, _both, _either) or exact"""
    name, _, value = text.partition(":")
    if name == "exact":
        return (name,)
    return (name, int(value)) if name in ("bp_ovr", "range") else (name, value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000, help="lines per input")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seeds", type=int, nargs=2, default=[20261015, 20261019], help="reference, map")
    ap.add_argument("--cols", default="echo,echo_map")
    ap.add_argument("--criterion", default="bp_ovr:1", help=criterion_of.__doc__)
    ap.add_argument("--nested", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mapel_bench: no GPU")
    cols = tuple(a.cols.split(","))
    crit = criterion_of(a.criterion)
    sizes = [sum(starch_amd.gen_bed_sizes(0, a.lines, seed=s)) for s in a.seeds]
    lead = len(COVER) if a.nested else 0
    host = torch.empty(sum(sizes) + lead, dtype=torch.uint8)
    offs = [0, sizes[0], sizes[0] + lead + sizes[1]]
    for s, sz, at in zip(a.seeds, sizes, (0, sizes[0] + lead)):
        k = starch_amd.gen_bed(0, a.lines, seed=s, into=ctypes.c_void_p(host.data_ptr() + at))
        assert k == sz
    if a.nested:
        ctypes.memmove(host.data_ptr() + sizes[0], COVER, lead)
    dev = host.to("cuda")
    torch.cuda.synchronize()
    del host
    n = offs[-1]
    ctx = starch_amd.Starch(0)
    for _ in range(a.warmup):
        ctx.map_elements_device(dev.data_ptr(), offs, cols=cols, criterion=crit)
    t, stats = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.map_elements_device(dev.data_ptr(), offs, cols=cols, criterion=crit)
        t.append((time.perf_counter() - t0) * 1e3)
        stats.append(ctx.mapel_stats())
    med = statistics.median(t)
    last = stats[-1]
    tile, fanout, heavy, bound = starch_amd.mapel_constants()
    res = {"cols": cols, "criterion": crit, "nested": a.nested, "lines_per_input": a.lines, "input_bytes": n,
           "tile_refs": tile, "fanout": fanout, "heavy_threshold": heavy, "steps_per_hit_bound": bound,
           "warmup": a.warmup, "reps": a.reps,
           "call_ms_median": round(med, 2), "call_ms_min": round(min(t), 2), "call_ms_max": round(max(t), 2),
           "stage_ms_median": {s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
           "ms_query_all": [round(x["ms_query"], 3) for x in stats],
           "input_gb_s": round(n / med / 1e6, 2),
           "counts": {k: last[k] for k in ("n_ref", "n_map", "n_chromosomes", "hits", "heavy_lines", "walk_steps",
                                           "lines_out", "output_bytes")}}
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
