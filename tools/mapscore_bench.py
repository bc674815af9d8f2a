"""bedmap-scores on one GPU, device bytes in (DESIGN.md "bedmap-scores"): a
generated sorted reference (the cfg2 generator's BED3, gen_bed kind 0) against a
generated sorted map with a score in column 5 (its narrowPeak, gen_bed kind 1),
--lines each, back to back in HBM.  starch_mapsc_device runs over them with
--cols, --criterion, --prec and --kth: --warmup runs, then --reps timed with a
host clock around the call (it ends in a stream synchronise).

One JSON line on stdout: the median, minimum and maximum call time, the median
of every stage time of starch_mapsc_stats over the same runs (device-event
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

STAGES = ("ms_parse", "ms_build", "ms_query", "ms_reduce", "ms_format")


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
    ap.add_argument("--cols", default="echo,mean")
    ap.add_argument("--criterion", default="bp_ovr:1", help=criterion_of.__doc__)
    ap.add_argument("--prec", type=int, default=6)
    ap.add_argument("--kth", default=None, help="a decimal in (0, 1], with the column kth")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mapscore_bench: no GPU")
    cols = tuple(a.cols.split(","))
    crit = criterion_of(a.criterion)
    kinds = (0, 1)
    sizes = [sum(starch_amd.gen_bed_sizes(k, a.lines, seed=s)) for k, s in zip(kinds, a.seeds)]
    host = torch.empty(sum(sizes), dtype=torch.uint8)
    offs = [0, sizes[0], sizes[0] + sizes[1]]
    for kind, s, sz, at in zip(kinds, a.seeds, sizes, offs):
        k = starch_amd.gen_bed(kind, a.lines, seed=s, into=ctypes.c_void_p(host.data_ptr() + at))
        assert k == sz
    dev = host.to("cuda")
    torch.cuda.synchronize()
    del host
    n = offs[-1]
    ctx = starch_amd.Starch(0)
    kw = dict(cols=cols, criterion=crit, prec=a.prec, kth=a.kth)
    for _ in range(a.warmup):
        ctx.map_scores_device(dev.data_ptr(), offs, **kw)
    t, stats = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.map_scores_device(dev.data_ptr(), offs, **kw)
        t.append((time.perf_counter() - t0) * 1e3)
        stats.append(ctx.mapsc_stats())
    med = statistics.median(t)
    last = stats[-1]
    tile, wave = starch_amd.mapsc_constants()
    res = {"cols": cols, "criterion": crit, "prec": a.prec, "kth": a.kth, "lines_per_input": a.lines, "input_bytes": n,
           "tile_hits": tile, "wave_copy_threshold": wave, "warmup": a.warmup, "reps": a.reps,
           "call_ms_median": round(med, 2), "call_ms_min": round(min(t), 2), "call_ms_max": round(max(t), 2),
           "stage_ms_median": {s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
           "ms_reduce_all": [round(x["ms_reduce"], 3) for x in stats],
           "input_gb_s": round(n / med / 1e6, 2),
           "counts": {k: last[k] for k in ("n_ref", "n_map", "n_chromosomes", "hits", "straddling", "sorted_hits",
                                           "radix_passes", "lines_out", "output_bytes")}}
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
