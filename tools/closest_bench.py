"""closest-features on one GPU, device bytes in (DESIGN.md "closest-features"):
a generated sorted reference against a generated sorted query, both the cfg2
generator's BED3 (gen_bed kind 0, two seeds, --lines each; both come out in
sort-bed order), back to back in HBM.  starch_closest_device runs over them:
--warmup runs, then --reps timed with a host clock around the call (it ends in a
stream synchronise).  The generator's lines overlap and nest; --flat replaces
the query by equally wide lines spread over hg38, none nested in another (the
stops are then in order as they stand).  --nested puts one line in front of every chromosome of
the query that covers all of it, so that every other query line is nested in
one and the search for the last overlapping line has to climb the hierarchy.

One JSON line on stdout: the median, minimum and maximum call time, the median
of every stage time of starch_closest_stats over the same runs (device-event
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


def cover_chromosomes(bed):
    """bed (the generator's sorted BED bytes) with `name 0 2000000000` ahead of every chromosome."""
    cuts = []
    for name in starch_amd.HG38:
        key = name.encode() + b"\t"
        at = 0 if bed.startswith(key) else bed.find(b"\n" + key) + 1
        if at or bed.startswith(key):
            cuts.append((at, key))
    cuts.sort()
    out = []
    for (at, key), end in zip(cuts, [c[0] for c in cuts[1:]] + [len(bed)]):
        out.append(key + b"0\t2000000000\n")
        out.append(bed[at:end])
    return b"".join(out)


def flat_bed(lines, seed, width=600):
    """About `lines` sorted hg38 BED3 lines of one width, spread by chromosome
    length: stops rise with starts, so no line is nested in another."""
    import numpy as np
    rng = np.random.default_rng(seed)
    total = sum(starch_amd.HG38_LEN)
    out = []
    for name, size in zip(starch_amd.HG38, starch_amd.HG38_LEN):
        starts = np.sort(rng.integers(1, size - width, size=lines * size // total))
        key = name.encode()
        out.append(b"".join(b"%s\t%d\t%d\n" % (key, s, s + width) for s in starts.tolist()))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000, help="lines per input")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seeds", type=int, nargs=2, default=[20261015, 20261019], help="reference, query")
    ap.add_argument("--closest", action="store_true")
    ap.add_argument("--dist", action="store_true")
    ap.add_argument("--no-overlaps", action="store_true")
    ap.add_argument("--flat", action="store_true", help="a query of equally wide lines, none nested in another")
    ap.add_argument("--nested", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("closest_bench: no GPU")
    parts = []
    for s in a.seeds:
        sz = sum(starch_amd.gen_bed_sizes(0, a.lines, seed=s))
        buf = ctypes.create_string_buffer(sz)
        assert starch_amd.gen_bed(0, a.lines, seed=s, into=ctypes.c_void_p(ctypes.addressof(buf))) == sz
        parts.append(buf.raw)
        del buf
    if a.flat:
        parts[1] = flat_bed(a.lines, a.seeds[1])
    if a.nested:
        parts[1] = cover_chromosomes(parts[1])
    offs = [0, len(parts[0]), len(parts[0]) + len(parts[1])]
    dev = torch.frombuffer(bytearray(parts[0] + parts[1]), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    del parts
    n = offs[-1]
    kw = dict(closest=a.closest, dist=a.dist, no_overlaps=a.no_overlaps)
    ctx = starch_amd.Starch(0)
    for _ in range(a.warmup):
        ctx.closest_device(dev.data_ptr(), offs, **kw)
    t, stats = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.closest_device(dev.data_ptr(), offs, **kw)
        t.append((time.perf_counter() - t0) * 1e3)
        stats.append(ctx.closest_stats())
    med = statistics.median(t)
    last = stats[-1]
    tile, fanout = starch_amd.closest_constants()
    res = dict(kw, flat=a.flat, nested=a.nested, lines_per_input=a.lines, input_bytes=n, tile_refs=tile, fanout=fanout,
               warmup=a.warmup, reps=a.reps,
               call_ms_median=round(med, 2), call_ms_min=round(min(t), 2), call_ms_max=round(max(t), 2),
               stage_ms_median={s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
               ms_query_all=[round(x["ms_query"], 3) for x in stats],
               input_gb_s=round(n / med / 1e6, 2),
               counts={k: last[k] for k in ("n_ref", "n_query", "n_chromosomes", "stops_sorted", "left_na", "right_na",
                                            "lines_out", "output_bytes")})
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
