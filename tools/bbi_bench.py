"""bigwig2bed / bigbed2bed on one GPU, host bytes in: a
generated file of --blocks blocks written with tests/bbi_writer.py -- bigWig
(--kind bigwig): bedGraph sections of --items items on 24 chromosomes; bigBed:
blocks of --items records with a name, a score and a strand -- compressed with
Python's zlib at --level, or left uncompressed with --level 0.  starch_bbi_host
runs over it: --warmup runs, then --reps timed with a host clock around the call
(host reading of the trees, upload, inflate, Adler-32, records, sort).

One JSON line on stdout: the sizes, the median, minimum and maximum call time,
the median of every stage time of starch_bbi_stats over the same runs
(device-event milliseconds), the counts of the last run, and GB/s of inflated
bytes.  Not a test: nothing asserts on its figures.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import starch_amd  # noqa: E402
from tests import bbi_writer as W  # noqa: E402

STAGES = ("ms_upload", "ms_size", "ms_inflate", "ms_adler", "ms_frame", "ms_parse", "ms_write", "ms_sort")
CHROMS = 24


def generate(kind, blocks, items, level):
    chroms = [(starch_amd.HG38[k].encode(), starch_amd.HG38_LEN[k]) for k in range(CHROMS)]
    out = []
    for b in range(blocks):
        c = b * CHROMS // blocks
        base = (blocks - b) * items * 30                     # descending, so that the sort has work to do
        if kind == "bigwig":
            sec = W.wig_section(c, [(base + 25 * k, base + 25 * k + 20, (b * 31 + k) % 1000 / 8) for k in range(items)], type_=1)
            out.append(W.Block(sec, W.wig_box(sec), level=level))
        else:
            recs = [(c, base + 25 * k, base + 25 * k + 20, b"item%d.%d\t%d\t%s" % (b, k, k % 1000, b"+-"[k & 1:][:1])) for k in range(items)]
            out.append(W.Block(W.bed_block(recs), W.bed_box(recs), level=level))
    return W.write(kind, chroms, out, ubs=None if level else 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--kind", choices=("bigwig", "bigbed"), default="bigwig")
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sort", action="store_true")
    a = ap.parse_args()
    data = generate(a.kind, a.blocks, a.items, a.level)
    ctx = starch_amd.Starch(0)
    times, stages, st = [], {s: [] for s in STAGES}, {}
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out = ctx.bbi2bed(data, sort=not a.no_sort)
        dt = (time.perf_counter() - t0) * 1e3
        st = ctx.bbi_stats()
        if r >= a.warmup:
            times.append(dt)
            for s in STAGES:
                stages[s].append(st[s])
    ctx.close()
    med = statistics.median(times)
    print(json.dumps(dict(kind=a.kind, blocks=a.blocks, items=a.items, level=a.level, sorted=not a.no_sort, file_bytes=len(data),
                          inflated_bytes=st["inflated_bytes"], records=st["records"], lines_out=st["lines_out"], output_bytes=len(out),
                          ms_call_median=med, ms_call_min=min(times), ms_call_max=max(times),
                          stage_ms={s: statistics.median(v) for s, v in stages.items()},
                          inflated_gb_per_s=st["inflated_bytes"] / med / 1e6, includes_python_output_copy=True)))


if __name__ == "__main__":
    main()
