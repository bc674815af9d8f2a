"""sam2bed, psl2bed and rmsk2bed on one GPU, device bytes in (DESIGN.md section
18): a generated input of --lines records in --format (150-base SAM reads, a
fifth of them spliced; PSL alignments of three blocks; RepeatMasker lines),
uploaded once.  starch_align_device runs over it: --warmup runs, then --reps
timed with a host clock around the call (it ends in a stream synchronise).  The
records are generated in descending position, so the sort that follows the
conversion has work to do; --no-sort leaves it out.

One JSON line on stdout: the median, minimum and maximum call time, the median
of every stage time of starch_align_stats over the same runs (device-event
milliseconds), the counts of the last run, and GB/s of input.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starch_amd  # noqa: E402

STAGES = ("ms_frame", "ms_parse", "ms_write", "ms_sort")


def generate(fmt, lines):
    chrom = lambda k: starch_amd.HG38[k % 24].encode()   # noqa: E731
    if fmt == "sam":
        seq, qual = b"ACGTTGCA" * 19, b"FFFFFFF:" * 19   # 152 bases; the CIGARs below consume 150 or 152
        seq, qual = seq[:150], qual[:150]
        rows = (b"read%d\t%d\t%s\t%d\t60\t%s\t=\t%d\t300\t%s\t%s\tNM:i:1\tAS:i:148"
                % (k, (0, 16, 99, 147)[k & 3], chrom(k), 3 * (lines - k) + 1, b"70M1200N80M" if k % 5 == 0 else b"150M", 3 * (lines - k) + 301,
                   seq, qual) for k in range(lines))
        return b"@HD\tVN:1.6\tSO:unsorted\n" + b"\n".join(rows) + b"\n"
    if fmt == "psl":
        rows = (b"290\t8\t0\t0\t1\t2\t2\t400\t+\tquery%d\t320\t10\t310\t%s\t250000000\t%d\t%d\t3\t100,100,98,\t10,110,212,\t%d,%d,%d,"
                % (k, chrom(k), 3 * (lines - k), 3 * (lines - k) + 698, 3 * (lines - k), 3 * (lines - k) + 300, 3 * (lines - k) + 600)
                for k in range(lines))
        return b"psLayout version 3\n\nmatch\tmis- \trep. \tN's\n" + b"-" * 80 + b"\n" + b"\n".join(rows) + b"\n"
    head = (b"   SW  perc perc perc  query      position in query           matching       repeat              position in  repeat\n"
            b"score  div. del. ins.  sequence    begin     end    (left)    repeat         class/family         begin  end (left)   ID\n\n")
    rows = (b"%5d  11.5  6.2  0.0  %-5s  %9d %9d (%d) %s  AluSx           SINE/Alu               1  310    (2) %6d"
            % (300 + k % 4000, chrom(k), 3 * (lines - k) + 1, 3 * (lines - k) + 310, 250000000 - 3 * (lines - k), b"+C"[k & 1:][:1], k)
            for k in range(lines))
    return head + b"\n".join(rows) + b"\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=sorted(starch_amd.ALIGN_FORMATS), default="sam")
    ap.add_argument("--lines", type=int, default=5_000_000)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--keep-header", action="store_true")
    ap.add_argument("--no-sort", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("align_bench: no GPU")
    data = generate(a.format, a.lines)
    n = len(data)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    del data
    kw = dict(split=a.split, keep_header=a.keep_header, sort=not a.no_sort)
    ctx = starch_amd.Starch(0)
    for _ in range(a.warmup):
        ctx.align2bed_device(dev.data_ptr(), n, a.format, **kw)
    t, stats = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.align2bed_device(dev.data_ptr(), n, a.format, **kw)
        t.append((time.perf_counter() - t0) * 1e3)
        stats.append(ctx.align_stats())
    med = statistics.median(t)
    last = stats[-1]
    block, wave_copy = starch_amd.align_constants()
    res = dict(kw, format=a.format, lines=a.lines, input_bytes=n, block_lines=block, wave_copy_bytes=wave_copy,
               warmup=a.warmup, reps=a.reps,
               call_ms_median=round(med, 2), call_ms_min=round(min(t), 2), call_ms_max=round(max(t), 2),
               stage_ms_median={s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
               input_gb_s=round(n / med / 1e6, 2),
               counts={k: last[k] for k in ("input_lines", "header_lines", "records", "unmapped_dropped", "lines_out",
                                            "output_bytes", "sorted")})
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
