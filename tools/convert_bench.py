"""convert2bed on one GPU, device bytes in (DESIGN.md "convert2bed"): a generated
input of --lines records in --format (GFF3 genes, GTF exons, VCF calls with
--samples sample columns, or WIG fixedStep sections of 10,000 values), uploaded
once.  starch_convert_device runs over it: --warmup runs, then --reps timed with
a host clock around the call (it ends in a stream synchronise).  The records
are generated in descending position, so the sort that follows the conversion
has work to do; --no-sort leaves it out.

One JSON line on stdout: the median, minimum and maximum call time, the median
of every stage time of starch_convert_stats over the same runs (device-event
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


def generate(fmt, lines, samples):
    chrom = lambda k: starch_amd.HG38[k % 24].encode()   # noqa: E731
    if fmt in ("gff", "gtf"):
        attrs = b"ID=gene%d;Name=G%d;biotype=protein_coding" if fmt == "gff" else b'gene_id "gene%d"; transcript_id "t%d"; gene_biotype "protein_coding";'
        rows = (b"%s\tbench\tgene\t%d\t%d\t.\t+\t.\t%s" % (chrom(k), 3 * (lines - k) + 1, 3 * (lines - k) + 900, attrs % (k, k))
                for k in range(lines))
        return b"##gff-version 3\n" + b"\n".join(rows) + b"\n"
    if fmt == "vcf":
        tail = b"\tGT" + b"".join(b"\t%d|%d" % (s & 1, s >> 1 & 1) for s in range(samples)) if samples else b""
        rows = (b"%s\t%d\trs%d\tAC\tA,GT,ACG\t50\tPASS\tDP=%d%s" % (chrom(k), 2 * (lines - k), k, k % 100, tail) for k in range(lines))
        return b"##fileformat=VCFv4.2\n" + b"\n".join(rows) + b"\n"
    out = [b"track type=wiggle_0\n"]
    for k in range(0, lines, 10000):
        out.append(b"fixedStep chrom=%s start=%d step=5 span=5\n" % (chrom(k // 10000), 5 * (lines - k) + 1))
        out.append(b"".join(b"%d.25\n" % (v % 100) for v in range(k, min(k + 10000, lines))))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=sorted(starch_amd.CONVERT_FORMATS), default="gff")
    ap.add_argument("--lines", type=int, default=5_000_000)
    ap.add_argument("--samples", type=int, default=0, help="vcf: sample columns per record")
    ap.add_argument("--vcf-class", choices=sorted(starch_amd.VCF_CLASSES), default="all")
    ap.add_argument("--keep-header", action="store_true")
    ap.add_argument("--no-sort", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("convert_bench: no GPU")
    data = generate(a.format, a.lines, a.samples)
    n = len(data)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    del data
    kw = dict(vcf_class=a.vcf_class, keep_header=a.keep_header, sort=not a.no_sort)
    ctx = starch_amd.Starch(0)
    for _ in range(a.warmup):
        ctx.convert_device(dev.data_ptr(), n, a.format, **kw)
    t, stats = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.convert_device(dev.data_ptr(), n, a.format, **kw)
        t.append((time.perf_counter() - t0) * 1e3)
        stats.append(ctx.convert_stats())
    med = statistics.median(t)
    last = stats[-1]
    block, wave_copy = starch_amd.convert_constants()
    res = dict(kw, format=a.format, lines=a.lines, samples=a.samples, input_bytes=n, block_lines=block, wave_copy_bytes=wave_copy,
               warmup=a.warmup, reps=a.reps,
               call_ms_median=round(med, 2), call_ms_min=round(min(t), 2), call_ms_max=round(max(t), 2),
               stage_ms_median={s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
               input_gb_s=round(n / med / 1e6, 2),
               counts={k: last[k] for k in ("input_lines", "header_lines", "data_lines", "declarations", "lines_out",
                                            "output_bytes", "sorted")})
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
