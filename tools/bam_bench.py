"""bam2bed on one GPU, host bytes in: a generated BAM of
--records 150-base reads (a fifth of them spliced, two tags and a small B array
each, in descending position so that the sort has work to do), framed as BGZF
with Python's zlib at --level in 65,280-byte blocks that ignore the record
boundaries.  starch_bam_host runs over it: --warmup runs, then --reps timed with
a host clock around the call (upload, inflate, framing, conversion, sort).

One JSON line on stdout: the sizes, the median, minimum and maximum call time,
the median of every stage time of starch_bam_stats over the same runs
(device-event milliseconds), the counts of the last run, and GB/s of inflated
bytes.
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import starch_amd  # noqa: E402

STAGES = ("ms_inflate", "ms_frame", "ms_parse", "ms_write", "ms_sort")
CHROMS = 24


def generate(records):
    """Inflated BAM."""
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (starch_amd.HG38[k].encode(), starch_amd.HG38_LEN[k])
                                                     for k in range(CHROMS))
    out = [b"BAM\1", struct.pack("<I", len(text)), text, struct.pack("<I", CHROMS)]
    for k in range(CHROMS):
        name = starch_amd.HG38[k].encode() + b"\0"
        out.append(struct.pack("<I", len(name)) + name + struct.pack("<I", starch_amd.HG38_LEN[k]))
    seq = bytes(((1, 2, 4, 8)[j & 3] << 4) | (8, 4, 2, 1)[j & 3] for j in range(75))
    qual = bytes(20 + j % 21 for j in range(150))
    cigars = (struct.pack("<I", 150 << 4), struct.pack("<III", 70 << 4, (1200 << 4) | 3, 80 << 4))
    for k in range(records):
        name = b"read%d\0" % k
        cigar = cigars[k % 5 == 0]
        pos = 3 * (records - k)
        tags = b"NMC\1ASC\x94XBBs" + struct.pack("<Ihhh", 3, -k % 30000, 7, 300) + b"XFf" + struct.pack("<f", 0.125 * (k % 1000))
        body = struct.pack("<iiBBHHHIiii", k % CHROMS, pos, len(name), 60, 4680, len(cigar) // 4, (0, 16, 99, 147)[k & 3], 150,
                           k % CHROMS, pos + 300, 300) + name + cigar + seq + qual + tags
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)


def bgzf(data, level):
    out = []
    for at in range(0, len(data), 65280):
        piece = data[at:at + 65280]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw +
                   struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--reduced", action="store_true")
    ap.add_argument("--no-sort", action="store_true")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    data = generate(a.records)
    z = bgzf(data, a.level)
    n = len(data)
    del data
    kw = dict(split=a.split, reduced=a.reduced, sort=not a.no_sort)
    ctx = starch_amd.Starch(0)
    for _ in range(a.warmup):
        ctx.bam2bed(z, **kw)
    t, stats = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.bam2bed(z, **kw)
        t.append((time.perf_counter() - t0) * 1e3)
        stats.append(ctx.bam_stats())
    med = statistics.median(t)
    last = stats[-1]
    tile, block, wave = starch_amd.bam_constants()
    res = dict(kw, records=a.records, level=a.level, bgzf_bytes=len(z), inflated_bytes=n, tile_bytes=tile, block_records=block,
               wave_threshold=wave, warmup=a.warmup, reps=a.reps,
               call_ms_median=round(med, 2), call_ms_min=round(min(t), 2), call_ms_max=round(max(t), 2),
               stage_ms_median={s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES},
               inflated_gb_s=round(n / med / 1e6, 2),
               counts={k: last[k] for k in ("references", "header_lines", "records", "unmapped_dropped", "tiles", "wave_records",
                                            "lines_out", "output_bytes", "sorted")})
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
