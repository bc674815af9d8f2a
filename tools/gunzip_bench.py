"""The inflater on one GPU against CPython's zlib on the host (DESIGN.md section
20): --lines lines of the project's generated BED are written as BGZF (zlib
level 6, 65280-byte blocks, the end-of-file block) and as one `gzip -6` member.
Starch.gunzip runs over each from host memory: --warmup runs, then --reps timed
through gunzip_stats() (device-event milliseconds per stage; ms_plan is host
clock).  In the same run zlib inflates the same BGZF blocks on 1 and on
--threads host threads (zlib releases the GIL), timed with a host clock.

One JSON line on stdout: the sizes, the median of every stage, GB/s of inflated
bytes over ms_inflate + ms_crc (BGZF) and over ms_size + ms_inflate + ms_crc
(generic), and the host figures.  The generic member is cut to --generic-mib
MiB of text: one wave decodes it.
"""
import argparse
import concurrent.futures
import gzip
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starch_amd  # noqa: E402

STAGES = ("ms_plan", "ms_upload", "ms_size", "ms_inflate", "ms_crc")
BLOCK = 65280


def bgzf(text, level=6):
    out, blocks = bytearray(), []
    for i in range(0, len(text), BLOCK):
        piece = text[i:i + BLOCK]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = c.compress(piece) + c.flush()
        blocks.append(raw)
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw + \
            struct.pack("<II", zlib.crc32(piece), len(piece))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return bytes(out), blocks


def timed(ctx, data, warmup, reps):
    for _ in range(warmup):
        ctx.gunzip(data)
    stats = []
    for _ in range(reps):
        ctx.gunzip(data)
        stats.append(ctx.gunzip_stats())
    return {s: round(statistics.median(x[s] for x in stats), 3) for s in STAGES}, stats[-1]


def host_inflate(blocks, threads, reps):
    def one(lo, hi):
        return sum(len(zlib.decompress(b, -15)) for b in blocks[lo:hi])
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        if threads == 1:
            one(0, len(blocks))
        else:
            step = (len(blocks) + threads - 1) // threads
            with concurrent.futures.ThreadPoolExecutor(threads) as ex:
                list(ex.map(lambda k: one(k * step, (k + 1) * step), range(threads)))
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--generic-mib", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gunzip_bench: no GPU")
    text = bytes(starch_amd.gen_bed(a.kind, a.lines))
    z, blocks = bgzf(text)
    gtext = text[:a.generic_mib << 20]
    g = gzip.compress(gtext, 6)
    ctx = starch_amd.Starch(0)
    assert ctx.gunzip(z) == text and ctx.gunzip(g) == gtext
    bs, blast = timed(ctx, z, a.warmup, a.reps)
    gs, glast = timed(ctx, g, a.warmup, a.reps)
    h1 = host_inflate(blocks, 1, max(1, a.reps // 2))
    hn = host_inflate(blocks, a.threads, a.reps)
    res = dict(lines=a.lines, kind=a.kind, text_bytes=len(text), bgzf_bytes=len(z), bgzf_members=blast["members"],
               generic_text_bytes=len(gtext), generic_bytes=len(g), constants=starch_amd.gunzip_constants(),
               warmup=a.warmup, reps=a.reps, bgzf_stage_ms_median=bs, generic_stage_ms_median=gs,
               bgzf_blocks=[blast[k] for k in ("stored_blocks", "fixed_blocks", "dynamic_blocks")],
               gpu_bgzf_gb_s=round(len(text) / (bs["ms_inflate"] + bs["ms_crc"]) / 1e6, 2),
               gpu_bgzf_inflate_only_gb_s=round(len(text) / bs["ms_inflate"] / 1e6, 2),
               gpu_generic_gb_s=round(len(gtext) / (gs["ms_size"] + gs["ms_inflate"] + gs["ms_crc"]) / 1e6, 3),
               host_threads=a.threads, host_1_thread_ms=round(h1, 1), host_n_threads_ms=round(hn, 1),
               host_1_thread_gb_s=round(len(text) / h1 / 1e6, 3), host_n_threads_gb_s=round(len(text) / hn / 1e6, 3))
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
