"""sort-bed on one GPU, device bytes to device bytes (DESIGN.md "sort-bed"):
the cfg2 generator's BED3 at 1/8 size and at full size, its lines shuffled on
the device with a seeded torch permutation, then starch_sort_device timed with
a host clock around the call (it ends in a stream synchronise): --warmup runs,
then the median, minimum and maximum of --reps.  The sorted output must equal
the generator's own bytes (which are in sort-bed order).

Per size one JSON line on stdout: the call times, starch_sort_stats of the
last run (device-event milliseconds per stage, radix_passes), GB/s of input,
and the bytes each stage has to move (computed here from the line count and
the pass count) over its stage time.  --cpu-sort also writes the shuffled
file and times `LC_ALL=C sort -s -k1,1 -k2,2n -k3,3n --parallel=16` on it,
for scale.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import starch_amd  # noqa: E402


def shuffled_on_device(total_lines, seed, dev="cuda"):
    """(generator's bytes, the same lines shuffled, line count); uint8 tensors on the device"""
    size = sum(starch_amd.gen_bed_sizes(0, total_lines))
    host = torch.empty(size, dtype=torch.uint8)
    k = starch_amd.gen_bed(0, total_lines, into=ctypes.c_void_p(host.data_ptr()))
    assert k == size
    src = host.to(dev)
    del host
    piece = 1 << 30                                           # (nonzero over 2^31 elements or more fails)
    ends = torch.cat([torch.nonzero(src[o:o + piece] == 10).flatten() + (o + 1)
                      for o in range(0, size, piece)])        # one past every '\n'
    begs = torch.cat([ends.new_zeros(1), ends[:-1]])
    lens = ends - begs
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    perm = torch.randperm(ends.numel(), device=dev, generator=g)
    plen = lens[perm]
    dst_end = torch.cumsum(plen, 0)
    shift = begs[perm] - (dst_end - plen)                     # source minus destination offset, per line
    out = torch.empty_like(src)
    step = 1 << 24                                            # lines per piece (bounds the per-byte index)
    for a in range(0, perm.numel(), step):
        b = min(a + step, perm.numel())
        lo = int(dst_end[a] - plen[a])
        hi = int(dst_end[b - 1])
        idx = torch.arange(lo, hi, device=dev) + torch.repeat_interleave(shift[a:b], plen[a:b])
        out[lo:hi] = src[idx]
        del idx
    if dev == "cuda":
        torch.cuda.synchronize()
    return src, out, int(ends.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, nargs="*", default=[12_500_000, 100_000_000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--cpu-sort", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sort_bench: no GPU")
    ctx = starch_amd.Starch(0)
    tile, _ = starch_amd.sort_constants()
    for total in a.lines:
        want, bed, nlines = shuffled_on_device(total, a.seed)
        n = bed.numel()
        for _ in range(a.warmup):
            ctx.sort_bed_device(bed.data_ptr(), n)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.sort_bed_device(bed.data_ptr(), n)
            t.append((time.perf_counter() - t0) * 1e3)
        st = ctx.sort_stats()
        k = ctx.sort_bed_device(bed.data_ptr(), n)
        got = np.frombuffer(ctx._output(), dtype=np.uint8)
        assert k == n and np.array_equal(got, want.cpu().numpy()), "sorted output differs from the generator's bytes"
        med = statistics.median(t)
        # bytes a stage cannot avoid: the input once for framing and once for the
        # parse plus 28 B of per-line results; per radix pass a 4 B index read,
        # a key-byte gather counted as 8 B, 1 B digit written and read again,
        # 4 B index read and written by the scatter; the gather reads and writes
        # the text once plus 8 B line ends, 4 B index, 4 B length, 8 B offset
        L, p = nlines, st["radix_passes"]
        moved = {"parse": 2 * n + 28 * L, "sort": p * L * (4 + 8 + 1 + 1 + 4 + 4) + 20 * L, "gather": 2 * n + 36 * L}
        res = {"lines": L, "bed_bytes": n, "tile_lines": tile, "warmup": a.warmup, "reps": a.reps,
               "call_ms_median": round(med, 2), "call_ms_min": round(min(t), 2), "call_ms_max": round(max(t), 2),
               "input_gb_s": round(n / med / 1e6, 2), "stats": st,
               "stage_gb_s": {s: round(moved[s] / st["ms_" + s] / 1e6, 1) for s in moved if st["ms_" + s] > 0},
               "stage_bytes": moved}
        if a.cpu_sort:
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "shuffled.bed")
                with open(path, "wb") as f:
                    f.write(bed.cpu().numpy().tobytes())
                env = dict(os.environ, LC_ALL="C")
                t0 = time.perf_counter()
                r = subprocess.run(["sort", "-s", "-k1,1", "-k2,2n", "-k3,3n", "--parallel=16", "-T", d, "-o",
                                    os.path.join(d, "sorted.bed"), path], env=env, timeout=900)
                res["cpu_sort_s"] = round(time.perf_counter() - t0, 2) if r.returncode == 0 else None
        print(json.dumps(res), flush=True)
        del want, bed, got
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
