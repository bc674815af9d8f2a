"""bench.py's N-rank launcher and CPU-baseline pool (CPU tests), plus the
launcher on one real GPU.

* `bench.py --gpus N` with no WORLD_SIZE starts N fresh ranks itself (the
  driver's scaling leg runs it that way); `--launch-selftest` makes the ranks
  join a gloo group and compute the same LPT chromosome shares as the GPU
  bench, so the launcher, its environment and the shard plan run on the CPU.
* `--gpus N` with fewer than N visible GPUs must fail, never run fewer ranks.
* oracle/cpu_pool.c (the cpu_baseline leg) must compute exactly the
  oracle's transform + bzip2 per piece.
"""
import json
import os
import subprocess
import sys

import pytest

from tests import corpus, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


@pytest.mark.parametrize("n", [1, 2, 4])
def test_launcher_starts_n_ranks(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--launch-selftest", "--lines", "1000000"],
                       env=_env(), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == n
    assert len(res["rank_bytes"]) == n and all(b > 0 for b in res["rank_bytes"])
    assert sum(res["rank_units"]) == 24


def test_launcher_refuses_missing_gpus():
    import torch
    have = torch.cuda.device_count()
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(max(2, have + 1)), "--steps", "1", "--warmup", "0"],
                       env=_env(), capture_output=True, timeout=300)
    assert r.returncode != 0
    assert b"refusing" in r.stderr


def test_kfd_gpu_count_from_sysfs(tmp_path):
    """The launcher counts GPUs from the KFD topology (no HIP call): nodes with
    SIMDs whose render node is accessible; CPU nodes (simd_count 0) and GPUs
    whose render node this process cannot open are not counted."""
    sys.path.insert(0, ROOT)
    import bench
    nodes, dri = tmp_path / "nodes", tmp_path / "dri"
    dri.mkdir()
    for i, (simd, minor, present) in enumerate([(0, 0, False), (1024, 128, True), (1024, 129, True),
                                                 (1024, 130, False)]):
        d = nodes / str(i)
        d.mkdir(parents=True)
        (d / "properties").write_text("cpu_cores_count 0\nsimd_count %d\ndrm_render_minor %d\n" % (simd, minor))
        if present:
            (dri / ("renderD%d" % minor)).write_text("")
    assert bench._kfd_gpus(str(nodes), str(dri)) == 2
    assert bench._kfd_gpus(str(tmp_path / "absent"), str(dri)) is None


def test_world_size_mismatch_fails():
    env = _env()
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--launch-selftest"], env=env, capture_output=True,
                       timeout=300)
    assert r.returncode != 0


def test_cpu_pool_matches_oracle():
    data = corpus.multi_chrom_bed(5, 3000, seed=5, kind="bed6") + corpus.multi_chrom_bed(3, 2000, seed=6)
    import starch_amd
    units = starch_amd.plan_units(data, 64)
    spans = [(u.offset, u.length) for u in units]
    secs, per, outb, kind = oracle_lib.cpu_pool(data, spans, 3)
    assert secs > 0 and len(per) == len(spans)
    for (o, l), got in zip(spans, outb):
        _, segs = oracle_lib.transform(data[o:o + l])
        want = sum(len(oracle_lib.ref_bz2(t, 9) if kind == "reference" else oracle_lib.bz2(t, 9))
                   for _, _, t in segs)
        assert got == want


def _fake_archive(n_payload, seed):
    """magic + seeded bytes cut into three 'streams' + a JSON index + the 32-byte footer."""
    import random
    import starch_amd
    payload = random.Random(seed).randbytes(n_payload)
    cuts = [0, n_payload // 3, n_payload // 2, n_payload]
    idx = {"streams": [{"chromosome": "chr%d" % (k + 1), "offset": 4 + cuts[k], "size": cuts[k + 1] - cuts[k],
                        "uncompressedLineCount": 10 * (k + 1)} for k in range(3)]}
    off = 4 + n_payload
    return starch_amd.MAGIC + payload + json.dumps(idx).encode() + b"%020d" % off + b" " * 11 + b"\n", idx


@pytest.mark.parametrize("n_payload", [1000, (1 << 16) - 4, 5 * (1 << 16) + 77])
def test_dump_outputs_files(tmp_path, n_payload):
    """--dump-outputs: float arrays only, the chunk sums cover every byte
    (sizes below, at and off a multiple of the 64 KiB chunk), head and sample
    hold the archive's own bytes, and the same archive gives the same files."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    arch, idx = _fake_archive(n_payload, seed=n_payload)
    bench.dump_outputs(str(tmp_path / "a"), arch)
    bench.dump_outputs(str(tmp_path / "b"), arch)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("archive_size", "stream_offsets", "stream_sizes", "stream_lines",
                                                "archive_chunk_sums", "archive_head", "archive_sample"))
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert got[n[:-4]].dtype in (np.float32, np.float64)
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    a = np.frombuffer(arch, dtype=np.uint8).astype(np.int64)
    assert got["archive_size"].tolist() == [len(arch)]
    assert got["stream_sizes"].tolist() == [s["size"] for s in idx["streams"]]
    assert got["stream_offsets"].tolist() == [s["offset"] for s in idx["streams"]]
    assert got["stream_lines"].tolist() == [10, 20, 30]
    want = [int((a[c:c + bench.DUMP_CHUNK] * np.arange(1, len(a[c:c + bench.DUMP_CHUNK]) + 1)).sum())
            for c in range(0, len(a), bench.DUMP_CHUNK)]
    assert got["archive_chunk_sums"].tolist() == want
    assert got["archive_head"].tolist() == a[:bench.DUMP_HEAD].tolist()
    assert len(got["archive_sample"]) == bench.DUMP_SAMPLE
    assert set(np.unique(got["archive_sample"]).tolist()) <= set(np.unique(a).tolist())
    # a changed byte anywhere shows in the chunk sums
    flipped = bytearray(arch)
    flipped[len(arch) // 2] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), bytes(flipped))
    assert np.load(tmp_path / "c" / "archive_chunk_sums.npy").tolist() != want


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_archive(tmp_path):
    """A plain run prints the headline line without the --full legs, and
    --dump-outputs holds the archive of its last timed step: the same bytes
    the library gives for the same seeded input in this process."""
    import numpy as np
    import starch_amd
    sys.path.insert(0, ROOT)
    import bench
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--lines", "1000000", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], env=_env(), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    res = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "MB/s" and res["dtype"] == "u8"
    assert res["value"] == pytest.approx(res["config"]["input_bytes"] / res["ms_per_step"] / 1e3, rel=1e-3)
    for k in ("roofline", "transform_roofline", "stage_ms_one_lane", "e2e", "cpu_baseline", "verify"):
        assert k not in res
    ctx = starch_amd.Starch(0)
    arch = ctx.compress(starch_amd.gen_bed(0, 1_000_000, seed=bench.SEED))
    ctx.close()
    a = np.frombuffer(arch, dtype=np.uint8)
    assert np.load(out / "archive_size.npy").tolist() == [len(arch)] == [res["config"]["archive_bytes"]]
    assert np.array_equal(np.load(out / "archive_head.npy"), a[:bench.DUMP_HEAD].astype(np.float32))
    bench.dump_outputs(str(tmp_path / "here"), arch)
    for n in os.listdir(out):
        assert (out / n).read_bytes() == (tmp_path / "here" / n).read_bytes(), n


@pytest.mark.gpu
def test_launcher_one_gpu_bench():
    """The launcher path on the GPU box: --gpus 1 --spawn: one launched
    rank (torch.distributed + the RCCL gather at world 1) on a small
    input; the line must say one GPU and carry the encode / gather split."""
    env = _env()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--spawn", "--lines", "2000000", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline", "--no-e2e"], env=env, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    res = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 1
    assert res["dist"]["ms_encode_max"] > 0 and res["dist"]["ms_gather_max"] >= 0


@pytest.mark.gpu
def test_launcher_counts_gpus_without_hip():
    """bench.visible_gpus() in a fresh process equals torch's device count
    (taken in another process) and leaves no HIP runtime mapped: the launcher
    must not initialise the GPU before it starts its rank processes."""
    code = ("import sys; sys.path.insert(0, %r); import bench; n = bench.visible_gpus(); "
            "maps = open('/proc/self/maps').read(); print(n, int('libamdhip64' in maps))" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=_env(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    n, hip = map(int, r.stdout.split())
    r2 = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], env=_env(),
                        capture_output=True, timeout=300)
    assert n == int(r2.stdout.split()[-1]) and n >= 1
    assert hip == 0
