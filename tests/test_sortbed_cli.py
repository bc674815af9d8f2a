"""CPU-side checks of sort-bed: the parts of the command and of the Python
interface that open no GPU."""
import ctypes
import errno
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORTBED = os.path.join(ROOT, "starch_amd", "_build", "sort-bed")
STARCH3 = os.path.join(ROOT, "starch_amd", "_build", "starch3")


def _run(exe, *args, **kw):
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, **kw)


def test_help_and_version_open_no_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = _run(SORTBED, "--help", env=env)
    assert r.returncode == 0 and r.stderr == b""
    assert b"USAGE: sort-bed [--check-sort]" in r.stdout
    assert b"keep their input order" in r.stdout          # the tie rule is part of the usage text
    r = _run(SORTBED, "--version", env=env)
    assert r.returncode == 0 and r.stdout.startswith(b"sort-bed\n  version: ")


def test_usage_errors():
    r = _run(SORTBED, "--no-such-option")
    assert r.returncode == 1 and r.stdout == b"" and b"USAGE: sort-bed" in r.stderr
    r = _run(SORTBED, "-", "-", stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and b"stdin" in r.stderr
    r = _run(SORTBED, os.path.join(ROOT, "no", "such", "file.bed"))
    assert r.returncode == errno.ENODATA and b"does not exist" in r.stderr and r.stdout == b""
    r = _run(SORTBED, "--check-sort", os.path.join(ROOT, "no-such-a.bed"), os.path.join(ROOT, "no-such-b.bed"))
    assert r.returncode == errno.ENODATA and r.stdout == b""


def test_starch3_usage_names_sort():
    r = _run(STARCH3, "--help")
    assert r.returncode == 0 and b"--sort" in r.stdout and b"read to its end" in r.stdout
    r = _run(STARCH3, "--sort", "--gpus", "2", stdin=subprocess.DEVNULL)
    assert r.returncode == errno.EINVAL and b"--sort runs on one device" in r.stderr


def test_ctypes_declarations_load():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_sort_host", "starch_sort_device", "starch_sort_get_stats", "starch_sort_check_host",
                 "starch_sort_encode_host", "starch_sort_constants"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    # starch_sort_stats: five u64, one u32, five floats
    assert ctypes.sizeof(starch_amd.SortStats) == 64
    assert starch_amd.SortStats.radix_passes.offset == 40 and starch_amd.SortStats.ms_total.offset == 60
    tile, wave_copy = starch_amd.sort_constants()
    assert tile >= 256 and tile % 256 == 0
    assert 64 <= wave_copy <= 4096
    for m in ("sort_bed", "sort_bed_device", "sort_check", "sort_stats", "compress_sorted"):
        assert callable(getattr(starch_amd.Starch, m))
    # a NULL context is refused before anything touches a device
    k = ctypes.c_uint64()
    assert L.starch_sort_host(None, b"", 0) == -2
    assert L.starch_sort_check_host(None, b"", 0, ctypes.byref(k)) == -2
    assert L.starch_sort_get_stats(None, None) == -2
