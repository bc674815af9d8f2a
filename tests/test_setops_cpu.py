"""CPU-side checks of the bedops set operations: the two oracles of
tests/setops_oracle.py against each other and against the hand-written table,
and the parts of the `bedops` command and of the Python interface that open no
GPU."""
import ctypes
import errno
import os
import random
import subprocess

import pytest

from tests import setops_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEDOPS = os.path.join(ROOT, "starch_amd", "_build", "bedops")


def _run(*args, **kw):
    return subprocess.run([BEDOPS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, **kw)


def random_case(rng, max_inputs=5, max_chroms=3, max_iv=40, limit=300):
    chroms = [b"chr1", b"chr10", b"chr2"][:rng.randint(1, max_chroms)]
    inputs = []
    for _ in range(rng.randint(1, max_inputs)):
        rows = []
        for _ in range(rng.randint(0, max_iv)):
            s = rng.randrange(0, limit - 1)
            rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit - 1, s + 1 + rng.choice((1, 5, 40))))))
        inputs.append(oracle.bed3(sorted(rows)))
    return inputs


def test_oracles_agree_on_random_cases():
    rng = random.Random(20261019)
    nonempty = {op: 0 for op in oracle.OPS}
    for _ in range(200):
        inputs = random_case(rng)
        for op in oracle.OPS:
            a, b = oracle.bitmap(op, inputs), oracle.sweep(op, inputs)
            assert a == b, (op, inputs)
            nonempty[op] += a != b""
    assert all(v > 20 for v in nonempty.values()), nonempty   # the cases exercise every op


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracles_give_the_hand_written_table(case):
    inputs, want = oracle.TABLE[case]
    for op, exp in want.items():
        assert oracle.bitmap(op, inputs) == exp, op
        assert oracle.sweep(op, inputs) == exp, op


def test_help_and_version_open_no_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = _run("--help", env=env)
    assert r.returncode == 0 and r.stderr == b""
    assert b"USAGE: bedops (-m|--merge" in r.stdout
    for word in (b"union", b"intersection", b"exactly one", b"outside the union", b"abutting pieces are joined",
                 b"unverified against a BEDOPS binary"):
        assert word in r.stdout, word
    r = _run("--version", env=env)
    assert r.returncode == 0 and r.stdout.startswith(b"bedops\n  version: ")


def test_usage_errors():
    missing = os.path.join(ROOT, "no", "such", "file.bed")
    r = _run(missing)                                   # no operation
    assert r.returncode == 1 and r.stdout == b"" and b"USAGE: bedops" in r.stderr
    r = _run("-m", "--intersect", missing)              # two operations
    assert r.returncode == 1 and r.stdout == b"" and b"USAGE: bedops" in r.stderr
    r = _run("--no-such-option", "-m", missing)
    assert r.returncode == 1 and r.stdout == b"" and b"USAGE: bedops" in r.stderr
    r = _run("-m", missing)
    assert r.returncode == errno.ENODATA and b"does not exist" in r.stderr and r.stdout == b""
    r = _run("-m", "-", "-", stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and b"stdin" in r.stderr


def test_ctypes_declarations_load():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_setop_host", "starch_setop_device", "starch_setop_get_stats", "starch_setop_constants",
                 "starch_output_size", "starch_output_copy"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    # starch_setop_stats: nine u64, one u32, seven floats
    assert ctypes.sizeof(starch_amd.SetopStats) == 104
    assert starch_amd.SetopStats.radix_passes.offset == 72 and starch_amd.SetopStats.ms_total.offset == 100
    assert ctypes.sizeof(starch_amd.SetopInput) == 16
    tile = starch_amd.setop_constants()
    assert tile >= 256 and tile % 256 == 0
    for m in ("setop", "merge", "intersect", "difference", "symmdiff", "complement", "setop_stats"):
        assert callable(getattr(starch_amd.Starch, m))
    assert starch_amd.SETOPS == {"merge": 0, "intersect": 1, "difference": 2, "symmdiff": 3, "complement": 4}
    # a NULL context is refused before anything touches a device
    one = (starch_amd.SetopInput * 1)()
    offs = (ctypes.c_uint64 * 2)(0, 0)
    assert L.starch_setop_host(None, 0, one, 1) == -2
    assert L.starch_setop_device(None, 0, None, offs, 1) == -2
    assert L.starch_setop_get_stats(None, None) == -2
