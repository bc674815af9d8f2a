"""The record logic of bigwig2bed / bigbed2bed on the host, under a sanitizer.

starch_amd/csrc/bed_bbi_rec.hpp holds what the kernels of bed_bbi_dev.hip decide
about a block's inflated bytes, as __host__ __device__ functions.
tools/bbi_rec_check.cpp runs them stage by stage as the kernels do; it is built
here as a stand-alone program with -fsanitize=address,undefined (no Python
extension, no preloaded runtime) and fed the inflated blocks of every case of
tests/bbi_cases.py.  Nothing here opens a GPU."""
import os
import random
import struct
import subprocess

import pytest

from tests import bbi_cases as cases
from tests import bbi_expect as expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bbi_rec_check") / "bbi_rec_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tools", "bbi_rec_check.cpp")])
    return exe


def _run(prog, tmp_path, blob, *flags):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(blob)
    return subprocess.run([prog, *flags, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV)


@pytest.mark.parametrize("name", sorted(cases.good()))
def test_good_cases_give_the_oracles_lines(prog, tmp_path, name):
    kind, data, regions = cases.good()[name]
    for rg in regions:
        r = _run(prog, tmp_path, expect.case_file(data, rg))
        assert r.returncode == 0 and r.stderr == b"", (rg, r.returncode, r.stderr[-2000:])
        assert r.stdout == expect.expected_text(data, rg), rg


def test_deflate_dynamic_and_three_sections_have_all_their_records(prog, tmp_path):
    for name in ("deflate_dynamic", "three_sections"):
        data = cases.good()[name][1]
        r = _run(prog, tmp_path, expect.case_file(data))
        assert r.returncode == 0 and r.stderr == b""
        lines = r.stdout.split(b"\n")[:-1]
        assert len(lines) == 1037 and r.stdout == expect.expected_text(data)
        assert lines[-1] == b"chr10\t2147483683\t2147483687\t11"          # fixedStep starts that crossed 2^31


@pytest.mark.parametrize("name", sorted(expect.RECORD_BAD))
def test_bad_blocks_are_refused_with_their_number(prog, tmp_path, name):
    data = cases.bad()[name][1]
    r = _run(prog, tmp_path, expect.case_file(data))
    assert r.returncode == 3 and r.stdout == b"", (r.returncode, r.stderr[-2000:])
    assert r.stderr.startswith(b"block %d: " % expect.RECORD_BAD[name]), r.stderr


def test_percent_g_of_float32_bit_patterns(prog, tmp_path):
    rng = random.Random(754)
    bits = list(cases.G_BITS) + [rng.getrandbits(32) for _ in range(4000)]
    bits += [(e << 23) | f for e in (0, 1, 126, 127, 149, 150, 173, 254) for f in (0, 1, 0x400000, 0x7FFFFF)]   # exponent edges
    r = _run(prog, tmp_path, struct.pack("<%dI" % len(bits), *bits), "--g")
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    got = r.stdout.split(b"\n")[:-1]
    assert len(got) == len(bits)
    for b, g in zip(bits, got):
        want = "%g" % struct.unpack("<f", struct.pack("<I", b))[0]
        if want == "-nan":
            want = "nan"                                   # a NaN prints nan whatever its sign
        assert g.decode() == want, hex(b)
