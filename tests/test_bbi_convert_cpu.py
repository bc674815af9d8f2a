"""The host-callable Adler-32 fold (starch_amd/csrc/gz_adler.hpp through
starch_bbi_adler32_host) against zlib.adler32: the piece sums and the fold of two
pieces that a kernel over the inflated blocks of a bigWig / bigBed file is to
run.  Nothing here opens a GPU.

The conversion of the blocks on the GPU (bigwig2bed, bigbed2bed) is not in the
tree, so nothing else of it is tested here."""
import ctypes
import os
import random
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = (4096, 1, 1000, 5552, 1 << 20)      # the piece meant for one wave, and others on both sides of zlib's 5552


def _adler(data, piece):
    import starch_amd
    a = ctypes.c_uint32(0xdeadbeef)
    assert starch_amd.load().starch_bbi_adler32_host(data, len(data), piece, ctypes.byref(a)) == 0
    return a.value


@pytest.mark.parametrize("n", (0, 1, 5551, 5552, 5553, 65536))
def test_adler_fold_of_ff_bytes_equals_zlib(n):
    data = b"\xff" * n
    for piece in PIECES:
        assert _adler(data, piece) == zlib.adler32(data), (n, piece)


def test_adler_fold_of_random_buffers_equals_zlib():
    rng = random.Random(1950)
    for n in (2, 63, 64, 65, 1023, 4095, 4096, 4097, 8192 + 17, 100003):
        data = bytes(rng.getrandbits(8) for _ in range(n))
        for piece in PIECES:
            assert _adler(data, piece) == zlib.adler32(data), (n, piece)
    data = bytes([0xff, 0, 0xfe, 1]) * 50000                    # 200,000 bytes: s1 and s2 wrap many times
    assert _adler(data, PIECES[0]) == zlib.adler32(data)


def test_adler_helper_refuses_bad_arguments():
    import starch_amd
    L = starch_amd.load()
    a = ctypes.c_uint32()
    assert L.starch_bbi_adler32_host(b"abc", 3, 0, ctypes.byref(a)) == -2
    assert L.starch_bbi_adler32_host(b"abc", 3, (1 << 20) + 1, ctypes.byref(a)) == -2
    assert L.starch_bbi_adler32_host(None, 3, 4096, ctypes.byref(a)) == -2
    assert L.starch_bbi_adler32_host(b"abc", 3, 4096, None) == -2
    assert L.starch_bbi_adler32_host(None, 0, 4096, ctypes.byref(a)) == 0 and a.value == 1


def test_the_widths_that_the_header_argues_hold():
    header = open(os.path.join(ROOT, "starch_amd", "csrc", "gz_adler.hpp")).read()
    assert "kAdlerPiece = 4096" in header and "kAdlerMaxPiece = 1u << 20" in header and "kAdlerMod = 65521" in header
    for piece in (4096, 1 << 20):                               # a and w of a piece of 0xff bytes, unreduced, and n * a
        assert 255 * piece * (piece - 1) // 2 < 1 << 64 and 255 * piece * piece < 1 << 64
    assert "starch_bbi_adler32_host" in open(os.path.join(ROOT, "include", "starch_amd.h")).read()
