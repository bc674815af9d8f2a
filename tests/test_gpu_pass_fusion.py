"""The fused passes round the leaf sorts: k3_pss_hist (bwt3_round0.hip: packed
symbol stream + top-level histogram in one kernel) and k_mtf_pre / k_mtf_scan
(bz2_mtf.hip: three MTF launches instead of five).  Small texts, each
compressed through the library and compared byte for byte with the CPU path
(the reference's libbz2 where oracle/_ref is built, the oracle otherwise):
tile edges of the PSS kernel, every symbol width and MTF class, chunk edges
of the MTF pre-pass, and a batch that mixes the alphabet classes."""
import bz2
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(path, pattern):
    src = open(os.path.join(ROOT, "starch_amd", "csrc", path)).read()
    m = re.search(pattern, src)
    assert m, pattern
    return m


PTILE = int(_const("bwt3_int.hpp", r"constexpr int PTILE = (\d+);").group(1))
# the chunk lengths launch_mtf picks by batch size; a one-block batch takes the shortest
_CS = _const("bz2_mtf.hip", r"const uint32_t cs = nb >= 256 \? MCS : nb >= 64 \? (\d+)u : nb >= 8 \? (\d+)u : (\d+)u;")
MCS = int(_const("bz2_mtf.hip", r"constexpr uint32_t MCS = (\d+);").group(1))
CHUNKS = sorted({MCS} | {int(x) for x in _CS.groups()})
CS1 = CHUNKS[0]


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def _cpu(text):
    return oracle_lib.ref_bz2(text, 9) if oracle_lib.ref() is not None else oracle_lib.bz2(text, 9)


def _rle1_len(text):
    """Length of the block after bzip2's initial run-length coding."""
    n = i = 0
    while i < len(text):
        j = i
        while j < len(text) and text[j] == text[i] and j - i < 255:
            j += 1
        n += min(j - i, 4) + (1 if j - i >= 4 else 0)
        i = j
    return n


def _values(size):
    """size distinct byte values, 0x00 and 0xFF among them where size allows."""
    if size == 1:
        return [0xFB]
    mid = random.Random(size).sample(range(1, 255), size - 2)
    return [0x00] + sorted(mid) + [0xFF]


def _text(n, size, seed):
    """n symbols over `size` byte values, seeded, no run of 4 or more."""
    r = random.Random(seed)
    vals = _values(size)
    out = bytearray()
    while len(out) < n:
        v = r.choice(vals)
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == v:
            if size == 1:
                break
            continue
        out.append(v)
    return bytes(out)


def _check(ctx, text, n):
    """One block of n symbols after RLE1, equal to the CPU stream."""
    assert _rle1_len(text) == n
    out = ctx.bz2_compress(text, 9)
    nblk, crc = ctypes.c_uint32(), ctypes.c_uint32()
    assert ctx._L.starch_bz2_stream_info(ctx._h, ctypes.byref(nblk), ctypes.byref(crc)) == 0
    assert nblk.value == 1
    assert out == _cpu(text)
    assert bz2.decompress(out) == text


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, PTILE - 1, PTILE, PTILE + 1, 2 * PTILE, 2 * PTILE + 1])
def test_tile_edges(ctx, n):
    text = _text(n, 12, seed=1000 + n)      # 12 symbols: B = 4, the 16-byte loads and their fallback
    assert len(text) == n
    _check(ctx, text, n)


SIZES = [1, 2, 3, 4, 5, 8, 9, 13, 16, 17, 20, 24, 25, 30, 32, 33, 64, 200]


def _alphabet_text(size):
    n = PTILE + 1000
    if size == 1:
        # 0xFB runs of 255 code as FB FB FB FB + count 251 = FB: one symbol, 5 per run
        return b"\xfb" * (255 * (n // 5)), 5 * (n // 5)
    text = _text(n, size, seed=2000 + size)
    assert len(set(text)) == size
    return text, n


@pytest.mark.parametrize("size", SIZES)
def test_every_symbol_width(ctx, size):
    """Size 1 is a block of one byte value of mainSort's size (>= 10000 symbols): libbz2 leaves its
    rotations in index order there, origPtr 0, not in fallbackSort's order (k_fb_origptr)."""
    text, n = _alphabet_text(size)
    _check(ctx, text, n)


CHILD_BZ2 = ("import sys; sys.path.insert(0, %r); import starch_amd; "
             "d = open(sys.argv[1], 'rb').read(); c = starch_amd.Starch(0); "
             "sys.stdout.buffer.write(c.bz2_compress(d, 9)); c.close()" % ROOT)
CHILD_ARCH = ("import sys; sys.path.insert(0, %r); import starch_amd; "
              "d = open(sys.argv[1], 'rb').read(); c = starch_amd.Starch(0); "
              "sys.stdout.buffer.write(c.compress(d)); c.close()" % ROOT)


def test_mixed_radix_width_with_binary_digit(tmp_path):
    """A 17..20-symbol block sorts by the 8192-bin digit; STARCH_WIDE=0 sorts it by the 4096-bin one."""
    text, _ = _alphabet_text(20)
    f = tmp_path / "t.bin"
    f.write_bytes(text)
    env = dict(os.environ, STARCH_WIDE="0")
    out = subprocess.run([sys.executable, "-c", CHILD_BZ2, str(f)], env=env, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert out.stdout == _cpu(text)


def _last_column(text):
    """Last column of the sorted rotations, as ranks among the byte values in use."""
    _, ptr = oracle_lib.block_sort(text)
    rank = {v: i for i, v in enumerate(sorted(set(text)))}
    return [rank[text[p - 1]] for p in ptr]


@pytest.mark.parametrize("cs", CHUNKS)
@pytest.mark.parametrize("size", [12, 20, 28])
def test_chunk_lengths(ctx, cs, size):
    for n in (cs - 1, cs, cs + 1, 3 * cs + 1):
        _check(ctx, _text(n, size, seed=3000 + n + size), n)


@pytest.mark.parametrize("cs", [CS1, MCS])
def test_zero_run_over_whole_chunks(ctx, cs):
    """8 chunks; "ab" * k sorts into two runs, each spanning whole chunks (a periodic block),
    and one changed symbol keeps the long runs in a block the sort itself finishes."""
    for text in (b"ab" * (4 * cs), b"ab" * (4 * cs - 1) + b"ac"):
        assert len(text) == 8 * cs
        L = _last_column(text)
        whole = [c for c in range(8) if len(set(L[c * cs - 1 if c else 0:(c + 1) * cs])) == 1]
        assert any(c + 1 in whole for c in whole), whole      # two neighbouring chunks inside one run
        _check(ctx, text, len(text))


def _find(size, n, want):
    for seed in range(400):
        text = _text(n, size, seed=4000 + seed)
        L = _last_column(text)
        if want(L):
            return text, L
    raise AssertionError("no seed has the property")


@pytest.mark.parametrize("size", [4, 20])
def test_zero_run_across_a_chunk_edge(ctx, size):
    """A zero run of exactly two: the last symbol of one chunk and the first of the next."""
    cs, n = CS1, 16 * CS1

    def want(L):
        return any(L[e - 3] != L[e - 2] == L[e - 1] == L[e] != L[e + 1] for e in range(cs, n, cs))
    text, L = _find(size, n, want)
    assert want(L)
    _check(ctx, text, n)


@pytest.mark.parametrize("size", [4, 20])
def test_first_symbol_is_not_symbol_zero(ctx, size):
    """The block's first symbol meets the initial list, whose front is symbol 0: a non-zero first index."""
    text = _text(4 * CS1 + 5, size, seed=5000 + size)
    assert _last_column(text)[0] != 0
    _check(ctx, text, len(text))


def test_first_symbol_is_symbol_zero(ctx):
    """... and a zero first index.  The smallest rotation starts a longest run of the smallest symbol, so
    another symbol precedes it whenever the block has two: only one-symbol blocks start with symbol 0."""
    for text, n in ((b"\xfb" * 3, 3), (b"\xfb" * (255 * (4 * CS1 + 5)), 5 * (4 * CS1 + 5))):
        assert set(_last_column(text[:_rle1_len(text)])) == {0}
        _check(ctx, text, n)


def test_mixed_classes_in_one_batch(tmp_path):
    """Streams of <= 16, 17..24 and > 32 symbols in one call, in one batch and in batches of one block."""
    import starch_amd
    r = random.Random(9)
    names = bytes(range(65, 91)) + bytes(range(97, 123))
    big = b"".join(b"chrZ\t%d\t%d\t%s\n" % (i * 10, i * 10 + 5, bytes(r.choice(names) for _ in range(8)))
                   for i in range(20_000))
    data = (bytes(starch_amd.gen_bed(0, 60_000, chroms=[20])) + bytes(starch_amd.gen_bed(1, 40_000, chroms=[21]))
            + big)
    _, osegs = oracle_lib.transform(data)
    kinds = [len(set(t)) for _, _, t in osegs]
    assert len(kinds) == 3 and kinds[0] <= 16 and 17 <= kinds[1] <= 24 and kinds[2] > 32, kinds
    f = tmp_path / "in.bed"
    f.write_bytes(data)
    archs = []
    for env in (dict(os.environ, STARCH_BWT_BATCH="1"), {k: v for k, v in os.environ.items() if k != "STARCH_BWT_BATCH"}):
        out = subprocess.run([sys.executable, "-c", CHILD_ARCH, str(f)], env=env, capture_output=True, timeout=300)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        archs.append(out.stdout)
    assert archs[0] == archs[1]
    _, streams = starch_amd.parse_archive(archs[1])
    assert len(streams) == 3
    for st, (_, _, t) in zip(streams, osegs):
        assert st == _cpu(t)
