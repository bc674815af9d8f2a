"""The work queue of the one-wave leaf sorts (WaveQueue, bz2_int.hpp): the pop
of a wave's next chunk of groups is issued ahead of need and read when the
current chunk runs out.  A wrong queue drops a group or takes it twice, which
shows as a stream that differs from the CPU path or as a bwt3 error, so every
case encodes BED already in HBM (the device path) and compares each stream of
the archive byte for byte with the CPU path (the reference's libbz2 where
oracle/_ref is built, the oracle otherwise).

The shapes: more blocks than XCDs with one and two encoder lanes; one block
and three (queues cut by 64-item runs, most of them empty, so waves steal from
their first pop); class lists shorter than a chunk and a multiple of the chunk
plus one; S lists that are empty at the top level; an input whose ties
need text rounds and prefix doubling (the DBL instantiations); and one block
whose sort needs more launches than the host's pool of queue sets holds.

List lengths come from a model of the top level only (_top_level: the groups
are the rotations that share their first three symbols, for 4-bit alphabets
and for the 8192-bin digit of 17 to 20 symbols alike; groups of 65..128
rotations are class S, 129..256 class S2); the cases assert the model's
figure, so a generator change cannot silently move them off their shape.
Groups cut from larger ones at deeper levels add to the lists and are not
modelled."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_MAX = 32                  # every chunk size of the build-time sweep (4, 8, 16, 32) divides it


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def _cpu(text, level):
    return oracle_lib.ref_bz2(text, level) if oracle_lib.ref() is not None else oracle_lib.bz2(text, level)


def _encode(ctx, data, level, lanes=0):
    import torch
    ctx.block_size_100k = level
    ctx.set_lanes(lanes)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    ctx.compress_device(dev.data_ptr(), len(data))
    arch = ctx.archive()
    ctx.set_lanes(0)
    ctx.block_size_100k = 9
    return arch


def _check_archive(arch, data, level):
    import starch_amd
    idx, streams = starch_amd.parse_archive(arch)
    _, osegs = oracle_lib.transform(data)
    assert len(streams) == len(osegs)
    for st, (chr_, lines, text), meta in zip(streams, osegs, idx["streams"]):
        assert meta["chromosome"].encode("latin-1") == chr_
        assert meta["uncompressedLineCount"] == lines
        assert st == _cpu(text, level), chr_
    return osegs


def _check(ctx, data, level=9, lanes=0):
    return _check_archive(_encode(ctx, data, level, lanes), data, level)


def _rle1(t):
    """The block bzip2 sorts: runs of 4..255 equal bytes as 4 bytes and a count."""
    out = bytearray()
    i = 0
    while i < len(t):
        j = i
        while j < len(t) and t[j] == t[i] and j - i < 255:
            j += 1
        out += t[i:i + 1] * min(j - i, 4)
        if j - i >= 4:
            out.append(j - i - 4)
        i = j
    return bytes(out)


def _top_level(text):
    """(symbols of the block, S groups, S2 groups) of a one-block text at the top level."""
    blk = np.frombuffer(_rle1(text), dtype=np.uint8).astype(np.int64)
    n = len(blk)
    assert 10000 <= n <= 899981            # one block, and not libbz2's small-block sort
    ext = np.concatenate([blk, blk[:2]])
    _, z = np.unique((ext[:n] << 16) | (ext[1:n + 1] << 8) | ext[2:n + 2], return_counts=True)
    return len(set(blk.tolist())), int(((z > 64) & (z <= 128)).sum()), int(((z > 128) & (z <= 256)).sum())


def _gen(kind, lines, chroms):
    import starch_amd
    return bytes(starch_amd.gen_bed(kind, lines, chroms=chroms))


def _blocks(osegs, level):
    return sum(math.ceil(len(_rle1(t)) / (100000 * level - 19)) for _, _, t in osegs)


def test_more_blocks_than_xcds_one_lane(ctx):
    data = _gen(0, 1_200_000, [20, 21])
    osegs = _check(ctx, data, level=1, lanes=1)
    assert _blocks(osegs, 1) >= 12


CHILD = r"""
import sys
sys.path.insert(0, %r)
import torch, starch_amd
data = open(sys.argv[1], "rb").read()
c = starch_amd.Starch(0)
c.block_size_100k = 1
c.set_lanes(2)
dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
c.compress_device(dev.data_ptr(), len(data))
sys.stdout.buffer.write(c.archive())
c.close()
""" % ROOT


def test_more_blocks_than_xcds_two_lanes(tmp_path):
    """Two lanes, each with its own block sort and queues, running at once.  The library splits an
    encode into lanes only above a text size it reads once per process (STARCH_DEV_LANES_MIN), so this
    case runs in a process of its own with that bound at 0."""
    data = _gen(0, 1_200_000, [20, 21])
    f = tmp_path / "in.bed"
    f.write_bytes(data)
    out = subprocess.run([sys.executable, "-c", CHILD, str(f)], env=dict(os.environ, STARCH_DEV_LANES_MIN="0"),
                         capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    osegs = _check_archive(out.stdout, data, 1)
    assert len(osegs) == 2 and _blocks(osegs, 1) >= 12


@pytest.mark.parametrize("lines,nblocks", [(1_500_000, 1), (4_600_000, 3)])
def test_fewer_blocks_than_xcds(ctx, lines, nblocks):
    data = _gen(0, lines, [20])
    osegs = _check(ctx, data)
    assert _blocks(osegs, 9) == nblocks


# (kind, total lines of the generator, S groups, S2 groups); kind 1: 17 to 20 symbols, the 8192-bin digit
SHORT = [(0, 22_500, 15, 4), (1, 4_000, 2, 4)]
PLUS_ONE = [(0, 152_500, 97, 147), (0, 142_500, 112, 129), (1, 88_000, 993, 241), (1, 61_000, 480, 193)]


@pytest.mark.parametrize("kind,lines,ns,ns2", SHORT + PLUS_ONE)
def test_list_lengths(ctx, kind, lines, ns, ns2):
    data = _gen(kind, lines, [20])
    _, osegs = oracle_lib.transform(data)
    nsym, s, s2 = _top_level(osegs[0][2])
    assert (s, s2) == (ns, ns2)
    assert nsym <= 16 if kind == 0 else 17 <= nsym <= 20
    if (kind, lines, ns, ns2) in SHORT:
        assert 0 < min(s, s2) < 8                       # shorter than a chunk
    else:
        assert 1 in (s % CHUNK_MAX, s2 % CHUNK_MAX)     # a multiple of every swept chunk, plus one
    _check(ctx, data)


def test_empty_s_lists(ctx):
    """Long runs of one byte: after the run-length step the block is a few symbols in a few
    contexts, so the top-level groups are far larger than S2 or tiny, and the S and S2 lists are
    empty there; a prefetched pop on an empty queue must come back as drained."""
    r = random.Random(5)
    data = b"".join(b"chrZ\t%d\t%d\t%s\n" % (i * 10, i * 10 + 5, bytes([r.choice(b"ACGT")]) * 200)
                    for i in range(3_000))
    _, osegs = oracle_lib.transform(data)
    _, s, s2 = _top_level(osegs[0][2])
    assert (s, s2) == (0, 0)
    _check(ctx, data)


def test_text_rounds_and_doubling(ctx):
    """Long lines repeated many times: the rotations inside them tie over far more than a key's
    64 bits, so the sort runs its text rounds and then prefix doubling, whose class lists go
    through the same queue (the DBL instantiations)."""
    r = random.Random(6)
    names = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(400)) for _ in range(12)]
    data = b"".join(b"chrZ\t%d\t%d\t%s\n" % (i * 10, i * 10 + 5, r.choice(names)) for i in range(1_500))
    _check(ctx, data)
    st = ctx.stats()
    assert st["bwt_rounds"] > 0 and st["bwt_tied"] > 0


# lines per run of equal gaps; the gap (1..9) is the run's own digit in the transformed text
POOL_RUNS = [100, 250, 400, 600, 1400, 3200, 7000, 14000, 20000]


def test_queue_pool_wraps(ctx):
    """One -1 block whose sort takes more persistent launches than the queue pool has sets (64 per
    batch, launch_bwt3's next_q), so the pool is cleared and reused in mid-sort.  Nine runs of
    intervals of one width, run k with gaps of k bases: the text of run k is its digit and a
    newline repeated, so its rotations tie in two groups of the run's length, one group in
    every size class from S to L, and prefix doubling peels them over a dozen rounds with most class
    lists in use in each: every list of every round is binned with a queue set of its own.
    (Checked once with a host-side print in next_q and read_ctr: 71 counter reads, every leaf
    class in both key forms, the pool cleared once.)"""
    lines, pos = [], 1000
    for gap, n in enumerate(POOL_RUNS, 1):
        for _ in range(n):
            lines.append(b"chrZ\t%d\t%d\n" % (pos, pos + 50))
            pos += 50 + gap
    data = b"".join(lines)
    osegs = _check(ctx, data, level=1)
    assert _blocks(osegs, 1) == 1
    t = osegs[0][2]
    for gap, n in enumerate(POOL_RUNS, 1):
        assert (b"%d\n" % gap) * (n - 1) in t          # the runs are there as described
    assert ctx.stats()["bwt_rounds"] >= 10
