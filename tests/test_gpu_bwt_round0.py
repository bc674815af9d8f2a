"""Round 0 of the block sort (bwt3_round0.hip): the top-level bucket scatter
(k3_scatter_lds) and the workgroup sort of the 1025..2048 class (k3_sort_lds),
at the smallest shapes where they can go wrong -- stage and tile edges of the
scatter, singleton and L-class buckets (the flag word of the write-out),
waves whose lanes all share / never share a digit, groups that the first MSD
digit does not spread, and the 8192-bin (wide digit) instantiations.
Every case is byte-for-byte against the CPU oracle's bzip2 stream."""
import random

import pytest

from tests import oracle_lib

pytestmark = pytest.mark.gpu

SYM13 = b"0123456789\t\n-"
SYM9 = b"012345678"


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def _text(r, alphabet, n):
    """n random symbols with no run of four, so bzip2's initial run-length
    stage leaves the text alone and the block is exactly n bytes."""
    out = bytearray()
    while len(out) < n:
        s = r.choice(alphabet)
        if len(out) >= 3 and out[-1] == s and out[-2] == s and out[-3] == s:
            continue
        out.append(s)
    return bytes(out)


def _check(ctx, data, bs):
    assert ctx.bz2_compress(data, bs) == oracle_lib.bz2(data, bs), (len(data), bs)


# one scatter stage is 16384 rotations, one tile 32768
@pytest.mark.parametrize("n", [16383, 16384, 16385, 32767, 32768, 32769, 49153])
def test_scatter_stage_and_tile_edges(ctx, n):
    _check(ctx, _text(random.Random(1000 + n), SYM13, n), 9)


@pytest.mark.parametrize("where", ["start", "end"])
def test_singleton_buckets_and_rotation0(ctx, where):
    # "XYZ" occurs once: its rotations sit alone in their buckets and are
    # final after the scatter; at the start, rotation 0 is one of them
    noise = _text(random.Random(21), SYM13, 100_000)
    _check(ctx, b"XYZ" + noise if where == "start" else noise + b"XYZ", 9)


def test_l_class_bucket_beside_singletons(ctx):
    # "000" starts 60,000 rotations (an L-class bucket, > 4096); "XYZ" stays a singleton
    r = random.Random(22)
    body = b"".join(b"000" + _text(r, SYM13[1:], 7) for _ in range(60_000))
    data = b"XYZ" + body[:600_000 - 3]
    assert data.count(b"000") > 4096 and data.count(b"XYZ") == 1
    _check(ctx, data, 9)


def test_all_lanes_share_a_digit(ctx):
    _check(ctx, b"0" * 70_000 + _text(random.Random(23), SYM13, 30_000), 9)


def test_no_lanes_share_a_digit(ctx):
    r = random.Random(24)
    _check(ctx, bytes(r.randrange(256) for _ in range(70_000)), 9)


def test_m2_groups(ctx):
    # 9 symbols: 729 buckets of about 1,234 rotations, all in 1025..2048
    _check(ctx, _text(random.Random(25), SYM9, 900_000), 9)


def test_m2_template_small_classes(ctx):
    # 5 symbols, 100 KB blocks: the same template at its smaller classes
    _check(ctx, _text(random.Random(26), SYM9[:5], 900_000), 1)


def test_m2_groups_with_shared_prefix(ctx):
    # text of repeated 10-symbol words: rotations that start a word share their
    # first 40 key bits, so the first digit does not spread their group
    r = random.Random(27)
    words = [_text(r, SYM9, 10) for _ in range(48)]
    data = b"".join(r.choice(words) for _ in range(90_000))
    _check(ctx, data, 9)


@pytest.mark.parametrize("nsym", [17, 20])
def test_wide_digit_block(ctx, nsym):
    r = random.Random(28 + nsym)
    alphabet = bytes(range(65, 65 + nsym))
    _check(ctx, _text(r, alphabet, 100_000), 9)
