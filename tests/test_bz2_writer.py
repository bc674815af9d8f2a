"""CPU: the permissive bzip2 writer (tests/bz2_writer.py) and the streams of
tests/bz2_foreign_cases.py, pinned by the system libbz2 through Python's bz2.

The reference decides what is valid: every stream that the GPU decoder is later
held to (test_gpu_decode_foreign.py) must decode here, by libbz2, to the bytes
the writer intended; every refused stream must be refused here.  The coverage
assertions check that a case reaches the decoder path it is named for (sample
on / off the walk's start node, a checkpoint on a count byte, ...), from what
the writer reports about the stream, not from any decoder.
"""
import bz2
import random

import pytest

from tests import bz2_foreign_cases as fc
from tests.bz2_writer import (Block, bwt, count_byte_positions, crc32, flat_lengths, rle1, stair_lengths, unrle1,
                              write_stream)


def test_crc_check_value():
    assert crc32(b"123456789") == 0xFC891918          # CRC-32/BZIP2's published check value


def test_rle1_round_trip_and_bwt():
    rng = random.Random(1)
    for _ in range(50):
        d = bytes(rng.choice(b"ab") for _ in range(rng.randrange(1, 700)))
        r = rle1(d)
        assert unrle1(r) == d
        assert all(r[p] <= 251 for p in count_byte_positions(r))
    assert bwt(b"banana") == (b"nnbaaa", 3)
    assert bwt(b"abab")[0] == b"bbaa"


def test_default_streams_decode():
    rng = random.Random(2)
    d = bytes(rng.choice(b"ACGT\n\t0123456789") for _ in range(3000)) + b"z" * 700
    assert bz2.decompress(write_stream([d]).data) == d
    s = write_stream([d[:1000], d[1000:1001], d[1001:]], level=3)
    assert bz2.decompress(s.data) == d and s.n_blocks == 3 and s.out == d
    assert bz2.decompress(write_stream([]).data) == b""
    assert s.data[:4] == b"BZh3"


def _kraft(lengths):
    return sum(2.0 ** -L for L in lengths)


def _coded_lengths(b):
    """Code lengths of the symbols the block actually codes, per table."""
    return {(b.selectors[i // 50], b.tables[b.selectors[i // 50]][s]) for i, s in enumerate(b.syms)}


@pytest.mark.parametrize("name", fc.GROUPS)
def test_libbz2_accepts_every_case(name):
    cases = fc.group(name)
    kept = []
    for c in cases:
        if c.conditional and not fc.accepted(c):
            continue                                    # only fc.CONDITIONAL; see test_only_the_listed_case_is_conditional
        assert bz2.decompress(c.stream.data) == c.stream.out, c.name
        kept.append(c)
    # and as the GPU test passes them: one concatenation per group
    assert bz2.decompress(b"".join(c.stream.data for c in kept)) == b"".join(c.stream.out for c in kept)


def test_only_the_listed_case_is_conditional():
    names = [c.name for g in fc.GROUPS for c in fc.group(g)]
    assert len(set(names)) == len(names)
    assert {n for n in names if n in fc.CONDITIONAL} == {"nsel_18102"} == set(fc.CONDITIONAL)
    # the two constructions the writer's first users left open are accepted by libbz2 and are unconditional
    assert {"oversubscribed_runa", "oversubscribed_runb", "count_252_middle", "count_255_end"} <= set(names)


def test_a_block_ending_in_four_equal_bytes_is_refused():
    # libbz2 always reads a count after four equal bytes, so this is no test case for a decoder
    with pytest.raises(OSError):
        bz2.decompress(write_stream([Block(raw=b"xyaaaa")]).data)


def test_coverage_lengths():
    g = {c.name: c.stream.blocks[0] for c in fc.group("lengths")}
    assert {L for _, L in _coded_lengths(g["all_20_bits"])} == {20}
    L = {L for _, L in _coded_lengths(g["stair_1_to_20"])}
    assert L & set(range(1, 11)) and L & set(range(11, 18)) and {18, 19, 20} <= L
    assert _kraft(g["stair_1_to_20"].tables[0]) == 1.0
    L = {L for _, L in _coded_lengths(g["straddle_9_to_12"])}
    assert L == {9, 10, 11, 12} and _kraft(g["straddle_9_to_12"].tables[0]) < 1.0
    b = g["complete_and_incomplete"]
    assert _kraft(b.tables[0]) == 1.0 and _kraft(b.tables[1]) < 1.0
    assert {t for t, _ in _coded_lengths(b)} == {0, 1}
    for n, runs in (("oversubscribed_runa", {0}), ("oversubscribed_runb", {1})):
        b = g[n]
        assert _kraft(b.tables[0]) > 1.0 and b.nin == 3 and set(b.raw) == {97}
        assert set(b.syms[:-1]) == runs and b.syms[-1] == 4


def test_coverage_tables_and_selectors():
    g = {c.name: c for c in fc.group("tables")}
    for nt in (2, 3, 6):
        b = g["tables_%d" % nt].stream.blocks[0]
        assert len(b.tables) == nt and {t for t, _ in _coded_lengths(b)} == set(range(nt))
        assert len({tuple(t) for t in b.tables}) == nt          # the wrong table gives the wrong bytes
    b = g["table_unused"].stream.blocks[0]
    assert len(b.tables) == 3 and set(b.selectors) == {0, 2}
    b = g["tables_6_on_30_symbols"].stream.blocks[0]
    assert len(b.tables) == 6 and b.nsym <= 30 and b.selectors == [5]
    b = g["selectors_100_unused"].stream.blocks[0]
    assert len(b.selectors) == (b.nsym + 49) // 50 + 100
    b = g["nsel_18102"].stream.blocks[0]
    assert len(b.selectors) == 18102 > 18002


def test_coverage_alphabet():
    g = {c.name: c for c in fc.group("alphabet")}
    for nin in (1, 2, 15, 16, 17, 255, 256):
        b = g["nin_%d_all_present" % nin].stream.blocks[0]
        assert b.nin == nin == len(set(b.raw))
        if nin > 1:
            b = g["nin_%d_one_present" % nin].stream.blocks[0]
            assert b.nin == nin and len(set(b.raw)) == 1
    for tag, nib in (("nibble", True), ("list", False)):
        f, l = g["front_run_first_" + tag].stream.blocks[0], g["front_run_last_" + tag].stream.blocks[0]
        assert f.syms[0] <= 1 and l.syms[-2] <= 1 and l.syms[-1] == l.nin + 1
        assert max(l.syms[:-1]) > 1 and len(set(l.raw)) > 1     # a run after other symbols, not the whole block
        assert (f.nin <= 16) == nib == (l.nin <= 16)


def test_coverage_sizes_and_walk_samples():
    cases = fc.group("sizes")
    assert sorted({c.stream.blocks[0].nblock for c in cases}) == sorted(fc.SIZES)
    assert [fc.walk_spacing(n) for n in (1023, 1024, 2046, 2047, 2048)] == [1, 2, 2, 4, 4]
    for n in fc.SIZES:
        here = [c for c in cases if c.stream.blocks[0].nblock == n]
        G = fc.walk_spacing(n)
        on = {c.stream.blocks[0].start % G == 0 for c in here}
        assert on == ({True} if G == 1 else {True, False}), n
        assert all(c.stream.blocks[0].raw == c.stream.out for c in here)   # no RLE1 run: n is the block's size


def _period(raw):
    return next(p for p in range(1, len(raw) + 1) if len(raw) % p == 0 and raw == raw[p:] + raw[:p])


def test_coverage_periodic():
    g = {c.name: c for c in fc.group("periodic")}
    for c in g.values():
        b = c.stream.blocks[0]
        assert _period(b.raw) == c.meta["period"] < b.nblock, c.name
        if c.meta["period"] in (2, 3):
            assert b.nblock & (b.nblock - 1), c.name
    assert g["period_1"].stream.blocks[0].nblock == 3
    assert all(fc.walk_spacing(g[n].stream.blocks[0].nblock) > 1 for n in g if n.endswith("_sampled"))


def test_coverage_bit_alignment():
    (c,) = fc.group("align")
    assert sorted(b.bit % 8 for b in c.stream.blocks) == list(range(8))


def test_coverage_rle1():
    g = {c.name: c for c in fc.group("rle1")}
    for r in fc.RUNS:
        for where in ("start", "middle", "end"):
            out = g["run_%d_%s" % (r, where)].stream.out
            assert out.count(b"a") == r and b"a" * r in out
        assert g["run_%d_start" % r].stream.out.startswith(b"a") and g["run_%d_end" % r].stream.out.endswith(b"a")
    for cnt in (0, 251, 252, 255):
        for where in ("middle", "end"):
            b = g["count_%d_%s" % (cnt, where)].stream.blocks[0]
            pos = count_byte_positions(b.raw)
            assert len(pos) == 1 and b.raw[pos[0]] == cnt and b.out_len == len(b.raw) - 1 + cnt
            assert (pos[0] == len(b.raw) - 1) == (where == "end")


def test_coverage_checkpoint_on_a_count_byte():
    """k_dec_unrle checkpoints its state at k * ceil(n / 64): for every n each
    such position that can hold a count byte (>= 4) does so in one of the cases."""
    raws = {(c.meta["n"], c.meta["r"]): c.stream.blocks[0].raw for c in fc.group("checkpoints")}
    for n in fc.CKPT_N:
        assert all(len(raws[n, r]) == n for r in range(5))
        counts = set().union(*(count_byte_positions(raws[n, r]) for r in range(5)))
        step = (n + 63) // 64
        assert (step == 1) == (n <= 64)
        want = {p for p in range(step, n, step) if p >= 4}
        assert want <= counts, (n, sorted(want - counts))


def test_coverage_largest_block():
    one, two = fc.group("largest")
    assert one.stream.level == 1 and [b.nblock for b in one.stream.blocks] == [100000]
    assert [b.nblock for b in two.stream.blocks] == [50000, 50000] and two.stream.out == one.stream.out


def test_libbz2_refuses_the_refused():
    for c in fc.refused():
        with pytest.raises(OSError):
            bz2.decompress(c.stream.data)
            pytest.fail("libbz2 accepts " + c.name)
    names = [c.name for c in fc.refused()]
    assert names == ["randomised", "tables_1", "tables_7", "nsel_0", "length_0", "length_21", "empty_map",
                     "origptr_nblock"]


def test_helpers():
    assert flat_lengths(3) == [2, 2, 2] and flat_lengths(258) == [9] * 258 and flat_lengths(4, 1) == [3] * 4
    assert stair_lengths(4) == [1, 2, 3, 3]
