"""GPU: the bzip2 decoder against libbz2's decoder on streams that libbz2's
encoder never writes (tests/bz2_foreign_cases.py, written by
tests/bz2_writer.py): code lengths up to 20 bits, incomplete and
over-subscribed codes, 2..6 tables whatever the block's size, unused and
surplus selectors, declared-but-absent bytes, every alphabet size at which the
MTF list changes form, block sizes around the inverse walk's sample spacing
and the tt and un-RLE tiles, periodic blocks, every bit alignment, count bytes
up to 255 and a block of exactly 100000 bytes at level 1.
test_bz2_writer.py pins every stream on the CPU first.

The streams of a group go through the decoder in one call, concatenated; on a
mismatch the members are decoded one by one to name the case."""
import bz2 as pybz2

import pytest

from tests import bz2_foreign_cases as fc


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def _check(ctx, cases):
    cases = [c for c in cases if not c.conditional or fc.accepted(c)]
    blob = b"".join(c.stream.data for c in cases)
    want = pybz2.decompress(blob)
    assert want == b"".join(c.stream.out for c in cases)
    import starch_amd
    try:
        got = ctx.bz2_decompress(blob)
        st = ctx.decoded_streams() if got == want else None
    except starch_amd.StarchError as e:
        if e.code != -12:                               # only a refusal of the data is looked into
            raise
        got = st = None
    if got != want:
        bad = []
        for c in cases:
            try:
                ok = ctx.bz2_decompress(c.stream.data) == pybz2.decompress(c.stream.data)
                bad += [] if ok else [c.name + ": wrong bytes"]
            except starch_amd.StarchError as e:
                if e.code != -12:
                    raise
                bad.append("%s: %s" % (c.name, e))
        raise AssertionError("decoder and libbz2 disagree on: " + "; ".join(bad or ["the concatenation only"]))
    assert len(st) == len(cases)
    for s, c in zip(st, cases):
        assert (s["level"], s["n_blocks"], s["out_len"]) == (c.stream.level, c.stream.n_blocks, len(c.stream.out)), \
            c.name


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g for g in fc.GROUPS if g != "checkpoints"])
def test_foreign_streams(ctx, name):
    _check(ctx, fc.group(name))


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(4))
def test_foreign_unrle_checkpoints(ctx, part):
    """Run-heavy blocks of 1..200 bytes: every checkpoint of k_dec_unrle lands
    on a count byte in one of them (asserted in test_bz2_writer.py)."""
    cases = fc.group("checkpoints")
    _check(ctx, cases[part::4])


@pytest.mark.gpu
def test_foreign_refusals(ctx):
    """Header-level faults: both decoders refuse, and the context decodes a good stream afterwards."""
    import starch_amd
    good = fc.group("lengths")[1].stream
    for c in fc.refused():
        with pytest.raises(OSError):
            pybz2.decompress(c.stream.data)
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.bz2_decompress(c.stream.data)
        assert e.value.code == -12, c.name
        assert ctx.bz2_decompress(good.data) == good.out, c.name
