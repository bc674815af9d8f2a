"""GPU: the inverse transform at its edges, against the oracle's restatement
(oracle_untransform, pinned by test_untransform_oracle.py) per segment, and by
the archive round trip unstarch(compress(bed)) == bed.

The kernels run one thread per line of the transformed text in tiles of
kT = 256 lines; cd comes from a max-scan over the lines, the stops from one
inclusive sum over all segments, modulo 2^64.  The cases put a tile boundary
next to a p-line and next to a segment's first line, make many one-line
segments, let the global sum wrap, and give values of 19 digits, negative
values and remainders of 0, 1 and 5000 bytes."""
import pytest

from tests import oracle_lib

kT = 256


def _lines(chr_, start, n, step=10, length=7, rem=b""):
    """n sorted lines; the first needs a p-line (length != 0), the rest keep its length."""
    return b"".join(b"%s\t%d\t%d%s\n" % (chr_, start + k * step, start + k * step + length, rem) for k in range(n))


def _text_lines(n, p_at=None):
    """One chromosome whose transformed text has n lines: a p-line first and, if
    p_at is given, a second p-line as line p_at (0-based) of the text."""
    if p_at is None:
        return _lines(b"chr1", 100, n - 1)
    head = _lines(b"chr1", 100, p_at - 1)
    return head + _lines(b"chr1", 100 + 10 * p_at, n - 1 - p_at, length=9)


def _two_segments(first_len):
    """The second segment's first line is line first_len of the text."""
    return _lines(b"chr1", 100, first_len - 1) + _lines(b"chr2", 5, 20, length=3)


BIG = 1 << 62


def _cases():
    for n in (255, 256, 257, 511, 512, 513):
        yield "text_lines_%d" % n, _text_lines(n), n
    yield "p_line_last_of_tile", _text_lines(300, p_at=kT - 1), 300
    yield "p_line_first_of_tile", _text_lines(300, p_at=kT), 300
    yield "segment_starts_on_tile_first_line", _two_segments(kT), kT + 21
    yield "segment_starts_on_tile_last_line", _two_segments(kT - 1), kT + 20
    yield "one_line_segments_40", b"".join(b"c%02d\t%d\t%d\n" % (k, 10 + k, 10 + k + k % 3) for k in range(40)), None
    # every segment's stops stay below 2^63; the sum over the segments passes 2^64 with the fourth
    yield "sum_wraps_across_segments", b"".join(_lines(b"w%d" % k, BIG + 1000 * k, 3) for k in range(7)), None
    yield "overlapping_negative_v", _lines(b"chr1", 50, 300, step=1, length=1000), None
    yield "value_of_19_digits", _lines(b"chr1", 10 ** 18, 3), None
    yield "remainder_1_byte", _lines(b"chr1", 7, 5, rem=b"\tx"), None
    yield "remainder_5000_bytes", _lines(b"chr1", 7, 3, rem=b"\t" + b"y" * 5000), None


CASES = list(_cases())

# The forward transform never writes a tab with nothing after it (it drops the
# tab), so that text is written by hand and has no round trip.
EMPTY_REMAINDER = b"p7\n7\t\n3\t\np0\n12\t\n"


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def oracle_segments(bed, text_lines=None):
    """[(chromosome, transformed text, its BED lines by the oracle)]; the oracle's round trip must hold."""
    text, segs = oracle_lib.transform(bed)
    if text_lines is not None:
        assert text.count(b"\n") == text_lines
    out = [(c, t, oracle_lib.untransform(t, c)) for c, _, t in segs]
    assert b"".join(w for _, _, w in out) == bed
    return out


@pytest.mark.parametrize("name,bed,text_lines", CASES, ids=[c[0] for c in CASES])
def test_oracle_round_trip_of_the_edge_cases(name, bed, text_lines):
    """CPU: the expectation itself -- the oracle inverts its own transform on every case."""
    segs = oracle_segments(bed, text_lines)
    if name == "sum_wraps_across_segments":
        stops = [int(w.split(b"\n")[-2].split(b"\t")[2]) for _, _, w in segs]
        assert max(stops) < 1 << 63 and sum(stops[:3]) < 1 << 64 <= sum(stops[:4])
    if name == "overlapping_negative_v":
        assert segs[0][1].count(b"\n-") > 250
    if name.startswith("p_line_"):
        lines = segs[0][1].split(b"\n")
        at = kT - 1 if name == "p_line_last_of_tile" else kT
        assert [i for i, l in enumerate(lines) if l[:1] == b"p"] == [0, at]


def test_oracle_keeps_a_tab_with_an_empty_remainder():
    assert oracle_lib.untransform(EMPTY_REMAINDER, b"chr1") == b"chr1\t7\t14\t\nchr1\t17\t24\t\nchr1\t36\t36\t\n"


@pytest.mark.gpu
def test_untransform_tab_with_empty_remainder(ctx):
    assert ctx.untransform(EMPTY_REMAINDER, b"chr1") == oracle_lib.untransform(EMPTY_REMAINDER, b"chr1")


@pytest.mark.gpu
@pytest.mark.parametrize("name,bed,text_lines", CASES, ids=[c[0] for c in CASES])
def test_untransform_edges(ctx, name, bed, text_lines):
    for chr_, text, want in oracle_segments(bed, text_lines):
        assert ctx.untransform(text, chr_) == want
    assert ctx.unstarch(ctx.compress(bed)) == bed
