"""The three transform paths write the same bytes for the same lines.

One list of short lines (`core`) is transformed three times: alone (the single
pass, k_tf_fused), with one line longer than the single pass's halo in the
middle (it hands the input to k_tf1 / k_tf2), and with one line whose start
does not parse in the middle (handed over as well; k_tf1 then reports the
failed sscanf and the general path, k_parse ... k_emit, runs).  Each result is
checked against the oracle, and every segment of `core` must come out of the
other two paths exactly as it came out of the single pass.

A transform context picks its path from the text ratio of its last input, so
every input gets a new context: that one starts with the single pass."""
import random
import re

import pytest

from tests import oracle_lib

pytestmark = pytest.mark.gpu

TILE = 8192
# what the SWAR parser accepts: <= 128 bytes, no NUL, two fields of 1..18 plain digits
FAST_LINE = re.compile(rb"[^\t\n\0]+\t[0-9]{1,18}\t[0-9]{1,18}(\t[^\n\0]*)?\n")

# chr1 -> chr11 and contig00B1 -> contig00B12 differ only in length,
# contig00A1 -> contig00B1 only in the 9th byte (names are compared 8 bytes at a time)
CHROMS = ["chr1", "chr11", "chr2", "contig00A1", "contig00B1", "contig00B12"]
PER_CHROM = 100
REMS = ["", "\t", "\tpeak%d", "\tname%d\t0\t+\tAAAACCCCGGGGTTTTAAAACCCCGGGGTTTT"]


def _core():
    r = random.Random(11)
    lines = []
    for c in CHROMS:
        pos = 0
        for k in range(PER_CHROM):
            pos += r.randint(0, 500)
            shape = k % 10
            if shape == 3:                      # stop < start: the "p" line is cut short
                a, b = pos + 40, pos
            elif shape == 4:                    # the same delta with the other sign
                a, b = pos, pos + 40
            elif shape == 6:                    # 18 digits, positive 18-digit delta after a small one
                a, b = 1 + k, 999999999999999999 - k
            elif shape == 7:                    # 18 digits both, negative 18-digit delta
                a, b = 999999999999999999 - k, 100000000000000000 + k
            elif shape in (8, 9):               # equal deltas: no "p" line for the second
                a, b = pos, pos + 150
            else:
                a, b = pos, pos + r.randint(1, 300)
            rem = REMS[(k // 2 + k // 10) % 4]
            lines.append("%s\t%d\t%d%s\n" % (c, a, b, rem % k if "%d" in rem else rem))
    return [s.encode() for s in lines]


CORE = _core()
MID = len(CORE) // 2                            # between chr2 and contig00A1
LONG_LINE = b"chrL\t5\t9\t" + b"A" * 1100 + b"\n"          # longer than the 1 KiB halo
STALE_LINE = b"chrN\tx\t7\n"                                # start fails to parse: a stale value


def _with(line):
    return b"".join(CORE[:MID] + [line] + CORE[MID:])


def _transform(data):
    import starch_amd
    c = starch_amd.Starch(0)
    try:
        return c.transform(data)
    finally:
        c.close()


@pytest.fixture(scope="module")
def core_result():
    data = b"".join(CORE)
    assert all(FAST_LINE.fullmatch(s) and len(s) <= 128 for s in CORE)
    assert 2 * TILE < len(data) <= 40960
    assert any(s.endswith(b"\t\n") for s in CORE) and any(s.count(b"\t") == 2 for s in CORE)
    text, segs = _transform(data)
    otext, osegs = oracle_lib.transform(data)
    assert [s[0] for s in osegs] == [c.encode() for c in CHROMS]
    assert all(s[1] == PER_CHROM for s in osegs)
    assert text == otext
    assert segs == osegs
    return segs


def test_core_alone(core_result):
    text = b"".join(s[2] for s in core_result)
    assert b"p-40" in text and b"p-40\n" not in text            # negative delta: the newline is cut off
    assert b"p-8999999999999999" in text and b"p9999999999999999" in text   # 18-digit deltas


@pytest.mark.parametrize("line", [LONG_LINE, STALE_LINE], ids=["long-line-two-pass", "stale-value-general"])
def test_other_paths_write_the_same_segments(core_result, line):
    data = _with(line)
    text, segs = _transform(data)
    otext, osegs = oracle_lib.transform(data)
    assert text == otext
    assert segs == osegs
    # the inserted line is a segment of its own, so it changes no line of core
    k = len(CHROMS) // 2
    assert segs[k][0] == line.split(b"\t")[0] and segs[k][1] == 1
    assert segs[:k] + segs[k + 1:] == core_result


EXTREMES = [
    b"chrA\t-9223372036854775808\t0\n",         # delta wraps to INT64_MIN: "p-9"
    b"chrA\t+1\t 9223372036854775807\n",        # 19-digit delta, written whole
    b"chrA\t 9223372036854775807\t+1\n",        # 19-digit negative delta: no newline left
    b"chrA\t-5\t-2\tx\n",
    b"chrA\t99999999999999999999\t-99999999999999999999\n",   # sscanf clamps both
    b"chrB\t-9223372036854775808\t0\t\n",
    b"chrB\t0\t-9223372036854775808\n",
    b"chrB\t +7\t +9\tname\t0\t-\n",
]


@pytest.mark.parametrize("stale", [False, True], ids=["two-pass", "general"])
def test_int64_extremes_byte_serial(stale):
    lines = EXTREMES * 40                        # 320 lines: more than one 256-line workgroup
    if stale:
        lines = lines[:160] + [STALE_LINE] + lines[160:]
    data = b"".join(lines)
    assert not any(FAST_LINE.fullmatch(s) for s in EXTREMES)
    text, segs = _transform(data)
    otext, osegs = oracle_lib.transform(data)
    assert b"p-9-9223372036854775808\n" in otext
    assert b"p9223372036854775806\n" in otext and b"p-9223372036854775806" in otext
    assert text == otext
    assert segs == osegs
