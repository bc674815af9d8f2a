"""Inputs for the tests of the copies a writing thread leaves to its wave.

A line of W = sort_constants()[1] bytes or more (without its newline) is copied
by the whole wave, a shorter one by its thread.  The lines here have an exact
size, so a test can put long ones at chosen positions of a wave.
"""
SHORT = 40
WAVE_SPOTS = (0, 63, 128)      # two lanes of the first wave, none of the second, one of the third
WAVE_LINES = 130


def line(k, size, off=0, width=5, score=b"1"):
    """Line k of a layout with 10 bases per slot: chr1, [10k + off, 10k + off + width), an
    id, a score and padding, `size` bytes without the newline"""
    head = b"chr1\t%d\t%d\tn%d\t%s\t" % (10 * k + off, 10 * k + off + width, k, score)
    assert size > len(head)
    return head + b"p" * (size - len(head)) + b"\n"


def lines(n, long_at, W, **kw):
    """n lines, those at the positions long_at of W + 3 bytes, the others short"""
    return b"".join(line(k, W + 3 if k in long_at else SHORT, **kw) for k in range(n))


def wave_pairs(W):
    """(reference, second input) twice: long lines at WAVE_SPOTS of both inputs, and none
    long.  Line k of the second input lies inside reference line k and after line k - 1
    of the reference ends, so it is hit k, the one map line of reference line k, and the
    right element of reference line k."""
    return [(lines(WAVE_LINES, spots, W), lines(WAVE_LINES, spots, W, off=1, width=2)) for spots in (WAVE_SPOTS, ())]
