"""GPU: sort-bed (Starch.sort_bed / sort_check / compress_sorted, the sort-bed
command, starch3 --sort).

The oracle is Python and takes nothing from the code under test: the input is
cut into lines at "\\n" (a last line without one is a line), and the expected
output is sorted() of the lines by (chrom bytes, int(start), int(stop)), every
line ending in "\\n".  Python compares bytes as unsigned values with a proper
prefix first, and sorted() is stable, so lines with equal keys keep their
input order -- the contract of include/starch_amd.h.  Every comparison is
equality of whole outputs, byte for byte.
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
SORTBED = os.path.join(BUILD, "sort-bed")
STARCH3 = os.path.join(BUILD, "starch3")
I63 = 2 ** 63 - 1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def consts():
    import starch_amd
    return starch_amd.sort_constants()   # (lines per radix tile, wave-copy threshold in bytes)


def _split(bed):
    lines = bed.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def _key(ln):
    f = ln.split(b"\t")
    return (f[0], int(f[1]), int(f[2]))


def oracle(bed):
    return b"".join(ln + b"\n" for ln in sorted(_split(bed), key=_key))


def first_descent(bed):
    keys = [_key(ln) for ln in _split(bed)]
    for i in range(1, len(keys)):
        if keys[i] < keys[i - 1]:
            return i + 1
    return 0


def _check(ctx, bed):
    got = ctx.sort_bed(bed)
    assert got == oracle(bed)
    return got


def _shuffled(lines, seed):
    lines = list(lines)
    random.Random(seed).shuffle(lines)
    return b"".join(ln + b"\n" for ln in lines)


# ---- 1. shapes ------------------------------------------------------------------
def test_shapes(ctx):
    assert ctx.sort_bed(b"") == b""
    assert ctx.sort_stats()["n_lines"] == 0
    assert ctx.sort_bed(b"chr1\t5\t9\n") == b"chr1\t5\t9\n"
    assert ctx.sort_bed(b"chr1\t5\t9") == b"chr1\t5\t9\n"
    assert ctx.sort_bed(b"chr1\t5\t9\tx\nchr1\t7\t8") == b"chr1\t5\t9\tx\nchr1\t7\t8\n"   # sorted, no final newline
    assert ctx.sort_stats()["already_sorted"] == 1
    assert ctx.sort_bed(b"chr2\t5\t9\nchr1\t7\t8\n") == b"chr1\t7\t8\nchr2\t5\t9\n"
    s = ctx.sort_stats()
    assert (s["n_lines"], s["n_chromosomes"], s["already_sorted"], s["first_unsorted_line"]) == (2, 2, 0, 2)
    assert ctx.sort_bed(b"chr1\t7\t8\nchr1\t5\t9") == b"chr1\t5\t9\nchr1\t7\t8\n"       # swapped, no final newline


# ---- 2. stability across tiles ------------------------------------------------------
def test_ties_keep_input_order_across_tiles(ctx, consts):
    n = 3 * consts[0] + 137
    tied = [b"chr1\t100\t200\tid%d" % i for i in range(n)]
    bed = b"".join(ln + b"\n" for ln in tied)
    assert ctx.sort_bed(bed) == bed
    # interleaved with a second key that sorts earlier: both runs keep their order
    early = [b"chr1\t50\t60\te%d" % i for i in range(n)]
    mixed = b"".join(a + b"\n" + b + b"\n" for a, b in zip(tied, early))
    want = b"".join(ln + b"\n" for ln in early) + bed
    assert oracle(mixed) == want
    assert ctx.sort_bed(mixed) == want
    assert ctx.sort_stats()["radix_passes"] >= 1


# ---- 3. digit skipping ----------------------------------------------------------------
def _digit_cases():
    r = random.Random(5)
    cases = {}
    cases["start_bits_ge_32"] = [b"chr1\t%d\t%d\tr%d" % (k << 32, I63, k) for k in range(300)]
    cases["start_top_byte"] = [b"chr1\t%d\t%d\tr%d" % ((k % 128) << 56 | 0x1234, I63, k) for k in range(384)]
    cases["stop_above_bit_40"] = [b"chr1\t77\t%d\tr%d" % (((k % 200) << 41) + 78, k) for k in range(400)]
    cases["zero_and_max"] = [b"chr1\t%d\t%d\tr%d" % (r.choice([0, I63]), r.choice([0, I63]), k) for k in range(300)]
    cases["leading_zeros_tie"] = [b"chr1\t8\t9\tz", b"chr1\t007\t9\ta", b"chr1\t7\t9\tb", b"chr1\t07\t09\tc",
                                  b"chr1\t0000000000000000007\t9\td", b"chr1\t6\t9\ty"]
    return cases


@pytest.mark.parametrize("name", sorted(_digit_cases()))
def test_digit_skipping(ctx, name):
    lines = _digit_cases()[name]
    bed = b"".join(ln + b"\n" for ln in lines) if name == "leading_zeros_tie" else _shuffled(lines, 9)
    _check(ctx, bed)
    s = ctx.sort_stats()
    assert s["already_sorted"] == 0 and 1 <= s["radix_passes"] <= 20
    if name == "start_bits_ge_32":
        assert s["radix_passes"] == 2            # 300 values of k: bytes 4 and 5 of start, nothing else
    if name == "start_top_byte":
        assert s["radix_passes"] == 1


def test_leading_zeros_are_a_tie(ctx):
    bed = b"chr1\t8\t9\tz\nchr1\t007\t9\ta\nchr1\t7\t9\tb\n"
    assert ctx.sort_bed(bed) == b"chr1\t007\t9\ta\nchr1\t7\t9\tb\nchr1\t8\t9\tz\n"
    bed = b"chr1\t8\t9\tz\nchr1\t7\t9\tb\nchr1\t007\t9\ta\n"
    assert ctx.sort_bed(bed) == b"chr1\t7\t9\tb\nchr1\t007\t9\ta\nchr1\t8\t9\tz\n"


# ---- 4. names -----------------------------------------------------------------------------
def test_name_prefix_order(ctx):
    names = [b"chr1_x", b"chr10", b"chr", b"chr1", b"chr1_x", b"chr", b"chr10", b"chr1"]
    bed = b"".join(nm + b"\t%d\t%d\n" % (100 - i, 200) for i, nm in enumerate(names))
    got = _check(ctx, bed)
    assert [ln.split(b"\t")[0] for ln in _split(got)] == [b"chr", b"chr", b"chr1", b"chr1", b"chr10", b"chr10",
                                                          b"chr1_x", b"chr1_x"]
    assert ctx.sort_stats()["n_chromosomes"] == 4


def test_long_and_high_byte_names(ctx):
    a = b"A" * 30 + b"b" + b"C" * 9
    b = b"A" * 30 + b"a" + b"C" * 9
    assert len(a) == 40 and len(b) == 40
    hi = b"chr\xe9\xff\x80", b"chr\x7f", b"chrz", b"\x80", b"\xff\xfe"
    lines = [nm + b"\t%d\t%d\tr%d" % (k % 7, 10 + k % 3, k) for k, nm in enumerate([a, b] * 20 + list(hi) * 8)]
    _check(ctx, _shuffled(lines, 2))
    assert ctx.sort_stats()["n_chromosomes"] == 7


def test_three_thousand_names(ctx):
    r = random.Random(17)
    names = [b"scaffold_%05d_unplaced_%d" % (r.randrange(100000), k) for k in range(3000)]
    lines = [nm + b"\t%d\t%d\tr%d" % (r.randrange(1000), 1000 + r.randrange(50), j) for nm in names for j in range(3)]
    _check(ctx, _shuffled(lines, 4))
    assert ctx.sort_stats()["n_chromosomes"] == 3000


# ---- 5. gather -------------------------------------------------------------------------------
def _line_of(total, k):
    """a line of `total` bytes with its newline, start descending in k"""
    head = b"chr1\t%d\t%d\t" % (5000 - k, 9000)
    assert total >= len(head) + 2
    return head + bytes([97 + k % 26]) * (total - len(head) - 1)


def test_long_line_between_short_lines(ctx):
    short = [b"chr1\t%d\t%d" % (400 - k, 99) for k in range(200)]
    assert all(len(s) + 1 == 12 for s in short)
    lines = short[:100] + [b"chr1\t250\t251\t" + b"Q" * 10240] + short[100:]
    _check(ctx, b"".join(ln + b"\n" for ln in lines))


def test_line_lengths_round_the_copy_paths(ctx, consts):
    t = consts[1]
    lengths = [63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 4 * t + 3]
    lines = [_line_of(n, k) for k, n in enumerate(lengths * 3)]
    assert sorted({len(ln) + 1 for ln in lines}) == sorted(set(lengths))
    _check(ctx, b"".join(ln + b"\n" for ln in lines))
    _check(ctx, b"\n".join(lines))                      # ... and a long last line without a newline


# ---- 6. random ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuffled():
    import starch_amd
    lines = _split(starch_amd.gen_bed(0, 200_000))
    perm = np.random.RandomState(20261019).permutation(len(lines))
    bed = b"".join(lines[i] + b"\n" for i in perm)
    return bed, oracle(bed)


def test_random_against_oracle(ctx, shuffled):
    bed, want = shuffled
    assert ctx.sort_bed(bed) == want
    s = ctx.sort_stats()
    assert s["n_lines"] == 200_000 and s["n_chromosomes"] == 24 and s["already_sorted"] == 0
    assert s["input_bytes"] == len(bed) and 1 <= s["radix_passes"] <= 20
    again = ctx.sort_bed(want)
    assert again == want
    s = ctx.sort_stats()
    assert s["already_sorted"] == 1 and s["first_unsorted_line"] == 0 and s["radix_passes"] == 0


def test_sort_check(ctx, shuffled):
    bed, want = shuffled
    line = first_descent(bed)
    assert line > 0
    assert ctx.sort_check(bed) == line
    assert ctx.sort_stats()["first_unsorted_line"] == line
    assert ctx.sort_check(want) == 0
    # a descent in the last line only, past a tile boundary
    assert ctx.sort_check(want + b"chr1\t0\t1\n") == 200_001


# ---- 7. refusals -----------------------------------------------------------------------------------
BAD_LINES = {
    "empty": b"",
    "two_fields": b"chr1\t5",
    "one_field": b"chr1",
    "non_digit_start": b"chr1\t5x\t9",
    "non_digit_stop": b"chr1\t5\t-9",
    "crlf_bed3": b"chr1\t5\t9\r",
    "twenty_digits": b"chr1\t00000000000000000005\t9",
    "above_int63": b"chr1\t5\t9223372036854775808",
    "track_header": b"track name=\"x\"\tdescription\t1",
    "hash_header": b"#chrom\t5\t9",
}


@pytest.mark.parametrize("kind", sorted(BAD_LINES))
def test_malformed_line_is_refused(ctx, kind):
    import starch_amd
    good = [b"chr1\t%d\t%d\tok" % (1000 - k, 2000) for k in range(700)]
    at = 301
    lines = good[:at - 1] + [BAD_LINES[kind]] + good[at - 1:]
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.sort_bed(b"".join(ln + b"\n" for ln in lines))
    assert e.value.code == -12
    assert "line %d:" % at in str(e.value)
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    with pytest.raises(starch_amd.StarchError) as e3:
        ctx.sort_check(b"".join(ln + b"\n" for ln in lines))
    assert e3.value.code == -12 and "line %d:" % at in str(e3.value)
    bed = b"".join(ln + b"\n" for ln in good)
    assert ctx.sort_bed(bed) == oracle(bed)                # the context serves the next call


def test_largest_values_are_accepted(ctx):
    import starch_amd
    bed = b"chr1\t9223372036854775807\t9223372036854775807\nchr1\t0009223372036854775806\t1\n"
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.sort_bed(bed)                                  # 22 digits, whatever their value
    assert e.value.code == -12 and "line 2:" in str(e.value)
    bed = b"chr1\t9223372036854775807\t9223372036854775807\nchr1\t9223372036854775806\t1\n"
    _check(ctx, bed)


# ---- 8. with the encoder ---------------------------------------------------------------------------------
def test_compress_sorted(ctx, shuffled):
    bed, want = shuffled
    arch = ctx.compress_sorted(bed)
    assert arch == ctx.compress(want)
    assert ctx.unstarch(arch) == want


def test_cat_of_sorted_parts_is_sorted_whole(ctx):
    r = random.Random(23)
    def part(tag, n):
        out = []
        for k in range(n):
            s = r.randrange(40)                        # few values: many tied keys, within and across the parts
            out.append(b"%s\t%d\t%d\t%s%d" % (r.choice([b"chr1", b"chr10", b"chr2"]), s, s + r.randrange(1, 3), tag, k))
        return b"".join(ln + b"\n" for ln in out)
    a, b = part(b"a", 5000), part(b"b", 5000) + b"chrOnlyB\t1\t2\n"
    parts = [ctx.compress(ctx.sort_bed(a)), ctx.compress(ctx.sort_bed(b))]
    whole = ctx.sort_bed(a + b)
    assert whole == oracle(a + b)
    assert ctx.cat(parts) == ctx.compress(whole)


# ---- 9. commands -----------------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_sort_bed_command(tmp_path):
    r = random.Random(3)
    def lines(n, tag):
        return [b"%s\t%d\t%d\t%s%d" % (r.choice([b"chrX", b"chr1", b"chr11"]), r.randrange(10 ** 6), 10 ** 6 + k, tag, k)
                for k in range(n)]
    a = b"\n".join(lines(3000, b"a"))                    # no final newline: the command adds it
    b = b"".join(ln + b"\n" for ln in lines(2000, b"b"))
    fa, fb = tmp_path / "a.bed", tmp_path / "b.bed"
    fa.write_bytes(a)
    fb.write_bytes(b)
    one = _run([SORTBED, str(fa)])
    assert one.returncode == 0 and one.stdout == oracle(a)
    two = _run([SORTBED, str(fa), str(fb)])
    assert two.returncode == 0 and two.stdout == oracle(a + b"\n" + b)
    piped = _run([SORTBED, "-"], input=b)
    assert piped.returncode == 0 and piped.stdout == oracle(b)
    mixed = _run([SORTBED, str(fa), "-"], input=b)
    assert mixed.returncode == 0 and mixed.stdout == two.stdout
    bad = _run([SORTBED, str(fb), "-"], input=b"chr1\t5\n")
    assert bad.returncode == 22 and bad.stdout == b"" and b"line 2001:" in bad.stderr


def test_check_sort_command(tmp_path):
    good = b"chr1\t5\t9\nchr1\t5\t10\nchr10\t1\t2\nchr2\t0\t1\n"
    fg, fu = tmp_path / "good.bed", tmp_path / "unsorted.bed"
    fg.write_bytes(good)
    fu.write_bytes(good + b"chr10\t7\t8\n")
    r = _run([SORTBED, "--check-sort", str(fg)])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    r = _run([SORTBED, "--check-sort", str(fu)])
    assert r.returncode == 1 and r.stdout == b"" and b"line 5 " in r.stderr


def test_starch3_sort(tmp_path, shuffled):
    bed, want = shuffled
    bed, want = bed[:bed.index(b"\n", 400_000) + 1], None
    want = oracle(bed)
    plain = _run([STARCH3], input=want)
    assert plain.returncode == 0 and plain.stdout[:4] == b"\xca\x5c\xad\x1a"
    piped = _run([STARCH3, "--sort"], input=bed)
    assert piped.returncode == 0 and piped.stdout == plain.stdout
    f = tmp_path / "shuffled.bed"
    f.write_bytes(bed)
    named = _run([STARCH3, "--sort", str(f)])
    assert named.returncode == 0 and named.stdout == plain.stdout
    refused = _run([STARCH3, "--sort"], input=b"chr1\t1\t2\n\nchr1\t0\t1\n")
    assert refused.returncode == 22 and refused.stdout == b"" and b"line 2:" in refused.stderr


# ---- 10. device entry ----------------------------------------------------------------------------------------------
def test_device_entry(ctx):
    import torch
    import starch_amd
    pieces = [(23, 1000, 3000), (0, 999_000, 3000), (23, 0, 500), (11, 5, 2000)]   # chrY, chr1, chrY, chr2
    sizes = [starch_amd.gen_perpos_device(c, first=f, count=n) for c, f, n in pieces]
    dev = torch.empty(sum(sizes) + 64, dtype=torch.uint8, device="cuda:0")
    at = 0
    for (c, f, n), sz in zip(pieces, sizes):
        assert starch_amd.gen_perpos_device(c, dev.data_ptr() + at, sz, first=f, count=n) == sz
        at += sz
    torch.cuda.synchronize()
    host = dev[:at].cpu().numpy().tobytes()
    assert host.count(b"\n") == 8500 and first_descent(host) == 3001
    k = ctx.sort_bed_device(dev.data_ptr(), at)
    assert k == at and ctx.output_device_ptr() != 0
    from_device = ctx._output()
    assert from_device == oracle(host)
    assert ctx.sort_bed(host) == from_device
