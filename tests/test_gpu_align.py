"""GPU: sam2bed, psl2bed and rmsk2bed (Starch.align2bed, align2bed_device,
compress_aligned, the three commands).

Every comparison is equality of whole outputs against tests/align_oracle.py.
T is the number of lines per block of the per-line kernels, W the bytes from
which a copied tail is left to a whole wave.
"""
import os
import random
import subprocess

import pytest

from tests import align_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
LIMIT = oracle.LIMIT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def TW():
    import starch_amd
    return starch_amd.align_constants()


def check(ctx, fmt, data, **kw):
    """Unsorted and sorted output against the oracle; returns the oracle's unsorted BED."""
    want = oracle.convert(fmt, data, **kw)
    assert ctx.align2bed(data, fmt, sort=False, **kw) == want, (fmt, kw)
    assert ctx.align2bed(data, fmt, **kw) == oracle.sort_bed(want), (fmt, kw)
    return want


def check_error(ctx, fmt, data, line, text, **kw):
    """The refusal, nothing left behind, and the context still serves a good call."""
    import starch_amd
    for sort in (False, True):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.align2bed(data, fmt, sort=sort, **kw)
        assert e.value.code == -12 and str(e.value).endswith("%s: line %d: %s" % (oracle.COMMANDS[fmt], line, text)), str(e.value)
        with pytest.raises(starch_amd.StarchError) as e:   # no output is left behind
            ctx._output()
        assert e.value.code == -4
    good = {"sam": oracle.sam_row(b"r", 0, b"c", 5, b"3M"), "psl": oracle.psl_row(b"c", 4, 7, sizes=(3,)),
            "rmsk": oracle.rmsk_row(b"c", 5, 7)}[fmt]
    assert ctx.align2bed(good, fmt).startswith(b"c\t4\t7\t")


def rows_of(fmt, n):
    """n good records in descending position."""
    if fmt == "sam":
        return [oracle.sam_row(b"r%d" % k, 16 * (k & 1), b"chr%d" % (k % 3), n - k, b"5M2N5M") for k in range(n)]
    if fmt == "psl":
        return [oracle.psl_row(b"chr%d" % (k % 3), n - k, n - k + 30, b"+-", sizes=(10, 10), tstarts=[n - k, n - k + 20], qname=b"q%d" % k)
                for k in range(n)]
    return [oracle.rmsk_row(b"chr%d" % (k % 3), n - k, n - k + 9, b"C+"[k & 1:][:1], k % 5 == 0, k) for k in range(n)]


BAD = {"sam": (b"r\t0\tc\t0\t9\t3M", oracle.E_ZERO), "psl": (oracle.psl_row(b"c", 9, 9), oracle.E_STOP),
       "rmsk": (oracle.rmsk_row(b"c", 9, 8), oracle.E_END)}
BAD2 = {"sam": (b"r\t0\tc\t5\t9\t3Q", oracle.E_CIGAR), "psl": (b"c\t1", oracle.E_FEW21), "rmsk": (b"a b c", oracle.E_TOKENS)}
SPLIT = {"sam": dict(split=True), "psl": dict(split=True), "rmsk": {}}


# ---- each format on random records ----------------------------------------------------
@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_random_records_unsorted_sorted_and_archive(ctx, fmt):
    rng = random.Random(11 + oracle.FORMATS.index(fmt))
    data = oracle.random_input(fmt, rng, 400)
    lines, hdr, rec, unmapped = oracle.counts(fmt, data)
    assert rec == 400 and hdr >= 3 and (unmapped > 50) == (fmt == "sam")
    want = check(ctx, fmt, data)
    kept = check(ctx, fmt, data, keep_header=True)
    assert oracle.sort_bed(want) != want                       # the sort has work to do
    st = ctx.align_stats()
    assert (st["input_bytes"], st["input_lines"], st["header_lines"], st["records"], st["unmapped_dropped"], st["lines_out"],
            st["output_bytes"], st["sorted"]) == (len(data), lines, hdr, rec, unmapped, rec - unmapped + hdr, len(kept), 1)
    assert ctx.compress_aligned(data, fmt) == ctx.compress(oracle.sort_bed(want))
    assert ctx.align_stats()["sorted"] == 1
    if fmt == "sam":
        for kw in (dict(split=True), dict(split=True, split_deletions=True), dict(all_reads=True), dict(reduced=True),
                   dict(split=True, split_deletions=True, all_reads=True, reduced=True, keep_header=True)):
            got = check(ctx, fmt, data, **kw)
            assert got.count(b"\n") > want.count(b"\n") or kw == dict(reduced=True)
        assert ctx.align_stats()["unmapped_dropped"] == 0
    if fmt == "psl":
        assert check(ctx, fmt, data, split=True, keep_header=True).count(b"\n") > 2 * rec
        assert ctx.compress_aligned(data, fmt, split=True) == ctx.compress(oracle.sort_bed(oracle.psl(data, split=True)))


def test_align2bed_device_reads_hbm(ctx):
    import torch
    data = oracle.random_input("sam", random.Random(99), 300)
    want = oracle.sort_bed(oracle.sam(data, split=True))
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert ctx.align2bed_device(dev.data_ptr(), len(data), "sam", split=True) == len(want) and ctx._output() == want
    ctx.align2bed_device(dev.data_ptr(), len(data), "sam", keep_header=True, sort=False)
    assert ctx._output() == oracle.sam(data, keep_header=True) and ctx.align_stats()["sorted"] == 0


# ---- the hand-written table: every rule and every error kind ----------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_the_hand_written_table(ctx, case):
    fmt, kw, data, want = oracle.TABLE[case]
    if isinstance(want, tuple):
        check_error(ctx, fmt, data, want[0], want[1], **kw)
    else:
        assert check(ctx, fmt, data, **kw) == want


# ---- block boundaries -------------------------------------------------------------------
@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_line_counts_and_bad_lines_around_the_block_size(ctx, TW, fmt):
    T, _ = TW
    for n in (T - 1, T, T + 1, 2 * T + 1):
        rows = rows_of(fmt, n)
        assert check(ctx, fmt, b"\n".join(rows) + b"\n", **SPLIT[fmt]).count(b"\n") == n * (1 if fmt == "rmsk" else 2)
        assert check(ctx, fmt, b"\n".join(rows)).count(b"\n") == n
    rows = rows_of(fmt, 2 * T + 1)
    for at in (0, T - 1, T, 2 * T):
        bad = list(rows)
        bad[at] = BAD[fmt][0]
        check_error(ctx, fmt, b"\n".join(bad) + b"\n", at + 1, BAD[fmt][1], **SPLIT[fmt])
    bad = list(rows)
    bad[2 * T - 3], bad[T - 2] = BAD[fmt][0], BAD2[fmt][0]          # two bad lines in two blocks: the lower is named
    check_error(ctx, fmt, b"\n".join(bad), T - 1, BAD2[fmt][1])
    bad[T - 2], bad[5] = rows[T - 2], BAD2[fmt][0]
    check_error(ctx, fmt, b"\n".join(bad), 6, BAD2[fmt][1])
    bad[5] = rows[5]
    check_error(ctx, fmt, b"\n".join(bad), 2 * T - 2, BAD[fmt][1])


@pytest.mark.parametrize("fmt", ("sam", "rmsk"))
def test_kept_headers_at_the_block_edges(ctx, TW, fmt):
    """Header ordinals and the tally's per-wave counts across a block boundary, beside records of two lines."""
    T, _ = TW
    rows = rows_of(fmt, 2 * T + 1)
    for at in (0, T - 1, T, 2 * T):
        rows[at] = b"@CO\tline %d" % at if fmt == "sam" else b""
    data = b"\n".join(rows) + b"\n"
    modes = [dict(keep_header=True), dict(keep_header=False)] + ([dict(split=True, keep_header=True)] if fmt == "sam" else [])
    for kw in modes:
        got = check(ctx, fmt, data, **kw)
        assert ctx.align_stats()["header_lines"] == 4
        assert (b"_header\t3\t4\t" in got) == kw["keep_header"]


# ---- long tails -------------------------------------------------------------------------
def test_tails_around_the_wave_copy_threshold(ctx, TW):
    T, W = TW
    for n in (W - 1, W, W + 1):
        # SAM: the tail is CIGAR, a TAB and SEQ/QUAL: n bytes
        seq = b"ACGT" * (n // 4) + b"A" * (n % 4)
        tail = b"5M\t=\t7\t0\t" + seq[:(n - 10) // 2] + b"\t" + b"I" * (n - 10 - (n - 10) // 2)
        assert len(tail) == n
        rows = rows_of("sam", 70)
        rows[0] = rows[69] = b"rX\t16\tc\t7\t60\t" + tail
        rows[33] = b"@CO\t" + tail[4:]                               # a kept header line of n bytes
        assert len(rows[33]) == n
        data = b"\n".join(rows) + b"\n"
        for kw in ({}, dict(split=True), dict(reduced=True)):
            check(ctx, "sam", data, keep_header=True, **kw)
        # PSL: the tail is blockCount and the three lists: n bytes
        starts = b"".join(b"%d," % (10 ** 6 + 2 * j) for j in range(4))
        q = b"0,1,2,3,"
        q = q[:-1] + b"0" * (n - len(b"4\t1,1,1,1,\t%s\t%s" % (q, starts))) + b","   # qStarts is unread: pad it
        tail = b"4\t1,1,1,1,\t%s\t%s" % (q, starts)
        assert len(tail) == n
        rows = rows_of("psl", 70)
        rows[1] = rows[68] = oracle._P + b"+-\tq1\t70\t5\t66\tc\t2000000\t5\t900\t" + tail
        rows.insert(0, b"psLayout version 3")
        rows.insert(1, b"-" * n)
        data = b"\n".join(rows) + b"\n"
        check(ctx, "psl", data, keep_header=True)
        check(ctx, "psl", data, split=True, keep_header=True)


def test_a_64_kib_line_among_short_ones(ctx):
    seq = b"ACGT" * 8192
    rows = rows_of("sam", 130)
    rows[64] = oracle.sam_row(b"long", 0, b"chrL", 100, b"32768M", b"*\t0\t0\t" + seq + b"\t" + b"I" * len(seq))
    rows[0] = b"@CO\t" + seq * 2
    assert len(rows[64]) > 65536 and len(rows[0]) > 65536
    data = b"\n".join(rows)
    want = check(ctx, "sam", data, keep_header=True)
    assert want.count(seq) == 3 and b"chrL\t99\t32867\tlong\t0\t+\t" in want
    check(ctx, "sam", data, split=True)
    n = 6000
    sizes, tstarts = [3] * n, [10 + 5 * k for k in range(n)]
    rows = rows_of("psl", 130)
    rows[129] = oracle.psl_row(b"chrL", 10, 10 + 5 * n, b"-", 10 ** 6, sizes, tstarts)
    assert len(rows[129]) > 65536
    data = b"\n".join(rows) + b"\n"
    assert check(ctx, "psl", data, keep_header=True).count(b"\n") == 130   # (split would write the 64 KiB tail n times)


# ---- split fan-out ----------------------------------------------------------------------
def test_split_fan_out_beside_one_piece_neighbours(ctx):
    counts = (1, 2, 63, 64, 65, 300)
    rows = [oracle.sam_row(b"one%d" % k, 0, b"chr1", 9000 - k, b"7M") for k in range(64)]
    for j, n in enumerate(counts):
        rows[3 + 9 * j] = oracle.sam_row(b"many%d" % n, 16, b"chr2", 100 * j + 1, b"3N".join([b"2M1I1D1M"] * n) + b"4S")
    data = b"\n".join(rows) + b"\n"
    assert check(ctx, "sam", data, split=True).count(b"\n") == 64 - len(counts) + sum(counts)
    assert check(ctx, "sam", data, split=True, split_deletions=True).count(b"\n") == 64 - len(counts) + 2 * sum(counts)
    assert check(ctx, "sam", data, split=True, reduced=True).count(b"\tmany300\t16\t-\n") == 300
    assert ctx.align_stats()["lines_out"] == 64 - len(counts) + sum(counts)
    rows = [oracle.psl_row(b"chr1", 9000 - k, 9010 - k, qname=b"one%d" % k) for k in range(64)]
    for j, n in enumerate(counts):
        rows[3 + 9 * j] = oracle.psl_row(b"chr2", 5, 5 + 7 * n, (b"+-", b"-")[j & 1], 10 ** 5, [1 + k % 4 for k in range(n)],
                                         [5 + 7 * k for k in range(n)], b"many%d" % n)
    data = b"\n".join(rows) + b"\n"
    assert check(ctx, "psl", data, split=True).count(b"\n") == 64 - len(counts) + sum(counts)
    assert check(ctx, "psl", data).count(b"\n") == 64


# ---- limits -----------------------------------------------------------------------------
def test_limits(ctx):
    row = lambda pos, cigar: oracle.sam_row(b"r", 0, b"c", pos, cigar)
    assert check(ctx, "sam", row(1, b"999999999M999999999D")).startswith(b"c\t0\t1999999998\t")
    check_error(ctx, "sam", row(1, b"1000000000M"), 1, oracle.E_CIGAR)
    assert check(ctx, "sam", row(LIMIT - 999999999 + 1, b"999999999M"), split=True).startswith(b"c\t%d\t%d\t" % (LIMIT - 999999999, LIMIT))
    check_error(ctx, "sam", row(LIMIT - 999999999 + 2, b"999999999M"), 1, oracle.E_OVER, split=True)
    assert check(ctx, "sam", row(LIMIT, b"*")).startswith(b"c\t%d\t%d\t" % (LIMIT - 1, LIMIT))
    check_error(ctx, "sam", row(LIMIT, b"1M1N"), 1, oracle.E_OVER)
    check_error(ctx, "sam", row(0, b"5M"), 1, oracle.E_ZERO)
    rev = lambda tsize: oracle.psl_row(b"c", 1, 9, b"+-", tsize, (4, 4), (0, 96))
    assert check(ctx, "psl", rev(100), split=True).startswith(b"c\t96\t100\t")
    check_error(ctx, "psl", rev(99), 1, oracle.E_UNDER, split=True)
    check(ctx, "psl", rev(99))                                      # unread without split
    check(ctx, "psl", oracle.psl_row(b"c", LIMIT - 1, LIMIT, b"+", LIMIT, (1,), (LIMIT - 1,)), split=True)
    check_error(ctx, "psl", oracle.psl_row(b"c", LIMIT - 1, LIMIT, b"+", LIMIT, (2,), (LIMIT - 1,)), 1, oracle.E_OVER, split=True)
    assert check(ctx, "rmsk", oracle.rmsk_row(b"c", LIMIT, LIMIT)).startswith(b"c\t%d\t%d\t" % (LIMIT - 1, LIMIT))


# ---- headers ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_empty_headers_only_and_single_lines(ctx, fmt):
    record = rows_of(fmt, 1)[0]
    head = {"sam": b"@HD\tVN:1.6\n\n@CO\tx", "psl": b"psLayout version 3\n\nmatch\n-----", "rmsk": b" SW perc\nscore div.\n  \t"}[fmt]
    for kw in ({}, dict(keep_header=True)):
        assert check(ctx, fmt, b"", **kw) == b""
        assert check(ctx, fmt, b"\n", **kw).count(b"\n") == len(kw)
        assert check(ctx, fmt, head, **kw).count(b"\n") == (head.count(b"\n") + 1) * len(kw)      # headers only, no final '\n'
        assert check(ctx, fmt, head + b"\n", **kw).count(b"\n") == (head.count(b"\n") + 1) * len(kw)
        assert check(ctx, fmt, record, **kw).count(b"\n") == 1   # one record, no '\n'
        assert check(ctx, fmt, head + b"\n" + record + b"\n\n" + record, **kw).count(b"\n") == 2 + (head.count(b"\n") + 2) * len(kw)
    st = ctx.align_stats()
    assert (st["input_lines"], st["header_lines"], st["records"]) == (head.count(b"\n") + 4, head.count(b"\n") + 2, 2)


def test_psl_header_end_in_the_second_block(ctx, TW):
    T, _ = TW
    junk = [b"psLayout version 3"] + [b"not\ta\trecord %d" % k for k in range(T + 5)]
    rows = rows_of("psl", T)
    data = b"\n".join(junk + [b"-----------"] + rows) + b"\n"
    for kw in ({}, dict(keep_header=True), dict(split=True, keep_header=True)):
        check(ctx, "psl", data, **kw)
    assert ctx.align_stats()["header_lines"] == T + 7
    check_error(ctx, "psl", b"\n".join(junk + rows) + b"\n", 1, oracle.E_NODASH)
    check_error(ctx, "psl", b"\n".join(junk[1:] + [b"-----"] + rows) + b"\n", 1, oracle.E_FEW21)   # no psLayout: no header


# ---- the commands -------------------------------------------------------------------------
def _cli(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_command_against_the_oracle(ctx, tmp_path, fmt):
    cmd = os.path.join(BUILD, oracle.COMMANDS[fmt])
    data = oracle.random_input(fmt, random.Random(3), 120)
    path = tmp_path / ("a." + fmt)
    path.write_bytes(data)
    want = oracle.sort_bed(oracle.convert(fmt, data))
    r = _cli([cmd, str(path)])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want
    flags, kw = {"sam": (["--split-with-deletions", "--all-reads"], dict(split=True, split_deletions=True, all_reads=True)),
                 "psl": (["--split"], dict(split=True)), "rmsk": ([], {})}[fmt]
    with open(path, "rb") as f:
        r = _cli([cmd, "--do-not-sort", "--keep-header"] + flags + ["-"], stdin=f)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == oracle.convert(fmt, data, keep_header=True, **kw)
    r = _cli([cmd, "--output=starch", str(path)])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == ctx.compress_aligned(data, fmt)
    (tmp_path / "a.starch").write_bytes(r.stdout)
    r = _cli([os.path.join(BUILD, "unstarch"), str(tmp_path / "a.starch")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want
    (tmp_path / "bad").write_bytes(data + BAD[fmt][0] + b"\n")
    r = _cli([cmd, str(tmp_path / "bad")])
    assert r.returncode == 22 and r.stdout == b""
    assert b"%s: line %d: %s" % (oracle.COMMANDS[fmt].encode(), data.count(b"\n") + 1, BAD[fmt][1].encode()) in r.stderr
