"""GPU: bam2bed (Starch.bam2bed, bam2bed_device, compress_bam, the command).

Every comparison is equality of whole outputs against tests/bam_oracle.py, and,
where the SAM text exists, against align2bed of that text on the same context.
T is the bytes of a framing tile (tile t is the bytes [t * T, (t + 1) * T) of the
inflated file), N the records per block of the per-record kernels, W the l_seq or
B count from which a record is left to a whole wave.

A record needs a read name of at least its NUL, so the shortest record that the
definition accepts has 37 bytes; records of 36 bytes (l_read_name 0) frame but are
refused, and both fill two tiles below.
"""
import itertools
import os
import random
import struct
import subprocess

import pytest

from tests import align_oracle
from tests import bam_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
HLEN = len(oracle.header(oracle.TEXT, oracle.REFS))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def TNW():
    import starch_amd
    return starch_amd.bam_constants()


def check(ctx, data, wrap=oracle.bgzf, **kw):
    """Unsorted and sorted output of inflated BAM `data`, given as wrap(data), against the oracle and against sam2bed
    of the SAM text; returns the oracle's unsorted BED."""
    text = oracle.sam_text(data)
    want = align_oracle.sam(text, **kw)
    assert ctx.bam2bed(wrap(data), sort=False, **kw) == want, kw
    assert ctx.align2bed(text, "sam", sort=False, **kw) == want, kw
    assert ctx.bam2bed(wrap(data), **kw) == align_oracle.sort_bed(want), kw
    return want


def check_error(ctx, data, record, text, **kw):
    """The refusal, nothing left behind, and the context still serves a good call."""
    import starch_amd
    for sort, wrap in ((False, oracle.bgzf), (True, bytes)):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.bam2bed(wrap(data), sort=sort, **kw)
        assert e.value.code == -12 and str(e.value).endswith("bam2bed: record %d: %s" % (record, text)), str(e.value)
        with pytest.raises(starch_amd.StarchError) as e:   # no output is left behind
            ctx._output()
        assert e.value.code == -4
    good = oracle.bam(b"", oracle.REFS, [dict(qname=b"r", ref=0, pos=4, cigar=[(3, b"M")])])
    assert ctx.bam2bed(good).startswith(b"chr1\t4\t7\tr\t0\t+\t")


def sized(total, k=0, **kw):
    """A mapped record of exactly `total` bytes (37, or 41 and more): a Z tag pads it."""
    rec = dict(qname=b"", flag=16 * (k & 1), ref=k % 3, pos=10 ** 6 - k, cigar=[], **kw)
    base = len(oracle.pack_record(rec))
    assert total == base or total >= base + 4, total
    if total > base:
        rec["tags"] = rec.get("tags", []) + [(b"PD", "Z", bytes(65 + (j * 7 + k) % 26 for j in range(total - base - 4)))]
    assert len(oracle.pack_record(rec)) == total
    return rec


def short(k):
    return dict(qname=b"s%d" % k, flag=16 * (k & 1), ref=k % 4, pos=5000 - k, mapq=k % 61, cigar=[(5, b"M"), (2, b"N"), (5, b"M")],
                seq=b"ACGTACGTACGT", qual=bytes(range(12)), tags=[(b"NM", "i", k)])


def placed(start, tail):
    """A BAM whose second record begins at byte `start` of the inflated file, followed by the records of tail."""
    return oracle.bam(oracle.TEXT, oracle.REFS, [sized(start - HLEN)] + tail)


# ---- random records over every option combination -------------------------------------------
@pytest.fixture(scope="module")
def random_case():
    data, recs = oracle.random_bam(random.Random(2026), 3000)
    return data, oracle.sam_text(data)


OPTIONS = [dict(zip(("split", "split_deletions", "all_reads", "reduced", "keep_header"), v))
           for v in itertools.product((False, True), repeat=5) if v[0] or not v[1]]


@pytest.mark.parametrize("kw", OPTIONS, ids=lambda kw: "".join(k[0] if v else "-" for k, v in kw.items()))
def test_random_records_unsorted_sorted_and_archive(ctx, random_case, kw):
    data, text = random_case
    z = oracle.bgzf(data)
    want = align_oracle.sam(text, **kw)
    assert ctx.bam2bed(z, sort=False, **kw) == want
    st = ctx.bam_stats()
    dropped = 0 if kw["all_reads"] else text.count(b"\n") - oracle.TEXT.count(b"\n") - align_oracle.sam(text, reduced=True).count(b"\n")
    assert (st["input_bytes"], st["inflated_bytes"], st["references"], st["header_lines"], st["records"], st["unmapped_dropped"],
            st["tiles"], st["wave_records"], st["lines_out"], st["output_bytes"], st["sorted"]) == \
           (len(z), len(data), len(oracle.REFS), oracle.TEXT.count(b"\n"), 3000, dropped, -(-len(data) // 16384), 0,
            want.count(b"\n"), len(want), 0)
    assert ctx.align2bed(text, "sam", sort=False, **kw) == want
    srt = align_oracle.sort_bed(want)
    assert srt != want and ctx.bam2bed(z, **kw) == srt and ctx.bam_stats()["sorted"] == 1
    assert ctx.compress_bam(z, **kw) == ctx.compress(srt)


def test_bam2bed_device_reads_inflated_hbm(ctx, random_case):
    import torch
    data, text = random_case
    dev = torch.frombuffer(bytearray(b"x" + data), dtype=torch.uint8).to("cuda:0")   # (not aligned to 4 bytes)
    torch.cuda.synchronize()
    want = align_oracle.sam(text, split=True)
    assert ctx.bam2bed_device(dev.data_ptr() + 1, len(data), split=True) == len(want) and ctx._output() == align_oracle.sort_bed(want)
    ctx.bam2bed_device(dev.data_ptr() + 1, len(data), keep_header=True, sort=False)
    assert ctx._output() == align_oracle.sam(text, keep_header=True) and ctx.bam_stats()["sorted"] == 0
    assert ctx.bam_stats()["input_bytes"] == ctx.bam_stats()["inflated_bytes"] == len(data)


# ---- the hand-written table -----------------------------------------------------------------
def test_the_hand_written_table(ctx):
    data = oracle.bam(oracle.TEXT, oracle.REFS, [rec for rec, _ in oracle.TABLE])
    for kw in (dict(), dict(all_reads=True, keep_header=True), dict(split=True), dict(split=True, split_deletions=True, reduced=True)):
        want = check(ctx, data, **kw)
    for _, line in oracle.TABLE:
        assert line.split(b"\t", 5)[5] in check(ctx, data, all_reads=True)


# ---- framing edges --------------------------------------------------------------------------
def test_block_size_straddles_a_tile_edge(ctx, TNW):
    T = TNW[0]
    for start in range(T - 4, T + 2):
        data = placed(start, [short(k) for k in range(5)])
        assert oracle.record_offsets(data)[1] == start
        assert check(ctx, data, keep_header=True).count(b"\n") == 6 + oracle.TEXT.count(b"\n")
    data = placed(2 * T - 2, [short(1), sized(T - len(oracle.pack_record(short(1))), 3), sized(37, 4), short(5)])   # and again at 3T - 2
    assert oracle.record_offsets(data)[3] + 2 == 3 * T
    check(ctx, data, split=True)


def test_records_of_a_tile_and_of_three_tiles_and_an_end_at_a_tile_edge(ctx, TNW):
    T = TNW[0]
    for big in (T, 3 * T + 5, T - 1, T + 1):
        data = oracle.bam(oracle.TEXT, oracle.REFS, [short(0), sized(big, 1), short(2), sized(big, 3), sized(big, 4), short(5)])
        assert check(ctx, data).count(b"\n") == 6
        assert ctx.bam_stats()["tiles"] == -(-len(data) // T)
    data = placed(T, [sized(3 * T + 5, 1), short(2)])            # tiles 2 and 3 have no entry
    check(ctx, data)
    data = placed(T + 100, [sized(T - 100, 1)])                   # the last record ends exactly at 2T
    assert len(data) == 2 * T
    assert check(ctx, data).count(b"\n") == 2
    data = placed(T - 100, [sized(100, 1)])                       # ... and at T
    assert len(data) == T
    check(ctx, data)


def test_minimal_records_fill_two_tiles(ctx, TNW):
    T = TNW[0]
    n = 2 * T // 37 + 40
    data = oracle.bam(b"", oracle.REFS, [sized(37, k) for k in range(n)])   # 443 hops in a tile: every doubling round is needed
    assert len(data) > 2 * T + 1000
    assert check(ctx, data, reduced=True).count(b"\n") == n
    check(ctx, data)
    # 36 bytes, l_read_name 0: the chain is followed to the end of the input, and then record 1 is refused for its name
    rec36 = struct.pack("<IiiBBHHHIiii", 32, 0, 5, 0, 0, 4680, 0, 0, 0, -1, -1, 0)
    head = oracle.header(b"", oracle.REFS)
    check_error(ctx, head + rec36 * (2 * T // 36 + 40), 1, oracle.E_NAME)
    good = oracle.pack_record(sized(37, 1))
    check_error(ctx, head + good * 3 + rec36 * 1000 + good, 4, oracle.E_NAME)
    check_error(ctx, head + good * 1000 + struct.pack("<I", 31) + b"\0" * 31, 1001, oracle.E_SHORT)


def test_record_counts_around_the_block_size(ctx, TNW):
    N = TNW[1]
    for n in (N - 1, N, N + 1, 2 * N + 1):
        data = oracle.bam(oracle.TEXT, oracle.REFS, [short(k) for k in range(n)])
        assert check(ctx, data, split=True).count(b"\n") == 2 * n
        assert ctx.bam_stats()["records"] == n
    recs = [short(k) for k in range(2 * N + 1)]
    for at in (0, N - 1, N, 2 * N):
        bad = list(recs)
        bad[at] = dict(short(at), pos=-1)
        check_error(ctx, oracle.bam(oracle.TEXT, oracle.REFS, bad), at + 1, oracle.E_ZERO, split=True)


def test_decoy_chains_inside_tags_are_ignored(ctx, TNW):
    T = TNW[0]
    chain = (struct.pack("<I", 32) + b"\x07" * 32) * 300                       # 300 records' worth of valid-looking block_size chain
    far = (b"\x24\x01\x01\x01" + b"A" * 32) * 100                               # a Z value cannot hold a NUL: these leave any tile
    recs = [short(0), dict(short(1), tags=[(b"DC", "B", ("C", list(chain)))]), short(2), dict(short(3), tags=[(b"DZ", "Z", far)]),
            dict(short(4), tags=[(b"DC", "B", ("C", list(chain[1:])))]), dict(short(5), tags=[(b"DC", "B", ("C", list(chain[2:])))]),
            dict(short(6), tags=[(b"DC", "B", ("C", list(chain[3:] * 2)))]), short(7)]
    data = oracle.bam(oracle.TEXT, oracle.REFS, recs)
    assert len(data) > 2 * T
    assert check(ctx, data).count(b"\n") == 8
    assert ctx.bam_stats()["records"] == 8


# ---- BGZF cut independently of the records ----------------------------------------------------
def test_every_framing_of_the_same_bam_gives_the_same_output(ctx, random_case):
    data, text = random_case
    data = data[:oracle.record_offsets(data)[700]]
    offs = oracle.record_offsets(data)
    want = align_oracle.sort_bed(align_oracle.sam(oracle.sam_text(data), split=True, keep_header=True))
    forms = [oracle.bgzf(data, cuts=offs), oracle.bgzf(data, cuts=[o + 2 for o in offs]), oracle.bgzf(data, cuts=[o + 35 for o in offs]),
             oracle.bgzf(data, block=999), oracle.bgzf(data, level=0), oracle.bgzf(data, eof=False), oracle.gzip_member(data), data]
    for form in forms:
        assert ctx.bam2bed(form, split=True, keep_header=True) == want
        assert ctx.bam_stats()["inflated_bytes"] == len(data)
    import starch_amd
    for junk in (b"", b"BAM", b"BAM\2" + data[4:], b"not a bam file at all", oracle.bgzf(b"SAM\1" + data[4:])):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.bam2bed(junk)
        assert e.value.code == -12


# ---- the wave path ----------------------------------------------------------------------------
def long_read(k, l_seq, **kw):
    rng = random.Random(l_seq + k)
    rec = dict(short(k), qname=b"long%d" % k, seq=bytes(rng.choice(oracle.BASES) for _ in range(l_seq)),
               qual=bytes(rng.randint(0, 93) for _ in range(l_seq)))
    rec.update(kw)
    return rec


def test_l_seq_around_the_wave_threshold(ctx, TNW):
    W = TNW[2]
    for l_seq in (W - 1, W, W + 1, 70000):
        recs = [short(k) for k in range(70)]
        recs[0] = recs[33] = long_read(1, l_seq)
        recs[69] = long_read(2, l_seq, qual=None)
        data = oracle.bam(oracle.TEXT, oracle.REFS, recs)
        for kw in (dict(), dict(split=True), dict(reduced=True)):
            check(ctx, data, **kw)
        assert ctx.bam_stats()["wave_records"] == (3 if l_seq >= W else 0)


EDGE_FLOATS = [0, 0x80000000, 1, 2, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001,
               0x3f800000, 0x3dcccccd, 0x38d1b717, 0x38d1b716, 0x38d1b718, 0x49742400, 0x497423f8, 0x497423f0, 0x47f12040, 0x47c34f80,
               0x47c35000, 0x3a83126f, 0x4b7fffff, 0x4b800000, 0x5f000000, 0x00000003, 0x80000001, 0x33d6bf95]


def test_float_arrays_of_65536_values_are_the_percent_g_test(ctx, TNW):
    W = TNW[2]
    rng = random.Random(715)
    recs = []
    for k in range(16):                                           # 2^20 bit patterns in all
        bits = (EDGE_FLOATS if k == 0 else []) + [rng.getrandbits(32) for _ in range(65536)]
        if k == 1:                                                # every exponent with a mantissa of 0, all ones and one half
            bits[:768] = [e << 23 | m for e in range(256) for m in (0, 0x7fffff, 0x400000)]
        recs.append(dict(short(k), tags=[(b"XF", "B", ("f", bits[:65536])), (b"Xf", "f", bits[0])]))
    data = oracle.bam(b"", oracle.REFS, recs)
    want = check(ctx, data)
    assert ctx.bam_stats()["wave_records"] == 16 and 65536 >= W
    assert b"XF:B:f,0,-0,1.4013e-45,2.8026e-45," in want and b",inf,-inf,nan,nan,nan,1,0.1,0.0001," in want


def test_a_byte_array_of_100000_and_a_long_record_between_short_ones(ctx, TNW):
    W = TNW[2]
    rng = random.Random(5)
    recs = [short(k) for k in range(64)]
    recs[31] = dict(long_read(31, 3 * W + 7), tags=[(b"Bc", "B", ("c", [rng.randint(-128, 127) for _ in range(100000)])), (b"ZZ", "Z", b"after")])
    recs[40] = dict(short(40), tags=[(b"BS", "B", ("S", [rng.randint(0, 65535) for _ in range(W)])), (b"Bi", "B", ("i", [-5] * (W - 1)))])
    data = oracle.bam(oracle.TEXT, oracle.REFS, recs)
    for kw in (dict(), dict(split=True, keep_header=True)):
        assert check(ctx, data, **kw).count(b"\tZZ:Z:after\n") == (2 if kw else 1)
    assert ctx.bam_stats()["wave_records"] == 2
    # the long-CIGAR convention with an array above the threshold
    n_ops = 2 * W + 1
    ops = [(3 << 4) | (0, 3)[j & 1] for j in range(n_ops)]
    recs[10] = dict(short(10), cigar=[(12, b"S"), (99, b"N")], tags=[(b"CG", "B", ("I", ops)), (b"XY", "A", b"q")])
    data = oracle.bam(oracle.TEXT, oracle.REFS, recs)
    assert check(ctx, data, split=True).count(b"\ts10\t") == W + 1
    check(ctx, data)


# ---- bad inputs -------------------------------------------------------------------------------
def test_bad_records_are_refused_with_their_number(ctx, TNW):
    W = TNW[2]
    recs = [oracle.pack_record(short(k)) for k in range(300)]

    def with_bad(at, raw):
        return oracle.bam(oracle.TEXT, oracle.REFS, recs[:at] + [raw] + recs[at + 1:])

    def patched(rec, at, byte):
        raw = bytearray(oracle.pack_record(rec))
        raw[at] = byte
        return bytes(raw)

    name_end = 36 + len(b"s7")
    cases = [(struct.pack("<I", 31) + b"\0" * 31, oracle.E_SHORT),
             (patched(short(7), name_end, 65), oracle.E_NAME),
             (oracle.pack_record(dict(short(7), ref=len(oracle.REFS))), oracle.E_REF),
             (oracle.pack_record(dict(short(7), next_ref=-2)), oracle.E_REF),
             (patched(short(7), name_end + 1 + 4, (2 << 4) | 9), oracle.E_CIGAR),
             (oracle.pack_record(dict(short(7), raw_tags=b"XXq\0")), oracle.E_TAGTYPE),
             (oracle.pack_record(dict(short(7), raw_tags=b"XBBq\0\0\0\0")), oracle.E_TAGTYPE),
             (oracle.pack_record(dict(short(7), raw_tags=b"XBBc" + struct.pack("<I", 1000) + b"abc")), oracle.E_TAGS),
             (oracle.pack_record(dict(short(7), raw_tags=b"XYi\1\0\0")), oracle.E_TAGS),
             (oracle.pack_record(dict(short(7), raw_tags=b"XZZno end")), oracle.E_TAGS),
             (oracle.pack_record(dict(short(7), raw_tags=b"XY")), oracle.E_TAGS),
             (patched(short(7), 12, 200), oracle.E_COUNTS),
             (oracle.pack_record(dict(short(7), ref=-1)), oracle.E_RNAME),
             (oracle.pack_record(dict(long_read(7, W + 5), raw_tags=b"XYi\1\0\0")), oracle.E_TAGS),      # in the wave path
             (oracle.pack_record(dict(short(7), tags=[(b"XB", "B", ("f", [1.0] * (W + 1)))], raw_tags=b"QQ?\0")), oracle.E_TAGTYPE)]
    for raw, text in cases:
        check_error(ctx, with_bad(7, raw), 8, text)
    check_error(ctx, with_bad(299, cases[5][0]), 300, oracle.E_TAGTYPE)
    good = oracle.bam(oracle.TEXT, oracle.REFS, recs)
    check_error(ctx, good[:-1], 300, oracle.E_PAST)                               # the chain overruns the end by one byte
    check_error(ctx, good + b"\x20", 301, oracle.E_PAST)                          # a block_size cut off
    check_error(ctx, good + struct.pack("<I", 32) + b"\0" * 31, 301, oracle.E_PAST)
    two = oracle.bam(oracle.TEXT, oracle.REFS, recs[:100] + [cases[4][0]] + recs[101:280] + [cases[0][0]] + recs[281:])
    check_error(ctx, two, 101, oracle.E_CIGAR)                                    # two bad records: the lower one is named
    two = oracle.bam(oracle.TEXT, oracle.REFS, recs[:100] + [cases[0][0]] + recs[101:280] + [cases[4][0]] + recs[281:])
    check_error(ctx, two, 101, oracle.E_SHORT)


# ---- headers ----------------------------------------------------------------------------------
def test_headers(ctx, TNW):
    import starch_amd
    T = TNW[0]
    unmapped = [dict(qname=b"u%d" % k, flag=4, seq=b"ACG", qual=bytes([3, 4, 5])) for k in range(5)]
    mapped = [short(k) for k in range(5)]
    long_text = b"".join(b"@SQ\tSN:contig%d\tLN:%d\n" % (k, 1000 + k) for k in range(900)) + b"@CO\t" + b"x" * 5000 + b"\n"
    many_refs = tuple((b"contig%d" % k, 1000 + k) for k in range(900))
    assert len(long_text) > T and len(oracle.header(long_text, many_refs)) > 2 * T
    cases = [(b"", (), unmapped), (b"", oracle.REFS, mapped), (oracle.TEXT + b"\0" * 7, oracle.REFS, mapped),
             (b"@CO\tno newline at the end", oracle.REFS, mapped), (b"\n\n@CO\tx\n\n", oracle.REFS, mapped),
             (long_text, many_refs, [dict(short(k), ref=899 - k, next_ref=k) for k in range(5)]),
             (oracle.TEXT, oracle.REFS, []), (b"", (), []), (long_text, many_refs, [])]
    for text, refs, recs in cases:
        data = oracle.bam(text, refs, recs)
        for kw in (dict(all_reads=True), dict(all_reads=True, keep_header=True)):
            plain = text.rstrip(b"\0")
            lines = plain.count(b"\n") + (1 if plain and not plain.endswith(b"\n") else 0)
            assert check(ctx, data, **kw).count(b"\n") == len(recs) + (lines if "keep_header" in kw else 0)
            assert ctx.bam_stats()["header_lines"] == lines
        st = ctx.bam_stats()
        assert (st["references"], st["records"]) == (len(refs), len(recs))
    head = oracle.header(oracle.TEXT, oracle.REFS)
    for bad in (head[:-1], head[:20], head[:-5] + b"X" + head[-4:], oracle.header(b"", ((b"", 5),))[:-9] + struct.pack("<II", 0, 5)):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.bam2bed(bad)
        assert e.value.code == -12 and "bam2bed: " in str(e.value), str(e.value)


# ---- the command ------------------------------------------------------------------------------
def _cli(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_command_against_the_library(ctx, tmp_path, random_case):
    cmd = os.path.join(BUILD, "bam2bed")
    data, _ = random_case
    data = data[:oracle.record_offsets(data)[300]]
    z = oracle.bgzf(data)
    path = tmp_path / "a.bam"
    path.write_bytes(z)
    want = align_oracle.sort_bed(oracle.expected(data))
    r = _cli([cmd, str(path)])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want
    with open(path, "rb") as f:
        r = _cli([cmd, "--do-not-sort", "--keep-header", "--split-with-deletions", "--all-reads", "-"], stdin=f)
    assert (r.returncode, r.stderr) == (0, b"")
    assert r.stdout == oracle.expected(data, keep_header=True, split=True, split_deletions=True, all_reads=True)
    r = _cli([cmd, "--output=starch", str(path)])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == ctx.compress_bam(z)
    (tmp_path / "a.starch").write_bytes(r.stdout)
    r = _cli([os.path.join(BUILD, "unstarch"), str(tmp_path / "a.starch")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want
    (tmp_path / "bad.bam").write_bytes(oracle.bgzf(data + struct.pack("<I", 31) + b"\0" * 31))
    r = _cli([cmd, str(tmp_path / "bad.bam")])
    assert r.returncode == 22 and r.stdout == b""
    assert b"bam2bed: record 301: " + oracle.E_SHORT.encode() in r.stderr
