"""GPU: the inflater (Starch.gunzip, gz_inflate.hip).

The referee for every case is CPython's zlib (tests/deflate_writer.referee:
zlib.decompressobj(wbits=31), member after member until the input is
exhausted), asked before the case goes to the GPU: the GPU returns the same
bytes, or refuses with -12 exactly when zlib raises.  One exception: bytes
after the last member that do not begin a member are a data error here."""
import gzip
import random
import zlib

import pytest

from tests import corpus
from tests import deflate_writer as dw
from tests import gunzip_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def texts():
    r = random.Random(5)
    bed = corpus.multi_chrom_bed(4, 2500, seed=9, kind="bed6")
    while len(bed) < 200 << 10:
        bed += bed
    return {"empty": b"", "one_byte": b"x", "64k_of_one_byte": b"A" * 65536, "bed_200k": bed[:200 << 10],
            "random_200k": bytes(r.getrandbits(8) for _ in range(200 << 10))}


def check(ctx, gz, want=None):
    """gz through the referee, then the GPU; returns the bytes"""
    ref = dw.referee(gz)
    if want is not None:
        assert ref == want
    got = ctx.gunzip(gz)
    assert got == ref
    s = ctx.gunzip_stats()
    assert s["bytes_in"] == len(gz) and s["bytes_out"] == len(ref)
    return got


def member_of(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    return dw.gzip_member(dw.raw_deflate(text, level, strategy), text)


# ---- zlib-made streams ----------------------------------------------------------------
STRATEGIES = (("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("dynamic", 9, zlib.Z_DEFAULT_STRATEGY),
              ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE))


@pytest.mark.parametrize("how,level,strategy", STRATEGIES, ids=[s[0] for s in STRATEGIES])
def test_zlib_streams(ctx, texts, how, level, strategy):
    for name, text in texts.items():
        check(ctx, member_of(text, level, strategy), text)
        s = ctx.gunzip_stats()
        assert s["members"] == 1 and not s["is_bgzf"], name
        kinds = (s["stored_blocks"], s["fixed_blocks"], s["dynamic_blocks"])
        assert sum(kinds) >= 1
        if how == "stored":
            assert kinds[1:] == (0, 0) or not text
        if how == "fixed":
            assert kinds[2] == 0


def test_rle_runs_distance_1_length_258(ctx):
    text = b"".join(bytes([65 + i % 7]) * (258 * 3 + i) for i in range(40))
    check(ctx, member_of(text, 6, zlib.Z_RLE), text)


def test_full_flush_every_1000_bytes(ctx, texts):
    text = texts["bed_200k"][:100_000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(c.compress(text[i:i + 1000]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(text), 1000)) + c.flush()
    check(ctx, dw.gzip_member(raw, text), text)
    s = ctx.gunzip_stats()
    assert s["stored_blocks"] >= 100          # the empty stored block of every flush


# ---- BGZF -----------------------------------------------------------------------------
def test_bgzf_eof_block_alone(ctx):
    assert check(ctx, dw.bgzf_eof()) == b""
    s = ctx.gunzip_stats()
    assert s["members"] == 1 and s["is_bgzf"] == 1


def test_bgzf_one_byte_members(ctx):
    text = b"chr1\t1\t2\n" * 7
    check(ctx, dw.bgzf_file(text, block=1), text)
    assert ctx.gunzip_stats()["members"] == len(text) + 1


def test_bgzf_65280_byte_members(ctx, texts):
    text = texts["bed_200k"]
    check(ctx, dw.bgzf_file(text, block=65280), text)
    s = ctx.gunzip_stats()
    assert s["members"] == 5 and s["is_bgzf"] == 1 and s["ms_size"] == 0


def test_bgzf_member_of_exactly_65536_bytes(ctx, texts):
    text = texts["bed_200k"][:65536]
    check(ctx, dw.bgzf_file(text, block=65536), text)
    noise = texts["random_200k"][:40000]          # a member of stored blocks
    check(ctx, dw.bgzf_member(dw.raw_deflate(noise, 0), noise) + dw.bgzf_eof(), noise)


def test_bgzf_300_members_of_mixed_sizes(ctx, texts):
    r = random.Random(11)
    bed, noise = texts["bed_200k"], texts["random_200k"]
    z, text = bytearray(), bytearray()
    for k in range(300):
        n = r.choice((0, 1, 15, 16, 17, 100, 1023, 1024, 1025, 4096, 5000, 20000))
        src = noise if k % 5 == 4 else bed
        at = r.randrange(0, len(src) - n)
        piece = src[at:at + n]
        z += dw.bgzf_member(dw.raw_deflate(piece, r.choice((0, 1, 6, 9)), r.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED))), piece)
        text += piece
    z += dw.bgzf_eof()
    check(ctx, bytes(z), bytes(text))
    assert ctx.gunzip_stats()["members"] == 301


def test_bgzf_more_members_than_the_grid(ctx):
    # 3000 members: every wave decodes several, one after the other, fixed and dynamic blocks mixed
    r = random.Random(12)
    z, text = bytearray(), bytearray()
    for k in range(3000):
        piece = b"".join(b"chr%d\t%d\t%d\n" % (k % 5, k + i, k + i + r.randrange(1, 90)) for i in range(r.choice((1, 1, 2, 300))))
        z += dw.bgzf_member(dw.raw_deflate(piece, 6), piece)
        text += piece
    check(ctx, bytes(z), bytes(text))
    s = ctx.gunzip_stats()
    assert s["members"] == 3000 and s["fixed_blocks"] > 100 and s["dynamic_blocks"] > 100


def test_gunzip_device_and_plan_agree(ctx, texts):
    import starch_amd
    text = texts["bed_200k"][:70000]
    z = dw.bgzf_file(text, block=30000)
    is_bgzf, members = starch_amd.gunzip_plan(z)
    assert is_bgzf and [m["isize"] for m in members] == [30000, 30000, 10000, 0]
    assert ctx.gunzip(z) == text
    # the same file from HBM
    n = ctx.gunzip_device(ctx_ptr_of(ctx, z), len(z))
    assert n == len(text) and ctx._output() == text


def ctx_ptr_of(ctx, data):
    """data in HBM: a torch tensor kept alive on the context object"""
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    ctx._keep = t
    return t.data_ptr()


# ---- generic gzip ---------------------------------------------------------------------
def test_two_members_concatenated(ctx, texts):
    a, b = texts["bed_200k"][:5000], texts["random_200k"][:3000]
    check(ctx, gzip.compress(a) + gzip.compress(b, 1), a + b)
    s = ctx.gunzip_stats()
    assert s["members"] == 2 and not s["is_bgzf"]
    # a BGZF member and a plain one: generic as a whole
    check(ctx, dw.bgzf_file(a) + gzip.compress(b), a + b)
    assert ctx.gunzip_stats()["members"] == 3


def test_small_members_of_every_block_type_in_a_chain(ctx):
    # one wave sizes the whole chain: its tables and bit reader start afresh with every member
    text = b"chr7\t5\t9\tname\n" * 20
    kinds = {"fixed": dw.gzip_member(dw.raw_deflate(text), text),
             "dynamic": gzip.compress(text * 50),
             "stored": dw.gzip_member(dw.raw_deflate(text, 0), text),
             "empty": dw.gzip_member(b"\x03\x00", b"")}
    assert all(dw.referee(m) is not None for m in kinds.values())
    for a in kinds:
        for b in kinds:
            check(ctx, kinds[a] + kinds[b] + kinds[a])
    check(ctx, b"".join(kinds.values()) * 5)


@pytest.mark.parametrize("name,gz,text", gunzip_cases.header_cases(), ids=[c[0] for c in gunzip_cases.header_cases()])
def test_header_fields(ctx, name, gz, text):
    check(ctx, gz, text)
    check(ctx, gz + gz, text + text)


def test_one_member_of_1_mib(ctx, texts):
    # crosses the LDS ring many times; matches reach back across flushes
    bed = texts["bed_200k"]
    text = (bed + texts["random_200k"][:30000]) * 5
    text = text[:1 << 20]
    check(ctx, member_of(text, 9), text)


# ---- streams zlib never emits ---------------------------------------------------------
def _writer_cases():
    import starch_amd
    c = starch_amd.gunzip_constants()
    return gunzip_cases.valid_cases(c["window_bytes"], 1024)


@pytest.mark.parametrize("k", range(10))
def test_writer_made_streams(ctx, k):
    name, gz, text = _writer_cases()[k]
    check(ctx, gz, text)
    # the same deflate data as a BGZF member, where it fits one
    if len(text) <= 65536 and len(gz) < 65000:
        z = dw.bgzf_member(gz[10:-8], text) + dw.bgzf_eof()
        check(ctx, z, text)
        assert ctx.gunzip_stats()["is_bgzf"] == 1, name


def test_writer_case_count():
    assert len(gunzip_cases.valid_cases()) == 10


# ---- own encoder ----------------------------------------------------------------------
def test_members_of_a_gzip_method_archive(ctx):
    import starch_amd
    enc = starch_amd.Starch(0)
    enc.set_compression_method(starch_amd.K_GZIP)
    try:
        for data in (corpus.cfg1_bed(10000), corpus.multi_chrom_bed(5, 3000, seed=4, kind="bed6"),
                     corpus.parseable_fuzz_bed(7, 4000), b"chr1\t10\t20\n"):
            _, members = starch_amd.parse_archive(enc.compress(data))
            for m in members:
                assert ctx.gunzip(m) == gzip.decompress(m)
            assert ctx.gunzip(b"".join(members)) == b"".join(gzip.decompress(m) for m in members)
    finally:
        enc.close()


# ---- refusals -------------------------------------------------------------------------
INVALID = gunzip_cases.invalid_cases()


@pytest.mark.parametrize("name,gz,bad,reason", INVALID, ids=[c[0] for c in INVALID])
def test_refusals(ctx, name, gz, bad, reason):
    import starch_amd
    if name != "bytes_after_last_member":          # the stated exception needs no referee
        with pytest.raises(zlib.error):
            dw.referee(gz)
    good = gzip.compress(b"chr1\t1\t2\n" * 100)
    assert ctx.gunzip(good) == b"chr1\t1\t2\n" * 100
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.gunzip(gz)
    assert e.value.code == -12 and ("gunzip: member %d at byte " % bad) in str(e.value), str(e.value)
    assert str(e.value).endswith(": " + reason), str(e.value)
    with pytest.raises(starch_amd.StarchError) as e2:       # nothing is published from a failed call
        ctx._output()
    assert e2.value.code == -4
    assert ctx.gunzip(good) == b"chr1\t1\t2\n" * 100


def test_refusals_without_a_member(ctx):
    import starch_amd
    for gz in (b"", b"\x1f\x8b\x08", b"plain text, not gzip at all, and long enough\n"):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.gunzip(gz)
        assert e.value.code == -12
