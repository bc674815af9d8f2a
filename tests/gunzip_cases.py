"""Streams for the inflater's tests, made with tests/deflate_writer.py (TEST
INFRASTRUCTURE ONLY): valid ones that zlib's compressor never emits, and one
invalid one per rule the inflater enforces.  test_deflate_writer_cpu.py puts
every one of them to zlib (and the valid ones to tests/deflate_trace.py);
test_gpu_gunzip.py puts them to the GPU.

The ring and flush sizes the valid cases aim at are read from the library
(starch_amd.gunzip_constants()) by the caller and passed in."""
import random
import zlib

from tests import deflate_writer as dw


def _noise(n, seed):
    r = random.Random(seed)
    return bytes(r.getrandbits(8) for _ in range(n))


def _member(build, **kw):
    """build(bw) writes the blocks and returns the text they stand for."""
    bw = dw.BitWriter()
    text = build(bw)
    return dw.gzip_member(bw.getvalue(), text, **kw), text


def _stored_run(bw, data, final=False):
    for i in range(0, len(data), 65535):
        dw.stored_block(bw, data[i:i + 65535], final and i + 65535 >= len(data))


def valid_cases(window=34816, flush=1024):
    """[(name, gz bytes, text)]"""
    cases = []

    def add(name, build, **kw):
        gz, text = _member(build, **kw)
        cases.append((name, gz, text))

    # distance 32768 and length 258 where the ring wraps: the match starts 100 bytes before the ring's end
    def wrap(bw):
        pre = _noise(window - 100, 1)
        _stored_run(bw, pre)
        toks = [(258, 32768), (258, 32768), 65, (258, 32768)]
        dw.fixed_block(bw, toks, True)
        from tests.deflate_trace import replay
        return pre + replay(toks, pre)
    add("dist32768_len258_at_wrap", wrap)

    # matches that end exactly where a flush is due, several flushes in a row
    def at_flush(bw):
        toks = []
        for k in range(6):
            toks += [97 + (i + k) % 23 for i in range(flush - 258)] + [(258, 5 + k)]
        dw.dynamic_block(bw, toks, True)
        from tests.deflate_trace import replay
        return replay(toks)
    add("match_ends_at_flush_boundary", at_flush)

    # a stair of code lengths 1, 2, ..., 14, 15, 15: literal codes of 11 to 15 bits take the canonical path
    def deep(bw):
        syms = [97 + i for i in range(15)] + [256]
        lens = [0] * 286
        for i, s in enumerate(syms):
            lens[s] = min(i + 1, 15)
        text = bytes(syms[(i * 7) % 15] for i in range(600)) + bytes(syms[:15]) * 3
        dw.dynamic_block(bw, list(text), True, lit_lens=lens, dist_lens=[0])
        return text
    add("15_bit_literal_codes", deep)

    # HLIT = 286 and HDIST = 30: every length of both alphabets is sent
    def full(bw):
        text = b"chr1\t100\t200\n" * 40
        toks = dw.lz_tokens(text)
        lf, df = dw.token_freqs(toks)
        lf[285] += 1
        df[29] += 1
        dw.dynamic_block(bw, toks, True, lit_lens=dw.huff_lengths(lf[:286], 15), dist_lens=dw.huff_lengths(df[:30], 15))
        return text
    add("hlit286_hdist30", full)

    # a symbol-16 repeat that runs from the last literal/length length into the distance lengths
    def crossing(bw):
        lit = [0] * 259
        lit[97], lit[98], lit[256], lit[257], lit[258] = 1, 3, 3, 3, 3
        dist = [3] * 8
        syms = dw.rle_cl_syms(lit + dist)
        at, spans = 0, False                 # a repeat that starts among the literal/length lengths and ends after them
        for s, x in syms:
            n = 1 if s < 16 else x + (3 if s < 18 else 11)
            spans = spans or (s == 16 and at < len(lit) < at + n)
            at += n
        assert spans
        toks = [97, 98, 97, 97, (4, 1), (3, 2), 98, (4, 4), (3, 3), (4, 8), (3, 7)]
        dw.dynamic_block(bw, toks, True, lit_lens=lit, dist_lens=dist, cl_syms=syms)
        from tests.deflate_trace import replay
        return replay(toks)
    add("repeat_crosses_into_distance_lengths", crossing)

    # one distance code of one bit: the incomplete code zlib lets through
    def one_dist(bw):
        toks = [120, (258, 1), 121, (17, 1)]
        dw.dynamic_block(bw, toks, True, dist_lens=[1])
        from tests.deflate_trace import replay
        return replay(toks)
    add("single_distance_code", one_dist)

    # no distance code at all: HDIST = 1 and that one length is zero
    def no_dist(bw):
        text = b"all literals, no matches\n" * 3
        dw.dynamic_block(bw, list(text), True, dist_lens=[0], hdist=1)
        return text
    add("all_literal_zero_distance_length", no_dist)

    def stored0(bw):
        dw.stored_block(bw, b"", False)
        dw.stored_block(bw, b"abc", False)
        dw.stored_block(bw, b"", True)
        return b"abc"
    add("stored_len_0", stored0)

    def stored_max(bw):
        data = _noise(65535, 2)
        dw.stored_block(bw, data, True)
        return data
    add("stored_len_65535", stored_max)

    # 3 header bits, six 9-bit literals, one 8-bit literal and the 7-bit end code: 72 bits, no padding
    def last_bit(bw):
        text = bytes([200, 201, 202, 203, 204, 205, 65])
        dw.fixed_block(bw, list(text), True)
        assert bw.bits % 8 == 0
        return text
    add("final_block_ends_on_last_bit", last_bit)

    return cases


def header_cases():
    """Generic members with every optional header field: [(name, gz, text)]"""
    text = b"chr7\t5\t9\tname\n" * 20
    raw = dw.raw_deflate(text)
    return [
        ("fname", dw.gzip_member(raw, text, name=b"x.bed"), text),
        ("fextra_not_bc", dw.gzip_member(raw, text, extra=b"AB\x03\x00xyz"), text),
        ("fcomment", dw.gzip_member(raw, text, comment=b"a comment that is longer than sixty-four bytes " * 3), text),
        ("fhcrc", dw.gzip_member(raw, text, hcrc=True), text),
        ("all_fields", dw.gzip_member(raw, text, extra=b"AB\x01\x00q", name=b"n", comment=b"c", hcrc=True, mtime=12345), text),
    ]


# the reason the library gives for each invalid case (its text after "member K at byte N: ")
REASONS = {
    "lit_oversubscribed": "literal/length code lengths over-subscribe the code",
    "lit_incomplete": "incomplete literal/length code",
    "dist_oversubscribed": "distance code lengths over-subscribe the code",
    "dist_incomplete": "incomplete distance code",
    "code_length_code_oversubscribed": "the code-length code is over-subscribed or incomplete",
    "repeat_with_nothing_before": "code-length repeat with nothing before it",
    "repeat_past_hlit_hdist": "code-length repeat runs past HLIT + HDIST",
    "hlit_above_286": "HLIT above 286",
    "hdist_above_30": "HDIST above 30",
    "no_end_of_block_code": "no end-of-block code",
    "literal_symbol_286": "literal/length symbol 286 or 287",
    "literal_symbol_287": "literal/length symbol 286 or 287",
    "distance_symbol_30": "distance symbol 30 or 31",
    "distance_symbol_31": "distance symbol 30 or 31",
    "btype_3": "block type 3",
    "stored_len_nlen_disagree": "stored block with LEN != ~NLEN",
    "input_ends_inside_block": "the input ends inside a block",
    "wrong_crc": "CRC-32 mismatch",
    "wrong_isize": "ISIZE does not match the bytes produced",
    "truncated_member": "the input ends inside a block",
    "distance_one_past_produced": "match distance beyond the bytes produced",
    "reserved_flg_bits": "reserved FLG bits are set",
    "bytes_after_last_member": "bytes after the last member do not begin a member",
    "bgzf_output_exceeds_isize": "more output than the member's size allows",
    "bgzf_match_into_previous_member": "match distance beyond the bytes produced",
    "bgzf_wrong_crc": "CRC-32 mismatch",
    "bgzf_corrupt_deflate": "block type 3",
}


def invalid_cases():
    """[(name, gz bytes, index of the member that is bad, the library's reason)]; zlib refuses every one."""
    cases = []
    good_text = b"chr1\t1\t2\n" * 30
    good = dw.gzip_member(dw.raw_deflate(good_text), good_text)

    def add(name, build, bad=0, **kw):
        cases.append((name, _member(build, **kw)[0], bad))

    def lens3(a, b, eob):
        lit = [0] * 257
        lit[97], lit[98], lit[256] = a, b, eob
        return lit

    add("lit_oversubscribed", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 1, 1), dist_lens=[0]) or b"ab")
    add("lit_incomplete", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(2, 2, 2), dist_lens=[0]) or b"ab")
    add("dist_oversubscribed", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[1, 1, 1]) or b"ab")
    add("dist_incomplete", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[2, 2]) or b"ab")
    cl_over = [0] * 19
    cl_over[0] = cl_over[1] = cl_over[2] = 1
    add("code_length_code_oversubscribed",
        lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[0], cl_lens=cl_over, rle=False) or b"ab")
    cl16 = [0] * 19
    cl16[16], cl16[0], cl16[1], cl16[2] = 2, 2, 2, 2
    add("repeat_with_nothing_before",
        lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[0], cl_lens=cl16,
                                    cl_syms=[(16, 0)] + [(0, 0)] * 255) or b"ab")
    cl18 = [0] * 19
    cl18[18], cl18[0], cl18[1], cl18[2] = 2, 2, 2, 2
    add("repeat_past_hlit_hdist",
        lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[0], cl_lens=cl18,
                                    cl_syms=[(18, 127), (18, 127)]) or b"ab")
    add("hlit_above_286", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[0], hlit=287) or b"ab")
    add("hdist_above_30", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 2, 2), dist_lens=[0], hdist=31) or b"ab")
    add("no_end_of_block_code", lambda bw: dw.dynamic_block(bw, [97, 98], True, lit_lens=lens3(1, 1, 0), dist_lens=[0], eob=False) or b"ab")
    add("literal_symbol_286", lambda bw: dw.fixed_block(bw, [97, ("sym", 286)], True) or b"a")
    add("literal_symbol_287", lambda bw: dw.fixed_block(bw, [97, ("sym", 287)], True) or b"a")
    add("distance_symbol_30", lambda bw: dw.fixed_block(bw, [97, 98, 99, ("dsym", 3, 30, 0)], True) or b"abc")
    add("distance_symbol_31", lambda bw: dw.fixed_block(bw, [97, 98, 99, ("dsym", 3, 31, 0)], True) or b"abc")

    def btype3(bw):
        bw.put(1, 1)
        bw.put(3, 2)
        bw.put(0, 29)
        return b""
    add("btype_3", btype3)
    add("stored_len_nlen_disagree", lambda bw: dw.stored_block(bw, b"abcd", True, nlen=0x1234) or b"abcd")
    raw = dw.raw_deflate(_noise(3000, 3), 6)
    cases.append(("input_ends_inside_block", dw.gzip_member(raw[:len(raw) // 2], _noise(3000, 3)), 0))
    cases.append(("wrong_crc", dw.gzip_member(dw.raw_deflate(good_text), good_text, crc=zlib.crc32(good_text) ^ 1), 0))
    cases.append(("wrong_isize", dw.gzip_member(dw.raw_deflate(good_text), good_text, isize=len(good_text) + 1), 0))
    cases.append(("truncated_member", good + good[:len(good) - 11], 1))
    add("distance_one_past_produced", lambda bw: dw.fixed_block(bw, [97, (3, 2)], True) or b"a")
    cases.append(("reserved_flg_bits", dw.gzip_member(dw.raw_deflate(good_text), good_text, flg=0x20), 0))
    cases.append(("bytes_after_last_member", good + b"not a member, just bytes", 1))

    # BGZF: the first member is good in each
    b0 = dw.bgzf_member(dw.raw_deflate(good_text), good_text)
    cases.append(("bgzf_output_exceeds_isize", b0 + dw.bgzf_member(dw.raw_deflate(good_text), good_text, isize=len(good_text) - 1)
                  + dw.bgzf_eof(), 1))
    bw = dw.BitWriter()
    dw.fixed_block(bw, [(3, 1), 97], True)
    cases.append(("bgzf_match_into_previous_member", b0 + dw.bgzf_member(bw.getvalue(), b"\n\n\na") + dw.bgzf_eof(), 1))
    cases.append(("bgzf_wrong_crc", b0 + dw.bgzf_member(dw.raw_deflate(good_text), good_text, crc=1) + dw.bgzf_eof(), 1))
    cases.append(("bgzf_corrupt_deflate", b0 + dw.bgzf_member(b"\x07" + dw.raw_deflate(good_text)[1:], good_text) + dw.bgzf_eof(), 1))
    assert [c[0] for c in cases] == list(REASONS)
    return [c + (REASONS[c[0]],) for c in cases]
