"""The test-side deflate reader (tests/deflate_trace.py) against zlib, the
parse model (tests/gz_model.py) against a brute-force search and against
zlib's Z_FIXED streams, and the teeth of gz_model.check_member: zlib's own
streams, framed as members, are refused for the reason each one breaks."""
import random
import zlib

import pytest

from tests import corpus, gz_model, oracle_lib
from tests.deflate_trace import DeflateError, inflate, read_member, replay, wrap_member
from tests.gz_model import MIN_MATCH, SUB


def _texts():
    r = random.Random(11)
    yield "empty", b""
    yield "one", b"a"
    yield "bed", corpus.multi_chrom_bed(2, 400, seed=5, kind="bed6")
    yield "fuzz", corpus.parseable_fuzz_bed(3, 300)
    yield "random", bytes(r.randrange(256) for _ in range(20000))
    yield "runs", b"".join(bytes([r.randrange(4)]) * r.choice([1, 2, 3, 4, 300, 700]) for _ in range(60))
    yield "two_symbols", bytes(r.choice(b"ab") for _ in range(5000))


TEXTS = list(_texts())
MODES = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
         ("fixed", 9, zlib.Z_FIXED), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]


def _raw(text, level, strategy, block=0):
    """zlib's raw deflate of text; with `block`, one deflate block per `block` bytes (Z_BLOCK keeps the
    history, so matches may reach back over the cut)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not block:
        return c.compress(text) + c.flush()
    out = b""
    for i in range(0, len(text), block):
        out += c.compress(text[i:i + block])
        if i + block < len(text):
            out += c.flush(zlib.Z_BLOCK)
    return out + c.flush()


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name,text", TEXTS, ids=[t[0] for t in TEXTS])
def test_trace_matches_zlib(name, text, mode):
    raw = _raw(text, mode[1], mode[2])
    blocks, end = inflate(raw)
    assert (end + 7) // 8 == len(raw)
    assert b"".join(b.out for b in blocks) == zlib.decompress(raw, -15) == text
    assert [b.bfinal for b in blocks] == [0] * (len(blocks) - 1) + [1]
    hist = b""
    pos = 0
    for b in blocks:
        assert b.bit_off == pos
        pos = b.bit_off + b.bit_len
        assert replay(b.tokens, hist) == b.out
        hist += b.out
        if b.btype == 2:
            assert len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist and 4 <= b.hclen <= 19
    assert pos == end
    if mode[0] == "l0":
        assert all(b.btype == 0 for b in blocks)
    if mode[0] == "fixed":
        assert all(b.btype == 1 or (b.btype == 0 and name == "random") for b in blocks)   # (stored when shorter)
    if mode[0] == "huffman":
        assert all(not isinstance(t, tuple) for b in blocks for t in b.tokens)
    if mode[0] == "rle":
        assert all(t[1] == 1 for b in blocks for t in b.tokens if isinstance(t, tuple))
    assert read_member(wrap_member(raw, text))[1] == text


def _zlib_refuses(raw):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(raw)
    except zlib.error:
        return True
    return not d.eof


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_trace_refuses_what_zlib_refuses(mode):
    text = TEXTS[2][1][:6000]
    raw = _raw(text, mode[1], mode[2])
    r = random.Random(7)
    refused = 0
    cuts = [len(raw) - 1, len(raw) // 2, 1, 0]
    for n in cuts:
        assert _zlib_refuses(raw[:n])
        with pytest.raises(DeflateError):
            inflate(raw[:n])
    for _ in range(150):
        bad = bytearray(raw)
        bad[r.randrange(len(bad))] ^= 1 << r.randrange(8)
        bad = bytes(bad)
        try:
            blocks, end = inflate(bad)
            ok = True
        except DeflateError:
            ok = False
        # whatever zlib refuses the reader refuses, and the other way round
        assert ok == (not _zlib_refuses(bad))
        if ok:
            assert b"".join(b.out for b in blocks) == zlib.decompress(bad, -15)
        refused += not ok
    assert refused or mode[0] in ("l0", "huffman", "rle")   # (most flips there leave a valid stream)


def test_member_frame_is_strict():
    text = TEXTS[2][1][:3000]
    raw = _raw(text, 9, zlib.Z_FIXED)
    m = wrap_member(raw, text)
    assert read_member(m)[1] == text
    for bad in (m + b"\0", m[:-1], m[:3] + b"\x08" + m[4:], m[:9] + b"\x03" + m[10:],
                m[:-8] + bytes([m[-8] ^ 1]) + m[-7:], m[:-4] + bytes([m[-4] ^ 1]) + m[-3:]):
        with pytest.raises(DeflateError):
            read_member(bad)
    blocks, end = inflate(raw)
    if end & 7:                                      # a bit set after the last block
        bad = bytearray(m)
        bad[10 + len(raw) - 1] |= 0x80
        with pytest.raises(DeflateError, match="bits set after"):
            read_member(bytes(bad))


# ---- the model ----

def _brute_candidates(t):
    cand = [-1] * len(t)
    for p in range(len(t) - MIN_MATCH + 1):
        for j in range(p - 1, -1, -1):
            if gz_model.hash4(t, j) == gz_model.hash4(t, p):
                cand[p] = j
                break
    return cand


@pytest.mark.parametrize("name,text", TEXTS, ids=[t[0] for t in TEXTS])
def test_model_replays_and_agrees_with_brute_force(name, text):
    text = text[:SUB + 700]
    for c, toks in zip(gz_model.sub_chunks(text), gz_model.parse_text(text)):
        assert replay(toks) == c
        for t in toks:
            assert not isinstance(t, tuple) or (gz_model.MIN_MATCH <= t[0] <= gz_model.MAX_MATCH)
    short = text[:900]
    assert gz_model.candidates(short) == _brute_candidates(short)
    # a 258-byte run and a tail shorter than MIN_MATCH
    t = b"x" * 600 + b"abc"
    assert gz_model.parse(t) == [120, (258, 1), (258, 1), (83, 1), 97, 98, 99]


@pytest.mark.parametrize("name,text", TEXTS, ids=[t[0] for t in TEXTS])
def test_fixed_cost_equals_zlib_fixed_streams(name, text):
    blocks, _ = inflate(_raw(text, 9, zlib.Z_FIXED))
    assert name == "random" or all(b.btype == 1 for b in blocks)   # (zlib stores random bytes: shorter)
    for b in blocks:
        assert b.btype == 0 or gz_model.fixed_cost(b.tokens) == b.bit_len


def test_huffman_restatement():
    r = random.Random(2)
    for _ in range(200):
        n = r.randrange(2, 40)
        freq = [r.choice([0, 1, 1, 2, 3, 5, 50, 1000]) * r.randrange(1, 4) for _ in range(n)]
        if sum(1 for f in freq if f) < 2:
            continue
        lens, rebuilds = gz_model.huff_lengths(freq, 15)
        assert sum(1 << (15 - l) for l in lens if l) == 1 << 15
        if not rebuilds:
            assert max(lens) == gz_model.huffman_depth(freq, leaf_first=True)
    fib = [1, 1, 1, 3, 4, 7, 11, 18, 29]             # w[k+2] > w[0] + .. + w[k]: a chain whatever the tie-breaking
    assert gz_model.huffman_depth(fib, True) == gz_model.huffman_depth(fib, False) == 8
    lens, rebuilds = gz_model.huff_lengths(fib, 7)
    assert rebuilds >= 1 and max(lens) <= 7 and sum(1 << (7 - l) for l in lens) == 1 << 7


# ---- check_member has teeth ----

def _canon(lens):
    """Canonical codes (RFC 1951 3.2.2) of a length array."""
    nxt, c = {}, 0
    for b in range(1, 16):
        c = (c + sum(1 for l in lens if l == b - 1 and l)) << 1
        nxt[b] = c
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _member(text, dynamic=False, pad_hclen=0, pad_hlit=0):
    """The model's tokens as a member that keeps every rule: fixed-Huffman blocks, or with `dynamic` blocks
    with codes of their own by the model's restatement of the documented length assignment.  pad_hclen and
    pad_hlit send that many more (zero) entries than the trimmed counts."""
    from tests.deflate_trace import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_LIT, LEN_BASE, LEN_EXTRA
    acc = n = 0

    def put(v, k):
        nonlocal acc, n
        acc |= v << n
        n += k

    def code(v, k):                                   # Huffman codes go in most significant bit first
        put(int(format(v, "0%db" % k)[::-1], 2), k)

    chunks = gz_model.sub_chunks(text)
    for k, c in enumerate(chunks):
        toks = gz_model.parse(c)
        put((1 if k == len(chunks) - 1 else 0) | (4 if dynamic else 2), 3)
        if dynamic:
            ll, dd = gz_model.histograms(toks)
            lit_l = gz_model.huff_lengths(gz_model.with_dummies(ll), 15)[0]
            dist_l = gz_model.huff_lengths(gz_model.with_dummies(dd), 15)[0]
            nlit = max([257] + [s + 1 for s, l in enumerate(lit_l) if l]) + pad_hlit
            ndist = max([1] + [s + 1 for s, l in enumerate(dist_l) if l])
            stream = gz_model.code_length_stream(lit_l, dist_l, pad_lit=pad_hlit)
            cl_l = gz_model.huff_lengths(gz_model.with_dummies(gz_model.code_length_counts(stream)), 7)[0]
            ncl = max(4, max(q + 1 for q in range(19) if cl_l[CL_ORDER[q]])) + pad_hclen
            put(nlit - 257, 5)
            put(ndist - 1, 5)
            put(ncl - 4, 4)
            for q in range(ncl):
                put(cl_l[CL_ORDER[q]], 3)
            cl_c = _canon(cl_l)
            for sy, ex in stream:
                code(cl_c[sy], cl_l[sy])
                put(ex, {16: 2, 17: 3, 18: 7}.get(sy, 0))
            lit_c, dist_c = _canon(lit_l), _canon(dist_l)
        else:
            lit_l, dist_l = FIXED_LIT, [5] * 30
            lit_c, dist_c = _canon(FIXED_LIT), list(range(30))
        for t in toks:
            if isinstance(t, tuple):
                ls, ds = gz_model.len_sym(t[0]), gz_model.dist_sym(t[1])
                code(lit_c[257 + ls], lit_l[257 + ls])
                put(t[0] - LEN_BASE[ls], LEN_EXTRA[ls])
                code(dist_c[ds], dist_l[ds])
                put(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])
            else:
                code(lit_c[t], lit_l[t])
        code(lit_c[256], lit_l[256])
    return wrap_member(acc.to_bytes((n + 7) // 8, "little"), text)


def _fixed_member(text):
    return _member(text)


def test_check_member_accepts_a_conforming_member():
    text = TEXTS[2][1][:2 * SUB + 3]
    tally = {}
    blocks = gz_model.check_member(_fixed_member(text), text, tally)
    assert len(blocks) == 3 and tally == {1: 3}
    assert any(isinstance(t, tuple) for b in blocks for t in b.tokens)
    gz_model.check_member(_fixed_member(b""), b"")


def test_check_member_on_dynamic_blocks():
    """The branch for blocks with codes of their own: a hand-made member is accepted, and refused when its
    header counts are padded or when the fixed code would have been no longer."""
    text = TEXTS[2][1][:2 * SUB + 700]
    tally = {}
    blocks = gz_model.check_member(_member(text, dynamic=True), text, tally)
    assert tally == {2: 3} and all(b.hdist >= 2 for b in blocks)
    for b, c in zip(blocks, gz_model.sub_chunks(text)):       # the restated run-length code is what was sent
        assert b.bit_len == gz_model.dynamic_cost(gz_model.parse(c))
        assert b.cl_syms == [s for s, _ in gz_model.code_length_stream(b.lit_lens, b.dist_lens)]
    nomatch, seen, r = bytearray(b"ab"), set(), random.Random(4)   # 32 symbols, no 3-gram twice: two dummy codes
    while len(nomatch) < 600:
        c = next(c for c in r.sample(range(97, 129), 32) if bytes(nomatch[-2:]) + bytes([c]) not in seen)
        seen.add(bytes(nomatch[-2:]) + bytes([c]))
        nomatch.append(c)
    nomatch = bytes(nomatch)
    assert all(isinstance(t, int) for t in gz_model.parse(nomatch))
    assert gz_model.check_member(_member(nomatch, dynamic=True), nomatch)[0].hdist == 2
    _refused(_member(text, dynamic=True, pad_hclen=1), text, "HCLEN")
    _refused(_member(text, dynamic=True, pad_hlit=1), text, "HLIT")
    _refused(_member(b"abcdefgh", dynamic=True), b"abcdefgh", "the fixed one costs")
    _refused(_member(b"ab", dynamic=True), b"ab", "the fixed one costs|must be fixed")


def test_code_length_limit_case():
    """The input of the GPU suite that makes the code-length code too deep for 7 bits, checked here without a GPU:
    its layout, the lengths its literals get, and the depth under both ways of breaking ties."""
    payload, lit = gz_model.code_length_limit_payload()
    text = b"p1\n0\t" + payload + b"\n"
    assert oracle_lib.transform(b"c\t0\t1\t" + payload + b"\n")[1][0][2] == text and len(text) == 2 * SUB - 1
    toks = gz_model.parse_text(text)[1]
    assert all(isinstance(t, int) for t in toks)
    ll, dd = gz_model.histograms(toks)
    assert gz_model.huff_lengths(gz_model.with_dummies(ll), 15) == (lit + [0] * 29, 0) and not any(dd)
    cnt = gz_model.predicted_code_length_counts(toks)
    assert sorted(c for c in cnt if c) == [1, 1, 2, 4, 5, 9, 14, 23, 64]
    assert gz_model.huffman_depth(cnt, True) == gz_model.huffman_depth(cnt, False) == 8
    lens, rebuilds = gz_model.huff_lengths(cnt, 7)
    assert rebuilds >= 1 and max(lens) <= 7
    blocks = gz_model.check_member(_member(text, dynamic=True), text)
    assert blocks[1].btype == 2 and gz_model.code_length_counts([(s, 0) for s in blocks[1].cl_syms]) == cnt


def test_pass_through_bytes():
    """The payload bytes the transform leaves alone: all but NUL (ends the field), newline and 0xFF (ends the
    input).  The GPU cases of tests/test_gpu_gzip_blocks.py build their payloads from these."""
    ok = set()
    for b in range(256):
        p = b"x" + bytes([b]) + b"y"
        segs = oracle_lib.transform(b"c\t0\t1\t" + p + b"\n")[1]
        if len(segs) == 1 and segs[0][2] == b"p1\n0\t" + p + b"\n":
            ok.add(b)
    assert ok == set(range(256)) - {0, 10, 255}


def _refused(m, text, why):
    with pytest.raises(AssertionError, match=why):
        gz_model.check_member(m, text)


def test_check_member_refuses_zlib_streams():
    r = random.Random(5)
    distinct = bytes(r.sample(range(1, 250), 200))
    # a 3-byte repeat: zlib's level 9 takes it as a match
    text = b"abcdefghijklmnopqrstuvwxyz0123456789ABCxyzQRS abc TUV hij WXY 012 ZZ"
    assert any(isinstance(t, tuple) and t[0] == 3 for b in inflate(_raw(text, 9, 0))[0] for t in b.tokens)
    _refused(wrap_member(_raw(text, 9, 0), text), text, "shorter than MIN_MATCH")
    # a repeat whose earlier copy lies in the previous sub-chunk: zlib reaches back over the block cut
    # (the first sub-chunk has no repeated 3-gram over 32 symbols, so zlib and the model both leave it as literals,
    # in a dynamic block)
    a, seen = bytearray(b"ab"), set()
    while len(a) < SUB:
        c = next(c for c in r.sample(range(97, 129), 32) if bytes(a[-2:]) + bytes([c]) not in seen)
        seen.add(bytes(a[-2:]) + bytes([c]))
        a.append(c)
    a = bytes(a)
    assert gz_model.parse(a) == list(a)
    text = a + b"@" + a[100:140] + b"#"
    raw = _raw(text, 9, 0, block=SUB)
    assert len(inflate(raw)[0]) == 2
    _refused(wrap_member(raw, text), text, "reaches before the sub-chunk")
    # the same text as one block: the block count
    _refused(wrap_member(_raw(text, 9, 0), text), text, "blocks for 2 sub-chunks")
    # stored
    text = distinct
    _refused(wrap_member(_raw(text, 0, 0), text), text, "stored block")
    # no match finder at all
    text = b"chr1\t100\t200\tname\t0\t+\n" * 50
    raw = _raw(text, 6, zlib.Z_HUFFMAN_ONLY)
    assert zlib.decompress(raw, -15) == text
    _refused(wrap_member(raw, text), text, "tokens differ from the model")
    # only some matches: zlib's fastest level misses or shortens what the model takes, or takes another copy
    text = TEXTS[2][1][:SUB]
    _refused(wrap_member(_raw(text, 1, 0), text), text, "tokens differ from the model|shorter than MIN_MATCH")
