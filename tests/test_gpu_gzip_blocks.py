"""Every deflate block of the gzip method (gz_deflate.hip) against a token-level
model.  The reference never implements the method, so there is no output to
pin; what the source documents is pinned instead: one block per 4 KiB
sub-chunk, the hash-match finder's candidate and the greedy parse
(tests/gz_model.py), fixed or dynamic codes by strict cost, complete codes
within the length limits, trimmed header counts, the member frame and the
CRC.  Each case is one chromosome whose column-4 payload carries the bytes of
interest; the oracle's transform says where the sub-chunks fall, and the
layout a case wants is asserted with the model before anything is compressed."""
import gzip
import random
import zlib

import pytest

from tests import gz_model, oracle_lib
from tests.gz_model import MAX_MATCH, SUB, candidates, hash4, match_len, parse, parse_text

pytestmark = pytest.mark.gpu

PRE = b"p1\n0\t"                                      # what the transform puts before the payload of a "0 1" line
ALPHA = bytes(b for b in range(1, 255) if b != 10)    # payload bytes that reach the text unchanged
#                                                       (tests/test_deflate_trace_cpu.py::test_pass_through_bytes)
A32 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef"             # 32 symbols: 5 bits each under a code of the block's own
TALLY = {}                                            # block types over the whole module


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    c.set_compression_method(starch_amd.K_GZIP)
    yield c
    c.close()


def _check(arch, data, trace=True):
    """Every member of the archive against the oracle's text and the model; -> the traced blocks per member."""
    import starch_amd
    idx, members = starch_amd.parse_archive(arch)
    assert idx["archive"]["compressionFormat"] == "gzip"
    _, osegs = oracle_lib.transform(data)
    assert len(members) == len(osegs)
    traced = []
    for m, meta, (chr_, lines, text) in zip(members, idx["streams"], osegs):
        assert meta["chromosome"].encode("latin-1") == chr_ and meta["uncompressedLineCount"] == lines
        assert m[:3] == b"\x1f\x8b\x08"
        assert gzip.decompress(m) == text
        assert meta["combinedCRC"] == zlib.crc32(text)
        traced.append(gz_model.check_member(m, text, TALLY) if trace else None)
    return traced


class Case:
    def __init__(self, name, payload=None, bed=None, text=None, model=None, traced=None):
        self.name, self.payload, self.bed = name, payload, bed
        self.text = PRE + payload + b"\n" if text is None else text
        self.model, self.traced = model, traced

    def lines(self, i):
        chrom = b"c%03d" % i
        return self.bed(chrom) if self.bed else b"%s\t0\t1\t%s\n" % (chrom, self.payload)


def _layout(cases):
    """The BED of the cases, one chromosome each, with every case's text and model expectation asserted."""
    data = b"".join(c.lines(i) for i, c in enumerate(cases))
    _, osegs = oracle_lib.transform(data)
    assert len(osegs) == len(cases)
    for c, (_, _, text) in zip(cases, osegs):
        assert text == c.text, c.name
        if c.model:
            c.model(parse_text(text))
    return data


def _run(ctx, cases):
    data = _layout(cases)
    traced = _check(ctx.compress(data), data)
    for c, blocks in zip(cases, traced):
        if c.traced:
            c.traced(blocks)
    return traced


def _distinct(n, seed, head=PRE, alphabet=ALPHA):
    """n bytes such that no two positions of head + bytes share a hash: no candidate anywhere."""
    r = random.Random(seed)
    t = bytearray(head)
    seen = {hash4(t, p) for p in range(len(t) - 3)}
    assert len(seen) == max(0, len(t) - 3)
    while len(t) < len(head) + n:
        for _ in range(400):
            c = r.choice(alphabet)
            if len(t) < 3:
                break
            h = hash4(bytes(t[-3:]) + bytes([c]), 0)
            if h not in seen:
                seen.add(h)
                break
        else:
            raise AssertionError("no free hash")
        t.append(c)
    out = bytes(t[len(head):])
    assert all(c == -1 for c in candidates(head + out))
    return out


def _matches(toks):
    return [t for t in toks if isinstance(t, tuple)]


def _seeded(build, tries=200):
    """The first seed whose payload has the layout its case wants (build returns None otherwise)."""
    for seed in range(tries):
        got = build(seed)
        if got is not None:
            return got
    raise AssertionError("no seed gives the layout")


def _expect(chunks):
    """model= callback: the matches of each sub-chunk, exactly."""
    def f(toks):
        assert [_matches(t) for t in toks] == chunks, [_matches(t) for t in toks]
    return f


# ---- lengths ----

def _bedlike(n, seed):
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += b"id%d;%s;%d|" % (r.randrange(50), r.choice([b"exon", b"gene", b"CDS", b"\xe9\xf1"]), r.randrange(10 ** 6))
    return bytes(out[:n])


def test_text_lengths(ctx):
    tails = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129]
    lens = [SUB - 1, SUB, SUB + 1, 2 * SUB, 2 * SUB + 1] + [2 * SUB + t for t in tails[1:]] + [SUB + t for t in tails]
    cases = [Case("smallest", bed=lambda ch: ch + b"\t0\t0\n", text=b"0\n")]
    for n in lens:
        cases.append(Case("len%d" % n, _bedlike(n - 6, n)))
        assert len(cases[-1].text) == n
    assert {len(c.text) % SUB for c in cases} >= set(tails) | {0, SUB - 1}
    traced = _run(ctx, cases)
    assert [len(b) for b in traced] == [max(1, -(-len(c.text) // SUB)) for c in cases]
    # a 1, 2 or 3 byte sub-chunk has no hash at all and is a fixed block of literals
    for c, blocks in zip(cases, traced):
        if 1 <= len(c.text) % SUB <= 3:
            assert blocks[-1].btype == 1 and blocks[-1].tokens == list(c.text[-(len(c.text) % SUB):])


# ---- match length ----

def _collision(seed, prefix=0):
    """Two different 4-grams of payload bytes with one hash, the first `prefix` bytes in common."""
    r = random.Random(seed)
    for _ in range(1000):
        by = {}
        pre = bytes(r.choice(ALPHA) for _ in range(prefix))
        for _k in range(2000):
            g = pre + bytes(r.choice(ALPHA) for _ in range(4 - prefix))
            h = hash4(g, 0)
            if h in by and by[h] != g:
                return by[h], g
            by[h] = g
    raise AssertionError("no collision")


def _repeat_case(L):
    def build(seed):
        d = _distinct(L + 16, 1000 * L + seed)
        a, sep, tail = d[:L], d[L:L + 8], d[L + 8:]
        p = a + sep + a + tail
        dist = L + 8
        want = [(min(L, MAX_MATCH), dist)] if L >= gz_model.MIN_MATCH else []   # a 3-byte repeat stays literals
        if L - MAX_MATCH >= 4:
            want.append((min(L - MAX_MATCH, MAX_MATCH), dist))
        return Case("repeat%d" % L, p, model=_expect([want])) if _matches(parse(PRE + p + b"\n")) == want else None
    return _seeded(build)


def _short_candidate_case():
    """A candidate that shares fewer than MIN_MATCH bytes.  (The hash keeps the top 12 bits of a product with an
    odd constant, so 4-grams that differ in the last byte alone never collide: three bytes in common is out of
    reach for a candidate, two is the most.)"""
    def build(seed):
        g1, g2 = _collision(seed, prefix=2)
        d = _distinct(24, seed)
        p = d[:8] + g1 + d[8:16] + g2 + d[16:]
        t = PRE + p + b"\n"
        at1, at2 = len(PRE) + 8, len(PRE) + 8 + 4 + 8
        if candidates(t)[at2] != at1 or match_len(t, at1, at2) != 2 or _matches(parse(t)):
            return None
        return Case("candidate2", p, model=_expect([[]]))
    return _seeded(build)


def test_match_lengths(ctx):
    cases = [_short_candidate_case()]
    for L in [3, 4, 5, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 226, 227, 257, 258, 259, 260, 261, 262, 516]:
        cases.append(_repeat_case(L))
    traced = _run(ctx, cases)
    assert sorted({t[0] for b in traced for t in _matches(b[0].tokens)}) == [
        4, 5, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 226, 227, 257, 258]


# ---- distance ----

def _distance_case(d):
    def build(seed):
        u = _distinct(d + 8, 7919 * d + seed)
        unit, tail = u[:d], u[d:]
        p = unit + (unit * 9)[:8] + tail
        return Case("dist%d" % d, p, model=_expect([[(8, d)]])) if _matches(parse(PRE + p + b"\n")) == [(8, d)] else None
    return _seeded(build)


def _largest_distance_case():
    d = SUB - 4

    def build(seed):
        r = random.Random(seed)
        f1 = bytes(r.choice(ALPHA) for _ in range(SUB - len(PRE)))
        a = bytes(r.choice(ALPHA) for _ in range(4))
        f2 = bytes(r.choice(ALPHA) for _ in range(SUB - 8))
        p = f1 + a + f2 + a
        want = [[], [(4, d)], []]
        if [_matches(t) for t in parse_text(PRE + p + b"\n")] != want:
            return None
        return Case("dist%d" % d, p, model=_expect(want))
    return _seeded(build)


def test_distances(ctx):
    from tests.deflate_trace import DIST_BASE
    bases = [b for b in DIST_BASE if b < SUB]
    ds = sorted(set(bases) | {b - 1 for b in bases if b > 1})
    assert ds[:9] == [1, 2, 3, 4, 5, 6, 7, 8, 9] and ds[-2:] == [3072, 3073]
    cases = [_distance_case(d) for d in ds] + [_largest_distance_case()]
    traced = _run(ctx, cases)
    got = sorted({t[1] for blocks in traced for b in blocks for t in _matches(b.tokens)})
    assert got == ds + [SUB - 4]


# ---- sub-chunk edges ----

def test_sub_chunk_edges(ctx):
    def run_model(toks):
        assert toks[0][-1] == ((SUB - len(PRE) - 1) % MAX_MATCH or MAX_MATCH, 1)     # stops at the edge
        assert toks[1][:2] == [65, (MAX_MATCH, 1)]                                    # and restarts with a literal
        assert all(t[1] == 1 for c in toks for t in _matches(c))
    cases = [Case("run5000", b"A" * 5000, model=run_model)]

    def clipped(seed):
        r = random.Random(seed)
        rnd = lambda n: bytes(r.choice(ALPHA) for _ in range(n))
        a = rnd(20)
        f1, f3 = rnd(100), rnd(50)
        f2 = rnd(SUB - 10 - len(PRE) - 100 - 20)
        p = f1 + a + f2 + a + f3
        want = [[(10, 20 + len(f2))], []]                   # lim = len - p clips the match; nothing to match after the edge
        ok = [_matches(t) for t in parse_text(PRE + p + b"\n")] == want
        return Case("clipped", p, model=_expect(want)) if ok else None
    cases.append(_seeded(clipped))

    def previous(seed):
        r = random.Random(seed)
        rnd = lambda n: bytes(r.choice(ALPHA) for _ in range(n))
        a = rnd(16)
        p = rnd(2000) + a + rnd(SUB - len(PRE) - 2016) + rnd(1000) + a + rnd(500)
        assert (PRE + p).index(a, SUB) == SUB + 1000        # the second copy lies in the second sub-chunk
        ok = [_matches(t) for t in parse_text(PRE + p + b"\n")] == [[], []]
        return Case("previous", p, model=_expect([[], []])) if ok else None
    cases.append(_seeded(previous))
    _run(ctx, cases)


# ---- many lanes of one hash in one 64-position step ----

def _period_case(period):
    def build(seed):
        u = _distinct(period + 11, 31 * period + seed)
        p = u[:3] + (u[3:3 + period] * 300)[:300] + u[3 + period:]
        m = _matches(parse(PRE + p + b"\n"))
        if not m or any(t[1] != period for t in m) or sum(t[0] for t in m) != 300 - period:
            return None

        def model(toks):
            mm = _matches(toks[0])
            assert mm and all(t[1] == period for t in mm) and sum(t[0] for t in mm) == 300 - period
        return Case("period%d" % period, p, model=model)
    return _seeded(build)


def test_equal_hashes_inside_one_step(ctx):
    _run(ctx, [_period_case(k) for k in (1, 2, 5, 7, 63, 64, 65)])


# ---- hash collisions ----

def test_hash_collisions(ctx):
    def build(seed):
        g1, g2 = _collision(seed)
        d = _distinct(32, seed)
        x = [d[i:i + 8] for i in range(0, 32, 8)]
        masked = x[0] + g1 + x[1] + g2 + x[2] + g1 + x[3]     # the collider takes the table entry: literals
        first = x[0] + g2 + x[1] + g1 + x[2] + g1 + x[3]      # the true repeat is the most recent: a match
        t = PRE + masked + b"\n"
        at = len(PRE) + 8
        if candidates(t)[at + 24] != at + 12 or _matches(parse(t)):
            return None
        if _matches(parse(PRE + first + b"\n")) != [(4, 12)]:
            return None
        return [Case("masked", masked, model=_expect([[]])), Case("first", first, model=_expect([[(4, 12)]]))]
    _run(ctx, _seeded(build))


# ---- alphabets ----

def test_alphabets(ctx):
    r = random.Random(8)
    hi = lambda n: bytes(r.randrange(128, 255) for _ in range(n))
    h3 = [hi(2), hi(2), hi(2)]

    # 18 literals, six of them 9-bit: 3 + 12 * 8 + 6 * 9 + 7 = 160 bits as a fixed block.  A dynamic header for
    # its 12 symbols, scattered from 9 to 256, is 29 bits and seven zero runs or more before the first token; by the
    # documented length assignment the dynamic block is the longer one (asserted), so the kernel must stay fixed.
    def fixed_wins(toks):
        assert gz_model.dynamic_cost(toks[0]) > gz_model.fixed_cost(toks[0]) == 160

    def fixed9(blocks):
        assert blocks[0].btype == 1 and sum(1 for t in blocks[0].tokens if t >= 144) == 6
    cases = [Case("high3", bed=lambda ch: b"".join(b"%s\t%d\t%d\t%s\n" % (ch, i, i + 1, h) for i, h in enumerate(h3)),
                  text=b"p1\n" + b"".join(b"0\t" + h + b"\n" for h in h3), model=fixed_wins, traced=fixed9),
             Case("high_full", hi(SUB - 6))]
    assert len(cases[1].text) == SUB
    a1, a2 = list(ALPHA), list(ALPHA)
    r.shuffle(a1)
    r.shuffle(a2)
    cases.append(Case("every_byte", bytes(a1 + a2), model=lambda toks: None))

    # 2500 literals over 32 symbols with no candidate anywhere.  The block must be dynamic: as a fixed block it is
    # 8 bits a literal, 20000 bits and more; the block's own (optimal) code spends at most 6 bits on each of at
    # most 39 symbols, and no dynamic header is longer than 17 + 57 + 316 * 14 bits.
    def dyn(hdist_max=None, hlit=None):
        def f(blocks):
            assert blocks[0].btype == 2
            assert hdist_max is None or blocks[0].hdist <= hdist_max
            assert hlit is None or blocks[0].hlit == hlit
        return f
    cases.append(Case("no_match", _distinct(2500, 1, alphabet=A32), model=_expect([[]]), traced=dyn(hdist_max=2)))

    def one(seed):
        d = _distinct(2500, 50 + seed, alphabet=A32)
        p = d[:1000] + d[10:18] + d[1000:]
        m = _matches(parse(PRE + p + b"\n"))
        return Case("one_distance", p, model=_expect([m]), traced=dyn()) if len(m) == 1 else None
    cases.append(_seeded(one))
    d = _distinct(2000, 3, alphabet=A32)
    cases.append(Case("len258", d[:1500] + b"~" * 300 + d[1500:], model=_expect([[(258, 1), (41, 1)]]),
                      traced=dyn(hlit=286)))                # symbol 285
    traced = _run(ctx, cases)
    assert all(isinstance(t, int) and t >= 128 for t in traced[1][0].tokens[5:-1])


# ---- the 7-bit limit of the code-length code ----

def test_code_length_limit(ctx):
    """A block whose code-length symbols count 1, 1, 2, 4, 5, 9, 14, 23 and 64: a Huffman chain 8 deep, so the
    kernel has to scale the counts down and build again (the limit-7 loop of huff_lengths).  _check holds the
    block to the limits and to complete codes; the symbols it sent are the run-length code the source describes."""
    payload, lit = gz_model.code_length_limit_payload()

    def model(toks):
        assert all(isinstance(t, int) for t in toks[1])
        cnt = gz_model.predicted_code_length_counts(toks[1])
        assert sorted(c for c in cnt if c) == [1, 1, 2, 4, 5, 9, 14, 23, 64]
        assert gz_model.huffman_depth(cnt, True) == gz_model.huffman_depth(cnt, False) == 8 > 7
        assert gz_model.huff_lengths(cnt, 7)[1] >= 1

    def traced(blocks):
        b = blocks[1]
        assert b.btype == 2 and b.lit_lens == lit and b.dist_lens == [1, 1]      # (counts are powers of two: forced)
        assert b.cl_syms == [s for s, _ in gz_model.code_length_stream(b.lit_lens, b.dist_lens)]
        assert max(b.clen_lens) <= 7 and sum(1 for l in b.clen_lens if l) == 9
    case = Case("limit7", payload, model=model, traced=traced)
    assert len(case.text) == 2 * SUB - 1
    _run(ctx, [case])


# ---- concatenation ----

def _tiny_cases():
    """64 one-line chromosomes of 5, 7, 8 or 10 bytes of text.  Each is one fixed block: a dynamic header is 29 bits,
    reaching symbol 256 takes three zero runs of 18 (8 bits each at least) and two of 17 (4 bits), the 7 codes or
    more another bit each, so 70 bits before the first token, and the fixed block of 10 bytes is 90 with them."""
    r = random.Random(12)
    cases = []
    for i in range(64):
        n = r.choice([0, 1, 2, 4])
        p = bytes(r.choice(b"ACGTNX") for _ in range(n))
        if n:
            cases.append(Case("tiny%d" % i, p))
        else:
            cases.append(Case("tiny%d" % i, bed=lambda ch: ch + b"\t0\t1\n", text=b"p1\n0\n"))
    return cases


def test_concat_word_phases(ctx):
    import starch_amd
    cases = _tiny_cases()
    data = _layout(cases)
    sizes = [10 + (gz_model.fixed_cost(parse(c.text)) + 7) // 8 + 8 for c in cases]
    offs = [4 + sum(sizes[:i]) for i in range(64)]          # the archive's magic, then the members back to back
    phases = [o % 4 for o in offs]
    assert all(phases.count(k) >= 8 for k in range(4)), phases
    arch = ctx.compress(data)
    traced = _check(arch, data)
    idx, members = starch_amd.parse_archive(arch)
    assert [(s["offset"], s["size"]) for s in idx["streams"]] == list(zip(offs, sizes))
    assert all(len(b) == 1 and b[0].btype == 1 for b in traced)
    # streaming, one batch per chromosome: the members are laid out from another base, and the archive is the same
    assert ctx.compress_stream([data[i:i + 37] for i in range(0, len(data), 37)], batch_bytes=1) == arch


def test_concat_member_ends_mid_word(ctx):
    import starch_amd
    cases = [Case("tiny", b"A"), Case("two_blocks", _bedlike(SUB + 700, 5))]
    data = _layout(cases)
    arch = ctx.compress(data)
    _check(arch, data)
    idx, _ = starch_amd.parse_archive(arch)
    first = 10 + (gz_model.fixed_cost(parse(cases[0].text)) + 7) // 8 + 8
    assert first % 4 and idx["streams"][1]["offset"] == 4 + first
    assert ctx.compress_stream([data[:100], data[100:]], batch_bytes=1) == arch


# ---- CRC fold over more than 256 sub-chunks ----

@pytest.mark.parametrize("nsub,tail", [(257, 1), (600, 65)])
def test_crc_fold_many_sub_chunks(ctx, nsub, tail):
    """k_gz_crc gives each of its 256 threads ceil(nsub / 256) registers: 2 with a short last thread, 3 with idle
    ones.  zlib and the index's CRC only: the Python trace of megabytes would take minutes."""
    want = (nsub - 1) * SUB + tail
    r = random.Random(nsub)
    body = r.randbytes(want).translate(bytes(b if b in ALPHA else 65 for b in range(256)))
    lines, n, i = [], 3, 0                                   # "p1\n", then "0\t" + payload + "\n" per line
    while want - n > 0:
        k = min(997, want - n - 3)
        if want - n - 3 - k in (1, 2, 3):                    # leave room for a last line
            k -= 4
        lines.append(b"chrC\t%d\t%d\t%s\n" % (i, i + 1, body[n:n + k]))
        n += 3 + k
        i += 1
    data = b"".join(lines)
    text = oracle_lib.transform(data)[1][0][2]
    assert len(text) == want and len(gz_model.sub_chunks(text)) == nsub and len(text) % SUB == tail
    _check(ctx.compress(data), data, trace=False)


# ---- coverage ----

def test_both_block_types_occurred():
    """Runs last: over the cases above the kernel chose each block type many times."""
    assert TALLY.get(1, 0) >= 10 and TALLY.get(2, 0) >= 10, TALLY
