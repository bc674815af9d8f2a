"""The parse that the header of gz_deflate.hip describes (TEST INFRASTRUCTURE ONLY).

Each SUB-byte sub-chunk of a segment's text is parsed on its own.  A position
p with p + MIN_MATCH <= len has the hash (le32(text[p:p+4]) * MULT mod 2^32)
>> SHIFT; its candidate is the most recent earlier position of the sub-chunk
with the same hash (every position enters the table, matched over or not);
the match length is the common prefix, capped at min(len - p, MAX_MATCH), and
counts from MIN_MATCH up; the parse is greedy from position 0.  The constants
are read from the source.  The Huffman codes are the kernel's own business:
this model pins the tokens and what the fixed code would cost for them, and
restates the documented length assignment (huff_lengths) only so that a CPU
search can tell whether an input makes it rebuild."""
import os
import re

from tests.deflate_trace import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "starch_amd", "csrc", "gz_deflate.hip")).read()


def _const(pattern):
    m = re.search(pattern, _SRC)
    assert m, pattern
    return m


SUB = int(_const(r"constexpr uint32_t SUB = (\d+);").group(1))
_h = _const(r"\(w \* (\d+)u\) >> (\d+)")
MULT, SHIFT = int(_h.group(1)), int(_h.group(2))
_m = _const(r"constexpr uint32_t MIN_MATCH = (\d+), MAX_MATCH = (\d+);")
MIN_MATCH, MAX_MATCH = int(_m.group(1)), int(_m.group(2))
assert MIN_MATCH == 4, "the hash reads 4 bytes"


def sub_chunks(text):
    """The sub-chunks of a segment's text (an empty text is one empty block)."""
    return [text[i:i + SUB] for i in range(0, len(text), SUB)] or [b""]


def hash4(t, p):
    return ((int.from_bytes(t[p:p + 4], "little") * MULT) & 0xFFFFFFFF) >> SHIFT


def candidates(t):
    """cand[p]: the most recent earlier position with p's hash, or -1."""
    n = len(t)
    last = {}
    cand = [-1] * n
    for p in range(n - MIN_MATCH + 1):
        h = hash4(t, p)
        cand[p] = last.get(h, -1)
        last[h] = p
    return cand


def match_len(t, j, p):
    lim = min(len(t) - p, MAX_MATCH)
    L = 0
    while L < lim and t[j + L] == t[p + L]:
        L += 1
    return L


def parse(t, cand=None):
    """Greedy token list of one sub-chunk: literal bytes and (length, distance) pairs."""
    assert len(t) <= SUB
    if cand is None:
        cand = candidates(t)
    toks = []
    p = 0
    n = len(t)
    while p < n:
        j = cand[p]
        L = match_len(t, j, p) if j >= 0 else 0
        if L >= MIN_MATCH:
            toks.append((L, p - j))
            p += L
        else:
            toks.append(t[p])
            p += 1
    return toks


def parse_text(text):
    return [parse(c) for c in sub_chunks(text)]


def len_sym(L):
    s = 28
    while LEN_BASE[s] > L:
        s -= 1
    return s


def dist_sym(d):
    s = 29
    while DIST_BASE[s] > d:
        s -= 1
    return s


def fixed_lit_len(s):
    return 8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8


def fixed_cost(tokens):
    """Bits of the tokens as one fixed-Huffman block (RFC 1951 3.2.6): the
    3-bit header, every code and its extra bits, the 7-bit end-of-block."""
    bits = 3 + 7
    for t in tokens:
        if isinstance(t, tuple):
            ls, ds = len_sym(t[0]), dist_sym(t[1])
            bits += fixed_lit_len(257 + ls) + LEN_EXTRA[ls] + 5 + DIST_EXTRA[ds]
        else:
            bits += fixed_lit_len(t)
    return bits


def histograms(tokens):
    """(literal/length counts [286] with the end-of-block, distance counts [30])."""
    ll, dd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll[257 + len_sym(t[0])] += 1
            dd[dist_sym(t[1])] += 1
        else:
            ll[t] += 1
    ll[256] = 1
    return ll, dd


def huffman_depth(freq, leaf_first=True):
    """Greatest code length of an unrestricted Huffman code for the non-zero
    counts, by the two-queue merge; on equal weights the leaf goes first, or
    the internal node does."""
    leaves = sorted(f for f in freq if f)
    if len(leaves) < 2:
        return len(leaves)
    il = ii = 0
    node_w, node_d = [], []                     # weight, height of each internal node

    def pick():
        nonlocal il, ii
        leaf_ok, node_ok = il < len(leaves), ii < len(node_w)
        take_leaf = leaf_ok and (not node_ok or leaves[il] < node_w[ii] or
                                 (leaves[il] == node_w[ii] and leaf_first))
        if take_leaf:
            il += 1
            return leaves[il - 1], 0
        ii += 1
        return node_w[ii - 1], node_d[ii - 1]

    for _ in range(len(leaves) - 1):
        (wa, da), (wb, db) = pick(), pick()
        node_w.append(wa + wb)
        node_d.append(max(da, db) + 1)
    return node_d[-1]


def huff_lengths(freq, maxlen):
    """The length assignment gz_deflate.hip documents: symbols ranked by
    (count, symbol), two queues with the leaf first on equal weights, and while
    the deepest code is too long every count becomes 1 + count / 2 and the tree
    is rebuilt.  -> (lengths, number of rebuilds)."""
    freq = list(freq)
    rebuilds = 0
    while True:
        order = sorted((f, s) for s, f in enumerate(freq) if f)
        m = len(order)
        lens = [0] * len(freq)
        if m == 1:
            lens[order[0][1]] = 1
            return lens, rebuilds
        il = ii = 0
        wint, pleaf, pint = [], [0] * m, [0] * m
        for _ in range(m - 1):
            picked = []
            for _k in range(2):
                if il < m and (ii >= len(wint) or order[il][0] <= wint[ii]):
                    picked.append((order[il][0], il, True))
                    il += 1
                else:
                    picked.append((wint[ii], ii, False))
                    ii += 1
            ni = len(wint)
            wint.append(picked[0][0] + picked[1][0])
            for _w, i, leaf in picked:
                if leaf:
                    pleaf[i] = ni
                else:
                    pint[i] = ni
        dep = [0] * len(wint)
        for j in range(len(wint) - 2, -1, -1):
            dep[j] = dep[pint[j]] + 1
        for i in range(m):
            lens[order[i][1]] = dep[pleaf[i]] + 1
        if m == 0 or max(lens) <= maxlen:
            return lens, rebuilds
        freq = [1 + f // 2 if f else 0 for f in freq]
        rebuilds += 1


def with_dummies(freq):
    """Counts as the kernel feeds them: at least two used symbols per code."""
    freq = list(freq)
    used = sum(1 for f in freq if f)
    for s in range(len(freq)):
        if used >= 2:
            break
        if not freq[s]:
            freq[s] = 1
            used += 1
    return freq


def code_length_stream(lit_lens, dist_lens, pad_lit=0):
    """The run-length coded length sequence the source writes (RFC 1951 3.2.7):
    HLIT and HDIST trimmed to the last used code, one run at a time, zeros as
    18 (11..138) then 17 (3..10), other lengths once then 16 (3..6), what is
    left singly.  -> [(code-length symbol, extra-bits value)]."""
    nlit = max([257] + [s + 1 for s, l in enumerate(lit_lens) if l])
    ndist = max([1] + [s + 1 for s, l in enumerate(dist_lens) if l])
    seq = list(lit_lens[:nlit]) + [0] * pad_lit + list(dist_lens[:ndist])   # (pad_lit: a header that is not trimmed)
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        r = 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        left = r
        if v == 0:
            while left >= 11:
                c = min(left, 138)
                out.append((18, c - 11))
                left -= c
            if left >= 3:
                out.append((17, left - 3))
                left = 0
        else:
            out.append((v, 0))
            left -= 1
            while left >= 3:
                c = min(left, 6)
                out.append((16, c - 3))
                left -= c
        out += [(v, 0)] * left
        i += r
    return out


def code_length_counts(stream):
    cnt = [0] * 19
    for s, _ in stream:
        cnt[s] += 1
    return cnt


def predicted_code_length_counts(tokens):
    """Counts of the code-length symbols for a sub-chunk's tokens, by the restatement above."""
    ll, dd = histograms(tokens)
    lit, _ = huff_lengths(with_dummies(ll), 15)
    dist, _ = huff_lengths(with_dummies(dd), 15)
    return code_length_counts(code_length_stream(lit, dist))


def dynamic_cost(tokens):
    """Bits of the tokens as a dynamic block whose three codes follow the documented length assignment."""
    from tests.deflate_trace import CL_ORDER
    ll, dd = histograms(tokens)
    lit, _ = huff_lengths(with_dummies(ll), 15)
    dist, _ = huff_lengths(with_dummies(dd), 15)
    stream = code_length_stream(lit, dist)
    cl, _ = huff_lengths(with_dummies(code_length_counts(stream)), 7)
    ncl = max(4, max(q + 1 for q in range(19) if cl[CL_ORDER[q]]))
    bits = 3 + 5 + 5 + 4 + 3 * ncl + sum(cl[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in stream)
    bits += sum(f * l for f, l in zip(ll, lit)) + sum(f * l for f, l in zip(dd, dist))
    return bits + sum(LEN_EXTRA[len_sym(t[0])] + DIST_EXTRA[dist_sym(t[1])] for t in tokens if isinstance(t, tuple))


def code_length_limit_payload(seed=0):
    """A payload whose text is two sub-chunks, the second of which makes the
    code-length code too deep for its 7-bit limit.

    The second sub-chunk is SUB - 2 payload bytes and the newline: SUB tokens
    with the end-of-block.  Its literals have counts that are powers of two
    and sum to SUB, so every Huffman code gives symbol s the length
    12 - log2(count): 23 bytes 128 times (5 bits), 5 bytes 64 times (6), 9
    bytes 32 times (7), 64 bytes 8 times (9), 14 bytes twice (11) and two
    bytes once, like the newline and the end-of-block (12).  No 4-gram occurs
    twice, so the block has no match and two dummy distance codes of 1 bit.
    The byte values are dealt so that no length comes four times in a row and
    the unused values from 119 up are one run of zeros.  The code-length
    symbols then count 0: 1, 18: 1, 1: 2, 12: 4, 6: 5, 7: 9, 11: 14, 5: 23
    and 9: 64; each count is above the sum of all counts two or more places
    below it, so the Huffman tree is a chain 8 deep however ties are broken."""
    import random
    r = random.Random(seed)
    classes = [(5, 23), (6, 5), (7, 9), (9, 64), (11, 14), (12, 2)]      # (length, number of byte values)
    slots = [b for b in range(1, 119) if b != 10]
    assert len(slots) == sum(n for _, n in classes)
    while True:                                      # deal the lengths: at most 3 of the 64 between two others
        others = [l for l, n in classes if l != 9 for _ in range(n)]
        r.shuffle(others)
        gaps = [0] * (len(others) + 1)
        for _ in range(64):
            g = r.choice([i for i, k in enumerate(gaps) if k < 3])
            gaps[g] += 1
        lens = []
        for i, k in enumerate(gaps):
            lens += [9] * k + others[i:i + 1]
        lit = [0] * 257
        for b, l in zip(slots, lens):
            lit[b] = l
        lit[10] = lit[256] = 12
        cnt = code_length_counts(code_length_stream(lit, [1, 1]))
        if [(s, c) for s, c in enumerate(cnt) if c] == [(0, 1), (1, 2), (5, 23), (6, 5), (7, 9), (9, 64), (11, 14),
                                                         (12, 4), (18, 1)]:
            break
    pool = [b for b, l in zip(slots, lens) for _ in range(1 << (12 - l))]
    assert len(pool) == SUB - 2
    while True:                                      # order them with no 4-gram twice
        r.shuffle(pool)
        left = list(pool)
        out = bytearray()
        seen = set()
        while left:
            for _ in range(200):
                i = r.randrange(len(left))
                g = bytes(out[-3:]) + bytes([left[i]])
                if len(g) < 4 or g not in seen:
                    break
            else:
                break
            seen.add(g)
            out.append(left[i])
            left[i] = left[-1]
            left.pop()
        if not left and (bytes(out[-3:]) + b"\n") not in seen:
            break
    filler = bytes(r.choice(range(1, 10)) for _ in range(SUB - 5))   # the first sub-chunk: "p1\n0\t" and these
    return filler + bytes(out), lit


def _show(tokens, at, span=6):
    return "tokens[%d:%d] = %r" % (max(0, at - span), at + span, tokens[max(0, at - span):at + span])


def check_member(m, text, tally=None):
    """Every invariant a member of the gzip method owes `text`; -> the blocks
    as traced.  `tally` (a dict) counts the block types seen."""
    import zlib

    from tests.deflate_trace import CL_ORDER, kraft, read_member
    blocks, got = read_member(m)                     # the frame, CRC-32 and ISIZE
    assert zlib.decompress(m, 31) == text and got == text, "member does not inflate to the text"
    chunks = sub_chunks(text)
    assert len(chunks) == max(1, -(-len(text) // SUB))
    assert len(blocks) == len(chunks), "%d blocks for %d sub-chunks" % (len(blocks), len(chunks))
    for k, (b, c) in enumerate(zip(blocks, chunks)):
        where = "block %d of %d (%d bytes, BTYPE %d, bits %d+%d)" % (k, len(blocks), len(c), b.btype, b.bit_off,
                                                                    b.bit_len)
        assert b.out == c, where + ": not its sub-chunk's bytes"
        assert b.bfinal == (1 if k == len(blocks) - 1 else 0), where + ": BFINAL"
        assert b.btype in (1, 2), where + ": stored block"
        pos = 0
        for i, t in enumerate(b.tokens):
            if isinstance(t, tuple):
                assert t[0] >= MIN_MATCH, where + ": match shorter than MIN_MATCH, " + _show(b.tokens, i)
                assert t[0] <= MAX_MATCH, where + ": match longer than MAX_MATCH, " + _show(b.tokens, i)
                assert t[1] <= pos, where + ": distance reaches before the sub-chunk, " + _show(b.tokens, i)
                pos += t[0]
            else:
                pos += 1
        want = parse(c)
        if b.tokens != want:
            i = next((i for i, (x, y) in enumerate(zip(b.tokens, want)) if x != y), min(len(b.tokens), len(want)))
            raise AssertionError("%s: tokens differ from the model at token %d: traced %s, model %s" %
                                 (where, i, _show(b.tokens, i), _show(want, i)))
        fc = fixed_cost(want)
        if tally is not None:
            tally[b.btype] = tally.get(b.btype, 0) + 1
        if b.btype == 1:
            assert b.bit_len == fc, where + ": fixed block of %d bits, fixed_cost %d" % (b.bit_len, fc)
            continue
        # the kernel takes its own code only when strictly shorter, and the fixed one is always there
        assert b.bit_len < fc, where + ": dynamic block of %d bits, the fixed one costs %d" % (b.bit_len, fc)
        # a dynamic header alone is 3 + 5 + 5 + 4 + 3 * 4 = 29 bits or more; 3 literals cost 3 + 3 * 9 + 7 = 37 at
        # the very most as a fixed block, and a dynamic one adds to its header 4 codes of a bit or more and the
        # code-length symbols that reach symbol 256
        assert len(c) > 3, where + ": a sub-chunk of 1 to 3 bytes must be fixed"
        assert max(b.lit_lens) <= 15 and max(b.dist_lens) <= 15 and max(b.clen_lens) <= 7, where + ": length limit"
        for name, lens in (("literal/length", b.lit_lens), ("distance", b.dist_lens), ("code-length", b.clen_lens)):
            assert kraft(lens) == 1 << 15, where + ": Kraft sum of the %s code is %d/32768" % (name, kraft(lens))
        ll, dd = histograms(want)
        for s, f in enumerate(ll):
            assert not f or b.lit_lens[s:s + 1] not in ([], [0]), where + ": literal/length symbol %d has no code" % s
        for s, f in enumerate(dd):
            assert not f or b.dist_lens[s:s + 1] not in ([], [0]), where + ": distance symbol %d has no code" % s
        assert b.hlit == max(257, max(s + 1 for s, f in enumerate(ll) if f)), where + ": HLIT %d" % b.hlit
        used = [s for s, f in enumerate(dd) if f]
        last = used[-1] + 1 if used else 0
        # HDIST is the number of distance codes sent.  The source completes a code of fewer than two used
        # symbols with dummies in the lowest free places, so none used, or symbol 0 alone, gives 2
        want_hdist = last if len(used) >= 2 or last >= 2 else 2
        assert b.hdist == want_hdist, where + ": HDIST %d, wanted %d (used %r)" % (b.hdist, want_hdist, used)
        sent = max(q + 1 for q in range(19) if b.clen_lens[CL_ORDER[q]])
        assert b.hclen == max(4, sent), where + ": HCLEN %d, last non-zero entry %d" % (b.hclen, sent)
    return blocks
