"""An inflater that reports what it read (TEST INFRASTRUCTURE ONLY).

A plain RFC 1951 reader that keeps, for every deflate block, where its bits
lie, the tokens it decoded (a literal byte as an int, a match as a
``(length, distance)`` pair) and, for a dynamic block, the header counts, the
three code-length arrays and the code-length symbols as sent.  It refuses what zlib refuses: a reserved block
type, a stored block whose LEN and NLEN disagree, an over-subscribed code, an
incomplete one (zlib allows only a lone 1-bit code, or none, in the two symbol
alphabets), a missing end-of-block code, HLIT above 286 or HDIST above 30, a
repeat with nothing before it or one that runs past the counts, the symbols
the alphabets reserve, a distance that reaches before the output, and a
stream that ends early.

``read_member`` adds the RFC 1952 frame of gz_deflate.hip, strictly: exactly
its 10-byte header, zero bits after the last block, CRC-32, ISIZE, and no
byte after the member."""
import zlib

HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])   # deflate, no flags, no mtime, OS unknown

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # 288 codes: 286 and 287 take part in the code
FIXED_DIST = [5] * 32


class DeflateError(ValueError):
    pass


class Block:
    """One deflate block as read."""
    __slots__ = ("bfinal", "btype", "bit_off", "bit_len", "out", "tokens", "hlit", "hdist", "hclen", "clen_lens",
                 "lit_lens", "dist_lens", "cl_syms")

    def __init__(self):
        self.hlit = self.hdist = self.hclen = None
        self.clen_lens = self.lit_lens = self.dist_lens = self.cl_syms = None


def kraft(lens):
    """Sum of 2^-l over the non-zero lengths, as a fraction of 2^15."""
    return sum(1 << (15 - l) for l in lens if l)


class _Bits:
    def __init__(self, data, bit):
        self.d = data
        self.pos = bit
        self.end = 8 * len(data)

    def get(self, n):
        v = 0
        p = self.pos
        if p + n > self.end:
            raise DeflateError("stream ends inside a block")
        d = self.d
        for i in range(n):
            v |= ((d[p >> 3] >> (p & 7)) & 1) << i
            p += 1
        self.pos = p
        return v


def _table(lens, kind):
    """Canonical code (RFC 1951 3.2.2) -> {(length, code): symbol}, with
    zlib's rules for which sets of lengths are a code at all."""
    k = kraft(lens)
    if k > 1 << 15:
        raise DeflateError("over-subscribed %s code" % kind)
    mx = max(lens) if lens else 0
    if k < 1 << 15 and mx and (kind == "code-length" or mx != 1):
        raise DeflateError("incomplete %s code" % kind)
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt = [0] * 16
    c = 0
    for b in range(1, 16):
        c = (c + cnt[b - 1]) << 1
        nxt[b] = c
    tab = {}
    for s, l in enumerate(lens):
        if l:
            tab[(l, nxt[l])] = s
            nxt[l] += 1
    return tab, mx


def _sym(br, tab, what):
    t, mx = tab
    d = br.d
    p = br.pos
    end = br.end
    c = 0
    for l in range(1, mx + 1):
        if p >= end:
            raise DeflateError("stream ends inside a block")
        c = (c << 1) | ((d[p >> 3] >> (p & 7)) & 1)     # Huffman codes come most significant bit first
        p += 1
        s = t.get((l, c))
        if s is not None:
            br.pos = p
            return s
    raise DeflateError("invalid %s code" % what)


_FIXED = None


def inflate(data, bit=0):
    """Raw deflate from bit offset `bit` of `data` -> (blocks, bit offset after
    the final block).  Distances reach back over the whole output so far."""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table(FIXED_LIT, "literal/length"), _table(FIXED_DIST, "distance"))
    br = _Bits(data, bit)
    out = bytearray()
    blocks = []
    while True:
        b = Block()
        b.bit_off = br.pos
        b.bfinal = br.get(1)
        b.btype = br.get(2)
        start = len(out)
        b.tokens = []
        if b.btype == 3:
            raise DeflateError("invalid block type")
        if b.btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.get(16), br.get(16)
            if n != (nn ^ 0xFFFF):
                raise DeflateError("invalid stored block lengths")
            if br.pos + 8 * n > br.end:
                raise DeflateError("stream ends inside a block")
            raw = data[br.pos >> 3:(br.pos >> 3) + n]
            br.pos += 8 * n
            out += raw
            b.tokens = list(raw)
        else:
            if b.btype == 1:
                lit, dist = _FIXED
            else:
                b.hlit, b.hdist, b.hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                if b.hlit > 286 or b.hdist > 30:
                    raise DeflateError("too many length or distance symbols")
                cl = [0] * 19
                for q in range(b.hclen):
                    cl[CL_ORDER[q]] = br.get(3)
                b.clen_lens = cl
                ct = _table(cl, "code-length")
                lens = []
                b.cl_syms = []                       # the code-length symbols as sent
                tot = b.hlit + b.hdist
                while len(lens) < tot:
                    s = _sym(br, ct, "code-length")
                    b.cl_syms.append(s)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise DeflateError("invalid bit length repeat")
                        v, r = lens[-1], 3 + br.get(2)
                    elif s == 17:
                        v, r = 0, 3 + br.get(3)
                    else:
                        v, r = 0, 11 + br.get(7)
                    if len(lens) + r > tot:
                        raise DeflateError("invalid bit length repeat")
                    lens += [v] * r
                b.lit_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]
                if b.lit_lens[256] == 0:
                    raise DeflateError("invalid code -- missing end-of-block")
                lit, dist = _table(b.lit_lens, "literal/length"), _table(b.dist_lens, "distance")
            toks = b.tokens
            while True:
                s = _sym(br, lit, "literal/length")
                if s < 256:
                    out.append(s)
                    toks.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise DeflateError("invalid literal/length code")
                L = LEN_BASE[s - 257] + br.get(LEN_EXTRA[s - 257])
                ds = _sym(br, dist, "distance")
                if ds > 29:
                    raise DeflateError("invalid distance code")
                D = DIST_BASE[ds] + br.get(DIST_EXTRA[ds])
                if D > len(out):
                    raise DeflateError("invalid distance too far back")
                toks.append((L, D))
                if D >= L:
                    out += out[len(out) - D:len(out) - D + L]
                else:
                    for _ in range(L):
                        out.append(out[-D])
        b.out = bytes(out[start:])
        b.bit_len = br.pos - b.bit_off
        blocks.append(b)
        if b.bfinal:
            return blocks, br.pos


def replay(tokens, history=b""):
    """The bytes a token list stands for, after `history`."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            L, D = t
            if D > len(out):
                raise DeflateError("distance too far back")
            for _ in range(L):
                out.append(out[-D])
        else:
            out.append(t)
    return bytes(out[len(history):])


def read_member(m):
    """One gzip member, framed as gz_deflate.hip frames it -> (blocks, text)."""
    if m[:10] != HEADER:
        raise DeflateError("member header is not %s" % HEADER.hex())
    blocks, end = inflate(m, 80)
    nbytes = (end + 7) >> 3
    if end & 7 and m[nbytes - 1] >> (end & 7):
        raise DeflateError("bits set after the last block")
    if len(m) < nbytes + 8:
        raise DeflateError("member ends before its trailer")
    if len(m) > nbytes + 8:
        raise DeflateError("bytes after the member")
    text = b"".join(b.out for b in blocks)
    if int.from_bytes(m[nbytes:nbytes + 4], "little") != zlib.crc32(text):
        raise DeflateError("CRC-32 mismatch")
    if int.from_bytes(m[nbytes + 4:nbytes + 8], "little") != len(text) & 0xFFFFFFFF:
        raise DeflateError("ISIZE mismatch")
    return blocks, text


def wrap_member(raw_deflate, text):
    """A raw deflate stream framed as read_member expects (for tests that feed zlib's own streams)."""
    return HEADER + raw_deflate + zlib.crc32(text).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")
