"""A permissive deflate, gzip and BGZF writer (TEST INFRASTRUCTURE ONLY).

A sibling of bz2_writer.py: plain Python that writes what it is told, valid or
not, so that the inflater can be put to streams no compressor emits.  A block
is written from explicit tokens (a literal byte as an int, a match as a
``(length, distance)`` pair, ``("sym", s)`` for a bare literal/length symbol,
``("dsym", length, s, extra)`` for a match with a bare distance symbol,
``("bits", value, n)`` for raw bits), explicit code lengths, an explicit
code-length-code stream, stored blocks with any LEN and NLEN, any gzip header
flags, and BGZF framing with any BSIZE and ISIZE.  tests/deflate_trace.py is
the matching reader."""
import heapq
import zlib

from tests.deflate_trace import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA


class BitWriter:
    """Bits least significant first, as deflate packs them."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, n):
        """A Huffman code: most significant bit first."""
        for i in range(n - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def bits(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        b = bytearray(self.out)
        if self.n:
            b.append(self.acc & 0xFF)
        return bytes(b)


def canon_codes(lens):
    """RFC 1951 3.2.2 codes for the lengths, whatever they sum to."""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt = [0] * 17
    c = 0
    for b in range(1, 17):
        c = (c + cnt[b - 1]) << 1
        nxt[b] = c
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return codes


def huff_lengths(freqs, maxlen):
    """Lengths of a complete Huffman code over the symbols with freq > 0 (two
    at least: a lone symbol gets a partner), none above maxlen."""
    freqs = list(freqs)
    used = [s for s, f in enumerate(freqs) if f]
    for s in range(len(freqs)):
        if len(used) >= 2:
            break
        if not freqs[s]:
            freqs[s] = 1
            used.append(s)
    while True:
        heap = [(freqs[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        lens = [0] * len(freqs)
        while len(heap) > 1:
            fa, ka, sa = heapq.heappop(heap)
            fb, kb, sb = heapq.heappop(heap)
            for s in sa + sb:
                lens[s] += 1
            heapq.heappush(heap, (fa + fb, min(ka, kb), sa + sb))
        if max(lens) <= maxlen:
            return lens
        freqs = [1 + f // 2 if f else 0 for f in freqs]


def len_sym(L):
    s = max(i for i in range(29) if LEN_BASE[i] <= L)
    if L == 258:
        s = 28
    return s, L - LEN_BASE[s]


def dist_sym(D):
    s = max(i for i in range(30) if DIST_BASE[i] <= D)
    return s, D - DIST_BASE[s]


def token_freqs(tokens, eob=True):
    lit, dist = [0] * 288, [0] * 32
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        elif t[0] == "sym":
            lit[t[1]] += 1
        elif t[0] == "dsym":
            lit[257 + len_sym(t[1])[0]] += 1
            dist[t[2]] += 1
        elif t[0] == "bits":
            pass
        else:
            lit[257 + len_sym(t[0])[0]] += 1
            dist[dist_sym(t[1])[0]] += 1
    if eob:
        lit[256] += 1
    return lit, dist


def put_tokens(bw, tokens, lit_lens, dist_lens, eob=True):
    lc, dc = canon_codes(lit_lens), canon_codes(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            bw.put_code(lc[t], lit_lens[t])
        elif t[0] == "sym":
            bw.put_code(lc[t[1]], lit_lens[t[1]])
        elif t[0] == "bits":
            bw.put(t[1], t[2])
        elif t[0] == "dsym":
            s, x = len_sym(t[1])
            bw.put_code(lc[257 + s], lit_lens[257 + s])
            bw.put(x, LEN_EXTRA[s])
            bw.put_code(dc[t[2]], dist_lens[t[2]])
            bw.put(t[3], DIST_EXTRA[t[2]] if t[2] < 30 else 0)
        else:
            s, x = len_sym(t[0])
            bw.put_code(lc[257 + s], lit_lens[257 + s])
            bw.put(x, LEN_EXTRA[s])
            s, x = dist_sym(t[1])
            bw.put_code(dc[s], dist_lens[s])
            bw.put(x, DIST_EXTRA[s])
    if eob:
        bw.put_code(lc[256], lit_lens[256])


def stored_block(bw, data, final, length=None, nlen=None):
    """BTYPE 0; length and nlen default to len(data) and its complement."""
    bw.put(1 if final else 0, 1)
    bw.put(0, 2)
    bw.align()
    L = len(data) if length is None else length
    bw.put(L, 16)
    bw.put((L ^ 0xFFFF) if nlen is None else nlen, 16)
    for c in data:
        bw.put(c, 8)


def fixed_block(bw, tokens, final, eob=True):
    bw.put(1 if final else 0, 1)
    bw.put(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST, eob)


def plain_cl_syms(lens):
    """The lengths sent one by one, no repeat symbols."""
    return [(l, 0) for l in lens]


def rle_cl_syms(lens):
    """The lengths run-length coded as RFC 1951 3.2.7 allows (16, 17, 18)."""
    out, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
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
        out.extend([(v, 0)] * left)
        i += r
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_block(bw, tokens, final, lit_lens=None, dist_lens=None, cl_syms=None, cl_lens=None, hlit=None, hdist=None,
                  hclen=None, eob=True, rle=True):
    """BTYPE 2.  lit_lens / dist_lens: the code lengths (default: Huffman
    codes of the tokens, two symbols at least in each); hlit / hdist: how many
    are sent (default: up to the last used, 257 and 1 at least); cl_syms: the
    code-length-code stream as (symbol, extra) pairs (default: the lengths,
    run-length coded if rle); cl_lens: the 19 lengths of the code-length code
    (default: a Huffman code of cl_syms); hclen: how many of them are sent."""
    if lit_lens is None or dist_lens is None:
        lf, df = token_freqs(tokens, eob)
        if lit_lens is None:
            lit_lens = huff_lengths(lf[:286], 15) + [0, 0]
        if dist_lens is None:
            dist_lens = huff_lengths(df[:30], 15) + [0, 0]
    lit_lens = list(lit_lens) + [0] * (288 - len(lit_lens))
    dist_lens = list(dist_lens) + [0] * (32 - len(dist_lens))
    if hlit is None:
        hlit = max([257] + [s + 1 for s in range(288) if lit_lens[s]])
    if hdist is None:
        hdist = max([1] + [s + 1 for s in range(32) if dist_lens[s]])
    if cl_syms is None:
        seq = lit_lens[:hlit] + dist_lens[:hdist]
        cl_syms = rle_cl_syms(seq) if rle else plain_cl_syms(seq)
    if cl_lens is None:
        f = [0] * 19
        for s, _ in cl_syms:
            f[s] += 1
        cl_lens = huff_lengths(f, 7)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    bw.put(1 if final else 0, 1)
    bw.put(2, 2)
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl_lens[CL_ORDER[i]], 3)
    cc = canon_codes(cl_lens)
    for s, x in cl_syms:
        bw.put_code(cc[s], cl_lens[s])
        if s in CL_EXTRA:
            bw.put(x, CL_EXTRA[s])
    put_tokens(bw, tokens, lit_lens, dist_lens, eob)


def lz_tokens(data, min_match=3, max_dist=32768):
    """A greedy parse with a hash of 3-byte strings: literals and matches."""
    out, last, i, n = [], {}, 0, len(data)
    while i < n:
        key = bytes(data[i:i + 3])
        j = last.get(key) if len(key) == 3 else None
        L = 0
        if j is not None and i - j <= max_dist:
            while L < 258 and i + L < n and data[j + L] == data[i + L]:
                L += 1
        if L >= min_match:
            out.append((L, i - j))
            for k in range(i, min(i + L, n - 2)):
                last[bytes(data[k:k + 3])] = k
            i += L
        else:
            if len(key) == 3:
                last[key] = i
            out.append(data[i])
            i += 1
    return out


def gzip_member(raw, text, flg=0, extra=None, name=None, comment=None, hcrc=False, crc=None, isize=None, mtime=0,
                xfl=0, os_=255):
    """An RFC 1952 member around raw deflate bytes.  flg: bits OR-ed into FLG
    besides those that extra (bytes: the whole extra field), name, comment
    (bytes, the zero is added) and hcrc set; crc, isize: the trailer, default right."""
    f = flg | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | \
        (2 if hcrc else 0)
    h = bytearray([0x1F, 0x8B, 8, f]) + mtime.to_bytes(4, "little") + bytes([xfl, os_])
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += (zlib.crc32(bytes(h)) & 0xFFFF).to_bytes(2, "little")
    c = zlib.crc32(text) if crc is None else crc
    z = len(text) & 0xFFFFFFFF if isize is None else isize
    return bytes(h) + raw + c.to_bytes(4, "little") + z.to_bytes(4, "little")


def bgzf_member(raw, text, bsize=None, isize=None, crc=None, more_extra=b""):
    """A BGZF block: FEXTRA with the BC subfield.  bsize: the value written
    (default: the member's size - 1)."""
    total = 12 + 6 + len(more_extra) + len(raw) + 8
    bs = total - 1 if bsize is None else bsize
    extra = b"BC" + (2).to_bytes(2, "little") + (bs & 0xFFFF).to_bytes(2, "little") + more_extra
    return gzip_member(raw, text, extra=extra, crc=crc, isize=isize)


def bgzf_eof():
    """bgzip's 28-byte end-of-file block."""
    return bgzf_member(b"\x03\x00", b"")


def raw_deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(text) + c.flush()


def bgzf_file(text, block=65280, level=6, eof=True):
    """text as bgzip writes it: blocks of `block` bytes and the end-of-file block."""
    out = bytearray()
    for i in range(0, len(text), block):
        piece = text[i:i + block]
        out += bgzf_member(raw_deflate(piece, level), piece)
    if eof:
        out += bgzf_eof()
    return bytes(out)


def referee(gz):
    """What CPython's zlib makes of gz, member after member until the input is
    exhausted: the bytes, or zlib.error (also for a member that ends early and
    for bytes after the last member that do not begin one)."""
    out, rest = bytearray(), gz
    while rest:
        d = zlib.decompressobj(wbits=31)
        out += d.decompress(rest)
        if not d.eof:
            raise zlib.error("incomplete member")
        rest = d.unused_data
    if not gz:
        raise zlib.error("empty input")
    return bytes(out)
