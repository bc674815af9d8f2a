"""A permissive bzip2 stream writer in plain Python, for decoder tests.

libbz2's encoder uses a small corner of the format (lengths <= 17, complete
codes, a table count fixed by the block size, exactly the needed selectors,
exactly the present bytes in the symbol map, count bytes <= 251).  This writer
leaves every such choice to the caller, per block, so a decoder can be held to
what libbz2's *decoder* accepts.  It does RLE1, a BWT by sorting rotations
(prefix doubling, cyclic), MTF with RUNA/RUNB and the bit stream; codes are
canonical in (length, symbol) order, as hbAssignCodes defines them; the block
CRCs and the combined CRC are computed over the bytes the stream decodes to.
No dependencies; inputs are small (the largest block here is 100000 bytes).
"""

MAGIC_BLOCK = 0x314159265359
MAGIC_END = 0x177245385090
RUNA, RUNB = 0, 1
GROUP = 50                  # symbols per selector (BZ_G_SIZE)

_CRC = []
for _i in range(256):
    _c = _i << 24
    for _ in range(8):
        _c = ((_c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if _c & 0x80000000 else (_c << 1) & 0xFFFFFFFF
    _CRC.append(_c)


def crc32(data: bytes) -> int:
    """bzip2's CRC: polynomial 0x04c11db7, MSB first, initial and final xor ~0."""
    c = 0xFFFFFFFF
    t = _CRC
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ t[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.nacc = 0

    @property
    def bits(self) -> int:
        return len(self.out) * 8 + self.nacc

    def put(self, nbits: int, value: int):
        assert 0 <= value < (1 << nbits), (nbits, value)
        self.acc = (self.acc << nbits) | value
        self.nacc += nbits
        while self.nacc >= 8:
            self.nacc -= 8
            self.out.append((self.acc >> self.nacc) & 0xFF)
        self.acc &= (1 << self.nacc) - 1

    def finish(self) -> bytes:
        if self.nacc:
            self.put(8 - self.nacc, 0)
        return bytes(self.out)


def rle1(data: bytes) -> bytes:
    """The first run-length stage: 4..255 equal bytes become 4 bytes and a count of the rest (0..251)."""
    out = bytearray()
    i, n = 0, len(data)
    while i < n:
        b = data[i]
        j = i
        while j < n and data[j] == b and j - i < 255:
            j += 1
        run = j - i
        if run >= 4:
            out += bytes([b]) * 4
            out.append(run - 4)
        else:
            out += bytes([b]) * run
        i = j
    return bytes(out)


def unrle1(raw: bytes) -> bytes:
    """What a post-RLE1 byte string decodes to (any count byte 0..255).  Four
    equal bytes at the very end, with no count after them, add nothing here;
    libbz2 refuses such a block."""
    out = bytearray()
    run, last = 0, -1
    for c in raw:
        if run == 4:
            out += bytes([last]) * c
            run = 0
            continue
        if run and c == last:
            run += 1
        else:
            run, last = 1, c
        out.append(c)
    return bytes(out)


def count_byte_positions(raw: bytes):
    """Positions of raw that a decoder reads as RLE1 count bytes."""
    pos = []
    run, last = 0, -1
    for i, c in enumerate(raw):
        if run == 4:
            pos.append(i)
            run = 0
            continue
        if run and c == last:
            run += 1
        else:
            run, last = 1, c
    return pos


def bwt(block: bytes):
    """-> (last column, origPtr) of the sorted cyclic rotations (equal rotations keep index order)."""
    n = len(block)
    assert n > 0
    rank = list(block)
    k = 1
    order = list(range(n))
    while True:
        key = [(rank[i], rank[(i + k) % n]) for i in range(n)]
        order.sort(key=key.__getitem__)
        new = [0] * n
        r = 0
        prev = key[order[0]]
        for idx in order:
            if key[idx] != prev:
                r += 1
                prev = key[idx]
            new[idx] = r
        rank = new
        if r == n - 1 or k >= n:
            break
        k *= 2
    order = sorted(range(n), key=rank.__getitem__)   # stable: equal rotations by index
    last = bytes(block[(i - 1) % n] for i in order)
    return last, order.index(0)


def start_node(last: bytes, orig_ptr: int) -> int:
    """tt[origPtr] >> 8 of libbz2's decoder: where the inverse walk starts."""
    return sorted(range(len(last)), key=last.__getitem__)[orig_ptr]


def mtf_rle2(last: bytes, symbols: bytes):
    """Move-to-front over the declared symbols with RUNA/RUNB zero runs; ends with EOB."""
    lst = list(range(len(symbols)))
    index = {b: i for i, b in enumerate(symbols)}
    out = []
    zrun = 0

    def flush():
        nonlocal zrun
        z = zrun
        while z > 0:                                  # bijective base 2: RUNA = 1, RUNB = 2
            if z & 1:
                out.append(RUNA)
                z = (z - 1) >> 1
            else:
                out.append(RUNB)
                z = (z - 2) >> 1
        zrun = 0

    for b in last:
        s = index[b]
        p = lst.index(s)
        if p == 0:
            zrun += 1
            continue
        flush()
        out.append(p + 1)
        del lst[p]
        lst.insert(0, s)
    flush()
    out.append(len(symbols) + 1)
    return out


def assign_codes(lengths):
    """hbAssignCodes: canonical codes in (length, symbol) order; no check that they fit their lengths."""
    code = [0] * len(lengths)
    vec = 0
    for n in range(min(lengths), max(lengths) + 1):
        for i, L in enumerate(lengths):
            if L == n:
                code[i] = vec
                vec += 1
        vec <<= 1
    return code


def flat_lengths(alpha: int, extra: int = 0):
    """Every symbol at the same length: the shortest that holds alpha codes, plus extra."""
    L = 1
    while (1 << L) < alpha:
        L += 1
    return [L + extra] * alpha


def stair_lengths(alpha: int):
    """A complete code 1, 2, 3, .., alpha-1, alpha-1 (alpha <= 21)."""
    assert 2 <= alpha <= 21
    return list(range(1, alpha)) + [alpha - 1]


class Block:
    """One block and everything the format leaves free in it.

    data            bytes before RLE1, or
    raw             bytes after RLE1, written as they are (count bytes 252..255)
    tables          list of code-length lists (one per table, each alpha long),
                    or a function alpha -> that list; default two flat tables
    selectors       list of table numbers, one per 50 symbols, or a function
                    (groups needed, tables) -> list; default cycles the tables
    extra_selectors selectors appended after the needed ones (never used)
    extra_map       bytes declared in the symbol map beyond those present
    Header overrides, for streams a decoder must refuse: rand, orig_ptr,
    n_tables_field, n_sel_field, empty_map, header_tables (lengths written in
    the header while the data keeps the codes of `tables`).
    """

    def __init__(self, data=None, raw=None, tables=None, selectors=None, extra_selectors=0, extra_map=b"",
                 rand=0, orig_ptr=None, n_tables_field=None, n_sel_field=None, empty_map=False,
                 header_tables=None):
        assert (data is None) != (raw is None)
        self.raw = rle1(data) if raw is None else bytes(raw)
        assert len(self.raw) > 0, "an empty block cannot be written; leave it out"
        self.out = unrle1(self.raw)
        self.tables, self.selectors = tables, selectors
        self.extra_selectors, self.extra_map = extra_selectors, bytes(extra_map)
        self.rand, self.orig_ptr = rand, orig_ptr
        self.n_tables_field, self.n_sel_field = n_tables_field, n_sel_field
        self.empty_map, self.header_tables = empty_map, header_tables


class BlockInfo:
    """What was written: raw (the bytes after RLE1) and their number nblock,
    origPtr, the start node of the inverse walk, the bit position of the block
    magic, nin, the number of symbols coded (EOB included), those symbols, the
    selectors and code lengths written and the decoded length."""
    __slots__ = ("raw", "nblock", "orig_ptr", "start", "bit", "nin", "nsym", "syms", "selectors", "out_len",
                 "tables")


def _write_block(bw: BitWriter, b: Block) -> BlockInfo:
    raw = b.raw
    last, orig = bwt(raw)
    symbols = bytes(sorted(set(raw) | set(b.extra_map)))
    nin = len(symbols)
    alpha = nin + 2
    syms = mtf_rle2(last, symbols)
    tables = b.tables(alpha) if callable(b.tables) else b.tables
    if tables is None:
        tables = [flat_lengths(alpha), flat_lengths(alpha)]
    assert all(len(t) == alpha for t in tables), (alpha, [len(t) for t in tables])
    need = (len(syms) + GROUP - 1) // GROUP
    sel = b.selectors(need, len(tables)) if callable(b.selectors) else b.selectors
    if sel is None:
        sel = [g % len(tables) for g in range(need)]
    sel = list(sel)
    assert len(sel) >= need and all(0 <= s < len(tables) for s in sel)
    sel += [0] * b.extra_selectors

    info = BlockInfo()
    info.raw = raw
    info.nblock, info.orig_ptr, info.start = len(raw), orig, start_node(last, orig)
    info.bit, info.nin, info.nsym, info.selectors = bw.bits, nin, len(syms), sel
    info.out_len, info.tables, info.syms = len(b.out), tables, syms

    bw.put(48, MAGIC_BLOCK)
    bw.put(32, crc32(b.out))
    bw.put(1, b.rand)
    bw.put(24, orig if b.orig_ptr is None else b.orig_ptr)
    used = [0] * 16
    if not b.empty_map:
        for s in symbols:
            used[s >> 4] |= 0x8000 >> (s & 15)
    bw.put(16, sum(0x8000 >> i for i in range(16) if used[i]))
    for u in used:
        if u:
            bw.put(16, u)
    bw.put(3, len(tables) if b.n_tables_field is None else b.n_tables_field)
    bw.put(15, len(sel) if b.n_sel_field is None else b.n_sel_field)
    mtf = list(range(len(tables)))
    for s in sel:                                     # selectors: MTF, then unary
        p = mtf.index(s)
        bw.put(p + 1, ((1 << p) - 1) << 1)
        del mtf[p]
        mtf.insert(0, s)
    for t in (b.header_tables or tables):             # code lengths: 5-bit start, then +-1 steps
        curr = t[0]
        bw.put(5, curr)
        for L in t:
            while curr < L:
                bw.put(2, 0b10)
                curr += 1
            while curr > L:
                bw.put(2, 0b11)
                curr -= 1
            bw.put(1, 0)
    codes = [assign_codes(t) for t in tables]
    for i, s in enumerate(syms):
        t = sel[i // GROUP]
        L = tables[t][s]
        assert codes[t][s] < (1 << L), "symbol %d of table %d has no code of its length" % (s, t)
        bw.put(L, codes[t][s])
    return info


class Stream:
    """data: the stream's bytes; out: what it decodes to; level, blocks (BlockInfo per block)."""

    def __init__(self, data, out, level, blocks):
        self.data, self.out, self.level, self.blocks = data, out, level, blocks

    @property
    def n_blocks(self):
        return len(self.blocks)


def write_stream(blocks, level: int = 9) -> Stream:
    """blocks: Block objects (or bytes, for defaults), cut where the caller cut them."""
    assert 1 <= level <= 9
    bw = BitWriter()
    for ch in b"BZh":
        bw.put(8, ch)
    bw.put(8, ord("0") + level)
    combined = 0
    infos = []
    out = bytearray()
    for b in blocks:
        if not isinstance(b, Block):
            b = Block(data=b)
        infos.append(_write_block(bw, b))
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc32(b.out)
        out += b.out
    bw.put(48, MAGIC_END)
    bw.put(32, combined)
    return Stream(bw.finish(), bytes(out), level, infos)
