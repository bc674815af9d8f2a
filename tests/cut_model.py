"""A model of libbz2's RLE1 and block cut (TEST INFRASTRUCTURE ONLY).

Restates bz:bzlib.c ADD_CHAR_TO_BLOCK / add_pair_to_block / flush_RL and the
`nblock >= nblockMAX` check of copy_input_until_stop on a run list, not on
bytes, so a 4 MB input costs milliseconds.  tests/test_cut_model_cpu.py pins
it to the library; tests/test_gpu_cut.py uses it to steer the encoder's block
cut (starch_amd/csrc/bz2_rle.hip k_cut_tab / k_cut) to chosen table entries.

What the library does.  The input is read a byte at a time into a pending run
(state_in_ch, state_in_len); a run is closed at 255 bytes or when the byte
changes, and only then added to the block (min(L, 4) copies, plus a count
byte when L >= 4).  Call such a closed run a chunk; it weighs 1..5 block
bytes.  The block-full test runs before every byte read, so a chunk joins
the block iff the block holds fewer than nblockMAX bytes when the chunk's
first byte is read.  A full block is compressed WITHOUT flush_RL
(bz:bzlib.c:399-402): the pending run -- one byte of it read so far -- stays
pending, keeps counting towards 255 and is added to the next block, whose
CRC covers all its bytes.  So blocks begin at chunk starts and chunk
positions do not depend on the blocks.  Only the end of the input flushes
the pending run into the current block, full or not (bz:bzlib.c:393-397):
when the last chunk is one byte long, that byte was read before the block
was seen to be full, and with BZ_FINISH given in the same call (`final_joins`)
it joins the full block; when it arrived with an earlier BZ_RUN call (Python's
bz2.compress) the full block is closed first and the byte gets its own.

An input is a list of items, each either
  bytes          a literal stretch: no two neighbouring bytes equal, so every
                 byte is a chunk of weight 1, or
  (byte, length) a run of `length` equal bytes (length >= 1),
where neighbouring items do not meet in equal bytes (checked).
"""
import bisect
import collections

import numpy as np

KTB = 4096      # bz2_int.hpp kTB: the tile of k_rle_sum / k_cut_tab
CUT_E = 128     # bz2_rle.hip CUT_E: offsets a table row holds

Block = collections.namedtuple("Block", "beg end n w e")
# beg, end: input span; n: RLE1 size; w: RLE1 offset of its start in the
# stream (W_k); e = w - k * nblockMAX


def nblock_max(level):
    return 100000 * level - 19          # bz:bzlib.c:194


def chunk_w(length):
    return length if length < 4 else 5


def _first_last(item):
    return (item[0], item[-1]) if isinstance(item, (bytes, bytearray)) else (item[0], item[0])


def check_items(items):
    prev = None
    for it in items:
        if isinstance(it, (bytes, bytearray)):
            assert len(it) > 0
            a = np.frombuffer(it, dtype=np.uint8)
            assert not (a[1:] == a[:-1]).any(), "literal stretch with equal neighbours"
        else:
            assert 0 <= it[0] < 256 and it[1] >= 1
        f, l = _first_last(it)
        assert f != prev, "neighbouring items meet in equal bytes"
        prev = l


def to_bytes(items):
    return b"".join(it if isinstance(it, (bytes, bytearray)) else bytes([it[0]]) * it[1] for it in items)


def from_bytes(data):
    """bytes -> items (runs of one byte gathered into literal stretches)."""
    if not data:
        return []
    a = np.frombuffer(data, dtype=np.uint8)
    starts = np.concatenate(([0], np.nonzero(a[1:] != a[:-1])[0] + 1))
    lens = np.diff(np.concatenate((starts, [len(a)])))
    items, lit0 = [], None
    for s, n in zip(starts.tolist(), lens.tolist()):
        if n == 1:
            if lit0 is None:
                lit0 = s
            continue
        if lit0 is not None:
            items.append(bytes(data[lit0:s]))
            lit0 = None
        items.append((data[s], n))
    if lit0 is not None:
        items.append(bytes(data[lit0:]))
    return items


class Cutter:
    """The encoder's input side: feed items, read off `fill` (the current
    block's nblock), finish() -> [Block]."""

    def __init__(self, level):
        self.max = nblock_max(level)
        self.pos = 0            # input bytes read
        self.w = 0              # RLE1 bytes of all closed chunks
        self.bs = 0             # current block: input start, RLE1 start
        self.wbs = 0
        self.blocks = []
        self.last_chunk = 0     # length of the last chunk fed

    @property
    def fill(self):
        return self.w - self.wbs

    @property
    def next_fill(self):
        """nblock as the next chunk will find it (a full block is cut first)."""
        return 0 if self.fill >= self.max else self.fill

    def _cut(self):
        k = len(self.blocks)
        self.blocks.append(Block(self.bs, self.pos, self.w - self.wbs, self.wbs, self.wbs - k * self.max))
        self.bs, self.wbs = self.pos, self.w

    def _chunks(self, count, length, weight):
        # `count` chunks of one length: each joins iff fill < max before it
        while count:
            if self.fill >= self.max:
                self._cut()
            take = min(count, -(-(self.max - self.fill) // weight))
            self.pos += take * length
            self.w += take * weight
            count -= take
        self.last_chunk = length

    def feed(self, item):
        if isinstance(item, (bytes, bytearray)):
            self._chunks(len(item), 1, 1)
        else:
            full, rest = divmod(item[1], 255)
            if full:
                self._chunks(full, 255, 5)
            if rest:
                self._chunks(1, rest, chunk_w(rest))

    def finish(self, final_joins=True):
        blocks = list(self.blocks)
        if self.pos > self.bs:
            k = len(blocks)
            last = Block(self.bs, self.pos, self.w - self.wbs, self.wbs, self.wbs - k * self.max)
            if final_joins and blocks and self.last_chunk == 1 and last.end - last.beg == 1:
                p = blocks.pop()
                last = Block(p.beg, last.end, p.n + 1, p.w, p.e)
            blocks.append(last)
        return blocks


def cut(items, level, final_joins=True):
    check_items(items)
    c = Cutter(level)
    for it in items:
        c.feed(it)
    return c.finish(final_joins)


class Offsets:
    """RLE1 offset W of input positions, as the encoder's tile sums count it:
    a byte at chunk position t weighs 1 (t < 3), 2 (t == 3: its copy and the
    count byte) or 0."""

    def __init__(self, items):
        self.items = items
        self.p0, self.w0 = [], []
        p = w = 0
        for it in items:
            self.p0.append(p)
            self.w0.append(w)
            if isinstance(it, (bytes, bytearray)):
                p += len(it)
                w += len(it)
            else:
                full, rest = divmod(it[1], 255)
                p += it[1]
                w += 5 * full + chunk_w(rest)
        self.length, self.wend = p, w

    def w_at(self, pos):
        if pos >= self.length:
            return self.wend
        i = bisect.bisect_right(self.p0, pos) - 1
        it, r = self.items[i], pos - self.p0[i]
        if isinstance(it, (bytes, bytearray)):
            return self.w0[i] + r
        full, rest = divmod(r, 255)
        return self.w0[i] + 5 * full + min(rest, 3) + (2 if rest >= 4 else 0)

    def row_tiles(self, k, level):
        """Table row k as k_cut_tab scans it: (lo, to_end) -- the tile lo with
        W(lo) < T0 <= W(lo + 1), T0 = (k + 1) * nblockMAX, and whether tiles
        lo and lo + 1 reach the stream's end.  None when T0 > W(end) (no row)."""
        T0 = (k + 1) * nblock_max(level)
        if T0 > self.wend:
            return None
        ntiles = -(-self.length // KTB)
        lo, hi = 0, ntiles                      # W(0) = 0 < T0 <= W(ntiles) = wend
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.w_at(mid * KTB) < T0:
                lo = mid
            else:
                hi = mid
        return lo, (lo + 2) * KTB >= self.length


HEAVY = 0x7A                 # the heavy chunks' byte; the filler stays below it
_ALPHA = 89                  # filler alphabet: bytes 0x21 .. 0x79


def filler(rng, n):
    """n seeded bytes of weight 1 each: neighbours always differ (so no run of
    4, no chunk longer than a byte), no period, new text at every call."""
    if n <= 0:
        return b""
    steps = rng.randint(1, _ALPHA, size=n)
    return ((int(rng.randint(_ALPHA)) + np.cumsum(steps)) % _ALPHA + 0x21).astype(np.uint8).tobytes()


def cut_stream(level, overshoots, tail_runs=(), seed=1):
    """One period per block: filler, then one heavy chunk (a run of 4..255
    bytes of HEAVY, weight 5) placed so that the block it closes ends
    `overshoots[k]` (0..4) bytes past its target W_k + nblockMAX: the chunk
    begins 5 - o bytes before the target, read off the model's fill.  Then
    `tail_runs` (items, or a function of the rng giving items).  -> items"""
    rng = np.random.RandomState(seed)
    mx = nblock_max(level)
    c = Cutter(level)
    items = []
    for k, o in enumerate(overshoots):
        assert 0 <= o <= 4
        for it in (filler(rng, mx + o - 5 - c.next_fill), (HEAVY, int(rng.randint(4, 256)))):
            items.append(it)
            c.feed(it)
        assert len(c.blocks) == k and c.fill == mx + o      # the next chunk start cuts here
    items.extend(tail_runs(rng) if callable(tail_runs) else tail_runs)
    return items


def e_seq(blocks):
    return [b.e for b in blocks]


# ---------------------------------------------------------------- the cases
# Shared by test_cut_model_cpu.py (pins every input's boundaries to libbz2)
# and test_gpu_cut.py (runs them through the encoder).  A case is (level,
# build); build() -> (items, aim), aim naming what the case steers at:
#   k         the block whose table lookup the case is about
#   e         e_k the model must report for it
#   d         the entry that lookup wants: e_{k+1}, or None when block k is
#             the last (no chunk start at or past its target)
#   to_end    what k_cut_tab's two tiles of row k must see (None: not asked)
#   visits    e values that must occur somewhere in the chain

def overs_for(e):
    """Overshoots after which a block starts at e (4 per block, the rest once)."""
    return [4] * (e // 4) + ([e % 4] if e % 4 else [])


def _tail(n):
    return lambda rng: [filler(rng, n)] if n else []


def _edge_last(e, tail):
    """(a) block k, the last full one, starts at e and overshoots by 4; the
    tail after the next chunk start is `tail` bytes, or just reaches / just
    misses the end of row k's second tile ("reach", "miss")."""
    def build():
        overs = overs_for(e) + [4]
        k = len(overs) - 1
        base = cut_stream(1, overs, seed=100 + e)
        lo, _ = Offsets(base + [b"!"]).row_tiles(k, 1)
        p = sum(len(it) if isinstance(it, bytes) else it[1] for it in base)
        reach = (lo + 2) * KTB - p
        assert 1 <= reach <= 2 * KTB
        n = {"reach": reach, "miss": reach + 1}.get(tail, tail)
        items = cut_stream(1, overs, _tail(n), seed=100 + e)
        return items, dict(k=k, e=e, d=e + 4, to_end=n <= reach, nblocks=k + 2)
    return build


def _edge_middle(e):
    def build():
        overs = overs_for(e) + [4] + [0, 1, 0, 2, 0, 0, 3, 0, 0, 1, 0]
        k = len(overs_for(e))
        return cut_stream(1, overs, _tail(777), seed=200 + e), dict(k=k, e=e, d=e + 4, to_end=False)
    return build


def _past_table(overs, visits, seed):
    def build():
        return cut_stream(1, overs, _tail(3000), seed=seed), dict(visits=visits)
    return build


def _ends_in_chunk(e, before, run):
    """(d) after blocks up to e, a last block: filler up to `before` bytes
    below the target, then a trailing run that ends the stream."""
    def build():
        overs = overs_for(e)
        mx = nblock_max(1)
        items = cut_stream(1, overs, lambda rng: [filler(rng, mx - before), (HEAVY, run)], seed=300 + e + run)
        return items, dict(k=len(overs), e=e, d=None, to_end=True, nblocks=len(overs) + 1)
    return build


def _run_cut_inside(e):
    """a trailing run of 600 whose first chunk crosses the target: the cut
    falls inside the run, at its second chunk"""
    def build():
        overs = overs_for(e)
        mx = nblock_max(1)
        items = cut_stream(1, overs, lambda rng: [filler(rng, mx - 2), (HEAVY, 600)], seed=400 + e)
        return items, dict(k=len(overs), e=e, d=e + 3, to_end=True, nblocks=len(overs) + 2)
    return build


def _pattern(overs, seed, level=1, tail=1500):
    def build():
        return cut_stream(level, overs, _tail(tail), seed=seed), dict(visits=[])
    return build


def _random_overs(seed, n):
    return [int(x) for x in np.random.RandomState(seed).randint(0, 5, size=n)]


EDGE_E = (120, 123, 124, 125, 126, 127)
CASES = collections.OrderedDict()
for _e in EDGE_E:
    for _t in (1, 200, 4000, 8100) + (("reach", "miss") if _e in (124, 127) else ()):
        CASES["a_last_e%d_tail_%s" % (_e, _t)] = (1, _edge_last(_e, _t))
for _e in EDGE_E:
    CASES["b_middle_e%d" % _e] = (1, _edge_middle(_e))
CASES["c_past_4x36_mixed"] = (1, _past_table([4] * 36 + [1, 3, 4, 2, 0], [124, 128, 132, 140, 144, 145], 31))
CASES["c_past_129"] = (1, _past_table([4] * 31 + [3, 2, 3, 4, 4], [124, 127, 129, 132, 140], 32))
CASES["d_run255_e12"] = (1, _ends_in_chunk(12, 2, 255))
CASES["d_run255_e125"] = (1, _ends_in_chunk(125, 2, 255))
CASES["d_run600_last_chunk_e12"] = (1, _ends_in_chunk(12, 12, 600))
CASES["d_run600_last_chunk_e126"] = (1, _ends_in_chunk(126, 12, 600))
CASES["d_run600_cut_inside_e12"] = (1, _run_cut_inside(12))
CASES["d_run600_cut_inside_e127"] = (1, _run_cut_inside(127))
CASES["d_ends_at_target_e12"] = (1, _ends_in_chunk(12, 5, 255))
CASES["d_ends_at_target_e127"] = (1, _ends_in_chunk(127, 5, 255))
CASES["e_all4"] = (1, _pattern([4] * 35, 51))
CASES["e_all0"] = (1, _pattern([0] * 35, 52))
CASES["e_cycle"] = (1, _pattern([1, 3, 4, 2, 0] * 7, 53))
CASES["e_random"] = (1, _pattern(_random_overs(54, 35), 54))
# (f) the batch: level 1 streams of three lengths with short ones between, a
# stream whose last block is at the edge in the middle; the level-9 stream
# goes in a call of its own (a call has one level)
CASES["f_len20"] = (1, _pattern(_random_overs(61, 20), 61, tail=5000))
CASES["f_short"] = (1, lambda: ([filler(np.random.RandomState(62), 700), (HEAVY, 300)], dict(visits=[])))
CASES["f_short_level9"] = (9, CASES["f_short"][1])
CASES["f_len33_all4"] = (1, _pattern([4] * 33, 63, tail=123))
CASES["f_level9_3blocks"] = (9, _pattern([4, 3, 4], 64, level=9, tail=60000))
BATCH_L1 = ["f_len20", "f_short", "a_last_e125_tail_200", "f_short", "f_len33_all4"]
BATCH_L9 = ["f_short_level9", "f_level9_3blocks", "f_short_level9"]
SEARCH_ONLY = [n for n in CASES if n[0] in "acd"]       # (g): run again with the table off

_built = {}


def case(name):
    """-> (level, items, aim, blocks), built once; the aim is checked on the model here."""
    if name not in _built:
        level, build = CASES[name]
        items, aim = build()
        blocks = cut(items, level)
        # the chain of chunk starts, as the table sees it: before the rule for a
        # final single byte, which the walk applies to what it has looked up
        es = e_seq(cut(items, level, final_joins=False))
        if "k" in aim:
            k = aim["k"]
            assert es[k] == aim["e"], (name, es)
            assert len(es) == aim.get("nblocks", len(es)), (name, len(es))
            assert (es[k + 1] if k + 1 < len(es) else None) == aim["d"], (name, es)
            if aim["d"] is None:
                assert Offsets(items).wend >= (k + 1) * nblock_max(level)     # the row is read
            if aim["to_end"] is not None:
                assert Offsets(items).row_tiles(k, level)[1] == aim["to_end"], name
        for v in aim.get("visits", ()):
            assert v in es, (name, v, es)
        _built[name] = (level, items, aim, blocks)
    return _built[name]
