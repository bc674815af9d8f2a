"""bzip2 streams that libbz2's encoder never writes but its decoder accepts,
built with tests/bz2_writer.py.  test_bz2_writer.py pins every one of them on
the CPU against the system libbz2 (Python's bz2); test_gpu_decode_foreign.py
then holds the GPU decoder to the same bytes.

group(name) -> [Case], built once per process.  A Case names the decoder path
it is there to reach.  Only the cases in CONDITIONAL depend on the installed
libbz2 (accepted() asks it at run time); every other case is unconditional.
"""
import bz2
import functools
import random

from tests.bz2_writer import Block, count_byte_positions, flat_lengths, rle1, stair_lengths, write_stream

# libbz2 before 1.0.8 refuses more than 18002 selectors; 1.0.8 reads and drops the extra ones
CONDITIONAL = frozenset({"nsel_18102"})

kWalkT = 1024               # k_dec_walk's workgroup: at most kWalkT - 1 sampled nodes besides the start node


class Case:
    def __init__(self, name, stream, **meta):
        self.name, self.stream, self.meta = name, stream, meta

    @property
    def conditional(self):
        return self.name in CONDITIONAL


def accepted(case) -> bool:
    """Does the installed libbz2 decode the case to the intended bytes?"""
    try:
        return bz2.decompress(case.stream.data) == case.stream.out
    except (OSError, ValueError):
        return False


def walk_spacing(n: int) -> int:
    """k_dec_walk's sample spacing G: the smallest power of two with G * (kWalkT - 1) >= n."""
    G = 1
    while G * (kWalkT - 1) < n:
        G <<= 1
    return G


def norun(rng, n, alphabet):
    """n bytes from alphabet without four equal bytes in a row: RLE1 leaves them as they are."""
    out = bytearray()
    while len(out) < n:
        b = rng.choice(alphabet)
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == b:
            continue
        out.append(b)
    return bytes(out)


def _one(name, block, level=9, **meta):
    return Case(name, write_stream([block], level), **meta)


# ---------------------------------------------------------------------------
def _lengths():
    rng = random.Random(101)
    d8 = norun(rng, 600, b"abcdefgh")
    d19 = norun(rng, 600, bytes(range(40, 59)))          # nin 19: alpha 21, a staircase up to 20 bits
    d40 = norun(rng, 600, bytes(range(60, 100)))
    out = [
        # every symbol by the limit/base/perm search at the longest length; fast[] all 0
        _one("all_20_bits", Block(data=d8, tables=lambda a: [[20] * a] * 2)),
        # complete code 1..20,20: lengths <= 10 from the lookup table, 11..20 by search
        _one("stair_1_to_20", Block(data=d19, tables=lambda a: [stair_lengths(a)] * 2)),
        # incomplete, lengths 9..12 interleaved: neighbours in and out of the table
        _one("straddle_9_to_12", Block(data=d40, tables=lambda a: [[9 + i % 4 for i in range(a)]] * 2)),
        # one table complete, one incomplete, alternating every 50 symbols
        _one("complete_and_incomplete", Block(data=d19, tables=lambda a: [stair_lengths(a), flat_lengths(a, 1)])),
        # Kraft sum above 1 (usefast = 0): only RUNA, RUNB and EOB are coded and their codes fit
        _one("oversubscribed_runa", Block(raw=b"aaa", extra_map=b"bc", tables=[[2, 2, 2, 2, 1]] * 2)),
        _one("oversubscribed_runb", Block(raw=b"aa", extra_map=b"bc", tables=[[2, 2, 2, 2, 1]] * 2)),
    ]
    return out


def _tables():
    rng = random.Random(102)
    d = norun(rng, 400, b"abcdefgh")
    out = []
    for nt in (2, 3, 6):
        out.append(_one("tables_%d" % nt, Block(data=d, tables=lambda a, nt=nt: [flat_lengths(a, k) for k in range(nt)]),
                        all_tables_used=nt))
    out.append(_one("table_unused", Block(data=d, tables=lambda a: [flat_lengths(a, k) for k in range(3)],
                                          selectors=lambda need, nt: [(0, 2)[g & 1] for g in range(need)])))
    out.append(_one("tables_6_on_30_symbols", Block(data=norun(rng, 26, b"abcdefgh"),
                                                    tables=lambda a: [flat_lengths(a, k) for k in range(6)],
                                                    selectors=[5]), max_symbols=30))
    out.append(_one("selectors_100_unused", Block(data=d, extra_selectors=100)))
    need = len(write_stream([d]).blocks[0].selectors)
    out.append(_one("nsel_18102", Block(data=d, extra_selectors=18102 - need), nsel=18102))
    return out


def _alphabet():
    rng = random.Random(103)
    out = []
    for nin in (1, 2, 15, 16, 17, 255, 256):
        syms = bytes(rng.sample(range(256), nin)) if nin < 256 else bytes(range(256))
        body = bytearray(syms * 3)
        rng.shuffle(body)
        out.append(_one("nin_%d_all_present" % nin, Block(data=bytes(body)), nin=nin))
        if nin > 1:
            one = bytes([sorted(syms)[nin // 2]])
            out.append(_one("nin_%d_one_present" % nin, Block(raw=one * 3, extra_map=syms), nin=nin))
    # a run of the front symbol as the first thing in the block, and as the last before EOB,
    # with the nibble list (nin <= 16) and with the LDS list
    # The first symbol coded can be a run only in a block of one repeated byte,
    # the smallest declared: the last column starts with the byte before the
    # smallest rotation, and were that the smallest byte, the rotation starting
    # there would be smaller still.
    for tag, alphabet in (("nibble", b"abcd"), ("list", bytes(range(100, 120)))):
        out.append(_one("front_run_first_" + tag, Block(raw=alphabet[:1] * 3, extra_map=alphabet)))
        for _ in range(1000):
            last = _one("front_run_last_" + tag, Block(data=norun(rng, 60, alphabet)))
            if last.stream.blocks[0].syms[-2] <= 1:
                break
        out.append(last)
    return out


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1022, 1023, 1024, 1025, 2046, 2047, 2048)


def _sizes():
    rng = random.Random(104)
    alphabet = bytes(range(65, 85))
    out = []
    for n in SIZES:
        G = walk_spacing(n)
        if G == 1:                                      # every node is a sample
            out.append(_one("n_%d" % n, Block(data=norun(rng, n, alphabet)), n=n, G=G))
            continue
        on = off = None                                 # the walk's start node on a sample, and off
        for _ in range(200):
            if on is not None and off is not None:
                break
            c = _one("", Block(data=norun(rng, n, alphabet)), n=n, G=G)
            if c.stream.blocks[0].start % G == 0:
                on = on or c
            else:
                off = off or c
        on.name, off.name = "n_%d_start_on_sample" % n, "n_%d_start_off_sample" % n
        on.meta["on_sample"], off.meta["on_sample"] = True, False
        out += [on, off]
    return out


def _periodic():
    out = [
        _one("one_byte_period_5", Block(data=b"a" * (255 * 4)), period=5),            # aaaa\xfb x 4
        _one("period_1", Block(raw=b"aaa"), period=1),                                 # a cycle of 1, n = 3
        _one("period_2", Block(data=b"ab" * 37), period=2),
        _one("period_3", Block(data=b"abc" * 35), period=3),
        # the same with sampled nodes more than one apart (n > 1023)
        _one("period_2_sampled", Block(data=b"ab" * 700), period=2),
        _one("period_3_sampled", Block(data=b"abc" * 500), period=3),
        _one("one_byte_period_5_sampled", Block(data=b"a" * (255 * 300)), period=5),
    ]
    return out


def _align():
    """One stream whose blocks start at every bit alignment, steered by unused selectors."""
    rng = random.Random(105)
    datas = [norun(rng, 90 + 7 * k, b"abcdefgh") for k in range(8)]
    extra = []                                          # block 0 starts at bit 32; block k + 1 is to start at k + 1 mod 8
    for k in range(7):
        for e in range(16):
            s = write_stream([Block(data=d, extra_selectors=x) for d, x in zip(datas, extra + [e, 0])])
            if s.blocks[k + 1].bit % 8 == k + 1:
                break
        else:
            raise AssertionError("no selector padding puts block %d at alignment %d" % (k + 1, k + 1))
        extra.append(e)
    s = write_stream([Block(data=d, extra_selectors=x) for d, x in zip(datas, extra + [0])])
    return [Case("blocks_at_every_bit_alignment", s)]


RUNS = (3, 4, 5, 255, 256, 259, 260)


def _rle1():
    rng = random.Random(106)
    out = []
    for r in RUNS:
        f1, f2 = norun(rng, 40, b"bcdefg"), norun(rng, 40, b"bcdefg")
        out.append(_one("run_%d_start" % r, Block(data=b"a" * r + f1)))
        out.append(_one("run_%d_middle" % r, Block(data=f1 + b"a" * r + f2)))
        out.append(_one("run_%d_end" % r, Block(data=f1 + b"a" * r)))
    for c in (0, 251, 252, 255):                        # libbz2's encoder stops at 251
        out.append(_one("count_%d_middle" % c, Block(raw=b"xaaaa" + bytes([c]) + b"y"), count=c))
        out.append(_one("count_%d_end" % c, Block(raw=b"xyaaaa" + bytes([c])), count=c))
    return out


CKPT_N = range(1, 201)


def checkpoint_raw(n: int, r: int) -> bytes:
    """n post-RLE1 bytes, run-heavy: r single bytes, then groups of four equal
    bytes and a count, so the count bytes sit at 4 + r, 9 + r, ...  Over
    r = 0..4 every position from 4 on is a count byte once."""
    raw = bytearray(b"wxyz"[:r])
    k = 0
    while len(raw) < n:
        raw += bytes([97 + k % 3]) * 4 + bytes([(0, 1, 3, 251, 17)[k % 5]])
        k += 1
    raw = raw[:n]
    if count_byte_positions(bytes(raw) + b"\0")[-1:] == [n]:
        raw[-1] = 48                                    # four equal bytes must not end the block: libbz2 wants the count
    return bytes(raw)


def _checkpoints():
    return [_one("ckpt_n%d_r%d" % (n, r), Block(raw=checkpoint_raw(n, r)), n=n, r=r) for n in CKPT_N for r in range(5)]


def _largest():
    rng = random.Random(107)
    big = norun(rng, 100000, bytes(range(256)))
    assert rle1(big) == big
    return [
        Case("level_1_block_of_100000", write_stream([big], level=1), nblock=100000),
        Case("level_1_cut_in_two", write_stream([big[:50000], big[50000:]], level=1)),
    ]


def _refused():
    """Header-level faults that libbz2 and the GPU decoder both refuse before they decode any data."""
    rng = random.Random(108)
    d = norun(rng, 300, b"abcdefgh")
    a = len(set(d)) + 2
    up = [flat_lengths(a), flat_lengths(a)]
    lo = [list(t) for t in up]
    hi = [list(t) for t in up]
    lo[1] = [1, 0] + [1] * (a - 2)                      # 1, then a step down to 0
    hi[1] = [20, 21] + [20] * (a - 2)                   # 20, then a step up to 21
    n = len(rle1(d))
    return [
        # libbz2 still undoes the randomisation of bzip2 < 0.9.5 (it first alters byte 618 of a
        # block), so it refuses this block, which was never randomised, by its CRC
        _one("randomised", Block(data=norun(rng, 700, b"abcdefgh"), rand=1)),
        _one("tables_1", Block(data=d, n_tables_field=1)),
        _one("tables_7", Block(data=d, n_tables_field=7)),
        _one("nsel_0", Block(data=d, n_sel_field=0)),
        _one("length_0", Block(data=d, header_tables=lo)),
        _one("length_21", Block(data=d, header_tables=hi)),
        _one("empty_map", Block(data=d, empty_map=True)),
        _one("origptr_nblock", Block(data=d, orig_ptr=n)),
    ]


_GROUPS = {
    "lengths": _lengths, "tables": _tables, "alphabet": _alphabet, "sizes": _sizes, "periodic": _periodic,
    "align": _align, "rle1": _rle1, "checkpoints": _checkpoints, "largest": _largest,
}
GROUPS = tuple(_GROUPS)


@functools.lru_cache(maxsize=None)
def group(name):
    cases = _GROUPS[name]()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def refused():
    return tuple(_refused())
