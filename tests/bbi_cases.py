"""The bigWig / bigBed files of test_bbi_cpu.py, written with tests/bbi_writer.py.
good(): name -> (kind, file, [regions to try]); bad(): name -> (kind, file): files
whose header and trees are sound and whose blocks are not; malformed(): name -> (file, a word of the reason) for files whose
header or trees are refused.  Built once, on first use."""
import functools
import struct
import zlib

from tests import bbi_writer as W
from tests import deflate_writer as D

CHROMS = [(b"chr1", 1 << 31), (b"chr10", 4000000000), (b"chr2", 3000), (b"chr3", 77), (b"chrX", 5)]   # ids 0..4; names sort chr1 < chr10 < chr2
BIG_UBS = (64 << 20) + 16     # a declared uncompressBufSize far above what any block of sizing_walk holds

# float32 bit patterns: 0, -0.0, 1, 0.1f, 1e-5f, 123456.7f, 1234567f, the least denormal, the greatest finite value, +inf, a NaN
G_BITS = [0x00000000, 0x80000000, 0x3F800000, 0x3DCCCCCD, 0x3727C5AC, 0x47F12059, 0x4996B438, 0x00000001, 0x7F7FFFFF, 0x7F800000,
          0x7FC00000]


def wig_file(sections, chroms=CHROMS, stored=None, **kw):
    blocks = [W.Block(s, W.wig_box(s), stored=stored[k] if stored else None) for k, s in enumerate(sections)]
    return W.write("bigwig", chroms, blocks, **kw)


def bed_file(blocks, chroms=CHROMS, **kw):
    return W.write("bigbed", chroms, [W.Block(W.bed_block(b), W.bed_box(b)) for b in blocks], **kw)


def three_sections():
    """One block of each type: one item; 1024 items; fixedStep whose starts cross 2^31."""
    s2 = W.wig_section(2, [(100, 1.5)], type_=2, span=7)
    s1 = W.wig_section(0, [(10 * k, 10 * k + 3 + k % 5, k * 0.25 - 17) for k in range(1024)], type_=1)
    s3 = W.wig_section(1, [float(k) for k in range(12)], type_=3, chrom_start=(1 << 31) - 20, step=5, span=4)
    return [s2, s1, s3]


def _deflated(payload, how):
    bw = D.BitWriter()
    if how == "stored":
        D.stored_block(bw, payload, True)
    elif how == "fixed":
        D.fixed_block(bw, D.lz_tokens(payload), True)
    else:
        D.dynamic_block(bw, D.lz_tokens(payload), True)
    return W.zlib_frame(bw.getvalue(), payload)


def sized_bed_block(size, k=0):
    """A bigBed block of exactly `size` bytes: one record whose rest pads it."""
    return [(0, 5 + k, 9 + k, bytes(65 + (j * 7 + k) % 26 for j in range(size - 13)))]


def region_file():
    """Four blocks on chr1 ([0, 400), [400, 800), ...) and two on chr2."""
    secs = [W.wig_section(0, [(400 * b + 40 * k, 400 * b + 40 * k + 40, b + k / 16) for k in range(10)], type_=1) for b in range(4)]
    secs += [W.wig_section(2, [(100 * b + 10 * k, 0.5 * k) for k in range(10)], type_=2, span=10) for b in range(2)]
    return wig_file(secs)


REGIONS = [b"chr1", b"chr2", (b"chr1", 450, 700), (b"chr1", 780, 830), (b"chr1", 799, 801), (b"chr2", 95, 96), (b"chr1", 5000, 6000),
           b"chr3", b"chr9", (b"chr10", 0, 10)]


@functools.lru_cache(maxsize=None)
def good():
    secs = three_sections()
    g = {}
    g["three_sections"] = ("bigwig", wig_file(secs), [None])
    for how in ("stored", "fixed", "dynamic"):
        g["deflate_" + how] = ("bigwig", wig_file(secs, stored=[_deflated(s, how) for s in secs]), [None])
    g["exact_ubs"] = ("bigwig", wig_file(secs, ubs=max(len(s) for s in secs)), [None])
    g["uncompressed"] = ("bigwig", wig_file(secs, ubs=0), [None, b"chr10"])
    many = [W.wig_section(k % 5, [(7 * k + j, 7 * k + j + 1, k + j / 4) for j in range(3)], type_=1) for k in range(1100)]
    g["many_blocks"] = ("bigwig", wig_file(many), [None])
    g["sizing_walk"] = ("bigwig", wig_file(secs + secs[:2], ubs=BIG_UBS), [None])
    g["g_values"] = ("bigwig", wig_file([W.wig_section(3, [(k, k + 1, b) for k, b in enumerate(G_BITS)], type_=1)]), [None])
    g["adler_sizes"] = ("bigbed", bed_file([sized_bed_block(n, k) for k, n in enumerate((5551, 5552, 5553, 13))]), [None])
    rests = [b"", b"r" * 63, b"s" * 64, b"t" * 65, b"u" * 1023, b"v" * 1024, b"name\t0\t+", b"w" * 3000]
    g["bed_framing"] = ("bigbed", bed_file([[(0, 0, 0, r) for r in rests], [(0, 0, 7, b"only")],
                                            [(0, 0, 1 + k, rests[k % 4]) for k in range(70)]]), [None])
    g["bed_uncompressed"] = ("bigbed", bed_file([[(0, 0, 0, r) for r in rests], [(1, 3, 3, b"")]], ubs=0), [None])
    five = [W.wig_section(c, [(10 * c + k, 10 * c + k + 2, c + k / 8) for k in range(4)], type_=1) for c in range(5) for _ in range(2)]
    g["deep_trees"] = ("bigwig", wig_file(five, chrom_block=2, index_block=2), [None, b"chr2", b"chr10"])
    g["regions"] = ("bigwig", region_file(), REGIONS)
    ties = [[(0, 100, 900 - k, b"n%d" % k) for k in range(40)], [(0, 100, 50 + 400 - k, b"m%d" % k) for k in range(300)],
            [(2, 5, 5, b""), (2, 5, 6, b"x")]]
    g["bed_ties"] = ("bigbed", bed_file(ties), [None, (b"chr1", 850, 900), b"chr2"])
    return g


def _flip_adler(data, which=0):
    """The file with one bit flipped in the Adler-32 trailer of block `which`."""
    from tests import bbi_oracle
    _, off, size = bbi_oracle.read(data)["blocks"][which]
    b = bytearray(data)
    b[off + size - 1] ^= 4
    return bytes(b)


@functools.lru_cache(maxsize=None)
def bad():
    """name -> (kind, file): the header and the trees are sound, a block is not (the comment says how)."""
    ok = W.wig_section(0, [(1, 2, 1.0), (5, 9, 2.0)], type_=1)
    b = {}
    # block 1 announces two items and holds one
    b["section_size"] = ("bigwig", wig_file([ok, W.wig_section(0, [(1, 2, 1.0)], type_=1, count=2)]))
    b["type4"] = ("bigwig", wig_file([W.wig_section(0, [1.0], type_=4, span=1)]))
    # block 2 names chromId 5 of five chromosomes
    b["chrom_range"] = ("bigwig", wig_file([ok, ok, W.wig_section(5, [(1, 2, 1.0)], type_=1)]))
    # the second item of the second block has start == end (the fourth record of the file)
    b["start_end"] = ("bigwig", wig_file([ok, W.wig_section(0, [(1, 2, 1.0), (9, 9, 2.0), (3, 1, 0.0)], type_=1)]))
    # block 1 inflates to one byte more than uncompressBufSize
    big = W.wig_section(0, [(k, k + 1, 0.5) for k in range(100)], type_=1)
    b["past_slot"] = ("bigwig", wig_file([ok, big], ubs=len(big) - 1))
    # zlib framing: FDICT set; a header whose check fails; a byte between the deflate data and the trailer
    fdict = W.zlib_frame(D.raw_deflate(ok), ok, flg=0x20 + (31 - (0x78 * 256 + 0x20) % 31) % 31)
    b["fdict"] = ("bigwig", wig_file([ok, ok], stored=[None, fdict]))
    b["zlib_header"] = ("bigwig", wig_file([ok], stored=[W.zlib_frame(D.raw_deflate(ok), ok, flg=0)]))
    b["extent"] = ("bigwig", wig_file([ok], stored=[W.zlib_frame(D.raw_deflate(ok) + b"\0", ok)]))
    # Adler-32: one bit of the trailer flipped, over 5,552 bytes and over 65,536 bytes of 0xff
    b["adler_flip"] = ("bigbed", _flip_adler(bed_file([sized_bed_block(5552)])))
    ff = W.Block(b"\xff" * 65536, (0, 0, 0, 1))
    b["adler_ff_flip"] = ("bigbed", _flip_adler(W.write("bigbed", CHROMS, [ff])))
    # right Adler-32, no chain of bigBed records: one byte; no zero byte at all; a last byte that is not zero
    b["adler_one_byte"] = ("bigbed", W.write("bigbed", CHROMS, [W.Block(b"\x07", (0, 0, 0, 1))]))
    b["adler_ff"] = ("bigbed", W.write("bigbed", CHROMS, [ff]))
    recs = [(0, 1, 2, b"a"), (0, 3, 4, b"bc")]
    b["last_not_zero"] = ("bigbed", W.write("bigbed", CHROMS, [W.Block(W.bed_block(recs), W.bed_box(recs)),
                                                              W.Block(W.bed_block(recs, last_zero=False), W.bed_box(recs))]))
    b["bed_newline"] = ("bigbed", bed_file([recs, [(0, 5, 6, b"x\ny")]]))
    b["bed_order"] = ("bigbed", bed_file([[(0, 5, 4, b"")]]))       # start above end
    return b


def node_chain(nodes=12000):
    """A file whose R-tree is a chain of overlapping inner nodes: node k, 28 bytes after node k - 1, claims
    as many 24-byte items as reach the end of the file, and only its first item's child (the next node) is
    an offset inside the file.  A walk that pushes a node's children before it checks them grows by that
    many entries per node; the nodes together claim far more bytes than the file has."""
    cto, fio = 64, 96
    size = fio + 48 + 28 * nodes
    head = struct.pack("<IHHQQQHHQQIQ", W.BIGWIG, 4, 0, cto, fio, fio, 0, 0, 0, 0, 0, 0)
    ctree = struct.pack("<IIIIQQ", 0x78CA8C91, 1, 4, 8, 0, 0)                      # no chromosomes: not walked
    rhead = struct.pack("<IIQIIIIQII", 0x2468ACE0, 1, 1, 0, 0, 0, 0, fio, 1, 0)
    body = bytearray()
    for k in range(nodes):
        off = fio + 48 + 28 * k
        body += struct.pack("<BBH", 0, 0, min(65535, (size - off - 4) // 24)) + bytes(16) + struct.pack("<Q", off + 28)
    return head + ctree + rhead + bytes(body)


@functools.lru_cache(maxsize=None)
def malformed():
    """name -> (file, a word of the reason): files that starch_bbi_info refuses."""
    secs = three_sections()
    good_file = wig_file(secs)
    m = {}
    m["bad_magic"] = (wig_file(secs, magic=0x12345678), "bad magic")
    m["swapped_magic"] = (wig_file(secs, swap_magic=True), "big-endian bigWig/bigBed is not supported")
    m["truncated_header"] = (good_file[:40], "truncated")
    m["truncated_tree"] = (good_file[:len(good_file) - 20], "past the end")
    m["offset_past_end"] = (wig_file(secs, full_index_offset=1 << 40), "past the end")
    m["chrom_offset_past_end"] = (wig_file(secs, chrom_tree_offset=len(good_file) - 8), "past the end")
    m["chrom_item_count"] = (wig_file(secs, chrom_item_count=1 << 40), "more than the file can hold")
    m["index_item_count"] = (wig_file(secs, index_item_count=1 << 40), "more than the file can hold")
    m["index_item_count_off"] = (wig_file(secs, index_item_count=2), "itemCount")
    m["chrom_twice"] = (wig_file(secs, chrom_ids=[0, 1, 1, 3, 4]), "appears twice")
    m["chrom_missing"] = (wig_file(secs, chrom_ids=[0, 1, 2, 3, 4], chrom_item_count=6), "is missing")
    m["chrom_id_range"] = (wig_file(secs, chrom_ids=[0, 1, 2, 3, 9]), "not below itemCount")
    m["self_child"] = (wig_file(secs, index_block=2, self_child=True), "reached twice")
    m["overlap"] = (wig_file(secs, data_offset_shift=(1, -3)), "overlap")
    m["outside_data"] = (wig_file(secs, data_offset_shift=(0, -30)), "lies outside")
    m["bad_name"] = (wig_file(secs, chroms=[(b"a\tb", 5)] + CHROMS[1:]), "TAB or a newline")
    m["node_chain"] = (node_chain(), "nodes overlap")
    return m
