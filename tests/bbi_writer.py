"""A permissive bigWig / bigBed writer (TEST INFRASTRUCTURE ONLY).

Plain Python that writes what it is told, valid or not: any section type, any
blockSize for the chromosome B+ tree and the R-tree (so trees of several levels
are cheap to make), blocks compressed with zlib at any level, left uncompressed,
or wrapped around a raw deflate payload of tests/deflate_writer.py, and wrong
fields on request.  tests/bbi_oracle.py is the matching reader; the two share
nothing but ``struct``."""
import struct
import zlib

BIGWIG, BIGBED = 0x888FFC26, 0x8789F2EB


def wig_section(chrom_id, items, type_=1, chrom_start=None, chrom_end=None, step=0, span=0, count=None):
    """A bigWig block.  items: (start, end, value) for type 1, (start, value) for
    type 2, value for type 3 (and any other type); a value is a float or, as an
    int, the 32 bits of one.  count: the itemCount written (default: len(items))."""
    def f32(v):
        return struct.pack("<I", v) if isinstance(v, int) else struct.pack("<f", v)
    body = b""
    for it in items:
        if type_ == 1:
            body += struct.pack("<II", it[0], it[1]) + f32(it[2])
        elif type_ == 2:
            body += struct.pack("<I", it[0]) + f32(it[1])
        else:
            body += f32(it)
    if chrom_start is None:
        chrom_start = items[0][0] if items and type_ in (1, 2) else 0
    if chrom_end is None:
        chrom_end = chrom_start + 1
    n = len(items) if count is None else count
    return struct.pack("<IIIIIBBH", chrom_id, chrom_start, chrom_end, step, span, type_, 0, n) + body


def bed_block(records, last_zero=True):
    """A bigBed block of (chrom_id, start, end, rest) records."""
    out = b"".join(struct.pack("<III", c, s, e) + rest + b"\0" for c, s, e, rest in records)
    return out if last_zero else out[:-1] + b"x"


def zlib_frame(raw, text, cmf=0x78, flg=None, adler=None):
    """A zlib stream around raw deflate bytes (of deflate_writer); flg defaults
    to the value that makes the header check right, adler to that of text."""
    if flg is None:
        flg = (31 - (cmf * 256) % 31) % 31
    a = zlib.adler32(text) & 0xFFFFFFFF if adler is None else adler
    return bytes([cmf, flg]) + raw + struct.pack(">I", a)


class Block:
    """One data block: payload (the inflated bytes) and how it is stored: level
    (zlib.compress), or stored: the very bytes of the file for it.  box: the
    R-tree's (startChromIx, startBase, endChromIx, endBase)."""

    def __init__(self, payload, box, level=6, stored=None):
        self.payload, self.box, self.level, self.stored = payload, box, level, stored


def _tree(items, block_size, leaf_fmt, inner_fmt, base):
    """Nodes of a tree over the packed leaf items, block_size per node, level
    after level from the root at offset `base`.  items: (key fields, leaf
    bytes); inner_fmt(first item's key fields, last's, child offset).  Returns
    the bytes."""
    levels = [[(k, leaf) for k, leaf in items]]          # level 0: leaf items
    groups = [levels[0][i:i + block_size] for i in range(0, len(items), block_size)] or [[]]
    node_levels = [groups]
    while len(node_levels[-1]) > 1:
        prev = node_levels[-1]
        node_levels.append([list(range(i, min(i + block_size, len(prev)))) for i in range(0, len(prev), block_size)])
    node_levels.reverse()                                 # root first
    # sizes, to place every node
    def node_size(depth, node):
        leaf = depth == len(node_levels) - 1
        return 4 + sum(len(it[1]) for it in node) if leaf else 4 + len(node) * inner_fmt(None, None, 0, size_only=True)
    offs, at = [], base
    for d, lvl in enumerate(node_levels):
        offs.append([])
        for node in lvl:
            offs[d].append(at)
            at += node_size(d, node)
    def span(depth, idx):
        """first and last leaf item under node idx of level depth"""
        node = node_levels[depth][idx]
        if depth == len(node_levels) - 1:
            return node[0][0], node[-1][0]
        return span(depth + 1, node[0])[0], span(depth + 1, node[-1])[1]
    out = b""
    for d, lvl in enumerate(node_levels):
        leaf = d == len(node_levels) - 1
        for node in lvl:
            out += struct.pack("<BBH", 1 if leaf else 0, 0, len(node))
            if leaf:
                out += b"".join(it[1] for it in node)
            else:
                for child in node:
                    first, last = span(d + 1, child)
                    out += inner_fmt(first, last, offs[d + 1][child])
    return out


def write(kind, chroms, blocks, ubs=None, chrom_block=256, index_block=256, version=4, zoom_levels=0, magic=None,
          swap_magic=False, key_size=None, chrom_ids=None, chrom_item_count=None, index_item_count=None, self_child=False,
          data_offset_shift=None, chrom_tree_offset=None, full_index_offset=None, pad_between=0):
    """The file.  chroms: [(name, size)], ids in order (chrom_ids: the ids
    written instead).  blocks: Block list in file order.  ubs: the
    uncompressBufSize written (default: the largest payload, 0 when no block is
    compressed: then every block is written as its payload).  The other
    arguments write wrong fields: an item count, the magic byte-swapped, an
    R-tree root whose first child is itself, a (index, delta) shift of one
    block's dataOffset in the index, header offsets past the end."""
    compressed = ubs != 0
    if ubs is None:
        ubs = max([len(b.payload) for b in blocks] + [1])
    key_size = key_size or max([len(n) for n, _ in chroms] + [1])
    ids = list(range(len(chroms))) if chrom_ids is None else chrom_ids
    by_name = sorted(range(len(chroms)), key=lambda k: chroms[k][0])
    citems = [((chroms[k][0],), chroms[k][0].ljust(key_size, b"\0") + struct.pack("<II", ids[k], chroms[k][1])) for k in by_name]

    def cinner(first, last, child, size_only=False):
        if size_only:
            return key_size + 8
        return first[0].ljust(key_size, b"\0") + struct.pack("<Q", child)
    cto = 64 + 24 * zoom_levels
    ctree = struct.pack("<IIIIQQ", 0x78CA8C91, chrom_block, key_size, 8, len(chroms) if chrom_item_count is None else chrom_item_count, 0)
    ctree += _tree(citems, chrom_block, None, cinner, cto + 32)
    fdo = cto + len(ctree)
    data, places, at = struct.pack("<Q", len(blocks)), [], fdo + 8
    for b in blocks:
        raw = b.stored if b.stored is not None else (zlib.compress(b.payload, b.level) if compressed else b.payload)
        data += b"\0" * pad_between
        at += pad_between
        places.append((at, len(raw)))
        data += raw
        at += len(raw)
    fio = fdo + len(data)
    if data_offset_shift:
        k, delta = data_offset_shift
        places[k] = (places[k][0] + delta, places[k][1])
    ritems = [(b.box, struct.pack("<IIIIQQ", *b.box, *places[k])) for k, b in enumerate(blocks)]

    def rinner(first, last, child, size_only=False):
        if size_only:
            return 24
        return struct.pack("<IIIIQ", first[0], first[1], last[2], last[3], child)
    first = blocks[0].box if blocks else (0, 0, 0, 0)
    last = blocks[-1].box if blocks else (0, 0, 0, 0)
    rtree = struct.pack("<IIQIIIIQII", 0x2468ACE0, index_block, len(blocks) if index_item_count is None else index_item_count,
                        first[0], first[1], last[2], last[3], fio, 1, 0)
    nodes = _tree(ritems, index_block, None, rinner, fio + 48)
    if self_child:
        assert nodes[0] == 0, "self_child needs an inner root (more blocks than index_block)"
        nodes = nodes[:4 + 16] + struct.pack("<Q", fio + 48) + nodes[4 + 24:]
    rtree += nodes
    m = (BIGWIG if kind == "bigwig" else BIGBED) if magic is None else magic
    head = struct.pack(">I" if swap_magic else "<I", m)
    head += struct.pack("<HHQQQHHQQIQ", version, zoom_levels, cto if chrom_tree_offset is None else chrom_tree_offset, fdo,
                        fio if full_index_offset is None else full_index_offset, 3 if kind == "bigbed" else 0,
                        3 if kind == "bigbed" else 0, 0, 0, ubs if compressed else 0, 0)
    assert len(head) == 64
    return head + b"\0" * (24 * zoom_levels) + ctree + data + rtree


def wig_box(section):
    """The R-tree box of a bigWig section written by wig_section (of the items that are there, whatever itemCount says)."""
    cid, cs, ce, step, span, type_, _, n = struct.unpack_from("<IIIIIBBH", section)
    n = min(n, (len(section) - 24) // {1: 12, 2: 8}.get(type_, 4))
    if type_ == 1 and n:
        starts = [struct.unpack_from("<I", section, 24 + 12 * k)[0] for k in range(n)]
        ends = [struct.unpack_from("<I", section, 28 + 12 * k)[0] for k in range(n)]
        return (cid, min(starts), cid, min(max(ends), 0xFFFFFFFF))
    if type_ == 2 and n:
        starts = [struct.unpack_from("<I", section, 24 + 8 * k)[0] for k in range(n)]
        return (cid, min(starts), cid, min(max(starts) + span, 0xFFFFFFFF))
    return (cid, cs, cid, min(cs + max(n - 1, 0) * step + span, 0xFFFFFFFF))


def bed_box(records):
    """The box of a bigBed block whose records are ordered by chromosome."""
    c0, c1 = records[0][0], records[-1][0]
    return (c0, min(r[1] for r in records if r[0] == c0), c1, max(r[2] for r in records if r[0] == c1))
