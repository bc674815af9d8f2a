"""An independent pure-Python bigWig / bigBed reader and formatter (TEST
INFRASTRUCTURE ONLY): the reference that readings of such files are compared with.
It follows the definition in include/starch_amd.h, takes nothing from the code
under test and shares nothing with tests/bbi_writer.py beyond ``struct``.
Values print as Python's ``'%g' % struct.unpack('<f', ...)[0]``."""
import struct
import zlib


class Malformed(Exception):
    pass


def _u(fmt, data, off):
    size = struct.calcsize(fmt)
    if off < 0 or off + size > len(data):
        raise Malformed("read past the end at %d" % off)
    return struct.unpack_from(fmt, data, off)


def _walk(data, root, leaf_size, inner_size):
    """(offset, is_leaf, count) of every node, each once; children in order."""
    stack, seen, claimed = [root], set(), 0
    while stack:
        off = stack.pop()
        if off in seen:
            raise Malformed("node reached twice")
        seen.add(off)
        is_leaf, _, count = _u("<BBH", data, off)
        size = leaf_size if is_leaf else inner_size
        if off + 4 + count * size > len(data):
            raise Malformed("node past the end")
        claimed += 4 + count * size                  # nodes are disjoint pieces of the file
        if claimed > len(data):
            raise Malformed("nodes overlap")
        yield off + 4, bool(is_leaf), count
        if not is_leaf:
            kids = [_u("<Q", data, off + 4 + k * size + size - 8)[0] for k in range(count)]
            stack.extend(reversed(kids))


def read(data):
    """dict: kind, version, ubs, chroms [(name, size)] by id, blocks [(box, offset, size)] by offset."""
    magic, = _u("<I", data, 0)
    kind = {0x888FFC26: "bigwig", 0x8789F2EB: "bigbed"}.get(magic)
    if kind is None:
        raise Malformed("bad magic")
    version, zooms, cto, fdo, fio, fc, dfc, asql, tso, ubs, _ = _u("<HHQQQHHQQIQ", data, 4)
    cmagic, cblock, key, val, n_chrom, _ = _u("<IIIIQQ", data, cto)
    if cmagic != 0x78CA8C91 or val != 8:
        raise Malformed("chromosome tree header")
    if n_chrom * (key + 8) > len(data):
        raise Malformed("chromosome itemCount")
    chroms = {}
    if n_chrom:
        for at, leaf, count in _walk(data, cto + 32, key + 8, key + 8):
            if not leaf:
                continue
            for k in range(count):
                o = at + k * (key + 8)
                name = data[o:o + key].split(b"\0")[0]
                cid, size = _u("<II", data, o + key)
                if cid in chroms or cid >= n_chrom or not name or b"\t" in name or b"\n" in name:
                    raise Malformed("chromosome item")
                chroms[cid] = (name, size)
    if sorted(chroms) != list(range(n_chrom)):
        raise Malformed("chromosome ids")
    rmagic, rblock, n_items = _u("<IIQ", data, fio)
    _u("<IIIIQII", data, fio + 16)
    if rmagic != 0x2468ACE0 or n_items * 32 > len(data) or fdo > fio:
        raise Malformed("R-tree header")
    blocks = []
    if n_items:
        for at, leaf, count in _walk(data, fio + 48, 32, 24):
            if leaf:
                for k in range(count):
                    v = _u("<IIIIQQ", data, at + 32 * k)
                    blocks.append((v[:4], v[4], v[5]))
    if len(blocks) != n_items:
        raise Malformed("R-tree itemCount")
    blocks.sort(key=lambda b: b[1])
    for k, (box, off, size) in enumerate(blocks):
        if off < fdo or off + size > fio or (k and blocks[k - 1][1] + blocks[k - 1][2] > off):
            raise Malformed("block placement")
    return dict(kind=kind, version=version, ubs=ubs, chroms=[chroms[k] for k in range(n_chrom)], blocks=blocks, zooms=zooms,
                cto=cto, fdo=fdo, fio=fio, field_count=fc, defined_field_count=dfc)


def selected(info, region):
    """Indices of the blocks whose box meets region: None, a name, or (name, start, end)."""
    if region is None:
        return list(range(len(info["blocks"])))
    name = region if isinstance(region, bytes) else region[0]
    ids = [k for k, (n, _) in enumerate(info["chroms"]) if n == name]
    if not ids:
        return []
    lo = (ids[0], 0 if isinstance(region, bytes) else region[1])
    hi = (ids[0], 1 << 32 if isinstance(region, bytes) else region[2])
    return [k for k, (box, _, _) in enumerate(info["blocks"]) if (box[0], box[1]) < hi and (box[2], box[3]) > lo]


def payload(data, info, k):
    _, off, size = info["blocks"][k]
    raw = data[off:off + size]
    if not info["ubs"]:
        return raw
    out = zlib.decompress(raw)
    if len(out) > info["ubs"]:
        raise Malformed("block inflates past uncompressBufSize")
    return out


def records(data, info, k):
    """(chrom id, start, end, tail) of block k: tail is the float's four bytes (bigWig) or the rest (bigBed)."""
    p = payload(data, info, k)
    out = []
    if info["kind"] == "bigwig":
        cid, cs, ce, step, span, type_, _, n = struct.unpack_from("<IIIIIBBH", p)
        if type_ not in (1, 2, 3) or len(p) != 24 + n * {1: 12, 2: 8, 3: 4}[type_] or cid >= len(info["chroms"]):
            raise Malformed("section")
        for i in range(n):
            if type_ == 1:
                s, e = struct.unpack_from("<II", p, 24 + 12 * i)
                v = p[24 + 12 * i + 8:24 + 12 * i + 12]
            elif type_ == 2:
                s, = struct.unpack_from("<I", p, 24 + 8 * i)
                e, v = s + span, p[24 + 8 * i + 4:24 + 8 * i + 8]
            else:
                s = cs + i * step
                e, v = s + span, p[24 + 4 * i:28 + 4 * i]
            if s >= e:
                raise Malformed("start >= end")
            out.append((cid, s, e, v))
        return out
    at = 0
    while at < len(p):
        if len(p) - at < 13:
            raise Malformed("chain")
        cid, s, e = struct.unpack_from("<III", p, at)
        z = p.find(b"\0", at + 12)
        if z < 0:
            raise Malformed("chain")
        rest = p[at + 12:z]
        if cid >= len(info["chroms"]) or s > e or b"\n" in rest:
            raise Malformed("record")
        out.append((cid, s, e, rest))
        at = z + 1
    return out


def value_text(four):
    return ("%g" % struct.unpack("<f", four)[0]).encode()


def expected(data, region=None, bedgraph=False):
    """The unsorted output, and the number of blocks decoded."""
    info = read(data)
    sel = selected(info, region)
    lines, n = [], 0
    for k in sel:
        for cid, s, e, tail in records(data, info, k):
            name = info["chroms"][cid][0]
            if region is not None:
                rn = region if isinstance(region, bytes) else region[0]
                if name != rn or (not isinstance(region, bytes) and not (s < region[2] and e > region[1])):
                    continue
            n += 1
            if info["kind"] == "bigwig":
                mid = b"" if bedgraph else b"id-%d\t" % n
                lines.append(b"%s\t%d\t%d\t%s%s\n" % (name, s, e, mid, value_text(tail)))
            else:
                lines.append(b"%s\t%d\t%d%s\n" % (name, s, e, b"\t" + tail if tail else b""))
    return b"".join(lines), len(sel)


def sort_bed(text):
    """sort-bed's order: chromosome bytes, start, stop; equal keys in input order."""
    def key(line):
        f = line.split(b"\t", 3)
        return (f[0], int(f[1]), int(f[2]))
    return b"".join(l + b"\n" for l in sorted(text.split(b"\n")[:-1], key=key))
