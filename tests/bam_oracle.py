"""A plain-Python BAM writer, BGZF framer and BAM reader for the tests of bam2bed
(the definition: include/starch_amd.h, "bam2bed: BAM records to BED").  struct and
zlib only; numpy supplies the float32 whose %g an f value prints.

  pack_record(rec), bam(text, refs, records)   write inflated BAM from dicts
  bgzf(data, cuts=...)                         BGZF with blocks cut where the test wants them
  sam_text(bam_bytes)                          the SAM text of inflated BAM, what samtools view -h prints
  expected(bam_bytes, **options)               the unsorted BED: tests.align_oracle.sam on that text
  random_bam(rng, records)                     a BAM of random records and the list of their dicts

TABLE holds hand-written records with the SAM line of each written out by hand."""
import struct
import zlib

import numpy

from tests import align_oracle

# what is wrong with a record, in the library's words (bed_bam.hip: bad_text)
E_SHORT = "block_size below 32"
E_PAST = "the record runs past the end of the input"
E_COUNTS = "block_size is below what l_read_name, n_cigar_op and l_seq announce"
E_NAME = "the read name is empty or does not end in NUL"
E_REF = "refID or next_refID is not -1 or a reference of the header"
E_CIGAR = "CIGAR operator above 8"
E_TAGTYPE = "unknown tag type"
E_TAGS = "the tags do not parse exactly to the end of the record"
E_RNAME = align_oracle.E_RNAME
E_ZERO = align_oracle.E_ZERO

OPS = b"MIDNSHP=X"
BASES = b"=ACMGRSVTWYHKDBN"
SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
FORMATS = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- writing ------------------------------------------------------------------------------
def pack_tag(tag, typ, value):
    """One tag; typ is a BAM type, or "B" with value = (subtype, values); a float may be given as its 32 bits in an int."""
    head = tag + typ.encode()
    if typ == "A":
        return head + value
    if typ in ("Z", "H"):
        return head + value + b"\0"
    if typ == "B":
        sub, values = value
        if sub == "f" and len(values) and isinstance(values[0], (int, numpy.integer)):
            body = numpy.asarray(values, dtype="<u4").tobytes()
        else:
            body = numpy.asarray(values, dtype="<" + {"c": "i1", "C": "u1", "s": "i2", "S": "u2", "i": "i4", "I": "u4", "f": "f4"}[sub]).tobytes()
        return head + sub.encode() + struct.pack("<I", len(values)) + body
    if typ == "f" and isinstance(value, int):
        return head + struct.pack("<I", value)
    return head + struct.pack("<" + FORMATS[typ], value)


def pack_record(rec):
    """A record from a dict: qname, flag, ref, pos (0-based), mapq, cigar [(count, op byte)], next_ref, next_pos, tlen,
    seq (bytes of BASES, b"" for *), qual (bytes of phred values, None for 0xFF) and tags [(tag, type, value)]."""
    name = rec.get("qname", b"r") + b"\0"
    cigar = rec.get("cigar", [])
    seq = rec.get("seq", b"")
    nib = [BASES.index(c) for c in seq] + [0]
    packed = bytes((nib[k] << 4) | nib[k + 1] for k in range(0, len(seq), 2))
    qual = rec.get("qual")
    qual = b"\xff" * len(seq) if qual is None else qual
    assert len(qual) == len(seq)
    body = struct.pack("<iiBBHHHIiii", rec.get("ref", -1), rec.get("pos", -1), len(name), rec.get("mapq", 0), rec.get("bin", 4680),
                       rec.get("n_cigar", len(cigar)), rec.get("flag", 0), len(seq), rec.get("next_ref", -1),
                       rec.get("next_pos", -1), rec.get("tlen", 0))
    body += name + b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for n, op in cigar) + packed + qual
    body += b"".join(pack_tag(*t) for t in rec.get("tags", [])) + rec.get("raw_tags", b"")
    return struct.pack("<I", len(body)) + body


def header(text=b"", refs=()):
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for name, length in refs:
        out += struct.pack("<I", len(name) + 1) + name + b"\0" + struct.pack("<I", length)
    return out


def bam(text=b"", refs=(), records=()):
    """Inflated BAM; a record is a dict (pack_record) or its bytes."""
    return header(text, refs) + b"".join(r if isinstance(r, bytes) else pack_record(r) for r in records)


def bgzf_block(data, level=6):
    assert len(data) <= 65280
    if level == 0:   # stored, as bgzip -u... writes: one stored deflate block
        raw = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = c.compress(data) + c.flush()
    size = 18 + len(raw) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + raw +
            struct.pack("<II", zlib.crc32(data), len(data)))


def bgzf(data, cuts=None, level=6, eof=True, block=65280):
    """data as BGZF.  cuts: the offsets at which a new block begins (pieces longer than a block are cut further)."""
    edges = sorted(set([0, len(data)] + [c for c in (cuts or ()) if 0 < c < len(data)]))
    out = []
    for a, b in zip(edges, edges[1:]):
        for at in range(a, b, block):
            out.append(bgzf_block(data[at:min(b, at + block)], level))
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def gzip_member(data, level=6):
    """data as one generic gzip member (no BC subfield)."""
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


# ---- reading ------------------------------------------------------------------------------
def _values(sub, raw, count):
    if sub == "f":
        with numpy.errstate(invalid="ignore"):   # (a signalling NaN widens to a quiet one: nan either way)
            return [b"%g" % v for v in numpy.frombuffer(raw, dtype="<f4", count=count).astype(numpy.float64).tolist()]
    dt = {"c": "i1", "C": "u1", "s": "<i2", "S": "<u2", "i": "<i4", "I": "<u4"}[sub]
    return [b"%d" % int(v) for v in numpy.frombuffer(raw, dtype=dt, count=count)]


def parse_tags(area):
    """[(tag, type, value text, raw value)] of a tag area that fits the grammar."""
    out, p = [], 0
    while p < len(area):
        tag, typ = area[p:p + 2], chr(area[p + 2])
        p += 3
        if typ == "A":
            text, n = area[p:p + 1], 1
        elif typ in ("Z", "H"):
            n = area.index(b"\0", p) - p
            text, n = area[p:p + n], n + 1
        elif typ == "B":
            sub, count = chr(area[p]), struct.unpack_from("<I", area, p + 1)[0]
            n = 5 + count * SIZES[sub]
            text = b",".join([sub.encode()] + _values(sub, area[p + 5:p + n], count))
        else:
            n = SIZES[typ]
            text = _values(typ, area[p:p + n], 1)[0]
        out.append((tag, typ, text, area[p:p + n]))
        p += n
    return out


def read_header(data):
    """(the text without its trailing NULs, [reference names], where the records begin)."""
    assert data[:4] == b"BAM\1"
    l_text = struct.unpack_from("<I", data, 4)[0]
    text = data[8:8 + l_text].rstrip(b"\0")
    n_ref = struct.unpack_from("<I", data, 8 + l_text)[0]
    p, names = 12 + l_text, []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<I", data, p)[0]
        names.append(data[p + 4:p + 4 + l_name - 1])
        p += 8 + l_name
    return text, names, p


def record_offsets(data):
    """Where each record of a well-framed BAM begins."""
    p, out = read_header(data)[2], []
    while p < len(data):
        out.append(p)
        p += 4 + struct.unpack_from("<I", data, p)[0]
    assert p == len(data)
    return out


def sam_line(data, p, names):
    """The SAM line (without '\\n') of the record at p."""
    (bs, ref, pos, l_name, mapq, _, n_cigar, flag, l_seq, next_ref, next_pos, tlen) = struct.unpack_from("<IiiBBHHHIiii", data, p)
    q = p + 36
    qname = data[q:q + l_name - 1]
    q += l_name
    ops = list(struct.unpack_from("<%dI" % n_cigar, data, q))
    q += 4 * n_cigar
    packed = data[q:q + (l_seq + 1) // 2]
    q += (l_seq + 1) // 2
    qual = data[q:q + l_seq]
    q += l_seq
    tags = parse_tags(data[q:p + 4 + bs])
    if n_cigar == 2 and ops[0] == (l_seq << 4 | 4) and ops[1] & 15 == 3:
        for k, (tag, typ, text, raw) in enumerate(tags):
            if tag == b"CG" and typ == "B" and raw[:1] == b"I":
                ops = list(numpy.frombuffer(raw, dtype="<u4", offset=5))
                del tags[k]
                break
    seq = bytes(BASES[(packed[k >> 1] >> (0 if k & 1 else 4)) & 15] for k in range(l_seq)) if l_seq < 4096 else \
        numpy.frombuffer(BASES, dtype="u1")[numpy.stack([numpy.frombuffer(packed, dtype="u1") >> 4,
                                                         numpy.frombuffer(packed, dtype="u1") & 15], 1).reshape(-1)[:l_seq]].tobytes()
    cols = [qname, b"%d" % flag, names[ref] if ref >= 0 else b"*", b"%d" % (pos + 1), b"%d" % mapq,
            b"".join(b"%d%c" % (int(v) >> 4, OPS[int(v) & 15]) for v in ops) or b"*",
            b"*" if next_ref < 0 else (b"=" if next_ref == ref else names[next_ref]), b"%d" % (next_pos + 1), b"%d" % tlen,
            seq or b"*", b"*" if not l_seq or qual[0] == 0xff else (numpy.frombuffer(qual, dtype="u1") + 33).astype("u1").tobytes()]
    cols += [b"%s:%s:%s" % (tag, b"i" if typ in "cCsSiI" else typ.encode(), text) for tag, typ, text, _ in tags]
    return b"\t".join(cols)


def sam_text(data):
    """The SAM text of inflated BAM: the header text, each of its lines ended by '\\n', then a line per record."""
    text, names, _ = read_header(data)
    if text and not text.endswith(b"\n"):
        text += b"\n"
    return text + b"".join(sam_line(data, p, names) + b"\n" for p in record_offsets(data))


def expected(data, **options):
    """The unsorted BED that bam2bed writes for inflated BAM: sam2bed's for its SAM text."""
    return align_oracle.sam(sam_text(data), **options)


# ---- random records -----------------------------------------------------------------------
REFS = ((b"chr1", 248956422), (b"chr2", 242193529), (b"chrX", 156040895), (b"chrUn_KI270302v1", 2274))
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n@PG\tID:x\n"


def random_record(rng, k=0):
    flag = rng.choice((0, 16, 99, 147, 4, 77, 141, 256, 2048 + 16))
    n_ops = rng.choice((0, 1, 1, 2, 3, 5, 9))
    cigar = [(rng.randint(1, 40) if rng.random() < 0.9 else rng.choice((0, 268435455)), bytes([rng.choice(OPS)])) for _ in range(n_ops)]
    l_seq = rng.choice((0, 1, 2, 7, 36, 37, 151))
    tags = []
    for _ in range(rng.randint(0, 6)):
        tag = bytes(rng.choice(b"ABNMXYZ") for _ in range(2))
        typ = rng.choice("AcCsSiIfZHB")
        if typ == "A":
            value = bytes([rng.randint(33, 126)])
        elif typ == "Z":
            value = bytes(rng.randint(32, 126) for _ in range(rng.randint(0, 30)))
        elif typ == "H":
            value = b"".join(b"%02X" % rng.randint(0, 255) for _ in range(rng.randint(0, 6)))
        elif typ == "f":
            value = rng.choice((0, 0x80000000, 0x3f800000, 0x7f800000, 0xff800000, 0x7fc00000, rng.getrandbits(32)))
        elif typ == "B":
            sub = rng.choice("cCsSiIf")
            value = (sub, [_random_value(rng, sub) for _ in range(rng.choice((0, 1, 3, 17)))])
        else:
            value = _random_value(rng, typ)
        tags.append((tag, typ, value))
    ref = rng.randint(0, len(REFS) - 1)
    return dict(qname=b"read%d/%d" % (k, rng.randint(0, 10 ** rng.randint(0, 6))), flag=flag, ref=ref, pos=rng.randint(0, 2 ** 31 - 2),
                mapq=rng.choice((0, 9, 60, 255)), cigar=cigar, next_ref=rng.choice((-1, ref, rng.randint(0, len(REFS) - 1))),
                next_pos=rng.randint(-1, 2 ** 31 - 2), tlen=rng.randint(-2 ** 31, 2 ** 31 - 1),
                seq=bytes(rng.choice(BASES) for _ in range(l_seq)),
                qual=None if rng.random() < 0.2 else bytes(rng.randint(0, 93) for _ in range(l_seq)), tags=tags)


def _random_value(rng, typ):
    if typ == "f":
        return rng.getrandbits(32)
    lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}[typ]
    return rng.choice((lo, hi, 0, rng.randint(lo, hi)))


def random_bam(rng, records, text=TEXT, refs=REFS):
    """(inflated BAM, the dicts of its records); a fifth of the records are unmapped."""
    recs = [random_record(rng, k) for k in range(records)]
    return bam(text, refs, recs), recs


# ---- the hand-written table -----------------------------------------------------------------
# (record, its SAM line); the references are REFS
TABLE = [
    (dict(qname=b"r001", flag=99, ref=0, pos=6, mapq=30, cigar=[(8, b"M"), (2, b"I"), (4, b"M"), (1, b"D"), (3, b"M")], next_ref=0,
          next_pos=36, tlen=39, seq=b"TTAGATAAAGGATACTG", qual=bytes([0, 1, 40, 93] + [30] * 13)),
     b"r001\t99\tchr1\t7\t30\t8M2I4M1D3M\t=\t37\t39\tTTAGATAAAGGATACTG\t!\"I~?????????????"),
    (dict(qname=b"r002", flag=16, ref=1, pos=0, mapq=255, cigar=[(1, b"M")], next_ref=2, next_pos=99, tlen=-2147483648, seq=b"A"),
     b"r002\t16\tchr2\t1\t255\t1M\tchrX\t100\t-2147483648\tA\t*"),
    (dict(qname=b"star", flag=0, ref=3, pos=2273, mapq=0),
     b"star\t0\tchrUn_KI270302v1\t2274\t0\t*\t*\t0\t0\t*\t*"),
    (dict(qname=b"un", flag=4, ref=-1, pos=-1, seq=b"=ACMGRSVTWYHKDBN", qual=bytes(range(16))),
     b"un\t4\t*\t0\t0\t*\t*\t0\t0\t=ACMGRSVTWYHKDBN\t!\"#$%&'()*+,-./0"),
    (dict(qname=b"ops", flag=0, ref=0, pos=99, cigar=[(1, b"M"), (2, b"I"), (3, b"D"), (4, b"N"), (5, b"S"), (6, b"H"), (7, b"P"), (8, b"="),
                                                      (268435455, b"X")], seq=b"ACG", qual=bytes([10, 20, 30])),
     b"ops\t0\tchr1\t100\t0\t1M2I3D4N5S6H7P8=268435455X\t*\t0\t0\tACG\t+5?"),
    (dict(qname=b"ints", flag=0, ref=0, pos=0, cigar=[(2, b"M")], seq=b"AC", qual=None,
          tags=[(b"Ac", "c", -128), (b"AC", "C", 255), (b"As", "s", -32768), (b"AS", "S", 65535), (b"Ai", "i", -2147483648),
                (b"AI", "I", 4294967295), (b"AA", "A", b"!"), (b"AZ", "Z", b"a b:c"), (b"EZ", "Z", b""), (b"AH", "H", b"1AE301")]),
     b"ints\t0\tchr1\t1\t0\t2M\t*\t0\t0\tAC\t*\tAc:i:-128\tAC:i:255\tAs:i:-32768\tAS:i:65535\tAi:i:-2147483648\tAI:i:4294967295"
     b"\tAA:A:!\tAZ:Z:a b:c\tEZ:Z:\tAH:H:1AE301"),
    (dict(qname=b"floats", flag=0, ref=0, pos=0,
          tags=[(b"F0", "f", 0.0), (b"F1", "f", 0x80000000), (b"F2", "f", 1e-5), (b"F3", "f", 123456.5), (b"F4", "f", 1e6),
                (b"F5", "f", 1), (b"F6", "f", 0x7f800000), (b"F7", "f", 0xff800000), (b"F8", "f", 0x7fc00000), (b"F9", "f", 0xffc00001),
                (b"Fa", "f", 0x00800000), (b"Fb", "f", 0x7f7fffff), (b"Fc", "f", 0.1), (b"Fd", "f", 999999.5), (b"Fe", "f", 0.0001),
                (b"Ff", "f", 100000.0), (b"Fg", "f", -2.5), (b"Fh", "f", 0x00000002)]),
     b"floats\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\t*\tF0:f:0\tF1:f:-0\tF2:f:1e-05\tF3:f:123456\tF4:f:1e+06\tF5:f:1.4013e-45\tF6:f:inf"
     b"\tF7:f:-inf\tF8:f:nan\tF9:f:nan\tFa:f:1.17549e-38\tFb:f:3.40282e+38\tFc:f:0.1\tFd:f:1e+06\tFe:f:0.0001\tFf:f:100000"
     b"\tFg:f:-2.5\tFh:f:2.8026e-45"),
    (dict(qname=b"arrays", flag=0, ref=0, pos=0,
          tags=[(b"Bc", "B", ("c", [-1, 0, 127])), (b"BC", "B", ("C", [200])), (b"Bs", "B", ("s", [-300, 300])), (b"BS", "B", ("S", [])),
                (b"Bi", "B", ("i", [-70000])), (b"BI", "B", ("I", [4000000000, 1])), (b"Bf", "B", ("f", [1.5, -0.25, 3e10]))]),
     b"arrays\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\t*\tBc:B:c,-1,0,127\tBC:B:C,200\tBs:B:s,-300,300\tBS:B:S\tBi:B:i,-70000\tBI:B:I,4000000000,1"
     b"\tBf:B:f,1.5,-0.25,3e+10"),
    (dict(qname=b"odd", flag=147, ref=2, pos=9, mapq=7, cigar=[(3, b"M")], next_ref=2, next_pos=-1, tlen=-5, seq=b"NAN", qual=bytes([0xff, 1, 2])),
     b"odd\t147\tchrX\t10\t7\t3M\t=\t0\t-5\tNAN\t*"),
    (dict(qname=b"long", flag=0, ref=0, pos=10, cigar=[(4, b"S"), (30, b"N")], seq=b"ACGT", qual=bytes([1, 2, 3, 4]),
          tags=[(b"NM", "C", 1), (b"CG", "B", ("I", [(2 << 4) | 0, (10 << 4) | 3, (2 << 4) | 0])), (b"XX", "Z", b"y")]),
     b"long\t0\tchr1\t11\t0\t2M10N2M\t*\t0\t0\tACGT\t\"#$%\tNM:i:1\tXX:Z:y"),
    (dict(qname=b"notlong", flag=0, ref=0, pos=10, cigar=[(3, b"S"), (30, b"N")], seq=b"ACGT", qual=bytes([1, 2, 3, 4]),
          tags=[(b"CG", "B", ("I", [(2 << 4) | 0]))]),
     b"notlong\t0\tchr1\t11\t0\t3S30N\t*\t0\t0\tACGT\t\"#$%\tCG:B:I,32"),
    (dict(qname=b"", flag=0, ref=0, pos=0, cigar=[(5, b"D")]),
     b"\t0\tchr1\t1\t0\t5D\t*\t0\t0\t*\t*"),
]
