"""A plain-Python convert2bed: the definitions of include/starch_amd.h
("convert2bed: GFF3, GTF, VCF and WIG to BED"), one function per format, each
returning the unsorted BED.  A line that does not fit its format raises
ConvertError with its number (from 1) and the library's text for it.

TABLE holds hand-written cases: (format, options, input, expected), where
expected is the output bytes or, for an error, (line, text)."""

LIMIT = (1 << 63) - 1

# what is wrong with a line, in the library's words (bed_convert.hip: bad_text)
E_FEW = "fewer tab-separated fields than the format needs"
E_MANY = "more than nine tab-separated fields"
E_NONAME = "empty sequence name"
E_EMPTY = "empty coordinate"
E_DIGIT = "non-digit in a coordinate"
E_RANGE = "coordinate has 20 or more digits or is above 2^63-1"
E_ZERO = "start or position below 1"
E_END = "end below start"
E_STOP = "stop not above start"
E_REF = "empty REF"
E_ALT = "empty ALT"
E_ALLELE = "empty ALT allele"
E_OVER = "coordinate would exceed 2^63-1"
E_TOKENS = "a data line has 1, 2 or 4 tokens"
E_NODECL = "data line before any declaration"
E_MISFIT = "data line does not fit the declaration in force"
E_KEY = "unknown key in a declaration"
E_TWICE = "repeated key in a declaration"
E_NOCHROM = "declaration without chrom"
E_NOSTART = "fixedStep declaration without start"
E_VALUE = "declaration value is not a number from 1 to 2^63-1"

FORMATS = ("gff", "gtf", "vcf", "wig")


class ConvertError(Exception):
    def __init__(self, line, text):
        super().__init__("line %d: %s" % (line, text))
        self.line, self.text = line, text


def lines_of(data):
    """The input cut at '\\n'; a last line without one is a line."""
    if not data:
        return []
    rows = data.split(b"\n")
    if data.endswith(b"\n"):
        rows.pop()
    return rows


def coord(field, no):
    if not field:
        raise ConvertError(no, E_EMPTY)
    if any(c not in b"0123456789" for c in field):
        raise ConvertError(no, E_DIGIT)
    if len(field) > 19 or int(field) > LIMIT:
        raise ConvertError(no, E_RANGE)
    return int(field)


class _Headers:
    def __init__(self, keep):
        self.keep, self.count = keep, 0

    def line(self, row):
        k = self.count
        self.count += 1
        return [b"_header\t%d\t%d\t%s\n" % (k, k + 1, row)] if self.keep else []


def gff_id(attrs):
    for piece in attrs.split(b";"):
        if piece.startswith(b"ID="):
            return piece[3:] or b"."
    return b"."


def gtf_id(attrs):
    at = 0
    while True:
        p = attrs.find(b'gene_id "', at)
        if p < 0:
            return b"."
        if p == 0 or attrs[p - 1:p] in (b";", b" "):
            q = attrs.find(b'"', p + 9)
            return (attrs[p + 9:q] or b".") if q >= 0 else b"."
        at = p + 1


def _annotation(data, keep_header, find_id, fasta):
    out, hdr = [], _Headers(keep_header)
    for no, row in enumerate(lines_of(data), 1):
        if fasta and row == b"##FASTA":
            break
        if not row or row.startswith(b"#"):
            out += hdr.line(row)
            continue
        f = row.split(b"\t")
        if len(f) < 9:
            raise ConvertError(no, E_FEW)
        if len(f) > 9:
            raise ConvertError(no, E_MANY)
        if not f[0]:
            raise ConvertError(no, E_NONAME)
        start, end = coord(f[3], no), coord(f[4], no)
        if start < 1:
            raise ConvertError(no, E_ZERO)
        if end < start:
            raise ConvertError(no, E_END)
        out.append(b"\t".join([f[0], b"%d" % (start - 1), b"%d" % end, find_id(f[8]), f[5], f[6], f[1], f[2], f[7], f[8]]) + b"\n")
    return b"".join(out)


def gff(data, keep_header=False):
    return _annotation(data, keep_header, gff_id, True)


def gtf(data, keep_header=False):
    return _annotation(data, keep_header, gtf_id, False)


def allele_class(allele, ref):
    return "snvs" if len(allele) == len(ref) else ("insertions" if len(allele) > len(ref) else "deletions")


def vcf(data, vcf_class="all", keep_header=False):
    out, hdr = [], _Headers(keep_header)
    for no, row in enumerate(lines_of(data), 1):
        if not row or row.startswith(b"#"):
            out += hdr.line(row)
            continue
        f = row.split(b"\t", 7)
        if len(f) < 8:
            raise ConvertError(no, E_FEW)
        if not f[0]:
            raise ConvertError(no, E_NONAME)
        pos = coord(f[1], no)
        if pos < 1:
            raise ConvertError(no, E_ZERO)
        if not f[3]:
            raise ConvertError(no, E_REF)
        if not f[4]:
            raise ConvertError(no, E_ALT)
        alleles = [f[4]] if vcf_class == "all" else f[4].split(b",")
        if b"" in alleles:
            raise ConvertError(no, E_ALLELE)
        start, stop = pos - 1, pos - 1 + len(f[3])
        if stop > LIMIT:
            raise ConvertError(no, E_OVER)
        for a in alleles:
            if vcf_class == "all" or allele_class(a, f[3]) == vcf_class:
                out.append(b"\t".join([f[0], b"%d" % start, b"%d" % stop, f[2], f[5], f[3], a, f[6], f[7]]) + b"\n")
    return b"".join(out)


def _tokens(row):
    return [t for t in row.replace(b"\t", b" ").split(b" ") if t]


def _declaration(tok, no):
    fixed = tok[0] == b"fixedStep"
    known = (b"chrom", b"start", b"step", b"span") if fixed else (b"chrom", b"span")
    d = {}
    for t in tok[1:]:
        key, eq, value = t.partition(b"=")
        if not eq or key not in known:
            raise ConvertError(no, E_KEY)
        if key in d:
            raise ConvertError(no, E_TWICE)
        if key == b"chrom":
            if not value:
                raise ConvertError(no, E_NOCHROM)
            d[key] = value
        else:
            if not value or any(c not in b"0123456789" for c in value) or len(value) > 19 or not 1 <= int(value) <= LIMIT:
                raise ConvertError(no, E_VALUE)
            d[key] = int(value)
    if b"chrom" not in d:
        raise ConvertError(no, E_NOCHROM)
    if fixed and b"start" not in d:
        raise ConvertError(no, E_NOSTART)
    return dict(fixed=fixed, chrom=d[b"chrom"], start=d.get(b"start", 0), step=d.get(b"step", 1), span=d.get(b"span", 1), k=0)


def wig(data, keep_header=False):
    out, hdr = [], _Headers(keep_header)
    decl, n = None, 0
    for no, row in enumerate(lines_of(data), 1):
        tok = _tokens(row)
        if not row or row.startswith(b"#") or (tok and tok[0] in (b"track", b"browser")):
            out += hdr.line(row)
            continue
        if tok and tok[0] in (b"variableStep", b"fixedStep"):
            decl = _declaration(tok, no)
            continue
        if len(tok) not in (1, 2, 4):
            raise ConvertError(no, E_TOKENS)
        if len(tok) == 4:
            chrom, start, stop = tok[0], coord(tok[1], no), coord(tok[2], no)
            if stop <= start:
                raise ConvertError(no, E_STOP)
        else:
            if len(tok) == 2:
                pos = coord(tok[0], no)
                if pos < 1:
                    raise ConvertError(no, E_ZERO)
            if decl is None:
                raise ConvertError(no, E_NODECL)
            if decl["fixed"] != (len(tok) == 1):
                raise ConvertError(no, E_MISFIT)
            if decl["fixed"]:
                start = decl["start"] - 1 + decl["k"] * decl["step"]
                decl["k"] += 1
            else:
                start = pos - 1
            chrom, stop = decl["chrom"], start + decl["span"]
            if stop > LIMIT:
                raise ConvertError(no, E_OVER)
        n += 1
        out.append(b"%s\t%d\t%d\tid-%d\t%s\n" % (chrom, start, stop, n, tok[-1]))
    return b"".join(out)


def convert(fmt, data, vcf_class="all", keep_header=False):
    """The unsorted BED of data in format fmt (a name of FORMATS)."""
    if fmt == "vcf":
        return vcf(data, vcf_class, keep_header)
    if vcf_class != "all":
        raise ValueError("vcf_class goes with vcf alone")
    return {"gff": gff, "gtf": gtf, "wig": wig}[fmt](data, keep_header)


def counts(fmt, data):
    """(input lines, header lines, data lines, declarations) as starch_convert_get_stats counts them."""
    rows = lines_of(data)
    used = rows[:rows.index(b"##FASTA")] if fmt == "gff" and b"##FASTA" in rows else rows
    hdr = dec = 0
    for row in used:
        tok = _tokens(row)
        if not row or row.startswith(b"#") or (fmt == "wig" and tok and tok[0] in (b"track", b"browser")):
            hdr += 1
        elif fmt == "wig" and tok and tok[0] in (b"variableStep", b"fixedStep"):
            dec += 1
    return len(rows), hdr, len(used) - hdr - dec, dec


def sort_bed(bed):
    """sort-bed's order: chromosome bytes, start, stop; equal keys in input order."""
    rows = bed.split(b"\n")[:-1]
    def key(r):
        f = r.split(b"\t")
        return f[0], int(f[1]), int(f[2])
    return b"".join(r + b"\n" for r in sorted(rows, key=key))


# ---- random inputs for the comparisons ------------------------------------------------
def random_input(fmt, rng, records, headers=True):
    chroms = [b"chr1", b"chr10", b"chr2", b"chrX"]
    rows = []
    if fmt in ("gff", "gtf"):
        if headers:
            rows.append(b"##gff-version 3")
        for k in range(records):
            s = rng.randint(1, 5000)
            e = s + rng.choice((0, 1, 30, 900))
            name = b"g%d" % rng.randrange(100)
            if fmt == "gff":
                attrs = rng.choice((b"ID=%s;Name=x", b"Name=x;ID=%s;Note=a b", b"Name=%s", b"ID=;Name=%s", b"fooID=%s;Parent=p")) % name
            else:
                attrs = rng.choice((b'gene_id "%s"; transcript_id "t1";', b'transcript_id "t"; gene_id "%s";',
                                    b'transcript_id "%s";', b'other_gene_id "x"; gene_id "%s";', b'gene_id ""; x "%s";')) % name
            rows.append(b"\t".join([rng.choice(chroms), b"src", rng.choice((b"gene", b"exon")), b"%d" % s, b"%d" % e,
                                    rng.choice((b".", b"0.5", b"13")), rng.choice((b"+", b"-", b".")), rng.choice((b".", b"0", b"2")), attrs]))
            if headers and rng.random() < 0.05:
                rows.append(rng.choice((b"", b"# a comment")))
    elif fmt == "vcf":
        if headers:
            rows += [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
        bases = (b"A", b"C", b"G", b"T", b"AC", b"GTT", b"ACGT")
        for k in range(records):
            ref = rng.choice(bases)
            alt = b",".join(rng.choice(bases) for _ in range(rng.choice((1, 1, 2, 3, 4))))
            f = [rng.choice(chroms), b"%d" % rng.randint(1, 5000), rng.choice((b".", b"rs%d" % k)), ref, alt,
                 rng.choice((b".", b"29", b"3.5")), rng.choice((b"PASS", b"q10")), b"NS=3;DP=%d" % rng.randrange(100)]
            if rng.random() < 0.5:
                f += [b"GT:GQ"] + [b"0|%d:%d" % (rng.randrange(2), rng.randrange(60)) for _ in range(3)]
            rows.append(b"\t".join(f))
    else:
        if headers:
            rows.append(b"track type=wiggle_0 name=x")
        mode = None
        for k in range(records):
            r = rng.random()
            if mode is None or r < 0.04:
                mode = rng.choice(("v", "f"))
                c = rng.choice(chroms)
                if mode == "v":
                    rows.append(rng.choice((b"variableStep chrom=%s", b"variableStep chrom=%s span=5", b"variableStep\tspan=2  chrom=%s")) % c)
                else:
                    rows.append(b"fixedStep chrom=%s start=%d step=%d span=%d"
                                % (c, rng.randint(1, 900), rng.choice((1, 10)), rng.choice((1, 3))))
            if r > 0.9:
                s = rng.randrange(5000)
                rows.append(b"%s\t%d\t%d\t%s" % (rng.choice(chroms), s, s + rng.randint(1, 50), b"%.2f" % rng.random()))
            elif mode == "v":
                rows.append(b"%d %s" % (rng.randint(1, 5000), b"%d" % rng.randrange(100)))
            else:
                rows.append(b"%.3f" % rng.random())
            if headers and rng.random() < 0.03:
                rows.append(rng.choice((b"", b"#c", b"browser position chr1:1-100")))
    return b"\n".join(rows) + b"\n"


# ---- the hand-written table ---------------------------------------------------------------
G = b"chr1\tsrc\tgene\t11\t20\t0.5\t+\t.\t"     # a GFF/GTF record up to its attributes
V = b"chr1\t10\trs1\t"                          # a VCF record up to REF
_BIG = b"9223372036854775807"                   # 2^63-1

TABLE = [
    # -- framing and headers
    ("gff", {}, b"", b""),
    ("gff", {}, b"##gff-version 3\n\n#c\n", b""),
    ("gff", dict(keep_header=True), b"##gff-version 3\n\n" + G + b"ID=a\n#c",
     b"_header\t0\t1\t##gff-version 3\n_header\t1\t2\t\nchr1\t10\t20\ta\t0.5\t+\tsrc\tgene\t.\tID=a\n_header\t2\t3\t#c\n"),
    ("gff", {}, G + b"ID=a", b"chr1\t10\t20\ta\t0.5\t+\tsrc\tgene\t.\tID=a\n"),                     # no final newline
    ("gff", {}, G + b"ID=a\r\n", b"chr1\t10\t20\ta\r\t0.5\t+\tsrc\tgene\t.\tID=a\r\n"),               # \r is a byte
    # -- gff: ID
    ("gff", {}, G + b"Name=n;ID=b;Note=x\n", b"chr1\t10\t20\tb\t0.5\t+\tsrc\tgene\t.\tName=n;ID=b;Note=x\n"),
    ("gff", {}, G + b"Name=n\n", b"chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\tName=n\n"),
    ("gff", {}, G + b"ID=;Name=n;ID=z\n", b"chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\tID=;Name=n;ID=z\n"),
    ("gff", {}, G + b"fooID=q;Name=n\n", b"chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\tfooID=q;Name=n\n"),
    ("gff", {}, G + b"fooID=q;ID=r\n", b"chr1\t10\t20\tr\t0.5\t+\tsrc\tgene\t.\tfooID=q;ID=r\n"),
    ("gff", {}, b"c\ts\tt\t5\t5\t.\t.\t.\t\n", b"c\t4\t5\t.\t.\t.\ts\tt\t.\t\n"),                     # start == end, empty attributes
    # -- gff: ##FASTA
    ("gff", dict(keep_header=True), b"##FASTA\n>seq\nACGT\n", b""),
    ("gff", dict(keep_header=True), b"#h\n" + G + b"ID=a\n##FASTA\n>chr1 not\ta record\nACGT\n##FASTA\n",
     b"_header\t0\t1\t#h\nchr1\t10\t20\ta\t0.5\t+\tsrc\tgene\t.\tID=a\n"),
    ("gff", dict(keep_header=True), G + b"ID=a\n##FASTA", b"chr1\t10\t20\ta\t0.5\t+\tsrc\tgene\t.\tID=a\n"),
    ("gff", dict(keep_header=True), b"##FASTA \n", b"_header\t0\t1\t##FASTA \n"),                    # not exactly ##FASTA
    ("gtf", dict(keep_header=True), b"##FASTA\n", b"_header\t0\t1\t##FASTA\n"),                      # no such rule in gtf
    # -- gff: errors
    ("gff", {}, G + b"ID=a\n" + G[:-1] + b"\n", (2, E_FEW)),
    ("gff", {}, G + b"ID=a\textra\n", (1, E_MANY)),
    ("gff", {}, b"\ts\tt\t5\t6\t.\t.\t.\tx\n", (1, E_NONAME)),
    ("gff", {}, b"c\ts\tt\t\t6\t.\t.\t.\tx\n", (1, E_EMPTY)),
    ("gff", {}, b"c\ts\tt\t5\t6x\t.\t.\t.\tx\n", (1, E_DIGIT)),
    ("gff", {}, b"c\ts\tt\t-5\t6\t.\t.\t.\tx\n", (1, E_DIGIT)),
    ("gff", {}, b"c\ts\tt\t5\t12345678901234567890\t.\t.\t.\tx\n", (1, E_RANGE)),
    ("gff", {}, b"c\ts\tt\t5\t9223372036854775808\t.\t.\t.\tx\n", (1, E_RANGE)),
    ("gff", {}, b"c\ts\tt\t5\t" + _BIG + b"\t.\t.\t.\tx\n", b"c\t4\t" + _BIG + b"\t.\t.\t.\ts\tt\t.\tx\n"),
    ("gff", {}, b"c\ts\tt\t0\t6\t.\t.\t.\tx\n", (1, E_ZERO)),
    ("gff", {}, b"c\ts\tt\t7\t6\t.\t.\t.\tx\n", (1, E_END)),
    ("gff", {}, b"c\ts\tt\t007\t0010\t.\t.\t.\tx\n", b"c\t6\t10\t.\t.\t.\ts\tt\t.\tx\n"),          # coordinates are numbers
    ("gff", {}, b"c\ts\tt\t7\t6\t.\t.\t.\tx\n##FASTA\n", (1, E_END)),                                # an error before ##FASTA counts
    # -- gtf: gene_id
    ("gtf", {}, G + b'gene_id "g1"; transcript_id "t1";\n', b'chr1\t10\t20\tg1\t0.5\t+\tsrc\tgene\t.\tgene_id "g1"; transcript_id "t1";\n'),
    ("gtf", {}, G + b'transcript_id "t1"; gene_id "g2";\n', b'chr1\t10\t20\tg2\t0.5\t+\tsrc\tgene\t.\ttranscript_id "t1"; gene_id "g2";\n'),
    ("gtf", {}, G + b'transcript_id "t1";gene_id "g3"\n', b'chr1\t10\t20\tg3\t0.5\t+\tsrc\tgene\t.\ttranscript_id "t1";gene_id "g3"\n'),
    ("gtf", {}, G + b'transcript_id "t1";\n', b'chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\ttranscript_id "t1";\n'),
    ("gtf", {}, G + b'gene_id ""; gene_id "z";\n', b'chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\tgene_id ""; gene_id "z";\n'),
    ("gtf", {}, G + b'other_gene_id "x"; gene_id "g4";\n', b'chr1\t10\t20\tg4\t0.5\t+\tsrc\tgene\t.\tother_gene_id "x"; gene_id "g4";\n'),
    ("gtf", {}, G + b'gene_id "open\n', b'chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\tgene_id "open\n'),   # no closing quote
    ("gtf", {}, G + b'ID=a\n', b'chr1\t10\t20\t.\t0.5\t+\tsrc\tgene\t.\tID=a\n'),                     # ID= means nothing in gtf
    ("gtf", {}, G[:-3] + b"\n", (1, E_FEW)),
    # -- vcf
    ("vcf", {}, b"##fileformat=VCFv4.2\n#CHROM\tPOS\n" + V + b"A\tG\t29\tPASS\tNS=3\n", b"chr1\t9\t10\trs1\t29\tA\tG\tPASS\tNS=3\n"),
    ("vcf", {}, V + b"ACG\tA,ACGT\t29\tPASS\tNS=3\tGT\t0|1\t1|1\t0|0\n", b"chr1\t9\t12\trs1\t29\tACG\tA,ACGT\tPASS\tNS=3\tGT\t0|1\t1|1\t0|0\n"),
    ("vcf", dict(keep_header=True), b"#h\n" + V + b"A\tG\t.\t.\t\n", b"_header\t0\t1\t#h\nchr1\t9\t10\trs1\t.\tA\tG\t.\t\n"),   # empty INFO
    ("vcf", dict(vcf_class="snvs"), V + b"AC\tA,GT,ACG,TT\t9\tq\tI\tS\n", b"chr1\t9\t11\trs1\t9\tAC\tGT\tq\tI\tS\nchr1\t9\t11\trs1\t9\tAC\tTT\tq\tI\tS\n"),
    ("vcf", dict(vcf_class="insertions"), V + b"AC\tA,GT,ACG,TT\t9\tq\tI\tS\n", b"chr1\t9\t11\trs1\t9\tAC\tACG\tq\tI\tS\n"),
    ("vcf", dict(vcf_class="deletions"), V + b"AC\tA,GT,ACG,TT\t9\tq\tI\tS\n", b"chr1\t9\t11\trs1\t9\tAC\tA\tq\tI\tS\n"),
    ("vcf", dict(vcf_class="all"), V + b"AC\tA,GT,ACG,TT\t9\tq\tI\tS\n", b"chr1\t9\t11\trs1\t9\tAC\tA,GT,ACG,TT\tq\tI\tS\n"),
    ("vcf", dict(vcf_class="deletions"), V + b"A\tG,TT\t9\tq\tI\n" + V + b"AC\tG\t9\tq\tI\n", b"chr1\t9\t11\trs1\t9\tAC\tG\tq\tI\n"),   # no allele of the class
    ("vcf", {}, V + b"A\tG,,T\t9\tq\tI\n", b"chr1\t9\t10\trs1\t9\tA\tG,,T\tq\tI\n"),                # ALT is not split by default
    ("vcf", dict(vcf_class="insertions"), V + b"A\tG,,T\t9\tq\tI\n", (1, E_ALLELE)),
    ("vcf", dict(vcf_class="snvs"), V + b"A\tG,\t9\tq\tI\n", (1, E_ALLELE)),
    ("vcf", {}, V + b"A\tG\t9\tq\n", (1, E_FEW)),
    ("vcf", {}, b"\t10\trs1\tA\tG\t9\tq\tI\n", (1, E_NONAME)),
    ("vcf", {}, b"c\t\trs1\tA\tG\t9\tq\tI\n", (1, E_EMPTY)),
    ("vcf", {}, b"c\t1e3\trs1\tA\tG\t9\tq\tI\n", (1, E_DIGIT)),
    ("vcf", {}, b"c\t12345678901234567890\trs1\tA\tG\t9\tq\tI\n", (1, E_RANGE)),
    ("vcf", {}, b"c\t0\trs1\tA\tG\t9\tq\tI\n", (1, E_ZERO)),
    ("vcf", {}, V + b"\tG\t9\tq\tI\n", (1, E_REF)),
    ("vcf", {}, V + b"A\t\t9\tq\tI\n", (1, E_ALT)),
    ("vcf", {}, b"c\t" + _BIG + b"\t.\tAC\tG\t9\tq\tI\n", (1, E_OVER)),
    ("vcf", {}, b"c\t" + _BIG + b"\t.\tA\tG\t9\tq\tI\n", b"c\t9223372036854775806\t" + _BIG + b"\t.\t9\tA\tG\tq\tI\n"),
    # -- wig
    ("wig", {}, b"track type=wiggle_0\nvariableStep chrom=chr2\n300 1.5\n310\t-2\n", b"chr2\t299\t300\tid-1\t1.5\nchr2\t309\t310\tid-2\t-2\n"),
    ("wig", {}, b"variableStep span=5 chrom=chr2\n  300   1.5  \n", b"chr2\t299\t304\tid-1\t1.5\n"),
    ("wig", {}, b"fixedStep chrom=c start=11 step=10 span=3\n1\n2\n3\n", b"c\t10\t13\tid-1\t1\nc\t20\t23\tid-2\t2\nc\t30\t33\tid-3\t3\n"),
    ("wig", {}, b"fixedStep span=2 start=5 chrom=c\n7\n8\n", b"c\t4\t6\tid-1\t7\nc\t5\t7\tid-2\t8\n"),                       # step defaults to 1
    ("wig", {}, b"c\t5\t9\t0.25\nfixedStep chrom=d start=1\n1\ne 7 8 x\n2\n", b"c\t5\t9\tid-1\t0.25\nd\t0\t1\tid-2\t1\ne\t7\t8\tid-3\tx\nd\t1\t2\tid-4\t2\n"),
    ("wig", {}, b"fixedStep chrom=a start=1\nvariableStep chrom=b\n5 x\nfixedStep chrom=a start=9\ny\n", b"b\t4\t5\tid-1\tx\na\t8\t9\tid-2\ty\n"),
    ("wig", dict(keep_header=True), b"browser position chr1\n#c\nvariableStep chrom=b\n5 x\ntrack a\n6 y\n\n",
     b"_header\t0\t1\tbrowser position chr1\n_header\t1\t2\t#c\nb\t4\t5\tid-1\tx\n_header\t2\t3\ttrack a\nb\t5\t6\tid-2\ty\n_header\t3\t4\t\n"),
    ("wig", {}, b"tracking\n", (1, E_NODECL)),                                       # 'track' must be the whole token
    ("wig", {}, b"5 x\n", (1, E_NODECL)),
    ("wig", {}, b"x\nvariableStep chrom=b\n", (1, E_NODECL)),
    ("wig", {}, b"variableStep chrom=b\n5 x\n7\n", (3, E_MISFIT)),
    ("wig", {}, b"fixedStep chrom=b start=1\n5 x\n", (2, E_MISFIT)),
    ("wig", {}, b"variableStep chrom=b\n5 x y\n", (2, E_TOKENS)),
    ("wig", {}, b"variableStep chrom=b\n1 2 3 4 5\n", (2, E_TOKENS)),
    ("wig", {}, b"variableStep chrom=b\n \t \n", (2, E_TOKENS)),
    ("wig", {}, b"variableStep chrom=b\n0 x\n", (2, E_ZERO)),
    ("wig", {}, b"variableStep chrom=b\n5x x\n", (2, E_DIGIT)),
    ("wig", {}, b"variableStep chrom=b\n12345678901234567890 x\n", (2, E_RANGE)),
    ("wig", {}, b"c 9 9 x\n", (1, E_STOP)),
    ("wig", {}, b"c 9 a x\n", (1, E_DIGIT)),
    ("wig", {}, b"variableStep\n", (1, E_NOCHROM)),
    ("wig", {}, b"variableStep chrom=\n", (1, E_NOCHROM)),
    ("wig", {}, b"fixedStep chrom=c step=2\n", (1, E_NOSTART)),
    ("wig", {}, b"variableStep chrom=c start=5\n", (1, E_KEY)),
    ("wig", {}, b"fixedStep chrom=c start=5 colour=red\n", (1, E_KEY)),
    ("wig", {}, b"fixedStep chrom=c start=5 step\n", (1, E_KEY)),
    ("wig", {}, b"fixedStep chrom=c start=5 start=6\n", (1, E_TWICE)),
    ("wig", {}, b"fixedStep chrom=c start=0\n", (1, E_VALUE)),
    ("wig", {}, b"fixedStep chrom=c start=1 step=0\n", (1, E_VALUE)),
    ("wig", {}, b"variableStep chrom=c span=0\n", (1, E_VALUE)),
    ("wig", {}, b"variableStep chrom=c span=x\n", (1, E_VALUE)),
    ("wig", {}, b"variableStep chrom=c span=\n", (1, E_VALUE)),
    ("wig", {}, b"variableStep chrom=c span=2\n" + _BIG + b" x\n", (2, E_OVER)),
    ("wig", {}, b"variableStep chrom=c\n" + _BIG + b" x\n", b"c\t9223372036854775806\t" + _BIG + b"\tid-1\tx\n"),
    ("wig", {}, b"fixedStep chrom=c start=9223372036854775806 step=1\n1\n2\n3\n", (4, E_OVER)),
    ("wig", {}, b"fixedStep chrom=c start=1 step=" + _BIG + b"\n1\n2\n3\n", (3, E_OVER)),
    # -- the lowest bad line is the one named
    ("vcf", {}, V + b"A\tG\t9\tq\tI\n" + b"c\t0\t.\tA\tG\t9\tq\tI\n" + V + b"A\tG\t9\n", (2, E_ZERO)),
]
