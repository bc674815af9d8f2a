"""A plain-Python sam2bed, psl2bed and rmsk2bed: the definitions of
include/starch_amd.h ("sam2bed, psl2bed, rmsk2bed: SAM, PSL and RepeatMasker .out
to BED"), one function per format, each returning the unsorted BED.  A line that
does not fit its format raises ConvertError with its number (from 1) and the
library's text for it.

TABLE holds hand-written cases: (format, options, input, expected), where
expected is the output bytes or, for an error, (line, text)."""
from tests.convert_oracle import LIMIT, ConvertError, _Headers, coord, lines_of, sort_bed  # noqa: F401
from tests.convert_oracle import E_DIGIT, E_EMPTY, E_END, E_OVER, E_RANGE, E_STOP, E_ZERO  # noqa: F401

# what is wrong with a line, in the library's words (bed_align.hip: bad_text)
E_FEW6 = "fewer than six tab-separated fields"
E_FLAG = "FLAG is not a decimal number from 0 to 65535"
E_RNAME = "mapped record without a reference name"
E_CIGAR = "CIGAR is not * or pieces of a count of 1 to 9 digits and one of MIDNSHP=X"
E_NODASH = "psLayout header without a line of dashes"
E_FEW21 = "fewer than 21 tab-separated fields"
E_MANY21 = "more than 21 tab-separated fields"
E_FIELD = "empty field"
E_STRAND = "strand is not +, - or two of them"
E_LIST = "blockSizes and tStarts do not hold blockCount comma-terminated numbers"
E_BLOCK0 = "block of size 0"
E_UNDER = "block start and size exceed tSize on the reverse strand"
E_TOKENS = "a record has 15 tokens, or 16 with a last *"
E_RSTRAND = "strand is not + or C"

FORMATS = ("sam", "psl", "rmsk")
COMMANDS = {"sam": "sam2bed", "psl": "psl2bed", "rmsk": "rmsk2bed"}
DIGITS = b"0123456789"


def _number(field):
    """1 to 19 digits up to 2^63-1, or None."""
    if not field or any(c not in DIGITS for c in field) or len(field) > 19 or int(field) > LIMIT:
        return None
    return int(field)


# ---- SAM ------------------------------------------------------------------------------
def cigar_pieces(cigar, no):
    """[(count, op)] of a CIGAR that is not '*'."""
    pieces, at = [], 0
    if not cigar:
        raise ConvertError(no, E_CIGAR)
    while at < len(cigar):
        end = at
        while end < len(cigar) and cigar[end] in DIGITS:
            end += 1
        if not 1 <= end - at <= 9 or end == len(cigar) or cigar[end] not in b"MIDNSHP=X":
            raise ConvertError(no, E_CIGAR)
        pieces.append((int(cigar[at:end]), cigar[end:end + 1]))
        at = end + 1
    return pieces


def cigar_runs(pieces, start, split_deletions):
    """The maximal runs of M D = X with positive length, as (start, stop)."""
    runs, at, length = [], start, 0
    for count, op in pieces + [(0, b"N")]:
        if op == b"N" or (split_deletions and op == b"D"):
            if length:
                runs.append((at, at + length))
            at, length = at + length + count, 0
        elif op in (b"M", b"D", b"=", b"X"):
            length += count
    return runs


def sam(data, split=False, split_deletions=False, all_reads=False, reduced=False, keep_header=False):
    if split_deletions and not split:
        raise ValueError("split_deletions goes with split")
    out, hdr = [], _Headers(keep_header)
    for no, row in enumerate(lines_of(data), 1):
        if not row or row.startswith(b"@"):
            out += hdr.line(row)
            continue
        f = row.split(b"\t", 5)
        if len(f) < 6:
            raise ConvertError(no, E_FEW6)
        qname, flag_text, rname, pos_text, mapq, rest = f
        flag = _number(flag_text)
        if flag is None or flag > 65535:
            raise ConvertError(no, E_FLAG)
        strand = b"-" if flag & 16 else b"+"
        if flag & 4:
            if not all_reads:
                continue
            rname, spans = b"_unmapped", [(0, 1)]
        else:
            if rname in (b"", b"*"):
                raise ConvertError(no, E_RNAME)
            pos = coord(pos_text, no)
            if pos < 1:
                raise ConvertError(no, E_ZERO)
            cigar = rest.split(b"\t", 1)[0]
            pieces = [] if cigar == b"*" else cigar_pieces(cigar, no)
            length = sum(c for c, op in pieces if op in (b"M", b"D", b"N", b"=", b"X"))
            stop = pos - 1 + max(1, length)
            if stop > LIMIT:
                raise ConvertError(no, E_OVER)
            spans = (cigar_runs(pieces, pos - 1, split_deletions) if split else []) or [(pos - 1, stop)]
        for a, b in spans:
            cols = [rname, b"%d" % a, b"%d" % b, qname, flag_text, strand]
            out.append(b"\t".join(cols if reduced else cols + [mapq, rest]) + b"\n")
    return b"".join(out)


# ---- PSL ------------------------------------------------------------------------------
def _list(field, no):
    if not field.endswith(b","):
        raise ConvertError(no, E_LIST)
    values = [_number(v) for v in field[:-1].split(b",")]
    if None in values:
        raise ConvertError(no, E_LIST)
    return values


def psl_header_end(rows):
    """The number of leading header lines of a PSL file (0: no psLayout), or None without the dashes."""
    if not rows or not rows[0].startswith(b"psLayout"):
        return 0
    for k, row in enumerate(rows):
        if row.startswith(b"-----"):
            return k + 1
    return None


def psl(data, split=False, keep_header=False):
    out, hdr = [], _Headers(keep_header)
    rows = lines_of(data)
    head = psl_header_end(rows)
    if head is None:
        raise ConvertError(1, E_NODASH)
    for no, row in enumerate(rows, 1):
        if no <= head or not row:
            out += hdr.line(row)
            continue
        f = row.split(b"\t")
        if len(f) < 21:
            raise ConvertError(no, E_FEW21)
        if len(f) > 21:
            raise ConvertError(no, E_MANY21)
        if b"" in f:
            raise ConvertError(no, E_FIELD)
        tsize, tstart, tend, blocks = coord(f[14], no), coord(f[15], no), coord(f[16], no), coord(f[17], no)
        if len(f[8]) not in (1, 2) or any(c not in b"+-" for c in f[8]):
            raise ConvertError(no, E_STRAND)
        if tstart >= tend:
            raise ConvertError(no, E_STOP)
        spans = [(tstart, tend)]
        if split:
            sizes, starts = _list(f[18], no), _list(f[20], no)
            spans = []
            for k in range(min(blocks, len(sizes), len(starts))):
                if sizes[k] == 0:
                    raise ConvertError(no, E_BLOCK0)
                if f[8][1:] == b"-":
                    if starts[k] + sizes[k] > tsize:
                        raise ConvertError(no, E_UNDER)
                    spans.append((tsize - starts[k] - sizes[k], tsize - starts[k]))
                else:
                    if starts[k] + sizes[k] > LIMIT:
                        raise ConvertError(no, E_OVER)
                    spans.append((starts[k], starts[k] + sizes[k]))
            if not len(sizes) == len(starts) == blocks:
                raise ConvertError(no, E_LIST)
        for a, b in spans:
            out.append(b"\t".join([f[13], b"%d" % a, b"%d" % b, f[9], f[0], f[8], f[10]] + f[1:8] + f[11:13] + [f[14]] + f[17:21]) + b"\n")
    return b"".join(out)


# ---- RepeatMasker .out ----------------------------------------------------------------
def _tokens(row):
    return [t for t in row.replace(b"\t", b" ").split(b" ") if t]


def rmsk(data, keep_header=False):
    out, hdr = [], _Headers(keep_header)
    for no, row in enumerate(lines_of(data), 1):
        t = _tokens(row)
        if not t or t[0] in (b"SW", b"score"):
            out += hdr.line(row)
            continue
        if not (len(t) == 15 or (len(t) == 16 and t[15] == b"*")):
            raise ConvertError(no, E_TOKENS)
        if t[8] not in (b"+", b"C"):
            raise ConvertError(no, E_RSTRAND)
        begin, end = coord(t[5], no), coord(t[6], no)
        if begin < 1:
            raise ConvertError(no, E_ZERO)
        if end < begin:
            raise ConvertError(no, E_END)
        strand = b"-" if t[8] == b"C" else b"+"
        out.append(b"\t".join([t[4], b"%d" % (begin - 1), b"%d" % end, t[9], t[0], strand, t[1], t[2], t[3], t[7]] + t[10:]) + b"\n")
    return b"".join(out)


def convert(fmt, data, **kw):
    """The unsorted BED of data in format fmt (a name of FORMATS)."""
    return {"sam": sam, "psl": psl, "rmsk": rmsk}[fmt](data, **kw)


def counts(fmt, data):
    """(input lines, header lines, records, unmapped records) as starch_align_get_stats counts them."""
    rows = lines_of(data)
    head = psl_header_end(rows) if fmt == "psl" else 0
    hdr = unmapped = 0
    for k, row in enumerate(rows):
        t = _tokens(row)
        if fmt == "sam":
            header = not row or row.startswith(b"@")
            if not header and int(row.split(b"\t")[1]) & 4:
                unmapped += 1
        elif fmt == "psl":
            header = k < head or not row
        else:
            header = not t or t[0] in (b"SW", b"score")
        hdr += header
    return len(rows), hdr, len(rows) - hdr, unmapped


# ---- random inputs for the comparisons ------------------------------------------------
def sam_row(qname, flag, rname, pos, cigar, rest=b"=\t0\t0\tACGT\tIIII\tNM:i:0", mapq=b"60"):
    return b"\t".join([qname, b"%d" % flag, rname, b"%d" % pos, mapq, cigar, rest])


def psl_row(tname, tstart, tend, strand=b"+", tsize=100000, sizes=(10,), tstarts=None, qname=b"q1", blocks=None):
    tstarts = [tstart] if tstarts is None else tstarts
    blocks = len(sizes) if blocks is None else blocks
    lists = [b"".join(b"%d," % v for v in sizes), b"".join(b"%d," % k for k in range(len(sizes))), b"".join(b"%d," % v for v in tstarts)]
    return b"\t".join([b"59", b"1", b"0", b"0", b"1", b"2", b"1", b"3", strand, qname, b"70", b"5", b"66", tname, b"%d" % tsize,
                       b"%d" % tstart, b"%d" % tend, b"%d" % blocks] + lists)


RMSK_HEAD = (b"   SW  perc perc perc  query      position in query           matching       repeat              position in  repeat\n"
             b"score  div. del. ins.  sequence    begin     end    (left)    repeat         class/family         begin  end (left)   ID\n"
             b"\n")


def rmsk_row(query, begin, end, strand=b"+", star=False, ident=1):
    return b"%5d  11.5  6.2  0.0  %s  %8d %8d (%d) %s  AluSx   SINE/Alu  %s  310  %s  %d%s" % (
        1000 + ident % 977, query, begin, end, 248956422 - end, strand,
        b"(2)" if strand == b"C" else b"1", b"1" if strand == b"C" else b"(2)", ident, b" *" if star else b"")


def random_input(fmt, rng, records, headers=True):
    chroms = [b"chr1", b"chr10", b"chr2", b"chrX"]
    rows = []
    if fmt == "sam":
        if headers:
            rows += [b"@HD\tVN:1.6\tSO:unsorted", b"@SQ\tSN:chr1\tLN:248956422"]
        ops = b"MIDNSHP=X"
        for k in range(records):
            cigar = rng.choice((b"*", b"50M", b"5S45M", b"20M1000N30M", b"10M2D5M3I20M", b"10=1X10=", b"3H10M500N10M2D10M20N5M4S", b"7I"))
            if rng.random() < 0.3:
                cigar = b"".join(b"%d%c" % (rng.randint(1, 40), rng.choice(ops)) for _ in range(rng.randint(1, 8)))
            flag = rng.choice((0, 16, 99, 147, 4, 77, 2064))
            mapped = not flag & 4
            rows.append(sam_row(b"read%d" % k, flag, rng.choice(chroms) if mapped else b"*", rng.randint(1, 5000) if mapped else 0,
                                cigar if mapped else b"*", mapq=b"%d" % rng.randrange(61),
                                rest=rng.choice((b"*\t0\t0\tACGT\tIIII", b"=\t%d\t-50\tAC\tII\tNM:i:1\tMD:Z:2" % k, b"*"))))
            if headers and rng.random() < 0.03:
                rows.append(rng.choice((b"", b"@CO\ta comment")))
    elif fmt == "psl":
        if headers:
            rows += [b"psLayout version 3", b"", b"match\tmis- \trep. \tN's", b"     \tmatch", b"-" * 60]
        for k in range(records):
            n = rng.choice((1, 1, 2, 3, 7))
            tsize = 100000
            sizes = [rng.randint(1, 30) for _ in range(n)]
            strand = rng.choice((b"+", b"-", b"++", b"+-", b"-+", b"--"))
            t, tstarts = rng.randrange(5000), []
            for sz in sizes:
                tstarts.append(t)
                t += sz + rng.randrange(40)
            rows.append(psl_row(rng.choice(chroms), tstarts[0], tstarts[-1] + sizes[-1], strand, tsize, sizes, tstarts, b"q%d" % k))
            if headers and rng.random() < 0.03:
                rows.append(b"")
    else:
        for k in range(records):
            if headers and (k == 0 or rng.random() < 0.01):
                rows += RMSK_HEAD.split(b"\n")[:-1]
            begin = rng.randint(1, 5000)
            rows.append(rmsk_row(rng.choice(chroms), begin, begin + rng.choice((0, 1, 300)), rng.choice((b"+", b"C")), rng.random() < 0.2, k))
    return b"\n".join(rows) + b"\n"


# ---- the hand-written table ---------------------------------------------------------------
_BIG = b"9223372036854775807"                   # 2^63-1
_R = b"\t=\t0\t0\tAC\tII"                       # what follows a CIGAR
_P = b"59\t1\t0\t0\t1\t2\t1\t3\t"               # a PSL record up to its strand
_M = b"1306  15.6  6.2  0.0  chr1  "            # a RepeatMasker record up to begin


def _s(cigar, flag=b"0", pos=b"11"):
    return b"r1\t" + flag + b"\tchr1\t" + pos + b"\t60\t" + cigar + _R + b"\n"


def _so(start, stop, cigar, flag=b"0", strand=b"+"):
    return b"chr1\t%d\t%d\tr1\t%s\t%s\t60\t%s" % (start, stop, flag, strand, cigar) + _R + b"\n"


TABLE = [
    # -- sam: framing and headers
    ("sam", {}, b"", b""),
    ("sam", {}, b"@HD\tVN:1.6\n\n@SQ\tSN:chr1\n", b""),
    ("sam", dict(keep_header=True), b"@HD\tVN:1.6\n\n" + _s(b"5M") + b"@CO\tx",
     b"_header\t0\t1\t@HD\tVN:1.6\n_header\t1\t2\t\n" + _so(10, 15, b"5M") + b"_header\t2\t3\t@CO\tx\n"),
    ("sam", {}, _s(b"5M")[:-1], _so(10, 15, b"5M")),                                         # no final newline
    ("sam", {}, b"r1\t0\tchr1\t11\t60\t5M\t*\r\n", b"chr1\t10\t15\tr1\t0\t+\t60\t5M\t*\r\n"),   # \r is a byte
    ("sam", {}, b"r1\t0\tchr1\t11\t60\t5M", b"chr1\t10\t15\tr1\t0\t+\t60\t5M\n"),           # six fields are enough
    # -- sam: every operator, *, clips
    ("sam", {}, _s(b"4M"), _so(10, 14, b"4M")),
    ("sam", {}, _s(b"4M3I2M"), _so(10, 16, b"4M3I2M")),
    ("sam", {}, _s(b"4M3D2M"), _so(10, 19, b"4M3D2M")),
    ("sam", {}, _s(b"4M3N2M"), _so(10, 19, b"4M3N2M")),
    ("sam", {}, _s(b"2S4M1S"), _so(10, 14, b"2S4M1S")),
    ("sam", {}, _s(b"2H4M"), _so(10, 14, b"2H4M")),
    ("sam", {}, _s(b"4M2P4M"), _so(10, 18, b"4M2P4M")),
    ("sam", {}, _s(b"4=1X4="), _so(10, 19, b"4=1X4=")),
    ("sam", {}, _s(b"*"), _so(10, 11, b"*")),
    ("sam", {}, _s(b"5S"), _so(10, 11, b"5S")),
    ("sam", {}, _s(b"10I"), _so(10, 11, b"10I")),
    ("sam", {}, _s(b"0M"), _so(10, 11, b"0M")),
    ("sam", {}, _s(b"007M"), _so(10, 17, b"007M")),
    # -- sam: split
    ("sam", {}, _s(b"3M2N4M"), _so(10, 19, b"3M2N4M")),
    ("sam", dict(split=True), _s(b"3M2N4M"), _so(10, 13, b"3M2N4M") + _so(15, 19, b"3M2N4M")),
    ("sam", dict(split=True, split_deletions=True), _s(b"3M2N4M"), _so(10, 13, b"3M2N4M") + _so(15, 19, b"3M2N4M")),
    ("sam", dict(split=True), _s(b"2M1D2M"), _so(10, 15, b"2M1D2M")),
    ("sam", dict(split=True, split_deletions=True), _s(b"2M1D2M"), _so(10, 12, b"2M1D2M") + _so(13, 15, b"2M1D2M")),
    ("sam", dict(split=True), _s(b"2N3M4N"), _so(12, 15, b"2N3M4N")),                          # N at both ends
    ("sam", dict(split=True), _s(b"2S3M1I2M5N2N1=1X3H"), _so(10, 15, b"2S3M1I2M5N2N1=1X3H") + _so(22, 24, b"2S3M1I2M5N2N1=1X3H")),
    ("sam", dict(split=True), _s(b"5N"), _so(10, 15, b"5N")),                                  # no run: the unsplit line
    ("sam", dict(split=True), _s(b"*"), _so(10, 11, b"*")),
    ("sam", dict(split=True, split_deletions=True), _s(b"3D"), _so(10, 13, b"3D")),
    ("sam", dict(split=True, reduced=True), _s(b"3M2N4M"), b"chr1\t10\t13\tr1\t0\t+\nchr1\t15\t19\tr1\t0\t+\n"),
    # -- sam: flags
    ("sam", {}, _s(b"4M", b"16"), _so(10, 14, b"4M", b"16", b"-")),
    ("sam", {}, _s(b"4M", b"65535", b"1"), b""),                                              # bit 4: dropped
    ("sam", {}, _s(b"4M", b"0083"), _so(10, 14, b"4M", b"0083", b"-")),                        # FLAG is copied as written
    ("sam", {}, b"r1\t4\t*\t0\t0\t*\t*\t0\t0\tAC\tII\n" + _s(b"4M"), _so(10, 14, b"4M")),
    ("sam", dict(all_reads=True), b"r1\t4\t*\t0\t0\t*\t*\t0\t0\tAC\tII\n", b"_unmapped\t0\t1\tr1\t4\t+\t0\t*\t*\t0\t0\tAC\tII\n"),
    ("sam", dict(all_reads=True, split=True), b"r1\t20\tchrZ\tx\t9\tjunk\n", b"_unmapped\t0\t1\tr1\t20\t-\t9\tjunk\n"),   # unread columns
    ("sam", dict(all_reads=True, reduced=True), b"r1\t4\t*\t0\t0\t*\n" + _s(b"4M"), b"_unmapped\t0\t1\tr1\t4\t+\nchr1\t10\t14\tr1\t0\t+\n"),
    ("sam", dict(reduced=True), _s(b"4M", b"16"), b"chr1\t10\t14\tr1\t16\t-\n"),
    # -- sam: errors
    ("sam", {}, _s(b"4M") + b"r1\t0\tchr1\t11\t60\n", (2, E_FEW6)),
    ("sam", {}, _s(b"4M", b""), (1, E_FLAG)),
    ("sam", {}, _s(b"4M", b"0x10"), (1, E_FLAG)),
    ("sam", {}, _s(b"4M", b"65536"), (1, E_FLAG)),
    ("sam", {}, b"r1\t0\t*\t11\t60\t4M\n", (1, E_RNAME)),
    ("sam", {}, b"r1\t0\t\t11\t60\t4M\n", (1, E_RNAME)),
    ("sam", {}, _s(b"4M", pos=b""), (1, E_EMPTY)),
    ("sam", {}, _s(b"4M", pos=b"1e3"), (1, E_DIGIT)),
    ("sam", {}, _s(b"4M", pos=b"12345678901234567890"), (1, E_RANGE)),
    ("sam", {}, _s(b"4M", pos=b"0"), (1, E_ZERO)),
    ("sam", {}, _s(b""), (1, E_CIGAR)),
    ("sam", {}, _s(b"4"), (1, E_CIGAR)),
    ("sam", {}, _s(b"M"), (1, E_CIGAR)),
    ("sam", {}, _s(b"4M*"), (1, E_CIGAR)),
    ("sam", {}, _s(b"*4M"), (1, E_CIGAR)),
    ("sam", {}, _s(b"4Q"), (1, E_CIGAR)),
    ("sam", {}, _s(b"4m"), (1, E_CIGAR)),
    ("sam", {}, _s(b"1234567890M"), (1, E_CIGAR)),                                             # ten digits
    ("sam", {}, _s(b"123456789M"), _so(10, 123456799, b"123456789M")),                         # nine
    ("sam", {}, _s(b"2M", pos=_BIG), (1, E_OVER)),
    ("sam", {}, _s(b"1M", pos=_BIG), b"chr1\t9223372036854775806\t" + _BIG + b"\tr1\t0\t+\t60\t1M" + _R + b"\n"),
    # -- psl
    ("psl", {}, b"", b""),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t161\t2\t30,31,\t5,35,\t100,130,\n",
     b"chr1\t100\t161\tq1\t59\t+\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t2\t30,31,\t5,35,\t100,130,\n"),
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t161\t2\t30,31,\t5,35,\t100,130,\n",
     b"chr1\t100\t130\tq1\t59\t+\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t2\t30,31,\t5,35,\t100,130,\n"
     b"chr1\t130\t161\tq1\t59\t+\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t2\t30,31,\t5,35,\t100,130,\n"),
    ("psl", dict(split=True), _P + b"+-\tq1\t70\t5\t66\tchr1\t1000\t839\t900\t2\t30,31,\t5,35,\t100,130,",
     b"chr1\t870\t900\tq1\t59\t+-\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t2\t30,31,\t5,35,\t100,130,\n"
     b"chr1\t839\t870\tq1\t59\t+-\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t2\t30,31,\t5,35,\t100,130,\n"),
    ("psl", dict(split=True), _P + b"-+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t100,\n",      # the second character decides
     b"chr1\t100\t130\tq1\t59\t-+\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t1\t30,\t5,\t100,\n"),
    ("psl", {}, _P + b"-\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t9\tx\ty\tz\n",                            # the lists are unread without split
     b"chr1\t100\t130\tq1\t59\t-\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t9\tx\ty\tz\n"),
    ("psl", dict(keep_header=True), b"psLayout version 3\n\nmatch\tmis\n---------\n\n" + _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t100,\n",
     b"_header\t0\t1\tpsLayout version 3\n_header\t1\t2\t\n_header\t2\t3\tmatch\tmis\n_header\t3\t4\t---------\n_header\t4\t5\t\n"
     b"chr1\t100\t130\tq1\t59\t+\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t1000\t1\t30,\t5,\t100,\n"),
    ("psl", {}, b"psLayout version 3\nmatch\n-----\n-----\n", (4, E_FEW21)),                            # only the first dashes line ends the header
    ("psl", {}, b"-----\n", (1, E_FEW21)),                                                              # no psLayout: no header
    ("psl", {}, b"psLayout version 3\nmatch\n", (1, E_NODASH)),
    ("psl", {}, b" psLayout\n", (1, E_FEW21)),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\n", (1, E_FEW21)),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t100,\t\n", (1, E_MANY21)),
    ("psl", {}, _P + b"+\t\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t100,\n", (1, E_FIELD)),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t\n", (1, E_FIELD)),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t1x0\t130\t1\t30,\t5,\t100,\n", (1, E_DIGIT)),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t12345678901234567890\t1\t30,\t5,\t100,\n", (1, E_RANGE)),
    ("psl", {}, _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t130\t130\t1\t30,\t5,\t100,\n", (1, E_STOP)),
    ("psl", {}, _P + b"*\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t100,\n", (1, E_STRAND)),
    ("psl", {}, _P + b"+-+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t100,\n", (1, E_STRAND)),
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t2\t30,\t5,\t100,\n", (1, E_LIST)),      # too few
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,1,\t5,\t100,\n", (1, E_LIST)),    # too many
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30\t5,\t100,\n", (1, E_LIST)),       # no comma
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t30,\t5,\t1o0,\n", (1, E_LIST)),
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t0\t30,\t5,\t100,\n", (1, E_LIST)),
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t0,\t5,\t100,\n", (1, E_BLOCK0)),
    ("psl", dict(split=True), _P + b"+-\tq1\t70\t5\t66\tchr1\t129\t100\t130\t1\t30,\t5,\t100,\n", (1, E_UNDER)),
    ("psl", dict(split=True), _P + b"+-\tq1\t70\t5\t66\tchr1\t130\t100\t130\t1\t30,\t5,\t100,\n",
     b"chr1\t0\t30\tq1\t59\t+-\t70\t1\t0\t0\t1\t2\t1\t3\t5\t66\t130\t1\t30,\t5,\t100,\n"),
    ("psl", dict(split=True), _P + b"+\tq1\t70\t5\t66\tchr1\t1000\t100\t130\t1\t2,\t5,\t9223372036854775806,\n", (1, E_OVER)),
    # -- rmsk
    ("rmsk", {}, RMSK_HEAD, b""),
    ("rmsk", dict(keep_header=True), b"  SW  perc\nscore  div.\n \t \n" + _M + b"11 20 (30) + AluSx SINE/Alu 1 310 (2) 7\n",
     b"_header\t0\t1\t  SW  perc\n_header\t1\t2\tscore  div.\n_header\t2\t3\t \t \nchr1\t10\t20\tAluSx\t1306\t+\t15.6\t6.2\t0.0\t(30)\tSINE/Alu\t1\t310\t(2)\t7\n"),
    ("rmsk", {}, b"   \t" + _M + b"11 20 (30) C AluSx SINE/Alu (2) 310 1 7 *  ",                       # C, *, leading and trailing blanks
     b"chr1\t10\t20\tAluSx\t1306\t-\t15.6\t6.2\t0.0\t(30)\tSINE/Alu\t(2)\t310\t1\t7\t*\n"),
    ("rmsk", {}, _M + b"11\t11\t(30)\t+\tL1\tLINE/L1\t1\t310\t(2)\t7\n", b"chr1\t10\t11\tL1\t1306\t+\t15.6\t6.2\t0.0\t(30)\tLINE/L1\t1\t310\t(2)\t7\n"),
    ("rmsk", {}, _M + b"11 20 (30) + AluSx SINE/Alu 1 310 (2)\n", (1, E_TOKENS)),
    ("rmsk", {}, _M + b"11 20 (30) + AluSx SINE/Alu 1 310 (2) 7 x\n", (1, E_TOKENS)),
    ("rmsk", {}, _M + b"11 20 (30) + AluSx SINE/Alu 1 310 (2) 7 * *\n", (1, E_TOKENS)),
    ("rmsk", {}, b"SWx\n", (1, E_TOKENS)),                                                              # 'SW' must be the whole token
    ("rmsk", {}, _M + b"11 20 (30) - AluSx SINE/Alu 1 310 (2) 7\n", (1, E_RSTRAND)),
    ("rmsk", {}, _M + b"1x 20 (30) + AluSx SINE/Alu 1 310 (2) 7\n", (1, E_DIGIT)),
    ("rmsk", {}, _M + b"11 12345678901234567890 (30) + AluSx SINE/Alu 1 310 (2) 7\n", (1, E_RANGE)),
    ("rmsk", {}, _M + b"0 20 (30) + AluSx SINE/Alu 1 310 (2) 7\n", (1, E_ZERO)),
    ("rmsk", {}, _M + b"21 20 (30) + AluSx SINE/Alu 1 310 (2) 7\n", (1, E_END)),
    # -- the lowest bad line is the one named
    ("sam", {}, _s(b"4M") + _s(b"4M", pos=b"0") + b"r1\t0\n", (2, E_ZERO)),
]
