"""GPU: convert2bed (Starch.convert, convert_device, compress_converted, the
convert2bed command).

Every comparison is equality of whole outputs against tests/convert_oracle.py.
T is the number of lines per block of the per-line kernels, W the bytes from
which a copied tail is left to a whole wave.
"""
import itertools
import os
import random
import subprocess

import pytest

from tests import convert_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
CONVERT = os.path.join(BUILD, "convert2bed")
G = oracle.G
LIMIT = oracle.LIMIT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def TW():
    import starch_amd
    return starch_amd.convert_constants()


def check(ctx, fmt, data, **kw):
    """Unsorted and sorted output against the oracle; returns the oracle's unsorted BED."""
    want = oracle.convert(fmt, data, **kw)
    assert ctx.convert(data, fmt, sort=False, **kw) == want, (fmt, kw)
    assert ctx.convert(data, fmt, **kw) == oracle.sort_bed(want), (fmt, kw)
    return want


def check_error(ctx, fmt, data, line, text, **kw):
    import starch_amd
    for sort in (False, True):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.convert(data, fmt, sort=sort, **kw)
        assert e.value.code == -12 and str(e.value).endswith("convert2bed: line %d: %s" % (line, text)), str(e.value)
        with pytest.raises(starch_amd.StarchError) as e:   # no output is left behind
            ctx._output()
        assert e.value.code == -4


def gff_rows(n, attrs=b"ID=a%d"):
    return [G.replace(b"11\t20", b"%d\t%d" % (n - k, n - k + 5)) + attrs % k for k in range(n)]


def vcf_rows(n):
    return [b"chr%d\t%d\t.\tAC\tA,GT,ACG\t9\tq\tDP=%d" % (k % 3, n - k, k) for k in range(n)]


# ---- each format on random records ----------------------------------------------------
@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_random_records_unsorted_sorted_and_archive(ctx, fmt):
    rng = random.Random(7 + oracle.FORMATS.index(fmt))
    data = oracle.random_input(fmt, rng, 400)
    lines, hdr, rec, dec = oracle.counts(fmt, data)
    assert rec == 400 and hdr >= 2 and (dec >= 5) == (fmt == "wig")
    want = check(ctx, fmt, data)
    check(ctx, fmt, data, keep_header=True)
    assert oracle.sort_bed(want) != want                       # the sort has work to do
    assert ctx.sort_bed(want) == oracle.sort_bed(want)
    assert ctx.compress_converted(data, fmt) == ctx.compress(ctx.sort_bed(want))
    assert ctx.convert_stats()["sorted"] == 1
    if fmt == "vcf":
        n = {c: check(ctx, fmt, data, vcf_class=c).count(b"\n") for c in ("snvs", "insertions", "deletions")}
        assert min(n.values()) > 50, n


# ---- framing edges --------------------------------------------------------------------
@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_empty_headers_only_and_single_lines(ctx, fmt):
    record = {"gff": G + b"ID=a", "gtf": G + b'gene_id "a";', "vcf": b"c\t5\t.\tA\tG\t9\tq\tI", "wig": b"c 5 9 0.5"}[fmt]
    for kw in ({}, dict(keep_header=True)):
        assert check(ctx, fmt, b"", **kw) == b""
        assert check(ctx, fmt, b"\n", **kw).count(b"\n") == len(kw)
        check(ctx, fmt, b"#a\n\n#b", **kw)                       # headers only, the last without '\n'
        assert check(ctx, fmt, record, **kw).count(b"\n") == 1   # one record, no '\n'
        assert check(ctx, fmt, record + b"\n", **kw).count(b"\n") == 1
        assert check(ctx, fmt, b"#h\n" + record + b"\n" + record, **kw).count(b"\n") == 2 + len(kw)
    assert ctx.convert_stats()["input_lines"] == 3


def test_a_line_across_the_framing_tile(ctx):
    rows = gff_rows(600)
    if (b"\n".join(rows))[16383:16384] == b"\n":
        rows[0] += b";pad=1"
    data = b"\n".join(rows) + b"\n"
    assert len(data) > 16384 + 64 and data[16383:16384] != b"\n"   # bytes 16383 and 16384 belong to one line
    check(ctx, "gff", data)


def test_line_counts_around_the_block_size(ctx, TW):
    T, _ = TW
    for n in (T - 1, T, T + 1, 3 * T + 1):
        assert check(ctx, "gff", b"\n".join(gff_rows(n)) + b"\n").count(b"\n") == n
        assert check(ctx, "gtf", b"\n".join(gff_rows(n, b'gene_id "g%d";'))).count(b"\n") == n
        assert check(ctx, "vcf", b"\n".join(vcf_rows(n)) + b"\n", vcf_class="snvs").count(b"\n") == n
        wig = b"variableStep chrom=c span=2\n" + b"".join(b"%d %d\n" % (n - k, k) for k in range(n - 1))
        assert wig.count(b"\n") == n and check(ctx, "wig", wig).count(b"\n") == n - 1


@pytest.mark.parametrize("fmt", ("gff", "vcf"))
def test_kept_headers_at_the_block_edges(ctx, TW, fmt):
    """Header ordinals and the tally's per-wave counts across a block boundary."""
    T, _ = TW
    rows = gff_rows(2 * T + 1) if fmt == "gff" else vcf_rows(2 * T + 1)
    for at in (0, T - 1, T, 2 * T):
        rows[at] = b"#comment %d" % at
    data = b"\n".join(rows) + b"\n"
    for keep in (True, False):
        got = check(ctx, fmt, data, keep_header=keep)
        assert ctx.convert_stats()["header_lines"] == 4
        assert (b"_header\t3\t4\t" in got) == keep


# ---- long tails -------------------------------------------------------------------------
def test_tails_around_the_wave_copy_threshold(ctx, TW):
    T, W = TW
    for n in range(W - 3, W + 3):
        attrs = b"ID=x;Note=" + b"n" * (n - 10)
        assert len(attrs) == n
        rows = gff_rows(5)
        rows[2] = G + attrs
        rows[4] = G + attrs[::-1]
        check(ctx, "gff", b"\n".join(rows) + b"\n")
        tail = b"DP=1\tGT\t" + b"0|1\t" * ((n - 8) // 4) + b"x" * ((n - 8) % 4)
        assert len(tail) == n
        rows = vcf_rows(70)
        rows[0] = rows[69] = b"c\t7\t.\tAC\tA,GT,TT\t9\tq\t" + tail
        rows[33] = b"#" + tail
        data = b"\n".join(rows) + b"\n"
        for c in ("all", "snvs", "deletions"):
            check(ctx, "vcf", data, vcf_class=c, keep_header=True)


def test_a_70_kb_tail_among_short_lines(ctx):
    big = b";".join(b"k%d=v%d" % (k, k) for k in range(6000)) + b";ID=late"
    assert 65536 < len(big) < 80000
    rows = gff_rows(130)
    rows[64] = G + big
    want = check(ctx, "gff", b"\n".join(rows) + b"\n")
    assert want.split(b"\n")[64].split(b"\t")[3] == b"late"
    samples = b"\t".join(b"%d|%d:%d" % (k & 1, k % 3 & 1, k % 97) for k in range(10000))
    assert 65536 < len(samples) < 80000
    rows = vcf_rows(130)
    rows[0] = b"#CHROM\tPOS\t" + samples
    rows[129] = b"chrZ\t1\t.\tAC\tA,GT,TT,ACG\t9\tq\tDP=1\tGT\t" + samples
    data = b"\n".join(rows)
    check(ctx, "vcf", data, keep_header=True)
    assert check(ctx, "vcf", data, vcf_class="snvs").count(samples) == 2   # the tail goes out once per allele


# ---- the hand-written table: every rule and every error kind ----------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_the_hand_written_table(ctx, case):
    fmt, kw, data, want = oracle.TABLE[case]
    if isinstance(want, tuple):
        check_error(ctx, fmt, data, want[0], want[1], **kw)
    else:
        assert check(ctx, fmt, data, **kw) == want


# ---- GFF, GTF ---------------------------------------------------------------------------
def test_gff_fasta_and_id(ctx):
    body = b"".join(G + a + b"\n" for a in (b"ID=first;Name=n", b"Name=n;ID=mid;Note=x", b"Name=none", b"ID=;Name=empty",
                                             b"fooID=inside;Name=n", b"Name=n;ID=last"))
    ids = [r.split(b"\t")[3] for r in check(ctx, "gff", body).split(b"\n")[:-1]]
    assert ids == [b"first", b"mid", b".", b".", b".", b"last"]
    junk = b">chr1 some\ttext\nACGT\nchr1\tx\ty\t0\t0\n"              # errors, were it parsed
    with pytest.raises(oracle.ConvertError):
        oracle.gff(junk)
    for kw in ({}, dict(keep_header=True)):
        assert check(ctx, "gff", b"##FASTA\n" + body + junk, **kw) == b""
        assert check(ctx, "gff", b"#h\n" + body + b"##FASTA\n" + junk, **kw).count(b"\n") == 6 + len(kw)
        assert check(ctx, "gff", b"#h\n" + body + b"##FASTA", **kw).count(b"\n") == 6 + len(kw)
        assert check(ctx, "gff", b"#h\n" + body + b"#t\n", **kw).count(b"\n") == 6 + 2 * len(kw)
        assert check(ctx, "gff", body + b"##FASTA\n" + junk + b"##FASTA\n" + junk, **kw).count(b"\n") == 6
    st = ctx.convert_stats()
    assert (st["input_lines"], st["header_lines"], st["data_lines"]) == (6 + 2 + 2 * 3, 0, 6)


def test_gtf_gene_id(ctx):
    body = b"".join(G + a + b"\n" for a in (b'gene_id "first"; transcript_id "t";', b'transcript_id "t"; gene_id "after";',
                                             b'transcript_id "t";', b'other_gene_id "x"; gene_id "real";', b'gene_id "";',
                                             b'a "b";gene_id "tight"', b'gene_id "open'))
    ids = [r.split(b"\t")[3] for r in check(ctx, "gtf", body + b"##FASTA\n", keep_header=True).split(b"\n")[:-1]]
    assert ids == [b"first", b"after", b".", b"real", b".", b"tight", b".", b"##FASTA"]


# ---- VCF --------------------------------------------------------------------------------
def test_vcf_fields_and_allele_classes(ctx):
    eight = b"c1\t100\trs1\tACG\tA,ACGT,TTT,AC,GGGGG,CCC\t50\tPASS\tDP=9"
    twelve = eight.replace(b"c1", b"c0") + b"\tGT:GQ\t0|1:9\t1|1:8\t0|0:7"
    none = b"c2\t5\t.\tA\tG,T\t.\t.\tX"                              # snvs only
    for data in (b"\n".join(rows) + b"\n" for rows in ((eight, twelve), (none, eight, twelve), (eight, none, twelve),
                                                      (twelve, eight, none), (none, none))):
        n = {c: check(ctx, "vcf", data, vcf_class=c).count(b"\n") for c in ("all", "snvs", "insertions", "deletions")}
        rec, k, z = data.count(b"\n"), data.count(b"ACG\t"), data.count(none)
        assert n == dict(all=rec, snvs=2 * k + 2 * z, insertions=2 * k, deletions=2 * k), (data, n)
    out = check(ctx, "vcf", twelve, vcf_class="insertions")
    assert out == b"c0\t99\t102\trs1\t50\tACG\tACGT\tPASS\tDP=9\tGT:GQ\t0|1:9\t1|1:8\t0|0:7\n" \
                  b"c0\t99\t102\trs1\t50\tACG\tGGGGG\tPASS\tDP=9\tGT:GQ\t0|1:9\t1|1:8\t0|0:7\n"


# ---- WIG: the carried state ---------------------------------------------------------------
def test_wig_one_declaration_over_four_blocks(ctx, TW):
    T, _ = TW
    data = b"fixedStep chrom=chr7 start=100 step=7 span=3\n" + b"".join(b"%d.5\n" % k for k in range(3 * T + 4))
    assert data.count(b"\n") == 3 * T + 5
    want = check(ctx, "wig", data)
    last = 99 + 7 * (3 * T + 3)
    assert want.endswith(b"chr7\t%d\t%d\tid-%d\t%d.5\n" % (last, last + 3, 3 * T + 4, 3 * T + 3))


def test_wig_declarations_at_the_block_edges(ctx, TW):
    T, _ = TW
    rows, mode = [], None
    for k in range(2 * T + 3):
        if k in (0, T - 1, T, T + 1, T + 40, T + 41):                # T, T + 1 and T + 40, T + 41: back to back, no data between
            mode = "vf"[len([r for r in rows if b"Step" in r]) % 2]
            rows.append(b"variableStep chrom=v%d span=%d" % (k, k + 1) if mode == "v" else b"fixedStep chrom=f%d start=%d step=3" % (k, k + 1))
        else:
            rows.append(b"%d 1.%d" % (1000 - k, k) if mode == "v" else b"0.%d" % k)
    data = b"\n".join(rows) + b"\n"
    assert [k for k, r in enumerate(rows) if b"Step" in r] == [0, T - 1, T, T + 1, T + 40, T + 41]
    want = check(ctx, "wig", data)
    assert {r.split(b"\t")[0] for r in want.split(b"\n")[:-1]} == {b"v0", b"f%d" % (T + 1), b"f%d" % (T + 41)}
    assert ctx.convert_stats()["declarations"] == 6


def test_wig_mixed_sections_headers_and_key_orders(ctx):
    data = (b"fixedStep chrom=a start=10 step=5 span=2\n1\n2\n"
            b"variableStep chrom=b span=4\n7 x\n9 y\n"
            b"c 100 200 z\nc 5 6 w\n"
            b"fixedStep chrom=a start=50\n3\nq 1 2 four\n4\ntrack name=mid\nq\t3\t4\tfour\n\n5\n#c\n6\n")
    want = check(ctx, "wig", data)
    assert want.split(b"\n")[-5:-1] == [b"a\t50\t51\tid-9\t4", b"q\t3\t4\tid-10\tfour", b"a\t51\t52\tid-11\t5", b"a\t52\t53\tid-12\t6"]
    kept = check(ctx, "wig", data, keep_header=True)
    assert kept.count(b"_header\t") == 3 and b"_header\t0\t1\ttrack name=mid\n" in kept
    keys = (b"chrom=k", b"start=9", b"step=4", b"span=3")
    for order in itertools.permutations(keys):
        assert check(ctx, "wig", b"fixedStep \t" + b"\t ".join(order) + b" \n1\n2\n") == b"k\t8\t11\tid-1\t1\nk\t12\t15\tid-2\t2\n"
    for order in itertools.permutations((b"chrom=k", b"span=3")):
        assert check(ctx, "wig", b"variableStep " + b" ".join(order) + b"\n9 1\n") == b"k\t8\t11\tid-1\t1\n"


# ---- errors ---------------------------------------------------------------------------------
def test_the_lowest_bad_line_is_named(ctx, TW):
    T, _ = TW
    rows = gff_rows(2 * T + 10)
    rows[2 * T + 2] = G[:-1]                                      # line 2T + 3: eight fields
    rows[4] = rows[4].replace(b"\t.\tID", b"\t.\t.\tID")          # line 5: ten fields
    check_error(ctx, "gff", b"\n".join(rows) + b"\n", 5, oracle.E_MANY)
    rows[4] = G + b"ID=fine"
    check_error(ctx, "gff", b"\n".join(rows) + b"\n", 2 * T + 3, oracle.E_FEW)
    rows = vcf_rows(2 * T + 10)
    rows[2 * T + 2] = b"c\t0\t.\tA\tG\t9\tq\tI"
    rows[4] = b"c\t5\t.\tA\tG,\t9\tq\tI"
    check_error(ctx, "vcf", b"\n".join(rows), 5, oracle.E_ALLELE, vcf_class="snvs")
    check_error(ctx, "vcf", b"\n".join(rows), 2 * T + 3, oracle.E_ZERO)


def test_wig_state_errors(ctx, TW):
    T, _ = TW
    check_error(ctx, "wig", b"#c\n0.5\nfixedStep chrom=c start=1\n", 2, oracle.E_NODECL)
    check_error(ctx, "wig", b"c 1 2 x\n7 0.5\nvariableStep chrom=c\n", 2, oracle.E_NODECL)
    check_error(ctx, "wig", b"variableStep chrom=c\n7 1\n0.5\n8 1\n", 3, oracle.E_MISFIT)
    check_error(ctx, "wig", b"fixedStep chrom=c start=1\n1\nvariableStep chrom=c\n" + b"5 1\n" * T + b"1\n", T + 4, oracle.E_MISFIT)
    check_error(ctx, "wig", b"fixedStep chrom=c start=1 step=x\n1\n", 1, oracle.E_VALUE)
    # start - 1 + k * step + span first exceeds 2^63-1 at data line k = T + 11: line T + 13, in the second block
    data = b"fixedStep chrom=c start=%d\n" % (LIMIT - (T + 10)) + b"1\n" * (T + 20)
    check_error(ctx, "wig", data, T + 13, oracle.E_OVER)
    ok = b"fixedStep chrom=c start=%d\n" % (LIMIT - (T + 10)) + b"1\n" * (T + 11)
    assert check(ctx, "wig", ok).endswith(b"c\t%d\t%d\tid-%d\t1\n" % (LIMIT - 1, LIMIT, T + 11))
    check_error(ctx, "wig", b"variableStep chrom=c\n12345678901234567890 1\n", 2, oracle.E_RANGE)
    check_error(ctx, "gff", G.replace(b"20", b"10000000000000000000") + b"x\n", 1, oracle.E_RANGE)


# ---- chaining in HBM ----------------------------------------------------------------------
def test_convert_device_then_bedmap_and_closest(ctx):
    import torch
    data = oracle.random_input("gff", random.Random(99), 300)
    want = oracle.sort_bed(oracle.gff(data))
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    n = ctx.convert_device(dev.data_ptr(), len(data), "gff")
    assert n == len(want) and ctx._output() == want
    st = ctx.convert_stats()
    lines, hdr, rec, dec = oracle.counts("gff", data)
    assert (st["input_bytes"], st["input_lines"], st["header_lines"], st["data_lines"], st["declarations"], st["lines_out"],
            st["output_bytes"], st["sorted"]) == (len(data), lines, hdr, rec, 0, rec, len(want), 1)
    ptr = ctx.output_device_ptr()
    cut = want.index(b"\n", len(want) // 2) + 1
    ctx.bedmap_device(ptr, [0, cut, n], cols=("echo", "count", "bases"))
    assert ctx._output() == ctx.bedmap(want[:cut], want[cut:], cols=("echo", "count", "bases"))
    n = ctx.convert_device(dev.data_ptr(), len(data), "gff", keep_header=True, sort=False)
    assert ctx._output() == oracle.gff(data, keep_header=True) and ctx.convert_stats()["sorted"] == 0
    n = ctx.convert_device(dev.data_ptr(), len(data), "gff")
    ctx.closest_device(ctx.output_device_ptr(), [0, cut, n], dist=True)
    assert ctx._output() == ctx.closest_features(want[:cut], want[cut:], dist=True)
    wig = oracle.random_input("wig", random.Random(5), 200)
    dev = torch.frombuffer(bytearray(wig), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    ctx.convert_device(dev.data_ptr(), len(wig), "wig", sort=False)
    st = ctx.convert_stats()
    lines, hdr, rec, dec = oracle.counts("wig", wig)
    assert dec > 3 and (st["input_lines"], st["header_lines"], st["data_lines"], st["declarations"], st["lines_out"]) == \
        (lines, hdr, rec, dec, rec)


# ---- the command ------------------------------------------------------------------------------
def _cli(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_command_against_the_oracle(tmp_path):
    rng = random.Random(3)
    gff, vcf, wig = (oracle.random_input(f, rng, 120) for f in ("gff", "vcf", "wig"))
    for name, blob in (("a.gff", gff), ("a.vcf", vcf), ("a.wig", wig)):
        (tmp_path / name).write_bytes(blob)
    r = _cli([CONVERT, "--input=gff", str(tmp_path / "a.gff")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == oracle.sort_bed(oracle.gff(gff))
    with open(tmp_path / "a.vcf", "rb") as f:
        r = _cli([CONVERT, "--input=VCF", "--snvs", "-"], stdin=f)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == oracle.sort_bed(oracle.vcf(vcf, "snvs")) and r.stdout
    r = _cli([CONVERT, "--input=wig", "--output=starch", str(tmp_path / "a.wig")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout[:4] == b"\xca\x5c\xad\x1a"
    (tmp_path / "a.starch").write_bytes(r.stdout)
    r = _cli([os.path.join(BUILD, "unstarch"), str(tmp_path / "a.starch")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == oracle.sort_bed(oracle.wig(wig))
    r = _cli([CONVERT, "--input=wig", "--do-not-sort", "--keep-header", str(tmp_path / "a.wig")])
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == oracle.wig(wig, keep_header=True)
    (tmp_path / "bad.gff").write_bytes(gff + G[:-1] + b"\n")
    r = _cli([CONVERT, "--input=gff", str(tmp_path / "bad.gff")])
    assert r.returncode == 22 and r.stdout == b"" and b"convert2bed: line %d: " % (gff.count(b"\n") + 1) in r.stderr
