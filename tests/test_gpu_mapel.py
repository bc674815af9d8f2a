"""GPU: bedmap-elements (Starch.map_elements, map_elements_device, the
bedmap-elements command).

Every comparison is equality of whole outputs against tests/mapel_oracle.py or
literal bytes.  T is the number of reference lines per workgroup, F the fan-out
of the hierarchy of maxima over the map stops, HEAVY the run of candidates from
which a whole wave tests them, BOUND the bound on walk_steps per reference line
and per hit; all four are read from mapel_constants().
"""
import os
import random
import subprocess

import pytest

from tests import mapel_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPEL = os.path.join(ROOT, "starch_amd", "_build", "bedmap-elements")
CRITS = (("bp_ovr", 1), ("bp_ovr", 3), ("range", 7), ("fraction_ref", "0.5"), ("fraction_map", "0.25"),
         ("fraction_both", "0.1"), ("fraction_either", "0.75"), ("exact",))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def K():
    import starch_amd
    return starch_amd.mapel_constants()


def bed(rows, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % ((chrom,) + tuple(r) if len(r) == 2 else tuple(r)) for r in rows)


def check(ctx, ref, mp=None, **kw):
    got = ctx.map_elements(ref, mp, **kw)
    assert got == oracle.mapel(ref, mp, **kw), kw
    return got


def random_bed(rng, chroms, lines, limit=300, lengths=(1, 2, 7, 40, 200)):
    rows = []
    for k in range(lines):
        s = rng.randrange(0, limit - 2)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths))), k, rng.randrange(1000)))
    return b"".join(b"%s\t%d\t%d\tn%d\t%d\n" % r for r in sorted(rows))


@pytest.fixture(scope="module")
def pair():
    rng = random.Random(1)
    return random_bed(rng, [b"chr1", b"chr2"], 400), random_bed(rng, [b"chr1", b"chr2", b"chr3"], 500)


# ---- 1. table, criteria, columns, shapes -------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_hand_written_table(ctx, case):
    ref, mp, kw, want = oracle.TABLE[case]
    assert ctx.map_elements(ref, mp, **kw) == want


@pytest.mark.parametrize("crit", CRITS, ids=lambda c: "-".join(map(str, c)))
def test_every_criterion_with_every_column(ctx, pair, crit):
    r, m = pair
    for col in oracle.COLS:
        check(ctx, r, m, cols=(col,), criterion=crit)
    check(ctx, r, m, cols=oracle.COLS, criterion=crit)
    check(ctx, r, m, cols=oracle.COLS[::-1], criterion=crit, skip_unmapped=True, delim=b"<=delim>", multidelim=b", ")
    check(ctx, r, None, cols=("echo_ref_row_id", "count", "echo_map_id", "echo_overlap_size", "echo_map_range"), criterion=crit)


def test_shapes_and_stats(ctx, pair):
    r, m = pair
    a, q = bed([(1, 5), (9, 12)]), bed([(4, 10), (20, 30)])
    assert ctx.map_elements(b"", q) == b""
    s = ctx.mapel_stats()
    assert (s["n_ref"], s["n_map"], s["hits"], s["lines_out"], s["output_bytes"]) == (0, 2, 0, 0, 0)
    assert ctx.map_elements(b"", b"") == b"" and ctx.map_elements(b"") == b""
    assert ctx.map_elements(a, b"") == b"chr1\t1\t5|\nchr1\t9\t12|\n"
    assert ctx.map_elements(a, q) == b"chr1\t1\t5|chr1\t4\t10\nchr1\t9\t12|chr1\t4\t10\n"
    # a last line without '\n', in either input: the inputs must not fuse, and the echo ends at the line
    want = oracle.mapel(a, q, cols=("echo", "echo_map", "count"))
    for x, y in ((a[:-1], q), (a, q[:-1]), (a[:-1], q[:-1])):
        assert ctx.map_elements(x, y, cols=("echo", "echo_map", "count")) == want
    assert ctx.map_elements(a[:-1], cols=("echo_map",)) == b"chr1\t1\t5\nchr1\t9\t12\n"
    # a reference line shorter than 30 bases has no hit under --bp-ovr 30, so skip_unmapped leaves lines out
    got = check(ctx, r, m, cols=("echo", "count"), criterion=("bp_ovr", 30), skip_unmapped=True)
    s = ctx.mapel_stats()
    lists = oracle.hits_brute(oracle.parse(r), oracle.parse(m), ("bp_ovr", 30))
    assert (s["n_ref"], s["n_map"], s["n_chromosomes"]) == (400, 500, 3)
    assert s["hits"] == sum(map(len, lists)) and s["lines_out"] == got.count(b"\n") == sum(bool(h) for h in lists)
    assert 0 < s["lines_out"] < 400
    assert s["output_bytes"] == s["out_bytes"] == len(got) and s["walk_steps"] > 0
    assert all(s[k] >= 0 for k in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_format")) and s["ms_total"] > 0


def test_random_dense_cases(ctx):
    names = [b"c", b"ch", b"chr", b"chr1"]
    for seed in range(120):
        rng = random.Random(7000 + seed)
        ref = random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(1, 80))
        mp = None if seed % 9 == 0 else random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(0, 80))
        kw = dict(cols=rng.sample(oracle.COLS, rng.randint(1, 12)), criterion=rng.choice(CRITS), skip_unmapped=rng.random() < 0.3)
        assert ctx.map_elements(ref, mp, **kw) == oracle.mapel(ref, mp, **kw), (seed, kw)


# ---- 2. the hierarchy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 2, 3))
def test_map_sizes_around_the_powers_of_the_fanout(ctx, K, k):
    F = K[1]
    for n in (F ** k - 1, F ** k, F ** k + 1):
        shorts = [(10 + 4 * i, 12 + 4 * i) for i in range(n - 1)]           # disjoint, gaps of 2
        big = 4 * n + 100
        pos = sorted(set(p for i in (0, 1, F - 1, F, F + 1, n // 2, n - 3, n - 2) if 0 <= i < n - 1
                         for p in (10 + 4 * i, 11 + 4 * i, 12 + 4 * i, 13 + 4 * i)))
        ref = bed(sorted([(p, p + 1) for p in pos] + [(0, 5), (12, big + 9), (big - 1, big), (big, big + 3)]))
        for at in sorted(set((0, min(F, n - 1), n - 1))):                   # the spanning line first, at a tile edge, last
            rows = shorts[:at] + [(9 + 4 * at, big)] + shorts[at:]
            mp = bed(rows)
            got = check(ctx, ref, mp, cols=("echo_ref_name", "count", "echo_map"))
            assert ctx.mapel_stats()["n_map"] == n
            if at == 0:
                assert b"chr1:12-13|1|chr1\t9\t%d\n" % big in got              # a gap: the spanning line alone
            check(ctx, ref, mp, cols=("count", "echo_map_size"), criterion=("bp_ovr", 2))
            check(ctx, ref, mp, cols=("count", "echo_overlap_size"), criterion=("range", 3))


def test_a_chromosome_before_shares_the_tile(ctx, K):
    F = K[1]
    # chr1's stops are far above chr2's: an item of maxima that spans both must not answer for chr2
    for n1 in (1, F - 1, F, F + 1, F * F + 3):
        mp = bed([(i, 10 ** 9 + i) for i in range(n1)], b"chr1") + bed([(5 * i, 5 * i + 2) for i in range(2 * F + 3)], b"chr2")
        ref = bed([(3, 4), (8, 9), (5 * F + 1, 5 * F + 2), (5 * F + 3, 5 * F + 4), (10 ** 6, 10 ** 6 + 1)], b"chr2")
        check(ctx, ref, mp, cols=("echo", "count", "echo_map"))
        check(ctx, bed([(1, 10 ** 9 + 7)], b"chr1") + ref, mp, cols=("count", "echo_map_range"))
        check(ctx, mp, mp, cols=("count",), criterion=("fraction_map", "1"))


def test_bounded_work(ctx, K):
    T, F, HEAVY, BOUND = K
    mp = bed([(0, 10 ** 6)] + [(100 + 10 * i, 105 + 10 * i) for i in range(4096)])
    ref = bed([(100 + 10 * i, 105 + 10 * i) for i in range(4096 - 64, 4096)])
    got = check(ctx, ref, mp, cols=("count", "echo_map"))
    s = ctx.mapel_stats()
    assert (s["n_ref"], s["n_map"], s["hits"]) == (64, 4097, 128) and got.count(b"2|chr1\t0\t1000000;chr1\t") == 64
    assert s["walk_steps"] <= BOUND * (s["n_ref"] + s["hits"])
    assert s["walk_steps"] < 64 * 4096 // 4           # a linear walk needs 64 * 4032 probes at least


# ---- 3. reference tiles, the whole-wave path -------------------------------------------------------------------
def test_reference_sizes_around_a_tile(ctx, K):
    T = K[0]
    rng = random.Random(3)
    mp = random_bed(rng, [b"chr1", b"chr2"], 900, limit=4000)
    for n in (T - 1, T, T + 1):
        n1 = n // 2 + 3                                                    # the chromosome changes inside the tile
        ref = random_bed(rng, [b"chr1"], n1, limit=4000) + random_bed(rng, [b"chr2"], n - n1, limit=4000)
        check(ctx, ref, mp, cols=("echo", "count", "echo_map_id"))
        assert ctx.mapel_stats()["n_ref"] == n
        check(ctx, ref, mp, cols=("count", "echo_map_score"), criterion=("fraction_either", "0.5"))


def test_heavy_lines_take_the_wave_path(ctx, K):
    HEAVY = K[2]
    for cnt in (HEAVY - 1, HEAVY, HEAVY + 65):
        # map lines of 1 and 2 bases in turn: every other one fails --bp-ovr 2
        mp = bed([(50, 60), (90, 101)] + [(100 + 3 * k, 101 + 3 * k + k % 2) for k in range(cnt)] + [(100 + 3 * cnt, 9000)])
        ref = bed([(20, 30), (100, 100 + 3 * cnt), (100 + 3 * cnt, 100 + 3 * cnt + 1)])
        got = check(ctx, ref, mp, cols=("count", "echo_map_size", "echo_map_range"), criterion=("bp_ovr", 2))
        s = ctx.mapel_stats()
        assert s["heavy_lines"] == (1 if cnt >= HEAVY else 0), cnt
        assert got.split(b"\n")[1].startswith(b"%d|2;2;" % (cnt // 2))
        check(ctx, ref, mp, cols=("echo_ref_row_id", "echo_map", "echo_overlap_size"))      # with the spanning (90, 101) ahead
        assert ctx.mapel_stats()["heavy_lines"] == (1 if cnt >= HEAVY else 0)
    # two heavy lines in one wave, and one in the next tile's wave
    mp = bed([(10 * k, 10 * k + 3) for k in range(3 * HEAVY)])
    ref = bed([(0, 10 * HEAVY), (5, 10 * HEAVY + 5)] + [(10 * HEAVY + 7, 10 * HEAVY + 8)] * K[0] + [(10 * HEAVY + 9, 30 * HEAVY)])
    check(ctx, ref, mp, cols=("count", "echo_map_size", "echo_map_range"), criterion=("fraction_map", "1"))
    assert ctx.mapel_stats()["heavy_lines"] == 3


def test_lines_and_hits_left_to_the_wave(ctx):
    import starch_amd
    from tests import wave_lines
    W = starch_amd.sort_constants()[1]
    # reference line k has the one hit k: long echoes and long hits at lanes 0 and 63 of the first wave
    # and lane 0 of the third, then none at all
    for r, m in wave_lines.wave_pairs(W):
        check(ctx, r, m, cols=("echo", "echo_map"))
        assert ctx.mapel_stats()["hits"] == wave_lines.WAVE_LINES
        check(ctx, r, m, cols=("echo_map", "count", "echo"), delim=b"<=>", multidelim=b", ")
    # the id and the score of a hit long too: all three slots of one lane
    spots = wave_lines.WAVE_SPOTS
    m = b"".join(b"chr1\t%d\t%d\t%s\t%s\n" % (10 * k + 1, 10 * k + 3, b"i" * (W + 5 if k in spots else 4), b"7" * (W + 9 if k in spots else 2))
                 for k in range(wave_lines.WAVE_LINES))
    check(ctx, wave_lines.lines(wave_lines.WAVE_LINES, spots, W), m, cols=("echo", "echo_map", "echo_map_id", "echo_map_score"))
    # two hits per reference line: every piece after the first follows its multi-delimiter
    check(ctx, wave_lines.lines(wave_lines.WAVE_LINES // 2, (), W, width=15), m, cols=("echo_map_id", "echo_map"), multidelim=b"<;>")


def test_long_map_lines_are_copied_by_the_wave(ctx):
    import starch_amd
    W = starch_amd.sort_constants()[1]
    tail = (bytes(range(48, 123)) * 9)[:2 * W + 11]
    mp = b"chr1\t9\t12\t" + tail + b"\t7\nchr1\t10\t13\tshort\t8\nchr1\t11\t60\tid\t" + tail[::-1] + b"\n" + \
        b"chr1\t50\t60\t" + tail[:W - 12] + b"\n"
    ref = bed([(1, 5), (10, 11), (11, 12), (55, 56)])
    check(ctx, ref, mp, cols=("echo", "echo_map"))
    check(ctx, ref, mp, cols=("echo_map_id", "count", "echo_map"))
    check(ctx, bed([(1, 5), (10, 11), (11, 12)]), mp, cols=("echo_map_score", "echo_map_id"))
    check(ctx, mp, None, cols=("echo", "echo_map"), criterion=("exact",))


# ---- 4. wide coordinates ------------------------------------------------------------------------------------------
def test_wide_coordinates(ctx):
    top = 2 ** 63 - 1
    mp = bed([(0, 1), (5, top), (top - 1, top)])
    ref = bed([(3, 4), (top - 3, top - 2)])
    for r in (top, 2 ** 64 - 1, 2 ** 63 + 5):                              # the window saturates at both ends
        got = check(ctx, ref, mp, cols=("count", "echo_overlap_size"), criterion=("range", r))
        assert got.startswith(b"3|1;%d;1\n" % (top - 5))
    check(ctx, ref, mp, cols=("count", "echo_map_size", "echo_map_range"))
    # a product of more than 64 bits: ov = 2^40 of a reference line of 2^41 bases, nine digits
    ref = bed([(0, 2 ** 41)])
    mp = bed([(2 ** 40, 2 ** 42)])
    assert ctx.map_elements(ref, mp, cols=("count",), criterion=("fraction_ref", "0.500000000")) == b"1\n"
    assert ctx.map_elements(ref, mp, cols=("count",), criterion=("fraction_ref", "0.500000001")) == b"0\n"
    assert ctx.map_elements(ref, mp, cols=("count",), criterion=("fraction_ref", "0.499999999")) == b"1\n"
    mp = bed([(2 ** 40 + 1, 2 ** 42)])
    assert ctx.map_elements(ref, mp, cols=("count",), criterion=("fraction_ref", "0.500000000")) == b"0\n"
    assert ctx.map_elements(ref, mp, cols=("count",), criterion=("fraction_ref", "0.499999999")) == b"1\n"
    big = bed([(2 ** 62, top)])
    for f in ("1", "0.999999999", "0.000000001"):
        for kind in ("fraction_ref", "fraction_map", "fraction_both", "fraction_either"):
            check(ctx, big, bed([(2 ** 62 + 5, top), (2 ** 62 + 2 ** 61, top)]), cols=("count", "echo_overlap_size"), criterion=(kind, f))
            check(ctx, big, big, cols=("count",), criterion=(kind, f))


# ---- 5. errors ------------------------------------------------------------------------------------------------------------
def _refused(ctx, ref, mp, code, *words, **kw):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.map_elements(ref, mp, **kw)
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    assert ctx.map_elements(bed([(1, 2)]), bed([(1, 6)])) == b"chr1\t1\t2|chr1\t1\t6\n"   # works again


def test_errors(ctx):
    hi, lo = bed([(500, 600), (700, 800)]), bed([(1, 2), (3, 4), (2, 9), (0, 1)])
    _refused(ctx, lo, hi, -12, "bedmap-elements: input 0, line 3:", "sort-bed")
    _refused(ctx, hi, lo, -12, "bedmap-elements: input 1, line 3:", "sort-bed")
    _refused(ctx, hi, bed([(1, 2), (5, 5)]), -12, "input 1, line 2:", "stop")
    _refused(ctx, lo, b"chr1\t1\t2\nchr1\t5\n", -12, "input 1, line 2:", "fewer than three")   # malformed goes first
    _refused(ctx, b"chr1\t1\t2\n\nchr1\t5\t6\n", None, -12, "input 0, line 2:", "empty line")
    # a hit without column 4 or 5; the same line as a non-hit is accepted
    mp = b"chr1\t1\t5\ta\t1\nchr1\t20\t30\nchr1\t40\t50\tc\nchr1\t60\t70\td\t\n"
    near, far = bed([(2, 3), (25, 26), (45, 46)]), bed([(2, 3), (65, 66)])
    _refused(ctx, near, mp, -12, "bedmap-elements: input 1, line 2:", cols=("echo_map_id",))
    _refused(ctx, near, mp, -12, "bedmap-elements: input 1, line 2:", cols=("echo_map_score",))
    _refused(ctx, bed([(2, 3), (45, 46)]), mp, -12, "input 1, line 3:", cols=("echo_map_id", "echo_map_score"))
    _refused(ctx, mp, None, -12, "bedmap-elements: input 0, line 2:", cols=("echo_map_id",))
    assert ctx.map_elements(bed([(2, 3), (45, 46)]), mp, cols=("echo_map_id",)) == b"a\nc\n"
    assert ctx.map_elements(far, mp, cols=("echo_map_id", "echo_map_score")) == b"a|1\nd|\n"
    assert ctx.map_elements(near, mp, cols=("echo_map", "echo_map_size")) == oracle.mapel(near, mp, cols=("echo_map", "echo_map_size"))
    with pytest.raises(oracle.MissingColumn) as e:
        oracle.mapel(near, mp, cols=("echo_map_score",))
    assert e.value.line == 2
    import starch_amd
    for kw in (dict(delim=b""), dict(multidelim=b"123456789"), dict(cols=()), dict(cols=("echo", "echo")),
               dict(criterion=("bp_ovr", 0))):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.map_elements(hi, hi, **kw)
        assert e.value.code == -2, kw
    assert ctx.map_elements(bed([(1, 2)]), bed([(1, 6)])) == b"chr1\t1\t2|chr1\t1\t6\n"


# ---- 6. archives, device entry, command, bedmap ---------------------------------------------------------------------------------
def test_archives(ctx, pair):
    import starch_amd
    r, m = pair
    ar, am = ctx.compress(r), ctx.compress(m)
    assert ar[:4] == b"\xca\x5c\xad\x1a"
    kw = dict(cols=("echo", "count", "echo_map_id"), criterion=("fraction_either", "0.5"))
    want = check(ctx, r, m, **kw)
    assert ctx.map_elements(ar, m, **kw) == ctx.map_elements(r, am, **kw) == ctx.map_elements(ar, am, **kw) == want
    assert ctx.map_elements(ar, None, **kw) == oracle.mapel(r, None, **kw)
    ctx.set_compression_method(starch_amd.K_GZIP)
    try:
        gz = ctx.compress(m)
    finally:
        ctx.set_compression_method(starch_amd.K_BZIP2)
    for a, b in ((r, gz), (gz, r), (gz, None)):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.map_elements(a, b)
        assert e.value.code == -2 and "gzip" in str(e.value)
    assert ctx.map_elements(ar, am, **kw) == want


def test_device_entry(ctx, pair):
    import torch
    r, m = pair
    kw = dict(cols=("echo_ref_row_id", "echo_map", "echo_overlap_size"), criterion=("range", 11))
    want = check(ctx, r, m, **kw)
    blob = r[:-1] + m                                          # the reference without its final newline
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    k = ctx.map_elements_device(dev.data_ptr(), [0, len(r) - 1, len(blob)], **kw)
    assert k == len(want) and ctx.output_device_ptr() != 0 and ctx._output() == want
    k = ctx.map_elements_device(dev.data_ptr(), [0, len(r) - 1], **kw)      # the reference as its own map
    assert ctx._output() == oracle.mapel(r, None, **kw) and k == len(ctx._output())
    k = ctx.map_elements_device(dev.data_ptr(), [0, len(r) - 1, len(r) - 1], **kw)      # an empty map
    assert ctx._output() == oracle.mapel(r, b"", **kw)


def test_command(ctx, pair, tmp_path):
    r, m = pair
    fr, fm, fs = tmp_path / "ref.bed", tmp_path / "map.bed", tmp_path / "map.starch"
    fr.write_bytes(r)
    fm.write_bytes(m)
    fs.write_bytes(ctx.compress(m))

    def run(args, **kw):
        return subprocess.run([MAPEL] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)
    p = run([str(fr), str(fm)])
    assert p.returncode == 0 and p.stdout == ctx.map_elements(r, m)
    want = ctx.map_elements(r, m, cols=("echo_ref_name", "count", "echo_map_id", "echo_map_score"), criterion=("fraction_map", ".5"),
                            skip_unmapped=True, delim=b"\t", multidelim=b",")
    p = run(["--echo-ref-name", "--count", "--echo-map-id", "--echo-map-score", "--fraction-map", ".5", "--skip-unmapped",
             "--delim", "\t", "--multidelim", ",", "-", str(fs)], input=r)
    assert p.returncode == 0 and p.stdout == want
    p = run(["--exact", "--indicator", "--echo-map-range", str(fm)])
    assert p.returncode == 0 and p.stdout == ctx.map_elements(m, None, cols=("indicator", "echo_map_range"), criterion=("exact",))
    fu = tmp_path / "unsorted.bed"
    fu.write_bytes(bed([(5, 6), (1, 2)]))
    p = run(["--count", str(fr), str(fu)])
    assert p.returncode == 22 and p.stdout == b"" and b"bedmap-elements: input 1, line 2:" in p.stderr
    fn = tmp_path / "noid.bed"
    fn.write_bytes(bed([(0, 10 ** 6)]))
    p = run(["--echo-map-id", str(fr), str(fn)])
    assert p.returncode == 22 and p.stdout == b"" and b"bedmap-elements: input 1, line 1:" in p.stderr


def test_counts_agree_with_bedmap(ctx, pair):
    r, m = pair
    assert ctx.map_elements(r, m, cols=("count",)) == ctx.bedmap(r, m, cols=("count",))
    for n in (0, 1, 25):
        assert ctx.map_elements(r, m, cols=("echo", "count", "indicator", "echo_ref_size"), criterion=("range", n)) == \
            ctx.bedmap(r, m, cols=("echo", "count", "indicator", "echo_ref_size"), range=n)
    assert ctx.map_elements(r, cols=("count",), skip_unmapped=True) == ctx.bedmap(r, cols=("count",), skip_unmapped=True)
