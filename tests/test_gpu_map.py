"""GPU: bedmap (Starch.bedmap, bedmap_device, the bedmap command).

Every comparison is equality of whole outputs against tests/map_oracle.py: the
bitmap oracle where the coordinates are below 4096, the pairs oracle otherwise,
or literal bytes.  T is the number of reference lines per query workgroup (a
window into the map arrays is found once per workgroup and chromosome), W the
largest window staged in LDS (0: no such path).
"""
import os
import random
import subprocess

import pytest

from tests import map_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEDMAP = os.path.join(ROOT, "starch_amd", "_build", "bedmap")
ALL = oracle.COLS
NUM = ("count", "bases", "bases_uniq", "indicator", "echo_ref_size")

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
    return starch_amd.map_constants()


def bed(rows, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % ((chrom,) + tuple(r) if len(r) == 2 else tuple(r)) for r in rows)


def check(ctx, ref, mp, ref_fn=oracle.bitmap, **kw):
    kw.setdefault("cols", ALL)
    got = ctx.bedmap(ref, mp, **kw)
    assert got == ref_fn(ref, mp, **kw), kw
    return got


def random_bed(rng, chroms, lines, limit=4096, lengths=(1, 2, 7, 40, 600)):
    rows = []
    for _ in range(lines):
        s = rng.randrange(0, limit - 2)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit, s + rng.choice(lengths)))))
    return bed(sorted(rows))


# ---- 1. table and shapes ---------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_hand_written_table(ctx, case):
    ref, mp, kw, want = oracle.TABLE[case]
    assert ctx.bedmap(ref, mp, **kw) == want


def test_shapes(ctx):
    a, m = bed([(1, 5), (9, 12)]), bed([(4, 10), (20, 30)])
    assert ctx.bedmap(b"", m, cols=ALL) == b""
    assert ctx.map_stats()["n_ref"] == 0 and ctx.map_stats()["lines_out"] == 0
    assert ctx.bedmap(b"", b"") == b"" and ctx.bedmap(b"") == b""
    assert ctx.bedmap(a, b"", cols=ALL) == b"chr1\t1\t5|0|0|0|0|4\nchr1\t9\t12|0|0|0|0|3\n"
    assert ctx.bedmap(a, m) == b"chr1\t1\t5|1\nchr1\t9\t12|1\n"          # the default columns
    # the map omitted: every line overlaps itself
    rng = random.Random(1)
    r = random_bed(rng, [b"chr1", b"chr2"], 700)
    got = check(ctx, r, None)
    assert all(int(ln.split(b"|")[1]) >= 1 for ln in got.split(b"\n")[:-1])
    assert ctx.map_stats()["n_map"] == ctx.map_stats()["n_ref"] == 700
    # a last line without '\n', in either input: the inputs must not fuse
    assert ctx.bedmap(a[:-1], m, cols=ALL) == ctx.bedmap(a, m, cols=ALL) == oracle.bitmap(a, m, cols=ALL)
    assert ctx.bedmap(a, m[:-1], cols=ALL) == oracle.bitmap(a, m, cols=ALL)
    assert ctx.bedmap(a[:-1], None, cols=ALL) == oracle.bitmap(a, None, cols=ALL)
    # extra columns are echoed verbatim, empty and space-holding fields too
    wide = b"chr1\t1\t5\tname\t0\t+\nchr1\t9\t12\t\t\nchr2\t3\t4\tx y  z\t\n"
    assert ctx.bedmap(wide, m, cols=("count", "echo")) == \
        b"1|chr1\t1\t5\tname\t0\t+\n1|chr1\t9\t12\t\t\n0|chr2\t3\t4\tx y  z\t\n"
    check(ctx, wide, wide)
    # an echoed line long enough for the whole-wave copy, among short ones
    long_ = b"chr1\t9\t12\t" + bytes(range(48, 123)) * 9 + b"\n"
    check(ctx, bed([(1, 5)]) + long_ + long_.replace(b"\t9\t", b"\t10\t") + bed([(11, 13)]), m)
    # every single column, and a mixed order
    for c in ALL:
        check(ctx, r, m, cols=(c,))
    check(ctx, r, m, cols=("bases_uniq", "echo_ref_size", "echo", "indicator", "bases", "count"))
    check(ctx, r, m, cols=ALL, delim=b"\t")
    check(ctx, r, m, cols=ALL, delim=b"<=delim>")                        # 8 bytes
    got = check(ctx, r, m, cols=("echo", "count", "bases"), skip_unmapped=True)
    assert 0 < got.count(b"\n") < 700
    check(ctx, r, m, cols=("echo", "bases_uniq"), skip_unmapped=True)      # the count is not among the columns
    with pytest.raises(ValueError):
        ctx.bedmap(a, m, cols=("sum",))


def test_echoes_left_to_the_wave(ctx):
    import starch_amd
    from tests import wave_lines
    W = starch_amd.sort_constants()[1]
    # long echoes at lanes 0 and 63 of the first wave and lane 0 of the third, then none at all
    for r, m in wave_lines.wave_pairs(W):
        check(ctx, r, m, cols=("echo", "count"))
        check(ctx, r, m, cols=("count", "echo", "bases"), delim=b"<=>")       # the cursor after a 3-byte delimiter
        check(ctx, r, m, cols=("echo", "bases_uniq"), delim=b"<=>", skip_unmapped=True)


def test_stats(ctx):
    rng = random.Random(2)
    r = random_bed(rng, [b"chr1", b"chr2"], 500)
    m = random_bed(rng, [b"chr1", b"chr3"], 300)
    got = ctx.bedmap(r, m, cols=ALL)
    s = ctx.map_stats()
    assert (s["n_ref"], s["n_map"], s["n_chromosomes"]) == (500, 300, 3)
    assert s["lines_out"] == 500 == got.count(b"\n") and s["output_bytes"] == len(got)
    assert 0 < s["map_runs_merged"] <= 300 and s["stops_sorted"] in (0, 1)
    assert all(s[k] >= 0 for k in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_format")) and s["ms_total"] > 0
    got = ctx.bedmap(r, m, cols=("echo", "count"), skip_unmapped=True)
    s = ctx.map_stats()
    assert s["lines_out"] == got.count(b"\n") < 500 and s["output_bytes"] == len(got)
    assert s["map_runs_merged"] == 0                                     # BASES_UNIQ was not asked for


# ---- 2. tiles -----------------------------------------------------------------------------
def test_tile_sizes(ctx, TW):
    T = TW[0]
    rng = random.Random(3)
    m = random_bed(rng, [b"chr1"], 1500)
    for n in (T - 1, T, T + 1, 3 * T + 137):
        check(ctx, random_bed(rng, [b"chr1"], n), m)
        assert ctx.map_stats()["n_ref"] == n


def test_chromosome_change_at_and_inside_a_tile(ctx, TW):
    T = TW[0]
    rng = random.Random(4)
    m = random_bed(rng, [b"chr1", b"chr2", b"chr3", b"chr4"], 2000)
    for n1 in (T, T // 2 + 3, 2 * T - 1):                # the change at a tile boundary, inside a tile, one line before
        r = random_bed(rng, [b"chr1"], n1) + random_bed(rng, [b"chr2"], T + 9)
        check(ctx, r, m)
    # a one-line chromosome as the first and as the last line of a tile
    one = bed([(1000, 1200)], b"chr2")
    check(ctx, one + random_bed(rng, [b"chr3"], 2 * T), m)
    check(ctx, random_bed(rng, [b"chr1"], T - 1) + one + random_bed(rng, [b"chr3"], T + 5), m)
    check(ctx, random_bed(rng, [b"chr1"], T) + one + random_bed(rng, [b"chr3"], T - 1) + bed([(7, 9)], b"chr4"), m)


def test_largest_window_end_on_the_first_line_of_a_tile(ctx, TW):
    T = TW[0]
    # a long reference line, then short ones far below its stop: a window
    # bounded by the last line's end would miss the map lines the first covers
    m = bed([(10 * i, 10 * i + 7) for i in range(400)])
    short = [(5 + i, 8 + i) for i in range(T - 1)]
    r = bed([(0, 4000)] + short)
    got = check(ctx, r, m)
    assert got.startswith(b"chr1\t0\t4000|400|2800|2800|1|4000\n")
    # the same line in the middle of the second tile, and as the last line of the first
    check(ctx, bed([(0, 1)] * (T + T // 2) + [(1, 4000)] + [(2 + i, 4 + i) for i in range(T)]), m)
    check(ctx, bed([(0, 1)] * (T - 1) + [(1, 4000)] + [(2 + i, 4 + i) for i in range(T)]), m)
    check(ctx, r, m, range=50)


# ---- 3. nesting ---------------------------------------------------------------------------
def test_nested_map_lines_sort_the_stops(ctx):
    inner = [(10 + 3 * i, 12 + 3 * i) for i in range(3000)]
    m_nested = bed([(0, 20000)] + inner)
    m_flat = bed(inner)
    rng = random.Random(5)
    r = bed(sorted((s, s + rng.choice((1, 4, 50, 3000))) for s in (rng.randrange(0, 21000) for _ in range(300))))
    got = check(ctx, r, m_nested, oracle.pairs)
    assert ctx.map_stats()["stops_sorted"] == 1 and ctx.map_stats()["map_runs_merged"] == 1
    assert any(f[2] != f[3] for f in (ln.split(b"|") for ln in got.split(b"\n")[:-1]))    # BASES != BASES_UNIQ
    check(ctx, r, m_flat, oracle.pairs)
    assert ctx.map_stats()["stops_sorted"] == 0 and ctx.map_stats()["map_runs_merged"] == 3000
    # nesting on one chromosome only, another after it
    check(ctx, r + bed([(5, 50)], b"chr2"), m_nested + bed([(0, 9), (20, 30)], b"chr2"), oracle.pairs)


def test_abutting_and_touching(ctx):
    m = bed([(10 * i, 10 * i + 10) for i in range(300)])                 # abutting map lines
    r = bed([(10 * i + 5, 10 * i + 25) for i in range(290)])
    got = check(ctx, r, m)
    assert got.startswith(b"chr1\t5\t25|3|20|20|1|20\n") and ctx.map_stats()["map_runs_merged"] == 1
    # a map stop equal to a reference start, a map start equal to a reference stop
    assert ctx.bedmap(bed([(100, 200)]), bed([(50, 100), (200, 250)]), cols=NUM) == b"0|0|0|0|100\n"
    assert ctx.bedmap(bed([(100, 200)]), bed([(50, 101), (199, 250)]), cols=NUM) == b"2|2|2|1|100\n"


# ---- 4. window (only with an LDS path) -----------------------------------------------------
def test_lds_window_edges(ctx, TW):
    T, W = TW
    if W == 0:
        return                                                           # no LDS path in this build: nothing switches on W
    for k in (W, W + 1):
        m = bed([(2 * i, 2 * i + 1) for i in range(k)])
        r = bed([(0, 2 * k)] + [(1 + i, 4 + i) for i in range(T - 1)])       # one tile whose window holds k elements
        check(ctx, r, m, oracle.pairs)
    m = bed([(2 * i, 2 * i + 1) for i in range(4 * W)])
    small = [(i, i + 3) for i in range(T)]
    large = [(2 * T, 8 * W)] + [(2 * T + 1 + i, 2 * T + 4 + i) for i in range(T - 1)]
    check(ctx, bed(small + large), m, oracle.pairs)


# ---- 5. chromosomes ---------------------------------------------------------------------------
def test_chromosomes(ctx):
    rng = random.Random(6)
    r = random_bed(rng, [b"chr1", b"chr10", b"chr2", b"chrM"], 600)
    m = random_bed(rng, [b"chr10", b"chr2", b"chr20", b"chrX"], 600)      # chr1, chrM not mapped; chr20, chrX not referenced
    got = check(ctx, r, m)
    assert b"chr1\t" in got and ctx.map_stats()["n_chromosomes"] == 6
    check(ctx, m, r)
    names = [b"c%02d" % k for k in range(40)]
    r40 = b"".join(random_bed(rng, [n], rng.randint(1, 5)) for n in names)
    m40 = b"".join(random_bed(rng, [n], rng.randint(1, 9)) for n in names[::-1][::2][::-1])
    check(ctx, r40, m40)
    check(ctx, r40, None)


# ---- 6. range -----------------------------------------------------------------------------------
def test_range(ctx):
    rng = random.Random(7)
    r = random_bed(rng, [b"chr1", b"chr2"], 500, lengths=(1, 5, 30))
    m = random_bed(rng, [b"chr1", b"chr2"], 800, lengths=(1, 5, 30))
    for k in (0, 1, 100, 5000):                          # 5000: above every start, the window clamps at 0
        got = check(ctx, r, m, range=k)
        sizes = [int(ln.split(b"|")[-1]) for ln in got.split(b"\n")[:-1]]
        assert sizes == [e - s for _, _, s, e in oracle.parse(r)]         # ECHO_REF_SIZE stays unpadded
    check(ctx, r, m, oracle.pairs, range=2 ** 64 - 1)


# ---- 7. wide coordinates ---------------------------------------------------------------------------
def test_wide_coordinates(ctx):
    rng = random.Random(8)
    base = 2 ** 62
    m = bed(sorted((base + s, base + s + rng.choice((1, 30, 2000))) for s in (rng.randrange(0, 100000) for _ in range(3000))))
    r = bed(sorted((base + s, base + s + rng.choice((1, 300, 50000))) for s in (rng.randrange(0, 100000) for _ in range(400))))
    # 3000 starts near 2^62 sum to far more than 2^64: the prefix sums wrap
    check(ctx, r, m, oracle.pairs)
    check(ctx, r, m, oracle.pairs, range=1000)
    top = 2 ** 63 - 1
    assert ctx.bedmap(bed([(top - 10, top)]), bed([(0, top), (top - 5, top)]), cols=NUM) == b"2|15|10|1|10\n"


# ---- 8. random -----------------------------------------------------------------------------------------
def test_random_cases_against_the_bitmap(ctx, TW):
    T = TW[0]
    names = [b"c", b"ch", b"chr", b"chr1"]           # prefixes of each other
    for seed in range(300):
        rng = random.Random(3000 + seed)
        chroms = rng.sample(names, rng.randint(1, 4))
        nr = rng.choice((1, 3, 30, 60)) if seed % 10 else rng.choice((T - 1, T + 1, 2 * T))
        ref = random_bed(rng, chroms, nr)
        mp = None if rng.random() < 0.15 else random_bed(rng, rng.sample(names, rng.randint(1, 4)), rng.randint(0, 80))
        kw = dict(cols=rng.sample(ALL, rng.randint(1, 6)), range=rng.choice((0, 0, 1, 9, 300)),
                  skip_unmapped=rng.random() < 0.25)
        assert ctx.bedmap(ref, mp, **kw) == oracle.bitmap(ref, mp, **kw), seed


def test_random_cases_against_the_pairs(ctx):
    for seed in range(40):
        rng = random.Random(4000 + seed)
        lim = rng.choice((5000, 10 ** 9, 2 ** 40))
        lens = (1, 7, lim // 50, lim // 3)
        ref = random_bed(rng, [b"chr1", b"chr2"], rng.randint(1, 300), limit=lim, lengths=lens)
        mp = random_bed(rng, [b"chr1", b"chr2", b"chr3"], rng.randint(0, 300), limit=lim, lengths=lens)
        check(ctx, ref, mp, oracle.pairs, range=rng.choice((0, 1, lim // 100)))


# ---- 9. archives -------------------------------------------------------------------------------------------
def test_archives(ctx):
    import starch_amd
    rng = random.Random(9)
    r = random_bed(rng, [b"chr1", b"chr10", b"chr2"], 700)
    m = random_bed(rng, [b"chr1", b"chr2", b"chrX"], 500)
    ar, am = ctx.compress(r), ctx.compress(m)
    assert ar[:4] == b"\xca\x5c\xad\x1a"
    want = check(ctx, r, m)
    assert ctx.bedmap(ar, m, cols=ALL) == want
    assert ctx.bedmap(r, am, cols=ALL) == want
    assert ctx.bedmap(ar, am, cols=ALL) == want
    assert ctx.bedmap(ar, None, cols=ALL) == ctx.bedmap(r, None, cols=ALL) == oracle.bitmap(r, None, cols=ALL)
    ctx.set_compression_method(starch_amd.K_GZIP)
    try:
        gz = ctx.compress(m)
    finally:
        ctx.set_compression_method(starch_amd.K_BZIP2)
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bedmap(r, gz)
    assert e.value.code == -2 and "gzip" in str(e.value)
    assert ctx.bedmap(ar, am, cols=ALL) == want


# ---- 10. errors ----------------------------------------------------------------------------------------------
def _refused(ctx, ref, mp, code, *words):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bedmap(ref, mp, cols=ALL)
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    assert ctx.bedmap(bed([(1, 2)])) == b"chr1\t1\t2|1\n"   # the context works again


def test_errors(ctx):
    hi, lo = bed([(500, 600), (700, 800)]), bed([(1, 2), (3, 4), (2, 9), (0, 1)])
    _refused(ctx, lo, hi, -12, "bedmap: input 0, line 3:", "sort-bed")                  # unsorted reference
    _refused(ctx, hi, lo, -12, "bedmap: input 1, line 3:", "sort-bed")                  # unsorted map
    _refused(ctx, lo, None, -12, "input 0, line 3:", "sort-bed")
    assert ctx.bedmap(hi, bed([(1, 2), (3, 4)])) == b"chr1\t500\t600|0\nchr1\t700\t800|0\n"   # the map may start below
    _refused(ctx, bed([(1, 2)], b"chr2") + bed([(1, 2)], b"chr10"), hi, -12, "input 0, line 2:", "sort-bed")
    _refused(ctx, hi, bed([(1, 2), (5, 5)]), -12, "input 1, line 2:", "stop")
    _refused(ctx, bed([(1, 2), (9, 7)]), hi, -12, "input 0, line 2:", "stop")
    # a malformed line in the map goes ahead of an order error in the reference
    _refused(ctx, lo, b"chr1\t1\t2\nchr1\t5\n", -12, "input 1, line 2:", "fewer than three")
    _refused(ctx, b"chr1\t1\t2\n\nchr1\t5\t6\n", hi, -12, "input 0, line 2:", "empty line")
    _refused(ctx, hi, b"track name=x\nchr1\t1\t2\n", -12, "input 1, line 1:", "track")
    _refused(ctx, b"", b"chr1\t1\tx\n", -12, "input 1, line 1:", "stop")                 # checked though nothing refers to it


def test_argument_errors(ctx):
    import ctypes
    import starch_amd
    a = bed([(1, 2)])
    for kw in (dict(cols=("count", "echo", "count")),          # a repeated column
               dict(cols=()),                                  # no columns
               dict(cols=ALL + ALL[:3]),                       # more than 8 (and repeated)
               dict(delim=b""), dict(delim=b"123456789")):
        with pytest.raises(starch_amd.StarchError) as e:
            ctx.bedmap(a, a, **kw)
        assert e.value.code == -2, kw
    L = starch_amd.load()
    one, opt = starch_amd.SetopInput(a, len(a)), starch_amd.MapOptions()
    opt.ncols, opt.delim_len, opt.delim = 1, 1, b"|"
    opt.cols[0] = 6                                            # an unknown code
    assert L.starch_map_host(ctx._h, ctypes.byref(one), None, ctypes.byref(opt)) == -2
    opt.cols[0] = 1
    assert L.starch_map_host(ctx._h, ctypes.byref(one), None, None) == -2
    assert L.starch_map_host(ctx._h, None, None, ctypes.byref(opt)) == -2
    offs = (ctypes.c_uint64 * 4)(0, 0, 0, 0)
    assert L.starch_map_device(ctx._h, None, offs, 0, ctypes.byref(opt)) == -2
    assert L.starch_map_device(ctx._h, None, offs, 3, ctypes.byref(opt)) == -2
    assert L.starch_map_host(ctx._h, ctypes.byref(one), None, ctypes.byref(opt)) == 0
    assert ctx._output() == b"1\n"


# ---- 11. device entry and chaining -------------------------------------------------------------------------------
def test_device_entry_and_chaining(ctx):
    import torch
    rng = random.Random(10)
    r = random_bed(rng, [b"chr1", b"chr2"], 900)
    m = random_bed(rng, [b"chr1", b"chr2", b"chr3"], 1200)
    want = check(ctx, r, m)
    blob = r[:-1] + m                                          # the reference without its final newline
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    k = ctx.bedmap_device(dev.data_ptr(), [0, len(r) - 1, len(blob)], cols=ALL)
    assert k == len(want) and ctx.output_device_ptr() != 0 and ctx._output() == want
    k = ctx.bedmap_device(dev.data_ptr(), [0, len(r) - 1], cols=ALL)
    assert ctx._output() == oracle.bitmap(r, None, cols=ALL) and k == len(ctx._output())
    # bytes left in HBM by sort_bed
    rows = r.split(b"\n")[:-1]
    rng.shuffle(rows)
    shuffled = torch.frombuffer(bytearray(b"\n".join(rows) + b"\n"), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    n = ctx.sort_bed_device(shuffled.data_ptr(), shuffled.numel())
    assert n == len(r)
    ctx.bedmap_device(ctx.output_device_ptr(), [0, n], cols=ALL)
    assert ctx._output() == oracle.bitmap(r, None, cols=ALL)
    # the output of merge as a reference
    merged = ctx.merge(r, m)
    check(ctx, merged, m)
    check(ctx, merged, r, cols=("echo", "count", "bases_uniq"), skip_unmapped=True)


# ---- 12. command ---------------------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_command(ctx, tmp_path):
    rng = random.Random(11)
    r = random_bed(rng, [b"chr1", b"chr2"], 800)
    m = random_bed(rng, [b"chr1", b"chr3"], 600)
    fr, fm, fs = tmp_path / "ref.bed", tmp_path / "map.bed", tmp_path / "map.starch"
    fr.write_bytes(r)
    fm.write_bytes(m)
    fs.write_bytes(ctx.compress(m))
    cols = ("echo", "count", "bases")
    p = _run([BEDMAP, "--echo", "--count", "--bases", str(fr), str(fs)])
    assert p.returncode == 0 and p.stdout == ctx.bedmap(r, m, cols=cols) == oracle.bitmap(r, m, cols=cols)
    p = _run([BEDMAP, "--bases-uniq", "--echo", "--range", "25", "--delim", "\t", "--skip-unmapped", "-", str(fm)], input=r)
    assert p.returncode == 0
    assert p.stdout == oracle.bitmap(r, m, cols=("bases_uniq", "echo"), range=25, delim=b"\t", skip_unmapped=True)
    p = _run([BEDMAP, str(fr)])                                # the default columns, the reference onto itself
    assert p.returncode == 0 and p.stdout == oracle.bitmap(r, None)
    fu = tmp_path / "unsorted.bed"
    fu.write_bytes(bed([(5, 6), (1, 2)]))
    p = _run([BEDMAP, "--count", str(fr), str(fu)])
    assert p.returncode == 22 and p.stdout == b"" and b"bedmap: input 1, line 2:" in p.stderr
