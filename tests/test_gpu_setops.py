"""GPU: the bedops set operations (Starch.setop / merge / intersect / difference /
symmdiff / complement, starch_setop_device, the bedops command).

Every comparison is equality of whole outputs against tests/setops_oracle.py:
the bitmap oracle where the coordinates are below 4096, the sweep oracle
otherwise.  T is the number of lines per tile of the segmented max-scan, where
its carry crosses.
"""
import ctypes
import os
import random
import subprocess

import pytest

from tests import setops_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEDOPS = os.path.join(ROOT, "starch_amd", "_build", "bedops")
OPS = oracle.OPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T():
    import starch_amd
    return starch_amd.setop_constants()


def bed(rows, chrom=b"chr1"):
    return b"".join(b"%s\t%d\t%d\n" % ((chrom,) + tuple(r) if len(r) == 2 else tuple(r)) for r in rows)


def check(ctx, inputs, ref, ops=OPS):
    out = {}
    for op in ops:
        out[op] = ctx.setop(op, inputs)
        assert out[op] == ref(op, inputs), op
    return out


# ---- 1. shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_hand_written_table(ctx, case):
    inputs, want = oracle.TABLE[case]
    for op, exp in want.items():
        assert ctx.setop(op, inputs) == exp, op
    check(ctx, inputs, oracle.bitmap)


def test_shapes(ctx):
    assert ctx.setop("merge", [b""]) == b""
    assert ctx.setop_stats()["n_inputs"] == 1 and ctx.setop_stats()["lines_out"] == 0
    for op in OPS:
        assert ctx.setop(op, [b"", b""]) == b""
    a, c = bed([(1, 5), (9, 12)]), bed([(4, 10), (20, 30)])
    check(ctx, [a, b"", c], oracle.bitmap)                 # an empty input among three
    assert ctx.intersect(a, b"", c) == b""
    assert ctx.merge(a, b"", c) == bed([(1, 12), (20, 30)])
    # no final newline, then another input: the two lines must not fuse
    open_end = b"chr1\t1\t5\nchr1\t9\t12"
    out = check(ctx, [open_end, c], oracle.bitmap)
    assert out["merge"] == bed([(1, 12), (20, 30)])
    check(ctx, [c, open_end], oracle.bitmap)
    check(ctx, [open_end], oracle.bitmap)
    # extra columns are ignored
    wide = b"chr1\t1\t5\tname\t0\t+\nchr1\t9\t12\t\t\nchr2\t3\t4\tx y z\n"
    check(ctx, [wide, c], oracle.bitmap)
    assert ctx.merge(wide) == bed([(1, 5), (9, 12)]) + bed([(3, 4)], b"chr2")
    # the wrappers are the ops
    assert ctx.difference(a, c) == ctx.setop("difference", [a, c]) == bed([(1, 4), (10, 12)])
    assert ctx.symmdiff(a, c) == bed([(1, 4), (5, 9), (10, 12), (20, 30)])
    assert ctx.complement(a, c) == bed([(12, 20)])
    got = ctx.setop("merge", [a, wide, c])
    s = ctx.setop_stats()
    assert s["lines_out"] == got.count(b"\n") and s["output_bytes"] == len(got)
    assert s["n_inputs"] == 3 and s["n_lines"] == 7 and s["n_chromosomes"] == 2 and s["archives_decoded"] == 0
    assert s["runs_merged"] == 7 and s["input_bytes"] == len(a) + len(wide) + len(c)
    with pytest.raises(ValueError):
        ctx.setop("union", [a])


# ---- 2. carry of the maximum across tiles ----------------------------------------
def test_maximum_carried_across_tiles(ctx, T):
    inner = [(10 + 3 * i, 11 + 3 * i) for i in range(3 * T + 137)]
    beyond = (2_000_000_000, 2_000_000_001)
    a = bed([(0, 1_000_000_000)] + inner + [beyond])
    assert ctx.merge(a) == bed([(0, 1_000_000_000), beyond])
    assert ctx.setop_stats()["runs_merged"] == 2
    other = bed([(5, 12), (999_999_999, 1_000_000_007)])
    check(ctx, [a, other], oracle.sweep)
    check(ctx, [other, a], oracle.sweep)
    # the long interval as the last line of tile 0
    lead = [(2 * i, 2 * i + 1) for i in range(T - 1)]
    inner = [(2 * T + 10 + 3 * i, 2 * T + 11 + 3 * i) for i in range(3 * T + 137)]
    b = bed(lead + [(2 * T, 1_000_000_000)] + inner + [beyond])
    assert ctx.merge(b) == bed(lead + [(2 * T, 1_000_000_000), beyond])
    check(ctx, [b, other], oracle.sweep)


# ---- 3. segment resets -------------------------------------------------------------------
def test_chromosome_change_at_tile_boundary(ctx, T):
    # lines 0 .. T-1 on chr1 (the first one covers the rest), line T alone on chr2, chr3 from line T + 1
    a = bed([(0, 4000)] + [(1 + i, 3 + i) for i in range(T - 1)]) + bed([(5, 6)], b"chr2") + \
        bed([(7, 8), (9, 10), (10, 12)], b"chr3")
    assert a.count(b"\n") == T + 4
    out = check(ctx, [a], oracle.bitmap)
    assert out["merge"] == bed([(0, 4000)]) + bed([(5, 6)], b"chr2") + bed([(7, 8), (9, 12)], b"chr3")
    b = bed([(3990, 4010)]) + bed([(0, 5)], b"chr2") + bed([(8, 9)], b"chr3")
    check(ctx, [a, b], oracle.bitmap)
    check(ctx, [b, a], oracle.bitmap)


def test_input_boundary_inside_a_tile(ctx, T):
    # both inputs on chr1; input 1's first interval lies inside input 0's last maximum
    a = bed([(0, 3000), (10, 20), (30, 40)])
    b = bed([(100, 200), (3500, 3600)])
    out = check(ctx, [a, b], oracle.bitmap)
    assert out["difference"] == bed([(0, 100), (200, 3000)])
    assert out["intersect"] == bed([(100, 200)])
    # the same with the boundary in the middle of the second tile
    a2 = bed([(i, i + 1) for i in range(0, 2 * T + T, 2)][:T + T // 2 - 1] + [(3100, 4000)])
    b2 = bed([(3200, 3300), (4050, 4060)])
    assert a2.count(b"\n") == T + T // 2
    out = check(ctx, [a2, b2], oracle.bitmap)
    assert out["intersect"] == bed([(3200, 3300)])
    assert out["difference"].endswith(bed([(3100, 3200), (3300, 4000)]))


# ---- 4. equal positions from different inputs --------------------------------------------------
def test_stop_equals_start_of_another_input(ctx, T):
    n = 2 * T + 5
    a = bed([(4 * i, 4 * i + 2) for i in range(n)])
    b = bed([(4 * i + 2, 4 * i + 4) for i in range(n)])
    out = check(ctx, [a, b], oracle.sweep)
    assert out["merge"] == out["symmdiff"] == bed([(0, 4 * n)])
    assert out["intersect"] == b"" and out["complement"] == b"" and out["difference"] == a


def test_ends_coincide_in_40_inputs(ctx):
    same = bed([(100, 200), (300, 400)]) + bed([(1, 2)], b"chr2")
    out = check(ctx, [same] * 40, oracle.bitmap)
    assert out["intersect"] == out["merge"] == same and out["symmdiff"] == out["difference"] == b""
    varied = [bed([(100, 200), (200, 201 + k), (999 - k, 1000)]) for k in range(40)]
    check(ctx, varied, oracle.bitmap)


# ---- 5. many inputs --------------------------------------------------------------------------
def _random_input(rng, chroms, lines, limit=4096, lengths=(1, 2, 7, 40, 600)):
    rows = []
    for _ in range(lines):
        s = rng.randrange(0, limit - 2)
        rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit - 1, s + rng.choice(lengths)))))
    return bed(sorted(rows))


def test_forty_inputs(ctx):
    rng = random.Random(40)
    # chr1: one long interval per input (so that all 40 meet) among short ones; chr2: sparse
    inputs = []
    for _ in range(40):
        rows = oracle.parse(_random_input(rng, [b"chr1"], 100, lengths=(1, 5, 40)) +
                            _random_input(rng, [b"chr2"], 100, lengths=(1, 2, 3)))
        inputs.append(bed(sorted(rows + ((b"chr1", rng.randrange(100, 1500), rng.randrange(2500, 4000)),))))
    out = check(ctx, inputs, oracle.bitmap)
    assert out["intersect"] != b"" and out["symmdiff"] != b"" and out["difference"] != b""


# ---- 6. wide coordinates and formatting ----------------------------------------------------------
def test_wide_coordinates(ctx):
    vals = sorted({10 ** k + d for k in range(19) for d in (-1, 0, 1)} | {2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1})
    assert vals[0] == 0 and vals[-1] == 2 ** 63 - 1
    a = [(vals[i], vals[i + 1]) for i in range(0, len(vals) - 1, 2)]
    b = [(vals[i], vals[i + 1]) for i in range(1, len(vals) - 1, 2)]
    c = [(vals[i], vals[i + 2]) for i in range(0, len(vals) - 2, 3)]
    A = bed(a) + bed(b, b"chr2")
    B = bed(b) + bed(c, b"chr2")
    C = bed(c) + bed(a, b"chr2")
    out = check(ctx, [A, B], oracle.sweep)
    assert out["merge"].startswith(b"chr1\t0\t%d\n" % max(a[-1][1], b[-1][1]))
    check(ctx, [A, C], oracle.sweep)
    check(ctx, [C, B, A], oracle.sweep)
    assert ctx.merge(bed([(2 ** 63 - 2, 2 ** 63 - 1)])) == b"chr1\t9223372036854775806\t9223372036854775807\n"


# ---- 7. random -----------------------------------------------------------------------------------
def test_random_cases(ctx, T):
    names = [b"c", b"ch", b"chr", b"chr1"]           # prefixes of each other
    for seed in range(30):
        rng = random.Random(1000 + seed)
        chroms = rng.sample(names, rng.randint(1, 4))
        cap = rng.choice((3, 50, T - 1, T, T + 1, 2 * T))
        inputs = [_random_input(rng, chroms, rng.randint(0, cap)) for _ in range(rng.randint(1, 6))]
        for op in OPS:
            assert ctx.setop(op, inputs) == oracle.bitmap(op, inputs), (seed, op)


# ---- 8. archives ---------------------------------------------------------------------------------
def test_archives(ctx):
    import starch_amd
    rng = random.Random(8)
    a = _random_input(rng, [b"chr1", b"chr10", b"chr2"], 700)
    b = _random_input(rng, [b"chr1", b"chr2", b"chrX"], 300)
    arch_a, arch_b = ctx.compress(a), ctx.compress(b)
    assert arch_a[:4] == b"\xca\x5c\xad\x1a"
    for op in OPS:
        want = oracle.bitmap(op, [a, b])
        assert ctx.setop(op, [arch_a, b]) == want, op
        assert ctx.setop_stats()["archives_decoded"] == 1
        assert ctx.setop(op, [a, arch_b]) == want, op
        assert ctx.setop(op, [arch_a, arch_b]) == want, op
        assert ctx.setop_stats()["archives_decoded"] == 2
        assert ctx.setop(op, [arch_a]) == oracle.bitmap(op, [a]), op
    ctx.set_compression_method(starch_amd.K_GZIP)
    try:
        gz = ctx.compress(a)
    finally:
        ctx.set_compression_method(starch_amd.K_BZIP2)
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.setop("merge", [b, gz])
    assert e.value.code == -2 and "gzip" in str(e.value)
    assert ctx.merge(arch_a, b) == oracle.bitmap("merge", [a, b])


# ---- 9. errors -----------------------------------------------------------------------------------
def _refused(ctx, inputs, code, *words):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.setop("merge", inputs)
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(starch_amd.StarchError) as e2:      # nothing was written as output
        ctx._output()
    assert e2.value.code == -4
    good = bed([(1, 2)])
    assert ctx.merge(good) == good                          # the context works again


def test_errors(ctx):
    hi, lo = bed([(500, 600), (700, 800)]), bed([(1, 2), (3, 4), (2, 9), (0, 1)])
    # input 1 starts below input 0's last line: not a descent; its line 3 is one
    _refused(ctx, [hi, lo], -12, "input 1, line 3:", "sort-bed")
    assert ctx.merge(hi, bed([(1, 2), (3, 4)])) == bed([(1, 2), (3, 4), (500, 600), (700, 800)])
    # chromosome order counts too
    _refused(ctx, [bed([(1, 2)], b"chr2") + bed([(1, 2)], b"chr10")], -12, "input 0, line 2:", "sort-bed")
    _refused(ctx, [hi, bed([(1, 2), (5, 5)])], -12, "input 1, line 2:", "stop")
    _refused(ctx, [hi, b"", bed([(1, 2), (3, 4), (9, 7)])], -12, "input 2, line 3:", "stop")
    # a malformed line in input 2 goes ahead of an order error in input 0
    _refused(ctx, [lo, hi, b"chr1\t1\t2\nchr1\t5\n"], -12, "input 2, line 2:", "fewer than three")
    _refused(ctx, [hi, b"track name=x\nchr1\t1\t2\n"], -12, "input 1, line 1:", "track")
    _refused(ctx, [hi, b"chr1\t1\t2\n\nchr1\t5\t6\n"], -12, "input 1, line 2:", "empty line")


def test_argument_errors(ctx):
    import starch_amd
    L = starch_amd.load()
    one = (starch_amd.SetopInput * 1)()
    assert L.starch_setop_host(ctx._h, 0, one, 0) == -2          # no inputs
    assert L.starch_setop_host(ctx._h, 5, one, 1) == -2          # unknown op
    assert L.starch_setop_host(ctx._h, -1, one, 1) == -2
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.setop("merge", [])
    assert e.value.code == -2


# ---- 10. device entry and chaining -------------------------------------------------------------------
def test_device_entry_and_chaining(ctx):
    import torch
    rng = random.Random(10)
    inputs = [_random_input(rng, [b"chr1", b"chr2"], n) for n in (900, 0, 1500)]
    inputs[0] = inputs[0][:-1]                                # no final newline
    blob = b"".join(inputs)
    offs = [0]
    for b in inputs:
        offs.append(offs[-1] + len(b))
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    for op in OPS:
        want = ctx.setop(op, inputs)
        assert want == oracle.bitmap(op, inputs)
        k = ctx.setop_device(op, dev.data_ptr(), offs)
        assert k == len(want) and ctx.output_device_ptr() != 0
        assert ctx._output() == want
        assert ctx.sort_check(want) == 0
        assert ctx.setop("merge", [want]) == want
    # the result is valid input for the encoder
    merged = ctx.merge(*inputs)
    assert ctx.unstarch(ctx.compress(merged)) == merged


# ---- 11. command ---------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_command(ctx, tmp_path):
    rng = random.Random(11)
    a = _random_input(rng, [b"chr1", b"chr2"], 800)
    b = _random_input(rng, [b"chr1", b"chr3"], 600)
    fa, fb, fs = tmp_path / "a.bed", tmp_path / "b.bed", tmp_path / "b.starch"
    fa.write_bytes(a)
    fb.write_bytes(b)
    fs.write_bytes(ctx.compress(b))
    r = _run([BEDOPS, "-m", str(fa), str(fs)])
    assert r.returncode == 0 and r.stdout == ctx.merge(a, b) == oracle.bitmap("merge", [a, b])
    r = _run([BEDOPS, "-i", "-", str(fb)], input=a)
    assert r.returncode == 0 and r.stdout == ctx.intersect(a, b)
    r = _run([BEDOPS, "--difference", str(fa), str(fb)])
    assert r.returncode == 0 and r.stdout == oracle.bitmap("difference", [a, b])
    fu = tmp_path / "unsorted.bed"
    fu.write_bytes(bed([(5, 6), (1, 2)]))
    r = _run([BEDOPS, "-m", str(fa), str(fu)])
    assert r.returncode == 22 and r.stdout == b"" and b"input 1, line 2:" in r.stderr
