"""GPU: starchcat (Starch.cat, the starchcat command).

What a cat must give is stated here over the parsed lines of the input BEDs,
never taken from the code under test: the lines are grouped by chromosome, a
group's lines being the inputs' lines in input order (and, inside an input,
in their order there, so a chromosome revisited later in an input comes
after its first visit); the chromosomes are ordered with sorted() on their
bytes and each group's lines with sorted(key=(start, stop)), which is stable:
lines with equal keys keep the order just described.  The expected archive is
compress() of that BED under the same note, level and base counts, and the
assertion is equality of the whole archive, byte for byte.
"""
import os
import random
import subprocess
import sys

import pytest

from tests import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STARCHCAT = os.path.join(ROOT, "starch_amd", "_build", "starchcat")
RUN_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def _lines(bed):
    out = []
    for ln in bed.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        out.append((f[0], int(f[1]), int(f[2]), ln + b"\n"))
    return out


def _key(t):
    return (t[1], t[2])


def _bed(lines):
    return b"".join(t[3] for t in lines)


def _expected(beds):
    groups = {}
    for bed in beds:
        for t in _lines(bed):
            groups.setdefault(t[0], []).append(t)
    return b"".join(_bed(sorted(groups[name], key=_key)) for name in sorted(groups))


def _chrom(name, n, seed, lo=0, span=1_000_000):
    """n sorted bed6 lines of one chromosome with start in [lo, lo + span)."""
    r = random.Random(seed)
    out = []
    for i in range(n):
        s = r.randrange(lo, lo + span)
        e = s + r.randint(1, 1500)
        out.append((name, s, e, name + b"\t%d\t%d\tid%d_%d\t%d\t%s\n" % (s, e, seed, i, r.randint(0, 1000),
                                                                          r.choice("+-.").encode())))
    return sorted(out, key=_key)


def _check(ctx, beds, archives=None):
    """cat of the beds' archives == compress(expected), and it reads back as the expected BED."""
    if archives is None:
        archives = [ctx.compress(b) for b in beds]
    want_bed = _expected(beds)
    got = ctx.cat(archives)
    assert got == ctx.compress(want_bed)
    assert ctx.unstarch(got) == want_bed
    return got


# ---- two inputs dealt from one file: every group is a merge ------------------
@pytest.fixture(scope="module")
def dealt():
    raw = _lines(corpus.multi_chrom_bed(3, 7000, seed=31, kind="narrowPeak"))
    names = sorted({t[0] for t in raw})
    lines = [t for name in names for t in sorted((u for u in raw if u[0] == name), key=_key)]
    return _bed(lines[0::2]), _bed(lines[1::2]), _bed(lines)


@pytest.mark.gpu
def test_two_inputs_dealt_from_one_file(ctx, dealt):
    a, b, whole = dealt
    assert _expected([a, b]) == whole             # dealing a sorted file and merging gives it back
    ctx.set_note("dealt")
    try:
        _check(ctx, [a, b])
    finally:
        ctx.set_note("")
    s = ctx.cat_stats()
    assert s["streams_in"] == 6 and s["streams_copied"] == 0 and s["groups_merged"] == 3 and s["runs_decoded"] == 6
    assert s["lines_merged"] == 21000 and s["bytes_copied"] == 0


# ---- mixed: copies and one merge ---------------------------------------------
@pytest.fixture(scope="module")
def mixed(ctx):
    beds = [_bed(_chrom(b"chr1", 900, 1) + _chrom(b"chr2", 700, 2)),
            _bed(_chrom(b"chr2", 800, 3) + _chrom(b"chr21", 300, 4)),
            _bed(_chrom(b"chrX", 500, 5))]
    archives = [ctx.compress(b) for b in beds]
    return beds, archives, _check(ctx, beds, archives)


def _stream_of(archive, name):
    import starch_amd
    _, entries = starch_amd.list_archive(archive)
    e = [x for x in entries if x["chromosome"] == name]
    assert len(e) == 1
    return e[0]["offset"], e[0]["size"]


@pytest.mark.gpu
def test_mixed_copies_are_verbatim(ctx, mixed):
    import starch_amd
    beds, archives, got = mixed
    assert ctx.cat(archives) == got
    s = ctx.cat_stats()
    assert s["streams_in"] == 5 and s["streams_copied"] == 3 and s["groups_merged"] == 1 and s["runs_decoded"] == 2
    assert s["lines_merged"] == 1500
    assert starch_amd.cat_plan(archives) == [(b"chr1", "copy", [(0, 0)]), (b"chr2", "merge", [(0, 1), (1, 0)]),
                                             (b"chr21", "copy", [(1, 1)]), (b"chrX", "copy", [(2, 0)])]
    copied = 0
    for k, name in ((0, b"chr1"), (1, b"chr21"), (2, b"chrX")):
        so, sn = _stream_of(archives[k], name)
        do, dn = _stream_of(got, name)
        assert dn == sn and got[do:do + dn] == archives[k][so:so + sn]
        copied += sn
    assert s["bytes_copied"] == copied


@pytest.mark.gpu
def test_mixed_damage_in_a_copied_and_in_a_merged_stream(ctx, mixed):
    import starch_amd
    beds, archives, got = mixed
    so, sn = _stream_of(archives[0], b"chr1")
    hurt = bytearray(archives[0])
    hurt[so + sn // 2] ^= 0x40
    do, _ = _stream_of(got, b"chr1")
    want = bytearray(got)
    want[do + sn // 2] ^= 0x40
    assert ctx.cat([bytes(hurt), archives[1], archives[2]]) == bytes(want)    # copied: not decoded, not detected
    so, sn = _stream_of(archives[0], b"chr2")
    hurt = bytearray(archives[0])
    hurt[so + sn // 2] ^= 0x40
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.cat([bytes(hurt), archives[1], archives[2]])
    assert e.value.code == -12
    assert ctx.cat(archives) == got                                           # the context still serves


# ---- ties, and run lengths around the wave (64) and block (256) sizes --------
def _tie_runs(k, scenario, seed):
    """k sorted runs on one chromosome; the remainder names run and line, so run order shows in the bytes."""
    r = random.Random(seed)
    lens = [RUN_LENGTHS[(seed + 4 * j) % len(RUN_LENGTHS)] for j in range(k)]
    runs = []
    for j, n in enumerate(lens):
        keys = []
        for i in range(n):
            if scenario == "ties":            # few starts, few lengths: equal keys and equal starts with other stops
                s = 10 * r.randrange(0, 40)
                keys.append((s, s + r.choice([0, 5, 5, 70, 300])))
            elif scenario == "all_equal":
                keys.append((100, 200))
            else:                             # "placed": run 1 wholly before run 0, run 2 wholly after, others interleaved
                lo = {0: 1_000_000, 1: 0, 2: 5_000_000}.get(j, 900_000)
                s = lo + r.randrange(0, 200_000)
                keys.append((s, s + r.randint(1, 9) * (i % 3 + 1)))
        keys.sort()
        runs.append([(b"chr7", s, e, b"chr7\t%d\t%d\trun%d_line%d\n" % (s, e, j, i)) for i, (s, e) in enumerate(keys)])
    return lens, [_bed(x) for x in runs]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_ties_and_run_lengths(ctx, k):
    used = set()
    for n, scenario in enumerate(("ties", "all_equal", "placed")):
        lens, beds = _tie_runs(k, scenario, seed=k + 3 * n)
        used.update(lens)
        got = _check(ctx, beds)
        out = _lines(ctx.unstarch(got))
        assert len(out) == sum(lens)
        if scenario == "all_equal":           # nothing but run order decides: run 0's lines, then run 1's, ...
            assert _bed(out) == b"".join(beds)
        if scenario == "placed":
            first = [t[3].split(b"\t")[3].split(b"_")[0] for t in out]
            assert first[0] == b"run1" and first[-1] == (b"run2" if k > 2 else b"run0")
        # the transform's p-lines (one per change of stop - start) make value ordinals differ from text lines
        if scenario != "all_equal" and sum(lens) > 2:
            assert len({t[2] - t[1] for t in out}) > 1
    # over the four values of k every run length is drawn
    drawn = {n for kk in (2, 3, 5, 8) for m in range(3) for n in _tie_runs(kk, "all_equal", kk + 3 * m)[0]}
    assert used <= drawn == set(RUN_LENGTHS)


# ---- a chromosome revisited inside one input ---------------------------------
@pytest.mark.gpu
def test_revisited_chromosome_gives_three_runs(ctx):
    import starch_amd
    a = _bed(_chrom(b"chr1", 300, 11, lo=0, span=50_000) + _chrom(b"chr2", 200, 12) +
             _chrom(b"chr1", 257, 13, lo=20_000, span=50_000))
    b = _bed(_chrom(b"chr1", 65, 14, lo=10_000, span=80_000))
    archives = [ctx.compress(a), ctx.compress(b)]
    plan = starch_amd.cat_plan(archives)
    assert plan == [(b"chr1", "merge", [(0, 0), (0, 2), (1, 0)]), (b"chr2", "copy", [(0, 1)])]
    _check(ctx, [a, b], archives)
    assert ctx.cat_stats()["runs_decoded"] == 3


# ---- batching: one group per batch gives the same bytes ----------------------
_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import starch_amd
c = starch_amd.Starch(0)
for job in sys.argv[2:]:
    ins, out = job.split("=")
    blobs = [open(p, "rb").read() for p in ins.split(",")]
    open(out, "wb").write(c.cat(blobs))
c.close()
"""


@pytest.mark.gpu
def test_one_group_per_batch_in_a_fresh_process(ctx, mixed, dealt, tmp_path):
    _, archives, got = mixed
    a, b, _ = dealt
    two = [ctx.compress(a), ctx.compress(b)]
    want_two = ctx.cat(two)
    jobs = []
    for tag, blobs in (("m", archives), ("d", two)):
        paths = []
        for k, blob in enumerate(blobs):
            paths.append(str(tmp_path / ("%s%d.starch" % (tag, k))))
            with open(paths[-1], "wb") as f:
                f.write(blob)
        jobs.append(",".join(paths) + "=" + str(tmp_path / (tag + ".out")))
    env = dict(os.environ, STARCH_CAT_BATCH_BYTES="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + jobs, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "m.out"), "rb").read() == got
    assert open(str(tmp_path / "d.out"), "rb").read() == want_two


# ---- level and base counts ---------------------------------------------------
@pytest.mark.gpu
def test_level_and_base_counts_re_encode(ctx):
    import starch_amd
    beds = [_bed(_chrom(b"chr3", 400, 21) + _chrom(b"chr5", 300, 22)), _bed(_chrom(b"chr5", 350, 23))]
    try:
        ctx.block_size_100k = 5
        at5 = [ctx.compress(b) for b in beds]
        ctx.block_size_100k = 9
        assert all(p[1] == "merge" for p in starch_amd.cat_plan(at5, level=9))
        _check(ctx, beds, at5)
        assert ctx.cat_stats()["streams_copied"] == 0 and ctx.cat_stats()["groups_merged"] == 2
        plain = [ctx.compress(b) for b in beds]
        ctx.base_counts = True
        assert all(p[1] == "merge" for p in starch_amd.cat_plan(plain, base_counts=True))
        got = _check(ctx, beds, plain)
        assert all("uniqueBaseCount" in e for e in starch_amd.list_archive(got)[1])
        # inputs that carry the counts: chr3 is a copy again, and the bytes are the same
        counted = [ctx.compress(b) for b in beds]
        assert starch_amd.cat_plan(counted, base_counts=True)[0][1] == "copy"
        assert ctx.cat(counted) == got
    finally:
        ctx.block_size_100k = 9
        ctx.base_counts = False


# ---- one input, and the same input twice -------------------------------------
@pytest.mark.gpu
def test_one_input_is_a_normalised_copy(ctx):
    bed = _bed(_chrom(b"chrX", 200, 31) + _chrom(b"chr10", 150, 32) + _chrom(b"chr1", 100, 33))
    got = _check(ctx, [bed])
    s = ctx.cat_stats()
    assert s["streams_copied"] == 3 and s["groups_merged"] == 0 and s["runs_decoded"] == 0
    assert [t[0] for t in _lines(ctx.unstarch(got))][::100][:3] == [b"chr1", b"chr10", b"chr10"]


@pytest.mark.gpu
def test_same_archive_twice(ctx):
    bed = _bed(_chrom(b"chr4", 513, 41) + _chrom(b"chr9", 64, 42))
    arch = ctx.compress(bed)
    got = _check(ctx, [bed, bed], [arch, arch])
    out = _lines(ctx.unstarch(got))
    assert len(out) == 2 * (513 + 64)
    assert all(out[2 * i] == out[2 * i + 1] for i in range(len(out) // 2))
    assert _bed(out[0::2]) == bed


# ---- an unsorted run -----------------------------------------------------------
@pytest.mark.gpu
def test_unsorted_run_is_refused_and_the_context_survives(ctx):
    import starch_amd
    a = [(b"chr1", 10 * i, 10 * i + 5 + i % 3, b"chr1\t%d\t%d\ta%d\n" % (10 * i, 10 * i + 5 + i % 3, i)) for i in range(400)]
    b = [(b"chr1", 7 * i + 3, 7 * i + 9 + i % 4, b"chr1\t%d\t%d\tb%d\n" % (7 * i + 3, 7 * i + 9 + i % 4, i)) for i in range(300)]
    p = 200
    moved = b[:p - 3] + [b[p]] + b[p - 3:p] + b[p + 1:]           # line p three places earlier
    good = [ctx.compress(_bed(a)), ctx.compress(_bed(b))]
    bad = ctx.compress(_bed(moved))
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.cat([good[0], bad])
    assert e.value.code == -12
    msg = str(e.value)
    assert '"chr1"' in msg and "input 1" in msg and "line %d " % (p - 1) in msg, msg
    _check(ctx, [_bed(a), _bed(b)], good)                          # a good pair afterwards
    # the only holder of its chromosome: copied without complaint
    other = _bed(_chrom(b"chr2", 100, 51))
    got = ctx.cat([ctx.compress(other), bad])
    assert ctx.unstarch(got) == _bed(moved) + other
    assert ctx.cat_stats()["streams_copied"] == 2


# ---- the command ---------------------------------------------------------------
@pytest.mark.gpu
def test_starchcat_command(ctx, mixed, tmp_path):
    _, archives, got = mixed
    paths = []
    for k, blob in enumerate(archives):
        paths.append(str(tmp_path / ("c%d.starch" % k)))
        with open(paths[-1], "wb") as f:
            f.write(blob)
    r = subprocess.run([STARCHCAT] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == got
    ctx.set_note("from the command")
    try:
        want = ctx.cat(archives[:2])
    finally:
        ctx.set_note("")
    r = subprocess.run([STARCHCAT, "--note", "from the command"] + paths[:2], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout == want, r.stderr
