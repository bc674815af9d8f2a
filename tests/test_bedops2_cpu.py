"""CPU-side checks of bedops' element-of, not-element-of, partition, chop and
everything: the two oracles of tests/bedops2_oracle.py against each other and
against the hand-written table, and the parts of the library, of the Python
interface and of the `bedops` command that open no GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from tests import bedops2_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEDOPS = os.path.join(ROOT, "starch_amd", "_build", "bedops")
THRESHOLDS = (1, 7, "1%", "50%", "100%")
CHOPS = ((1, 1, False), (5, 5, False), (5, 2, False), (5, 9, True), (4096, 4096, False))


def _run(*args, **kw):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([BEDOPS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=env, **kw)


def random_case(rng, max_inputs=4, max_iv=30, limit=300):
    chroms = [b"chr1", b"chr10", b"chr2"][:rng.randint(1, 3)]
    inputs = []
    for k in range(rng.randint(2, max_inputs)):
        rows = []
        for _ in range(rng.randint(0, max_iv)):
            s = rng.randrange(0, limit - 1)
            rows.append((rng.choice(chroms), s, rng.randint(s + 1, min(limit - 1, s + 1 + rng.choice((1, 5, 40))))))
        rows.sort()
        inputs.append(b"".join(b"%s\t%d\t%d\tid%d.%d\n" % (r + (k, n)) for n, r in enumerate(rows)))
    return inputs


def test_oracles_agree_on_random_cases():
    rng = random.Random(20261019)
    nonempty = {op: 0 for op in oracle.OPS}
    for case in range(200):
        inputs = random_case(rng)
        t = THRESHOLDS[case % len(THRESHOLDS)]
        w, g, x = CHOPS[case % len(CHOPS)]
        for op in oracle.OPS:
            kw = {"threshold": t} if "element" in op else {"width": w, "stagger": g, "exclude_short": x} if op == "chop" else {}
            a, b = oracle.bitmap(op, inputs, **kw), oracle.integers(op, inputs, **kw)
            assert a == b, (op, kw, inputs)
            nonempty[op] += a != b""
    assert all(v > 20 for v in nonempty.values()), nonempty   # the cases exercise every op


@pytest.mark.parametrize("case", range(len(oracle.TABLE)))
def test_oracles_give_the_hand_written_table(case):
    op, inputs, kw, want = oracle.TABLE[case]
    assert oracle.bitmap(op, inputs, **kw) == want
    assert oracle.integers(op, inputs, **kw) == want


def test_integer_oracle_near_2_63():
    top = 2 ** 63 - 1
    ref = b"chr1\t0\t%d\n" % top
    assert oracle.integers("element_of", [ref, ref]) == ref
    assert oracle.integers("element_of", [ref, b"chr1\t0\t%d\n" % (top - 1)]) == b""
    assert oracle.integers("element_of", [ref, b"chr1\t0\t%d\n" % (top - 1)], threshold="99%") == ref
    assert oracle.integers("chop", [b"chr1\t%d\t%d\n" % (top - 5, top)], width=2 ** 62, stagger=3) == \
        b"chr1\t%d\t%d\nchr1\t%d\t%d\n" % (top - 5, top, top - 2, top)


def test_symbols_and_python_surface():
    import starch_amd
    L = starch_amd.load()
    for name in ("starch_bedops_host", "starch_bedops_device", "starch_bedops_constants", "starch_setop_get_stats"):
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    assert starch_amd.BEDOPS_OPS == {"merge": 0, "intersect": 1, "difference": 2, "symmdiff": 3, "complement": 4,
                                     "element_of": 5, "not_element_of": 6, "partition": 7, "chop": 8, "everything": 9}
    assert starch_amd.SETOPS == {"merge": 0, "intersect": 1, "difference": 2, "symmdiff": 3, "complement": 4}
    # starch_bedops_options: i32, u64, u32, u64, u64, u32, each naturally aligned
    o = starch_amd.BedopsOptions
    assert ctypes.sizeof(o) == 48
    assert (o.op.offset, o.threshold.offset, o.threshold_is_percent.offset, o.chop.offset, o.stagger.offset,
            o.exclude_short.offset) == (0, 8, 16, 24, 32, 40)
    rmq, expand = starch_amd.bedops_constants()
    assert rmq >= 2 and expand >= 64 and expand % 64 == 0
    for m in ("bedops", "bedops_device", "element_of", "not_element_of", "partition", "chop", "everything"):
        assert callable(getattr(starch_amd.Starch, m))
    with pytest.raises(ValueError):
        starch_amd._bedops_options("union", "100%", 1, None, False)
    with pytest.raises(ValueError):
        starch_amd._bedops_options("element_of", "half", 1, None, False)
    p = starch_amd._bedops_options("element_of", "50%", 1, None, False)
    assert (p.op, p.threshold, p.threshold_is_percent) == (5, 50, 1)
    p = starch_amd._bedops_options("chop", 7, 100, 40, True)
    assert (p.op, p.threshold, p.threshold_is_percent, p.chop, p.stagger, p.exclude_short) == (8, 7, 0, 100, 40, 1)


def test_argument_errors_need_no_device():
    """Every argument error is answered before the context is looked at: a NULL
    context and a NULL array are among them, and no call here can reach a device."""
    import starch_amd
    L = starch_amd.load()
    one = (starch_amd.SetopInput * 2)()
    offs = (ctypes.c_uint64 * 3)(0, 0, 0)

    def opts(op, threshold=100, pct=1, chop=1):
        o = starch_amd.BedopsOptions()
        o.op, o.threshold, o.threshold_is_percent, o.chop = op, threshold, pct, chop
        return ctypes.byref(o)

    for o in (opts(5, 0, 0), opts(5, 0, 1), opts(6, 101, 1), opts(8, chop=0), opts(10), opts(-1), None):
        assert L.starch_bedops_host(None, o, one, 2) == -2
        assert L.starch_bedops_device(None, o, None, offs, 2) == -2
    assert L.starch_bedops_host(None, opts(5), one, 1) == -2       # element-of with one input
    assert L.starch_bedops_host(None, opts(9), None, 1) == -2
    assert L.starch_bedops_host(None, opts(9), one, 0) == -2
    assert L.starch_bedops_device(None, opts(9), None, None, 1) == -2
    assert L.starch_setop_host(None, 5, one, 1) == -2              # the old entry still stops at op 4


def test_help_lists_ten_operations():
    r = _run("--help")
    assert r.returncode == 0 and r.stderr == b""
    assert b"USAGE: bedops (-m|--merge" in r.stdout
    for word in (b"--merge", b"--intersect", b"--difference", b"--symmdiff", b"--complement", b"--element-of",
                 b"--not-element-of", b"--partition", b"--chop", b"--everything", b"--stagger", b"-x",
                 b"largest overlap with one run", b"distinct starts and", b"a + k*G < b", b"ties by file",
                 b"unverified against a BEDOPS binary"):
        assert word in r.stdout, word


def test_bad_command_lines():
    missing = os.path.join(ROOT, "no", "such", "file.bed")
    for args in (["-m", "--stagger", "4", missing],            # --stagger without --chop
                 ["-p", "-x", missing],                        # -x without --chop
                 ["--stagger", "4", missing],                  # no operation
                 ["-e", missing],                              # element-of with one file
                 ["-n", "50%", missing],
                 ["-e", "0", missing, missing],                # bad values
                 ["-e", "0%", missing, missing],
                 ["-n", "101%", missing, missing],
                 ["-w", "0", missing],
                 ["-w", "5", "--stagger", "0", missing],
                 ["-w", "5", "--stagger", "x", missing],
                 ["-w", "5", "--stagger"],
                 ["-w", "99999999999999999999999", missing],
                 ["-e", "-p", missing, missing],               # two operations
                 ["-u", "-w", missing]):
        r = _run(*args)
        assert r.returncode == 1 and r.stdout == b"" and b"USAGE: bedops" in r.stderr, args
    # a value that does not match in full is a file
    r = _run("-e", "5x", missing)
    assert r.returncode == errno_nodata() and b"does not exist (5x)" in r.stderr and r.stdout == b""
    r = _run("-w", "-x", "--stagger", "3", missing)
    assert r.returncode == errno_nodata() and b"does not exist" in r.stderr
    r = _run("-u", missing)
    assert r.returncode == errno_nodata()
    # long options may be cut short while one name is meant, as before
    for args in (["--merg", missing], ["--every", "--device", "0", missing], ["--chop=5", "--stag=2", missing],
                 ["--not-el", "5%", missing, missing], ["--el", missing, missing]):
        r = _run(*args)
        assert r.returncode == errno_nodata() and r.stdout == b"", args
    for args in (["--e", missing, missing], ["--d", missing], ["--", missing], ["--merge=1", missing]):
        r = _run(*args)
        assert r.returncode == 1 and r.stdout == b"" and b"USAGE: bedops" in r.stderr, args


def errno_nodata():
    import errno
    return errno.ENODATA
