"""What the thirteen commands show before any GPU work: the help text byte for
byte, the version line, and the exit codes and messages for a missing input,
an unknown option, stdin named twice and every other bad command line of the
commands whose option parsers are built from tools/cli_common.hpp.  None of
this opens a device.

tests/golden/cli_help/<command>.txt is the --help output of the commands as
they were before their shared code moved into tools/cli_common.hpp, and
tests/golden/cli_usage.json (command, arguments, exit status, first line of
stderr) what they answered then; {bed} in it stands for a small BED file.  Checks
that test_sortbed_cli.py, test_setops_cpu.py, test_bedops2_cpu.py and
test_map_cpu.py already make (sort-bed, bedops and bedmap: missing input,
unknown option) are not repeated here."""
import errno
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help")
COMMANDS = ("starch3", "unstarch", "starchcat", "sort-bed", "bedops", "bedmap", "closest-features", "convert2bed",
            "bedmap-elements", "bedmap-scores", "sam2bed", "psl2bed", "rmsk2bed")
with open(os.path.join(ROOT, "tests", "golden", "cli_usage.json")) as _f:
    USAGE_TABLE = json.load(_f)
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
MISSING = os.path.join(ROOT, "no", "such", "file")


def _run(cmd, *args, **kw):
    kw.setdefault("stdin", subprocess.DEVNULL)
    return subprocess.run([os.path.join(BUILD, cmd)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=60, **kw)


@pytest.mark.parametrize("cmd", COMMANDS)
def test_help_text(cmd):
    r = _run(cmd, "--help", env=NO_GPU)
    assert r.returncode == 0 and r.stderr == b""
    with open(os.path.join(GOLDEN, cmd + ".txt"), "rb") as f:
        assert r.stdout == f.read()


# A bad command line: its message, then the usage text, and exit 2.  An accepted one gets as far as
# asking for a device, and with none visible that is EINVAL after one line.
@pytest.mark.parametrize("cmd", sorted(set(e["cmd"] for e in USAGE_TABLE)))
def test_bad_command_lines(cmd, tmp_path):
    bed = tmp_path / "in.bed"
    bed.write_bytes(b"chr1\t1\t2\n")
    with open(os.path.join(GOLDEN, cmd + ".txt"), "rb") as f:
        usage = f.read()
    entries = [e for e in USAGE_TABLE if e["cmd"] == cmd]
    assert entries and {e["status"] for e in entries} == {2, errno.EINVAL}
    for e in entries:
        r = _run(cmd, *[a.replace("{bed}", str(bed)) for a in e["argv"]], env=NO_GPU)
        first, _, rest = r.stderr.partition(b"\n")
        assert r.returncode == e["status"] and r.stdout == b"", e
        assert first == e["stderr_first_line"].replace("{bed}", str(bed)).encode(), e
        assert rest == (usage if e["status"] == 2 else b""), e


@pytest.mark.parametrize("cmd", ("starch3", "unstarch", "starchcat"))
def test_version_line(cmd):
    r = _run(cmd, "--version", env=NO_GPU)
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout.startswith(cmd.encode() + b"\n  version: ") and r.stdout.count(b"\n") == 2


# starchcat, like the others: ENODATA for a missing input (with --plan too, which opens
# no GPU either), 1 with the usage for an unknown option
@pytest.mark.parametrize("cmd", ("unstarch", "starchcat"))
def test_missing_input_and_unknown_option(cmd):
    r = _run(cmd, MISSING, env=NO_GPU)
    assert r.returncode == errno.ENODATA and r.stdout == b""
    assert r.stderr == b"Error: Input file does not exist (" + MISSING.encode() + b")\n"
    r = _run(cmd, "--no-such-option", MISSING, env=NO_GPU)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.startswith(cmd.encode() + b"\n  version: ") and b"USAGE: " + cmd.encode() in r.stderr


def test_starchcat_plan_of_a_missing_input():
    r = _run("starchcat", "--plan", MISSING, env=NO_GPU)
    assert r.returncode == errno.ENODATA and b"does not exist" in r.stderr and r.stdout == b""


@pytest.mark.parametrize("cmd, args, status", (("bedops", ("-m", "-", "-"), 1), ("bedmap", ("--count", "-", "-"), 2)))
def test_stdin_named_twice(cmd, args, status):
    r = _run(cmd, *args, env=NO_GPU)
    assert r.returncode == status and r.stdout == b""
    assert r.stderr.startswith(b"Error: stdin (-) may be named once\n")


# the inputs are read and the device is asked for; with none visible every command says so the same way
@pytest.mark.parametrize("cmd, args", (("sort-bed", ()), ("bedops", ("-m",)), ("bedmap", ("--count",)), ("unstarch", ())))
def test_no_visible_device(cmd, args, tmp_path):
    p = tmp_path / "in.bed"
    p.write_bytes(b"chr1\t1\t2\n")
    r = _run(cmd, *(args + (str(p),)), env=NO_GPU)
    assert r.returncode == errno.EINVAL and r.stdout == b""
    assert r.stderr == b"Error: no GPU context (HIP device error)\n"
