"""The deflate / gzip / BGZF writer of the inflater's tests against CPython's
zlib and tests/deflate_trace.py, and what the inflater's host side answers
without a GPU: the BGZF plan (starch_amd.gunzip_plan), the new symbols of the
library, and the starch-zcat command's help text, bad command lines and
--list."""
import ctypes
import errno
import gzip
import os
import subprocess
import zlib

import pytest

import starch_amd
from tests import deflate_trace as dt
from tests import deflate_writer as dw
from tests import gunzip_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "starch_amd", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_help", "starch-zcat.txt")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")

VALID = gunzip_cases.valid_cases() + gunzip_cases.header_cases()
INVALID = gunzip_cases.invalid_cases()


def _zcat(*args, **kw):
    kw.setdefault("stdin", subprocess.DEVNULL)
    return subprocess.run([os.path.join(BUILD, "starch-zcat")] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=60, env=NO_GPU, **kw)


def _deflate_of(gz):
    """The raw deflate bytes of a one-member gzip file without optional fields (plus its trailer)."""
    assert gz[3] == 0
    return gz[10:]


@pytest.mark.parametrize("name,gz,text", VALID, ids=[c[0] for c in VALID])
def test_valid_streams_inflate_under_zlib(name, gz, text):
    assert dw.referee(gz) == text
    assert gzip.decompress(gz) == text


@pytest.mark.parametrize("name,gz,text", gunzip_cases.valid_cases(), ids=[c[0] for c in gunzip_cases.valid_cases()])
def test_valid_streams_inflate_under_the_trace_reader(name, gz, text):
    blocks, end = dt.inflate(_deflate_of(gz))
    assert b"".join(b.out for b in blocks) == text
    assert (end + 7) // 8 == len(gz) - 10 - 8


@pytest.mark.parametrize("name,gz,bad,reason", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_streams_raise_in_zlib(name, gz, bad, reason):
    with pytest.raises(zlib.error):
        dw.referee(gz)


def test_writer_against_zlib_streams():
    # the writer re-encodes what the trace reader saw in zlib's own streams
    text = b"".join(b"chr%d\t%d\t%d\tid%d\n" % (i % 3, i * 10, i * 10 + 7, i) for i in range(400))
    for level, strategy in ((9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (1, zlib.Z_HUFFMAN_ONLY)):
        blocks, _ = dt.inflate(dw.raw_deflate(text, level, strategy))
        bw = dw.BitWriter()
        for b in blocks:
            if b.btype == 0:
                dw.stored_block(bw, b.out, b.bfinal)
            elif b.btype == 1:
                dw.fixed_block(bw, b.tokens, b.bfinal)
            else:
                dw.dynamic_block(bw, b.tokens, b.bfinal, lit_lens=b.lit_lens, dist_lens=b.dist_lens)
        assert zlib.decompress(bw.getvalue(), -15) == text
    assert dt.replay(dw.lz_tokens(text)) == text


def test_bgzf_framing():
    text = bytes(range(256)) * 300
    z = dw.bgzf_file(text, block=65280)
    assert dw.referee(z) == text
    assert len(dw.bgzf_eof()) == 28
    assert dw.bgzf_eof() == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_plan_of_a_bgzf_file():
    text = b"".join(b"chr1\t%d\t%d\n" % (i, i + 1) for i in range(30000))[:1 + 65280 + 65536 + 5000]
    pieces = [text[:1], text[1:65281], text[65281:65281 + 65536], b"", text[65281 + 65536:]]
    z, want = b"", []
    for p in pieces:
        m = dw.bgzf_member(dw.raw_deflate(p), p)
        want.append({"in_off": len(z), "in_len": len(m), "out_off": sum(w["isize"] for w in want), "isize": len(p),
                     "crc": zlib.crc32(p)})
        z += m
    eof = dw.bgzf_eof()
    want.append({"in_off": len(z), "in_len": 28, "out_off": len(text), "isize": 0, "crc": 0})
    z += eof
    assert starch_amd.is_gzip(z) and not starch_amd.is_gzip(text) and not starch_amd.is_gzip(z[:17])
    is_bgzf, members = starch_amd.gunzip_plan(z)
    assert is_bgzf and members == want
    # a BC member with more subfields, a name and a header CRC
    def member(bsize):
        return dw.gzip_member(dw.raw_deflate(b"xy"), b"xy", name=b"f", hcrc=True,
                              extra=b"AB\x01\x00q" + b"BC\x02\x00" + bsize.to_bytes(2, "little"))
    m = member(len(member(0)) - 1)
    assert dw.referee(m) == b"xy"
    assert starch_amd.gunzip_plan(m) == (True, [{"in_off": 0, "in_len": len(m), "out_off": 0, "isize": 2,
                                                 "crc": zlib.crc32(b"xy")}])


def test_plan_of_generic_gzip():
    assert starch_amd.gunzip_plan(gzip.compress(b"hello")) == (False, [])
    # one member without BC makes the whole input generic
    assert starch_amd.gunzip_plan(dw.bgzf_file(b"abc") + gzip.compress(b"hello")) == (False, [])


def test_plan_refusals():
    z = dw.bgzf_file(b"abc" * 1000)
    for bad in (z[:-1],                                                     # BSIZE past the end
                dw.bgzf_member(dw.raw_deflate(b"abc"), b"abc", bsize=4000),
                dw.bgzf_member(dw.raw_deflate(b"abc"), b"abc", isize=65537),   # more than a BGZF member holds
                z + b"trailing bytes that are no member",
                dw.bgzf_file(b"abc", eof=False) + dw.gzip_member(dw.raw_deflate(b"a"), b"a", flg=0x40, extra=b""),
                b"plain text, long enough to be looked at\n"):
        with pytest.raises(starch_amd.StarchError) as e:
            starch_amd.gunzip_plan(bad)
        assert e.value.code == -12


def test_constants_and_symbols():
    c = starch_amd.gunzip_constants()
    assert c["bgzf_max"] == 65536 and c["copy_width"] == 64
    assert c["window_bytes"] >= 32768 + 258 and c["window_bytes"] % 16 == 0 and c["window_bytes"] <= 48 << 10
    assert 9 <= c["primary_bits"] <= 12
    L = ctypes.CDLL(os.path.join(BUILD, "libstarch_amd.so"))
    for sym in ("starch_gunzip_host", "starch_gunzip_device", "starch_gunzip_plan", "starch_gunzip_get_stats",
                "starch_gunzip_constants", "starch_is_gzip"):
        assert hasattr(L, sym), sym
    for m in ("gunzip", "gunzip_stats"):
        assert callable(getattr(starch_amd.Starch, m))


def test_zcat_help_and_version():
    r = _zcat("--help")
    assert r.returncode == 0 and r.stderr == b""
    with open(GOLDEN, "rb") as f:
        assert r.stdout == f.read()
    r = _zcat("--version")
    assert r.returncode == 0 and r.stdout.startswith(b"starch-zcat\n  version: ")


def test_zcat_bad_command_lines(tmp_path):
    with open(GOLDEN, "rb") as f:
        usage = f.read()
    for argv, first in ((["--no-such-option"], b"Error: unsupported or unknown option: --no-such-option"),
                        (["-", "-"], b"Error: stdin (-) may be named once")):
        r = _zcat(*argv)
        head, _, rest = r.stderr.partition(b"\n")
        assert r.returncode == 2 and r.stdout == b"" and head == first and rest == usage
    missing = str(tmp_path / "none.gz")
    r = _zcat(missing)
    assert r.returncode == errno.ENODATA and r.stderr == b"Error: Input file does not exist (" + missing.encode() + b")\n"
    # an accepted command line gets as far as asking for a device
    p = tmp_path / "a.gz"
    p.write_bytes(gzip.compress(b"x"))
    r = _zcat(str(p))
    assert r.returncode == errno.EINVAL and r.stdout == b"" and r.stderr.startswith(b"Error: no GPU context")


def test_zcat_list_needs_no_device(tmp_path):
    text = b"chr1\t1\t2\n" * 10000
    z = dw.bgzf_file(text, block=65280)
    a, b, c = tmp_path / "a.bed.gz", tmp_path / "b.gz", tmp_path / "c.gz"
    a.write_bytes(z)
    b.write_bytes(gzip.compress(text))
    c.write_bytes(z[:-5])
    r = _zcat("--list", str(a), str(b))
    assert r.returncode == 0 and r.stderr == b""
    lines = r.stdout.decode().splitlines()
    _, members = starch_amd.gunzip_plan(z)
    assert lines[-1] == "generic" and len(lines) == len(members) + 1
    for ln, m in zip(lines, members):
        assert ln == "%d\t%d\t%d\t%d\t%08x" % (m["in_off"], m["in_len"], m["out_off"], m["isize"], m["crc"])
    r = _zcat("--list", stdin=open(a, "rb"))
    assert r.returncode == 0 and r.stdout.decode().splitlines() == lines[:-1]
    r = _zcat("--list", str(c))
    assert r.returncode == errno.EINVAL and r.stdout == b"" and b"malformed or corrupt" in r.stderr
