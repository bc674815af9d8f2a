"""CPU: the archive index reader behind indexed extraction (starch_archive_index,
starch_amd.list_archive) and the unstarch command's listing forms, none of
which opens a GPU context.

The archive is put together without a GPU: segment texts from the oracle's
transform, bzip2 streams from the oracle's compressor, the index from
starch_amd.build_index.  list_archive is checked field for field against the
index parsed as JSON (parse_archive), an independent reader of the same bytes.
"""
import os
import subprocess

import pytest

import starch_amd
from tests import corpus, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSTARCH = os.path.join(ROOT, "starch_amd", "_build", "unstarch")
ODD_NAME = b"c\thr\xe9 \"x\"\\"          # a tab, a byte >= 0x80, a quote and a backslash


def _archive(base_counts, note, size_slack=0):
    bed = corpus.multi_chrom_bed(3, 400, seed=5, kind="bed6") + b"chr1\t5\t10\tback\n"
    _, osegs = oracle_lib.transform(bed)
    assert len(osegs) == 4
    names = [c for c, _, _ in osegs]
    names[1] = ODD_NAME                   # the index stores any bytes as a name
    streams = [oracle_lib.bz2(t, 9) for _, _, t in osegs]
    segs, off = [], 4
    for k, ((_, lines, text), st) in enumerate(zip(osegs, streams)):
        segs.append(starch_amd.Segment(lines, len(text), off, len(st), len(names[k]), 1, 0x9E3779B9 + k, k,
                                       1000 + k if k != 2 else -7, 2000 + k))
        off += len(st)
    segs[-1].stream_bytes += size_slack
    blob = starch_amd.MAGIC + b"".join(streams)
    blob += starch_amd.build_index(segs, names, off, note=note, level=9, base_counts=base_counts)
    return blob, names, segs


@pytest.mark.parametrize("base_counts,note", [(False, None), (True, "café \"run 7\"\ttab €")])
def test_list_archive_equals_the_json_index(base_counts, note):
    blob, names, segs = _archive(base_counts, note)
    idx, _ = starch_amd.parse_archive(blob)
    info, entries = starch_amd.list_archive(blob)
    assert info == {k: idx["archive"][k] for k in ("compressionFormat", "blockSize100k", "note")}
    assert info["note"] == (note or "") and info["blockSize100k"] == 9 and info["compressionFormat"] == "bzip2"
    assert len(entries) == len(idx["streams"]) == 4
    for e, j, name in zip(entries, idx["streams"], names):
        assert e["chromosome"] == j["chromosome"].encode("latin-1") == name
        assert set(e) == set(j)
        for k in j:
            if k != "chromosome":
                assert e[k] == j[k], k
        assert ("uniqueBaseCount" in e) == base_counts
    if base_counts:
        assert entries[2]["uniqueBaseCount"] == -7


def test_damaged_archives_are_data_errors():
    blob, _, _ = _archive(False, "n")
    bad = {
        "footer cut by one byte": blob[:-1],
        "footer cut away": blob[:-32],
        "footer cut to 20 bytes": blob[:-12],
        "too short for a footer": blob[:20],
        "index offset past the end": blob[:-32] + b"%020d" % (len(blob) + 100) + blob[-12:],
        "stream past the index offset": _archive(False, "n", size_slack=1)[0],
    }
    for what, b in bad.items():
        with pytest.raises(starch_amd.StarchError) as e:
            starch_amd.list_archive(b)
        assert e.value.code == -12, what


def _run(args, **kw):
    return subprocess.run([UNSTARCH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, **kw)


def test_unstarch_listing_forms(tmp_path):
    blob, names, segs = _archive(True, "listing")
    path = str(tmp_path / "a.starch")
    with open(path, "wb") as f:
        f.write(blob)
    want = b"".join(n + b"\t%d\t%d\t%d\t%d\t%d\t%08x\n" % (s.stream_offset, s.stream_bytes, s.line_count, s.text_bytes,
                                                         s.n_blocks, s.combined_crc)
                    for n, s in zip(names, segs))
    r = _run(["--list", path])
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = _run(["--list-chromosomes", path])
    assert r.returncode == 0 and r.stdout == b"".join(n + b"\n" for n in names[:3])   # chr1 comes back: listed once
    r = _run(["--elements", path])
    assert r.returncode == 0 and r.stdout == b"%d\n" % sum(s.line_count for s in segs)
    r = _run(["--elements", "chr1", "chrNone", path])
    assert r.returncode == 0 and r.stdout == b"%d\n" % (segs[0].line_count + segs[3].line_count)
    r = _run(["--bases", path])
    assert r.returncode == 0 and r.stdout == b"%d\n" % sum(s.base_count_nonunique for s in segs)
    r = _run(["--bases-uniq", "chr1", path])
    assert r.returncode == 0 and r.stdout == b"%d\n" % (segs[0].base_count_unique + segs[3].base_count_unique)


def test_unstarch_bases_without_base_counts(tmp_path):
    blob, _, _ = _archive(False, None)
    path = str(tmp_path / "b.starch")
    with open(path, "wb") as f:
        f.write(blob)
    for form in ("--bases", "--bases-uniq"):
        r = _run([form, path])
        assert r.returncode == 2 and r.stdout == b"" and b"base counts" in r.stderr
    r = _run(["--list", str(tmp_path / "missing.starch")])
    assert r.returncode != 0 and r.stdout == b""
