"""What the tests of bigwig2bed / bigbed2bed share beyond tests/bbi_cases.py: the
block that every bad() case's comment names, the case files of
tools/bbi_rec_check.cpp, and the expected text of a good case (TEST
INFRASTRUCTURE ONLY)."""
import struct

from tests import bbi_cases as cases
from tests import bbi_oracle as oracle

# bad() case -> the number (in the file's block table) of the block that is wrong.
RECORD_BAD = {"section_size": 1, "type4": 0, "chrom_range": 2, "start_end": 1, "adler_one_byte": 0, "adler_ff": 0,
              "last_not_zero": 1, "bed_newline": 1, "bed_order": 0}           # the inflated bytes are wrong
ZLIB_BAD = {"past_slot": 1, "fdict": 1, "zlib_header": 0, "extent": 0, "adler_flip": 0, "adler_ff_flip": 0}   # the zlib stage refuses
assert sorted(list(RECORD_BAD) + list(ZLIB_BAD)) == sorted(cases.bad())


def region_words(info, region):
    """(mode, chromId, start, end) of a region as the converters' kernels take it; chromId 0xffffffff: absent."""
    if region is None:
        return 0, 0, 0, 0
    name = region if isinstance(region, bytes) else region[0]
    ids = [k for k, (n, _) in enumerate(info["chroms"]) if n == name]
    cid = ids[0] if ids else 0xFFFFFFFF
    return (1, cid, 0, 0) if isinstance(region, bytes) else (2, cid, region[1], region[2])


def case_file(data, region=None):
    """The case file of tools/bbi_rec_check.cpp for the blocks that `region` selects: their inflated bytes."""
    info = oracle.read(data)
    sel = oracle.selected(info, region)
    mode, cid, a, b = region_words(info, region)
    out = struct.pack("<IIIIIIQQ", 1 if info["kind"] == "bigwig" else 2, len(info["chroms"]), len(sel), mode, cid, 0, a, b)
    for name, _ in info["chroms"]:
        out += struct.pack("<I", len(name)) + name
    for k in sel:
        p = oracle.payload(data, info, k)
        out += struct.pack("<QQ", k, len(p)) + p
    return out


def expected_text(data, region=None):
    """The unsorted lines of a file: bigWig as bedGraph (chrom, start, end, value)."""
    return oracle.expected(data, region, bedgraph=True)[0]
