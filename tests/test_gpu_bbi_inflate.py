"""GPU: the zlib stage of bigwig2bed / bigbed2bed alone (Starch.bbi_inflate): the
inflater's decoder driven over the table of a file's zlib blocks, the extent of
the deflate data and the Adler-32 of the output checked on the device.

Every block must inflate to zlib.decompress of the same bytes.  The slots are
packed `gap` bytes apart with gap odd, so their strides are no multiples of 16;
the gap behind every slot holds 0xA5 and must still hold it, and the zero
padding behind the last uploaded input byte must still be zero."""
import zlib

import pytest

from tests import bbi_cases as cases
from tests import bbi_expect as expect
from tests import bbi_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import starch_amd
    c = starch_amd.Starch(0)
    yield c
    c.close()


def check(ctx, data, gap, region=None):
    info = oracle.read(data)
    sel = oracle.selected(info, region)
    area, table, pad_ok = ctx.bbi_inflate(data, region=region, gap=gap)
    assert pad_ok and len(table) == len(sel)
    want = bytearray(b"\xa5" * len(area))                                   # the gaps, and what a block leaves of its slot
    end = 0
    for k, (off, n) in zip(sel, table):
        _, at, size = info["blocks"][k]
        assert off >= end and off + n + gap <= len(area), k
        want[off:off + n] = zlib.decompress(data[at:at + size])
        end = off + n + gap
    assert area == bytes(want)
    return table


@pytest.mark.parametrize("name", ("deflate_stored", "deflate_fixed", "deflate_dynamic", "adler_sizes", "many_blocks", "exact_ubs",
                                  "sizing_walk", "three_sections", "bed_framing"))
@pytest.mark.parametrize("gap", (3, 7))
def test_blocks_inflate_to_what_zlib_gives(ctx, name, gap):
    data = cases.good()[name][1]
    table = check(ctx, data, gap)
    info = oracle.read(data)
    if name == "adler_sizes":
        assert [n for _, n in table] == [5551, 5552, 5553, 13]
    if name == "many_blocks":
        assert len(table) == 1100
    if name == "sizing_walk":                                                # slots of what the blocks hold, not of the declared size
        assert info["ubs"] == cases.BIG_UBS and table[-1][0] + table[-1][1] + gap < 1 << 20
        assert [table[k + 1][0] - table[k][0] for k in range(len(table) - 1)] == [n + gap for _, n in table[:-1]]
    elif name == "exact_ubs":                                                # a block that fills its slot to the last byte
        assert max(n for _, n in table) == info["ubs"]
        assert [table[k + 1][0] - table[k][0] for k in range(len(table) - 1)] == [info["ubs"] + gap] * (len(table) - 1)


def test_a_region_uploads_and_inflates_its_blocks_only(ctx):
    data = cases.good()["regions"][1]
    for rg in cases.REGIONS:
        check(ctx, data, 5, region=rg)
    check(ctx, cases.good()["deep_trees"][1], 1, region=b"chrX")           # the last blocks: the upload ends at the file's index


@pytest.mark.parametrize("name", sorted(expect.ZLIB_BAD))
def test_bad_zlib_blocks_are_refused_with_their_number(ctx, name):
    import starch_amd
    kind, data = cases.bad()[name]
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bbi_inflate(data, gap=3)
    tool = "bigwig2bed" if kind == "bigwig" else "bigbed2bed"
    assert e.value.code == -12 and "%s: block %d: " % (tool, expect.ZLIB_BAD[name]) in str(e.value), str(e.value)
    word = {"past_slot": "more output than", "fdict": "FDICT", "zlib_header": "header check", "extent": "does not end at the trailer",
            "adler_flip": "Adler-32 mismatch", "adler_ff_flip": "Adler-32 mismatch"}[name]
    assert word in str(e.value), str(e.value)
    with pytest.raises(starch_amd.StarchError) as e:                        # nothing is left behind
        ctx._output()
    assert e.value.code == -4
    check(ctx, cases.good()["deflate_fixed"][1], 3)                          # and the context serves a good call


def test_an_uncompressed_file_has_no_zlib_stage(ctx):
    import starch_amd
    with pytest.raises(starch_amd.StarchError) as e:
        ctx.bbi_inflate(cases.good()["uncompressed"][1])
    assert e.value.code == -2
