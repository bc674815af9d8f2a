// tools/bigwig2bed_cli.cpp -- the `bigwig2bed` command: a bigWig file to BED
// (bedGraph columns) on the GPU (tools/bbi2bed_cli.hpp has the command line and
// the exit codes).
#include "bbi2bed_cli.hpp"

static const char* kHelp =
    "USAGE: bigwig2bed [--output=bed|starch] [--do-not-sort] [--region chr[:a-b]] [--device N] file\n\n"
    "  The blocks of a bigWig file are uploaded, inflated, checked and converted to BED on the GPU and\n"
    "  written to stdout, in sort-bed's order unless --do-not-sort is given.  The file is memory-mapped;\n"
    "  stdin is not supported, because the format needs seeks.\n\n"
    "  Columns: chromosome, start, end, value.  A bedGraph item gives its own start and end, a\n"
    "  variableStep item start and start + span, a fixedStep item chromStart + i * step and that + span.\n"
    "  The value is C's %g of the float32, computed exactly; infinities and NaNs print inf, -inf and nan.\n\n"
    "  --output=bed      BED text (the default)\n"
    "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
    "  --do-not-sort     leave the lines in block order\n"
    "  --region R        chr, or chr:start-end (0-based, half-open): only the blocks the file's index\n"
    "                    gives for R are uploaded, and only records that meet R are written\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Modelled on UCSC's bigWigToBedGraph, unverified against UCSC's tools.  Zoom levels are not read.\n"
    "  A block that does not fit the format is reported with its number in the file's block table\n"
    "  (from 0) and nothing is written.  A bigBed file is refused with exit status 2.\n";

int main(int argc, char** argv)
{
    const bbi_cli::Command cmd = {"bigwig2bed", STARCH_BBI_BIGWIG, 0x888FFC26u, 0x8789F2EBu, kHelp};
    return bbi_cli::run(cmd, argc, argv);
}
