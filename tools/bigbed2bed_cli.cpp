// tools/bigbed2bed_cli.cpp -- the `bigbed2bed` command: a bigBed file to BED on the
// GPU (tools/bbi2bed_cli.hpp has the command line and the exit codes).
#include "bbi2bed_cli.hpp"

static const char* kHelp =
    "USAGE: bigbed2bed [--output=bed|starch] [--do-not-sort] [--region chr[:a-b]] [--device N] file\n\n"
    "  The blocks of a bigBed file are uploaded, inflated, cut into records and converted to BED on the\n"
    "  GPU and written to stdout, in sort-bed's order unless --do-not-sort is given.  The file is\n"
    "  memory-mapped; stdin is not supported, because the format needs seeks.\n\n"
    "  Columns: chromosome, start, end, then the rest of the record as the file holds it (TAB-separated\n"
    "  columns from the fourth on); a record with an empty rest gives three columns.\n\n"
    "  --output=bed      BED text (the default)\n"
    "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
    "  --do-not-sort     leave the lines in block order\n"
    "  --region R        chr, or chr:start-end (0-based, half-open): only the blocks the file's index\n"
    "                    gives for R are uploaded, and only records that meet R are written\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Modelled on UCSC's bigBedToBed, unverified against UCSC's tools.  Zoom levels, autoSql and extra\n"
    "  indices are not read.  A block that does not fit the format (it does not end on a record's zero\n"
    "  byte, a newline inside a record, start above end) is reported with its number in the file's block\n"
    "  table (from 0) and nothing is written.  A bigWig file is refused with exit status 2.\n";

int main(int argc, char** argv)
{
    const bbi_cli::Command cmd = {"bigbed2bed", STARCH_BBI_BIGBED, 0x8789F2EBu, 0x888FFC26u, kHelp};
    return bbi_cli::run(cmd, argc, argv);
}
