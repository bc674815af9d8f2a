// tools/psl2bed_cli.cpp -- the `psl2bed` command: BLAT's PSL text to BED on the GPU
// (tools/align2bed_cli.hpp has the command line and the exit codes).
#include "align2bed_cli.hpp"

static const char* kHelp =
    "USAGE: psl2bed [--output=bed|starch] [--do-not-sort] [--keep-header] [--split] [--device N] [file | -]\n\n"
    "  PSL text (no file, or -: stdin) is converted to BED on the GPU and written to stdout, in\n"
    "  sort-bed's order unless --do-not-sort is given.  Lines end at a newline; a carriage return\n"
    "  is an ordinary byte.  A record has exactly 21 tab-separated non-empty fields.\n\n"
    "  Columns: tName, tStart, tEnd, qName, matches, strand, qSize, misMatches, repMatches, nCount,\n"
    "  qNumInsert, qBaseInsert, tNumInsert, tBaseInsert, qStart, qEnd, tSize, blockCount, blockSizes,\n"
    "  qStarts, tStarts.\n\n"
    "  --output=bed      BED text (the default)\n"
    "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
    "  --do-not-sort     leave the lines in input order\n"
    "  --keep-header     header line K (from 0: an empty line; when line 1 begins with psLayout,\n"
    "                    every line up to the first that begins with -----) becomes\n"
    "                    _header TAB K TAB K+1 TAB line ; by default header lines are dropped\n"
    "  --split           one line per block: tStarts[k], tStarts[k] + blockSizes[k]; when the strand\n"
    "                    has two characters and the second is -, tSize - tStarts[k] - blockSizes[k],\n"
    "                    tSize - tStarts[k]\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Not supported: --max-mem, --sort-tmpdir, --zero-indexed, --do-not-split.\n\n"
    "  The definitions are modelled on BEDOPS' convert2bed (its psl2bed), but they are unverified\n"
    "  against a BEDOPS binary.  Known or possible differences:\n"
    "    A psLayout header without a line of dashes is an error.\n"
    "    Without --split, blockSizes and tStarts are copied unread; with it they must hold exactly\n"
    "    blockCount comma-terminated numbers.\n\n"
    "  A line that does not fit the format is reported with its line number (from 1) and nothing\n"
    "  is written.\n";

int main(int argc, char** argv)
{
    const align_cli::Command cmd = {"psl2bed", STARCH_ALIGN_PSL, align_cli::TAKES_SPLIT, kHelp};
    return align_cli::run(cmd, argc, argv);
}
