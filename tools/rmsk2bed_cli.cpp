// tools/rmsk2bed_cli.cpp -- the `rmsk2bed` command: RepeatMasker .out text to BED
// on the GPU (tools/align2bed_cli.hpp has the command line and the exit codes).
#include "align2bed_cli.hpp"

static const char* kHelp =
    "USAGE: rmsk2bed [--output=bed|starch] [--do-not-sort] [--keep-header] [--device N] [file | -]\n\n"
    "  RepeatMasker .out text (no file, or -: stdin) is converted to BED on the GPU and written to\n"
    "  stdout, in sort-bed's order unless --do-not-sort is given.  Lines end at a newline; a\n"
    "  carriage return is an ordinary byte.  Tokens are separated by runs of spaces and tabs; a\n"
    "  record has 15 tokens, or 16 with a last * .\n\n"
    "  Columns, tab-joined: query, begin-1, end, repeat, SW score, strand (C becomes -), %div, %del,\n"
    "  %ins, (left), class/family, the three repeat positions as written, ID, and * when present.\n\n"
    "  --output=bed      BED text (the default)\n"
    "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
    "  --do-not-sort     leave the lines in input order\n"
    "  --keep-header     header line K (from 0: a line without a token, a line whose first token is\n"
    "                    SW or score) becomes  _header TAB K TAB K+1 TAB line ; by default header\n"
    "                    lines are dropped\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Not supported: --max-mem, --sort-tmpdir, --zero-indexed, --do-not-split.\n\n"
    "  The definitions are modelled on BEDOPS' convert2bed (its rmsk2bed), but they are unverified\n"
    "  against a BEDOPS binary.  Known or possible differences:\n"
    "    The numbers other than begin and end are copied unread.\n\n"
    "  A line that does not fit the format is reported with its line number (from 1) and nothing\n"
    "  is written.\n";

int main(int argc, char** argv)
{
    const align_cli::Command cmd = {"rmsk2bed", STARCH_ALIGN_RMSK, 0, kHelp};
    return align_cli::run(cmd, argc, argv);
}
