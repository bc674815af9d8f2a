// tools/closestfeatures_cli.cpp -- the `closest-features` command: for every
// line of a sorted input file, the nearest line of a sorted query file to its
// left and to its right, found on the GPU (starch_closest_host).  Inputs are
// sorted BED files, .starch archives (recognised by their magic) or stdin; one
// line per input line goes to stdout.
//
// Exit codes: 2 for a bad command line or an option this closest-features does
// not have (answered before a GPU is opened), otherwise as bedmap
// (tools/bedmap_cli.cpp): ENODATA for a missing input, EINVAL for a data error
// (the library's text names the input and the line), ENOMEM, EIO.
#include "cli_common.hpp"

static const char* kHelp =
    "USAGE: closest-features [--closest|--shortest] [--dist] [--no-overlaps] [--no-ref] [--delim S]\n"
    "                        [--device N] input-file query-file\n\n"
    "  input-file and query-file are sorted BED (see sort-bed) or .starch archives, which\n"
    "  are recognised by their first four bytes and not by their names; - is stdin and may\n"
    "  be named once.  Every line needs stop > start.\n"
    "  One line is written per line of input-file, in its order: the line itself, the\n"
    "  nearest query line on its left and the nearest on its right, joined by the\n"
    "  delimiter; NA where a side has none.  Only lines of one chromosome are compared.\n"
    "  A query line that sorts below the input line (by start, then stop) counts as left,\n"
    "  any other as right; one that overlaps the input line is at distance 0.  Among\n"
    "  equally near lines the left side takes the last, the right side the first.\n\n"
    "  --closest         write the nearer of the two alone; a tie goes to the left one\n"
    "  --shortest        the same as --closest\n"
    "  --dist            after every query line its signed distance in bases: 0 when it\n"
    "                    overlaps, -1 or 1 when it abuts on the left or right; NA for NA\n"
    "  --no-overlaps     query lines that overlap the input line are not considered\n"
    "  --no-ref          do not write the input line\n"
    "  --delim S         the field delimiter, 1 to 8 bytes (default |)\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Not supported: --center, --chrom, --ec, --header.\n\n"
    "  This is modelled on BEDOPS' closest-features for the options above, but it is\n"
    "  unverified against a BEDOPS binary.\n\n"
    "  An unsorted input, a line with stop <= start or a malformed line is reported\n"
    "  with its input number (input-file is 0, query-file is 1) and line number\n"
    "  (from 1); nothing is written.\n";
static const cli::Command kCmd = {"closest-features", "0.1 (mi355x)", kHelp, 2};   // 2: the exit code for a bad command line

int main(int argc, char** argv)
{
    enum { O_CLOSEST = 256, O_DIST, O_NOOVR, O_NOREF, O_DELIM };
    static struct option longs[] = {{"closest", no_argument, nullptr, O_CLOSEST},
                                    {"shortest", no_argument, nullptr, O_CLOSEST},
                                    {"dist", no_argument, nullptr, O_DIST},
                                    {"no-overlaps", no_argument, nullptr, O_NOOVR},
                                    {"no-ref", no_argument, nullptr, O_NOREF},
                                    {"delim", required_argument, nullptr, O_DELIM},
                                    CLI_COMMON_OPTIONS,
                                    {nullptr, 0, nullptr, 0}};
    starch_closest_options opt;
    memset(&opt, 0, sizeof opt);
    opt.delim_len = 1;
    opt.delim[0] = '|';
    int device = 0;
    bool have_delim = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e = cli::GO_ON;
        switch (c) {
            case O_CLOSEST: opt.closest = 1; break;
            case O_DIST: opt.dist = 1; break;
            case O_NOOVR: opt.no_overlaps = 1; break;
            case O_NOREF: opt.no_ref = 1; break;
            case O_DELIM: e = cli::take_delim(kCmd, opt.delim, &opt.delim_len, &have_delim, "--delim", "--delim needs 1 to 8 bytes"); break;
            default: e = cli::take_common(kCmd, c, argv, &device);
        }
        if (e != cli::GO_ON) return e;
    }
    return cli::run_two_inputs(kCmd, argc, argv, 2, "one input file and one query file are needed", device, starch_closest_host, &opt);
}
