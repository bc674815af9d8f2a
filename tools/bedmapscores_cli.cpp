// tools/bedmapscores_cli.cpp -- the `bedmap-scores` command: for every line of a
// sorted reference, exact statistics (sum, mean, min, max, median, k-th) of the
// scores of the map lines that satisfy an overlap criterion, computed on the GPU
// (starch_mapsc_host).  Inputs are sorted BED files, .starch archives
// (recognised by their magic) or stdin; one line per reference line goes to
// stdout.
//
// Exit codes: 2 for a bad command line or an option this command does not have
// (answered before a GPU is opened), otherwise as bedmap (tools/bedmap_cli.cpp):
// ENODATA for a missing input, EINVAL for a data error (the library's text
// names the input and the line), ENOMEM, EIO.
#include "cli_common.hpp"

static const char* kHelp =
    "USAGE: bedmap-scores [--echo] [--count] [--indicator] [--sum] [--mean] [--min] [--max]\n"
    "                     [--median] [--kth F] [--min-element] [--max-element] [criterion]\n"
    "                     [--prec P] [--delim S] [--skip-unmapped] [--device N] ref [map]\n\n"
    "  ref and map are sorted BED (see sort-bed) or .starch archives, which are recognised\n"
    "  by their first four bytes and not by their names; - is stdin and may be named once.\n"
    "  Without map, ref is mapped onto itself.  Every line needs stop > start.\n"
    "  One line is written per line of ref, in ref's order: the chosen columns in the\n"
    "  order of the options, joined by the delimiter.  The hits of a ref line are the map\n"
    "  lines on its chromosome that satisfy the criterion, in map order; the score of a\n"
    "  hit is column 5 of its map line.\n\n"
    "  Columns:\n"
    "  --echo               the ref line, every column of it\n"
    "  --count              the number of hits\n"
    "  --indicator          1 if there is a hit, else 0\n"
    "  --sum                the sum of the hits' scores\n"
    "  --mean               the sum divided by the number of hits\n"
    "  --min, --max         the least and the greatest score\n"
    "  --median             the middle score in ascending order, or the mean of the two\n"
    "                       middle ones when the number of hits is even\n"
    "  --kth F              the k-th score in ascending order, k = ceil(F * hits)\n"
    "  --min-element        the map line with the least score, every column of it; among\n"
    "                       equal scores the first in map order\n"
    "  --max-element        the same for the greatest score\n"
    "  A ref line without a hit has NAN in the columns from --sum on.\n\n"
    "  Criterion, at most one (default --bp-ovr 1):\n"
    "  --bp-ovr N           at least N shared bases, N >= 1\n"
    "  --range N            at least one base shared with the ref line padded by N bases\n"
    "                       on both sides (never below 0)\n"
    "  --fraction-ref F     shared bases / length of the ref line >= F\n"
    "  --fraction-map F     shared bases / length of the map line >= F\n"
    "  --fraction-both F    both of these\n"
    "  --fraction-either F  either of these\n"
    "  --exact              the same start and stop as the ref line\n"
    "  F is a decimal above 0 and up to 1 with at most 9 digits after the point (1, 1.0,\n"
    "  0.5, .25); it is used exactly, without floating point.\n\n"
    "  --prec P             digits after the point of --sum to --kth, 0 to 9 (default 6)\n"
    "  --delim S            the column delimiter, 1 to 8 bytes (default |)\n"
    "  --skip-unmapped      leave out ref lines without a hit\n"
    "  --device N           GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  With no column option: --echo --mean.\n"
    "  A score is an optional sign, up to 9 digits, and a point with up to 9 digits (7, +7,\n"
    "  -.5, 3., 0.25); every result is computed exactly and rounded once, ties to even.\n"
    "  Not supported: --stdev, --variance, --cv, --mad, --tmean, --wmean,\n"
    "  --echo-map-id-uniq, the --echo-map columns (see bedmap-elements), --bases and its\n"
    "  variants (see bedmap), --chrom, --ec, --header, --sci, --faster, --sweep-all.\n\n"
    "  This is modelled on BEDOPS' bedmap for the options above, but it is unverified\n"
    "  against a BEDOPS binary.  Known differences: scores are exact decimals, not strtod\n"
    "  doubles (an exponent form or more than 9+9 digits is a data error); rounding is\n"
    "  exact, ties to even, not printf of a double; there is no negative zero; element\n"
    "  ties go to map order; --kth is defined as above.\n\n"
    "  An unsorted input, a line with stop <= start, a malformed line or, when a column\n"
    "  from --sum on is asked for, a hit without a valid score is reported with its input\n"
    "  number (ref is 0, map is 1) and line number (from 1); nothing is written.\n";
static const cli::Command kCmd = {"bedmap-scores", "0.1 (mi355x)", kHelp, 2};   // 2: the exit code for a bad command line

int main(int argc, char** argv)
{
    enum { O_CRIT = 64, O_DELIM = 256, O_PREC, O_SKIP, O_REFUSED };
    static struct option longs[] = {{"echo", no_argument, nullptr, STARCH_MAPSC_ECHO + 1},
                                    {"count", no_argument, nullptr, STARCH_MAPSC_COUNT + 1},
                                    {"indicator", no_argument, nullptr, STARCH_MAPSC_INDICATOR + 1},
                                    {"sum", no_argument, nullptr, STARCH_MAPSC_SUM + 1},
                                    {"mean", no_argument, nullptr, STARCH_MAPSC_MEAN + 1},
                                    {"min", no_argument, nullptr, STARCH_MAPSC_MIN + 1},
                                    {"max", no_argument, nullptr, STARCH_MAPSC_MAX + 1},
                                    {"median", no_argument, nullptr, STARCH_MAPSC_MEDIAN + 1},
                                    {"kth", required_argument, nullptr, STARCH_MAPSC_KTH + 1},
                                    {"min-element", no_argument, nullptr, STARCH_MAPSC_MIN_ELEMENT + 1},
                                    {"max-element", no_argument, nullptr, STARCH_MAPSC_MAX_ELEMENT + 1},
                                    CLI_CRITERION_OPTIONS(O_CRIT),
                                    {"prec", required_argument, nullptr, O_PREC},
                                    {"delim", required_argument, nullptr, O_DELIM},
                                    {"skip-unmapped", no_argument, nullptr, O_SKIP},
                                    CLI_COMMON_OPTIONS,
                                    {"ec", no_argument, nullptr, O_REFUSED},   // or getopt reads it as --echo
                                    {nullptr, 0, nullptr, 0}};
    starch_mapsc_options opt;
    memset(&opt, 0, sizeof opt);
    opt.criterion = STARCH_MAPEL_CRIT_BP_OVR;
    opt.n = 1;
    opt.prec = 6;
    opt.delim_len = 1;
    opt.delim[0] = '|';
    int device = 0;
    bool have_crit = false, have_delim = false, have_prec = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e;
        uint64_t p = 0;
        if (c >= 1 && c <= STARCH_MAPSC_MAX_ELEMENT + 1) {
            e = cli::take_column(kCmd, &opt, c - 1, (std::string("--") + longs[c - 1].name).c_str());
            if (e == cli::GO_ON && c - 1 == STARCH_MAPSC_KTH && !cli::parse_fraction(optarg, &opt.kth_num, &opt.kth_digits))
                e = kCmd.bad("--kth needs a decimal above 0 and up to 1 with at most 9 digits after the point", optarg);
        } else if (c >= O_CRIT && c <= O_CRIT + STARCH_MAPEL_CRIT_EXACT) e = cli::take_criterion(kCmd, &opt, &have_crit, c - O_CRIT, argv);
        else if (c == O_DELIM) e = cli::take_delim(kCmd, opt.delim, &opt.delim_len, &have_delim, "--delim", "a delimiter needs 1 to 8 bytes");
        else if (c == O_PREC) {
            e = cli::take_once(kCmd, &have_prec, "--prec");
            if (e == cli::GO_ON && (!cli::parse_u64(optarg, &p) || p > 9)) e = kCmd.bad("--prec needs a number of digits, 0 to 9", optarg);
            opt.prec = (uint32_t)p;
        } else if (c == O_SKIP) e = cli::take_once(kCmd, &opt.skip_unmapped, "--skip-unmapped");
        else e = cli::take_common(kCmd, c, argv, &device);   // O_REFUSED too: an unknown option
        if (e != cli::GO_ON) return e;
    }
    cli::default_columns(&opt, STARCH_MAPSC_ECHO, STARCH_MAPSC_MEAN);
    return cli::run_two_inputs(kCmd, argc, argv, 1, "one reference and at most one map are needed", device, starch_mapsc_host, &opt);
}
