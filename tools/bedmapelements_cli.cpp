// tools/bedmapelements_cli.cpp -- the `bedmap-elements` command: for every line
// of a sorted reference, the map lines that satisfy an overlap criterion, listed
// on the GPU (starch_mapel_host).  Inputs are sorted BED files, .starch archives
// (recognised by their magic) or stdin; one line per reference line goes to
// stdout.
//
// Exit codes: 2 for a bad command line or an option this command does not have
// (answered before a GPU is opened), otherwise as bedmap (tools/bedmap_cli.cpp):
// ENODATA for a missing input, EINVAL for a data error (the library's text
// names the input and the line), ENOMEM, EIO.
#include "cli_common.hpp"

static const char* kHelp =
    "USAGE: bedmap-elements [columns] [criterion] [--delim S] [--multidelim S] [--skip-unmapped]\n"
    "                       [--device N] ref [map]\n\n"
    "  ref and map are sorted BED (see sort-bed) or .starch archives, which are recognised\n"
    "  by their first four bytes and not by their names; - is stdin and may be named once.\n"
    "  Without map, ref is mapped onto itself.  Every line needs stop > start.\n"
    "  One line is written per line of ref, in ref's order: the chosen columns in the\n"
    "  order of the options, joined by the delimiter.  The hits of a ref line are the map\n"
    "  lines on its chromosome that satisfy the criterion, in map order.\n\n"
    "  Columns, one value per ref line:\n"
    "  --echo               the ref line, every column of it\n"
    "  --count              the number of hits\n"
    "  --indicator          1 if there is a hit, else 0\n"
    "  --echo-ref-size      stop - start of the ref line\n"
    "  --echo-ref-name      chrom:start-stop of the ref line\n"
    "  --echo-ref-row-id    id-N, N the number of the ref line from 1\n"
    "  Columns, one value per hit, joined by the multi-delimiter:\n"
    "  --echo-map           the map line, every column of it\n"
    "  --echo-map-id        its column 4\n"
    "  --echo-map-score     its column 5, copied byte for byte\n"
    "  --echo-map-size      its stop - start\n"
    "  --echo-overlap-size  the bases it shares with the ref line's window\n"
    "  --echo-map-range     chrom, least start and greatest stop of the hits (one BED3,\n"
    "                       empty when there is no hit)\n\n"
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
    "  0.5, .25); it is compared exactly, without floating point.\n\n"
    "  --delim S            the column delimiter, 1 to 8 bytes (default |)\n"
    "  --multidelim S       the delimiter between hits, 1 to 8 bytes (default ;)\n"
    "  --skip-unmapped      leave out ref lines without a hit\n"
    "  --device N           GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  With no column option: --echo --echo-map.  Numbers are unsigned 64-bit.\n"
    "  Not supported: --echo-map-id-uniq, the score operations (--sum, --mean, --min,\n"
    "  --max, --median, ...), --bases and its variants (see bedmap), --chrom, --ec,\n"
    "  --header, --prec, --sci, --faster, --sweep-all.\n\n"
    "  This is modelled on BEDOPS' bedmap for the options above, but it is unverified\n"
    "  against a BEDOPS binary.  Known differences: scores are copied, not reformatted;\n"
    "  --echo-map-range is empty when there is no hit.\n\n"
    "  An unsorted input, a line with stop <= start, a malformed line or a hit that lacks\n"
    "  the column --echo-map-id or --echo-map-score asks for is reported with its input\n"
    "  number (ref is 0, map is 1) and line number (from 1); nothing is written.\n";
static const cli::Command kCmd = {"bedmap-elements", "0.1 (mi355x)", kHelp, 2};   // 2: the exit code for a bad command line

int main(int argc, char** argv)
{
    enum { O_CRIT = 64, O_DELIM = 256, O_MULTI, O_SKIP };
    static struct option longs[] = {{"echo", no_argument, nullptr, STARCH_MAPEL_ECHO + 1},
                                    {"count", no_argument, nullptr, STARCH_MAPEL_COUNT + 1},
                                    {"indicator", no_argument, nullptr, STARCH_MAPEL_INDICATOR + 1},
                                    {"echo-ref-size", no_argument, nullptr, STARCH_MAPEL_ECHO_REF_SIZE + 1},
                                    {"echo-ref-name", no_argument, nullptr, STARCH_MAPEL_ECHO_REF_NAME + 1},
                                    {"echo-ref-row-id", no_argument, nullptr, STARCH_MAPEL_ECHO_REF_ROW_ID + 1},
                                    {"echo-map", no_argument, nullptr, STARCH_MAPEL_ECHO_MAP + 1},
                                    {"echo-map-id", no_argument, nullptr, STARCH_MAPEL_ECHO_MAP_ID + 1},
                                    {"echo-map-score", no_argument, nullptr, STARCH_MAPEL_ECHO_MAP_SCORE + 1},
                                    {"echo-map-size", no_argument, nullptr, STARCH_MAPEL_ECHO_MAP_SIZE + 1},
                                    {"echo-overlap-size", no_argument, nullptr, STARCH_MAPEL_ECHO_OVERLAP_SIZE + 1},
                                    {"echo-map-range", no_argument, nullptr, STARCH_MAPEL_ECHO_MAP_RANGE + 1},
                                    CLI_CRITERION_OPTIONS(O_CRIT),
                                    {"delim", required_argument, nullptr, O_DELIM},
                                    {"multidelim", required_argument, nullptr, O_MULTI},
                                    {"skip-unmapped", no_argument, nullptr, O_SKIP},
                                    CLI_COMMON_OPTIONS,
                                    {nullptr, 0, nullptr, 0}};
    starch_mapel_options opt;
    memset(&opt, 0, sizeof opt);
    opt.criterion = STARCH_MAPEL_CRIT_BP_OVR;
    opt.n = 1;
    opt.delim_len = 1;
    opt.delim[0] = '|';
    opt.multidelim_len = 1;
    opt.multidelim[0] = ';';
    int device = 0;
    bool have_crit = false, have_delim = false, have_multi = false;
    const char* why_length = "a delimiter needs 1 to 8 bytes";
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e;
        if (c >= 1 && c <= STARCH_MAPEL_ECHO_MAP_RANGE + 1) e = cli::take_column(kCmd, &opt, c - 1, argv[optind - 1]);
        else if (c >= O_CRIT && c <= O_CRIT + STARCH_MAPEL_CRIT_EXACT) e = cli::take_criterion(kCmd, &opt, &have_crit, c - O_CRIT, argv);
        else if (c == O_DELIM) e = cli::take_delim(kCmd, opt.delim, &opt.delim_len, &have_delim, "--delim", why_length);
        else if (c == O_MULTI) e = cli::take_delim(kCmd, opt.multidelim, &opt.multidelim_len, &have_multi, "--multidelim", why_length);
        else if (c == O_SKIP) e = cli::take_once(kCmd, &opt.skip_unmapped, "--skip-unmapped");
        else e = cli::take_common(kCmd, c, argv, &device);
        if (e != cli::GO_ON) return e;
    }
    cli::default_columns(&opt, STARCH_MAPEL_ECHO, STARCH_MAPEL_ECHO_MAP);
    return cli::run_two_inputs(kCmd, argc, argv, 1, "one reference and at most one map are needed", device, starch_mapel_host, &opt);
}
