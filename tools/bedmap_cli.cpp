// tools/bedmap_cli.cpp -- the `bedmap` command: for every line of a sorted
// reference, the map lines that overlap it counted and measured on the GPU
// (starch_map_host).  Inputs are sorted BED files, .starch archives (recognised
// by their magic) or stdin; the annotated reference lines go to stdout.
//
// Exit codes: 2 for a bad command line or an option this bedmap does not have
// (answered before a GPU is opened), otherwise as bedops (tools/bedops_cli.cpp):
// ENODATA for a missing input, EINVAL for a data error (the library's text
// names the input and the line), ENOMEM, EIO.
#include "cli_common.hpp"

static const char* kHelp =
    "USAGE: bedmap [--echo] [--count] [--bases] [--bases-uniq] [--indicator] [--echo-ref-size]\n"
    "              [--range N] [--delim S] [--skip-unmapped] [--device N] ref [map]\n\n"
    "  ref and map are sorted BED (see sort-bed) or .starch archives, which are recognised\n"
    "  by their first four bytes and not by their names; - is stdin and may be named once.\n"
    "  Without map, ref is mapped onto itself.  Every line needs stop > start.\n"
    "  One line is written per line of ref, in ref's order: the chosen columns in the\n"
    "  order of the options, joined by the delimiter.  A map line overlaps a ref line\n"
    "  when they share at least one base of the ref line's window, which is the ref\n"
    "  line padded by --range on both sides (never below 0).\n\n"
    "  --echo            the ref line, every column of it\n"
    "  --count           the number of overlapping map lines\n"
    "  --bases           the bases of the window the overlapping map lines cover, each\n"
    "                    map line counted for itself\n"
    "  --bases-uniq      the bases of the window that at least one map line covers\n"
    "  --indicator       1 if a map line overlaps, else 0\n"
    "  --echo-ref-size   stop - start of the ref line (without the padding)\n"
    "  --range N         pad every ref line by N bases on both sides (default 0)\n"
    "  --delim S         the column delimiter, 1 to 8 bytes (default |)\n"
    "  --skip-unmapped   leave out ref lines that no map line overlaps\n"
    "  --bp-ovr 1        the overlap criterion; 1 is the default and the only one here\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  With no column option: --echo --count.  Numbers are unsigned 64-bit.\n"
    "  Not supported: the score operations (--sum, --mean, ...), --echo-map and its\n"
    "  variants, --bp-ovr above 1, --fraction-*, --exact, --bases-uniq-f.\n\n"
    "  This is believed to match BEDOPS' bedmap for the options above, but that is\n"
    "  unverified against a BEDOPS binary.\n\n"
    "  An unsorted input, a line with stop <= start or a malformed line is reported\n"
    "  with its input number (ref is 0, map is 1) and line number (from 1); nothing\n"
    "  is written.\n";
static const cli::Command kCmd = {"bedmap", "0.1 (mi355x)", kHelp, 2};   // 2: the exit code for a bad command line

int main(int argc, char** argv)
{
    enum { O_RANGE = 256, O_DELIM, O_SKIP, O_BPOVR };
    static struct option longs[] = {{"echo", no_argument, nullptr, STARCH_MAP_ECHO + 1},
                                    {"count", no_argument, nullptr, STARCH_MAP_COUNT + 1},
                                    {"bases", no_argument, nullptr, STARCH_MAP_BASES + 1},
                                    {"bases-uniq", no_argument, nullptr, STARCH_MAP_BASES_UNIQ + 1},
                                    {"indicator", no_argument, nullptr, STARCH_MAP_INDICATOR + 1},
                                    {"echo-ref-size", no_argument, nullptr, STARCH_MAP_ECHO_REF_SIZE + 1},
                                    {"range", required_argument, nullptr, O_RANGE},
                                    {"delim", required_argument, nullptr, O_DELIM},
                                    {"skip-unmapped", no_argument, nullptr, O_SKIP},
                                    {"bp-ovr", required_argument, nullptr, O_BPOVR},
                                    CLI_COMMON_OPTIONS,
                                    {nullptr, 0, nullptr, 0}};
    starch_map_options opt;
    memset(&opt, 0, sizeof opt);
    opt.delim_len = 1;
    opt.delim[0] = '|';
    int device = 0;
    bool have_range = false, have_delim = false, have_bpovr = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e;
        uint64_t v = 0;
        if (c >= 1 && c <= STARCH_MAP_ECHO_REF_SIZE + 1) e = cli::take_column(kCmd, &opt, c - 1, argv[optind - 1]);
        else switch (c) {
            case O_RANGE:
                e = cli::take_once(kCmd, &have_range, "--range");
                if (e == cli::GO_ON && !cli::parse_u64(optarg, &opt.range)) e = kCmd.bad("--range needs a number of bases", optarg);
                break;
            case O_DELIM: e = cli::take_delim(kCmd, opt.delim, &opt.delim_len, &have_delim, "--delim", "--delim needs 1 to 8 bytes"); break;
            case O_SKIP: e = cli::take_once(kCmd, &opt.skip_unmapped, "--skip-unmapped"); break;
            case O_BPOVR:
                e = cli::take_once(kCmd, &have_bpovr, "--bp-ovr");
                if (e == cli::GO_ON && (!cli::parse_u64(optarg, &v) || v != 1)) e = kCmd.bad("unsupported: --bp-ovr other than 1", optarg);
                break;
            default: e = cli::take_common(kCmd, c, argv, &device);
        }
        if (e != cli::GO_ON) return e;
    }
    cli::default_columns(&opt, STARCH_MAP_ECHO, STARCH_MAP_COUNT);
    return cli::run_two_inputs(kCmd, argc, argv, 1, "one reference and at most one map are needed", device, starch_map_host, &opt);
}
