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
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cli_common.hpp"

static const char* kName = "bedmap-elements";
static const char* kVersion = "0.1 (mi355x)";
static const int kUsageError = 2;

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
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
            "  number (ref is 0, map is 1) and line number (from 1); nothing is written.\n",
            kName, kVersion);
}

static int bad_usage(const char* why, const char* what)
{
    fprintf(stderr, "Error: %s%s%s\n", why, what ? ": " : "", what ? what : "");
    usage(stderr);
    return kUsageError;
}

static bool parse_u64(const char* s, uint64_t* v)
{
    if (!*s) return false;
    uint64_t x = 0;
    for (const char* p = s; *p; ++p) {
        if (*p < '0' || *p > '9') return false;
        const uint64_t d = (uint64_t)(*p - '0');
        if (x > (~0ull - d) / 10) return false;
        x = x * 10 + d;
    }
    *v = x;
    return true;
}

// digits [. digits] with a digit somewhere, at most 9 after the point and a value in (0, 1]
static bool parse_fraction(const char* s, uint64_t* num, uint32_t* digits)
{
    uint64_t whole = 0, frac = 0, den = 1;
    uint32_t nd = 0, any = 0;
    const char* p = s;
    for (; *p >= '0' && *p <= '9'; ++p, ++any)
        if ((whole = whole * 10 + (uint64_t)(*p - '0')) > 1) return false;
    if (*p == '.')
        for (++p; *p >= '0' && *p <= '9'; ++p, ++any) {
            if (++nd > 9) return false;
            frac = frac * 10 + (uint64_t)(*p - '0');
            den *= 10;
        }
    if (*p || !any) return false;
    const uint64_t v = whole * den + frac;
    if (v == 0 || v > den) return false;
    *num = v;
    *digits = nd;
    return true;
}

int main(int argc, char** argv)
{
    enum { O_CRIT = 64, O_DELIM = 256, O_MULTI, O_SKIP, O_DEVICE, O_HELP, O_VERSION };
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
                                    {"bp-ovr", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_BP_OVR},
                                    {"range", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_RANGE},
                                    {"fraction-ref", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_REF},
                                    {"fraction-map", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_MAP},
                                    {"fraction-both", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_BOTH},
                                    {"fraction-either", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_EITHER},
                                    {"exact", no_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_EXACT},
                                    {"delim", required_argument, nullptr, O_DELIM},
                                    {"multidelim", required_argument, nullptr, O_MULTI},
                                    {"skip-unmapped", no_argument, nullptr, O_SKIP},
                                    {"device", required_argument, nullptr, O_DEVICE},
                                    {"help", no_argument, nullptr, O_HELP},
                                    {"version", no_argument, nullptr, O_VERSION},
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
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        if (c >= 1 && c <= STARCH_MAPEL_ECHO_MAP_RANGE + 1) {
            for (uint32_t k = 0; k < opt.ncols; ++k)
                if (opt.cols[k] == c - 1) return bad_usage("an option is given twice", argv[optind - 1]);
            opt.cols[opt.ncols++] = (uint8_t)(c - 1);
            continue;
        }
        if (c >= O_CRIT && c <= O_CRIT + STARCH_MAPEL_CRIT_EXACT) {
            if (have_crit) return bad_usage("at most one overlap criterion may be given", argv[optind - 1]);
            have_crit = true;
            opt.criterion = (uint32_t)(c - O_CRIT);
            opt.n = 0;
            if (opt.criterion == STARCH_MAPEL_CRIT_BP_OVR) {
                if (!parse_u64(optarg, &opt.n) || opt.n == 0) return bad_usage("--bp-ovr needs a number of bases, 1 or more", optarg);
            } else if (opt.criterion == STARCH_MAPEL_CRIT_RANGE) {
                if (!parse_u64(optarg, &opt.range)) return bad_usage("--range needs a number of bases", optarg);
            } else if (opt.criterion != STARCH_MAPEL_CRIT_EXACT) {
                if (!parse_fraction(optarg, &opt.frac_num, &opt.frac_digits))
                    return bad_usage("a fraction is a decimal above 0 and up to 1 with at most 9 digits after the point", optarg);
            }
            continue;
        }
        switch (c) {
            case O_DELIM:
            case O_MULTI: {
                bool& have = c == O_DELIM ? have_delim : have_multi;
                if (have) return bad_usage("an option is given twice", c == O_DELIM ? "--delim" : "--multidelim");
                const size_t n = strlen(optarg);
                if (n < 1 || n > sizeof opt.delim) return bad_usage("a delimiter needs 1 to 8 bytes", optarg);
                memcpy(c == O_DELIM ? opt.delim : opt.multidelim, optarg, n);
                (c == O_DELIM ? opt.delim_len : opt.multidelim_len) = (uint32_t)n;
                have = true;
                break;
            }
            case O_SKIP:
                if (opt.skip_unmapped) return bad_usage("an option is given twice", "--skip-unmapped");
                opt.skip_unmapped = 1;
                break;
            case O_DEVICE: device = atoi(optarg); break;
            case O_HELP: usage(stdout); return 0;
            case O_VERSION: cli::print_version(kName, kVersion); return 0;
            default: return bad_usage("unsupported or unknown option", argv[optind - 1]);
        }
    }
    if (opt.ncols == 0) {
        opt.cols[0] = STARCH_MAPEL_ECHO;
        opt.cols[1] = STARCH_MAPEL_ECHO_MAP;
        opt.ncols = 2;
    }
    std::vector<std::string> paths;
    for (int i = optind; i < argc; ++i) paths.push_back(argv[i]);
    if (paths.empty() || paths.size() > 2) return bad_usage("one reference and at most one map are needed", nullptr);
    if (paths.size() == 2 && paths[0] == "-" && paths[1] == "-") return bad_usage("stdin (-) may be named once", nullptr);

    std::vector<std::vector<char>> data;
    if (const int e = cli::load_inputs(paths, &data)) return e;
    starch_setop_input in[2];
    for (size_t k = 0; k < paths.size(); ++k) in[k] = starch_setop_input{data[k].data(), (uint64_t)data[k].size()};

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    return cli::finish_output(ctx, starch_mapel_host(ctx, &in[0], paths.size() == 2 ? &in[1] : nullptr, &opt), "Error: %s (%s)\n");
}
