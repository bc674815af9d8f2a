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
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cli_common.hpp"

static const char* kName = "bedmap-scores";
static const char* kVersion = "0.1 (mi355x)";
static const int kUsageError = 2;

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
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
    enum { O_CRIT = 64, O_DELIM = 256, O_PREC, O_SKIP, O_DEVICE, O_HELP, O_VERSION, O_REFUSED };
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
                                    {"bp-ovr", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_BP_OVR},
                                    {"range", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_RANGE},
                                    {"fraction-ref", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_REF},
                                    {"fraction-map", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_MAP},
                                    {"fraction-both", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_BOTH},
                                    {"fraction-either", required_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_FRACTION_EITHER},
                                    {"exact", no_argument, nullptr, O_CRIT + STARCH_MAPEL_CRIT_EXACT},
                                    {"prec", required_argument, nullptr, O_PREC},
                                    {"delim", required_argument, nullptr, O_DELIM},
                                    {"skip-unmapped", no_argument, nullptr, O_SKIP},
                                    {"device", required_argument, nullptr, O_DEVICE},
                                    {"help", no_argument, nullptr, O_HELP},
                                    {"version", no_argument, nullptr, O_VERSION},
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
        if (c >= 1 && c <= STARCH_MAPSC_MAX_ELEMENT + 1) {
            for (uint32_t k = 0; k < opt.ncols; ++k)
                if (opt.cols[k] == c - 1) return bad_usage("an option is given twice", (std::string("--") + longs[c - 1].name).c_str());
            if (c - 1 == STARCH_MAPSC_KTH && !parse_fraction(optarg, &opt.kth_num, &opt.kth_digits))
                return bad_usage("--kth needs a decimal above 0 and up to 1 with at most 9 digits after the point", optarg);
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
            case O_DELIM: {
                if (have_delim) return bad_usage("an option is given twice", "--delim");
                const size_t n = strlen(optarg);
                if (n < 1 || n > sizeof opt.delim) return bad_usage("a delimiter needs 1 to 8 bytes", optarg);
                memcpy(opt.delim, optarg, n);
                opt.delim_len = (uint32_t)n;
                have_delim = true;
                break;
            }
            case O_PREC: {
                if (have_prec) return bad_usage("an option is given twice", "--prec");
                uint64_t p = 0;
                if (!parse_u64(optarg, &p) || p > 9) return bad_usage("--prec needs a number of digits, 0 to 9", optarg);
                opt.prec = (uint32_t)p;
                have_prec = true;
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
        opt.cols[0] = STARCH_MAPSC_ECHO;
        opt.cols[1] = STARCH_MAPSC_MEAN;
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
    return cli::finish_output(ctx, starch_mapsc_host(ctx, &in[0], paths.size() == 2 ? &in[1] : nullptr, &opt), "Error: %s (%s)\n");
}
