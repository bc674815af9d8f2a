// tools/bedmap_cli.cpp -- the `bedmap` command: for every line of a sorted
// reference, the map lines that overlap it counted and measured on the GPU
// (starch_map_host).  Inputs are sorted BED files, .starch archives (recognised
// by their magic) or stdin; the annotated reference lines go to stdout.
//
// Exit codes: 2 for a bad command line or an option this bedmap does not have
// (answered before a GPU is opened), otherwise as bedops (tools/bedops_cli.cpp):
// ENODATA for a missing input, EINVAL for a data error (the library's text
// names the input and the line), ENOMEM, EIO.
#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "cli_common.hpp"

static const char* kName = "bedmap";
static const char* kVersion = "0.1 (mi355x)";
static const int kUsageError = 2;

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
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
            "  is written.\n",
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

int main(int argc, char** argv)
{
    enum { O_RANGE = 256, O_DELIM, O_SKIP, O_BPOVR, O_DEVICE, O_HELP, O_VERSION };
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
                                    {"device", required_argument, nullptr, O_DEVICE},
                                    {"help", no_argument, nullptr, O_HELP},
                                    {"version", no_argument, nullptr, O_VERSION},
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
        if (c >= 1 && c <= STARCH_MAP_ECHO_REF_SIZE + 1) {
            for (uint32_t k = 0; k < opt.ncols; ++k)
                if (opt.cols[k] == c - 1) return bad_usage("an option is given twice", argv[optind - 1]);
            opt.cols[opt.ncols++] = (uint8_t)(c - 1);
            continue;
        }
        switch (c) {
            case O_RANGE:
                if (have_range) return bad_usage("an option is given twice", "--range");
                if (!parse_u64(optarg, &opt.range)) return bad_usage("--range needs a number of bases", optarg);
                have_range = true;
                break;
            case O_DELIM: {
                if (have_delim) return bad_usage("an option is given twice", "--delim");
                const size_t n = strlen(optarg);
                if (n < 1 || n > sizeof opt.delim) return bad_usage("--delim needs 1 to 8 bytes", optarg);
                memcpy(opt.delim, optarg, n);
                opt.delim_len = (uint32_t)n;
                have_delim = true;
                break;
            }
            case O_SKIP:
                if (opt.skip_unmapped) return bad_usage("an option is given twice", "--skip-unmapped");
                opt.skip_unmapped = 1;
                break;
            case O_BPOVR: {
                uint64_t v = 0;
                if (have_bpovr) return bad_usage("an option is given twice", "--bp-ovr");
                if (!parse_u64(optarg, &v) || v != 1) return bad_usage("unsupported: --bp-ovr other than 1", optarg);
                have_bpovr = true;
                break;
            }
            case O_DEVICE: device = atoi(optarg); break;
            case O_HELP: usage(stdout); return 0;
            case O_VERSION: cli::print_version(kName, kVersion); return 0;
            default: return bad_usage("unsupported or unknown option", argv[optind - 1]);
        }
    }
    if (opt.ncols == 0) {
        opt.cols[0] = STARCH_MAP_ECHO;
        opt.cols[1] = STARCH_MAP_COUNT;
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
    return cli::finish_output(ctx, starch_map_host(ctx, &in[0], paths.size() == 2 ? &in[1] : nullptr, &opt), "Error: %s (%s)\n");
}
