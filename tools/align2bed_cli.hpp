// tools/align2bed_cli.hpp -- what the `sam2bed`, `psl2bed`, `rmsk2bed` and `bam2bed`
// commands share: an input (a file or stdin) converted to BED on the GPU
// (starch_align_host, starch_bam_host), by default in sort-bed's order, to
// stdout; --output=starch writes the archive starch3 writes for that sorted BED
// (starch_align_encode_host, starch_bam_encode_host).  A command names its
// format, the format options it takes and its help.
//
// Exit codes as convert2bed (tools/convert2bed_cli.cpp): 2 for a bad command line
// or an option the command does not have (answered before a GPU is opened),
// ENODATA for a missing input, EINVAL for a line that does not fit its format
// (the library's text names the line), ENOMEM, EIO.
#pragma once
#include "cli_common.hpp"

namespace align_cli {

enum : unsigned { TAKES_SPLIT = 1, TAKES_SAM = 2 };   // --split; --split-with-deletions, --all-reads, --reduced

struct Command {
    const char* name;
    uint32_t format;        // STARCH_ALIGN_*
    unsigned takes;
    const char* help;       // after the version lines; holds the USAGE line
};

static const char* kVersion = "0.1 (mi355x)";
static const int kUsageError = 2;

// opt: the command's options (starch_align_options with its format set, or
// starch_bam_options); host and encode: the library calls that take them
template <class Options, class Host, class Encode>
static int run_with(const Command& which, Options& opt, Host host, Encode encode, int argc, char** argv)
{
    enum { O_OUTPUT = 256, O_NOSORT, O_KEEP, O_SPLIT, O_SPLITDEL, O_ALL, O_REDUCED };
    static struct option longs[] = {{"output", required_argument, nullptr, O_OUTPUT},
                                    {"do-not-sort", no_argument, nullptr, O_NOSORT},
                                    {"keep-header", no_argument, nullptr, O_KEEP},
                                    {"split", no_argument, nullptr, O_SPLIT},
                                    {"split-with-deletions", no_argument, nullptr, O_SPLITDEL},
                                    {"all-reads", no_argument, nullptr, O_ALL},
                                    {"reduced", no_argument, nullptr, O_REDUCED},
                                    CLI_COMMON_OPTIONS,
                                    {nullptr, 0, nullptr, 0}};
    const cli::Command cmd = {which.name, kVersion, which.help, kUsageError};
    int device = 0;
    bool starch = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        const unsigned needs = c == O_SPLIT ? TAKES_SPLIT : (c == O_SPLITDEL || c == O_ALL || c == O_REDUCED ? TAKES_SAM : 0u);
        int e = cli::GO_ON;
        if (needs && !(which.takes & needs)) c = '?';   // an option of another of the three commands
        switch (c) {
            case O_OUTPUT: e = cli::take_output_format(cmd, &starch); break;
            case O_NOSORT: opt.no_sort = 1; break;
            case O_KEEP: opt.keep_header = 1; break;
            case O_SPLIT: opt.split = 1; break;
            case O_SPLITDEL: opt.split = opt.split_deletions = 1; break;
            case O_ALL: opt.all_reads = 1; break;
            case O_REDUCED: opt.reduced = 1; break;
            default: e = cli::take_common(cmd, c, argv, &device);
        }
        if (e != cli::GO_ON) return e;
    }
    return cli::run_converter(cmd, argc, argv, device, starch, host, encode, &opt);
}

static int run(const Command& which, int argc, char** argv)
{
    starch_align_options opt;
    memset(&opt, 0, sizeof opt);
    opt.format = which.format;
    return run_with(which, opt, starch_align_host, starch_align_encode_host, argc, argv);
}

}  // namespace align_cli
