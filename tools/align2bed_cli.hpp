// tools/align2bed_cli.hpp -- what the `sam2bed`, `psl2bed` and `rmsk2bed` commands
// share: text (a file or stdin) converted to BED on the GPU (starch_align_host),
// by default in sort-bed's order, to stdout; --output=starch writes the archive
// starch3 writes for that sorted BED (starch_align_encode_host).  A command
// names its format, the format options it takes and its help.
//
// Exit codes as convert2bed (tools/convert2bed_cli.cpp): 2 for a bad command line
// or an option the command does not have (answered before a GPU is opened),
// ENODATA for a missing input, EINVAL for a line that does not fit its format
// (the library's text names the line), ENOMEM, EIO.
#pragma once
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <string>
#include <vector>

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

static void usage(const Command& cmd, FILE* f) { fprintf(f, "%s\n  version: %s\n\n%s", cmd.name, kVersion, cmd.help); }

static int bad_usage(const Command& cmd, const char* why, const char* what)
{
    fprintf(stderr, "Error: %s%s%s\n", why, what ? ": " : "", what ? what : "");
    usage(cmd, stderr);
    return kUsageError;
}

static int run(const Command& cmd, int argc, char** argv)
{
    enum { O_OUTPUT = 256, O_NOSORT, O_KEEP, O_SPLIT, O_SPLITDEL, O_ALL, O_REDUCED, O_DEVICE, O_HELP, O_VERSION };
    static struct option longs[] = {{"output", required_argument, nullptr, O_OUTPUT},
                                    {"do-not-sort", no_argument, nullptr, O_NOSORT},
                                    {"keep-header", no_argument, nullptr, O_KEEP},
                                    {"split", no_argument, nullptr, O_SPLIT},
                                    {"split-with-deletions", no_argument, nullptr, O_SPLITDEL},
                                    {"all-reads", no_argument, nullptr, O_ALL},
                                    {"reduced", no_argument, nullptr, O_REDUCED},
                                    {"device", required_argument, nullptr, O_DEVICE},
                                    {"help", no_argument, nullptr, O_HELP},
                                    {"version", no_argument, nullptr, O_VERSION},
                                    {nullptr, 0, nullptr, 0}};
    starch_align_options opt;
    memset(&opt, 0, sizeof opt);
    opt.format = cmd.format;
    int device = 0;
    bool starch = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        const unsigned needs = c == O_SPLIT ? TAKES_SPLIT : (c == O_SPLITDEL || c == O_ALL || c == O_REDUCED ? TAKES_SAM : 0u);
        if (needs && !(cmd.takes & needs)) return bad_usage(cmd, "unsupported or unknown option", argv[optind - 1]);
        switch (c) {
            case O_OUTPUT:
                if (!strcasecmp(optarg, "starch")) starch = true;
                else if (!strcasecmp(optarg, "bed")) starch = false;
                else return bad_usage(cmd, "unsupported or unknown output format", optarg);
                break;
            case O_NOSORT: opt.no_sort = 1; break;
            case O_KEEP: opt.keep_header = 1; break;
            case O_SPLIT: opt.split = 1; break;
            case O_SPLITDEL: opt.split = opt.split_deletions = 1; break;
            case O_ALL: opt.all_reads = 1; break;
            case O_REDUCED: opt.reduced = 1; break;
            case O_DEVICE: device = atoi(optarg); break;
            case O_HELP: usage(cmd, stdout); return 0;
            case O_VERSION: cli::print_version(cmd.name, kVersion); return 0;
            default: return bad_usage(cmd, "unsupported or unknown option", argv[optind - 1]);
        }
    }
    if (starch && opt.no_sort) return bad_usage(cmd, "--output=starch needs the sort", "--do-not-sort");
    std::vector<std::string> paths;
    for (int i = optind; i < argc; ++i) paths.push_back(argv[i]);
    if (paths.size() > 1) return bad_usage(cmd, "one input file at most", paths[1].c_str());
    if (paths.empty()) paths.push_back("-");

    std::vector<std::vector<char>> data;
    if (const int e = cli::load_inputs(paths, &data)) return e;

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    if (!starch)
        return cli::finish_output(ctx, starch_align_host(ctx, data[0].data(), data[0].size(), &opt), "Error: %s (%s)\n");

    int rc = starch_align_encode_host(ctx, data[0].data(), data[0].size(), &opt, nullptr);
    uint64_t bytes = 0;
    std::vector<char> out;
    if (rc == STARCH_OK) rc = starch_archive_size(ctx, &bytes);
    if (rc == STARCH_OK) {
        out.resize(bytes);
        rc = starch_archive_copy(ctx, out.data(), bytes);
    }
    if (rc != STARCH_OK) {
        fprintf(stderr, "Error: %s (%s)\n", starch_last_error(ctx), starch_strerror(rc));
        starch_destroy(ctx);
        return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
    }
    for (uint64_t w = 0; w < bytes;) {
        const size_t k = fwrite(out.data() + w, 1, bytes - w, stdout);
        if (k == 0) break;
        w += k;
    }
    const bool ok = cli::stdout_ok("archive");
    starch_destroy(ctx);
    return ok ? 0 : EIO;
}

}  // namespace align_cli
