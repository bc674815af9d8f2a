// tools/bbi2bed_cli.hpp -- what the `bigwig2bed` and `bigbed2bed` commands share:
// a bigWig / bigBed file, memory-mapped, converted to BED on the GPU
// (starch_bbi_host), by default in sort-bed's order, to stdout; --output=starch
// writes the archive starch3 writes for that sorted BED (starch_bbi_encode_host).
// Only the blocks that --region needs are uploaded.
//
// Exit codes as the other converters (tools/align2bed_cli.hpp): 2 for a bad
// command line, for stdin (the format needs seeks) and for a file of the other
// kind, which the magic shows before a GPU is opened; ENODATA for a missing
// input, EINVAL for a file or block that does not fit its format, ENOMEM, EIO.
#pragma once
#include <sys/mman.h>
#include <sys/stat.h>

#include "cli_common.hpp"

namespace bbi_cli {

struct Command {
    const char* name;
    uint32_t kind;          // STARCH_BBI_BIGWIG or STARCH_BBI_BIGBED
    uint32_t magic, other_magic;
    const char* help;       // after the version lines; holds the USAGE line
};

static const char* kVersion = "0.1 (mi355x)";
static const int kUsageError = 2;

// chr, or chr:a-b with a < b
static bool parse_region(const char* s, std::string* chrom, starch_bbi_query* q)
{
    const char* colon = strrchr(s, ':');
    if (!colon) {
        *chrom = s;
        q->region = 1;
        return !chrom->empty();
    }
    const char* dash = strchr(colon + 1, '-');
    if (!dash) return false;
    const std::string a(colon + 1, dash), b(dash + 1);
    chrom->assign(s, colon);
    q->region = 2;
    return !chrom->empty() && cli::parse_u64(a.c_str(), &q->start) && cli::parse_u64(b.c_str(), &q->end) && q->start < q->end;
}

static int run(const Command& which, int argc, char** argv)
{
    enum { O_OUTPUT = 256, O_NOSORT, O_REGION };
    static struct option longs[] = {{"output", required_argument, nullptr, O_OUTPUT},
                                    {"do-not-sort", no_argument, nullptr, O_NOSORT},
                                    {"region", required_argument, nullptr, O_REGION},
                                    CLI_COMMON_OPTIONS,
                                    {nullptr, 0, nullptr, 0}};
    const cli::Command cmd = {which.name, kVersion, which.help, kUsageError};
    int device = 0;
    bool starch = false, no_sort = false;
    starch_bbi_query q;
    memset(&q, 0, sizeof q);
    q.kind = which.kind;
    std::string chrom;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e = cli::GO_ON;
        switch (c) {
            case O_OUTPUT: e = cli::take_output_format(cmd, &starch); break;
            case O_NOSORT: no_sort = true; break;
            case O_REGION:
                if (!parse_region(optarg, &chrom, &q)) e = cmd.bad("a region is chr or chr:start-end with start below end", optarg);
                break;
            default: e = cli::take_common(cmd, c, argv, &device);
        }
        if (e != cli::GO_ON) return e;
    }
    if (starch && no_sort) return cmd.bad("--output=starch needs the sort", "--do-not-sort");
    if (optind + 1 != argc) return cmd.bad("one input file", nullptr);
    const char* path = argv[optind];
    if (!strcmp(path, "-")) return cmd.bad("stdin is not supported: the format needs seeks", nullptr);
    q.chrom = chrom.c_str();
    q.chrom_len = chrom.size();
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "Error: Input file does not exist (%s)\n", path);
        return ENODATA;
    }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        close(fd);
        return cmd.bad("the input must be a regular file: the format needs seeks", path);
    }
    const uint64_t n = (uint64_t)sb.st_size;
    void* map = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (n && map == MAP_FAILED) {
        fprintf(stderr, "Error: mapping %s failed (%s)\n", path, strerror(errno));
        return EIO;
    }
    uint32_t magic = 0;
    if (n >= 4) memcpy(&magic, map, 4);
    if (magic == which.other_magic) {        // decided before a GPU is opened
        if (map) munmap(map, n);
        return cmd.bad(which.kind == STARCH_BBI_BIGWIG ? "the file is a bigBed file: use bigbed2bed" : "the file is a bigWig file: use bigwig2bed",
                       path);
    }
    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    const int rc = starch ? starch_bbi_encode_host(ctx, map, n, &q, nullptr) : starch_bbi_host(ctx, map, n, &q, no_sort ? 1 : 0);
    const int code = cli::finish_output(ctx, rc, "Error: %s (%s)\n", starch);
    if (map) munmap(map, n);
    return code;
}

}  // namespace bbi_cli
