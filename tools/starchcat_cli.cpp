// tools/starchcat_cli.cpp -- the `starchcat` command: several Starch archives
// of this library merged into one on stdout (starch_cat_host).  A chromosome
// held by one input at the requested bzip2 level is copied byte for byte; the
// others are decoded, merged by (start, stop) and encoded again on the GPU.
// --plan prints what would happen and opens no GPU; the GPU context is created
// only when the plan holds a chromosome that has to be merged.
//
// The inputs are mapped read-only: only their footers, indexes and the
// streams that are copied or decoded are touched.  Exit codes as starch3
// (tools/starch3_cli.cpp): ENODATA for a missing input, EINVAL for a bad
// archive or option, ENOMEM, EIO when stdout cannot be written.
#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "cli_common.hpp"

static const char* kName = "starchcat";
static const char* kVersion = "0.1 (mi355x)";

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
            "USAGE: starchcat [options] a.starch b.starch ... > out.starch\n\n"
            "  Merges the archives into one: one stream per chromosome, the chromosomes in\n"
            "  sort-bed (bytewise) order, each chromosome's lines ordered by start, then stop.\n"
            "  Every input must be sorted (sort-bed) within each of its streams.\n\n"
            "  --note TEXT           free text for the index\n"
            "  --level N             bzip2 block size 1..9 (default 9; also --bzip2-level)\n"
            "  --base-counts         per-chromosome base counts in the index\n"
            "                        (also --report-base-counts)\n"
            "  --plan                print chromosome, action (copy | merge) and the runs\n"
            "                        (input:stream, ...) tab-separated; no GPU, no archive\n"
            "  --device N            GPU to merge on (default 0)\n"
            "  --stats               counts of the run on stderr\n"
            "  --help, --version\n",
            kName, kVersion);
}

int main(int argc, char** argv)
{
    const char* note = nullptr;
    int level = 9, bases = 0, plan_only = 0, device = 0, stats = 0;
    static struct option longs[] = {
        {"note", required_argument, nullptr, 'n'},        {"level", required_argument, nullptr, 'L'},
        {"bzip2-level", required_argument, nullptr, 'L'}, {"base-counts", no_argument, nullptr, 'B'},
        {"report-base-counts", no_argument, nullptr, 'B'}, {"plan", no_argument, nullptr, 'p'},
        {"device", required_argument, nullptr, 'D'},      {"stats", no_argument, nullptr, 'S'},
        {"help", no_argument, nullptr, 'h'},              {"version", no_argument, nullptr, 'v'},
        {nullptr, 0, nullptr, 0}};
    opterr = 0;
    int c, li;
    while ((c = getopt_long(argc, argv, "n:hv", longs, &li)) != -1) {
        switch (c) {
            case 'n': note = optarg; break;
            case 'L': level = atoi(optarg); break;
            case 'B': bases = 1; break;
            case 'p': plan_only = 1; break;
            case 'D': device = atoi(optarg); break;
            case 'S': stats = 1; break;
            case 'h': usage(stdout); return 0;
            case 'v': cli::print_version(kName, kVersion); return 0;
            default: usage(stderr); return EXIT_FAILURE;
        }
    }
    if (optind >= argc) {
        fprintf(stderr, "Error: No archive is specified\n");
        usage(stderr);
        return ENODATA;
    }
    if (level < 1 || level > 9) {
        fprintf(stderr, "Error: --level must be 1..9\n");
        return EINVAL;
    }
    if (!plan_only && isatty(STDOUT_FILENO)) {
        fprintf(stderr, "Error: the archive is binary; redirect stdout to a file or a pipe\n");
        return EINVAL;
    }
    std::vector<const void*> maps;
    std::vector<uint64_t> lens;
    for (int i = optind; i < argc; ++i) {
        const int fd = open(argv[i], O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0) {
            fprintf(stderr, "Error: Input file does not exist (%s)\n", argv[i]);
            return ENODATA;
        }
        const uint64_t n = (uint64_t)sb.st_size;
        void* map = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
        close(fd);
        if (map == MAP_FAILED) {
            fprintf(stderr, "Error: the archive could not be mapped (%s: %s)\n", argv[i], n ? strerror(errno) : "empty file");
            return EINVAL;
        }
        maps.push_back(map);
        lens.push_back(n);
    }
    starch_options opt;
    starch_options_init(&opt);
    opt.block_size_100k = level;
    opt.note = note;
    opt.base_counts = bases;

    uint64_t ng = 0, nr = 0, nb = 0;
    int rc = starch_cat_plan(maps.data(), lens.data(), maps.size(), &opt, nullptr, 0, &ng, nullptr, 0, &nr, nullptr, 0, &nb);
    std::vector<starch_cat_group> groups(ng ? ng : 1);
    std::vector<starch_cat_run> runs(nr ? nr : 1);
    std::vector<char> names(nb ? nb : 1);
    if (rc == STARCH_OK)
        rc = starch_cat_plan(maps.data(), lens.data(), maps.size(), &opt, groups.data(), ng, &ng, runs.data(), nr, &nr,
                             names.data(), nb, &nb);
    if (rc != STARCH_OK) {
        fprintf(stderr, "Error: reading the archives' indexes failed (%s)\n", starch_strerror(rc));
        return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
    }
    bool any_merge = false;
    for (uint64_t g = 0; g < ng; ++g) any_merge = any_merge || groups[g].merge;
    if (plan_only) {
        for (uint64_t g = 0; g < ng; ++g) {
            fwrite(names.data() + groups[g].name_off, 1, groups[g].name_len, stdout);
            fputs(groups[g].merge ? "\tmerge\t" : "\tcopy\t", stdout);
            for (uint32_t k = 0; k < groups[g].n_runs; ++k) {
                const starch_cat_run r = runs[groups[g].first_run + k];
                printf("%s%u:%u", k ? "," : "", r.input, r.entry);
            }
            fputc('\n', stdout);
        }
        return cli::stdout_ok("archive") ? 0 : EIO;
    }

    starch_ctx* ctx = nullptr;
    if (any_merge)
        if (const int e = cli::open_ctx(device, &ctx)) return e;
    void* out = nullptr;
    uint64_t bytes = 0;
    rc = starch_cat_host(ctx, maps.data(), lens.data(), maps.size(), &opt, &out, &bytes);
    if (rc != STARCH_OK) {
        fprintf(stderr, "Error: starchcat failed (%s: %s)\n", starch_strerror(rc), ctx ? starch_last_error(ctx) : "");
        if (ctx) starch_destroy(ctx);
        return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
    }
    if (bytes) fwrite(out, 1, bytes, stdout);
    starch_free(out);
    const bool ok = cli::stdout_ok("archive");
    if (ok && stats) {
        starch_cat_stats s;
        if (ctx && starch_cat_get_stats(ctx, &s) == STARCH_OK)
            fprintf(stderr,
                    "{\"streams_in\": %llu, \"streams_copied\": %llu, \"groups_merged\": %llu, \"runs_decoded\": %llu, "
                    "\"lines_merged\": %llu, \"bytes_copied\": %llu, \"bytes_decoded\": %llu, \"archive_bytes\": %llu}\n",
                    (unsigned long long)s.streams_in, (unsigned long long)s.streams_copied,
                    (unsigned long long)s.groups_merged, (unsigned long long)s.runs_decoded,
                    (unsigned long long)s.lines_merged, (unsigned long long)s.bytes_copied,
                    (unsigned long long)s.bytes_decoded, (unsigned long long)bytes);
        else
            fprintf(stderr, "{\"streams_copied\": %llu, \"groups_merged\": 0, \"archive_bytes\": %llu}\n",
                    (unsigned long long)ng, (unsigned long long)bytes);
    }
    if (ctx) starch_destroy(ctx);
    return ok ? 0 : EIO;
}
