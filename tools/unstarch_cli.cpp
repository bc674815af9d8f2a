// tools/unstarch_cli.cpp -- the `unstarch` command: a Starch archive of this
// library back to BED on stdout, whole or by chromosome / region through the
// archive's index (starch_extract_host), and the index listings (BEDOPS
// unstarch's --list, --list-chromosomes, --elements, --bases, --bases-uniq),
// which read the index alone and open no GPU context.
//
// The archive is mapped read-only: only the footer, the index and the chosen
// streams' pages are touched.  Exit codes as starch3 (tools/starch3_cli.cpp):
// ENODATA for a missing input, EINVAL for a bad archive or query, ENOMEM, EIO
// when stdout cannot be written; 2 when --bases is asked of an archive
// without base counts.
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

static const char* kName = "unstarch";
static const char* kVersion = "0.1 (mi355x)";

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
            "USAGE: unstarch [options] [chrom ...] <archive.starch>\n\n"
            "  With no option the archive's BED lines go to stdout: all of them, or those of\n"
            "  the named chromosomes (exact names), in archive order.\n\n"
            "  --region chr:start-stop   lines overlapping [start, stop) (repeatable)\n"
            "  --regions FILE            the same for every BED3 line of FILE (- : stdin)\n"
            "  --list                    one row per stream: chromosome, offset, size, lines,\n"
            "                            transformed bytes, blocks, CRC (tab-separated)\n"
            "  --list-chromosomes        the distinct chromosome names, in archive order\n"
            "  --elements                number of BED lines (of the named chromosomes)\n"
            "  --bases, --bases-uniq     base counts from the index (archives written with\n"
            "                            starch3 --base-counts)\n"
            "  --device N                GPU to decode on (default 0)\n"
            "  --help, --version\n",
            kName, kVersion);
}

struct Query {
    std::string chr;
    int64_t start = 0, stop = 0;
    bool whole = true;
};

static bool parse_i64(const char* b, const char* e, int64_t* v)
{
    if (b == e) return false;
    std::string s(b, e);
    char* end = nullptr;
    errno = 0;
    const long long x = strtoll(s.c_str(), &end, 10);
    if (errno || *end) return false;
    *v = x;
    return true;
}

// chr:start-stop; the name may itself hold ':' (the last one splits)
static bool parse_region(const char* s, Query* q)
{
    const char* colon = strrchr(s, ':');
    if (!colon || colon == s) return false;
    const char* dash = strchr(colon[1] == '-' ? colon + 2 : colon + 1, '-');   // start may be negative
    if (!dash) return false;
    q->chr.assign(s, colon);
    q->whole = false;
    return parse_i64(colon + 1, dash, &q->start) && parse_i64(dash + 1, s + strlen(s), &q->stop);
}

static bool read_regions(const char* path, std::vector<Query>* out)
{
    FILE* f = strcmp(path, "-") ? fopen(path, "rb") : stdin;
    if (!f) return false;
    std::string line;
    bool ok = true;
    int ch;
    auto flush = [&]() {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) return;
        const size_t t1 = line.find('\t');
        const size_t t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == std::string::npos) { ok = false; return; }
        size_t t3 = line.find('\t', t2 + 1);
        if (t3 == std::string::npos) t3 = line.size();
        Query q;
        q.chr = line.substr(0, t1);
        q.whole = false;
        if (!parse_i64(line.data() + t1 + 1, line.data() + t2, &q.start) ||
            !parse_i64(line.data() + t2 + 1, line.data() + t3, &q.stop))
            ok = false;
        out->push_back(q);
    };
    while ((ch = fgetc(f)) != EOF) {
        if (ch == '\n') { flush(); line.clear(); }
        else line += (char)ch;
    }
    flush();
    if (f != stdin) fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    enum { M_EXTRACT, M_LIST, M_CHROMS, M_ELEMENTS, M_BASES, M_BASES_UNIQ };
    int mode = M_EXTRACT, device = 0;
    std::vector<Query> queries;
    static struct option longs[] = {
        {"region", required_argument, nullptr, 'r'},  {"regions", required_argument, nullptr, 'R'},
        {"list", no_argument, nullptr, 'l'},          {"list-chromosomes", no_argument, nullptr, 'c'},
        {"elements", no_argument, nullptr, 'e'},      {"bases", no_argument, nullptr, 'b'},
        {"bases-uniq", no_argument, nullptr, 'u'},    {"device", required_argument, nullptr, 'D'},
        {"help", no_argument, nullptr, 'h'},          {"version", no_argument, nullptr, 'v'},
        {nullptr, 0, nullptr, 0}};
    opterr = 0;
    int c, li;
    while ((c = getopt_long(argc, argv, "hv", longs, &li)) != -1) {
        switch (c) {
            case 'r': {
                Query q;
                if (!parse_region(optarg, &q)) {
                    fprintf(stderr, "Error: --region wants chr:start-stop (%s)\n", optarg);
                    return EINVAL;
                }
                queries.push_back(q);
                break;
            }
            case 'R':
                if (!read_regions(optarg, &queries)) {
                    fprintf(stderr, "Error: --regions wants a file of BED3 lines (%s)\n", optarg);
                    return EINVAL;
                }
                break;
            case 'l': mode = M_LIST; break;
            case 'c': mode = M_CHROMS; break;
            case 'e': mode = M_ELEMENTS; break;
            case 'b': mode = M_BASES; break;
            case 'u': mode = M_BASES_UNIQ; break;
            case 'D': device = atoi(optarg); break;
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
    const char* path = argv[argc - 1];
    for (int i = optind; i < argc - 1; ++i) {
        Query q;
        q.chr = argv[i];
        queries.push_back(q);
    }
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) {
        fprintf(stderr, "Error: Input file does not exist (%s)\n", path);
        return ENODATA;
    }
    const uint64_t n = (uint64_t)sb.st_size;
    void* map = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
    close(fd);
    if (map == MAP_FAILED) {
        fprintf(stderr, "Error: the archive could not be mapped (%s)\n", n ? strerror(errno) : "empty file");
        return EINVAL;
    }

    if (mode != M_EXTRACT) {   // the index alone
        uint64_t count = 0, names_len = 0;
        int method = 0, bs = 0;
        int rc = starch_archive_index(map, n, nullptr, 0, &count, nullptr, 0, &names_len, &method, &bs);
        std::vector<starch_index_entry> en(count ? count : 1);
        std::vector<char> names(names_len ? names_len : 1);
        if (rc == STARCH_OK)
            rc = starch_archive_index(map, n, en.data(), count, &count, names.data(), names_len, &names_len, &method, &bs);
        if (rc != STARCH_OK) {
            fprintf(stderr, "Error: reading the archive's index failed (%s)\n", starch_strerror(rc));
            return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
        }
        auto name_of = [&](uint64_t k) { return std::string(names.data() + en[k].name_off, en[k].name_len); };
        auto wanted = [&](uint64_t k) {
            if (queries.empty()) return true;
            const std::string nm = name_of(k);
            for (const Query& q : queries)
                if (q.chr == nm) return true;
            return false;
        };
        if (mode == M_LIST) {
            for (uint64_t k = 0; k < count; ++k) {
                if (!wanted(k)) continue;
                fwrite(names.data() + en[k].name_off, 1, en[k].name_len, stdout);
                printf("\t%llu\t%llu\t%llu\t%llu\t%u\t%08x\n", (unsigned long long)en[k].offset,
                       (unsigned long long)en[k].size, (unsigned long long)en[k].line_count,
                       (unsigned long long)en[k].text_bytes, en[k].n_blocks, en[k].combined_crc);
            }
        } else if (mode == M_CHROMS) {
            std::vector<std::string> seen;
            for (uint64_t k = 0; k < count; ++k) {
                const std::string nm = name_of(k);
                bool dup = false;
                for (const std::string& s : seen) dup = dup || s == nm;
                if (dup) continue;
                seen.push_back(nm);
                fwrite(nm.data(), 1, nm.size(), stdout);
                fputc('\n', stdout);
            }
        } else if (mode == M_ELEMENTS) {
            unsigned long long sum = 0;
            for (uint64_t k = 0; k < count; ++k)
                if (wanted(k)) sum += en[k].line_count;
            printf("%llu\n", sum);
        } else {
            long long sum = 0;
            for (uint64_t k = 0; k < count; ++k) {
                if (!wanted(k)) continue;
                if (!en[k].has_base_counts) {
                    fprintf(stderr, "Error: the archive's index holds no base counts (write it with starch3 --base-counts)\n");
                    return 2;
                }
                sum += mode == M_BASES ? en[k].base_count_nonunique : en[k].base_count_unique;
            }
            printf("%lld\n", sum);
        }
        return cli::stdout_ok("output") ? 0 : EIO;
    }

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    std::vector<starch_region> regions;
    for (const Query& q : queries)
        regions.push_back(starch_region{q.chr.data(), q.chr.size(), q.start, q.stop, q.whole ? 1 : 0});
    return cli::finish_output(ctx, starch_extract_host(ctx, map, n, regions.data(), regions.size()),
                              "Error: extraction failed (%2$s: %1$s)\n");
}
