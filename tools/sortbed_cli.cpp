// tools/sortbed_cli.cpp -- the `sort-bed` command: BED files (or stdin) into
// the order starch3, unstarch and starchcat expect, sorted on the GPU
// (starch_sort_host), to stdout; --check-sort only tells whether the input is
// in that order already.
//
// One regular file is mapped read-only and handed to the library as it is;
// several inputs, or stdin, are read into one buffer, each file that does not
// end in '\n' getting one, and sorted as their concatenation.  Exit codes as
// unstarch (tools/unstarch_cli.cpp): ENODATA for a missing input, EINVAL for a
// malformed line, ENOMEM, EIO when stdout cannot be written; --check-sort
// exits 1 for an input that is not sorted.
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

static const char* kName = "sort-bed";
static const char* kVersion = "0.1 (mi355x)";

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
            "USAGE: sort-bed [--check-sort] [--device N] [file ... | -]\n\n"
            "  The BED lines of the files (no file, or -: stdin), sorted, go to stdout.  Several\n"
            "  files are sorted as their concatenation; a file whose last line lacks a newline\n"
            "  gets one.\n\n"
            "  Order: the chromosome name as bytes (chr1 < chr10 < chr2; a name before every\n"
            "  longer name it starts), then start, then stop as numbers.  Lines equal in all\n"
            "  three keep their input order, which is the order starchcat merges by; BEDOPS\n"
            "  sort-bed orders such lines by the rest of the line instead.\n\n"
            "  A line must be chrom TAB start TAB stop [TAB rest], with 1 to 19 digits in each\n"
            "  coordinate and a value of at most 2^63-1.  An empty line, a '#' or track header,\n"
            "  a CRLF line end in a three-column file: the first such line is reported with\n"
            "  its number and nothing is written.\n\n"
            "  --check-sort   exit 0 if the input is sorted; otherwise exit 1 and name the\n"
            "                 first line that sorts before its predecessor on stderr\n"
            "  --device N     GPU to sort on (default 0)\n"
            "  --help, --version\n",
            kName, kVersion);
}

int main(int argc, char** argv)
{
    int check = 0, device = 0;
    static struct option longs[] = {{"check-sort", no_argument, nullptr, 'c'},
                                    {"device", required_argument, nullptr, 'D'},
                                    {"help", no_argument, nullptr, 'h'},
                                    {"version", no_argument, nullptr, 'v'},
                                    {nullptr, 0, nullptr, 0}};
    opterr = 0;
    int c, li;
    while ((c = getopt_long(argc, argv, "hv", longs, &li)) != -1) {
        switch (c) {
            case 'c': check = 1; break;
            case 'D': device = atoi(optarg); break;
            case 'h': usage(stdout); return 0;
            case 'v': cli::print_version(kName, kVersion); return 0;
            default: usage(stderr); return EXIT_FAILURE;
        }
    }
    std::vector<std::string> inputs;
    for (int i = optind; i < argc; ++i) inputs.push_back(argv[i]);
    if (inputs.empty()) inputs.push_back("-");
    int dashes = 0;
    for (const std::string& p : inputs) dashes += p == "-";
    if (dashes > 1) {
        fprintf(stderr, "Error: stdin (-) may be named once\n");
        return EXIT_FAILURE;
    }
    struct stat st;
    if (dashes && fstat(STDIN_FILENO, &st) == 0 && S_ISCHR(st.st_mode)) {
        fprintf(stderr, "Error: No input is specified; please redirect or pipe in BED data, or name a file\n");
        usage(stderr);
        return ENODATA;
    }

    const void* bed = nullptr;
    uint64_t n = 0;
    void* map = MAP_FAILED;
    std::vector<std::vector<char>> data(1);   // the input read, when it is not mapped
    if (inputs.size() == 1 && inputs[0] != "-") {
        const int fd = open(inputs[0].c_str(), O_RDONLY);
        if (fd < 0 || fstat(fd, &st) != 0) {
            fprintf(stderr, "Error: Input file does not exist (%s)\n", inputs[0].c_str());
            return ENODATA;
        }
        if (S_ISREG(st.st_mode) && st.st_size > 0) {
            n = (uint64_t)st.st_size;
            map = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (map != MAP_FAILED) bed = map;
        }
        if (map == MAP_FAILED && !cli::read_all(fd, &data[0])) {   // not a regular file (or an empty one): read it
            fprintf(stderr, "Error: reading %s failed (%s)\n", inputs[0].c_str(), strerror(errno));
            return EIO;
        }
        close(fd);
    } else if (const int e = cli::load_inputs(inputs, &data, true)) {
        return e;
    }
    if (map == MAP_FAILED) {
        bed = data[0].data();
        n = data[0].size();
    }

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    if (check) {
        uint64_t line = 0;
        const int rc = starch_sort_check_host(ctx, bed, n, &line);
        if (rc != STARCH_OK) {
            fprintf(stderr, "Error: %s (%s)\n", starch_last_error(ctx), starch_strerror(rc));
            starch_destroy(ctx);
            return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
        }
        if (line) fprintf(stderr, "sort-bed: not sorted: line %llu sorts before line %llu\n", (unsigned long long)line,
                          (unsigned long long)(line - 1));
        starch_destroy(ctx);
        return line ? 1 : 0;
    }
    return cli::finish_output(ctx, starch_sort_host(ctx, bed, n), "Error: %s (%s)\n");
}
