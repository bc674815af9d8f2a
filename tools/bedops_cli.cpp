// tools/bedops_cli.cpp -- the `bedops` command: --merge, --intersect,
// --difference, --symmdiff or --complement over sorted BED files, .starch
// archives (recognised by their magic) or stdin, computed on the GPU
// (starch_setop_host), BED3 to stdout.
//
// Exit codes as sort-bed (tools/sortbed_cli.cpp): 1 with the usage for a bad
// command line, ENODATA for a missing input, EINVAL for a data error (the
// library's text names the input and the line), ENOMEM, EIO.
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

#include "../include/starch_amd.h"

static const char* kName = "bedops";
static const char* kVersion = "0.1 (mi355x)";

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
            "USAGE: bedops (-m|--merge | -i|--intersect | -d|--difference | -s|--symmdiff |\n"
            "               -c|--complement) [--device N] file ...\n\n"
            "  Every file is sorted BED (see sort-bed) or a .starch archive, which is recognised\n"
            "  by its first four bytes and not by its name; - is stdin and may be named once.\n"
            "  Only the first three columns count, and every line needs stop > start.  Input k\n"
            "  covers the bases start <= x < stop of its lines; call that set S_k, with the\n"
            "  inputs numbered from 0 in argument order.  The result, as BED3 on stdout:\n\n"
            "  -m, --merge        the union of all S_k\n"
            "  -i, --intersect    the intersection of all S_k\n"
            "  -d, --difference   S_0 minus the union of the other inputs\n"
            "  -s, --symmdiff     the bases that lie in exactly one S_k\n"
            "  -c, --complement   per chromosome, the bases outside the union that lie between\n"
            "                     the chromosome's smallest start and its largest stop\n\n"
            "  One line is written for each maximal run of consecutive result bases, so\n"
            "  abutting pieces are joined: 0-10 and 10-20 become 0-20, wherever they came from.\n"
            "  Chromosomes come in sort-bed's order.  Exactly one operation must be given.\n\n"
            "  This is a definition by sets: it is believed to match BEDOPS' bedops for these\n"
            "  five options, but that is unverified against a BEDOPS binary.\n\n"
            "  An unsorted input, a line with stop <= start or a malformed line is reported\n"
            "  with its input number (from 0) and line number (from 1); nothing is written.\n\n"
            "  --device N     GPU to compute on (default 0)\n"
            "  --help, --version\n",
            kName, kVersion);
}

static bool read_all(int fd, std::vector<char>* out)
{
    const size_t kPiece = 16u << 20;
    for (;;) {
        const size_t at = out->size();
        out->resize(at + kPiece);
        const ssize_t r = read(fd, out->data() + at, kPiece);
        if (r < 0 && errno == EINTR) { out->resize(at); continue; }
        if (r < 0) { out->resize(at); return false; }
        out->resize(at + (size_t)r);
        if (r == 0) return true;
    }
}

int main(int argc, char** argv)
{
    int op = -1, nops = 0, device = 0;
    static struct option longs[] = {{"merge", no_argument, nullptr, 'm'},
                                    {"intersect", no_argument, nullptr, 'i'},
                                    {"difference", no_argument, nullptr, 'd'},
                                    {"symmdiff", no_argument, nullptr, 's'},
                                    {"complement", no_argument, nullptr, 'c'},
                                    {"device", required_argument, nullptr, 'D'},
                                    {"help", no_argument, nullptr, 'h'},
                                    {"version", no_argument, nullptr, 'v'},
                                    {nullptr, 0, nullptr, 0}};
    opterr = 0;
    int c, li;
    while ((c = getopt_long(argc, argv, "midschv", longs, &li)) != -1) {
        switch (c) {
            case 'm': op = STARCH_SETOP_MERGE; ++nops; break;
            case 'i': op = STARCH_SETOP_INTERSECT; ++nops; break;
            case 'd': op = STARCH_SETOP_DIFFERENCE; ++nops; break;
            case 's': op = STARCH_SETOP_SYMMDIFF; ++nops; break;
            case 'c': op = STARCH_SETOP_COMPLEMENT; ++nops; break;
            case 'D': device = atoi(optarg); break;
            case 'h': usage(stdout); return 0;
            case 'v': printf("%s\n  version: %s\n", kName, kVersion); return 0;
            default: usage(stderr); return EXIT_FAILURE;
        }
    }
    std::vector<std::string> paths;
    for (int i = optind; i < argc; ++i) paths.push_back(argv[i]);
    int dashes = 0;
    for (const std::string& p : paths) dashes += p == "-";
    if (nops != 1 || paths.empty() || dashes > 1) {
        if (dashes > 1) fprintf(stderr, "Error: stdin (-) may be named once\n");
        usage(stderr);
        return EXIT_FAILURE;
    }

    std::vector<std::vector<char>> data(paths.size());
    for (size_t k = 0; k < paths.size(); ++k) {
        const std::string& p = paths[k];
        const int fd = p == "-" ? STDIN_FILENO : open(p.c_str(), O_RDONLY);
        if (fd < 0) {
            fprintf(stderr, "Error: Input file does not exist (%s)\n", p.c_str());
            return ENODATA;
        }
        const bool ok = read_all(fd, &data[k]);
        if (fd != STDIN_FILENO) close(fd);
        if (!ok) {
            fprintf(stderr, "Error: reading %s failed (%s)\n", p.c_str(), strerror(errno));
            return EIO;
        }
    }
    std::vector<starch_setop_input> in(paths.size());
    for (size_t k = 0; k < paths.size(); ++k) in[k] = starch_setop_input{data[k].data(), (uint64_t)data[k].size()};

    starch_ctx* ctx = nullptr;
    int rc = starch_create(device, &ctx);
    if (rc != STARCH_OK) {
        fprintf(stderr, "Error: no GPU context (%s)\n", starch_strerror(rc));
        return EINVAL;
    }
    rc = starch_setop_host(ctx, op, in.data(), in.size());
    uint64_t bytes = 0;
    std::vector<char> out;
    if (rc == STARCH_OK) rc = starch_output_size(ctx, &bytes);
    if (rc == STARCH_OK && bytes) {
        out.resize(bytes);
        rc = starch_output_copy(ctx, out.data(), bytes);
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
    const bool ok = fflush(stdout) == 0 && !ferror(stdout);
    if (!ok) fprintf(stderr, "Error: writing the output failed (%s)\n", strerror(errno ? errno : EIO));
    starch_destroy(ctx);
    return ok ? 0 : EIO;
}
