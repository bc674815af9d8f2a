// tools/starchzcat_cli.cpp -- the `starch-zcat` command: gzip and BGZF files
// inflated on the GPU (starch_gunzip_host) to stdout, in the order given;
// --list prints the member table that the headers of a BGZF file give
// (starch_gunzip_plan) and opens no GPU.
//
// Exit codes: 2 for a bad command line (answered before a GPU is opened),
// ENODATA for a missing input, EINVAL for a data error after the library's
// message (it names the member, its byte offset and the reason), ENOMEM, EIO.
#include "cli_common.hpp"

static const char* kHelp =
    "USAGE: starch-zcat [--list] [--device N] [file ... | -]\n\n"
    "  The files (no file, or -: stdin) are gzip: one or more members back to back, as\n"
    "  gzip, pigz and bgzip write them.  Their inflated bytes go to stdout in order.\n"
    "  A file whose every member has bgzip's BC subfield (BGZF: .vcf.gz, .bed.gz from\n"
    "  bgzip, BAM's framing) is decoded with all its members at once, one wave each;\n"
    "  any other gzip file is found member by member and a single member is decoded\n"
    "  by one wave: correct, and serial.  CRC-32 and ISIZE of every member are checked.\n\n"
    "  --list         the plan, and nothing is inflated: for a BGZF file one line per\n"
    "                 member (offset, compressed bytes, output offset, ISIZE, CRC-32;\n"
    "                 tab-separated), for any other gzip file the word generic\n"
    "  --device N     GPU to inflate on (default 0)\n"
    "  --help, --version\n\n"
    "  A corrupt or truncated member, bytes after the last member that begin no\n"
    "  member, or an input that is not gzip: the first bad member is reported with\n"
    "  its number (from 0) and byte offset, and nothing of that file is written.\n";
static const cli::Command kCmd = {"starch-zcat", "0.1 (mi355x)", kHelp, 2};   // 2: the exit code for a bad command line

int main(int argc, char** argv)
{
    enum { O_LIST = 256 };
    static struct option longs[] = {{"list", no_argument, nullptr, O_LIST}, CLI_COMMON_OPTIONS, {nullptr, 0, nullptr, 0}};
    int device = 0;
    bool list = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e = cli::GO_ON;
        switch (c) {
            case O_LIST: list = true; break;
            default: e = cli::take_common(kCmd, c, argv, &device);
        }
        if (e != cli::GO_ON) return e;
    }
    std::vector<std::string> paths(argv + optind, argv + argc);
    if (paths.empty()) paths.push_back("-");
    int dashes = 0;
    for (const std::string& p : paths) dashes += p == "-";
    if (dashes > 1) return kCmd.bad("stdin (-) may be named once", nullptr);
    std::vector<std::vector<char>> data;
    if (const int e = cli::load_inputs(paths, &data)) return e;

    if (list) {
        for (size_t k = 0; k < paths.size(); ++k) {
            uint64_t count = 0;
            int bgzf = 0;
            int rc = starch_gunzip_plan(data[k].data(), data[k].size(), nullptr, 0, &count, &bgzf);
            std::vector<starch_gunzip_member> mem(count ? count : 1);
            if (rc == STARCH_OK && count)
                rc = starch_gunzip_plan(data[k].data(), data[k].size(), mem.data(), count, &count, &bgzf);
            if (rc != STARCH_OK) {
                fprintf(stderr, "Error: %s: the gzip headers could not be read (%s)\n", paths[k].c_str(), starch_strerror(rc));
                return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
            }
            if (!bgzf) { printf("generic\n"); continue; }
            for (uint64_t m = 0; m < count; ++m)
                printf("%llu\t%llu\t%llu\t%u\t%08x\n", (unsigned long long)mem[m].in_off, (unsigned long long)mem[m].in_len,
                       (unsigned long long)mem[m].out_off, mem[m].isize, mem[m].crc);
        }
        return cli::stdout_ok("output") ? 0 : EIO;
    }

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    std::vector<char> out;
    for (size_t k = 0; k < paths.size(); ++k) {
        uint64_t bytes = 0;
        int rc = starch_gunzip_host(ctx, data[k].data(), data[k].size());
        if (rc == STARCH_OK) rc = starch_output_size(ctx, &bytes);
        if (rc == STARCH_OK && bytes) {
            out.resize(bytes);
            rc = starch_output_copy(ctx, out.data(), bytes);
        }
        if (rc != STARCH_OK) {
            fflush(stdout);
            fprintf(stderr, "Error: %s: %s (%s)\n", paths[k].c_str(), starch_last_error(ctx), starch_strerror(rc));
            starch_destroy(ctx);
            return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
        }
        for (uint64_t w = 0; w < bytes;) {
            const size_t n = fwrite(out.data() + w, 1, bytes - w, stdout);
            if (n == 0) break;
            w += n;
        }
    }
    const bool ok = cli::stdout_ok("output");
    starch_destroy(ctx);
    return ok ? 0 : EIO;
}
