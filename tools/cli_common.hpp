// tools/cli_common.hpp -- what the commands under tools/ share: reading their
// inputs, opening a GPU context, and bringing a result to stdout.  Header only.
// Every command keeps its own option parser, usage text and exit codes for a
// bad command line.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../include/starch_amd.h"

namespace cli {

inline void print_version(const char* name, const char* version) { printf("%s\n  version: %s\n", name, version); }

// fd read to its end, appended to *out
inline bool read_all(int fd, std::vector<char>* out)
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

// Every path (- is stdin) read to its end, path k into (*data)[k]; joined: all
// into (*data)[0], a file that does not end in '\n' getting one.  Returns 0,
// or after its message the exit code: ENODATA, EIO.
inline int load_inputs(const std::vector<std::string>& paths, std::vector<std::vector<char>>* data, bool joined = false)
{
    data->resize(joined ? 1 : paths.size());
    for (size_t k = 0; k < paths.size(); ++k) {
        const std::string& p = paths[k];
        std::vector<char>& buf = (*data)[joined ? 0 : k];
        const int fd = p == "-" ? STDIN_FILENO : open(p.c_str(), O_RDONLY);
        if (fd < 0) {
            fprintf(stderr, "Error: Input file does not exist (%s)\n", p.c_str());
            return ENODATA;
        }
        const size_t before = buf.size();
        const bool ok = read_all(fd, &buf);
        if (fd != STDIN_FILENO) close(fd);
        if (!ok) {
            fprintf(stderr, "Error: reading %s failed (%s)\n", p.c_str(), strerror(errno));
            return EIO;
        }
        if (joined && buf.size() > before && buf.back() != '\n') buf.push_back('\n');
    }
    return 0;
}

// starch_create; returns 0, or after its message the exit code EINVAL
inline int open_ctx(int device, starch_ctx** ctx)
{
    const int rc = starch_create(device, ctx);
    if (rc == STARCH_OK) return 0;
    fprintf(stderr, "Error: no GPU context (%s)\n", starch_strerror(rc));
    return EINVAL;
}

// stdout flushed; what: "output" or "archive", for the message when that failed
inline bool stdout_ok(const char* what)
{
    if (fflush(stdout) != 0 || ferror(stdout)) {
        fprintf(stderr, "Error: writing the %s failed (%s)\n", what, strerror(errno ? errno : EIO));
        fflush(stderr);
        return false;
    }
    return true;
}

// The end of a command whose library call (status rc) leaves its result in the
// context: the result goes to stdout and the context is destroyed.  Returns
// the exit code: 0, or EIO; for a failed call ENOMEM or EINVAL after the
// message err_fmt, whose two %s are starch_last_error and starch_strerror
// (%1$s and %2$s to print them the other way round).
inline int finish_output(starch_ctx* ctx, int rc, const char* err_fmt)
{
    uint64_t bytes = 0;
    std::vector<char> out;
    if (rc == STARCH_OK) rc = starch_output_size(ctx, &bytes);
    if (rc == STARCH_OK && bytes) {
        out.resize(bytes);
        rc = starch_output_copy(ctx, out.data(), bytes);
    }
    if (rc != STARCH_OK) {
        fprintf(stderr, err_fmt, starch_last_error(ctx), starch_strerror(rc));
        starch_destroy(ctx);
        return rc == STARCH_ERR_MEM ? ENOMEM : EINVAL;
    }
    for (uint64_t w = 0; w < bytes;) {
        const size_t k = fwrite(out.data() + w, 1, bytes - w, stdout);
        if (k == 0) break;
        w += k;
    }
    const bool ok = stdout_ok("output");
    starch_destroy(ctx);
    return ok ? 0 : EIO;
}

}  // namespace cli
