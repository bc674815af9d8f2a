// tools/cli_common.hpp -- what the commands under tools/ share: the pieces of
// an option parser, reading their inputs, opening a GPU context, and bringing a
// result to stdout.  Header only.  A command keeps its usage text, its option
// table and defaults, its exit code for a bad command line and the options that
// no other command has; the texts in which the commands differ are parameters.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <unistd.h>

#include <functional>
#include <string>
#include <vector>

#include "../include/starch_amd.h"

namespace cli {

inline void print_version(const char* name, const char* version) { printf("%s\n  version: %s\n", name, version); }

// ---- the command line.  The take_* functions below return GO_ON, or the
// exit code after what they wrote; they read getopt's optarg and optind. ----
enum { GO_ON = -1 };
typedef std::function<void(FILE*)> usage_fn;

// "Error: why[: what]" and the usage text to stderr; returns exit_code
inline int bad_usage(const usage_fn& usage, int exit_code, const char* why, const char* what)
{
    fprintf(stderr, "Error: %s%s%s\n", why, what ? ": " : "", what ? what : "");
    usage(stderr);
    return exit_code;
}

// A command's name, version, help (all of --help after the version lines; it
// holds the USAGE line) and exit code for a bad command line
struct Command {
    const char* name;
    const char* version;
    const char* help;
    int usage_error;
    void usage(FILE* f) const { fprintf(f, "%s\n  version: %s\n\n%s", name, version, help); }
    int bad(const char* why, const char* what) const
    {
        return bad_usage([this](FILE* f) { usage(f); }, usage_error, why, what);
    }
};

// --device N, --help and --version: their getopt values, above any command's own, and their table entries
enum { O_DEVICE = 1000, O_HELP, O_VERSION };
#define CLI_COMMON_OPTIONS \
    {"device", required_argument, nullptr, cli::O_DEVICE}, {"help", no_argument, nullptr, cli::O_HELP}, \
    {"version", no_argument, nullptr, cli::O_VERSION}

// The options every command has; any other value of c is an unknown option
inline int take_common(const Command& cmd, int c, char** argv, int* device)
{
    if (c == O_DEVICE) { *device = atoi(optarg); return GO_ON; }
    if (c == O_HELP) { cmd.usage(stdout); return 0; }
    if (c == O_VERSION) { print_version(cmd.name, cmd.version); return 0; }
    return cmd.bad("unsupported or unknown option", argv[optind - 1]);
}

// all of s as an unsigned decimal that fits 64 bits
inline bool parse_u64(const char* s, uint64_t* v)
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

// digits [. digits] with a digit somewhere, at most 9 after the point and a value in (0, 1]
inline bool parse_fraction(const char* s, uint64_t* num, uint32_t* digits)
{
    uint64_t whole = 0, frac = 0, den = 1;
    uint32_t nd = 0, any = 0;
    const char* p = s;
    for (; *p >= '0' && *p <= '9'; ++p, ++any)
        if ((whole = whole * 10 + (uint64_t)(*p - '0')) > 1) return false;
    if (*p == '.')
        for (++p; *p >= '0' && *p <= '9'; ++p, ++any) {
            if (++nd > 9) return false;
            frac = frac * 10 + (uint64_t)(*p - '0');
            den *= 10;
        }
    if (*p || !any) return false;
    const uint64_t v = whole * den + frac;
    if (v == 0 || v > den) return false;
    *num = v;
    *digits = nd;
    return true;
}

// An option that may be given once, which *have (a bool, or a flag of the
// options) records; name is its name for the message
template <class Flag>
int take_once(const Command& cmd, Flag* have, const char* name)
{
    if (*have) return cmd.bad("an option is given twice", name);
    *have = 1;
    return GO_ON;
}

// A column option: col is appended to opt->cols unless it is there already
template <class Options>
int take_column(const Command& cmd, Options* opt, int col, const char* name)
{
    for (uint32_t k = 0; k < opt->ncols; ++k)
        if (opt->cols[k] == col) return cmd.bad("an option is given twice", name);
    opt->cols[opt->ncols++] = (uint8_t)col;
    return GO_ON;
}

// With no column option: the columns a and b
template <class Options>
void default_columns(Options* opt, uint8_t a, uint8_t b)
{
    if (opt->ncols) return;
    opt->cols[0] = a;
    opt->cols[1] = b;
    opt->ncols = 2;
}

// The overlap criteria of bedmap-elements and bedmap-scores, from the value first on
#define CLI_CRITERION_OPTIONS(first) \
    {"bp-ovr", required_argument, nullptr, (first) + STARCH_MAPEL_CRIT_BP_OVR}, \
    {"range", required_argument, nullptr, (first) + STARCH_MAPEL_CRIT_RANGE}, \
    {"fraction-ref", required_argument, nullptr, (first) + STARCH_MAPEL_CRIT_FRACTION_REF}, \
    {"fraction-map", required_argument, nullptr, (first) + STARCH_MAPEL_CRIT_FRACTION_MAP}, \
    {"fraction-both", required_argument, nullptr, (first) + STARCH_MAPEL_CRIT_FRACTION_BOTH}, \
    {"fraction-either", required_argument, nullptr, (first) + STARCH_MAPEL_CRIT_FRACTION_EITHER}, \
    {"exact", no_argument, nullptr, (first) + STARCH_MAPEL_CRIT_EXACT}

// A criterion option (crit: STARCH_MAPEL_CRIT_*) into the fields that
// starch_mapel_options and starch_mapsc_options both have; at most one
template <class Options>
int take_criterion(const Command& cmd, Options* opt, bool* have, uint32_t crit, char** argv)
{
    if (*have) return cmd.bad("at most one overlap criterion may be given", argv[optind - 1]);
    *have = true;
    opt->criterion = crit;
    opt->n = 0;
    if (crit == STARCH_MAPEL_CRIT_BP_OVR) {
        if (!parse_u64(optarg, &opt->n) || opt->n == 0) return cmd.bad("--bp-ovr needs a number of bases, 1 or more", optarg);
    } else if (crit == STARCH_MAPEL_CRIT_RANGE) {
        if (!parse_u64(optarg, &opt->range)) return cmd.bad("--range needs a number of bases", optarg);
    } else if (crit != STARCH_MAPEL_CRIT_EXACT) {
        if (!parse_fraction(optarg, &opt->frac_num, &opt->frac_digits))
            return cmd.bad("a fraction is a decimal above 0 and up to 1 with at most 9 digits after the point", optarg);
    }
    return GO_ON;
}

// A delimiter option of 1 to 8 bytes, given once; why_length is the command's message for another length
inline int take_delim(const Command& cmd, char (&delim)[8], uint32_t* len, bool* have, const char* name, const char* why_length)
{
    if (const int e = take_once(cmd, have, name); e != GO_ON) return e;
    const size_t n = strlen(optarg);
    if (n < 1 || n > sizeof delim) return cmd.bad(why_length, optarg);
    memcpy(delim, optarg, n);
    *len = (uint32_t)n;
    return GO_ON;
}


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
// (%1$s and %2$s to print them the other way round).  archive: the result is
// the context's archive (never empty) and not its output.
inline int finish_output(starch_ctx* ctx, int rc, const char* err_fmt, bool archive = false)
{
    uint64_t bytes = 0;
    std::vector<char> out;
    if (rc == STARCH_OK) rc = (archive ? starch_archive_size : starch_output_size)(ctx, &bytes);
    if (rc == STARCH_OK && bytes) {
        out.resize(bytes);
        rc = (archive ? starch_archive_copy : starch_output_copy)(ctx, out.data(), bytes);
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
    const bool ok = stdout_ok(archive ? "archive" : "output");
    starch_destroy(ctx);
    return ok ? 0 : EIO;
}

// The end of a command with two inputs.  The arguments after the options are
// their paths: least (1 or 2) to two of them, else why_count is the message; -
// may be one of them.  They are read, a context is opened on device,
// host(ctx, first, second or NULL, opt) is called and its output written.
// Returns the exit code.
template <class Host, class Options>
int run_two_inputs(const Command& cmd, int argc, char** argv, size_t least, const char* why_count, int device, Host host,
                   const Options* opt)
{
    const std::vector<std::string> paths(argv + optind, argv + argc);
    if (paths.size() < least || paths.size() > 2) return cmd.bad(why_count, nullptr);
    if (paths.size() == 2 && paths[0] == "-" && paths[1] == "-") return cmd.bad("stdin (-) may be named once", nullptr);
    std::vector<std::vector<char>> data;
    if (const int e = load_inputs(paths, &data)) return e;
    starch_setop_input in[2];
    for (size_t k = 0; k < paths.size(); ++k) in[k] = starch_setop_input{data[k].data(), (uint64_t)data[k].size()};
    starch_ctx* ctx = nullptr;
    if (const int e = open_ctx(device, &ctx)) return e;
    return finish_output(ctx, host(ctx, &in[0], paths.size() == 2 ? &in[1] : nullptr, opt), "Error: %s (%s)\n");
}

// The end of a converter: its one input (a path after the options, or stdin)
// read, a context opened on device, and the output of host(ctx, data, n, opt)
// written, or with archive the archive of encode(ctx, data, n, opt, NULL),
// which needs the sort.
template <class Host, class Encode, class Options>
int run_converter(const Command& cmd, int argc, char** argv, int device, bool archive, Host host, Encode encode, const Options* opt)
{
    if (archive && opt->no_sort) return cmd.bad("--output=starch needs the sort", "--do-not-sort");
    std::vector<std::string> paths(argv + optind, argv + argc);
    if (paths.size() > 1) return cmd.bad("one input file at most", paths[1].c_str());
    if (paths.empty()) paths.push_back("-");
    std::vector<std::vector<char>> data;
    if (const int e = load_inputs(paths, &data)) return e;
    starch_ctx* ctx = nullptr;
    if (const int e = open_ctx(device, &ctx)) return e;
    const int rc = archive ? encode(ctx, data[0].data(), data[0].size(), opt, nullptr) : host(ctx, data[0].data(), data[0].size(), opt);
    return finish_output(ctx, rc, "Error: %s (%s)\n", archive);
}

// --output=bed|starch of a converter, in either case
inline int take_output_format(const Command& cmd, bool* archive)
{
    if (!strcasecmp(optarg, "starch")) *archive = true;
    else if (!strcasecmp(optarg, "bed")) *archive = false;
    else return cmd.bad("unsupported or unknown output format", optarg);
    return GO_ON;
}

}  // namespace cli
