// tools/bedops_cli.cpp -- the `bedops` command: --merge, --intersect,
// --difference, --symmdiff, --complement, --element-of, --not-element-of,
// --partition, --chop or --everything over sorted BED files, .starch archives
// (recognised by their magic) or stdin, computed on the GPU
// (starch_bedops_host), to stdout.
//
// Exit codes as sort-bed (tools/sortbed_cli.cpp): 1 with the usage for a bad
// command line, ENODATA for a missing input, EINVAL for a data error (the
// library's text names the input and the line), ENOMEM, EIO.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "cli_common.hpp"

static const char* kName = "bedops";
static const char* kVersion = "0.2 (mi355x)";

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
            "USAGE: bedops (-m|--merge | -i|--intersect | -d|--difference | -s|--symmdiff |\n"
            "               -c|--complement | -e|--element-of [V] | -n|--not-element-of [V] |\n"
            "               -p|--partition | -w|--chop [W] [--stagger G] [-x] | -u|--everything)\n"
            "              [--device N] file ...\n\n"
            "  Every file is sorted BED (see sort-bed) or a .starch archive, which is recognised\n"
            "  by its first four bytes and not by its name; - is stdin and may be named once.\n"
            "  Every line needs stop > start.  Input k covers the bases start <= x < stop of its\n"
            "  lines; call that set S_k, with the inputs numbered from 0 in argument order.\n"
            "  Exactly one operation must be given.\n\n"
            "  Five operations look at the first three columns only and write BED3:\n\n"
            "  -m, --merge        the union of all S_k\n"
            "  -i, --intersect    the intersection of all S_k\n"
            "  -d, --difference   S_0 minus the union of the other inputs\n"
            "  -s, --symmdiff     the bases that lie in exactly one S_k\n"
            "  -c, --complement   per chromosome, the bases outside the union that lie between\n"
            "                     the chromosome's smallest start and its largest stop\n\n"
            "  One line is written for each maximal run of consecutive result bases, so\n"
            "  abutting pieces are joined: 0-10 and 10-20 become 0-20, wherever they came from.\n"
            "  Chromosomes come in sort-bed's order.\n\n"
            "  Two keep whole lines of the first file, every column, in its order:\n\n"
            "  -e, --element-of [V]      the lines of file 0 that overlap the other files enough\n"
            "  -n, --not-element-of [V]  the lines of file 0 that do not\n"
            "                     At least two files.  U is the set of maximal runs of the union\n"
            "                     of files 1 .. N-1, abutting runs joined.  For a line (c, s, e),\n"
            "                     ov is the largest min(b,e) - max(a,s) over the runs [a,b) of U\n"
            "                     on c, 0 if none overlaps: the largest overlap with one run, not\n"
            "                     the total over several.  V is a number of bases (the line is\n"
            "                     selected when ov >= V, V >= 1) or a percentage such as 50%%\n"
            "                     (selected when ov * 100 >= V * (e - s), V from 1 to 100).\n"
            "                     V is read only when the next argument is all digits, with or\n"
            "                     without a final %%; otherwise it is a file.  Default 100%%.\n\n"
            "  Two more write BED3 and never join pieces:\n\n"
            "  -p, --partition    all lines of all files together, not merged: per chromosome,\n"
            "                     for consecutive p, q in the sorted set of distinct starts and\n"
            "                     stops, c p q when at least one line covers it; a piece is\n"
            "                     written once however many lines cover it\n"
            "  -w, --chop [W]     the merged regions cut into pieces of W bases (default 1): for a\n"
            "                     run [a,b) of the merge of all files and k = 0, 1, ... while\n"
            "                     a + k*G < b, the piece from a + k*G to min(a + k*G + W, b)\n"
            "      --stagger G    the step from one piece's start to the next (default W)\n"
            "      -x             leave out pieces shorter than W\n"
            "                     --stagger and -x are valid only with --chop.  A result of 2^32\n"
            "                     pieces or 2^40 bytes or more is refused.\n\n"
            "  And one writes every line of every file, every column:\n\n"
            "  -u, --everything   ordered by chromosome, start and stop as sort-bed orders them;\n"
            "                     ties by file and then line number\n\n"
            "  These are definitions by sets: they are believed to match BEDOPS' bedops for these\n"
            "  ten options, but that is unverified against a BEDOPS binary.\n\n"
            "  An unsorted input, a line with stop <= start or a malformed line is reported\n"
            "  with its input number (from 0) and line number (from 1); nothing is written.\n\n"
            "  --device N     GPU to compute on (default 0)\n"
            "  --help, --version\n\n"
            "  A long option may be cut short while only one name begins that way, and its value\n"
            "  may be attached with = (--chop=100, --element-of=50%%).\n",
            kName, kVersion);
}

// [0-9]+ (pct == nullptr) or [0-9]+%? in full, and the number fits 64 bits
static bool number_arg(const char* s, uint64_t* v, bool* pct)
{
    size_t n = strlen(s);
    if (pct) {
        *pct = n > 0 && s[n - 1] == '%';
        if (*pct) --n;
    }
    if (n == 0) return false;
    uint64_t x = 0;
    for (size_t k = 0; k < n; ++k) {
        if (s[k] < '0' || s[k] > '9') return false;
        if (x > (~0ull - (uint64_t)(s[k] - '0')) / 10) { x = ~0ull; continue; }   // too large: saturates, refused below
        x = x * 10 + (uint64_t)(s[k] - '0');
    }
    *v = x;
    return true;
}

int main(int argc, char** argv)
{
    int nops = 0, device = 0;
    bool have_stagger = false, have_x = false, bad = false;
    starch_bedops_options opt;
    memset(&opt, 0, sizeof(opt));
    opt.op = -1;
    opt.threshold = 100;
    opt.threshold_is_percent = 1;
    opt.chop = 1;
    std::vector<std::string> paths;

    // the optional value of the option at argv[i]: taken only when argv[i + 1] has its form in full;
    // a value attached with = (--chop=5) must have it
    const char* attached_value = nullptr;
    auto optional = [&](int* i, bool with_pct, uint64_t* v, bool* pct) {
        uint64_t x = 0;
        bool p = false;
        if (attached_value) {
            if (!number_arg(attached_value, &x, with_pct ? &p : nullptr)) { bad = true; return; }
            *v = x;
            if (pct) *pct = p;
        } else if (*i + 1 < argc && number_arg(argv[*i + 1], &x, with_pct ? &p : nullptr)) {
            ++*i;
            *v = x;
            if (pct) *pct = p;
        }
    };
    auto set_op = [&](int op) { opt.op = op; ++nops; };
    auto element = [&](int op, int* i) {
        set_op(op);
        uint64_t v = 100;
        bool pct = true;
        optional(i, true, &v, &pct);
        opt.threshold = v;
        opt.threshold_is_percent = pct ? 1 : 0;
        if (v == 0 || v == ~0ull || (pct && v > 100)) bad = true;
    };
    auto chop = [&](int* i) {
        set_op(STARCH_SETOP_CHOP);
        uint64_t v = 1;
        optional(i, false, &v, nullptr);
        opt.chop = v;
        if (v == 0 || v == ~0ull) bad = true;
    };
    // a value that must follow (--stagger G, --device N)
    auto required = [&](int* i, const char* attached, uint64_t* v) {
        const char* s = attached ? attached : (*i + 1 < argc ? argv[++*i] : nullptr);
        if (!s || !number_arg(s, v, nullptr) || *v == ~0ull) bad = true;
    };

    bool files_only = false;
    for (int i = 1; i < argc && !bad; ++i) {
        const std::string a = argv[i];
        if (files_only || a == "-" || a.empty() || a[0] != '-') { paths.push_back(a); continue; }
        if (a == "--") { files_only = true; continue; }
        if (a[1] == '-') {
            const size_t eq = a.find('=');
            std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            const char* attached = eq == std::string::npos ? nullptr : argv[i] + eq + 1;
            // as getopt_long did: an exact name, or a prefix that only one name has
            static const char* const kLongs[] = {"merge", "intersect", "difference", "symmdiff", "complement", "element-of",
                                                 "not-element-of", "partition", "chop", "everything", "stagger", "device",
                                                 "help", "version"};
            const char* match = nullptr;
            int matches = 0;
            for (const char* l : kLongs) {
                if (name == l) { match = l; matches = 1; break; }
                if (!name.empty() && strncmp(l, name.c_str(), name.size()) == 0) { match = l; ++matches; }
            }
            if (matches != 1) { bad = true; continue; }
            name = match;
            uint64_t v = 0;
            if (name == "stagger") { required(&i, attached, &v); opt.stagger = v; have_stagger = true; if (v == 0) bad = true; continue; }
            if (name == "device") {   // read with atoi, as before
                const char* s = attached ? attached : (i + 1 < argc ? argv[++i] : nullptr);
                if (!s) bad = true;
                else device = atoi(s);
                continue;
            }
            const bool takes_value = name == "element-of" || name == "not-element-of" || name == "chop";
            if (attached && !takes_value) { bad = true; continue; }
            attached_value = attached;
            if (name == "merge") set_op(STARCH_SETOP_MERGE);
            else if (name == "intersect") set_op(STARCH_SETOP_INTERSECT);
            else if (name == "difference") set_op(STARCH_SETOP_DIFFERENCE);
            else if (name == "symmdiff") set_op(STARCH_SETOP_SYMMDIFF);
            else if (name == "complement") set_op(STARCH_SETOP_COMPLEMENT);
            else if (name == "element-of") element(STARCH_SETOP_ELEMENT_OF, &i);
            else if (name == "not-element-of") element(STARCH_SETOP_NOT_ELEMENT_OF, &i);
            else if (name == "partition") set_op(STARCH_SETOP_PARTITION);
            else if (name == "chop") chop(&i);
            else if (name == "everything") set_op(STARCH_SETOP_EVERYTHING);
            else if (name == "help") { usage(stdout); return 0; }
            else if (name == "version") { cli::print_version(kName, kVersion); return 0; }
            else bad = true;
            attached_value = nullptr;
            continue;
        }
        // short options, possibly several in one argument; -e, -n and -w look for their value only as the last one
        for (size_t k = 1; k < a.size() && !bad; ++k) {
            const bool is_last = k + 1 == a.size();
            int at = i;
            switch (a[k]) {
                case 'm': set_op(STARCH_SETOP_MERGE); break;
                case 'i': set_op(STARCH_SETOP_INTERSECT); break;
                case 'd': set_op(STARCH_SETOP_DIFFERENCE); break;
                case 's': set_op(STARCH_SETOP_SYMMDIFF); break;
                case 'c': set_op(STARCH_SETOP_COMPLEMENT); break;
                case 'p': set_op(STARCH_SETOP_PARTITION); break;
                case 'u': set_op(STARCH_SETOP_EVERYTHING); break;
                case 'x': have_x = true; break;
                case 'e':
                case 'n':
                case 'w':
                    if (!is_last) at = argc;   // no value to look at
                    if (a[k] == 'w') chop(&at);
                    else element(a[k] == 'e' ? STARCH_SETOP_ELEMENT_OF : STARCH_SETOP_NOT_ELEMENT_OF, &at);
                    if (is_last) i = at;
                    break;
                case 'h': usage(stdout); return 0;
                case 'v': cli::print_version(kName, kVersion); return 0;
                default: bad = true;
            }
        }
    }
    opt.exclude_short = have_x ? 1 : 0;
    int dashes = 0;
    for (const std::string& p : paths) dashes += p == "-";
    const bool element_op = opt.op == STARCH_SETOP_ELEMENT_OF || opt.op == STARCH_SETOP_NOT_ELEMENT_OF;
    if (bad || nops != 1 || paths.empty() || dashes > 1 || ((have_stagger || have_x) && opt.op != STARCH_SETOP_CHOP) ||
        (element_op && paths.size() < 2)) {
        if (dashes > 1) fprintf(stderr, "Error: stdin (-) may be named once\n");
        else if (!bad && nops == 1 && (have_stagger || have_x) && opt.op != STARCH_SETOP_CHOP)
            fprintf(stderr, "Error: --stagger and -x are valid only with --chop\n");
        else if (!bad && nops == 1 && element_op && paths.size() == 1)
            fprintf(stderr, "Error: --element-of and --not-element-of need at least two files\n");
        usage(stderr);
        return EXIT_FAILURE;
    }

    std::vector<std::vector<char>> data;
    if (const int e = cli::load_inputs(paths, &data)) return e;
    std::vector<starch_setop_input> in(paths.size());
    for (size_t k = 0; k < paths.size(); ++k) in[k] = starch_setop_input{data[k].data(), (uint64_t)data[k].size()};

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    return cli::finish_output(ctx, starch_bedops_host(ctx, &opt, in.data(), in.size()), "Error: %s (%s)\n");
}
