// tools/convert2bed_cli.cpp -- the `convert2bed` command: GFF3, GTF, VCF or WIG
// text (a file or stdin) converted to BED on the GPU (starch_convert_host), by
// default in sort-bed's order, to stdout; --output=starch writes the archive
// starch3 writes for that sorted BED (starch_convert_encode_host).
//
// Exit codes: 2 for a bad command line, an input format or an option this
// convert2bed does not have (answered before a GPU is opened), otherwise as
// bedops (tools/bedops_cli.cpp): ENODATA for a missing input, EINVAL for a line
// that does not fit its format (the library's text names the line), ENOMEM, EIO.
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <string>
#include <vector>

#include "cli_common.hpp"

static const char* kName = "convert2bed";
static const char* kVersion = "0.1 (mi355x)";
static const int kUsageError = 2;

static void usage(FILE* f)
{
    fprintf(f,
            "%s\n  version: %s\n\n"
            "USAGE: convert2bed --input=gff|gtf|vcf|wig [--output=bed|starch] [--do-not-sort] [--keep-header]\n"
            "                   [--snvs|--insertions|--deletions] [--device N] [file | -]\n\n"
            "  The file (no file, or -: stdin) is converted to BED on the GPU and written to stdout,\n"
            "  in sort-bed's order unless --do-not-sort is given.  The format name may be in either\n"
            "  case.  Lines end at a newline; a carriage return is an ordinary byte.\n\n"
            "  --input=gff       seqid, start-1, end, ID, score, strand, source, type, phase, attributes;\n"
            "                    ID is the value of the first ID= piece of the attributes, or . ;\n"
            "                    a line that is exactly ##FASTA ends the input\n"
            "  --input=gtf       the same; ID is the value of the first gene_id \"...\", or .\n"
            "  --input=vcf       CHROM, POS-1, POS-1+len(REF), ID, QUAL, REF, ALT, FILTER, INFO and\n"
            "                    every column after it\n"
            "  --input=wig       chrom, start, stop, id-N, score for every data line of variableStep,\n"
            "                    fixedStep and four-column sections; N counts the data lines from 1\n"
            "  --output=bed      BED text (the default)\n"
            "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
            "  --do-not-sort     leave the lines in input order\n"
            "  --keep-header     header line K (from 0: an empty line, a # line, a WIG track or\n"
            "                    browser line) becomes  _header TAB K TAB K+1 TAB line ; by default\n"
            "                    header lines are dropped\n"
            "  --snvs, --insertions, --deletions\n"
            "                    vcf only, one of them: ALT is split at commas and one line is written\n"
            "                    per allele as long as REF, longer than REF, or shorter than REF\n"
            "  --device N        GPU to compute on (default 0)\n"
            "  --help, --version\n\n"
            "  Not supported: --input=bam|sam|psl|rmsk, --multisplit, --zero-indexed, --do-not-split,\n"
            "  --max-mem, --sort-tmpdir.\n\n"
            "  The definitions are modelled on BEDOPS' convert2bed, but they are unverified against a\n"
            "  BEDOPS binary.  Known differences:\n"
            "    gff  BEDOPS adds zero_length_insertion=True to the attributes when start equals end;\n"
            "         this converter does not.\n"
            "    gtf  BEDOPS refuses a record without gene_id; here its ID is . .\n"
            "    vcf  the stop is start + len(REF), the REF-length rule; BEDOPS' rule has changed\n"
            "         between releases.\n"
            "    wig  the score is copied byte for byte; BEDOPS re-parses it and prints it with %%f.\n\n"
            "  A line that does not fit its format is reported with its line number (from 1) and\n"
            "  nothing is written.\n",
            kName, kVersion);
}

static int bad_usage(const char* why, const char* what)
{
    fprintf(stderr, "Error: %s%s%s\n", why, what ? ": " : "", what ? what : "");
    usage(stderr);
    return kUsageError;
}

int main(int argc, char** argv)
{
    enum { O_INPUT = 256, O_OUTPUT, O_NOSORT, O_KEEP, O_SNVS, O_INS, O_DEL, O_DEVICE, O_HELP, O_VERSION };
    static struct option longs[] = {{"input", required_argument, nullptr, O_INPUT},
                                    {"output", required_argument, nullptr, O_OUTPUT},
                                    {"do-not-sort", no_argument, nullptr, O_NOSORT},
                                    {"keep-header", no_argument, nullptr, O_KEEP},
                                    {"snvs", no_argument, nullptr, O_SNVS},
                                    {"insertions", no_argument, nullptr, O_INS},
                                    {"deletions", no_argument, nullptr, O_DEL},
                                    {"device", required_argument, nullptr, O_DEVICE},
                                    {"help", no_argument, nullptr, O_HELP},
                                    {"version", no_argument, nullptr, O_VERSION},
                                    {nullptr, 0, nullptr, 0}};
    static const char* const formats[] = {"gff", "gtf", "vcf", "wig"};   // STARCH_CONVERT_*
    starch_convert_options opt;
    memset(&opt, 0, sizeof opt);
    int device = 0, classes = 0;
    bool have_input = false, starch = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        switch (c) {
            case O_INPUT: {
                if (have_input) return bad_usage("an option is given twice", "--input");
                for (uint32_t k = 0; k < 4; ++k)
                    if (!strcasecmp(optarg, formats[k])) { opt.format = k; have_input = true; }
                if (!have_input) return bad_usage("unsupported or unknown input format", optarg);
                break;
            }
            case O_OUTPUT:
                if (!strcasecmp(optarg, "starch")) starch = true;
                else if (!strcasecmp(optarg, "bed")) starch = false;
                else return bad_usage("unsupported or unknown output format", optarg);
                break;
            case O_NOSORT: opt.no_sort = 1; break;
            case O_KEEP: opt.keep_header = 1; break;
            case O_SNVS: opt.vcf_class = STARCH_VCF_SNVS; ++classes; break;
            case O_INS: opt.vcf_class = STARCH_VCF_INSERTIONS; ++classes; break;
            case O_DEL: opt.vcf_class = STARCH_VCF_DELETIONS; ++classes; break;
            case O_DEVICE: device = atoi(optarg); break;
            case O_HELP: usage(stdout); return 0;
            case O_VERSION: cli::print_version(kName, kVersion); return 0;
            default: return bad_usage("unsupported or unknown option", argv[optind - 1]);
        }
    }
    if (!have_input) return bad_usage("--input=gff|gtf|vcf|wig is needed", nullptr);
    if (classes > 1) return bad_usage("at most one of --snvs, --insertions and --deletions", nullptr);
    if (classes && opt.format != STARCH_CONVERT_VCF) return bad_usage("--snvs, --insertions and --deletions go with --input=vcf", nullptr);
    if (starch && opt.no_sort) return bad_usage("--output=starch needs the sort", "--do-not-sort");
    std::vector<std::string> paths;
    for (int i = optind; i < argc; ++i) paths.push_back(argv[i]);
    if (paths.size() > 1) return bad_usage("one input file at most", paths[1].c_str());
    if (paths.empty()) paths.push_back("-");

    std::vector<std::vector<char>> data;
    if (const int e = cli::load_inputs(paths, &data)) return e;

    starch_ctx* ctx = nullptr;
    if (const int e = cli::open_ctx(device, &ctx)) return e;
    if (!starch)
        return cli::finish_output(ctx, starch_convert_host(ctx, data[0].data(), data[0].size(), &opt), "Error: %s (%s)\n");

    int rc = starch_convert_encode_host(ctx, data[0].data(), data[0].size(), &opt, nullptr);
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
