// tools/convert2bed_cli.cpp -- the `convert2bed` command: GFF3, GTF, VCF or WIG
// text (a file or stdin) converted to BED on the GPU (starch_convert_host), by
// default in sort-bed's order, to stdout; --output=starch writes the archive
// starch3 writes for that sorted BED (starch_convert_encode_host).
//
// Exit codes: 2 for a bad command line, an input format or an option this
// convert2bed does not have (answered before a GPU is opened), otherwise as
// bedops (tools/bedops_cli.cpp): ENODATA for a missing input, EINVAL for a line
// that does not fit its format (the library's text names the line), ENOMEM, EIO.
#include "cli_common.hpp"

static const char* kHelp =
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
    "    wig  the score is copied byte for byte; BEDOPS re-parses it and prints it with %f.\n\n"
    "  A line that does not fit its format is reported with its line number (from 1) and\n"
    "  nothing is written.\n";
static const cli::Command kCmd = {"convert2bed", "0.1 (mi355x)", kHelp, 2};   // 2: the exit code for a bad command line

int main(int argc, char** argv)
{
    enum { O_INPUT = 256, O_OUTPUT, O_NOSORT, O_KEEP, O_SNVS, O_INS, O_DEL };
    static struct option longs[] = {{"input", required_argument, nullptr, O_INPUT},
                                    {"output", required_argument, nullptr, O_OUTPUT},
                                    {"do-not-sort", no_argument, nullptr, O_NOSORT},
                                    {"keep-header", no_argument, nullptr, O_KEEP},
                                    {"snvs", no_argument, nullptr, O_SNVS},
                                    {"insertions", no_argument, nullptr, O_INS},
                                    {"deletions", no_argument, nullptr, O_DEL},
                                    CLI_COMMON_OPTIONS,
                                    {nullptr, 0, nullptr, 0}};
    static const char* const formats[] = {"gff", "gtf", "vcf", "wig"};   // STARCH_CONVERT_*
    starch_convert_options opt;
    memset(&opt, 0, sizeof opt);
    int device = 0, classes = 0;
    bool have_input = false, starch = false;
    opterr = 0;
    int c;
    while ((c = getopt_long(argc, argv, "", longs, nullptr)) != -1) {
        int e = cli::GO_ON;
        switch (c) {
            case O_INPUT: {
                if (have_input) return kCmd.bad("an option is given twice", "--input");
                for (uint32_t k = 0; k < 4; ++k)
                    if (!strcasecmp(optarg, formats[k])) { opt.format = k; have_input = true; }
                if (!have_input) return kCmd.bad("unsupported or unknown input format", optarg);
                break;
            }
            case O_OUTPUT: e = cli::take_output_format(kCmd, &starch); break;
            case O_NOSORT: opt.no_sort = 1; break;
            case O_KEEP: opt.keep_header = 1; break;
            case O_SNVS: opt.vcf_class = STARCH_VCF_SNVS; ++classes; break;
            case O_INS: opt.vcf_class = STARCH_VCF_INSERTIONS; ++classes; break;
            case O_DEL: opt.vcf_class = STARCH_VCF_DELETIONS; ++classes; break;
            default: e = cli::take_common(kCmd, c, argv, &device);
        }
        if (e != cli::GO_ON) return e;
    }
    if (!have_input) return kCmd.bad("--input=gff|gtf|vcf|wig is needed", nullptr);
    if (classes > 1) return kCmd.bad("at most one of --snvs, --insertions and --deletions", nullptr);
    if (classes && opt.format != STARCH_CONVERT_VCF) return kCmd.bad("--snvs, --insertions and --deletions go with --input=vcf", nullptr);
    return cli::run_converter(kCmd, argc, argv, device, starch, starch_convert_host, starch_convert_encode_host, &opt);
}
