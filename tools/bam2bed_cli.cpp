// tools/bam2bed_cli.cpp -- the `bam2bed` command: BAM (BGZF, gzip or inflated) to
// BED on the GPU (tools/align2bed_cli.hpp has the command line and the exit codes).
#include "align2bed_cli.hpp"

static const char* kHelp =
    "USAGE: bam2bed [--output=bed|starch] [--do-not-sort] [--keep-header] [--split] [--split-with-deletions]\n"
    "               [--all-reads] [--reduced] [--device N] [file | -]\n\n"
    "  BAM (no file, or -: stdin) is inflated, cut into records and converted to BED on the GPU and\n"
    "  written to stdout, in sort-bed's order unless --do-not-sort is given.  The output is, byte for\n"
    "  byte, what sam2bed with the same options writes for  samtools view -h  of the file.  The input\n"
    "  is BGZF as samtools writes it, any other gzip file of the same bytes, or inflated BAM.\n\n"
    "  Columns: RNAME, POS-1, stop, QNAME, FLAG, strand (- when FLAG has bit 16, else +), MAPQ, then\n"
    "  CIGAR, RNEXT, PNEXT, TLEN, SEQ, QUAL and the tags as SAM text.  stop = POS-1 + max(1, the sum\n"
    "  of the counts of the CIGAR operations M D N = X); no operators give one base.\n\n"
    "  --output=bed      BED text (the default)\n"
    "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
    "  --do-not-sort     leave the lines in input order\n"
    "  --keep-header     line K (from 0) of the header text becomes\n"
    "                    _header TAB K TAB K+1 TAB line ; by default the header is dropped\n"
    "  --split           one line per maximal run of M D = X operations with a positive length; N\n"
    "                    ends a run; I S H P consume nothing; a record without a run keeps its line\n"
    "  --split-with-deletions\n"
    "                    --split, and D ends a run too and belongs to none\n"
    "  --all-reads       a record with FLAG bit 4 becomes  _unmapped TAB 0 TAB 1  and its columns; by\n"
    "                    default unmapped records are dropped\n"
    "  --reduced         the first six columns only\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Not supported: --max-mem, --sort-tmpdir, --zero-indexed, --do-not-split.\n\n"
    "  The SAM text of a record follows the SAM specification (section 4.2); the BED follows sam2bed,\n"
    "  with its known or possible differences from BEDOPS.  Believed, but unverified against samtools\n"
    "  or BEDOPS (*):\n"
    "    An f tag is C's %g of the float32, computed exactly; infinities and NaNs print inf, -inf\n"
    "    and nan (a NaN of either sign).\n"
    "    A TAB, a newline or a NUL inside a read name or a tag value is copied, not escaped.\n"
    "    A mapped record whose reference name is empty or * is refused, as sam2bed refuses its text.\n"
    "    With n_cigar_op = 2, a first operator <l_seq>S, a second N and a CG:B:I tag, the first such\n"
    "    tag's array is the CIGAR and the tag is not printed.\n\n"
    "  A record that does not fit the format is reported with its number (from 1) and nothing is\n"
    "  written.\n";

int main(int argc, char** argv)
{
    const align_cli::Command cmd = {"bam2bed", 0, align_cli::TAKES_SPLIT | align_cli::TAKES_SAM, kHelp};
    starch_bam_options opt;
    memset(&opt, 0, sizeof opt);
    return align_cli::run_with(cmd, opt, starch_bam_host, starch_bam_encode_host, argc, argv);
}
