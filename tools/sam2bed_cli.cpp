// tools/sam2bed_cli.cpp -- the `sam2bed` command: SAM text to BED on the GPU
// (tools/align2bed_cli.hpp has the command line and the exit codes).
#include "align2bed_cli.hpp"

static const char* kHelp =
    "USAGE: sam2bed [--output=bed|starch] [--do-not-sort] [--keep-header] [--split] [--split-with-deletions]\n"
    "               [--all-reads] [--reduced] [--device N] [file | -]\n\n"
    "  SAM text (no file, or -: stdin; for BAM pipe in  samtools view -h ) is converted to BED on\n"
    "  the GPU and written to stdout, in sort-bed's order unless --do-not-sort is given.  Lines end\n"
    "  at a newline; a carriage return is an ordinary byte.\n\n"
    "  Columns: RNAME, POS-1, stop, QNAME, FLAG, strand (- when FLAG has bit 16, else +), MAPQ, then\n"
    "  CIGAR and every column after it unchanged.  stop = POS-1 + max(1, the sum of the counts of\n"
    "  the CIGAR operations M D N = X); a CIGAR of * gives one base.\n\n"
    "  --output=bed      BED text (the default)\n"
    "  --output=starch   the archive starch3 writes for the sorted BED; not with --do-not-sort\n"
    "  --do-not-sort     leave the lines in input order\n"
    "  --keep-header     header line K (from 0: an empty line, an @ line) becomes\n"
    "                    _header TAB K TAB K+1 TAB line ; by default header lines are dropped\n"
    "  --split           one line per maximal run of M D = X operations with a positive length; N\n"
    "                    ends a run; I S H P consume nothing; a record without a run keeps its line\n"
    "  --split-with-deletions\n"
    "                    --split, and D ends a run too and belongs to none\n"
    "  --all-reads       a record with FLAG bit 4 becomes  _unmapped TAB 0 TAB 1  and its columns; by\n"
    "                    default unmapped records are dropped\n"
    "  --reduced         the first six columns only\n"
    "  --device N        GPU to compute on (default 0)\n"
    "  --help, --version\n\n"
    "  Not supported: BAM input, --max-mem, --sort-tmpdir, --zero-indexed, --do-not-split.\n\n"
    "  The definitions are modelled on BEDOPS' convert2bed (its sam2bed), but they are unverified\n"
    "  against a BEDOPS binary.  Known or possible differences:\n"
    "    A record needs its first six fields; what follows CIGAR is copied byte for byte and is\n"
    "    neither counted nor checked, where BEDOPS needs eleven fields.\n"
    "    --split keeps the whole CIGAR and the plain QNAME on every line; BEDOPS may write a\n"
    "    per-piece name.\n\n"
    "  A line that does not fit the format is reported with its line number (from 1) and nothing\n"
    "  is written.\n";

int main(int argc, char** argv)
{
    const align_cli::Command cmd = {"sam2bed", STARCH_ALIGN_SAM, align_cli::TAKES_SPLIT | align_cli::TAKES_SAM, kHelp};
    return align_cli::run(cmd, argc, argv);
}
