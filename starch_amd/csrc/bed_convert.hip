// starch_amd/csrc/bed_convert.hip -- convert2bed on MI355X: GFF3, GTF, VCF and
// WIG text into BED lines (the definitions: include/starch_amd.h).
//
// Stages (per-line arrays are struct-of-arrays, indexed by input line):
//   1. framing: the sort's line-end pass (sb::SortWorkspace::stage_frame).
//   2. k_cv_classify<format>, one thread per line: the line's class, the
//      offsets of the fields it needs (relative to the line, 32 bits), its
//      parsed coordinates, its number of output lines and their bytes.  The
//      walk over a line stops after the last field it needs: a VCF line is
//      read up to the start of INFO, a WIG line up to its fifth token; GFF and
//      GTF attributes are read to their end (the ID may stand anywhere, and a
//      tenth field is an error).  The lowest bad line is an atomicMin of
//      (line << 8) | kind, the first ##FASTA line of GFF an atomicMin too:
//      lines from it on are cut off before anything else looks at them.
//   3. WIG state.  k_cv_wig_decl parses the rare declaration lines in a launch
//      of its own (the data lines leave it at once), into the declaration
//      line's own slots.  One exclusive sum over (is data line) + (is 1-token
//      line) << 32 gives every line N and, against the sum at its declaration,
//      k; an inclusive running maximum of (line + 1 if it is a declaration)
//      gives every data line its declaration.  k_cv_wig_resolve then computes
//      the coordinates and bytes of the data lines.
//   4. br::place (k_br_tally): class counts, and with keep_header the bytes of
//      the header lines from the exclusive sum of (is header).  An exclusive sum
//      of the bytes places every line; k_cv_write<format>, one thread per input
//      line, writes its output lines (several in the VCF split modes, round
//      after round across the wave).  A copied tail (attributes, INFO and sample
//      columns, a kept header line) of sb::kWaveCopyBytes or more is left to
//      the whole wave, as in k_bm_write.
// The skeleton (arrays, scalars, the end of classify, tally, the host steps) is
// bed_records.hpp's.  All arithmetic is unsigned 64-bit integer.
#include <algorithm>

#include "bed_convert.hpp"

namespace cv {
namespace {

using br::S_BAD, br::S_MARK, br::S_OWN, br::S_HDR, br::S_REC, br::S_LINES, br::S_BYTES, br::C_BAD, br::C_HEADER, br::C_TOOL;
using br::K_LONG, br::K_ZERO, br::K_OVER, br::K_END, br::K_STOP, br::K_TOOL;
using br::dec_digits, br::is_blank, br::is_word, br::line_beg, br::Writer, br::parse_coord, br::token_is, br::tokens;
using br::drop_bad, br::store_line, br::header_line, br::reset_and_bind, br::first_of, br::First, br::throw_bad, br::place, br::Placed;
using bt::kLimit;
enum : int { S_FASTA = S_MARK, S_DECL = S_OWN };   // the first ##FASTA line of GFF; the WIG declarations
enum : uint8_t { C_REC = C_TOOL, C_DECL, C_DATA1, C_DATA2, C_DATA4 };
enum : uint32_t {
    K_FEW = K_TOOL, K_MANY, K_NONAME, K_REF, K_ALT, K_ALLELE, K_TOKENS, K_NODECL, K_MISFIT, K_KEY, K_TWICE, K_NOCHROM, K_NOSTART,
    K_VALUE
};
// slots of a line (Rec::fo).  GFF, GTF: the starts of fields 1 to 8, then the
// ID's offset and length (0: none).  VCF: the starts of fields 1 to 7.  A WIG
// data line: chromosome token [0, 1), score token [2, 3), its declaration's
// line [4].  A WIG declaration: chromosome value [0, 1), mode [2] (0: bad).
enum : uint32_t { O_ID = 8, O_IDLEN = 9, O_CHR = 0, O_CHREND = 1, O_SCORE = 2, O_SCOREEND = 3, O_DECL = 4, O_MODE = 2 };
enum : uint32_t { M_VARIABLE = 1, M_FIXED = 2 };

struct Rec : br::Rec {     // a and b of a declaration: its start and step
    uint64_t* aux;         // WIG: a declaration's span
    uint64_t* pk;          // WIG: (is data line) | (is 1-token line) << 32, then its exclusive sum
    uint64_t* dmax;        // WIG: line + 1 of a declaration, then its running maximum
    uint32_t vcf_class;
};

struct Tally {             // what k_br_tally counts
    static constexpr uint32_t kOwn = C_DECL;
    static __device__ bool record(uint32_t c) { return c == C_REC || c == C_DATA1 || c == C_DATA2 || c == C_DATA4; }
};

// ---- 2. classify and measure ---------------------------------------------------------
struct Line : br::Line<kSlots> {   // what k_cv_classify leaves of a line
    uint64_t pk = 0;
};

// a GFF (gtf == false) or GTF record s[0, n)
template <bool kGtf>
__device__ __forceinline__ void annotation_line(const uint8_t* __restrict__ s, uint32_t n, Line& ln)
{
    uint32_t nf = 1, p = 0;
    for (; p < n && nf < 9; ++p)
        if (s[p] == '\t') ln.fo[nf++ - 1] = p + 1;
    if (nf < 9) { ln.kind = K_FEW; return; }
    // the attributes s[p, n): no further TAB, and the ID
    const uint32_t a0 = p;
    bool many = false;
    uint32_t ido = 0, idl = 0;
    if (kGtf) {
        int state = 0;   // 1: inside the first gene_id "...", 2: past it
        for (; p < n; ++p) {
            const uint8_t c = s[p];
            if (c == '\t') { many = true; break; }
            if (state == 0 && c == 'g' && p + 9 <= n && (p == a0 || s[p - 1] == ';' || s[p - 1] == ' ') && is_word(s + p, "gene_id \"", 9)) {
                state = 1;
                ido = p + 9;
            } else if (state == 1 && p >= ido && c == '"') {
                state = 2;
                idl = p - ido;
            }
        }
    } else {
        bool found = false;
        uint32_t ps = a0;   // where the piece begins
        for (; p <= n; ++p) {
            if (p < n && s[p] == '\t') { many = true; break; }
            if (p == n || s[p] == ';') {
                if (!found && p - ps >= 3 && s[ps] == 'I' && s[ps + 1] == 'D' && s[ps + 2] == '=') {
                    found = true;
                    ido = ps + 3;
                    idl = p - ido;
                }
                ps = p + 1;
            }
        }
    }
    if (many) { ln.kind = K_MANY; return; }
    if (ln.fo[0] == 1) { ln.kind = K_NONAME; return; }
    uint64_t start = 0, end = 0;
    if ((ln.kind = parse_coord(s, ln.fo[2], ln.fo[3] - 1, &start))) return;
    if ((ln.kind = parse_coord(s, ln.fo[3], ln.fo[4] - 1, &end))) return;
    if (start < 1) { ln.kind = K_ZERO; return; }
    if (end < start) { ln.kind = K_END; return; }
    ln.cls = C_REC;
    ln.a = start - 1;
    ln.b = end;
    ln.fo[O_ID] = ido;
    ln.fo[O_IDLEN] = idl;
    ln.cnt = 1;
    // ten columns for nine: start and end (fo[4] - 2 - fo[2] bytes) are written anew, the ID and its TAB are new
    ln.ob = (uint64_t)n + 2 - (ln.fo[4] - 2 - ln.fo[2]) + dec_digits(ln.a) + dec_digits(ln.b) + (idl ? idl : 1);
}

// allele s[b, e) of a REF of ref bytes is of class c (STARCH_VCF_SNVS, ...)
__device__ __forceinline__ bool allele_is(uint32_t c, uint32_t len, uint32_t ref)
{
    return c == STARCH_VCF_SNVS ? len == ref : (c == STARCH_VCF_INSERTIONS ? len > ref : len < ref);
}

__device__ __forceinline__ void vcf_line(const uint8_t* __restrict__ s, uint32_t n, uint32_t vclass, Line& ln)
{
    uint32_t nf = 1, p = 0;
    for (; p < n && nf < 8; ++p)   // stops at the start of INFO
        if (s[p] == '\t') ln.fo[nf++ - 1] = p + 1;
    if (nf < 8) { ln.kind = K_FEW; return; }
    if (ln.fo[0] == 1) { ln.kind = K_NONAME; return; }
    uint64_t pos = 0;
    if ((ln.kind = parse_coord(s, ln.fo[0], ln.fo[1] - 1, &pos))) return;
    if (pos < 1) { ln.kind = K_ZERO; return; }
    const uint32_t ref = ln.fo[3] - 1 - ln.fo[2], alt0 = ln.fo[3], alt1 = ln.fo[4] - 1;
    if (ref == 0) { ln.kind = K_REF; return; }
    if (alt0 == alt1) { ln.kind = K_ALT; return; }
    uint32_t cnt = 1;
    uint64_t alleles = alt1 - alt0;   // the bytes of the ALT columns written
    if (vclass != STARCH_VCF_ALL) {
        cnt = 0;
        alleles = 0;
        bool empty = false;
        for (uint32_t as = alt0, q = alt0; q <= alt1; ++q)
            if (q == alt1 || s[q] == ',') {
                const uint32_t al = q - as;
                if (al == 0) empty = true;
                else if (allele_is(vclass, al, ref)) { ++cnt; alleles += al; }
                as = q + 1;
            }
        if (empty) { ln.kind = K_ALLELE; return; }
    }
    const uint64_t start = pos - 1, stop = start + ref;
    if (stop > kLimit) { ln.kind = K_OVER; return; }
    ln.cls = C_REC;
    ln.a = start;
    ln.b = stop;
    ln.cnt = cnt;
    // CHROM start stop ID QUAL REF <ALT> FILTER INFO...: all of the line but POS and ALT, one TAB more, '\n'
    const uint64_t fixed = (uint64_t)n - (ln.fo[1] - 1 - ln.fo[0]) - (alt1 - alt0) + dec_digits(start) + dec_digits(stop) + 2;
    ln.ob = cnt * fixed + alleles;
}

__device__ __forceinline__ void wig_line(const uint8_t* __restrict__ s, uint32_t n, Line& ln)
{
    uint32_t ts[4], te[4];
    const uint32_t nt = tokens(s, n, ts, te);   // 5: more than four
    if (nt && (token_is(s, ts[0], te[0], "track", 5) || token_is(s, ts[0], te[0], "browser", 7))) { ln.cls = C_HEADER; return; }
    if (nt && (token_is(s, ts[0], te[0], "variableStep", 12) || token_is(s, ts[0], te[0], "fixedStep", 9))) { ln.cls = C_DECL; return; }
    if (nt != 1 && nt != 2 && nt != 4) { ln.kind = K_TOKENS; return; }
    const uint32_t sc = nt - 1;   // the score is the last token
    if (nt == 4) {
        if ((ln.kind = parse_coord(s, ts[1], te[1], &ln.a))) return;
        if ((ln.kind = parse_coord(s, ts[2], te[2], &ln.b))) return;
        if (ln.b <= ln.a) { ln.kind = K_STOP; return; }
        ln.fo[O_CHR] = ts[0];
        ln.fo[O_CHREND] = te[0];
        ln.cls = C_DATA4;
    } else if (nt == 2) {
        if ((ln.kind = parse_coord(s, ts[0], te[0], &ln.a))) return;
        if (ln.a < 1) { ln.kind = K_ZERO; return; }
        ln.cls = C_DATA2;
    } else {
        ln.cls = C_DATA1;
    }
    ln.fo[O_SCORE] = ts[sc];
    ln.fo[O_SCOREEND] = te[sc];
    ln.pk = 1ull | (nt == 1 ? 1ull << 32 : 0ull);
}

template <int kFormat>
__global__ void __launch_bounds__(kThreads) k_cv_classify(const Rec r)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.L) return;
    const uint64_t b = line_beg(r.line_end, i), e = r.line_end[i] - 1;
    const uint8_t* s = r.in + b;
    Line ln;
    if (e - b >= 0xffffffffull) ln.kind = K_LONG;
    else if (e == b || s[0] == '#') {
        ln.cls = C_HEADER;
        if (kFormat == STARCH_CONVERT_GFF && e - b == 7 && is_word(s, "##FASTA", 7)) atomicMin(&r.scal[S_FASTA], (unsigned long long)i);
    }
    else if (kFormat == STARCH_CONVERT_WIG) wig_line(s, (uint32_t)(e - b), ln);
    else if (kFormat == STARCH_CONVERT_VCF) vcf_line(s, (uint32_t)(e - b), r.vcf_class, ln);
    else annotation_line<kFormat == STARCH_CONVERT_GTF>(s, (uint32_t)(e - b), ln);
    drop_bad(r, i, ln);   // (two calls on purpose: merged into one function the kernel is other code, bed_records.hpp)
    store_line<kSlots>(r, i, ln);
    if (kFormat == STARCH_CONVERT_WIG) {
        r.pk[i] = ln.pk;
        r.dmax[i] = ln.cls == C_DECL ? i + 1 : 0;
    }
}

// ---- 3. WIG state -----------------------------------------------------------------------
// the value s[b, e) of start, step or span: 1 to 2^63-1
__device__ __forceinline__ bool decl_value(const uint8_t* __restrict__ s, uint32_t b, uint32_t e, uint64_t* v)
{
    return parse_coord(s, b, e, v) == 0 && *v >= 1;
}

// every declaration line into its record: fo[O_CHR], fo[O_CHREND], fo[O_MODE], a (start), b (step), aux (span)
__global__ void __launch_bounds__(kThreads) k_cv_wig_decl(const Rec r)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.L || r.cls[i] != C_DECL) return;
    const uint64_t b = line_beg(r.line_end, i);
    const uint8_t* s = r.in + b;
    const uint32_t n = (uint32_t)(r.line_end[i] - 1 - b);
    uint32_t p = 0;
    while (is_blank(s[p])) ++p;   // the line has a first token
    const bool fixed = s[p] == 'f';
    while (p < n && !is_blank(s[p])) ++p;
    enum : uint32_t { CHROM = 1, START = 2, STEP = 4, SPAN = 8 };
    uint32_t seen = 0, kind = 0, c0 = 0, c1 = 0;
    uint64_t start = 0, step = 1, span = 1;
    while (!kind) {
        while (p < n && is_blank(s[p])) ++p;
        if (p == n) break;
        const uint32_t t0 = p;
        while (p < n && !is_blank(s[p])) ++p;
        uint32_t eq = t0;
        while (eq < p && s[eq] != '=') ++eq;
        uint32_t key = 0;
        if (eq < p) {
            if (token_is(s, t0, eq, "chrom", 5)) key = CHROM;
            else if (token_is(s, t0, eq, "span", 4)) key = SPAN;
            else if (fixed && token_is(s, t0, eq, "start", 5)) key = START;
            else if (fixed && token_is(s, t0, eq, "step", 4)) key = STEP;
        }
        if (!key) kind = K_KEY;
        else if (seen & key) kind = K_TWICE;
        else if (key == CHROM) {
            c0 = eq + 1;
            c1 = p;
            if (c0 == c1) kind = K_NOCHROM;
        } else if (!decl_value(s, eq + 1, p, key == START ? &start : (key == STEP ? &step : &span))) kind = K_VALUE;
        seen |= key;
    }
    if (!kind && !(seen & CHROM)) kind = K_NOCHROM;
    if (!kind && fixed && !(seen & START)) kind = K_NOSTART;
    if (kind) atomicMin(&r.scal[S_BAD], (unsigned long long)((i << 8) | kind));
    r.fo[(uint64_t)O_CHR * r.L + i] = c0;
    r.fo[(uint64_t)O_CHREND * r.L + i] = c1;
    r.fo[(uint64_t)O_MODE * r.L + i] = kind ? 0u : (fixed ? M_FIXED : M_VARIABLE);
    r.a[i] = start;
    r.b[i] = step;
    r.aux[i] = span;
}

// coordinates and bytes of the data lines; pk and dmax hold their scans
__global__ void __launch_bounds__(kThreads) k_cv_wig_resolve(const Rec r)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.L) return;
    const uint32_t cls = r.cls[i];
    if (cls != C_DATA1 && cls != C_DATA2 && cls != C_DATA4) return;
    const uint64_t pk = r.pk[i];
    uint64_t start = r.a[i], stop = r.b[i];
    uint32_t kind = 0, chrom = r.fo[(uint64_t)O_CHREND * r.L + i] - r.fo[(uint64_t)O_CHR * r.L + i];
    if (cls != C_DATA4) {
        const uint64_t d = r.dmax[i];
        const uint32_t mode = d ? r.fo[(uint64_t)O_MODE * r.L + (d - 1)] : 0u;
        if (d == 0) kind = K_NODECL;
        else if (mode != (cls == C_DATA1 ? M_FIXED : M_VARIABLE)) kind = K_MISFIT;   // (a bad declaration is reported on its own line)
        else {
            const uint64_t dl = d - 1, span = r.aux[dl];
            if (cls == C_DATA2) start -= 1;
            else {
                const uint64_t k = (pk >> 32) - (r.pk[dl] >> 32), step = r.b[dl];
                const uint64_t prod = k * step;
                start = r.a[dl] - 1 + prod;
                if (__umul64hi(k, step) || prod > kLimit || start > kLimit) kind = K_OVER;
            }
            stop = start + span;   // both below 2^63
            if (!kind && stop > kLimit) kind = K_OVER;
            chrom = r.fo[(uint64_t)O_CHREND * r.L + dl] - r.fo[(uint64_t)O_CHR * r.L + dl];
            r.fo[(uint64_t)O_DECL * r.L + i] = (uint32_t)dl;
        }
    }
    if (kind) {
        atomicMin(&r.scal[S_BAD], (unsigned long long)((i << 8) | kind));
        return;   // cnt and ob stay 0
    }
    const uint32_t score = r.fo[(uint64_t)O_SCOREEND * r.L + i] - r.fo[(uint64_t)O_SCORE * r.L + i];
    r.a[i] = start;
    r.b[i] = stop;
    r.cnt[i] = 1;
    // chrom start stop id-N score
    r.ob[i] = (uint64_t)chrom + dec_digits(start) + dec_digits(stop) + 3 + dec_digits((pk & 0xffffffffull) + 1) + score + 5;
}

// ---- 4. output ---------------------------------------------------------------------------
// A thread writes the output lines of its input line, one per round; a tail of
// kWaveCopyBytes or more is left to the whole wave, line after line.
template <int kFormat>
__global__ void __launch_bounds__(kThreads)
k_cv_write(const Rec r, uint64_t Le, const uint64_t* __restrict__ hord, const uint64_t* __restrict__ off, uint64_t out_bytes,
           uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < Le;
    uint32_t nout = valid ? r.cnt[i] : 0u;
    if (nout && off[i] + r.ob[i] > out_bytes) nout = 0;
    const uint64_t b = valid ? line_beg(r.line_end, i) : 0;
    const uint8_t* s = r.in + b;
    const uint32_t n = valid ? (uint32_t)(r.line_end[i] - 1 - b) : 0u;
    const uint32_t cls = nout ? r.cls[i] : (uint32_t)C_BAD;
    uint32_t f[kSlots + 1];   // f[k]: where field k starts (GFF, GTF, VCF), or slot k - 1
    f[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSlots; ++k) f[k + 1] = nout ? r.fo[(uint64_t)k * r.L + i] : 0u;
    Writer<> w{out, nout ? off[i] : 0};
    uint32_t ap = f[4];       // VCF: where the next allele begins
    for (uint32_t round = 0; __ballot(round < nout) != 0; ++round) {
        w.big_len[0] = 0;
        if (round < nout) {
            if (cls == C_HEADER) {
                header_line(w, hord[i], s, n);
            } else if (kFormat == STARCH_CONVERT_WIG) {
                const uint64_t from = cls == C_DATA4 ? i : (uint64_t)f[O_DECL + 1];   // the line that names the chromosome
                const uint8_t* c = r.in + line_beg(r.line_end, from);
                w.bytes(c + r.fo[(uint64_t)O_CHR * r.L + from], r.fo[(uint64_t)O_CHREND * r.L + from] - r.fo[(uint64_t)O_CHR * r.L + from]);
                w.tab();
                w.dec(r.a[i]);
                w.tab();
                w.dec(r.b[i]);
                w.bytes(reinterpret_cast<const uint8_t*>("\tid-"), 4);
                w.dec((r.pk[i] & 0xffffffffull) + 1);
                w.tab();
                w.tail(s + f[O_SCORE + 1], f[O_SCOREEND + 1] - f[O_SCORE + 1]);
            } else if (kFormat == STARCH_CONVERT_VCF) {
                uint32_t as = f[4], ae = f[5] - 1;   // the ALT column of this line
                if (r.vcf_class != STARCH_VCF_ALL) {
                    const uint32_t ref = f[4] - 1 - f[3];
                    for (;;) {   // the next allele of the class: cnt of them are there
                        as = ap;
                        ae = as;
                        while (ae < f[5] - 1 && s[ae] != ',') ++ae;
                        ap = ae + 1;
                        if (allele_is(r.vcf_class, ae - as, ref) || ap > f[5] - 1) break;
                    }
                }
                w.bytes(s, f[1] - 1);
                w.tab();
                w.dec(r.a[i]);
                w.tab();
                w.dec(r.b[i]);
                w.tab();
                w.bytes(s + f[2], f[3] - f[2]);   // ID and its TAB
                w.bytes(s + f[5], f[6] - f[5]);   // QUAL
                w.bytes(s + f[3], f[4] - f[3]);   // REF
                w.bytes(s + as, ae - as);
                w.tab();
                w.bytes(s + f[6], f[7] - f[6]);   // FILTER
                w.tail(s + f[7], n - f[7]);       // INFO and every column after it
            } else {
                w.bytes(s, f[1] - 1);
                w.tab();
                w.dec(r.a[i]);
                w.tab();
                w.dec(r.b[i]);
                w.tab();
                if (f[O_IDLEN + 1]) w.bytes(s + f[O_ID + 1], f[O_IDLEN + 1]);
                else w.out[w.o++] = '.';
                w.tab();
                w.bytes(s + f[5], f[7] - f[5]);   // score, strand and their TABs
                w.bytes(s + f[1], f[3] - f[1]);   // source, type
                w.bytes(s + f[7], f[8] - f[7]);   // phase
                w.tail(s + f[8], n - f[8]);       // attributes
            }
        }
        bt::wave_copy_tails(w, out, lane);
    }
}

template <int kFormat>
void launch_format(const Rec& r, uint64_t Le, const uint64_t* hord, const uint64_t* off, uint64_t bytes, uint8_t* o, bool write,
                   hipStream_t st)
{
    if (write)
        hipLaunchKernelGGL(k_cv_write<kFormat>, dim3(blocks_for(Le, kThreads)), dim3(kThreads), 0, st, r, Le, hord, off, bytes, o);
    else
        hipLaunchKernelGGL(k_cv_classify<kFormat>, dim3(blocks_for(r.L, kThreads)), dim3(kThreads), 0, st, r);
}

void launch(uint32_t format, const Rec& r, uint64_t Le, const uint64_t* hord, const uint64_t* off, uint64_t bytes, uint8_t* o,
            bool write, hipStream_t st)
{
    switch (format) {
        case STARCH_CONVERT_GFF: launch_format<STARCH_CONVERT_GFF>(r, Le, hord, off, bytes, o, write, st); break;
        case STARCH_CONVERT_GTF: launch_format<STARCH_CONVERT_GTF>(r, Le, hord, off, bytes, o, write, st); break;
        case STARCH_CONVERT_VCF: launch_format<STARCH_CONVERT_VCF>(r, Le, hord, off, bytes, o, write, st); break;
        default: launch_format<STARCH_CONVERT_WIG>(r, Le, hord, off, bytes, o, write, st); break;
    }
    HIP_CHECK(hipGetLastError());
}

const char* bad_text(uint32_t k)
{
    switch (k) {
        case K_FEW: return "fewer tab-separated fields than the format needs";
        case K_MANY: return "more than nine tab-separated fields";
        case K_NONAME: return "empty sequence name";
        case K_REF: return "empty REF";
        case K_ALT: return "empty ALT";
        case K_ALLELE: return "empty ALT allele";
        case K_TOKENS: return "a data line has 1, 2 or 4 tokens";
        case K_NODECL: return "data line before any declaration";
        case K_MISFIT: return "data line does not fit the declaration in force";
        case K_KEY: return "unknown key in a declaration";
        case K_TWICE: return "repeated key in a declaration";
        case K_NOCHROM: return "declaration without chrom";
        case K_NOSTART: return "fixedStep declaration without start";
        case K_VALUE: return "declaration value is not a number from 1 to 2^63-1";
        default: return br::bad_text(k);
    }
}

}  // namespace

void ConvertWorkspace::run(sb::SortWorkspace& sorter, const ConvertOptions& opt, const uint8_t* d_in, uint64_t n, hipStream_t st,
                           DevBuf& out, ConvertResult& res)
{
    res = ConvertResult{};
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) { timer.finish(from, st, {&res.ms_frame, &res.ms_parse, &res.ms_write}); };
    if (n == 0) return finish(1);

    // 1. framing
    const uint64_t L = sorter.stage_frame(d_in, n, st);
    res.n_lines = L;
    timer.mark(1, st);

    // 2. classify and measure
    const bool wig = opt.format == STARCH_CONVERT_WIG;
    Rec r{};
    reset_and_bind(rb, r, d_in, sorter.ln.line_end, L, kSlots, st);
    if (wig) {
        r.aux = b_aux.as<uint64_t>(L);
        r.pk = b_pk.as<uint64_t>(L);
        r.dmax = b_dmax.as<uint64_t>(L);
    }
    r.vcf_class = opt.vcf_class;
    r.keep_header = opt.keep_header;
    const unsigned lblocks = blocks_for(L, kThreads);
    launch(opt.format, r, L, nullptr, nullptr, 0, nullptr, false, st);

    // 3. WIG state
    if (wig) {
        hipLaunchKernelGGL(k_cv_wig_decl, dim3(lblocks), dim3(kThreads), 0, st, r);
        scan::excl_sum_u64(r.pk, r.pk, L, (uint64_t*)nullptr, rb.tmp, st);
        scan::incl_max_u64(r.dmax, L, rb.tmp, st);
        hipLaunchKernelGGL(k_cv_wig_resolve, dim3(lblocks), dim3(kThreads), 0, st, r);
        HIP_CHECK(hipGetLastError());
    }
    const First first = first_of(rb, st);
    const uint64_t Le = std::min(L, first.mark);   // the lines before ##FASTA
    if (first.bad != ~0ull && (first.bad >> 8) < Le) throw_bad("convert2bed", first.bad, bad_text);

    // 4. header ordinals, counts, places
    const Placed p = place<Tally>(rb, r, Le, "convert2bed", st);
    res.header_lines = p.tot[S_HDR];
    res.data_lines = p.tot[S_REC];
    res.declarations = p.tot[S_DECL];
    timer.mark(2, st);
    const uint64_t bytes = p.tot[S_BYTES];
    if (bytes) {
        uint8_t* o = out.as<uint8_t>(bytes + 64);
        launch(opt.format, r, Le, p.hord, p.off, bytes, o, true, st);
    }
    res.lines_out = p.tot[S_LINES];
    res.out_bytes = bytes;
    finish(3);
}

}  // namespace cv
