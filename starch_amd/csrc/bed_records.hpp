// starch_amd/csrc/bed_records.hpp -- the skeleton of a converter that turns text
// into BED line by line (bed_convert.hip, bed_align.hip):
// the per-line arrays and device scalars, what a classify kernel leaves of a
// line, the tally of classes and kept header lines, the kept header line as it
// is written, and the host steps between a tool's own launches.  A
// format's parsers, its walks and its write kernel stay in the tool's file (the
// write kernels' prologue and round loop too: section 19).
#pragma once
#include <string>

#include "../../include/starch_amd.h"
#include "bed_text.hpp"

namespace br {

constexpr int kThreads = 256;           // threads per block of the per-line kernels (one line each)

// device scalars (u64).  S_BAD: the lowest bad line as (line << 8) | kind;
// S_MARK: a line the tool looks for (GFF's ##FASTA, PSL's dashes); both start as
// all ones.  S_FLAG and S_OWN (the count of Tally::kOwn) are the tool's.
enum : int { S_BAD = 0, S_MARK, S_FLAG, S_HDR, S_REC, S_OWN, S_LINES, S_BYTES, S_COUNT = 8 };
enum : uint8_t { C_BAD = 0, C_HEADER, C_TOOL };          // a tool's classes start at C_TOOL
enum : uint32_t { K_LONG = 1, K_EMPTY, K_DIGIT, K_RANGE, K_ZERO, K_OVER, K_END, K_STOP, K_TOOL };   // its kinds at K_TOOL

inline const char* bad_text(uint32_t k)
{
    switch (k) {
        case K_LONG: return "line of 2^32 bytes or more";
        case K_EMPTY: return "empty coordinate";
        case K_DIGIT: return "non-digit in a coordinate";
        case K_RANGE: return "coordinate has 20 or more digits or is above 2^63-1";
        case K_ZERO: return "start or position below 1";
        case K_OVER: return "coordinate would exceed 2^63-1";
        case K_END: return "end below start";
        case K_STOP: return "stop not above start";
        default: return "malformed line";
    }
}

struct Rec {               // per-line arrays, indexed by input line; a tool's Rec derives from it
    const uint8_t* in;
    const uint64_t* line_end;
    uint64_t L;
    uint8_t* cls;
    uint32_t* fo;          // slots x L: 32-bit values of a line, the tool says which
    uint64_t *a, *b;       // output start and stop
    uint32_t* cnt;         // output lines
    uint64_t* ob;          // their bytes
    uint32_t* hflag;       // 1: a header line
    unsigned long long* scal;
    uint32_t keep_header;
};

using bt::dec_digits;
using bt::is_blank;
using bt::is_word;
using bt::line_beg;
using bt::Writer;

// decimal field s[b, e): 0, or K_EMPTY, K_DIGIT, K_RANGE (20 digits or more, or above 2^63-1)
__device__ __forceinline__ uint32_t parse_coord(const uint8_t* __restrict__ s, uint32_t b, uint32_t e, uint64_t* v)
{
    return bt::parse_coord<K_EMPTY, K_DIGIT, K_RANGE>(s, b, e, v);
}

__device__ __forceinline__ bool token_is(const uint8_t* __restrict__ s, uint32_t b, uint32_t e, const char* w, uint32_t k)
{
    return e - b == k && is_word(s + b, w, k);
}

// The first kMax tokens of s[0, n), separated by runs of blanks: [ts[k], te[k]),
// empty past the last one.  Returns their number, kMax + 1 for more.  Unrolled,
// so that the bounds stay in registers.
template <uint32_t kMax>
__device__ __forceinline__ uint32_t tokens(const uint8_t* __restrict__ s, uint32_t n, uint32_t (&ts)[kMax], uint32_t (&te)[kMax])
{
    uint32_t p = 0, nt = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMax; ++k) {
        while (p < n && is_blank(s[p])) ++p;
        ts[k] = p;
        while (p < n && !is_blank(s[p])) ++p;
        te[k] = p;
        if (te[k] > ts[k]) nt = k + 1;
    }
    while (p < n && is_blank(s[p])) ++p;
    return p < n ? kMax + 1 : nt;
}

// ---- classify ---------------------------------------------------------------------------
template <uint32_t kSlots>
struct Line {              // what a classify kernel leaves of a line
    uint32_t cls = C_BAD, kind = 0, cnt = 0;
    uint64_t ob = 0, a = 0, b = 0;
    uint32_t fo[kSlots] = {};
};

// The end of a classify kernel, in two calls: a bad line (ln.kind) enters the
// atomicMin of S_BAD and leaves nothing else; then ln goes into the arrays,
// kSlots of its slots.  (Two functions that the kernel calls one after the
// other: as one function k_cv_classify is other code)
template <class LineT>
__device__ __forceinline__ void drop_bad(const Rec& r, uint64_t i, LineT& ln)
{
    if (ln.kind) {
        atomicMin(&r.scal[S_BAD], (unsigned long long)((i << 8) | ln.kind));
        ln = LineT{};
    }
}

template <uint32_t kSlots, class LineT>
__device__ __forceinline__ void store_line(const Rec& r, uint64_t i, const LineT& ln)
{
    r.cls[i] = (uint8_t)ln.cls;
    r.hflag[i] = ln.cls == C_HEADER ? 1u : 0u;
    r.cnt[i] = ln.cnt;
    r.ob[i] = ln.ob;
    r.a[i] = ln.a;
    r.b[i] = ln.b;
#pragma unroll
    for (uint32_t k = 0; k < kSlots; ++k) r.fo[(uint64_t)k * r.L + i] = ln.fo[k];
}

// ---- tally ------------------------------------------------------------------------------
// Class counts and output lines of the lines [0, Le); the bytes of a kept header
// line.  Tally::record(cls): the class counts as a record; Tally::kOwn: the class
// counted in S_OWN.
template <class Tally>
__global__ void __launch_bounds__(kThreads) k_br_tally(const Rec r, uint64_t Le, const uint64_t* __restrict__ hord)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool valid = i < Le;
    const uint32_t cls = valid ? r.cls[i] : (uint32_t)C_BAD;
    uint32_t cnt = valid ? r.cnt[i] : 0u;
    if (cls == C_HEADER && r.keep_header) {
        const uint64_t k = hord[i];
        cnt = 1;
        r.cnt[i] = 1;
        // _header K K+1 line
        r.ob[i] = 8 + dec_digits(k) + 1 + dec_digits(k + 1) + 1 + (r.line_end[i] - 1 - line_beg(r.line_end, i)) + 1;
    }
    const uint32_t hdr = __popcll(__ballot(cls == C_HEADER)), own = __popcll(__ballot(cls == Tally::kOwn));
    const uint32_t rec = __popcll(__ballot(Tally::record(cls)));
    const uint32_t lines = wave_reduce_add<uint32_t>(cnt);
    if ((threadIdx.x & 63) == 0) {
        if (hdr) atomicAdd(&r.scal[S_HDR], (unsigned long long)hdr);
        if (own) atomicAdd(&r.scal[S_OWN], (unsigned long long)own);
        if (rec) atomicAdd(&r.scal[S_REC], (unsigned long long)rec);
        if (lines) atomicAdd(&r.scal[S_LINES], (unsigned long long)lines);
    }
}

// ---- write ------------------------------------------------------------------------------
// the kept header line s[0, n), the k-th of the input: _header K K+1 line
__device__ __forceinline__ void header_line(Writer<>& w, uint64_t k, const uint8_t* __restrict__ s, uint32_t n)
{
    w.bytes(reinterpret_cast<const uint8_t*>("_header\t"), 8);
    w.dec(k);
    w.tab();
    w.dec(k + 1);
    w.tab();
    w.tail(s, n);
}

// ---- host -------------------------------------------------------------------------------
struct Buffers {           // behind Rec's arrays, and what place() needs
    DevBuf scal, tmp, cls, fo, a, b, cnt, ob, off, hflag, hord;
};

// the device scalars at their start values (S_BAD and S_MARK all ones, the others 0), and r's arrays for L lines of `slots` slots
inline void reset_and_bind(Buffers& B, Rec& r, const uint8_t* d_in, const uint64_t* line_end, uint64_t L, uint32_t slots, hipStream_t st)
{
    uint64_t* scal = B.scal.as<uint64_t>(S_COUNT);
    HIP_CHECK(hipMemsetAsync(scal, 0xff, 2 * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(scal + 2, 0, (S_COUNT - 2) * sizeof(uint64_t), st));
    r.in = d_in;
    r.line_end = line_end;
    r.L = L;
    r.cls = B.cls.as<uint8_t>(L);
    r.fo = B.fo.as<uint32_t>((uint64_t)slots * L);
    r.a = B.a.as<uint64_t>(L);
    r.b = B.b.as<uint64_t>(L);
    r.cnt = B.cnt.as<uint32_t>(L);
    r.ob = B.ob.as<uint64_t>(L);
    r.hflag = B.hflag.as<uint32_t>(L);
    r.scal = reinterpret_cast<unsigned long long*>(scal);
}

struct First { uint64_t bad, mark; };   // S_BAD and S_MARK after the classification; all ones: none
static_assert(sizeof(First) == 2 * sizeof(uint64_t) && S_BAD == 0 && S_MARK == 1, "First is the first two scalars");

inline First first_of(Buffers& B, hipStream_t st)
{
    First f{};
    HIP_CHECK(hipMemcpyAsync(&f, B.scal.as<uint64_t>(S_COUNT) + S_BAD, sizeof f, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return f;
}

// the error for the lowest bad line; text: the tool's bad_text
[[noreturn]] inline void throw_bad(const char* command, uint64_t bad, const char* (*text)(uint32_t))
{
    throw StarchError(STARCH_ERR_DATA, std::string(command) + ": line " + std::to_string((bad >> 8) + 1) + ": " + text((uint32_t)(bad & 255)));
}

struct Placed {            // the scalars after the tally, and where every line's output goes
    uint64_t tot[S_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t* hord = nullptr;   // with keep_header: the header lines before a line
    const uint64_t* off = nullptr;
};

// The lines [0, Le): header ordinals, the tally, the place of every line's
// output.  Throws STARCH_ERR_ARG for 2^32 output lines or more.
template <class Tally>
Placed place(Buffers& B, const Rec& r, uint64_t Le, const char* command, hipStream_t st)
{
    Placed p;
    if (Le) {
        if (r.keep_header) {
            uint64_t* h = B.hord.as<uint64_t>(Le);
            scan::excl_sum_u32_to_u64(r.hflag, h, Le, (uint64_t*)nullptr, B.tmp, st);
            p.hord = h;
        }
        uint64_t* off = B.off.as<uint64_t>(Le);
        hipLaunchKernelGGL(k_br_tally<Tally>, dim3(blocks_for(Le, kThreads)), dim3(kThreads), 0, st, r, Le, p.hord);
        HIP_CHECK(hipGetLastError());
        uint64_t* scal = reinterpret_cast<uint64_t*>(r.scal);
        scan::excl_sum_u64(r.ob, off, Le, scal + S_BYTES, B.tmp, st);
        HIP_CHECK(hipMemcpyAsync(p.tot, scal, sizeof p.tot, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        p.off = off;
    }
    if (p.tot[S_LINES] >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, std::string(command) + ": 2^32 output lines or more");
    return p;
}

}  // namespace br
