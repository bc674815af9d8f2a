// starch_amd/csrc/bed_bbi_dev.hip -- bigwig2bed and bigbed2bed on MI355X: the
// inflated blocks of a bigWig / bigBed file into BED lines (the definition:
// include/starch_amd.h).  What is decided about a block's
// bytes is decided by the functions of bed_bbi_rec.hpp, which the host runs too;
// the kernels here find the records, call those functions and place the text.
//   bigWig.  A block is one section.  k_bw_sections, a thread per block: the
//     section against its header and the chromosome count; its itemCount is its
//     number of records.  An exclusive sum gives every record its global index.
//   bigBed.  Records are chromId, start, end, rest NUL and aligned to nothing.
//     k_bb_chain, one wave per block: from the record at `cur` the wave looks
//     through the bytes from cur + 12 on, kChainWindow at a time and 16 to a lane,
//     for the first zero byte; the lowest lane that found one ends the record.
//     Once to count a block's records and, after the exclusive sum, once to
//     write their offsets.  Blocks are independent: no walk crosses the file.
//   Both.  k_*_measure, a thread per record: the record's own check, the region's
//     choice and the bytes of its line; an exclusive sum places the lines;
//     k_*_write writes them.  A bigBed rest of kWaveRest bytes or more is
//     searched for a newline and copied by the record's whole wave.
// A bad block enters an atomicMin as (block << 8) | kind, so the lowest bad block
// is the one reported, and nothing is written.  A thread reads only bytes of its
// own block, inside the length the block table gave, and writes only its placed
// range, which is checked against the output's size.
#include "bed_bbi_dev.hpp"

#include "../../include/starch_amd.h"

namespace bbidev {
namespace {

using namespace bbirec;

enum : int { S_BAD = 0, S_TOTAL, S_LINES, S_BYTES, S_WAVE, S_COUNT = 8 };   // device scalars (u64); S_BAD starts as all ones

struct Par {               // what every kernel takes
    const uint8_t* d;
    const uint64_t *boff, *blen;
    uint64_t B;
    uint32_t* cnt;         // records per block
    const uint64_t* base;  // their exclusive sum
    const uint32_t* name_off;
    const uint8_t* names;
    uint32_t n_chroms;
    Region rg;
    uint64_t* ob;          // bytes of every record's line
    unsigned long long* scal;
};

__device__ __forceinline__ void report(const Par& P, uint64_t block, uint32_t kind)
{
    atomicMin(&P.scal[S_BAD], (unsigned long long)((block << 8) | kind));
}

// the block that holds record i: the last one whose base is at or below i
__device__ __forceinline__ uint64_t block_of(const uint64_t* __restrict__ base, uint64_t B, uint64_t i)
{
    uint64_t lo = 0, hi = B;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (base[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;         // base[0] = 0, so lo >= 1
}

__device__ __forceinline__ void count_lines(const Par& P, bool line, bool wave_rec)
{
    const uint32_t n = __popcll(__ballot(line)), w = __popcll(__ballot(wave_rec));
    if ((threadIdx.x & 63) == 0) {
        if (n) atomicAdd(&P.scal[S_LINES], (unsigned long long)n);
        if (w) atomicAdd(&P.scal[S_WAVE], (unsigned long long)w);
    }
}

// ---- bigWig ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_bw_sections(const Par P)
{
    const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= P.B) return;
    WigSec s;
    const uint32_t e = wig_section(P.d + P.boff[b], P.blen[b], P.n_chroms, &s);
    if (e) report(P, b, e);
    P.cnt[b] = e ? 0u : s.count;
}

// record i of R: its section, its number in it, and what wig_record says of it; false when it is not to be touched
__device__ __forceinline__ bool bw_record(const Par& P, uint64_t i, uint64_t* block, WigSec* s, uint64_t* a, uint64_t* b, uint32_t* bits,
                                          uint32_t* err)
{
    const uint64_t k = block_of(P.base, P.B, i);
    const uint8_t* p = P.d + P.boff[k];
    if (wig_section(p, P.blen[k], P.n_chroms, s)) return false;   // (counted as 0 records: not reached)
    const uint64_t j = i - P.base[k];
    if (j >= s->count) return false;
    *block = k;
    *err = wig_record(p, *s, (uint32_t)j, a, b, bits);
    return true;
}

__global__ void __launch_bounds__(kThreads) k_bw_measure(const Par P, uint64_t R)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint64_t bytes = 0;
    if (i < R) {
        WigSec s;
        uint64_t k = 0, a = 0, b = 0;
        uint32_t bits = 0, err = 0;
        if (bw_record(P, i, &k, &s, &a, &b, &bits, &err)) {
            if (err) report(P, k, err);
            else if (region_keeps(P.rg, s.chrom, a, b)) bytes = wig_line_len(P.name_off[s.chrom + 1] - P.name_off[s.chrom], a, b, bits);
        }
        P.ob[i] = bytes;
    }
    count_lines(P, bytes != 0, false);
}

__global__ void __launch_bounds__(kThreads) k_bw_write(const Par P, uint64_t R, const uint64_t* __restrict__ off, uint64_t out_bytes,
                                                       uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= R) return;
    const uint64_t bytes = P.ob[i], at = off[i];
    if (!bytes || at + bytes > out_bytes) return;
    WigSec s;
    uint64_t k = 0, a = 0, b = 0;
    uint32_t bits = 0, err = 0;
    if (!bw_record(P, i, &k, &s, &a, &b, &bits, &err) || err) return;
    const uint32_t n0 = P.name_off[s.chrom];
    (void)wig_line_write(out + at, P.names + n0, P.name_off[s.chrom + 1] - n0, a, b, bits);
}

// ---- bigBed ---------------------------------------------------------------------------
// One wave per block: its chain of records.  Counting, a block that does not
// end on a record's zero byte is reported and counts no records; with kWrite
// the offsets (into d) and the bytes of the records go to rec_off and rec_len
// from base[block] on, at most cnt[block] of them.
template <bool kWrite>
__global__ void __launch_bounds__(64) k_bb_chain(const Par P, uint64_t* __restrict__ rec_off, uint32_t* __restrict__ rec_len)
{
    const uint64_t k = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint64_t len = P.blen[k], b0 = P.boff[k];
    const uint8_t* p = P.d + b0;
    const uint64_t at = kWrite ? P.base[k] : 0;
    const uint32_t most = kWrite ? P.cnt[k] : 0xffffffffu;
    uint32_t c = 0, err = 0;
    for (uint64_t cur = 0; cur < len && c < most;) {
        if ((err = bed_room(len, cur))) break;
        uint64_t z = len;
        for (uint64_t w = cur + kBedFixed; w < len; w += kChainWindow) {
            const uint64_t lo = w + 16ull * lane, hi = lo + 16 < len ? lo + 16 : len;
            const uint64_t f = lo < hi ? bed_first_zero(p, lo, hi) : hi;
            const unsigned long long m = __ballot(lo < hi && f < hi);
            if (m) {
                z = __shfl(f, __ffsll(m) - 1, 64);
                break;
            }
        }
        uint64_t next = 0;
        if ((err = bed_close(len, z, &next))) break;
        if (kWrite && lane == 0) {
            rec_off[at + c] = b0 + cur;
            rec_len[at + c] = (uint32_t)(next - cur);
        }
        ++c;
        cur = next;
    }
    if (!kWrite && lane == 0) {
        if (err) report(P, k, err);
        P.cnt[k] = err ? 0u : c;
    }
}

__global__ void __launch_bounds__(kThreads) k_bb_measure(const Par P, uint64_t R, const uint64_t* __restrict__ rec_off,
                                                         const uint32_t* __restrict__ rec_len)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool valid = i < R;
    const uint64_t at = valid ? rec_off[i] : 0;
    const uint64_t rest = valid ? (uint64_t)rec_len[i] - kBedMinRecord : 0;
    uint32_t chrom = 0, err = 0;
    uint64_t a = 0, b = 0;
    if (valid) err = bed_record(P.d + at, P.n_chroms, &chrom, &a, &b);
    const bool big = valid && rest >= kWaveRest;
    bool nl = valid && !big && bed_has_newline(P.d + at, kBedFixed, kBedFixed + rest);
    unsigned long long m = __ballot(big);
    while (m) {            // a long rest: searched by the whole wave, 16 bytes to a lane per round
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const uint8_t* p = P.d + __shfl(at, l, 64);
        const uint64_t end = kBedFixed + __shfl(rest, l, 64);
        bool f = false;
        for (uint64_t q = kBedFixed + 16ull * lane; q < end; q += 16ull * 64) f |= bed_has_newline(p, q, q + 16 < end ? q + 16 : end);
        const bool any = __ballot(f) != 0;
        if ((int)lane == l) nl = any;
    }
    if (!err && nl) err = K_BED_NEWLINE;
    uint64_t bytes = 0;
    if (valid) {
        if (err) report(P, block_of(P.base, P.B, i), err);
        else if (region_keeps(P.rg, chrom, a, b)) bytes = bed_line_len(P.name_off[chrom + 1] - P.name_off[chrom], a, b, rest);
        P.ob[i] = bytes;
    }
    count_lines(P, bytes != 0, big && bytes != 0);
}

__global__ void __launch_bounds__(kThreads) k_bb_write(const Par P, uint64_t R, const uint64_t* __restrict__ rec_off,
                                                       const uint32_t* __restrict__ rec_len, const uint64_t* __restrict__ off,
                                                       uint64_t out_bytes, uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool valid = i < R;
    const uint64_t bytes = valid ? P.ob[i] : 0, to = valid ? off[i] : 0;
    const bool line = bytes != 0 && to + bytes <= out_bytes;
    const uint64_t at = line ? rec_off[i] : 0;
    const uint64_t rest = line ? (uint64_t)rec_len[i] - kBedMinRecord : 0;
    uint64_t rest_to = 0;
    if (line) {
        uint32_t chrom = 0;
        uint64_t a = 0, b = 0;
        (void)bed_record(P.d + at, P.n_chroms, &chrom, &a, &b);   // checked when it was measured
        const uint32_t n0 = P.name_off[chrom];
        rest_to = to + bed_line_head(out + to, P.names + n0, P.name_off[chrom + 1] - n0, a, b, rest);
        if (rest < kWaveRest)
            for (uint64_t q = 0; q < rest; ++q) out[rest_to + q] = P.d[at + kBedFixed + q];
        out[to + bytes - 1] = '\n';
    }
    unsigned long long m = __ballot(line && rest >= kWaveRest);
    while (m) {            // a long rest: copied by the whole wave
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const uint8_t* src = P.d + __shfl(at, l, 64) + kBedFixed;
        const uint64_t dst = __shfl(rest_to, l, 64), n = __shfl(rest, l, 64);
        for (uint64_t q = lane; q < n; q += 64) out[dst + q] = src[q];
    }
}

[[noreturn]] void throw_block(const Input& in, uint64_t bad)
{
    const uint64_t k = bad >> 8;
    throw StarchError(STARCH_ERR_DATA, std::string(in.kind == 1 ? "bigwig2bed" : "bigbed2bed") + ": block " +
                                           std::to_string(k < in.index.size() ? in.index[k] : k) + ": " + bad_text((uint32_t)(bad & 255)));
}

}  // namespace

void Workspace::run(const Input& in, hipStream_t st, DevBuf& out, Result& res)
{
    res = Result{};
    (void)out.as<uint8_t>(64);
    const uint64_t B = in.off.size(), C = in.chroms.size();
    const bool wig = in.kind == 1;
    const char* tool = wig ? "bigwig2bed" : "bigbed2bed";
    res.blocks = B;
    if (!B) return;
    if (B >= (1ull << 31)) throw StarchError(STARCH_ERR_ARG, std::string(tool) + ": 2^31 blocks or more");
    // the block table and the chromosome names (offsets, then the bytes) go up
    std::vector<uint32_t> noff(C + 1, 0);
    std::string nbytes;
    for (uint64_t k = 0; k < C; ++k) {
        nbytes += in.chroms[k];
        noff[k + 1] = (uint32_t)nbytes.size();
    }
    uint64_t* d_boff = boff.as<uint64_t>(B);
    uint64_t* d_blen = blen.as<uint64_t>(B);
    uint8_t* d_names = names.as<uint8_t>((C + 1) * 4 + nbytes.size() + 8);
    HIP_CHECK(hipMemcpyAsync(d_boff, in.off.data(), B * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_blen, in.len.data(), B * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_names, noff.data(), (C + 1) * 4, hipMemcpyHostToDevice, st));
    if (!nbytes.empty()) HIP_CHECK(hipMemcpyAsync(d_names + (C + 1) * 4, nbytes.data(), nbytes.size(), hipMemcpyHostToDevice, st));
    uint64_t* d_scal = scal.as<uint64_t>(S_COUNT);
    HIP_CHECK(hipMemsetAsync(d_scal, 0xff, sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(d_scal + 1, 0, (S_COUNT - 1) * sizeof(uint64_t), st));
    uint64_t* d_base = base.as<uint64_t>(B);
    Par P{};
    P.d = in.d;
    P.boff = d_boff;
    P.blen = d_blen;
    P.B = B;
    P.cnt = cnt.as<uint32_t>(B);
    P.base = d_base;
    P.name_off = reinterpret_cast<const uint32_t*>(d_names);
    P.names = d_names + (C + 1) * 4;
    P.n_chroms = (uint32_t)C;
    P.rg = in.rg;
    P.scal = reinterpret_cast<unsigned long long*>(d_scal);
    timer.start(st);
    auto scalars = [&](uint64_t* h) {
        HIP_CHECK(hipMemcpyAsync(h, d_scal, S_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));   // (the host vectors above are free again, too)
        if (h[S_BAD] != ~0ull) throw_block(in, h[S_BAD]);
    };

    // 1. the records of every block, counted
    if (wig) hipLaunchKernelGGL(k_bw_sections, dim3(blocks_for(B, kThreads)), dim3(kThreads), 0, st, P);
    else hipLaunchKernelGGL(k_bb_chain<false>, dim3((unsigned)B), dim3(64), 0, st, P, nullptr, nullptr);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(P.cnt, d_base, B, d_scal + S_TOTAL, tmp, st);
    uint64_t h[S_COUNT];
    scalars(h);
    const uint64_t R = h[S_TOTAL];
    if (R >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, std::string(tool) + ": 2^32 records or more");
    res.records = R;
    uint64_t* d_rec = nullptr;
    uint32_t* d_len = nullptr;
    if (!wig && R) {
        d_rec = rec_off.as<uint64_t>(R);
        d_len = rec_len.as<uint32_t>(R);
        hipLaunchKernelGGL(k_bb_chain<true>, dim3((unsigned)B), dim3(64), 0, st, P, d_rec, d_len);
        HIP_CHECK(hipGetLastError());
    }
    timer.mark(1, st);

    // 2. every record checked and measured, the lines placed
    uint64_t* d_off = off.as<uint64_t>(R);
    P.ob = ob.as<uint64_t>(R);
    if (R) {
        const dim3 grid(blocks_for(R, kThreads));
        if (wig) hipLaunchKernelGGL(k_bw_measure, grid, dim3(kThreads), 0, st, P, R);
        else hipLaunchKernelGGL(k_bb_measure, grid, dim3(kThreads), 0, st, P, R, d_rec, d_len);
        HIP_CHECK(hipGetLastError());
        scan::excl_sum_u64(P.ob, d_off, R, d_scal + S_BYTES, tmp, st);
    }
    scalars(h);
    timer.mark(2, st);

    // 3. the text
    const uint64_t bytes = h[S_BYTES];
    if (h[S_LINES] >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, std::string(tool) + ": 2^32 output lines or more");
    if (bytes) {
        uint8_t* o = out.as<uint8_t>(bytes + 64);
        const dim3 grid(blocks_for(R, kThreads));
        if (wig) hipLaunchKernelGGL(k_bw_write, grid, dim3(kThreads), 0, st, P, R, d_off, bytes, o);
        else hipLaunchKernelGGL(k_bb_write, grid, dim3(kThreads), 0, st, P, R, d_rec, d_len, d_off, bytes, o);
        HIP_CHECK(hipGetLastError());
    }
    res.lines_out = h[S_LINES];
    res.wave_records = h[S_WAVE];
    res.out_bytes = bytes;
    timer.finish(3, st, {&res.ms_frame, &res.ms_parse, &res.ms_write});
}

}  // namespace bbidev
