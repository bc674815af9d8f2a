// starch_amd/csrc/bed_mapscore.hip -- bedmap-scores on MI355X: for every line of a
// sorted reference, exact statistics of the scores (column 5) of the map lines
// that satisfy an overlap criterion (include/starch_amd.h has the definition).
// There is no floating point here: a score is a signed 64-bit count of 10^-9
// units, a sum is 128 bits wide, and every number that is printed is a
// rational rounded once, ties to even.
//
// Stages 1 to 3 are bedmap-elements' (me::MapelWorkspace::hits): they leave per
// reference line i the hits [hoff[i], hoff[i + 1]) of the hit list, hit h being
// map line H[h] of reference line R[h].  R never decreases, so a reference
// line's hits are one contiguous segment of the list.  Then, each part only
// when a requested column needs it:
//   4a. k_ms_parse, one thread per map line: column 5 into V (units) and ok.
//   4b. k_ms_reduce, hit-parallel.  A workgroup takes kTileHits contiguous hits,
//       a wave kWaveHits of them, 64 at a time: a segmented inclusive scan by
//       shuffles (equal R at distance d means the same segment, R being
//       sorted), with the open segment carried from one 64 to the next.  The
//       last hit of a segment holds its total.  A segment that lies wholly in a
//       wave's hits is stored by that lane; the two a wave shares with its
//       neighbours go through LDS, where one thread joins them across the
//       workgroup.  What lies wholly in the tile is stored; only a segment that
//       straddles a tile border is combined in HBM, by 64-bit integer atomics:
//       lo = sum of v & 0xffffffff, hi = sum of v >> 32 (sum = hi * 2^32 + lo),
//       min and max of the key v ^ 2^63.  Every accumulator is an integer and
//       every operation commutes, so the result does not depend on the order
//       the workgroups run in.  A hit with no valid score leaves the lowest
//       such map line by atomicMin.
//   4c. k_ms_elem: among the hits whose key is the line's min (max), the lowest
//       hit by atomicMin: ties go to map order.
//   4d. the sort's stable radix stage over (R, key) for MEDIAN and KTH; the
//       k-th smallest value of line i is then at position hoff[i] + k - 1.
//   5. format: k_ms_len measures every line, an exclusive sum places them,
//      k_ms_write divides, rounds and writes the digits, and copies the echoed
//      lines (sb::kWaveCopyBytes or more: by the whole wave).  The writer and
//      its wave copy are bed_text.hpp's, the host steps between the two kernels
//      format_tail's (common.hpp); both are shared with every BED command.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_mapscore.hpp"
#include "bed_text.hpp"

namespace ms {
namespace {

constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kNoLine = ~0u;                 // no reference line: there are fewer than 2^32 - 1 of them
constexpr uint64_t kBias = 1ull << 63;            // v ^ kBias orders signed values as unsigned keys
constexpr uint64_t kUnit = 1000000000ull;         // units per 1
enum : int { S_BYTES = 0, S_KEPT, S_STRADDLE, S_BAD, S_COUNT = 8 };   // device scalars (u64)
typedef unsigned __int128 u128;
typedef __int128 i128;

using bt::dec_digits;
using bt::line_beg;

// ---- 4a. scores -----------------------------------------------------------------------
// [+-]? D{1,9} ( '.' D{0,9} )?   or   [+-]? '.' D{1,9}   over the whole of column 5
__global__ void __launch_bounds__(kThreads)
k_ms_parse(const uint8_t* __restrict__ bed, const uint64_t* __restrict__ line_end, uint64_t m0, uint64_t Lm,
           int64_t* __restrict__ V, uint8_t* __restrict__ ok)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= Lm) return;
    const uint64_t g = m0 + j, le = line_end[g] - 1;
    uint64_t p = line_beg(line_end, g);
    bool good = true;
    for (int c = 0; c < 4 && good; ++c) {
        while (p < le && bed[p] != '\t') ++p;
        if (p == le) good = false;
        ++p;
    }
    int64_t v = 0;
    if (good) {
        bool neg = false;
        if (p < le && (bed[p] == '+' || bed[p] == '-')) { neg = bed[p] == '-'; ++p; }
        uint64_t whole = 0, frac = 0;
        uint32_t nw = 0, nf = 0;
        while (p < le && bed[p] >= '0' && bed[p] <= '9' && nw < 10) { whole = whole * 10 + (uint64_t)(bed[p] - '0'); ++nw; ++p; }
        if (p < le && bed[p] == '.') {
            ++p;
            while (p < le && bed[p] >= '0' && bed[p] <= '9' && nf < 10) { frac = frac * 10 + (uint64_t)(bed[p] - '0'); ++nf; ++p; }
        }
        good = (p == le || bed[p] == '\t') && nw <= 9 && nf <= 9 && nw + nf >= 1;
        for (uint32_t k = nf; k < 9; ++k) frac *= 10;
        if (good) v = (int64_t)(whole * kUnit + frac) * (neg ? -1 : 1);
    }
    V[j] = v;
    ok[j] = good ? 1 : 0;
}

// ---- 4b. segmented reduction ------------------------------------------------------------
struct Acc {
    uint64_t lo, hi, mn, mx;   // hi: the sum of v >> 32 in two's complement
};

__device__ __forceinline__ Acc acc_none() { return Acc{0, 0, kNone, 0}; }

__device__ __forceinline__ Acc comb(const Acc& a, const Acc& b)
{
    return Acc{a.lo + b.lo, a.hi + b.hi, a.mn < b.mn ? a.mn : b.mn, a.mx > b.mx ? a.mx : b.mx};
}

__device__ __forceinline__ Acc acc_up(const Acc& a, int d)
{
    return Acc{__shfl_up(a.lo, d, 64), __shfl_up(a.hi, d, 64), __shfl_up(a.mn, d, 64), __shfl_up(a.mx, d, 64)};
}

__device__ __forceinline__ Acc acc_of(const Acc& a, int l)
{
    return Acc{__shfl(a.lo, l, 64), __shfl(a.hi, l, 64), __shfl(a.mn, l, 64), __shfl(a.mx, l, 64)};
}

struct Reduce {
    const uint32_t *R, *H;
    const int64_t* V;
    const uint8_t* ok;
    const uint64_t* hoff;
    uint64_t T;
    uint64_t *lo, *hi, *mn, *mx;          // per reference line; lo, hi, mx start as 0, mn as all ones
    uint64_t* key;                        // per hit, for the sort (may be NULL)
    unsigned long long* scal;
};

__device__ __forceinline__ void store_line(const Reduce& f, uint32_t r, const Acc& a)
{
    f.lo[r] = a.lo;
    f.hi[r] = a.hi;
    f.mn[r] = a.mn;
    f.mx[r] = a.mx;
}

__global__ void __launch_bounds__(kThreads)
k_ms_reduce(const Reduce f)
{
    constexpr int kWaves = kThreads / 64;
    __shared__ Acc s_acc[kWaves][2];      // per wave: the segment that began before it, the one that goes on after it
    __shared__ uint32_t s_r[kWaves][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t tile_base = (uint64_t)blockIdx.x * kTileHits;
    const uint64_t tile_end = tile_base + kTileHits < f.T ? tile_base + kTileHits : f.T;
    const uint64_t wave_base = tile_base + (uint64_t)w * kWaveHits;
    const uint64_t wave_end = wave_base + kWaveHits < tile_end ? wave_base + kWaveHits : tile_end;
    if (lane < 2) s_r[w][lane] = kNoLine;
    Acc carry = acc_none();
    uint32_t carry_r = kNoLine;
    for (int c = 0; c < kChunks; ++c) {
        const uint64_t p0 = wave_base + (uint64_t)c * 64;
        if (p0 >= wave_end) break;        // the same for the whole wave
        const uint64_t i = p0 + lane;
        const bool valid = i < wave_end;
        uint32_t r = kNoLine;
        Acc a = acc_none();
        if (valid) {
            r = f.R[i];
            const uint32_t j = f.H[i];
            const int64_t v = f.V[j];
            if (!f.ok[j]) atomicMin(f.scal + S_BAD, (unsigned long long)j);
            const uint64_t key = (uint64_t)v ^ kBias;
            if (f.key) f.key[i] = key;
            a = Acc{(uint64_t)v & 0xffffffffull, (uint64_t)(v >> 32), key, key};
        }
        if (lane == 0 && r == carry_r) a = comb(carry, a);   // lane 0 is valid here
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Acc o = acc_up(a, d);
            const uint32_t o_r = __shfl_up(r, d, 64);
            if (lane >= d && o_r == r) a = comb(o, a);
        }
        const uint32_t n_r = __shfl_down(r, 1, 64);
        if (valid && (lane == 63 || n_r != r)) {             // the last hit of its segment among these 64
            const uint64_t hb = f.hoff[r], he = f.hoff[r + 1];
            if (i + 1 == he) {
                if (hb >= wave_base) store_line(f, r, a);
                else { s_acc[w][0] = a; s_r[w][0] = r; }
            } else if (i + 1 == wave_end) { s_acc[w][1] = a; s_r[w][1] = r; }
        }
        carry = acc_of(a, 63);
        carry_r = __shfl(r, 63, 64);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t cr = kNoLine;
    Acc ca = acc_none();
    auto emit = [&] {
        if (cr == kNoLine) return;
        const uint64_t hb = f.hoff[cr], he = f.hoff[cr + 1];
        if (hb >= tile_base && he <= tile_end) return store_line(f, cr, ca);
        atomicAdd(reinterpret_cast<unsigned long long*>(f.lo + cr), (unsigned long long)ca.lo);
        atomicAdd(reinterpret_cast<unsigned long long*>(f.hi + cr), (unsigned long long)ca.hi);
        atomicMin(reinterpret_cast<unsigned long long*>(f.mn + cr), (unsigned long long)ca.mn);
        atomicMax(reinterpret_cast<unsigned long long*>(f.mx + cr), (unsigned long long)ca.mx);
        if (hb >= tile_base) atomicAdd(f.scal + S_STRADDLE, 1ull);   // counted once, where it begins
    };
    for (int k = 0; k < 2 * kWaves; ++k) {
        const uint32_t r = s_r[k >> 1][k & 1];
        if (r == kNoLine) continue;
        if (r == cr) ca = comb(ca, s_acc[k >> 1][k & 1]);
        else {
            emit();
            cr = r;
            ca = s_acc[k >> 1][k & 1];
        }
    }
    emit();
}

// ---- 4c. elements -----------------------------------------------------------------------
// imin, imax (either may be NULL) start as all ones.  A hit whose predecessor in
// the wave is of the same line and has the same key leaves the atomic to it.
__global__ void __launch_bounds__(kThreads)
k_ms_elem(const uint32_t* __restrict__ R, const uint32_t* __restrict__ H, const int64_t* __restrict__ V, uint64_t T,
          const uint64_t* __restrict__ mn, const uint64_t* __restrict__ mx, uint64_t* imin, uint64_t* imax)
{
    const uint64_t h = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t r = kNoLine;
    uint64_t key = 0;
    if (h < T) {
        r = R[h];
        key = (uint64_t)V[H[h]] ^ kBias;
    }
    const uint32_t p_r = __shfl_up(r, 1, 64);
    const uint64_t p_key = __shfl_up(key, 1, 64);
    if (h >= T || (lane > 0 && p_r == r && p_key == key)) return;
    if (imin && key == mn[r]) atomicMin(reinterpret_cast<unsigned long long*>(imin + r), (unsigned long long)h);
    if (imax && key == mx[r]) atomicMin(reinterpret_cast<unsigned long long*>(imax + r), (unsigned long long)h);
}

// ---- 5. format --------------------------------------------------------------------------
struct Format {
    const uint8_t* bed;
    const uint64_t* line_end;             // of every line of the buffer; map line j is line m0 + j
    const uint64_t *cnt, *hoff;
    const uint32_t* H;
    const uint64_t *lo, *hi, *mn, *mx, *imin, *imax;
    const uint64_t* key;                  // per hit
    const uint32_t* order;                // position in (R, key) order -> hit; NULL: the hits are in that order
    uint64_t Lr, m0;
    uint64_t kth_num, kth_den;
    uint64_t unit;                        // 10^(9 - prec): units per 10^-prec
    uint32_t ncols, prec, skip_unmapped, delim_len;
    uint8_t cols[kMaxCols];
    uint8_t delim[8];
};

// the k-th smallest (k from 1) score of line i
__device__ __forceinline__ int64_t kth_value(const Format& f, uint64_t i, uint64_t k)
{
    const uint64_t pos = f.hoff[i] + k - 1;
    return (int64_t)(f.key[f.order ? f.order[pos] : pos] ^ kBias);
}

// A number as it is printed: |m| = top * 10^18 + low with low < 10^18, m the
// integer nearest to x * 10^prec, ties to even; neg only when m < 0.
struct Num {
    uint64_t top, low;
    bool neg;
};

// column col (SUM .. KTH) of line i with c >= 1 hits: x = num / den units, and num / (den * unit) is rounded
__device__ __forceinline__ Num number(const Format& f, uint32_t col, uint64_t i, uint64_t c)
{
    i128 num = 0;
    uint64_t den = f.unit;
    switch (col) {
        case STARCH_MAPSC_SUM:
        case STARCH_MAPSC_MEAN:
            num = (i128)(int64_t)f.hi[i] * ((i128)1 << 32) + (i128)f.lo[i];
            if (col == STARCH_MAPSC_MEAN) den *= c;      // below 2^32 * 10^9
            break;
        case STARCH_MAPSC_MIN: num = (int64_t)(f.mn[i] ^ kBias); break;
        case STARCH_MAPSC_MAX: num = (int64_t)(f.mx[i] ^ kBias); break;
        case STARCH_MAPSC_MEDIAN:
            if (c & 1) num = kth_value(f, i, (c + 1) / 2);
            else {
                num = (i128)kth_value(f, i, c / 2) + (i128)kth_value(f, i, c / 2 + 1);
                den *= 2;
            }
            break;
        default:   // KTH: k = ceil(f * c), 1 <= k <= c
            num = kth_value(f, i, (f.kth_num * c + f.kth_den - 1) / f.kth_den);
    }
    const bool neg = num < 0;
    const u128 mag = neg ? (u128)(-num) : (u128)num;
    u128 q = mag / den;
    const uint64_t rem = (uint64_t)(mag % den);          // den < 2^62: 2 * rem does not wrap
    if (2 * rem > den || (2 * rem == den && ((uint64_t)q & 1))) ++q;
    const uint64_t e18 = 1000000000000000000ull;
    return Num{(uint64_t)(q / e18), (uint64_t)(q % e18), neg && q != 0};
}

__device__ __forceinline__ uint32_t num_len(const Num& x, uint32_t prec)
{
    const uint32_t d = x.top ? 18 + dec_digits(x.top) : dec_digits(x.low);
    return (x.neg ? 1u : 0u) + (d > prec ? d - prec : 1u) + (prec ? 1u + prec : 0u);
}

// writes the len = num_len(x, prec) bytes of x, from its last digit backwards
__device__ __forceinline__ void num_put(uint8_t* o, Num x, uint32_t prec, uint32_t len)
{
    uint32_t p = len, taken = 0;
    auto digit = [&]() -> uint8_t {
        uint64_t& v = taken < 18 ? x.low : x.top;
        const uint8_t d = (uint8_t)('0' + v % 10);
        v /= 10;
        ++taken;
        return d;
    };
    for (uint32_t k = 0; k < prec; ++k) o[--p] = digit();
    if (prec) o[--p] = '.';
    do o[--p] = digit();
    while (x.top || x.low);
    if (x.neg) o[--p] = '-';
}

// the bytes of the map line (without '\n') that MIN_ELEMENT or MAX_ELEMENT copies for line i
__device__ __forceinline__ void element(const Format& f, uint32_t col, uint64_t i, uint64_t* src, uint64_t* n)
{
    const uint64_t h = col == STARCH_MAPSC_MIN_ELEMENT ? f.imin[i] : f.imax[i];
    const uint64_t g = f.m0 + f.H[h];
    *src = line_beg(f.line_end, g);
    *n = f.line_end[g] - 1 - *src;
}

// len: bytes of output line i with its '\n' (0: left out); keep (may be NULL): 1 when it is written
__global__ void __launch_bounds__(kThreads)
k_ms_len(const Format f, uint64_t* __restrict__ len, uint32_t* __restrict__ keep)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f.Lr) return;
    const uint64_t c = f.cnt[i];
    uint64_t n = 0;
    if (!(f.skip_unmapped && c == 0)) {
        n = (uint64_t)f.delim_len * (f.ncols - 1) + 1;
        for (uint32_t k = 0; k < f.ncols; ++k) {
            const uint32_t col = f.cols[k];
            if (col == STARCH_MAPSC_ECHO) n += f.line_end[i] - 1 - line_beg(f.line_end, i);
            else if (col == STARCH_MAPSC_COUNT) n += dec_digits(c);
            else if (col == STARCH_MAPSC_INDICATOR) n += 1;
            else if (c == 0) n += 3;      // NAN
            else if (col >= STARCH_MAPSC_MIN_ELEMENT) {
                uint64_t src, m;
                element(f, col, i, &src, &m);
                n += m;
            } else n += num_len(number(f, col, i, c), f.prec);
        }
    }
    len[i] = n;
    if (keep) keep[i] = n ? 1u : 0u;
}

// A thread writes its line; a copy of sb::kWaveCopyBytes or more (the echo and
// the two element columns) is left to the whole wave, one after another.
__global__ void __launch_bounds__(kThreads)
k_ms_write(const Format f, const uint64_t* __restrict__ len, const uint64_t* __restrict__ off, uint64_t out_bytes,
           uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bt::Writer<3> w{out, 0};   // slots: the echo, the min element, the max element
    if (i < f.Lr && len[i] && off[i] + len[i] <= out_bytes) {
        const uint64_t c = f.cnt[i];
        w.o = off[i];
        for (uint32_t k = 0; k < f.ncols; ++k) {
            const uint32_t col = f.cols[k];
            if (k) w.delim(f.delim, f.delim_len);
            if (col == STARCH_MAPSC_ECHO) {
                const uint64_t b = line_beg(f.line_end, i);
                w.copy(0, f.bed + b, f.line_end[i] - 1 - b);
            } else if (col == STARCH_MAPSC_COUNT) w.dec(c);
            else if (col == STARCH_MAPSC_INDICATOR) out[w.o++] = c ? '1' : '0';
            else if (c == 0) w.bytes(reinterpret_cast<const uint8_t*>("NAN"), 3);
            else if (col >= STARCH_MAPSC_MIN_ELEMENT) {
                uint64_t src, m;
                element(f, col, i, &src, &m);
                if (col == STARCH_MAPSC_MIN_ELEMENT) w.copy(1, f.bed + src, m);   // (a constant slot keeps w in registers)
                else w.copy(2, f.bed + src, m);
            } else {
                const Num x = number(f, col, i, c);
                const uint32_t d = num_len(x, f.prec);
                num_put(out + w.o, x, f.prec, d);
                w.o += d;
            }
        }
        out[w.o] = '\n';
    }
    bt::wave_copy_tails(w, out, lane);
}

}  // namespace

void MapscWorkspace::run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, me::MapelWorkspace& hitter,
                         const MapscOptions& opt, const uint8_t* d_cat, uint64_t n, const std::vector<uint64_t>& in_end,
                         hipStream_t st, DevBuf& out, MapscResult& res)
{
    res = MapscResult{};
    const uint64_t N = in_end.size();
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) {
        timer.finish(from, st, {&res.ms_parse, &res.ms_build, &res.ms_query, &res.ms_reduce, &res.ms_format});
    };

    // 1 to 3. the hit list
    me::HitList hl;
    const int done = hitter.hits(sorter, lines, "bedmap-scores", opt.crit, d_cat, n, in_end, st, timer.marks_from(1), hl);
    res.n_ref = hl.Lr;
    res.n_map = hl.Lm;
    res.n_chromosomes = hl.n_chromosomes;
    res.hits = hl.T;
    if (done < 3) return finish(done + 1);
    const uint64_t Lr = hl.Lr, Lm = hl.Lm, m0 = hl.m0, T = hl.T;

    // 4. what the columns need
    uint32_t want = 0;
    for (uint32_t k = 0; k < opt.ncols; ++k) want |= 1u << opt.cols[k];
    const bool scores = (want >> STARCH_MAPSC_SUM) != 0;
    const bool order = (want & ((1u << STARCH_MAPSC_MEDIAN) | (1u << STARCH_MAPSC_KTH))) != 0;
    const bool emin = (want >> STARCH_MAPSC_MIN_ELEMENT) & 1, emax = (want >> STARCH_MAPSC_MAX_ELEMENT) & 1;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    HIP_CHECK(hipMemsetAsync(scal, 0, S_COUNT * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(scal + S_BAD, 0xff, sizeof(uint64_t), st));
    Format f{};
    if (scores && T) {
        int64_t* V = b_V.as<int64_t>(Lm);
        uint8_t* ok = b_ok.as<uint8_t>(Lm);
        hipLaunchKernelGGL(k_ms_parse, dim3(blocks_for(Lm, kThreads)), dim3(kThreads), 0, st, d_cat, sorter.ln.line_end, m0, Lm,
                           V, ok);
        HIP_CHECK(hipGetLastError());
        Reduce q{};
        q.R = hl.R;
        q.H = hl.H;
        q.V = V;
        q.ok = ok;
        q.hoff = hl.hoff;
        q.T = T;
        q.lo = b_lo.as<uint64_t>(Lr);
        q.hi = b_hi.as<uint64_t>(Lr);
        q.mn = b_min.as<uint64_t>(Lr);
        q.mx = b_max.as<uint64_t>(Lr);
        q.key = order ? b_key.as<uint64_t>(T) : nullptr;
        q.scal = reinterpret_cast<unsigned long long*>(scal);
        HIP_CHECK(hipMemsetAsync(q.lo, 0, Lr * sizeof(uint64_t), st));
        HIP_CHECK(hipMemsetAsync(q.hi, 0, Lr * sizeof(uint64_t), st));
        HIP_CHECK(hipMemsetAsync(q.mx, 0, Lr * sizeof(uint64_t), st));
        HIP_CHECK(hipMemsetAsync(q.mn, 0xff, Lr * sizeof(uint64_t), st));
        hipLaunchKernelGGL(k_ms_reduce, dim3(blocks_for(T, kTileHits)), dim3(kThreads), 0, st, q);
        HIP_CHECK(hipGetLastError());
        uint64_t got[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(got, scal + S_STRADDLE, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (got[1] != kNone)
            throw StarchError(STARCH_ERR_DATA, "bedmap-scores: input " + std::to_string(N == 2 ? 1 : 0) + ", line " +
                                                   std::to_string(got[1] + 1) +
                                                   ": the line is a hit and its column 5 is missing or is no score (an optional "
                                                   "sign, up to 9 digits, and a point with up to 9 digits)");
        res.straddling = got[0];
        f.lo = q.lo;
        f.hi = q.hi;
        f.mn = q.mn;
        f.mx = q.mx;
        f.key = q.key;
        if (emin || emax) {
            uint64_t* imin = emin ? b_imin.as<uint64_t>(Lr) : nullptr;
            uint64_t* imax = emax ? b_imax.as<uint64_t>(Lr) : nullptr;
            if (imin) HIP_CHECK(hipMemsetAsync(imin, 0xff, Lr * sizeof(uint64_t), st));
            if (imax) HIP_CHECK(hipMemsetAsync(imax, 0xff, Lr * sizeof(uint64_t), st));
            hipLaunchKernelGGL(k_ms_elem, dim3(blocks_for(T, kThreads)), dim3(kThreads), 0, st, hl.R, hl.H, V, T, q.mn, q.mx, imin,
                               imax);
            HIP_CHECK(hipGetLastError());
            f.imin = imin;
            f.imax = imax;
        }
        if (order) {
            // the radix stage's scratch (its index, digit and histogram buffers) is none of the sorter's per-line arrays
            const sb::KeyBits kb = sorter.stage_check(hl.R, q.key, q.key, T, st);
            if (kb.desc != kNone) {       // a hit's (line, key) is below its predecessor's
                uint32_t passes = 0;
                f.order = sorter.stage_radix(hl.R, q.key, nullptr, T, kb, st, &passes);
                if (!f.order) throw StarchError(STARCH_ERR_INTERNAL, "bedmap-scores: no order for the hits");
                res.sorted_hits = T;
                res.radix_passes = passes;
            }
        }
    }
    timer.mark(4, st);

    // 5. format
    f.bed = d_cat;
    f.line_end = sorter.ln.line_end;
    f.cnt = hl.cnt;
    f.hoff = hl.hoff;
    f.H = hl.H;
    f.Lr = Lr;
    f.m0 = m0;
    f.kth_num = opt.kth_num;
    f.kth_den = opt.kth_den;
    f.unit = 1;
    for (uint32_t k = opt.prec; k < 9; ++k) f.unit *= 10;
    f.ncols = opt.ncols;
    f.prec = opt.prec;
    f.skip_unmapped = opt.skip_unmapped;
    f.delim_len = opt.delim_len;
    for (uint32_t k = 0; k < opt.ncols; ++k) f.cols[k] = opt.cols[k];
    for (uint32_t k = 0; k < opt.delim_len; ++k) f.delim[k] = opt.delim[k];
    const unsigned rblocks = blocks_for(Lr, kThreads);
    uint64_t* len = b_len.as<uint64_t>(Lr);
    uint64_t* off = b_off.as<uint64_t>(Lr);
    uint32_t* keep = opt.skip_unmapped ? b_keep.as<uint32_t>(Lr) : nullptr;
    hipLaunchKernelGGL(k_ms_len, dim3(rblocks), dim3(kThreads), 0, st, f, len, keep);
    HIP_CHECK(hipGetLastError());
    // (the kept lines are counted; the lengths of the others are 0, which leaves them out)
    uint64_t tot[2] = {0, 0};
    const FormatTail ft = format_tail(Lr, len, off, keep, keep ? b_kpos.as<uint64_t>(Lr) : nullptr, scal + S_BYTES, tot,
                                      keep ? 2 : 1, b_tmp, out, st, "bedmap-scores", true);
    hipLaunchKernelGGL(k_ms_write, dim3(rblocks), dim3(kThreads), 0, st, f, len, off, ft.bytes, static_cast<uint8_t*>(out.p));
    HIP_CHECK(hipGetLastError());
    res.out_bytes = ft.bytes;
    res.lines_out = ft.lines_kept;
    finish(5);
}

}  // namespace ms
