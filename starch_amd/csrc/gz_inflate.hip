// starch_amd/csrc/gz_inflate.hip -- gzip and BGZF inputs inflated on MI355X
// (RFC 1951/1952).
//
// The unit of work is a gzip member.  BGZF (bgzip's framing: every member holds
// its compressed size in a BC extra subfield and inflates to at most 64 KiB) is
// planned on the host from the headers alone; generic gzip (gzip, pigz, zlib)
// by k_gz_size, one wave that walks the Huffman symbols of the whole chain of
// members and sums lengths without copying anything.  Either way the result is
// a table of members {in_off, in_len, out_off, out_len, crc, isize}.
//   k_gz_inflate  one 64-lane wave per member, grid-stride over the table.  The
//                 wave reads bits uniformly: a 64-bit bit buffer refilled from a
//                 512-byte window of the input held 8 bytes per lane.  A dynamic
//                 block's tables are built from its code lengths across the
//                 lanes (counts per length, first codes, a primary LDS table
//                 for codes up to kPrimaryBits, longer codes resolved
//                 canonically).  A literal is one LDS byte store; a match is
//                 copied by the whole wave, lane i taking out[p + i] =
//                 out[p - dist + i % dist] in rounds of 64; a stored block is a
//                 wave copy.  The output window is an LDS ring (matches read
//                 what the wave has just written) flushed to HBM in aligned
//                 16-byte stores.
//   k_gz_crc_chunks, k_gz_crc_members   CRC-32 of every member's output,
//                 folded from 4 KiB pieces (gz_crc.hpp), against its trailer.
//   k_tab_inflate, k_tab_adler   the same decoder over a table its caller made
//                 (TableInflater: the zlib blocks of a bigWig / bigBed file):
//                 header and trailer lengths are the table's and the caller's,
//                 a member's out_len is a slot it may not pass, and the check
//                 is Adler-32, folded from 4 KiB pieces (gz_adler.hpp).
// The inputs are untrusted.  Every loop iteration consumes input bits or ends
// the member, the bit position is checked against the member's extent, every
// output write against the member's slot, every match distance against the
// bytes the member has produced; a violation sets the member's error word and
// stops that member only.
#include "gz_inflate.hpp"
#include "gz_adler.hpp"
#include "gz_crc.hpp"

#include <algorithm>
#include <chrono>

namespace gz {
namespace {

constexpr uint32_t W = kWindowBytes;
constexpr uint32_t PB_LIT = kPrimaryBits, PB_DIST = 9, PB_CL = 7;
constexpr uint32_t CRC_CHUNK = 4096;
static_assert(W % 16 == 0 && W >= 32768 + 258 + 16 && W >= kFlushBytes + 2 * 258 + 32, "ring too small");

enum Err : uint32_t {
    E_OK = 0, E_MAGIC, E_FLG, E_HDR_TRUNC, E_TRAILING, E_BTYPE, E_STORED_LEN, E_TRUNC, E_HLIT, E_HDIST, E_CL_SET,
    E_REP_FIRST, E_REP_PAST, E_NO_EOB, E_LIT_OVER, E_LIT_INCOMPLETE, E_DIST_OVER, E_DIST_INCOMPLETE, E_LIT_SYM,
    E_DIST_SYM, E_BAD_CODE, E_DIST_FAR, E_OUT_OVER, E_EXTENT, E_ISIZE, E_CRC, E_ADLER, E_COUNT
};
const char* const kErrText[E_COUNT] = {
    "ok",
    "not a gzip member (ID1, ID2, CM are not 1f 8b 08)",
    "reserved FLG bits are set",
    "the header runs past the end of the input",
    "bytes after the last member do not begin a member",
    "block type 3",
    "stored block with LEN != ~NLEN",
    "the input ends inside a block",
    "HLIT above 286",
    "HDIST above 30",
    "the code-length code is over-subscribed or incomplete",
    "code-length repeat with nothing before it",
    "code-length repeat runs past HLIT + HDIST",
    "no end-of-block code",
    "literal/length code lengths over-subscribe the code",
    "incomplete literal/length code",
    "distance code lengths over-subscribe the code",
    "incomplete distance code",
    "literal/length symbol 286 or 287",
    "distance symbol 30 or 31",
    "a bit pattern that is no code",
    "match distance beyond the bytes produced",
    "more output than the member's size allows",
    "the deflate data does not end at the trailer",
    "ISIZE does not match the bytes produced",
    "CRC-32 mismatch",
    "Adler-32 mismatch",
};

struct Result {                  // per member, written by k_gz_inflate and k_gz_crc_members
    uint32_t err;
    uint32_t stored, fixed, dynamic;
    uint64_t produced;
};

struct SizeHdr {                 // what k_gz_size leaves besides the table
    uint32_t err, pad;
    uint64_t members;            // found (the table holds the first `cap` of them)
    uint64_t bad_member, bad_off;
    uint64_t total;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v)
{
    return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}
__device__ __forceinline__ uint64_t lane64(uint64_t v, uint32_t j)   // lane j's v (j uniform)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
    return ((uint64_t)hi << 32) | lo;
}

// Orders this wave's LDS accesses across lanes: what any lane stored before is
// what every lane reads after.  The ring is written by one lane and read by
// others (a literal, then a match or a flush).
__device__ __forceinline__ void lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The wave's bit reader.  Everything but w is the same in every lane.
struct Bits {
    const uint8_t* in;           // the whole input, 8-byte aligned
    uint64_t cap;                // readable bytes of it, a multiple of 8
    uint64_t pos;                // byte offset of the next byte that enters bb
    uint64_t wbase;              // byte offset of the window, a multiple of 8
    uint64_t w;                  // this lane's 8 bytes of the window
    uint64_t bb;                 // bit buffer, next bit at bit 0
    uint32_t nb;                 // valid bits in bb
};

__device__ __forceinline__ void load_window(Bits& b, uint32_t lane)
{
    b.wbase = b.pos & ~7ull;
    const uint64_t off = b.wbase + 8ull * lane;
    b.w = off + 8 <= b.cap ? *reinterpret_cast<const uint64_t*>(b.in + off) : 0ull;
}
__device__ __forceinline__ void start_bits(Bits& b, uint64_t pos, uint32_t lane)
{
    b.pos = pos;
    b.bb = 0;
    b.nb = 0;
    load_window(b, lane);
}
// at least 56 valid bits afterwards (zeros past the readable bytes)
__device__ __forceinline__ void refill(Bits& b, uint32_t lane)
{
    if (b.nb >= 48) return;
    if (b.pos - b.wbase > 512 - 16) load_window(b, lane);
    const uint32_t k = uni((uint32_t)(b.pos - b.wbase));
    const uint32_t j = k >> 3, sh = (k & 7u) * 8u;
    const uint64_t lo = lane64(b.w, j), hi = lane64(b.w, j + 1);
    const uint64_t v = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
    b.bb |= v << b.nb;
    const uint32_t adv = (63u - b.nb) >> 3;
    b.pos += adv;
    b.nb += adv * 8u;
}
__device__ __forceinline__ void drop(Bits& b, uint32_t n) { b.bb >>= n; b.nb -= n; }
__device__ __forceinline__ uint32_t take(Bits& b, uint32_t n)   // n <= 16
{
    const uint32_t v = (uint32_t)b.bb & ((1u << n) - 1u);
    drop(b, n);
    return v;
}
__device__ __forceinline__ uint64_t bits_used(const Bits& b) { return b.pos * 8ull - b.nb; }   // absolute bit position

struct Lds {
    uint8_t ring[W];             // (first: 16-byte aligned)
    uint16_t lit[1u << PB_LIT];  // (symbol << 4) | length; 0: no code this short
    uint16_t dist[1u << PB_DIST];
    uint16_t cl[1u << PB_CL];
    uint16_t lit_long[288], dist_long[32];   // symbols of the codes longer than the primary tables, by (length, symbol)
    uint16_t lit_cnt[16], lit_first[16], lit_offs[16];
    uint16_t dist_cnt[16], dist_first[16], dist_offs[16];
    uint16_t cl_cnt[16], cl_first[16], cl_offs[16];
    uint8_t lens[320];           // code lengths: literal/length, then distance
    uint8_t cll[32];             // lengths of the code-length code
};

// A canonical Huffman decoder from the lengths lens[0, n), built by the wave:
// lanes 1..15 take one code length each.  Returns 0, 1 over-subscribed, 2
// incomplete (a code whose longest length is 1, or no code at all, is let
// through as zlib does unless `whole`: its unused patterns decode as errors).
// Always inlined: emitted out of line (a call through generic pointers, which
// hipcc chose at -O2 and -O3) the kernels decoded wrongly; DESIGN.md section 20.
template <uint32_t PB>
__device__ __forceinline__ uint32_t build_table(const uint8_t* lens, uint32_t n, uint16_t* tab, uint16_t* longs, uint16_t* cnt,
                                uint16_t* first, uint16_t* offs, bool whole, uint32_t lane)
{
    for (uint32_t i = lane; i < (1u << PB); i += 64) tab[i] = 0;
    if (lane < 16) {
        uint32_t c = 0;
        if (lane)
            for (uint32_t s = 0; s < n; ++s) c += lens[s] == lane ? 1u : 0u;
        cnt[lane] = (uint16_t)c;
    }
    __syncthreads();
    int left = 1;
    uint32_t code = 0, off = 0, maxl = 0, my_code = 0, my_off = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t c = uni(cnt[l]);
        left = left * 2 - (int)c;
        if (left < 0) return 1;
        if (l == lane) { my_code = code; my_off = off; }
        if (lane == 0) { first[l] = (uint16_t)code; offs[l] = (uint16_t)off; }
        if (l > PB) off += c;
        code = (code + c) << 1;
        if (c) maxl = l;
    }
    if (left > 0 && (whole || maxl > 1)) return 2;
    if (lane >= 1 && lane < 16 && cnt[lane]) {
        const uint32_t l = lane;
        for (uint32_t s = 0; s < n; ++s) {
            if (lens[s] != l) continue;
            const uint32_t c = my_code++;
            if (l <= PB) {
                const uint16_t e = (uint16_t)((s << 4) | l);
                for (uint32_t k = __brev(c) >> (32u - l); k < (1u << PB); k += 1u << l) tab[k] = e;
            } else if (longs) {
                longs[my_off++] = (uint16_t)s;
            }
        }
    }
    __syncthreads();
    return 0;
}

// the symbol whose code starts the bit buffer: (symbol << 4) | length, or 0 when the bits are no code
template <uint32_t PB>
__device__ __forceinline__ uint32_t decode_sym(const Bits& b, const uint16_t* tab, const uint16_t* longs,
                                               const uint16_t* cnt, const uint16_t* first, const uint16_t* offs)
{
    const uint32_t e = uni(tab[(uint32_t)b.bb & ((1u << PB) - 1u)]);
    if (e & 15u) return e;
    uint32_t code = __brev((uint32_t)b.bb & ((1u << PB) - 1u)) >> (32u - PB);
    for (uint32_t l = PB + 1; l < 16; ++l) {
        code = (code << 1) | ((uint32_t)(b.bb >> (l - 1)) & 1u);
        const uint32_t d = code - uni(first[l]);
        if (d < uni(cnt[l])) return ((uint32_t)uni(longs[uni(offs[l]) + d]) << 4) | l;
    }
    return 0;
}

__device__ __forceinline__ uint32_t wrap(uint32_t x) { return x >= W ? x - W : x; }

// The member's bytes [f, e) from the ring to out (its first output byte).  The
// ring index of byte q is (q + a) % W with a = the address of out mod 16, so a
// 16-byte piece is aligned in the ring and in HBM alike; rf is the index of f.
__device__ void flush(const uint8_t* ring, uint8_t* out, uint64_t& f, uint32_t& rf, uint64_t e, uint32_t lane)
{
    lds_order();
    uint64_t q = f;
    uint32_t r = rf;
    uint32_t head = (16u - (r & 15u)) & 15u;
    if ((uint64_t)head > e - q) head = (uint32_t)(e - q);
    if (lane < head) out[q + lane] = ring[r + lane];
    q += head;
    r = wrap(r + head);
    const uint32_t n16 = (uint32_t)((e - q) >> 4);
    for (uint32_t c = lane; c < n16; c += 64) {
        const uint32_t ri = wrap(r + 16u * c);
        *reinterpret_cast<uint4*>(out + q + 16ull * c) = *reinterpret_cast<const uint4*>(ring + ri);
    }
    q += 16ull * n16;
    r = wrap(r + 16u * n16);
    const uint32_t tail = (uint32_t)(e - q);
    if (lane < tail) out[q + lane] = ring[r + lane];
    lds_order();
    f = e;
    rf = wrap(r + tail);
}

// One member's deflate data, from the reader's position; it must end at or
// before byte end_byte of the input.  COPY: the bytes go to out[0, cap) through
// the ring; else lengths are summed only.  Returns the error; *produced: the
// bytes.  nblk[0..2]: stored, fixed and dynamic blocks.
template <bool COPY>
__device__ uint32_t inflate_body(Bits& b, uint64_t end_byte, Lds& L, uint8_t* out, uint64_t cap, uint64_t* produced,
                                 uint32_t* nblk, uint32_t lane)
{
    static constexpr uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
                                              67, 83, 99, 115, 131, 163, 195, 227, 258};
    static constexpr uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static constexpr uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513,
                                               769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static constexpr uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10,
                                               11, 11, 12, 12, 13, 13};
    static constexpr uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const uint64_t end_bits = end_byte * 8ull;
    const uint32_t a = COPY ? (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u) : 0u;
    uint64_t p = 0, f = 0;       // bytes produced, bytes flushed
    uint32_t rp = a, rf = a;     // their ring indices
    bool have_fixed = false;
    *produced = 0;
    for (;;) {
        refill(b, lane);
        const uint32_t bfinal = take(b, 1), btype = take(b, 2);
        if (bits_used(b) > end_bits) return E_TRUNC;
        if (btype == 3) return E_BTYPE;
        if (btype == 0) {
            drop(b, b.nb & 7u);
            refill(b, lane);
            const uint32_t len = take(b, 16), nlen = take(b, 16);
            if (bits_used(b) > end_bits) return E_TRUNC;
            if (len != (nlen ^ 0xffffu)) return E_STORED_LEN;
            const uint64_t sp = b.pos - (b.nb >> 3);    // nb is a multiple of 8 here
            if (sp + len > end_byte) return E_TRUNC;
            if (p + len > cap) return E_OUT_OVER;
            for (uint32_t done = 0; done < len;) {
                const uint32_t c = len - done < 256u ? len - done : 256u;
                if (COPY) {
                    for (uint32_t k = lane; k < c; k += 64) L.ring[wrap(rp + k)] = b.in[sp + done + k];
                    rp = wrap(rp + c);
                }
                p += c;
                done += c;
                if (COPY && p - f >= kFlushBytes) flush(L.ring, out, f, rf, p - (rp & 15u), lane);
            }
            start_bits(b, sp + len, lane);
            ++nblk[0];
        } else {
            if (btype == 1) {
                if (!have_fixed) {
                    for (uint32_t s = lane; s < 320; s += 64)
                        L.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                    __syncthreads();
                    build_table<PB_LIT>(L.lens, 288, L.lit, L.lit_long, L.lit_cnt, L.lit_first, L.lit_offs, false, lane);
                    build_table<PB_DIST>(L.lens + 288, 32, L.dist, L.dist_long, L.dist_cnt, L.dist_first, L.dist_offs,
                                         false, lane);
                    have_fixed = true;
                }
                ++nblk[1];
            } else {
                have_fixed = false;
                refill(b, lane);
                const uint32_t hlit = take(b, 5) + 257u, hdist = take(b, 5) + 1u, hclen = take(b, 4) + 4u;
                if (bits_used(b) > end_bits) return E_TRUNC;
                if (hlit > 286) return E_HLIT;
                if (hdist > 30) return E_HDIST;
                if (lane < 32) L.cll[lane] = 0;
                __syncthreads();
                for (uint32_t i = 0; i < hclen; ++i) {
                    refill(b, lane);
                    const uint32_t v = take(b, 3);
                    if (lane == 0) L.cll[ord[i]] = (uint8_t)v;
                }
                if (bits_used(b) > end_bits) return E_TRUNC;
                __syncthreads();
                if (build_table<PB_CL>(L.cll, 19, L.cl, nullptr, L.cl_cnt, L.cl_first, L.cl_offs, true, lane))
                    return E_CL_SET;
                const uint32_t tot = hlit + hdist;
                uint32_t prev = 0;
                for (uint32_t i = 0; i < tot;) {
                    refill(b, lane);
                    const uint32_t e = uni(L.cl[(uint32_t)b.bb & ((1u << PB_CL) - 1u)]);
                    if (!(e & 15u)) return E_BAD_CODE;
                    drop(b, e & 15u);
                    const uint32_t sym = e >> 4;
                    uint32_t rep = 1, val = sym;
                    if (sym == 16) {
                        if (i == 0) return E_REP_FIRST;
                        rep = 3u + take(b, 2);
                        val = prev;
                    } else if (sym == 17) {
                        rep = 3u + take(b, 3);
                        val = 0;
                    } else if (sym == 18) {
                        rep = 11u + take(b, 7);
                        val = 0;
                    }
                    if (bits_used(b) > end_bits) return E_TRUNC;
                    if (i + rep > tot) return E_REP_PAST;
                    for (uint32_t k = lane; k < rep; k += 64) L.lens[i + k] = (uint8_t)val;
                    prev = val;
                    i += rep;
                }
                __syncthreads();
                if (uni(L.lens[256]) == 0) return E_NO_EOB;
                uint32_t r = build_table<PB_LIT>(L.lens, hlit, L.lit, L.lit_long, L.lit_cnt, L.lit_first, L.lit_offs,
                                                 false, lane);
                if (r) return r == 1 ? E_LIT_OVER : E_LIT_INCOMPLETE;
                r = build_table<PB_DIST>(L.lens + hlit, hdist, L.dist, L.dist_long, L.dist_cnt, L.dist_first,
                                         L.dist_offs, false, lane);
                if (r) return r == 1 ? E_DIST_OVER : E_DIST_INCOMPLETE;
                ++nblk[2];
            }
            for (;;) {               // the block's symbols; an iteration needs at most 48 bits
                refill(b, lane);
                const uint32_t e = decode_sym<PB_LIT>(b, L.lit, L.lit_long, L.lit_cnt, L.lit_first, L.lit_offs);
                if (!e) return E_BAD_CODE;
                drop(b, e & 15u);
                const uint32_t sym = e >> 4;
                if (sym < 256) {
                    if (p >= cap) return E_OUT_OVER;
                    if (COPY) {
                        if (lane == 0) L.ring[rp] = (uint8_t)sym;
                        rp = wrap(rp + 1);
                    }
                    ++p;
                } else if (sym == 256) {
                    if (bits_used(b) > end_bits) return E_TRUNC;
                    break;
                } else {
                    if (sym > 285) return E_LIT_SYM;
                    const uint32_t ls = sym - 257u;
                    const uint32_t len = len_base[ls] + take(b, len_extra[ls]);
                    const uint32_t de = decode_sym<PB_DIST>(b, L.dist, L.dist_long, L.dist_cnt, L.dist_first, L.dist_offs);
                    if (!de) return E_BAD_CODE;
                    drop(b, de & 15u);
                    const uint32_t ds = de >> 4;
                    if (ds > 29) return E_DIST_SYM;
                    const uint32_t dist = dist_base[ds] + take(b, dist_extra[ds]);
                    if (bits_used(b) > end_bits) return E_TRUNC;
                    if (dist > p) return E_DIST_FAR;
                    if (p + len > cap) return E_OUT_OVER;
                    if (COPY) {
                        lds_order();
                        const uint32_t src0 = rp >= dist ? rp - dist : rp + W - dist;
                        for (uint32_t k = lane; k < len; k += kCopyWidth) {
                            const uint32_t o = k < dist ? k : k % dist;
                            L.ring[wrap(rp + k)] = L.ring[wrap(src0 + o)];
                        }
                        rp = wrap(rp + len);
                    }
                    p += len;
                }
                if (bits_used(b) > end_bits) return E_TRUNC;
                if (COPY && p - f >= kFlushBytes) flush(L.ring, out, f, rf, p - (rp & 15u), lane);
            }
        }
        if (bfinal) break;
    }
    if (COPY && p > f) flush(L.ring, out, f, rf, p, lane);
    *produced = p;
    return E_OK;
}

__global__ void __launch_bounds__(64) k_gz_inflate(const uint8_t* __restrict__ in, uint64_t in_cap,
                                                   const Member* __restrict__ tab, uint32_t nmem,
                                                   uint8_t* __restrict__ out, Result* __restrict__ res)
{
    __shared__ __attribute__((aligned(16))) Lds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t m = blockIdx.x; m < nmem; m += gridDim.x) {
        const Member mb = tab[m];
        Bits b;
        b.in = in;
        b.cap = in_cap;
        start_bits(b, mb.in_off + mb.hdr_len, lane);
        uint32_t nblk[3] = {0, 0, 0};
        uint64_t produced = 0;
        const uint64_t end_byte = mb.in_off + mb.in_len - 8;
        uint32_t err = inflate_body<true>(b, end_byte, L, out + mb.out_off, mb.out_len, &produced, nblk, lane);
        if (!err && (bits_used(b) + 7) / 8 != end_byte) err = E_EXTENT;
        if (!err && (produced != mb.out_len || (uint32_t)produced != mb.isize)) err = E_ISIZE;
        if (lane == 0) res[m] = Result{err, nblk[0], nblk[1], nblk[2], produced};
        __syncthreads();             // the next member reuses the tables and the ring
    }
}

// Generic gzip: the chain of members walked by one wave.  No copies, no
// window: lengths are summed.  tab[0, cap) receives the first cap members.
__global__ void __launch_bounds__(64) k_gz_size(const uint8_t* __restrict__ in, uint64_t in_cap, uint64_t n,
                                                Member* __restrict__ tab, uint64_t cap, SizeHdr* __restrict__ hdr)
{
    __shared__ __attribute__((aligned(16))) Lds L;
    const uint32_t lane = threadIdx.x;
    uint64_t pos = 0, m = 0, out_off = 0;
    uint32_t err = E_OK;
    while (pos < n) {
        if (n - pos < 18) { err = E_TRAILING; break; }
        if (in[pos] != 0x1f || in[pos + 1] != 0x8b || in[pos + 2] != 8) { err = m ? E_TRAILING : E_MAGIC; break; }
        const uint32_t flg = in[pos + 3];
        if (flg & 0xe0u) { err = E_FLG; break; }
        const uint64_t lim = n - 8;          // the deflate data starts at or before it
        uint64_t h = pos + 10;
        if (flg & 4u) {                      // FEXTRA
            if (h + 2 > lim) { err = E_HDR_TRUNC; break; }
            h += 2ull + ((uint32_t)in[h] | ((uint32_t)in[h + 1] << 8));
        }
        for (uint32_t bit = 8; bit <= 16 && h <= lim; bit <<= 1) {   // FNAME, FCOMMENT: to the zero byte, 64 bytes a step
            if (!(flg & bit)) continue;
            for (;;) {
                const uint64_t q = h + lane;
                const uint64_t z = __ballot(q < lim && in[q] == 0);
                if (z) { h += (uint64_t)__builtin_ctzll(z) + 1; break; }
                h += 64;
                if (h > lim) break;
            }
        }
        if (flg & 2u) h += 2;                // FHCRC (skipped, not verified)
        if (h > lim) { err = E_HDR_TRUNC; break; }
        h = uni64(h);
        Bits b;
        b.in = in;
        b.cap = in_cap;
        start_bits(b, h, lane);
        uint32_t nblk[3] = {0, 0, 0};
        uint64_t produced = 0;
        err = inflate_body<false>(b, lim, L, nullptr, ~0ull, &produced, nblk, lane);
        if (err) break;
        const uint64_t t = (bits_used(b) + 7) / 8;   // the trailer; t + 8 <= n
        const uint32_t crc = (uint32_t)in[t] | ((uint32_t)in[t + 1] << 8) | ((uint32_t)in[t + 2] << 16) | ((uint32_t)in[t + 3] << 24);
        const uint32_t isz = (uint32_t)in[t + 4] | ((uint32_t)in[t + 5] << 8) | ((uint32_t)in[t + 6] << 16) | ((uint32_t)in[t + 7] << 24);
        if ((uint32_t)produced != isz) { err = E_ISIZE; break; }
        if (m < cap && lane == 0) tab[m] = Member{pos, t + 8 - pos, out_off, produced, crc, isz, (uint32_t)(h - pos), 0};
        ++m;
        out_off += produced;
        pos = t + 8;
        __syncthreads();
    }
    if (lane == 0) *hdr = SizeHdr{err, 0, m, m, pos, out_off};
}

// CRC register of every 4 KiB piece of every member's output: one wave per
// piece, a 64-byte strip per lane, the strips folded over the lanes in order.
// Piece c belongs to the member m with chunk0[m] <= c < chunk0[m + 1].
__global__ void __launch_bounds__(64) k_gz_crc_chunks(const uint8_t* __restrict__ out, const Member* __restrict__ tab,
                                                      const uint32_t* __restrict__ chunk0, uint32_t nmem,
                                                      uint32_t* __restrict__ creg)
{
    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    uint32_t lo = 0, hi = nmem - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const Member mb = tab[lo];
    const uint64_t beg = (uint64_t)(c - chunk0[lo]) * CRC_CHUNK;
    const uint32_t len = (uint32_t)(mb.out_len - beg < CRC_CHUNK ? mb.out_len - beg : CRC_CHUNK);
    const uint8_t* src = out + mb.out_off + beg;
    uint32_t r = 0;
    const uint32_t sb = lane * 64u, se = sb + 64u < len ? sb + 64u : (sb < len ? len : sb);
    for (uint32_t i = sb; i < se; ++i) r = (r >> 8) ^ c_crc_tab[(r ^ src[i]) & 0xffu];
    uint64_t slen = se - sb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {          // combine with the strip d lanes before (lengths grow with d)
        const uint32_t ro = (uint32_t)__shfl_up((int)r, d, 64);
        const uint32_t lo2 = (uint32_t)__shfl_up((int)(uint32_t)slen, d, 64);
        if ((int)lane >= d && lane % (2 * d) == 2 * d - 1) {
            r = crc_cat(ro, r, slen);
            slen += lo2;
        }
    }
    if (lane == 63) creg[c] = r;
}

// per member: its pieces' registers folded (each thread a run of pieces, then
// a tree over threads) and compared with the trailer
__global__ void __launch_bounds__(256) k_gz_crc_members(const Member* __restrict__ tab,
                                                        const uint32_t* __restrict__ chunk0,
                                                        const uint32_t* __restrict__ creg, Result* __restrict__ res)
{
    __shared__ uint32_t rs[256];
    __shared__ uint64_t ls[256];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const uint64_t total = tab[s].out_len;
    const uint32_t a = chunk0[s], e = chunk0[s + 1], nb = e - a;
    const uint32_t per = (nb + 255) / 256;
    const uint64_t b0 = (uint64_t)a + (uint64_t)tid * per, b1 = b0 + per < e ? b0 + per : e;
    uint32_t r = 0;
    uint64_t l = 0;
    for (uint64_t b = b0; b < b1; ++b) {
        const uint64_t beg = (b - a) * CRC_CHUNK;
        const uint64_t len = total - beg < CRC_CHUNK ? total - beg : CRC_CHUNK;
        r = crc_cat(r, creg[b], len);
        l += len;
    }
    rs[tid] = r;
    ls[tid] = l;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        if (tid % (2 * d) == 0 && tid + d < 256) {
            rs[tid] = crc_cat(rs[tid], rs[tid + d], ls[tid + d]);
            ls[tid] += ls[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0 && res[s].err == E_OK && ~(rs[0] ^ gf_mul(0xFFFFFFFFu, x8n(total))) != tab[s].crc) res[s].err = E_CRC;
}

// ---- a caller-made table (TableInflater): zlib blocks, or any framing around raw deflate data ----
// One wave per member, as k_gz_inflate: the deflate data begins hdr_len bytes into
// the member and must end exactly `trailer` bytes before its end.  out_len is the
// member's slot: a member that would inflate past it ends in E_OUT_OVER and has
// written nothing behind the slot.  Without COPY nothing is written at all and
// res[m].produced is what the member inflates to (the sizing walk).
template <bool COPY>
__global__ void __launch_bounds__(64) k_tab_inflate(const uint8_t* __restrict__ in, uint64_t in_cap,
                                                    const Member* __restrict__ tab, uint32_t nmem, uint32_t trailer,
                                                    uint8_t* __restrict__ out, TableResult* __restrict__ res)
{
    __shared__ __attribute__((aligned(16))) Lds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t m = blockIdx.x; m < nmem; m += gridDim.x) {
        const Member mb = tab[m];
        Bits b;
        b.in = in;
        b.cap = in_cap;
        start_bits(b, mb.in_off + mb.hdr_len, lane);
        uint32_t nblk[3] = {0, 0, 0};
        uint64_t produced = 0;
        const uint64_t end_byte = mb.in_off + mb.in_len - trailer;   // (the host made in_len >= hdr_len + trailer)
        uint32_t err = inflate_body<COPY>(b, end_byte, L, COPY ? out + mb.out_off : nullptr, mb.out_len, &produced, nblk, lane);
        if (!err && (bits_used(b) + 7) / 8 != end_byte) err = E_EXTENT;
        if (lane == 0) res[m] = TableResult{err, 0, produced};
        __syncthreads();             // the next member reuses the tables and the ring
    }
}

// Adler-32 of every good member's output against tab[m].crc: one wave per
// member, piece after piece of kAdlerPiece bytes, every piece summed in the
// lanes' shares and folded (gz_adler.hpp).
__global__ void __launch_bounds__(64) k_tab_adler(const uint8_t* __restrict__ out, const Member* __restrict__ tab, uint32_t nmem,
                                                  TableResult* __restrict__ res)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t m = blockIdx.x; m < nmem; m += gridDim.x) {
        if (res[m].err) continue;
        const uint64_t n = res[m].produced;
        const uint8_t* x = out + tab[m].out_off;
        AdlerSum s{0, 0, 0};
        for (uint64_t at = 0; at < n; at += kAdlerPiece) {
            const uint32_t len = (uint32_t)(n - at < kAdlerPiece ? n - at : kAdlerPiece);
            uint64_t a = 0, w = 0;
            adler_share(x + at, len, lane, &a, &w);
            a = wave_reduce_add<uint64_t>(a);
            w = wave_reduce_add<uint64_t>(w);
            s = adler_fold(s, adler_piece(a, w, len));
        }
        if (lane == 0 && adler_value(s) != tab[m].crc) res[m].err = E_ADLER;
    }
}

[[noreturn]] void bad_member(uint64_t k, uint64_t off, uint32_t err)
{
    throw StarchError(-12, "gunzip: member " + std::to_string(k) + " at byte " + std::to_string(off) + ": " +
                               (err < E_COUNT ? std::string(kErrText[err]) : "error word " + std::to_string(err)));
}

uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

}  // namespace

bool plan_bgzf(const uint8_t* gz, uint64_t n, std::vector<Member>& table)
{
    table.clear();
    uint64_t pos = 0, out_off = 0;
    while (pos < n) {
        const uint64_t k = table.size();
        if (n - pos < 18) bad_member(k, pos, E_TRAILING);
        const uint8_t* m = gz + pos;
        if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8) bad_member(k, pos, k ? E_TRAILING : E_MAGIC);
        const uint32_t flg = m[3];
        if (flg & 0xe0u) bad_member(k, pos, E_FLG);
        if (!(flg & 4u)) { table.clear(); return false; }
        const uint64_t left = n - pos;
        if (12 > left - 8) bad_member(k, pos, E_HDR_TRUNC);
        const uint64_t xlen = rd16(m + 10);
        uint64_t h = 12 + xlen;
        if (h > left - 8) bad_member(k, pos, E_HDR_TRUNC);
        int64_t bsize = -1;
        for (uint64_t x = 12; x + 4 <= 12 + xlen;) {   // the subfields: SI1 SI2 SLEN data
            const uint64_t slen = rd16(m + x + 2);
            if (x + 4 + slen > 12 + xlen) break;
            if (m[x] == 66 && m[x + 1] == 67 && slen == 2) { bsize = rd16(m + x + 4); break; }
            x += 4 + slen;
        }
        if (bsize < 0) { table.clear(); return false; }
        for (uint32_t bit = 8; bit <= 16; bit <<= 1) {   // FNAME, FCOMMENT
            if (!(flg & bit)) continue;
            while (h < left - 8 && m[h]) ++h;
            ++h;
        }
        if (flg & 2u) h += 2;                            // FHCRC (skipped, not verified)
        const uint64_t len = (uint64_t)bsize + 1;
        if (len > left) bad_member(k, pos, E_TRUNC);
        if (h + 8 > len) bad_member(k, pos, E_HDR_TRUNC);
        Member mb{};
        mb.in_off = pos;
        mb.in_len = len;
        mb.out_off = out_off;
        mb.crc = rd32(m + len - 8);
        mb.isize = rd32(m + len - 4);
        mb.out_len = mb.isize;
        mb.hdr_len = (uint32_t)h;
        if (mb.isize > kBgzfMax) bad_member(k, pos, E_OUT_OVER);
        table.push_back(mb);
        out_off += mb.isize;
        pos += len;
    }
    return true;
}

uint64_t Inflater::plan(const uint8_t* h_in, const uint8_t* d_in, uint64_t n, hipStream_t st)
{
    stats = InflateStats{};
    table_.clear();
    d_in_ = d_in;
    n_ = n;
    if (!is_gzip(h_in, n)) bad_member(0, 0, n >= 18 ? E_MAGIC : E_HDR_TRUNC);
    if ((reinterpret_cast<uintptr_t>(d_in) & 7u) != 0) throw StarchError(-2, "gunzip: the device input must be 8-byte aligned");
    const auto t0 = std::chrono::steady_clock::now();
    const bool bgzf = plan_bgzf(h_in, n, table_);
    stats.ms_plan = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats.is_bgzf = bgzf ? 1 : 0;
    stats.bytes_in = n;
    if (!bgzf) {
        upload_crc_tables();
        StageTimer<2> tm;
        tm.start(st);
        uint64_t cap = std::max<uint64_t>(4096, b_table.cap / sizeof(Member));
        SizeHdr h{};
        for (int pass = 0; pass < 2; ++pass) {
            Member* d_tab = b_table.as<Member>(cap);
            SizeHdr* d_hdr = b_cnt.as<SizeHdr>(1);
            hipLaunchKernelGGL(k_gz_size, dim3(1), dim3(64), 0, st, d_in, (n + kInPad) & ~7ull, n, d_tab, cap, d_hdr);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (h.err) bad_member(h.bad_member, h.bad_off, h.err);
            if (h.members <= cap) break;
            cap = h.members;
        }
        float ms = 0;
        tm.finish(1, st, {&ms});
        stats.ms_size = ms;
        table_.resize(h.members);
        if (h.members)
            HIP_CHECK(hipMemcpy(table_.data(), b_table.p, h.members * sizeof(Member), hipMemcpyDeviceToHost));
    }
    if (table_.size() >= (1ull << 31)) throw StarchError(-2, "gunzip: 2^31 members or more");
    uint64_t total = 0;
    for (const Member& m : table_) total += m.out_len;
    stats.members = table_.size();
    stats.bytes_out = total;
    return total;
}

void Inflater::inflate(uint8_t* d_out, hipStream_t st)
{
    const uint32_t nmem = (uint32_t)table_.size();
    if (!nmem) return;
    upload_crc_tables();
    std::vector<uint32_t> chunk0(nmem + 1, 0);
    uint64_t nchunk = 0;
    for (uint32_t m = 0; m < nmem; ++m) {
        chunk0[m] = (uint32_t)nchunk;
        nchunk += ceil_div(table_[m].out_len, CRC_CHUNK);
    }
    if (nchunk >= (1ull << 32)) throw StarchError(-2, "gunzip: output too large (16 TiB or more)");
    chunk0[nmem] = (uint32_t)nchunk;
    Member* d_tab = b_table.as<Member>(nmem);   // (the sizing launch's copy may be gone: the host's is uploaded)
    Result* d_res = b_res.as<Result>(nmem);
    uint32_t* d_chunk0 = b_chunk0.as<uint32_t>(nmem + 1);
    uint32_t* d_creg = b_creg.as<uint32_t>(nchunk);
    HIP_CHECK(hipMemcpyAsync(d_tab, table_.data(), nmem * sizeof(Member), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_chunk0, chunk0.data(), (nmem + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t grid = std::min<uint32_t>(nmem, (uint32_t)std::max(cus, 1) * 4u);   // four one-wave workgroups fit a CU's LDS
    StageTimer<3> tm;
    tm.start(st);
    hipLaunchKernelGGL(k_gz_inflate, dim3(grid), dim3(64), 0, st, d_in_, (n_ + kInPad) & ~7ull, d_tab, nmem, d_out,
                       d_res);
    HIP_CHECK(hipGetLastError());
    tm.mark(1, st);
    if (nchunk)
        hipLaunchKernelGGL(k_gz_crc_chunks, dim3((uint32_t)nchunk), dim3(64), 0, st, d_out, d_tab, d_chunk0, nmem, d_creg);
    hipLaunchKernelGGL(k_gz_crc_members, dim3(nmem), dim3(256), 0, st, d_tab, d_chunk0, d_creg, d_res);
    HIP_CHECK(hipGetLastError());
    std::vector<Result> res(nmem);
    HIP_CHECK(hipMemcpyAsync(res.data(), d_res, nmem * sizeof(Result), hipMemcpyDeviceToHost, st));
    tm.finish(2, st, {&stats.ms_inflate, &stats.ms_crc});
    for (uint32_t m = 0; m < nmem; ++m)
        if (res[m].err) bad_member(m, table_[m].in_off, res[m].err);
    for (const Result& r : res) {
        stats.stored_blocks += r.stored;
        stats.fixed_blocks += r.fixed;
        stats.dynamic_blocks += r.dynamic;
    }
}

const char* inflate_error_text(uint32_t err) { return err < E_COUNT ? kErrText[err] : "unknown error word"; }

void TableInflater::run(const uint8_t* d_in, uint64_t n, const std::vector<Member>& tab, uint32_t trailer, bool copy, bool adler,
                        uint8_t* d_out, hipStream_t st, std::vector<TableResult>& res)
{
    const uint32_t nmem = (uint32_t)tab.size();
    res.assign(nmem, TableResult{});
    ms_inflate = ms_check = 0;
    if (!nmem) return;
    if (tab.size() >= (1ull << 31)) throw StarchError(-2, "inflate: 2^31 members or more");
    if ((reinterpret_cast<uintptr_t>(d_in) & 7u) != 0) throw StarchError(-2, "inflate: the device input must be 8-byte aligned");
    for (const Member& m : tab)
        if (m.in_off + m.in_len > n || m.in_len < (uint64_t)m.hdr_len + trailer)
            throw StarchError(-2, "inflate: a member of the table lies outside the input or is shorter than its framing");
    Member* d_tab = b_table.as<Member>(nmem);
    TableResult* d_res = b_res.as<TableResult>(nmem);
    HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), nmem * sizeof(Member), hipMemcpyHostToDevice, st));
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t grid = std::min<uint32_t>(nmem, (uint32_t)std::max(cus, 1) * 4u);   // four one-wave workgroups fit a CU's LDS
    const uint64_t in_cap = (n + kInPad) & ~7ull;
    tm_.start(st);
    if (copy) hipLaunchKernelGGL(k_tab_inflate<true>, dim3(grid), dim3(64), 0, st, d_in, in_cap, d_tab, nmem, trailer, d_out, d_res);
    else hipLaunchKernelGGL(k_tab_inflate<false>, dim3(grid), dim3(64), 0, st, d_in, in_cap, d_tab, nmem, trailer, d_out, d_res);
    HIP_CHECK(hipGetLastError());
    tm_.mark(1, st);
    if (copy && adler) {
        hipLaunchKernelGGL(k_tab_adler, dim3(std::min<uint32_t>(nmem, 65536u)), dim3(64), 0, st, d_out, d_tab, nmem, d_res);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(res.data(), d_res, nmem * sizeof(TableResult), hipMemcpyDeviceToHost, st));
    tm_.finish(2, st, {&ms_inflate, &ms_check});
}

}  // namespace gz
