// starch_amd/csrc/gz_inflate.hpp -- gzip and BGZF inputs inflated on the GPU
// (gz_inflate.hip).  Two phases, as the encoders and bz::Decoder have them:
// plan() makes the member table and sizes the output, inflate() decodes every
// member into the caller's HBM and checks its CRC-32 and ISIZE.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

namespace gz {

constexpr uint32_t kWindowBytes = 34u << 10;   // the LDS ring: 32 KiB of history plus what is in flight
constexpr uint32_t kFlushBytes = 1024;         // unflushed bytes from which the ring is written out
constexpr uint32_t kPrimaryBits = 10;          // codes up to this length decode by one table lookup
constexpr uint32_t kCopyWidth = 64;            // bytes of a match copied per round (one per lane)
constexpr uint32_t kBgzfMax = 65536;           // most bytes a BGZF member inflates to
constexpr uint32_t kInPad = 64;                // readable zero bytes the caller leaves after the input

struct Member {                  // one gzip member (host and device)
    uint64_t in_off;             // its first header byte
    uint64_t in_len;             // header, deflate data and trailer
    uint64_t out_off;            // exclusive sum of the members' sizes
    uint64_t out_len;            // BGZF: ISIZE (a capacity until decoded); generic: what the sizing walk counted
    uint32_t crc, isize;         // the trailer
    uint32_t hdr_len;            // bytes before the deflate data
    uint32_t pad;
};

struct InflateStats {
    uint64_t members = 0, is_bgzf = 0;
    uint64_t stored_blocks = 0, fixed_blocks = 0, dynamic_blocks = 0;
    uint64_t bytes_in = 0, bytes_out = 0;
    float ms_plan = 0, ms_upload = 0, ms_size = 0, ms_inflate = 0, ms_crc = 0;
};

// an input of at least 18 bytes that begins 1f 8b 08
inline bool is_gzip(const void* p, uint64_t n)
{
    const uint8_t* a = static_cast<const uint8_t*>(p);
    return n >= 18 && a[0] == 0x1f && a[1] == 0x8b && a[2] == 8;
}

// The member table of a BGZF input from its headers alone (host; no device).
// Returns false, with the table empty, when some member lacks the BC
// subfield: generic gzip.  Throws StarchError(-12) for a malformed header, a
// BSIZE past the input, an ISIZE above 65536 and bytes that begin no member.
bool plan_bgzf(const uint8_t* gz, uint64_t n, std::vector<Member>& table);

class Inflater {
public:
    // h_in[0, n): the input; d_in: the same bytes in HBM, 8-byte aligned, with
    // kInPad readable bytes after them.  Returns the inflated size.  BGZF is
    // planned on the host; generic gzip by a sizing launch on st.
    uint64_t plan(const uint8_t* h_in, const uint8_t* d_in, uint64_t n, hipStream_t st);
    // every member of the plan into d_out[0, planned size); throws -12 naming the first bad member
    void inflate(uint8_t* d_out, hipStream_t st);
    const std::vector<Member>& table() const { return table_; }
    InflateStats stats;

private:
    std::vector<Member> table_;
    const uint8_t* d_in_ = nullptr;
    uint64_t n_ = 0;
    DevBuf b_table, b_res, b_chunk0, b_creg, b_cnt;
};

// ---- a caller-made member table: raw deflate data inside any framing (the zlib blocks of a bigWig / bigBed file) ----
struct TableResult {             // per member
    uint32_t err, pad;           // 0, or an error word: inflate_error_text
    uint64_t produced;           // the bytes it inflates to
};
const char* inflate_error_text(uint32_t err);

// The inflater's decoder over a table the caller made, one wave per member.
// Of a Member: in_off, in_len and hdr_len frame the deflate data, which must end
// exactly `trailer` bytes before the member's end (8 for gzip, 4 for zlib);
// out_off and out_len are the member's slot in d_out: a member that inflates past
// out_len is an error and writes nothing behind its slot; crc is the Adler-32
// expected of the output when adler is set (RFC 1950's trailer, which the caller
// reads: it is big-endian).  isize is unused.
class TableInflater {
public:
    // d_in: the input in HBM, 8-byte aligned, n bytes with kInPad readable zero
    // bytes after them.  copy false: the sizing walk, nothing is written and
    // d_out may be NULL.  res[m]: the member's error word and size.  Throws only
    // for a table that does not fit the input.
    void run(const uint8_t* d_in, uint64_t n, const std::vector<Member>& tab, uint32_t trailer, bool copy, bool adler,
             uint8_t* d_out, hipStream_t st, std::vector<TableResult>& res);
    float ms_inflate = 0, ms_check = 0;

private:
    DevBuf b_table, b_res;
    StageTimer<3> tm_;
};

}  // namespace gz
