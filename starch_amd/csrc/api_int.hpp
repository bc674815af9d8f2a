// starch_amd/csrc/api_int.hpp -- what the files behind the C ABI
// (include/starch_amd.h) share: api_core.hip, api_archive.cpp, api_encode.hip,
// api_stream.hip, api_decode.hip, api_cat.hip, api_bed.hip, api_gunzip.hip, and gather.hip for
// the device guard and install_archive.  Declarations and a few inline helpers
// (the guards, Caught); each function names the file that defines it.  Everything here has hidden visibility: none of it is a symbol
// of the shared library.
#pragma once
#include "ctx.hpp"

#pragma GCC visibility push(hidden)
namespace api {

using archive::build_index;
using archive::kMagic;

// STARCH_TRACE=1: host-side timeline of the batched paths on stderr (api_core.hip)
double trace_t0();
bool tracing();
#define STRACE(...)                                                              \
    do {                                                                         \
        if (api::tracing()) {                                                    \
            fprintf(stderr, "[starch %9.3f ms] ", api::trace_t0());              \
            fprintf(stderr, __VA_ARGS__);                                        \
            fputc('\n', stderr);                                                \
        }                                                                        \
    } while (0)

inline int fail(starch_ctx* c, const StarchError& e)
{
    if (c) c->err = e.what();
    return e.code;
}

struct Ctx {   // device guard
    int prev = -1;
    explicit Ctx(int device) { (void)hipGetDevice(&prev); (void)hipSetDevice(device); }
    explicit Ctx(starch_ctx* c) : Ctx(c->device) {}
    ~Ctx() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define GUARD(c)                                         \
    if (!(c)) return STARCH_ERR_ARG;                     \
    try {                                                \
        api::Ctx _g(c);
#define END_GUARD(c)                                     \
    }                                                    \
    catch (const StarchError& e) { return api::fail(c, e); }  \
    catch (const std::exception& e) { (c)->err = e.what(); return STARCH_ERR_INTERNAL; }

// A worker's error, kept until every worker has been joined: run() records
// what f throws, rethrow() throws it again.  Anything else passes through run().
struct Caught {
    int code = 0;
    std::string msg;
    template <class F> void run(F&& f)
    {
        try { f(); }
        catch (const StarchError& e) { code = e.code; msg = e.what(); }
        catch (const std::exception& e) { code = STARCH_ERR_INTERNAL; msg = e.what(); }
    }
    void rethrow(const std::string& prefix = "") const;   // (api_encode.hip)
};

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// the result that starch_output_* hands out: the first `bytes` bytes of `buf`
inline void publish(starch_ctx* c, const DevBuf& buf, uint64_t bytes)
{
    c->out_dev = static_cast<const uint8_t*>(buf.p);
    c->out_bytes = bytes;
    c->have_out = true;
}

// the caller's options, or the defaults
inline starch_options options_of(const starch_options* opt)
{
    starch_options o;
    starch_options_init(&o);
    return opt ? *opt : o;
}
// block size 1 to 9, method bzip2 or gzip: what every encode entry point asks of them
inline bool options_ok(const starch_options& o)
{
    return o.block_size_100k >= 1 && o.block_size_100k <= 9 &&
           (o.compression_method == STARCH_METHOD_BZIP2 || o.compression_method == STARCH_METHOD_GZIP);
}

// ---- api_archive.cpp: the index writer's string escape and the index reader ----
void json_str(std::string& o, const char* p, size_t n, bool keep_utf8 = false);

struct IndexEntry {
    std::string chr;
    uint64_t offset, size;
    uint64_t line_count = 0, text_bytes = 0;
    uint32_t n_blocks = 0, combined_crc = 0;
    bool has_base_counts = false;
    int64_t base_unique = 0, base_nonunique = 0;
};
struct ArchiveInfo {
    std::string format;          // "compressionFormat"
    int block_size_100k = 0;
    std::string note;            // UTF-8
};
std::vector<IndexEntry> read_index(const uint8_t* a, uint64_t n, uint64_t* index_off, ArchiveInfo* info = nullptr);
// build_index over segs and their names, with the options' note, level, base counts and method
std::string index_of(const std::vector<starch_segment>& segs, const std::vector<std::string>& names, uint64_t index_off,
                     const starch_options& opt);
void check_bounds(const std::vector<IndexEntry>& idx, uint64_t index_off);

// ---- api_encode.hip: transform + compression over units ----
struct UnitIn {
    uint64_t off, len;           // byte range relative to the device base pointer
    int64_t init_start, init_stop;
    uint64_t id;                 // global unit index (archive order)
};
enum Layout { L_ARCHIVE, L_STREAMS };
struct PendingNames {
    std::vector<uint64_t> at;    // nseg + 1 offsets into the packed bytes
    const uint8_t* host = nullptr;
    hipEvent_t ev = nullptr;
    ~PendingNames() { if (ev) (void)hipEventDestroy(ev); }
};
void fetch_names(starch_ctx* c, const uint8_t* d_base, const std::vector<SegInfo>& si, PendingNames& pn);
void finish_names(starch_ctx* c, PendingNames& pn);
starch_ctx* lane_ctx(starch_ctx* c, int i);
// an encode's counters and stage times (every other field zero)
starch_stats stats_of(const bz::Stats& b, float ms_transform, float ms_total);
// x's lines, text, counters and times added to t's (concurrent, as shards on several devices: the
// longest of each time stays instead); input_bytes, n_segments and archive_bytes are the caller's
void add_stats(starch_stats& t, const starch_stats& x, bool concurrent = false);
// whole streams over the segments' text, one group each
std::vector<bz::StreamIn> streams_of(const std::vector<SegInfo>& si);
// a batch's segments and names appended, its stream offsets moved by stream_base
void append_segments(std::vector<starch_segment>& dst_segs, std::vector<std::string>& dst_names,
                     const std::vector<starch_segment>& segs, const std::vector<std::string>& names,
                     uint64_t stream_base);
// an archive put together from several encodes becomes the context's result: segs and names
// swapped in, stats with archive_bytes = bytes, no text
void install_archive(starch_ctx* c, std::vector<starch_segment>& segs, std::vector<std::string>& names,
                     const starch_stats& stats, uint64_t bytes);
void encode_units(starch_ctx* c, const uint8_t* d_base, const std::vector<UnitIn>& units, const starch_options& opt,
                  Layout lay, bool planned = false, bool split_ok = false);
void encode_device(starch_ctx* c, const uint8_t* d_bed, uint64_t n, const starch_options& opt);

// ---- api_decode.hip ----
uint64_t unstarch_to_ut_out(starch_ctx* c, const uint8_t* a, uint64_t n, const char* refuse_gzip);

// ---- api_gunzip.hip: a gzip input of a host entry point ----
// gz[0, n) (gz::is_gzip) copied to c->dec_in and planned; returns the inflated size
uint64_t gunzip_plan(starch_ctx* c, const uint8_t* gz, uint64_t n);
// the planned members inflated into d_out and checked; c->gstats filled
void gunzip_into(starch_ctx* c, uint8_t* d_out);

}  // namespace api
#pragma GCC visibility pop
