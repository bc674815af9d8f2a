// starch_amd/csrc/api_gunzip.hip -- the C ABI of the inflater (gz_inflate.hip):
// starch_gunzip_*, and what the BED commands' loaders call for a gzip input.
#include <string.h>

#include <vector>

#include "api_int.hpp"

using namespace api;

namespace api {

uint64_t gunzip_plan(starch_ctx* c, const uint8_t* gz, uint64_t n)
{
    c->have_gstats = false;
    uint8_t* d = c->dec_in.as<uint8_t>(n + gz::kInPad);   // aligned copy with read-ahead padding
    StageTimer<2> tm;
    tm.start(c->st);
    HostRegistration reg(gz, n, 256ull << 20);
    reg.h2d(d, gz, n, c->st);
    HIP_CHECK(hipMemsetAsync(d + n, 0, gz::kInPad, c->st));
    float ms_upload = 0;
    tm.finish(1, c->st, {&ms_upload});
    const uint64_t total = c->inflater.plan(gz, d, n, c->st);
    c->inflater.stats.ms_upload = ms_upload;
    return total;
}

void gunzip_into(starch_ctx* c, uint8_t* d_out)
{
    c->inflater.inflate(d_out, c->st);
    const gz::InflateStats& s = c->inflater.stats;
    c->gstats = starch_gunzip_stats{s.members, s.is_bgzf, s.stored_blocks, s.fixed_blocks, s.dynamic_blocks, s.bytes_in,
                                    s.bytes_out, s.ms_plan, s.ms_upload, s.ms_size, s.ms_inflate, s.ms_crc};
    c->have_gstats = true;
}

}  // namespace api

extern "C" {

int starch_gunzip_host(starch_ctx* c, const void* gz, uint64_t n)
{
    GUARD(c)
    if (n && !gz) return STARCH_ERR_ARG;
    c->have_out = false;
    const uint64_t total = gunzip_plan(c, static_cast<const uint8_t*>(gz), n);
    gunzip_into(c, c->dec_out.as<uint8_t>(total + 64));
    publish(c, c->dec_out, total);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_gunzip_device(starch_ctx* c, const void* d_gz, uint64_t n)
{
    GUARD(c)
    if (n && !d_gz) return STARCH_ERR_ARG;
    c->have_out = false;
    std::vector<uint8_t> h(n);                 // the headers are read on the host
    if (n) HIP_CHECK(hipMemcpyAsync(h.data(), d_gz, n, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    const uint64_t total = gunzip_plan(c, h.data(), n);
    gunzip_into(c, c->dec_out.as<uint8_t>(total + 64));
    publish(c, c->dec_out, total);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_gunzip_plan(const void* gz, uint64_t n, starch_gunzip_member* out, uint64_t cap, uint64_t* n_members,
                       int* is_bgzf)
{
    if ((n && !gz) || (cap && !out) || !n_members || !is_bgzf) return STARCH_ERR_ARG;
    *n_members = 0;
    *is_bgzf = 0;
    try {
        if (!gz::is_gzip(gz, n)) return STARCH_ERR_DATA;
        std::vector<gz::Member> t;
        if (!gz::plan_bgzf(static_cast<const uint8_t*>(gz), n, t)) return STARCH_OK;
        *is_bgzf = 1;
        *n_members = t.size();
        for (uint64_t k = 0; k < t.size() && k < cap; ++k)
            out[k] = starch_gunzip_member{t[k].in_off, t[k].in_len, t[k].out_off, t[k].isize, t[k].crc};
        return t.size() > cap && (cap || out) ? STARCH_ERR_MEM : STARCH_OK;
    } catch (const StarchError& e) {
        return e.code;
    } catch (const std::exception&) {
        return STARCH_ERR_INTERNAL;
    }
}

int starch_gunzip_get_stats(starch_ctx* c, starch_gunzip_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_gstats) return STARCH_ERR_STATE;
    *out = c->gstats;
    return STARCH_OK;
}

int starch_gunzip_constants(uint32_t* window_bytes, uint32_t* primary_bits, uint32_t* copy_width, uint32_t* bgzf_max)
{
    if (window_bytes) *window_bytes = gz::kWindowBytes;
    if (primary_bits) *primary_bits = gz::kPrimaryBits;
    if (copy_width) *copy_width = gz::kCopyWidth;
    if (bgzf_max) *bgzf_max = gz::kBgzfMax;
    return STARCH_OK;
}

int starch_is_gzip(const void* data, uint64_t n) { return data && gz::is_gzip(data, n) ? 1 : 0; }

}  // extern "C"
