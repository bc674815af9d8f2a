// starch_amd/csrc/api_decode.hip -- the C ABI's decode side: bzip2 decompression, the
// inverse transform, unstarch and indexed extraction.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "api_int.hpp"

using namespace api;

namespace {

// A query per chromosome: whole, or disjoint ranges with increasing qstart.
// Ranges merge only when they strictly overlap: touching [a,b) [b,c) stay
// apart, since their union would select a zero-length element at b that
// neither selects.
struct ChrQuery {
    bool whole = false;
    std::vector<std::pair<int64_t, int64_t>> r;
};

std::vector<std::pair<std::string, ChrQuery>> normalise_regions(const starch_region* regions, uint64_t nregions)
{
    std::vector<std::pair<std::string, ChrQuery>> q;
    for (uint64_t k = 0; k < nregions; ++k) {
        const starch_region& g = regions[k];
        if (g.chr_len && !g.chr) throw StarchError(STARCH_ERR_ARG, "extract: region with a NULL chromosome name");
        if (!g.whole && g.start >= g.stop)
            throw StarchError(STARCH_ERR_ARG, "extract: region " + std::to_string(k) + " has start >= stop");
        const std::string name(g.chr ? g.chr : "", g.chr_len);
        size_t i = 0;
        while (i < q.size() && q[i].first != name) ++i;
        if (i == q.size()) q.emplace_back(name, ChrQuery{});
        if (g.whole) q[i].second.whole = true;
        else q[i].second.r.emplace_back(g.start, g.stop);
    }
    for (auto& e : q) {
        ChrQuery& c = e.second;
        if (c.whole) { c.r.clear(); continue; }
        std::sort(c.r.begin(), c.r.end());
        size_t w = 0;
        for (size_t k = 1; k < c.r.size(); ++k) {
            if (c.r[k].first < c.r[w].second) c.r[w].second = std::max(c.r[w].second, c.r[k].second);
            else c.r[++w] = c.r[k];
        }
        if (!c.r.empty()) c.r.resize(w + 1);
    }
    return q;
}

}  // namespace

namespace api {

// The whole archive a[0, n) decoded and inverse-transformed into c->ut_out;
// returns the BED bytes.  refuse_gzip: the caller's name for the error that a
// gzip-method archive gets (nullptr: the decoder decides).
uint64_t unstarch_to_ut_out(starch_ctx* c, const uint8_t* a, uint64_t n, const char* refuse_gzip)
{
    uint64_t index_off = 0;
    ArchiveInfo info;
    const std::vector<IndexEntry> idx = read_index(a, n, &index_off, &info);
    if (refuse_gzip && info.format == "gzip")
        throw StarchError(STARCH_ERR_ARG,
                          std::string(refuse_gzip) + ": gzip archives are not decoded (compressionFormat \"gzip\")");
    // the streams region [4, index_off) is the concatenated bzip2 streams, in index order
    const uint64_t m = index_off - 4;
    uint8_t* d = c->dec_in.as<uint8_t>(m + 256);
    if (m) HIP_CHECK(hipMemcpyAsync(d, a + 4, m, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemsetAsync(d + m, 0, 256, c->st));
    const uint64_t tbytes = c->dec.decode(d, m, a + 4, c->st, c->dec_out, c->dstreams);
    if (c->dstreams.size() != idx.size()) throw StarchError(STARCH_ERR_DATA, "archive: index and streams disagree");
    std::vector<ut::Untransform::Seg> segs;
    for (size_t k = 0; k < idx.size(); ++k) {
        const bz::DecStream& s = c->dstreams[k];
        if (s.in_beg + 4 != idx[k].offset || s.in_end - s.in_beg != idx[k].size)
            throw StarchError(STARCH_ERR_DATA, "archive: stream " + std::to_string(k) + " is not where the index says");
        segs.push_back(ut::Untransform::Seg{s.out_off, s.out_len, idx[k].chr});
    }
    return c->untf.run(c->tf, static_cast<const uint8_t*>(c->dec_out.p), tbytes, segs, c->st, c->ut_out);
}

}  // namespace api

extern "C" {

// in: n bytes of bzip2 streams in HBM, or in host memory (then the decoder reads them there too)
static int bz2_decompress(starch_ctx* c, const void* in, uint64_t n, bool on_host)
{
    GUARD(c)
    if (n && !in) return STARCH_ERR_ARG;
    c->have_out = false;
    uint8_t* d = c->dec_in.as<uint8_t>(n + 256);   // aligned copy with read-ahead padding
    if (n) HIP_CHECK(hipMemcpyAsync(d, in, n, on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->st));
    HIP_CHECK(hipMemsetAsync(d + n, 0, 256, c->st));
    const uint8_t* h_in = on_host ? static_cast<const uint8_t*>(in) : nullptr;
    publish(c, c->dec_out, c->dec.decode(d, n, h_in, c->st, c->dec_out, c->dstreams));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_bz2_decompress_device(starch_ctx* c, const void* d_in, uint64_t n) { return bz2_decompress(c, d_in, n, false); }

int starch_bz2_decompress_host(starch_ctx* c, const void* in, uint64_t n) { return bz2_decompress(c, in, n, true); }

int starch_bz2_stream_count(starch_ctx* c, uint64_t* n)
{
    if (!c || !n) return STARCH_ERR_ARG;
    if (!c->have_out) return STARCH_ERR_STATE;
    *n = c->dstreams.size();
    return STARCH_OK;
}

int starch_bz2_streams(starch_ctx* c, starch_dec_stream* out, uint64_t cap)
{
    if (!c || (cap && !out)) return STARCH_ERR_ARG;
    if (!c->have_out) return STARCH_ERR_STATE;
    if (cap < c->dstreams.size()) return STARCH_ERR_MEM;
    for (size_t k = 0; k < c->dstreams.size(); ++k) {
        const bz::DecStream& s = c->dstreams[k];
        out[k] = starch_dec_stream{s.in_beg, s.in_end, s.out_off, s.out_len, s.level, s.n_blocks, s.stored_crc};
    }
    return STARCH_OK;
}

int starch_untransform_host(starch_ctx* c, const void* text, uint64_t n, const char* chr, uint64_t chr_len)
{
    GUARD(c)
    if ((n && !text) || (chr_len && !chr)) return STARCH_ERR_ARG;
    c->have_out = false;
    uint8_t* d = c->dec_out.as<uint8_t>(n + 64);
    if (n) HIP_CHECK(hipMemcpyAsync(d, text, n, hipMemcpyHostToDevice, c->st));
    std::vector<ut::Untransform::Seg> segs;
    if (n) segs.push_back(ut::Untransform::Seg{0, n, std::string(chr ? chr : "", chr_len)});
    publish(c, c->ut_out, c->untf.run(c->tf, d, n, segs, c->st, c->ut_out));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_unstarch_host(starch_ctx* c, const void* archive, uint64_t n)
{
    GUARD(c)
    if (!archive) return STARCH_ERR_ARG;
    c->have_out = false;
    publish(c, c->ut_out, unstarch_to_ut_out(c, static_cast<const uint8_t*>(archive), n, nullptr));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_extract_host(starch_ctx* c, const void* archive, uint64_t n, const starch_region* regions,
                        uint64_t nregions)
{
    GUARD(c)
    if (!archive || (nregions && !regions)) return STARCH_ERR_ARG;
    c->have_out = false;
    c->have_xstats = false;
    const auto query = normalise_regions(regions, nregions);
    const uint8_t* a = static_cast<const uint8_t*>(archive);
    uint64_t index_off = 0;
    ArchiveInfo info;
    const std::vector<IndexEntry> idx = read_index(a, n, &index_off, &info);
    if (info.format == "gzip")
        throw StarchError(STARCH_ERR_ARG, "extract: gzip archives are not decoded (compressionFormat \"gzip\")");
    check_bounds(idx, index_off);
    // the index entries whose chromosome is queried, in archive order
    std::vector<size_t> pick, qof;
    for (size_t k = 0; k < idx.size(); ++k) {
        if (query.empty()) { pick.push_back(k); qof.push_back(0); continue; }
        for (size_t i = 0; i < query.size(); ++i)
            if (query[i].first == idx[k].chr) { pick.push_back(k); qof.push_back(i); break; }
    }
    starch_extract_stats xs{};
    xs.streams_total = idx.size();
    xs.streams_decoded = pick.size();
    if (pick.empty()) {
        c->ut_out.as<uint8_t>(64);
        c->dstreams.clear();
        c->out_bytes = 0;
    } else {
        // their bytes back to back in dec_in: one copy per run of adjacent entries
        uint64_t m = 0;
        for (size_t k : pick) m += idx[k].size;
        xs.compressed_bytes_decoded = m;
        uint8_t* d = c->dec_in.as<uint8_t>(m + 256);
        struct Run { uint64_t src, dst, len; };
        std::vector<Run> runs;
        uint64_t pos = 0;
        for (size_t k : pick) {
            if (!runs.empty() && runs.back().src + runs.back().len == idx[k].offset) runs.back().len += idx[k].size;
            else runs.push_back(Run{idx[k].offset, pos, idx[k].size});
            pos += idx[k].size;
        }
        for (const Run& r : runs)
            if (r.len) HIP_CHECK(hipMemcpyAsync(d + r.dst, a + r.src, r.len, hipMemcpyHostToDevice, c->st));
        HIP_CHECK(hipMemsetAsync(d + m, 0, 256, c->st));
        // the decoder's host view of the same bytes: the archive itself for one run, else a packed copy
        std::vector<uint8_t> staging;
        const uint8_t* h_in = a + runs[0].src;
        if (runs.size() > 1) {
            staging.resize(m);
            for (const Run& r : runs) memcpy(staging.data() + r.dst, a + r.src, r.len);
            h_in = staging.data();
        }
        const uint64_t tbytes = c->dec.decode(d, m, h_in, c->st, c->dec_out, c->dstreams);
        if (c->dstreams.size() != pick.size()) throw StarchError(STARCH_ERR_DATA, "archive: index and streams disagree");
        std::vector<ut::Untransform::Seg> segs;
        ut::Untransform::Selection sel;
        pos = 0;
        for (size_t i = 0; i < pick.size(); ++i) {
            const IndexEntry& en = idx[pick[i]];
            const bz::DecStream& s = c->dstreams[i];
            if (s.in_beg != pos || s.in_end - s.in_beg != en.size)
                throw StarchError(STARCH_ERR_DATA,
                                  "archive: stream " + std::to_string(pick[i]) + " is not where the index says");
            pos += en.size;
            segs.push_back(ut::Untransform::Seg{s.out_off, s.out_len, en.chr});
            const bool whole = query.empty() || query[qof[i]].second.whole;
            sel.whole.push_back(whole ? 1u : 0u);
            sel.q_lo.push_back((uint32_t)sel.qs.size());
            if (!whole)
                for (const auto& r : query[qof[i]].second.r) {
                    sel.qs.push_back(r.first);
                    sel.qe.push_back(r.second);
                }
            sel.q_hi.push_back((uint32_t)sel.qs.size());
        }
        c->out_bytes = c->untf.run(c->tf, static_cast<const uint8_t*>(c->dec_out.p), tbytes, segs, c->st, c->ut_out, &sel);
        xs.lines_scanned = sel.lines_scanned;
        xs.lines_out = sel.lines_out;
    }
    publish(c, c->ut_out, c->out_bytes);
    c->xstats = xs;
    c->have_xstats = true;
    return STARCH_OK;
    END_GUARD(c)
}

int starch_extract_get_stats(starch_ctx* c, starch_extract_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_xstats) return STARCH_ERR_STATE;
    *out = c->xstats;
    return STARCH_OK;
}

}  // extern "C"
