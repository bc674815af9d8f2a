// starch_amd/csrc/api_encode.hip -- the C ABI's encode side: transform + compression over
// units into an archive or a shard's streams, on one device, pipelined from
// host memory, or over several devices; and the calls that read the result.
// Host orchestration only: every byte of the transform and of the bzip2
// streams is produced by the HIP kernels in this directory.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "api_int.hpp"
#include "shard.hpp"

using namespace api;

namespace {

// chr token of the last line before `j` and of the line at `j`, read from small
// device windows; false when a line does not fit the window (the caller then
// takes the exact per-unit route)
bool junction_differs(starch_ctx* c, const uint8_t* d_base, uint64_t lo, uint64_t j, uint64_t hi)
{
    const uint64_t W = 1024;
    uint8_t a[W], b[W];
    const uint64_t a0 = (j - lo > W) ? j - W : lo, an = j - a0;
    const uint64_t bn = std::min<uint64_t>(W, hi - j);
    if (an) HIP_CHECK(hipMemcpyAsync(a, d_base + a0, an, hipMemcpyDeviceToHost, c->st));
    if (bn) HIP_CHECK(hipMemcpyAsync(b, d_base + j, bn, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (an == 0 || bn == 0) return false;
    // previous line: [ls, an) in a (a[an-1] is its '\n')
    uint64_t ls = an - 1;
    while (ls > 0 && a[ls - 1] != '\n') --ls;
    if (ls == 0 && a0 > lo) return false;
    auto tok = [](const uint8_t* x, uint64_t beg, uint64_t n, bool complete, uint64_t* len) {
        uint64_t p = beg;
        while (p < n && x[p] != '\t' && x[p] != '\n') ++p;
        if (p == n && !complete) return false;
        uint64_t e = (p < n && x[p] == '\n') ? p + 1 : p;
        const void* z = memchr(x + beg, 0, e - beg);
        *len = z ? (uint64_t)(static_cast<const uint8_t*>(z) - (x + beg)) : e - beg;
        return true;
    };
    uint64_t la = 0, lb = 0;
    if (!tok(a, ls, an, true, &la) || !tok(b, 0, bn, j + bn >= hi, &lb)) return false;
    return la != lb || memcmp(a + ls, b, la) != 0;
}

struct FFInBatch {};   // transform_units(planned): the batch holds a 0xFF (hpp:181: EOF)

// Transform stage over units.  One launch sequence over the whole range when
// the units are back to back, every junction changes chromosome (so it is a
// segment start in the concatenation too) and no sscanf value goes stale;
// otherwise each unit runs on its own with its initial values.  Fills the host
// segment table (name_off relative to d_base, text_off into the returned text)
// and the unit of every segment.
const uint8_t* transform_units(starch_ctx* c, const uint8_t* d_base, const std::vector<UnitIn>& u,
                               std::vector<SegInfo>& si, std::vector<uint64_t>& unit_of, uint64_t& text_bytes,
                               uint64_t& n_lines, bool planned = false)
{
    si.clear();
    unit_of.clear();
    text_bytes = n_lines = 0;
    if (u.empty()) return nullptr;
    bool joint = true;
    for (size_t k = 1; k < u.size() && joint; ++k) joint = u[k].off == u[k - 1].off + u[k - 1].len;
    // units from shard::plan_units start a new chromosome by construction
    for (size_t k = 1; k < u.size() && joint && !planned; ++k)
        if (u[k].len && u[k - 1].len) joint = junction_differs(c, d_base, u[k - 1].off, u[k].off, u[k].off + u[k].len);
    if (joint) {
        const uint64_t beg = u[0].off, end = u.back().off + u.back().len;
        TransformResult tr;
        c->tf.run(d_base + beg, end - beg, c->st, tr, u[0].init_start, u[0].init_stop);
        if (planned && tr.ff_pos != ~0ull) throw FFInBatch{};
        if (u.size() > 1 && tr.ff_pos != ~0ull)
            throw StarchError(STARCH_ERR_ARG, "a unit contains byte 0xFF (plan units with starch_plan_units)");
        if (u.size() == 1 || !tr.general) {
            si.resize(tr.n_segments);
            if (tr.n_segments)
                HIP_CHECK(hipMemcpyAsync(si.data(), c->tf.seg_info_dev, tr.n_segments * sizeof(SegInfo),
                                         hipMemcpyDeviceToHost, c->st));
            HIP_CHECK(hipStreamSynchronize(c->st));
            unit_of.resize(si.size());
            size_t k = 0;
            for (size_t s = 0; s < si.size(); ++s) {
                si[s].name_off += beg;
                while (k + 1 < u.size() && si[s].name_off >= u[k + 1].off) ++k;
                unit_of[s] = u[k].id;
            }
            text_bytes = tr.text_bytes;
            n_lines = tr.n_lines;
            return c->tf.text;
        }
    }
    // exact per-unit route: each unit with the sscanf values current before it
    uint8_t* all = static_cast<uint8_t*>(c->text_all.p);   // staging text of all units
    uint64_t cap = c->text_all.cap;
    for (size_t k = 0; k < u.size(); ++k) {
        TransformResult tr;
        c->tf.run(d_base + u[k].off, u[k].len, c->st, tr, u[k].init_start, u[k].init_stop);
        if (planned && tr.ff_pos != ~0ull) throw FFInBatch{};
        if (tr.ff_pos != ~0ull)
            throw StarchError(STARCH_ERR_ARG, "a unit contains byte 0xFF (plan units with starch_plan_units)");
        std::vector<SegInfo> part(tr.n_segments);
        if (tr.n_segments)
            HIP_CHECK(hipMemcpyAsync(part.data(), c->tf.seg_info_dev, tr.n_segments * sizeof(SegInfo),
                                     hipMemcpyDeviceToHost, c->st));
        if (text_bytes + tr.text_bytes + 64 > cap) {   // grow the staging text, keeping what it holds
            const uint64_t ncap = std::max<uint64_t>(2 * cap, text_bytes + tr.text_bytes + 64);
            DevBuf nb;
            uint8_t* np = nb.as<uint8_t>(ncap);
            if (text_bytes) HIP_CHECK(hipMemcpyAsync(np, all, text_bytes, hipMemcpyDeviceToDevice, c->st));
            HIP_CHECK(hipStreamSynchronize(c->st));
            std::swap(c->text_all.p, nb.p);
            std::swap(c->text_all.cap, nb.cap);
            all = np;
            cap = ncap;
        }
        if (tr.text_bytes)
            HIP_CHECK(hipMemcpyAsync(all + text_bytes, c->tf.text, tr.text_bytes, hipMemcpyDeviceToDevice, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
        for (auto& g : part) {
            g.name_off += u[k].off;
            g.text_off += text_bytes;
            g.first_line += n_lines;
            si.push_back(g);
            unit_of.push_back(u[k].id);
        }
        text_bytes += tr.text_bytes;
        n_lines += tr.n_lines;
    }
    return all;
}

// Segment names (the chr tokens, in the input) -> c->names.  One gather
// kernel packs them into a device buffer and ONE copy brings them to pinned
// host memory (one copy per name costs a host round trip each: ~20 us per
// segment).  fetch_names issues the work on c->st; finish_names fills
// c->names once the stream has passed it (the caller syncs or waits on ev).
struct NameDesc { uint64_t src, dst, len; };

__global__ void k_gather_names(const uint8_t* __restrict__ base, const NameDesc* __restrict__ d, uint8_t* __restrict__ out)
{
    const NameDesc x = d[blockIdx.x];
    for (uint64_t i = threadIdx.x; i < x.len; i += blockDim.x) out[x.dst + i] = base[x.src + i];
}

}  // namespace

namespace api {

void fetch_names(starch_ctx* c, const uint8_t* d_base, const std::vector<SegInfo>& si, PendingNames& pn)
{
    const uint64_t nseg = si.size();
    pn.at.assign(nseg + 1, 0);
    for (uint64_t s = 0; s < nseg; ++s) pn.at[s + 1] = pn.at[s] + si[s].name_len;
    const uint64_t total = pn.at[nseg];
    if (!total) return;
    uint8_t* hp = static_cast<uint8_t*>(c->names_pin.get(total + nseg * sizeof(NameDesc) + 64));
    NameDesc* hd = reinterpret_cast<NameDesc*>(hp + align_up(total, 64));
    for (uint64_t s = 0; s < nseg; ++s) hd[s] = NameDesc{si[s].name_off, pn.at[s], si[s].name_len};
    uint8_t* dp = c->names_dev.as<uint8_t>(align_up(total, 64) + nseg * sizeof(NameDesc));
    NameDesc* dd = reinterpret_cast<NameDesc*>(dp + align_up(total, 64));
    HIP_CHECK(hipMemcpyAsync(dd, hd, nseg * sizeof(NameDesc), hipMemcpyHostToDevice, c->st));
    hipLaunchKernelGGL(k_gather_names, dim3((unsigned)nseg), dim3(64), 0, c->st, d_base, dd, dp);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hp, dp, total, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipEventCreateWithFlags(&pn.ev, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(pn.ev, c->st));
    pn.host = hp;
}

void finish_names(starch_ctx* c, PendingNames& pn)
{
    const uint64_t nseg = pn.at.empty() ? 0 : pn.at.size() - 1;
    c->names.assign(nseg, std::string());
    if (pn.ev) {
        HIP_CHECK(hipEventSynchronize(pn.ev));
        (void)hipEventDestroy(pn.ev);
        pn.ev = nullptr;
        for (uint64_t s = 0; s < nseg; ++s)
            c->names[s].assign(reinterpret_cast<const char*>(pn.host) + pn.at[s], pn.at[s + 1] - pn.at[s]);
    }
}

}  // namespace api

namespace {

// Encoder lanes of a one-transform encode (STARCH_DEV_LANES, default 2): the
// segments split into contiguous runs of about equal text, each planned
// (RLE1 .. tables) by its own encoder on its own stream and host thread, so
// one lane's host round trips and the drain of its persistent kernels are
// filled by the other lanes' kernels.  Returns the first segment of every
// lane (empty: one lane).  Streams keep their order; the archive is the same
// bytes.
std::vector<uint64_t> lane_cuts(const std::vector<SegInfo>& si, uint64_t tbytes, int want)
{
    static const int nl_env = [] { const char* e = getenv("STARCH_DEV_LANES"); return e ? atoi(e) : 2; }();
    const int nl_req = want > 0 ? want : nl_env;
    static const uint64_t min_b = [] {
        const char* e = getenv("STARCH_DEV_LANES_MIN");
        return e ? (uint64_t)atoll(e) : (uint64_t)(16ull << 20);
    }();
    const uint64_t nseg = si.size();
    const uint64_t nl = std::min<uint64_t>({(uint64_t)std::max(nl_req, 1), nseg, 8});
    std::vector<uint64_t> cuts;
    if (nl < 2 || tbytes < min_b) return cuts;
    cuts.push_back(0);
    uint64_t acc = 0, k = 0;
    for (uint64_t i = 1; i < nl; ++i) {
        const uint64_t target = tbytes * i / nl;   // lane i starts at the segment whose middle passes it
        while (k < nseg && 2 * acc + si[k].text_len < 2 * target) acc += si[k++].text_len;
        if (k <= cuts.back()) acc += si[k++].text_len;
        if (k >= nseg) break;
        cuts.push_back(k);
    }
    if (cuts.size() < 2) cuts.clear();
    return cuts;
}

// per stage, the wall time during which any lane ran it (union of intervals)
void stage_union(const std::vector<bz::Encoder::Interval>& iv, bz::Stats& st)
{
    float* f[5] = {&st.rle, &st.bwt, &st.mtf, &st.tables, &st.emit};
    for (int k = 0; k < 5; ++k) {
        std::vector<std::pair<float, float>> x;
        for (auto& v : iv)
            if (v.stage == k) x.emplace_back(v.a, v.b);
        std::sort(x.begin(), x.end());
        float tot = 0, ca = 0, cb = -1e30f;
        for (auto& p : x) {
            if (p.first > cb) {
                if (cb > ca) tot += cb - ca;
                ca = p.first;
                cb = p.second;
            } else if (p.second > cb) {
                cb = p.second;
            }
        }
        if (cb > ca) tot += cb - ca;
        *f[k] = tot;
    }
}

}  // namespace

namespace api {

void Caught::rethrow(const std::string& prefix) const
{
    if (code) throw StarchError(code, std::string(prefix).append(msg));
}

starch_stats stats_of(const bz::Stats& b, float ms_transform, float ms_total)
{
    starch_stats s{};
    s.n_blocks = b.n_blocks, s.rle_bytes = b.rle_bytes, s.bwt_rounds = b.bwt_rounds;
    s.periodic_blocks = b.periodic_blocks, s.bwt_tied = b.bwt_tied, s.dedup_blocks = b.dedup_blocks;
    s.ms_transform = ms_transform, s.ms_total = ms_total;
    s.ms_rle = b.rle, s.ms_bwt = b.bwt, s.ms_mtf = b.mtf, s.ms_tables = b.tables, s.ms_emit = b.emit;
    return s;
}

void add_stats(starch_stats& t, const starch_stats& x, bool concurrent)
{
    for (uint64_t starch_stats::*f : {&starch_stats::n_lines, &starch_stats::text_bytes, &starch_stats::n_blocks,
                                      &starch_stats::rle_bytes, &starch_stats::bwt_rounds,
                                      &starch_stats::periodic_blocks, &starch_stats::bwt_tied,
                                      &starch_stats::dedup_blocks})
        t.*f += x.*f;
    for (float starch_stats::*f : {&starch_stats::ms_transform, &starch_stats::ms_rle, &starch_stats::ms_bwt,
                                   &starch_stats::ms_mtf, &starch_stats::ms_tables, &starch_stats::ms_emit,
                                   &starch_stats::ms_total})
        t.*f = concurrent ? std::max(t.*f, x.*f) : t.*f + x.*f;
}

std::vector<bz::StreamIn> streams_of(const std::vector<SegInfo>& si)
{
    std::vector<bz::StreamIn> sin(si.size());
    for (size_t s = 0; s < si.size(); ++s) {
        sin[s].text_off = si[s].text_off;
        sin[s].text_len = si[s].text_len;
        sin[s].final_run_joins = 1;
        sin[s].group = (uint32_t)s;
    }
    return sin;
}

void append_segments(std::vector<starch_segment>& dst_segs, std::vector<std::string>& dst_names,
                     const std::vector<starch_segment>& segs, const std::vector<std::string>& names,
                     uint64_t stream_base)
{
    for (size_t s = 0; s < segs.size(); ++s) {
        dst_segs.push_back(segs[s]);
        dst_segs.back().stream_offset += stream_base;
        dst_names.push_back(names[s]);
    }
}

void install_archive(starch_ctx* c, std::vector<starch_segment>& segs, std::vector<std::string>& names,
                     const starch_stats& stats, uint64_t bytes)
{
    c->segs.swap(segs);
    c->names.swap(names);
    c->stats = stats;
    c->stats.archive_bytes = bytes;
    c->text_bytes = 0;
    c->text_dev = nullptr;
    c->archive_bytes = bytes;
    c->have = true;
    c->streamed = false;
}

// transform + bzip2 over units.  L_ARCHIVE: magic + streams + index in
// c->archive (the whole-input result); L_STREAMS: the streams alone, back to
// back from offset 0 of c->part (one shard of a multi-GPU run).
void encode_units(starch_ctx* c, const uint8_t* d_base, const std::vector<UnitIn>& units, const starch_options& opt,
                  Layout lay, bool planned, bool split_ok)
{
    hipEvent_t* tv = c->timers();   // owned by the context: nothing to release on a throw
    hipEvent_t e0 = tv[0], e1 = tv[1], e2 = tv[2];
    HIP_CHECK(hipEventRecord(e0, c->st));
    c->have = false;
    c->streamed = false;
    c->gathered = false;
    c->stats = starch_stats{};
    for (auto& u : units) c->stats.input_bytes += u.len;
    std::vector<SegInfo> si;
    std::vector<uint64_t> unit_of;
    uint64_t tbytes = 0, nlines = 0;
    const uint8_t* text = transform_units(c, d_base, units, si, unit_of, tbytes, nlines, planned);
    std::vector<uint64_t> bc_u, bc_n;
    if (opt.base_counts) {   // per unit (units start segments), in segment order
        std::vector<uint64_t> uu, nn;
        for (auto& u : units) {
            c->tf.base_counts(d_base + u.off, u.len, c->st, u.init_start, u.init_stop, uu, nn);
            bc_u.insert(bc_u.end(), uu.begin(), uu.end());
            bc_n.insert(bc_n.end(), nn.begin(), nn.end());
        }
        if (bc_u.size() != si.size()) throw StarchError(STARCH_ERR_INTERNAL, "base counts: segment count mismatch");
    }
    HIP_CHECK(hipEventRecord(e1, c->st));
    const uint64_t nseg = si.size();
    c->stats.n_lines = nlines;
    c->stats.n_segments = nseg;
    c->stats.text_bytes = tbytes;
    c->text_bytes = tbytes;
    c->text_dev = text;
    // segment names: one gather + one copy, read once the encoder has synced
    PendingNames pnames;
    fetch_names(c, d_base, si, pnames);
    c->segs.assign(nseg, starch_segment{});
    for (uint64_t s = 0; s < nseg; ++s) {
        c->segs[s].line_count = si[s].line_count;
        c->segs[s].text_bytes = si[s].text_len;
        c->segs[s].name_len = si[s].name_len;
        c->segs[s].unit = unit_of[s];
        if (opt.base_counts) {
            c->segs[s].base_count_unique = (int64_t)bc_u[s];
            c->segs[s].base_count_nonunique = (int64_t)bc_n[s];
        }
    }
    const uint64_t base = (lay == L_ARCHIVE) ? 4 : 0;
    if (opt.reference_compat && lay == L_ARCHIVE) {   // the reference writes only the magic (hpp:765-769)
        uint8_t* out = c->archive.as<uint8_t>(64);
        HIP_CHECK(hipMemcpyAsync(out, kMagic, 4, hipMemcpyHostToDevice, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
        finish_names(c, pnames);
        c->archive_bytes = 4;
        c->have = true;
        return;
    }
    std::vector<bz::StreamIn> sin = streams_of(si);
    std::vector<bz::StreamOut> outs;
    bz::Stats bst;
    const bool gzip = opt.compression_method == STARCH_METHOD_GZIP;
    const std::vector<uint64_t> cuts = !gzip && split_ok ? lane_cuts(si, tbytes, c->dev_lanes) : std::vector<uint64_t>();
    const size_t nl = cuts.size();
    std::vector<starch_ctx*> ln(nl);
    std::vector<std::vector<bz::StreamOut>> lo(nl);   // each lane's streams (offsets from its own base)
    std::vector<bz::Stats> lst(nl);
    std::vector<uint64_t> lbase(nl, 0);                // lane i's first byte after `base`
    if (gzip) {
        c->genc.plan(text, sin, c->st, outs, &bst);
    } else if (nl) {
        std::vector<Caught> err(nl);
        std::vector<std::vector<bz::StreamIn>> li(nl);
        for (size_t i = 0; i < nl; ++i) {
            ln[i] = lane_ctx(c, (int)i);
            ln[i]->enc.set_mem_share(1.0 / (double)nl);
            const uint64_t s0 = cuts[i], s1 = i + 1 < nl ? cuts[i + 1] : nseg;
            li[i].assign(sin.begin() + s0, sin.begin() + s1);
            for (auto& x : li[i]) x.group -= (uint32_t)s0;
        }
        auto plan_lane = [&](size_t i) {
            err[i].run([&] {
                Ctx g(ln[i]);
                ln[i]->enc.plan(text, li[i], opt.block_size_100k, ln[i]->st, lo[i], &lst[i]);
            });
        };
        for (size_t i = 1; i < nl; ++i) HIP_CHECK(hipStreamWaitEvent(ln[i]->st, e1, 0));   // the text is written
        for (size_t i = 1; i < nl; ++i) ln[i]->worker.start([&plan_lane, i] { plan_lane(i); });
        plan_lane(0);
        for (size_t i = 1; i < nl; ++i) ln[i]->worker.wait();
        for (size_t i = 0; i < nl; ++i)
            if (err[i].code) {
                for (size_t j = 1; j < nl; ++j) (void)hipStreamSynchronize(ln[j]->st);
                err[i].rethrow();
            }
        uint64_t end = 0;
        for (size_t i = 0; i < nl; ++i) {
            lbase[i] = end;
            uint64_t b = 0;
            for (auto o : lo[i]) {
                b = std::max(b, o.out_off + o.bytes);
                o.out_off += end;
                outs.push_back(o);
            }
            end += b;
            if (i) lst[0].add_counters(lst[i]);
        }
        bst = lst[0];
    } else {
        c->enc.set_mem_share(1.0);
        c->enc.plan(text, sin, opt.block_size_100k, c->st, outs, &bst);
    }
    finish_names(c, pnames);
    uint64_t streams_bytes = 0;
    for (auto& o : outs) streams_bytes = std::max(streams_bytes, o.out_off + o.bytes);
    for (uint64_t s = 0; s < nseg; ++s) {
        c->segs[s].stream_offset = base + outs[s].out_off;
        c->segs[s].stream_bytes = outs[s].bytes;
        c->segs[s].n_blocks = outs[s].n_blocks;
    }
    const uint64_t index_off = base + streams_bytes;
    uint64_t names_b = 0;
    for (auto& nm : c->names) names_b += 6 * nm.size();
    const bool index = lay == L_ARCHIVE && opt.emit_index;
    const uint64_t cap = align_up(index_off + 4 + (index ? 256 + 256 * nseg + 64 + names_b : 0) +
                                      (opt.note && index ? 6 * strlen(opt.note) : 0),
                                  256);
    uint8_t* out = (lay == L_ARCHIVE ? c->archive : c->part).as<uint8_t>(cap);
    if (lay == L_ARCHIVE) HIP_CHECK(hipMemcpyAsync(out, kMagic, 4, hipMemcpyHostToDevice, c->st));
    if (gzip) {
        c->genc.emit(out, cap, base, outs, c->st, &bst);
    } else if (nl) {   // (plan left the lanes' streams idle: every lane's emit goes on this one, in order)
        uint64_t s = 0;
        for (size_t i = 0; i < nl; ++i) {
            ln[i]->enc.emit(out, cap, base + lbase[i], lo[i], c->st, &lst[i]);
            for (auto& o : lo[i]) outs[s++].combined_crc = o.combined_crc;
        }
    } else {
        c->enc.emit(out, cap, base, outs, c->st, &bst);
    }
    for (uint64_t s = 0; s < nseg; ++s) c->segs[s].combined_crc = outs[s].combined_crc;
    uint64_t total = index_off;
    std::string idx;
    if (index) {
        idx = index_of(c->segs, c->names, index_off, opt);
        if (index_off + idx.size() > cap) throw StarchError(STARCH_ERR_INTERNAL, "index capacity");
        HIP_CHECK(hipMemcpyAsync(out + index_off, idx.data(), idx.size(), hipMemcpyHostToDevice, c->st));
        total += idx.size();
    }
    HIP_CHECK(hipEventRecord(e2, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (nl) {
        std::vector<bz::Encoder::Interval> iv;
        for (size_t i = 0; i < nl; ++i) ln[i]->enc.take_intervals(e1, iv);
        stage_union(iv, bst);
    } else if (!gzip) {
        c->enc.resolve_timers(&bst);
    }
    float ms_t = 0, ms_all = 0;
    HIP_CHECK(hipEventElapsedTime(&ms_t, e0, e1));
    HIP_CHECK(hipEventElapsedTime(&ms_all, e0, e2));
    if (lay == L_ARCHIVE) c->archive_bytes = total;
    else c->part_bytes = total;
    c->stats.archive_bytes = total;
    add_stats(c->stats, stats_of(bst, ms_t, ms_all));   // (to the input, lines, segments and text set above)
    c->have = true;
}

// transform + bzip2 + archive of a whole input into ctx->archive (device)
void encode_device(starch_ctx* c, const uint8_t* d_bed, uint64_t n, const starch_options& opt)
{
    std::vector<UnitIn> u(1, UnitIn{0, n, 0, 0, 0});
    encode_units(c, d_bed, u, opt, L_ARCHIVE, false, true);
}

starch_ctx* lane_ctx(starch_ctx* c, int i)
{
    if (i == 0) return c;
    while ((int)c->lanes.size() < i) {
        std::unique_ptr<starch_ctx> L(new starch_ctx());
        L->device = c->device;
        L->is_lane = true;
        HIP_CHECK(hipStreamCreateWithFlags(&L->own, hipStreamNonBlocking));
        L->st = L->own;
        c->lanes.push_back(std::move(L));
    }
    return c->lanes[i - 1].get();
}

}  // namespace api

namespace {

// Pipelined encode of pinned host bytes (the one-call host path).  The input
// is cut at chromosome boundaries (shard::plan_units) into batches; every
// batch crosses PCIe in input order on one copy stream into one device buffer,
// and the batches go round robin to "lanes": the context itself and extra
// contexts on the same device (ctx->lanes), each with its own stream, encoder
// scratch and host thread.  A lane encodes a batch as soon as its bytes are in
// HBM, and the lanes' encodes run concurrently, so one lane's host syncs and
// small end-of-round launches are filled by the other's kernels.  Every
// batch's streams are appended to its lane's collect buffer; the archive is
// then laid out in batch (= input) order, and its bytes equal encode_device's:
// units are independent (shard.cpp), the index is built over all segments at
// the end.  The planner runs to the end of the bytes without a host 0xFF scan;
// a batch whose transform meets a 0xFF (which reads as EOF, hpp:181) abandons
// the pipeline and the caller takes the one-copy path.
bool host_is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

struct LaneBatch {
    int lane = 0;
    uint64_t coll_off = 0, bytes = 0;
    std::vector<starch_segment> segs;
    std::vector<std::string> names;
    starch_stats stats{};
};

// append n device bytes to a lane's collect buffer (grown keeping its bytes)
void collect_append(starch_ctx* L, uint64_t& end, const void* src, uint64_t n)
{
    if (end + n > L->collect.cap) {
        const uint64_t ncap = align_up(std::max<uint64_t>(end + n, L->collect.cap + L->collect.cap / 2) + 4096, 1 << 20);
        DevBuf nb;
        uint8_t* np = nb.as<uint8_t>(ncap);
        if (end) HIP_CHECK(hipMemcpyAsync(np, L->collect.p, end, hipMemcpyDeviceToDevice, L->st));
        HIP_CHECK(hipStreamSynchronize(L->st));
        std::swap(L->collect.p, nb.p);
        std::swap(L->collect.cap, nb.cap);
    }
    if (n) HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t*>(L->collect.p) + end, src, n, hipMemcpyDeviceToDevice, L->st));
    end += n;
}

// Host output of the pipelined encode (starch_encode_host_into): a batch's
// archive offset is known once every earlier batch has finished, so each
// finished batch whose predecessors are done goes device-to-host at once, on
// its lane's stream (after the append that put it in the collect buffer).
// Appends run under mu, so collect.p is read consistently, and a collect
// reallocation syncs its stream before freeing, so a queued copy's source
// stays valid.
struct HostOut {
    uint8_t* out = nullptr;
    uint64_t cap = 0, off = 4;     // next batch's archive offset (after the magic)
    size_t next = 0;               // first batch not yet written
    bool overflow = false;
    std::mutex mu;
    std::vector<char> done;
    std::vector<starch_ctx*> lane;
    void finished(size_t k, const std::vector<LaneBatch>& res)
    {
        std::lock_guard<std::mutex> lk(mu);
        done[k] = 1;
        while (next < done.size() && done[next]) {
            const LaneBatch& r = res[next];
            if (off + r.bytes > cap) overflow = true;
            else if (r.bytes) {
                starch_ctx* L = lane[r.lane];
                HIP_CHECK(hipMemcpyAsync(out + off, static_cast<uint8_t*>(L->collect.p) + r.coll_off, r.bytes,
                                         hipMemcpyDeviceToHost, L->st));
            }
            off += r.bytes;
            ++next;
        }
    }
};

// one lane: batches `mine` (indices into `batches`) in order, each once its
// bytes are in HBM (ev[k], recorded on the shared copy stream after its H2D)
void run_lane(starch_ctx* L, const uint8_t* d_in, const std::vector<shard::Unit>& plan,
              const std::vector<std::pair<size_t, size_t>>& batches, const std::vector<hipEvent_t>& ev,
              const std::vector<size_t>& mine, const starch_options& opt, std::vector<LaneBatch>& out, int lane,
              const std::atomic<bool>& stop, HostOut* hout)
{
    uint64_t total = 0;
    for (size_t k : mine)
        for (size_t u = batches[k].first; u < batches[k].second; ++u) total += plan[u].length;
    uint64_t cend = 0;
    if (L->collect.cap < total / 3 + (1 << 20)) L->collect.as<uint8_t>(total / 3 + (1 << 20));
    for (size_t j = 0; j < mine.size() && !stop.load(); ++j) {
        const size_t k = mine[j];
        HIP_CHECK(hipStreamWaitEvent(L->st, ev[k], 0));
        const uint64_t base = plan[batches[k].first].offset;
        std::vector<UnitIn> u;
        for (size_t q = batches[k].first; q < batches[k].second; ++q)
            u.push_back(UnitIn{plan[q].offset - base, plan[q].length, plan[q].init_start, plan[q].init_stop, q});
        STRACE("lane %d batch %zu: %zu units, encode", lane, k, u.size());
        encode_units(L, d_in + base, u, opt, L_STREAMS, true);
        STRACE("lane %d batch %zu: encoded, %llu stream bytes, device %.3f ms", lane, k,
               (unsigned long long)L->part_bytes, L->stats.ms_total);
        LaneBatch& r = out[k];
        r.lane = lane;
        r.coll_off = cend;
        r.bytes = L->part_bytes;
        r.segs = L->segs;
        r.names = L->names;
        r.stats = L->stats;
        if (hout) {   // appends (and collect reallocations) under the writer's lock: it reads collect.p
            {
                std::lock_guard<std::mutex> lk(hout->mu);
                collect_append(L, cend, L->part.p, L->part_bytes);
            }
            hout->finished(k, out);
        } else {
            collect_append(L, cend, L->part.p, L->part_bytes);
        }
    }
    HIP_CHECK(hipStreamSynchronize(L->st));
}

bool encode_host_pipelined(starch_ctx* c, const uint8_t* bed, uint64_t n, const starch_options& opt,
                           const HostRegistration& reg_in, uint8_t* hout_p = nullptr, uint64_t hout_cap = 0,
                           uint64_t* hout_len = nullptr)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    std::vector<shard::Unit> plan;
    shard::plan_units_upto(bed, n, 4096, plan);
    // batches of consecutive units: a small first one (the GPU starts early),
    // then an eighth of the input, halving toward the end (the encode after the
    // last copy is short)
    static const int nbatch = [] { const char* e = getenv("STARCH_PIPE_BATCHES"); return e ? std::max(1, atoi(e)) : 8; }();
    static const int nlanes = [] { const char* e = getenv("STARCH_LANES"); return e ? std::min(4, std::max(1, atoi(e))) : 2; }();
    static const int first_div = [] { const char* e = getenv("STARCH_PIPE_FIRST"); return e ? std::max(1, atoi(e)) : 24; }();
    std::vector<std::pair<size_t, size_t>> batches;   // [u0, u1)
    {
        const uint64_t target = std::max<uint64_t>(64ull << 20, n / (uint64_t)nbatch);
        uint64_t left = n;
        for (size_t k = 0; k < plan.size();) {
            uint64_t want = std::max<uint64_t>(32ull << 20, std::min<uint64_t>(target, left / 2));
            if (k == 0) want = std::max<uint64_t>(32ull << 20, std::min<uint64_t>(want, n / (uint64_t)first_div));
            size_t e = k;
            uint64_t b = 0;
            while (e < plan.size() && (b == 0 || b + plan[e].length <= want)) b += plan[e++].length;
            batches.emplace_back(k, e);
            left -= b;
            k = e;
        }
    }
    const int nl = (int)std::min<size_t>((size_t)nlanes, std::max<size_t>(1, batches.size()));
    std::vector<std::vector<size_t>> mine(nl);
    for (size_t k = 0; k < batches.size(); ++k) mine[k % nl].push_back(k);
    std::vector<starch_ctx*> lane(nl);
    for (int i = 0; i < nl; ++i) lane[i] = lane_ctx(c, i);
    std::vector<LaneBatch> res(batches.size());
    std::atomic<bool> stop{false}, saw_ff{false};
    std::unique_ptr<HostOut> hout;
    if (hout_p) {
        hout.reset(new HostOut());
        hout->out = hout_p;
        hout->cap = hout_cap;
        hout->done.assign(batches.size(), 0);
        hout->lane = lane;
    }
    std::vector<Caught> err(nl);
    // every batch crosses PCIe in input order on one copy stream, into one
    // device buffer, so the first batch arrives at full link rate
    if (!c->cst) HIP_CHECK(hipStreamCreateWithFlags(&c->cst, hipStreamNonBlocking));
    uint8_t* d_in = c->input.as<uint8_t>(n + 64);
    std::vector<hipEvent_t> ev(batches.size(), nullptr);
    for (auto& e : ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    try {
        for (size_t k = 0; k < batches.size(); ++k) {
            const uint64_t o = plan[batches[k].first].offset;
            const uint64_t e = batches[k].second < plan.size() ? plan[batches[k].second].offset : n;
            if (e > o) reg_in.h2d(d_in + o, bed + o, e - o, c->cst);
            HIP_CHECK(hipEventRecord(ev[k], c->cst));
        }
    } catch (...) {
        (void)hipStreamSynchronize(c->cst);
        for (auto& e : ev) (void)hipEventDestroy(e);
        throw;
    }
    auto work = [&](int i) {
        try {
            err[i].run([&] {
                Ctx g(lane[i]);
                run_lane(lane[i], d_in, plan, batches, ev, mine[i], opt, res, i, stop, hout.get());
            });
            if (err[i].code) stop = true;
        } catch (const FFInBatch&) {   // not an error: the caller falls back
            saw_ff = true;
            stop = true;
        }
    };
    {
        std::vector<std::thread> th;
        for (int i = 1; i < nl; ++i) th.emplace_back(work, i);
        work(0);
        for (auto& t : th) t.join();
    }
    (void)hipStreamSynchronize(c->cst);
    for (int i = 0; i < nl; ++i) (void)hipStreamSynchronize(lane[i]->st);   // device-to-host writes queued by other lanes
    for (auto& e : ev) (void)hipEventDestroy(e);
    for (auto& e : err) e.rethrow();
    if (saw_ff) return false;
    // archive: magic, the batches' streams in input order, index; one copy per
    // run of batches adjacent in a lane's collect buffer
    uint64_t end = 4;
    std::vector<starch_segment> segs;
    std::vector<std::string> names;
    std::vector<shard::CopyRun> runs;
    starch_stats st{};
    for (auto& r : res) {
        append_segments(segs, names, r.segs, r.names, end);
        shard::add_run(runs, r.lane, r.coll_off, end, r.bytes);
        end += r.bytes;
        add_stats(st, r.stats);   // (ms_total is set below)
    }
    std::string idx;
    if (opt.emit_index) idx = index_of(segs, names, end, opt);
    uint8_t* arch = c->archive.as<uint8_t>(align_up(end + idx.size() + 64, 256));
    HIP_CHECK(hipMemcpyAsync(arch, kMagic, 4, hipMemcpyHostToDevice, c->st));
    for (auto& r : runs)
        if (r.len)
            HIP_CHECK(hipMemcpyAsync(arch + r.dst_off, static_cast<uint8_t*>(lane[r.src]->collect.p) + r.src_off, r.len,
                                     hipMemcpyDeviceToDevice, c->st));
    if (!idx.empty()) HIP_CHECK(hipMemcpyAsync(arch + end, idx.data(), idx.size(), hipMemcpyHostToDevice, c->st));
    if (hout) {   // every batch went out already (all lanes finished); magic and index from the host
        if (hout->overflow || hout->off != end || end + idx.size() > hout_cap) {
            HIP_CHECK(hipStreamSynchronize(c->st));
            *hout_len = end + idx.size();   // the size needed; the buffer's contents are undefined
            throw StarchError(STARCH_ERR_MEM, "output buffer too small");
        }
        memcpy(hout_p, kMagic, 4);
        memcpy(hout_p + end, idx.data(), idx.size());
        *hout_len = end + idx.size();
    }
    HIP_CHECK(hipStreamSynchronize(c->st));
    st.input_bytes = n;
    st.n_segments = segs.size();
    st.ms_total = std::chrono::duration<float, std::milli>(clk::now() - t0).count();
    install_archive(c, segs, names, st, end + idx.size());
    return true;
}

// Host bytes into c->archive.  Large pinned inputs go through the pipeline: the
// PCIe copy of the next batch overlaps the encode (STARCH_PIPELINE=0 turns it
// off; pageable memory has no async copy); then true, and out (if given) holds
// the archive too.  Otherwise one copy and encode_device, and false.
bool encode_host(starch_ctx* c, const void* bed, uint64_t n, const starch_options& o, uint8_t* out = nullptr,
                 uint64_t cap = 0, uint64_t* out_len = nullptr)
{
    static const bool pipe_off = [] { const char* e = getenv("STARCH_PIPELINE"); return e && !strcmp(e, "0"); }();
    HostRegistration reg(pipe_off || o.reference_compat ? nullptr : bed, n, 256ull << 20);
    if (!pipe_off && !o.reference_compat && n >= (256ull << 20) && (reg.ok() || host_is_pinned(bed)) &&
        encode_host_pipelined(c, static_cast<const uint8_t*>(bed), n, o, reg, out, cap, out_len))
        return true;
    uint8_t* d = c->input.as<uint8_t>(n + 64);
    reg.h2d(d, bed, n, c->st);
    HIP_CHECK(hipStreamSynchronize(c->st));
    encode_device(c, d, n, o);
    return false;
}

// Multi-device encode of host bytes: plan units, LPT them over the contexts,
// encode every shard on its own device in its own host thread, then gather
// the finished streams into ctxs[0]'s HBM (peer copies over xGMI; a plain
// device copy when two contexts share a device) and write magic + index.
void encode_multi(starch_ctx* const* ctxs, int nctx, const uint8_t* bed, uint64_t n, const starch_options& opt)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    starch_ctx* c0 = ctxs[0];
    std::vector<shard::Unit> plan;
    shard::plan_units(bed, n, 64ull * (uint64_t)nctx, plan);
    std::vector<int32_t> shard_of;
    shard::assign_lpt(plan, nctx, shard_of);
    std::vector<std::vector<UnitIn>> mine(nctx);
    std::vector<uint64_t> dev_bytes(nctx, 0);
    for (size_t k = 0; k < plan.size(); ++k) {
        const int s = shard_of[k];
        mine[s].push_back(UnitIn{dev_bytes[s], plan[k].length, plan[k].init_start, plan[k].init_stop, k});
        dev_bytes[s] += plan[k].length;
    }
    std::vector<Caught> err(nctx);
    auto work = [&](int s) {
        starch_ctx* c = ctxs[s];
        err[s].run([&] {
            Ctx g(c);
            uint8_t* d = c->input.as<uint8_t>(dev_bytes[s] + 64);
            for (auto& u : mine[s]) {
                const uint64_t src = plan[u.id].offset;
                if (u.len) HIP_CHECK(hipMemcpyAsync(d + u.off, bed + src, u.len, hipMemcpyHostToDevice, c->st));
            }
            encode_units(c, d, mine[s], opt, L_STREAMS);
        });
    };
    {
        std::vector<std::thread> th;
        for (int s = 1; s < nctx; ++s) th.emplace_back(work, s);
        work(0);
        for (auto& t : th) t.join();
    }
    for (int s = 0; s < nctx; ++s) err[s].rethrow("shard " + std::to_string(s) + ": ");
    // gather: archive order = unit order
    std::vector<uint64_t> unit_of, bytes;
    std::vector<std::pair<int, uint64_t>> src;   // (shard, segment) of each gathered segment
    for (int s = 0; s < nctx; ++s)
        for (uint64_t j = 0; j < ctxs[s]->segs.size(); ++j) {
            unit_of.push_back(ctxs[s]->segs[j].unit);
            bytes.push_back(ctxs[s]->segs[j].stream_bytes);
            src.emplace_back(s, j);
        }
    const uint64_t nseg = unit_of.size();
    std::vector<uint64_t> order, offset;
    uint64_t end = 4;
    shard::layout(unit_of.data(), bytes.data(), nseg, 4, order, offset, &end);
    std::vector<starch_segment> segs(nseg);
    std::vector<std::string> names(nseg);
    std::vector<shard::CopyRun> runs;   // one copy per run of segments adjacent both in the part and in the archive
    for (uint64_t k = 0; k < nseg; ++k) {
        const auto& sj = src[order[k]];
        segs[k] = ctxs[sj.first]->segs[sj.second];
        shard::add_run(runs, sj.first, segs[k].stream_offset, offset[order[k]], bytes[order[k]]);
        segs[k].stream_offset = offset[order[k]];
        names[k] = ctxs[sj.first]->names[sj.second];
    }
    std::string idx;
    if (opt.emit_index && !opt.reference_compat) idx = index_of(segs, names, end, opt);
    Ctx g(c0);
    const uint64_t total = opt.reference_compat ? 4 : end + idx.size();
    uint8_t* out = c0->archive.as<uint8_t>(align_up(total + 64, 256));
    HIP_CHECK(hipMemcpyAsync(out, kMagic, 4, hipMemcpyHostToDevice, c0->st));
    if (!opt.reference_compat) {
        for (int s = 0; s < nctx; ++s) {
            starch_ctx* c = ctxs[s];
            if (c->device != c0->device) (void)hipDeviceEnablePeerAccess(c->device, 0);
            (void)hipGetLastError();   // already enabled / not supported: the copy still works
        }
        for (auto& r : runs) {
            if (!r.len) continue;
            starch_ctx* c = ctxs[r.src];
            const uint8_t* from = static_cast<uint8_t*>(c->part.p) + r.src_off;
            if (c->device == c0->device)
                HIP_CHECK(hipMemcpyAsync(out + r.dst_off, from, r.len, hipMemcpyDeviceToDevice, c0->st));
            else
                HIP_CHECK(hipMemcpyPeerAsync(out + r.dst_off, c0->device, from, c->device, r.len, c0->st));
        }
        if (!idx.empty()) HIP_CHECK(hipMemcpyAsync(out + end, idx.data(), idx.size(), hipMemcpyHostToDevice, c0->st));
    }
    HIP_CHECK(hipStreamSynchronize(c0->st));
    starch_stats st{};
    for (int s = 0; s < nctx; ++s) add_stats(st, ctxs[s]->stats, true);   // (ms_total is set below)
    st.input_bytes = n;
    st.n_segments = nseg;
    st.ms_total = std::chrono::duration<float, std::milli>(clk::now() - t0).count();
    install_archive(c0, segs, names, st, total);
}

}  // namespace

extern "C" {

int starch_encode_device(starch_ctx* c, const void* d_bed, uint64_t n, const starch_options* opt)
{
    GUARD(c)
    const starch_options o = options_of(opt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    if (n && !d_bed) return STARCH_ERR_ARG;
    encode_device(c, static_cast<const uint8_t*>(d_bed), n, o);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_encode_host(starch_ctx* c, const void* bed, uint64_t n, const starch_options* opt)
{
    GUARD(c)
    if (n && !bed) return STARCH_ERR_ARG;
    const starch_options o = options_of(opt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    encode_host(c, bed, n, o);
    return STARCH_OK;
    END_GUARD(c)
}

static int units_in(const starch_unit* units, const uint64_t* ids, uint64_t nunits, std::vector<UnitIn>& u)
{
    if (nunits && !units) return STARCH_ERR_ARG;
    u.resize(nunits);
    for (uint64_t k = 0; k < nunits; ++k)
        u[k] = UnitIn{units[k].offset, units[k].length, units[k].init_start, units[k].init_stop, ids ? ids[k] : k};
    for (uint64_t k = 1; k < nunits; ++k)
        if (u[k].id <= u[k - 1].id) return STARCH_ERR_ARG;   // units in input order
    return STARCH_OK;
}

int starch_encode_host_into(starch_ctx* c, const void* bed, uint64_t n, const starch_options* opt, void* out,
                            uint64_t cap, uint64_t* out_len)
{
    GUARD(c)
    if ((n && !bed) || !out || !out_len) return STARCH_ERR_ARG;
    const starch_options o = options_of(opt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    if (encode_host(c, bed, n, o, static_cast<uint8_t*>(out), cap, out_len)) return STARCH_OK;
    if (cap < c->archive_bytes) { *out_len = c->archive_bytes; return STARCH_ERR_MEM; }
    if (c->archive_bytes) HIP_CHECK(hipMemcpyAsync(out, c->archive.p, c->archive_bytes, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    *out_len = c->archive_bytes;
    return STARCH_OK;
    END_GUARD(c)
}

int starch_encode_units_device(starch_ctx* c, const void* d_base, const starch_unit* units, const uint64_t* unit_ids,
                               uint64_t nunits, const starch_options* opt)
{
    GUARD(c)
    const starch_options o = options_of(opt);
    if (!options_ok(o) || (nunits && !d_base)) return STARCH_ERR_ARG;
    std::vector<UnitIn> u;
    int rc = units_in(units, unit_ids, nunits, u);
    if (rc) return rc;
    encode_units(c, static_cast<const uint8_t*>(d_base), u, o, L_STREAMS, false, true);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_encode_units_host(starch_ctx* c, const void* bed, const starch_unit* units, const uint64_t* unit_ids,
                             uint64_t nunits, const starch_options* opt)
{
    GUARD(c)
    const starch_options o = options_of(opt);
    if (!options_ok(o) || (nunits && !bed)) return STARCH_ERR_ARG;
    std::vector<UnitIn> u;
    int rc = units_in(units, unit_ids, nunits, u);
    if (rc) return rc;
    uint64_t total = 0;
    for (auto& x : u) total += x.len;
    uint8_t* d = c->input.as<uint8_t>(total + 64);
    uint64_t pos = 0;
    const uint8_t* h = static_cast<const uint8_t*>(bed);
    for (auto& x : u) {   // packed copies; coalesce units adjacent on the host
        const uint64_t src = x.off;
        x.off = pos;
        if (x.len) HIP_CHECK(hipMemcpyAsync(d + pos, h + src, x.len, hipMemcpyHostToDevice, c->st));
        pos += x.len;
    }
    encode_units(c, d, u, o, L_STREAMS);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_streams_device(starch_ctx* c, const void** d_ptr, uint64_t* n)
{
    if (!c || !d_ptr || !n) return STARCH_ERR_ARG;
    if (!c->have || c->gathered) return STARCH_ERR_STATE;
    *d_ptr = c->part.p;
    *n = c->part_bytes;
    return STARCH_OK;
}

int starch_streams_copy(starch_ctx* c, void* dst, uint64_t cap)
{
    GUARD(c)
    if (!c->have || c->gathered) return STARCH_ERR_STATE;
    if (cap < c->part_bytes || (c->part_bytes && !dst)) return STARCH_ERR_MEM;
    if (c->part_bytes) HIP_CHECK(hipMemcpyAsync(dst, c->part.p, c->part_bytes, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_encode_multi_host(starch_ctx* const* ctxs, int nctx, const void* bed, uint64_t n, const starch_options* opt)
{
    if (!ctxs || nctx < 1 || (n && !bed)) return STARCH_ERR_ARG;
    for (int i = 0; i < nctx; ++i) {
        if (!ctxs[i]) return STARCH_ERR_ARG;
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return STARCH_ERR_ARG;   // one context per shard
    }
    starch_ctx* c = ctxs[0];
    GUARD(c)
    const starch_options o = options_of(opt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    if (nctx == 1) {
        uint8_t* d = c->input.as<uint8_t>(n + 64);
        if (n) HIP_CHECK(hipMemcpyAsync(d, bed, n, hipMemcpyHostToDevice, c->st));
        encode_device(c, d, n, o);
    } else {
        encode_multi(ctxs, nctx, static_cast<const uint8_t*>(bed), n, o);
    }
    return STARCH_OK;
    END_GUARD(c)
}

int starch_plan_units(const void* bed, uint64_t n, uint64_t max_units, starch_unit* out, uint64_t* nunits)
{
    return starch_plan_units_from(bed, n, max_units, 0, 0, out, nunits);
}

int starch_plan_units_from(const void* bed, uint64_t n, uint64_t max_units, int64_t init_start, int64_t init_stop,
                           starch_unit* out, uint64_t* nunits)
{
    if (!nunits || !out || max_units < 1 || (n && !bed)) return STARCH_ERR_ARG;
    try {
        std::vector<shard::Unit> u;
        shard::plan_units(static_cast<const uint8_t*>(bed), n, max_units, u, init_start, init_stop);
        for (size_t k = 0; k < u.size(); ++k)
            out[k] = starch_unit{u[k].offset, u[k].length, u[k].init_start, u[k].init_stop};
        *nunits = u.size();
    } catch (const std::exception&) {
        return STARCH_ERR_MEM;
    }
    return STARCH_OK;
}

int starch_assign_shards(const starch_unit* units, uint64_t nunits, int nshards, int32_t* shard_of)
{
    if ((nunits && (!units || !shard_of)) || nshards < 1) return STARCH_ERR_ARG;
    std::vector<shard::Unit> u(nunits);
    for (uint64_t k = 0; k < nunits; ++k)
        u[k] = shard::Unit{units[k].offset, units[k].length, units[k].init_start, units[k].init_stop};
    std::vector<int32_t> s;
    shard::assign_lpt(u, nshards, s);
    if (nunits) memcpy(shard_of, s.data(), nunits * sizeof(int32_t));
    return STARCH_OK;
}

int starch_archive_size(starch_ctx* c, uint64_t* n)
{
    if (!c || !n) return STARCH_ERR_ARG;
    if (!c->have || c->streamed) return STARCH_ERR_STATE;
    *n = c->archive_bytes;
    return STARCH_OK;
}

int starch_archive_device(starch_ctx* c, const void** p)
{
    if (!c || !p) return STARCH_ERR_ARG;
    if (!c->have || c->streamed) return STARCH_ERR_STATE;
    *p = c->archive.p;
    return STARCH_OK;
}

int starch_archive_copy(starch_ctx* c, void* dst, uint64_t cap)
{
    GUARD(c)
    if (!c->have || c->streamed) return STARCH_ERR_STATE;
    if (cap < c->archive_bytes || !dst) return STARCH_ERR_MEM;
    if (c->archive_bytes)
        HIP_CHECK(hipMemcpyAsync(dst, c->archive.p, c->archive_bytes, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_segment_count(starch_ctx* c, uint64_t* n)
{
    if (!c || !n) return STARCH_ERR_ARG;
    if (!c->have) return STARCH_ERR_STATE;
    *n = c->segs.size();
    return STARCH_OK;
}

int starch_segments(starch_ctx* c, starch_segment* out, uint64_t cap)
{
    if (!c || (!out && cap)) return STARCH_ERR_ARG;
    if (!c->have) return STARCH_ERR_STATE;
    if (cap < c->segs.size()) return STARCH_ERR_MEM;
    if (!c->segs.empty()) memcpy(out, c->segs.data(), c->segs.size() * sizeof(starch_segment));
    return STARCH_OK;
}

int starch_segment_name(starch_ctx* c, uint64_t i, char* buf, uint64_t cap, uint64_t* len)
{
    if (!c) return STARCH_ERR_ARG;
    if (!c->have) return STARCH_ERR_STATE;
    if (i >= c->names.size()) return STARCH_ERR_ARG;
    const std::string& s = c->names[i];
    if (len) *len = s.size();
    if (buf) {
        if (cap < s.size()) return STARCH_ERR_MEM;
        memcpy(buf, s.data(), s.size());
    }
    return STARCH_OK;
}

int starch_get_stats(starch_ctx* c, starch_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    *out = c->stats;
    return STARCH_OK;
}

// transform stage only on device-resident BED bytes (segments: stream_offset =
// offset of the segment's text in the text buffer)
static void transform_only(starch_ctx* c, const uint8_t* d, uint64_t n, int64_t init_start = 0, int64_t init_stop = 0)
{
    hipEvent_t* tv = c->timers();
    hipEvent_t e0 = tv[0], e1 = tv[1];
    HIP_CHECK(hipEventRecord(e0, c->st));
    TransformResult tr;
    c->tf.run(d, n, c->st, tr, init_start, init_stop);
    HIP_CHECK(hipEventRecord(e1, c->st));
    std::vector<SegInfo> si(tr.n_segments);
    if (tr.n_segments)
        HIP_CHECK(hipMemcpyAsync(si.data(), c->tf.seg_info_dev, tr.n_segments * sizeof(SegInfo),
                                 hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->segs.assign(tr.n_segments, starch_segment{});
    PendingNames pnames;
    fetch_names(c, d, si, pnames);
    for (uint64_t s = 0; s < tr.n_segments; ++s) {
        c->segs[s].line_count = si[s].line_count;
        c->segs[s].text_bytes = si[s].text_len;
        c->segs[s].stream_offset = si[s].text_off;   // transform-only: offset into the text
        c->segs[s].name_len = si[s].name_len;
    }
    finish_names(c, pnames);
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    c->stats = stats_of(bz::Stats(), ms, ms);
    c->stats.input_bytes = n;
    c->stats.n_lines = tr.n_lines;
    c->stats.n_segments = tr.n_segments;
    c->stats.text_bytes = tr.text_bytes;
    c->text_bytes = tr.text_bytes;
    c->text_dev = c->tf.text;
    c->archive_bytes = 0;
    c->have = true;
}

int starch_transform_host(starch_ctx* c, const void* bed, uint64_t n)
{
    return starch_transform_host_init(c, bed, n, 0, 0);
}

int starch_transform_host_init(starch_ctx* c, const void* bed, uint64_t n, int64_t init_start, int64_t init_stop)
{
    GUARD(c)
    if (n && !bed) return STARCH_ERR_ARG;
    uint8_t* d = c->input.as<uint8_t>(n + 64);
    {
        HostRegistration reg(bed, n, 64ull << 20);   // (a mapped file: DMA instead of staging)
        reg.h2d(d, bed, n, c->st);
        HIP_CHECK(hipStreamSynchronize(c->st));
    }
    transform_only(c, d, n, init_start, init_stop);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_transform_device(starch_ctx* c, const void* d_bed, uint64_t n)
{
    GUARD(c)
    if (n && !d_bed) return STARCH_ERR_ARG;
    transform_only(c, static_cast<const uint8_t*>(d_bed), n);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_text_size(starch_ctx* c, uint64_t* n)
{
    if (!c || !n) return STARCH_ERR_ARG;
    if (!c->have) return STARCH_ERR_STATE;
    *n = c->text_bytes;
    return STARCH_OK;
}

int starch_text_copy(starch_ctx* c, void* dst, uint64_t cap)
{
    GUARD(c)
    if (!c->have) return STARCH_ERR_STATE;
    if (cap < c->text_bytes) return STARCH_ERR_MEM;
    if (c->text_bytes) HIP_CHECK(hipMemcpyAsync(dst, c->text_dev, c->text_bytes, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_text_read(starch_ctx* c, uint64_t off, void* dst, uint64_t n)
{
    GUARD(c)
    if (!c->have) return STARCH_ERR_STATE;
    if (off > c->text_bytes || n > c->text_bytes - off || (n && !dst)) return STARCH_ERR_ARG;
    if (n) HIP_CHECK(hipMemcpyAsync(dst, c->text_dev + off, n, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_bz2_compress_many_device(starch_ctx* c, const void* d_in, const uint64_t* offs, const uint64_t* lens,
                                    uint64_t nstreams, int bs, void* d_out, uint64_t cap, uint64_t* out_offs,
                                    uint64_t* out_lens)
{
    GUARD(c)
    if (bs < 1 || bs > 9 || (nstreams && (!offs || !lens || !out_offs || !out_lens))) return STARCH_ERR_ARG;
    std::vector<bz::StreamIn> sin(nstreams);
    for (uint64_t s = 0; s < nstreams; ++s) {
        sin[s].text_off = offs[s];
        sin[s].text_len = lens[s];
        sin[s].final_run_joins = 1;
        sin[s].group = (uint32_t)s;
    }
    std::vector<bz::StreamOut> outs;
    c->enc.plan_and_encode(static_cast<const uint8_t*>(d_in), sin, bs, static_cast<uint8_t*>(d_out), cap, 0, outs,
                           c->st, nullptr);
    HIP_CHECK(hipStreamSynchronize(c->st));
    for (uint64_t s = 0; s < nstreams; ++s) { out_offs[s] = outs[s].out_off; out_lens[s] = outs[s].bytes; }
    c->bz_nblocks = nstreams ? outs[0].n_blocks : 0;
    c->bz_crc = nstreams ? outs[0].combined_crc : 0;
    return STARCH_OK;
    END_GUARD(c)
}

int starch_bz2_compress_host(starch_ctx* c, const void* in, uint64_t n, int bs, void* out, uint64_t cap,
                             uint64_t* out_len)
{
    GUARD(c)
    if (bs < 1 || bs > 9 || !out_len || (n && !in)) return STARCH_ERR_ARG;
    uint8_t* d = c->raw_in.as<uint8_t>(n + 64);
    if (n) HIP_CHECK(hipMemcpyAsync(d, in, n, hipMemcpyHostToDevice, c->st));
    uint64_t ocap = n + n / 50 + 4096;
    uint8_t* dout = c->raw_out.as<uint8_t>(ocap);
    uint64_t off = 0, len = 0, zero = 0;
    int rc = starch_bz2_compress_many_device(c, d, &zero, &n, 1, bs, dout, ocap, &off, &len);
    if (rc) return rc;
    *out_len = len;
    if (cap < len) return STARCH_ERR_MEM;
    HIP_CHECK(hipMemcpyAsync(out, dout + off, len, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return STARCH_OK;
    END_GUARD(c)
}

int starch_bz2_stream_info(starch_ctx* c, uint32_t* n_blocks, uint32_t* combined_crc)
{
    if (!c || !n_blocks || !combined_crc) return STARCH_ERR_ARG;
    *n_blocks = c->bz_nblocks;
    *combined_crc = c->bz_crc;
    return STARCH_OK;
}

}  // extern "C"
