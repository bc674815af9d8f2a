// starch_amd/csrc/api_stream.hip -- the C ABI's streaming encode (starch_stream_*).
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "api_int.hpp"
#include "shard.hpp"

using namespace api;

// ---- streaming ingestion (starch_stream_*) ---------------------------------
// The input arrives in pieces of any size.  Bytes not yet encoded are held in
// pinned host memory from a segment boundary on, together with the sscanf
// values current before them (shard.cpp: a unit boundary is any line start
// where the chr token changes, and a unit encoded on its own with those
// values gives exactly the streams of the whole input).  When at least a batch
// of input is held, the planner finds the last segment boundary among the
// complete lines; the prefix before it goes to the session's encoder thread
// (H2D, transform, bzip2 on the GPU, streams D2H into the ready bytes) while
// the held tail -- the last chromosome run, which may continue in the next
// piece -- moves to the other pinned buffer and the caller keeps feeding.
// end() encodes the rest and appends the index.

namespace {

void stream_reserve(starch_ctx* c, int i, uint64_t need)
{
    auto& m = c->sm;
    if (need <= m.cap[i]) return;
    const uint64_t cap = align_up(std::max<uint64_t>(need, 2 * m.cap[i]), 1ull << 20);
    void* p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, cap, hipHostMallocDefault));
    const bool keep = i == m.cur && m.held_n;
    if (keep) memcpy(p, m.buf[i], m.held_n);
    if (m.buf[i]) (void)hipHostFree(m.buf[i]);
    m.buf[i] = static_cast<uint8_t*>(p);
    m.cap[i] = cap;
    // the device mirror keeps the held bytes too (their H2D is ordered before on cst)
    DevBuf nb;
    uint8_t* d = nb.as<uint8_t>(cap + 64);
    if (keep) HIP_CHECK(hipMemcpyAsync(d, m.dbuf[i].p, m.held_n, hipMemcpyDeviceToDevice, c->cst));
    HIP_CHECK(hipStreamSynchronize(c->cst));
    std::swap(m.dbuf[i].p, nb.p);
    std::swap(m.dbuf[i].cap, nb.cap);
}

// pin buffer i (not the current one: nothing held) for `need` bytes, with its
// device mirror; the session's prepin thread runs this while the first batch
// is read
void stream_prepin_one(starch_ctx* c, int i, uint64_t need)
{
    auto& m = c->sm;
    if (need <= m.cap[i]) return;
    const uint64_t cap = align_up(need, 1ull << 20);
    void* p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, cap, hipHostMallocDefault));
    if (m.buf[i]) (void)hipHostFree(m.buf[i]);
    m.buf[i] = static_cast<uint8_t*>(p);
    m.cap[i] = cap;
    DevBuf nb;
    (void)nb.as<uint8_t>(cap + 64);
    std::swap(m.dbuf[i].p, nb.p);
    std::swap(m.dbuf[i].cap, nb.cap);
}

void stream_prepin_join(starch_ctx* c)
{
    if (c->sm.prepin.joinable()) c->sm.prepin.join();
}

// Streaming inside a chromosome (bzip2): a batch may end inside a chromosome
// (open) and the next one then starts with the last line of it (ctx bytes of
// context).  The chromosome's stream is encoded in pieces: every batch
// encodes the complete bzip2 blocks of its text and carries the text after
// the last block boundary (a block starts a fresh RLE1 run, so the rest
// encodes the same in front of the next batch's text), the bits of the last
// partial byte, the combined CRC and the block count to the next piece; the
// header goes with the first piece, the trailer with the last one.  The
// context line is transformed on its own as well, and that output (the line
// as a segment's first) is dropped from the batch's first segment.
void stream_flush(starch_ctx::Streaming& m);

void stream_encode_pieces(starch_ctx* c, const uint8_t* d, uint64_t n, int64_t is, int64_t ip, uint64_t ctx,
                          bool open)
{
    auto& m = c->sm;
    auto& os = m.os;
    hipEvent_t* tv = c->timers();   // owned by the context: nothing to release on a throw
    hipEvent_t e0 = tv[0], e1 = tv[1], e2 = tv[2];
    HIP_CHECK(hipEventRecord(e0, c->st));
    c->stats = starch_stats{};
    c->stats.input_bytes = n - ctx;
    uint64_t o_ctx = 0;
    if (ctx) {
        TransformResult tc;
        c->tf.run(d, ctx, c->st, tc, is, ip);
        if (tc.n_lines != 1 || tc.n_segments != 1) throw StarchError(STARCH_ERR_INTERNAL, "stream: context line");
        o_ctx = tc.text_bytes;
    }
    TransformResult tr;
    c->tf.run(d, n, c->st, tr, is, ip);
    std::vector<SegInfo> si(tr.n_segments);
    if (tr.n_segments)
        HIP_CHECK(hipMemcpyAsync(si.data(), c->tf.seg_info_dev, tr.n_segments * sizeof(SegInfo), hipMemcpyDeviceToHost,
                                 c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (ctx) {
        if (si.empty() || si[0].line_count < 1 || si[0].text_len < o_ctx)
            throw StarchError(STARCH_ERR_INTERNAL, "stream: context segment");
        si[0].text_off += o_ctx;
        si[0].text_len -= o_ctx;
        si[0].line_count -= 1;
        si[0].first_line += 1;
    }
    HIP_CHECK(hipEventRecord(e1, c->st));
    const uint64_t nseg = si.size();
    const bool cont = os.active;
    if (cont != (ctx > 0) || nseg == 0) throw StarchError(STARCH_ERR_INTERNAL, "stream: piece state");
    PendingNames pn;
    fetch_names(c, d, si, pn);
    // the open stream's rest, then the batch's text from segment 0 on
    const uint8_t* T = c->tf.text;
    const uint64_t new0 = si[0].text_len;
    if (cont && os.rest_len) {
        const uint64_t R = os.rest_len, t0 = si[0].text_off, span = tr.text_bytes - t0;
        uint8_t* Tb = c->text_all.as<uint8_t>(R + span + 64);
        HIP_CHECK(hipMemcpyAsync(Tb, os.rest.p, R, hipMemcpyDeviceToDevice, c->st));
        if (span) HIP_CHECK(hipMemcpyAsync(Tb + R, c->tf.text + t0, span, hipMemcpyDeviceToDevice, c->st));
        for (auto& x : si) x.text_off = x.text_off - t0 + R;
        si[0].text_off = 0;
        si[0].text_len += R;
        T = Tb;
    }
    std::vector<bz::StreamIn> sin = streams_of(si);
    if (cont) {
        sin[0].cont = 1;
        sin[0].phase = os.phase;
        sin[0].comb_in = os.comb;
    }
    if (open) {
        sin[nseg - 1].open = 1;
        sin[nseg - 1].final_run_joins = 0;
    }
    std::vector<bz::StreamOut> outs;
    bz::Stats bst;
    c->enc.plan(T, sin, m.opt.block_size_100k, c->st, outs, &bst);
    finish_names(c, pn);
    if (cont && c->names[0] != os.name) throw StarchError(STARCH_ERR_INTERNAL, "stream: continued chromosome");
    uint64_t total = 0;
    for (auto& o : outs) total = std::max(total, o.out_off + o.bytes);
    const uint64_t cap = align_up(total + 64, 256);
    uint8_t* out = c->part.as<uint8_t>(cap);
    c->enc.emit(out, cap, 0, outs, c->st, &bst);
    uint8_t* part = static_cast<uint8_t*>(m.back[0].get(total + 64));   // pinned: D2H at full PCIe rate
    if (total) HIP_CHECK(hipMemcpyAsync(part, out, total, hipMemcpyDeviceToHost, c->st));
    if (open) {   // the text after the last complete block waits for the next batch
        const uint64_t r0 = c->enc.open_rest(), r1 = sin[nseg - 1].text_off + sin[nseg - 1].text_len;
        os.rest_len = r1 - r0;
        if (os.rest.cap < os.rest_len + 64) HIP_CHECK(hipStreamSynchronize(c->st));   // T may hold the old rest
        uint8_t* rp = os.rest.as<uint8_t>(os.rest_len + 64);
        if (os.rest_len) HIP_CHECK(hipMemcpyAsync(rp, T + r0, os.rest_len, hipMemcpyDeviceToDevice, c->st));
    }
    HIP_CHECK(hipEventRecord(e2, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->enc.resolve_timers(&bst);
    float ms_t = 0, ms_all = 0;
    HIP_CHECK(hipEventElapsedTime(&ms_t, e0, e1));
    HIP_CHECK(hipEventElapsedTime(&ms_all, e0, e2));
    STRACE("stream batch %llu: %llu bytes in %llu segments (%s%s), device %.3f ms", (unsigned long long)m.batches,
           (unsigned long long)(n - ctx), (unsigned long long)nseg, cont ? "continues a chromosome" : "",
           open ? (cont ? ", open" : "open") : "", ms_all);
    std::lock_guard<std::mutex> lk(m.mu);
    for (uint64_t s = 0; s < nseg; ++s) {
        const bz::StreamOut& o = outs[s];
        const bool is_cont = s == 0 && cont, is_open = s + 1 == nseg && open;
        const uint8_t* b = part + o.out_off;
        const uint64_t bits = bz::frame_bits(o.frame) + o.block_bits;
        const uint64_t full = is_open ? bits / 8 : o.bytes;   // an open piece keeps its last partial byte
        const size_t at = m.ready.size();
        m.ready.insert(m.ready.end(), b, b + full);
        if (is_cont && full) m.ready[at] |= os.carry;   // the previous piece's bits of this byte
        uint8_t carry = 0;
        if (is_open && (bits & 7u)) carry = (uint8_t)(b[full] | ((is_cont && full == 0) ? os.carry : 0u));
        const uint64_t off = m.stream_end;
        m.stream_end += full;
        if (!is_cont) {               // a stream starts here
            os.clear();
            if (is_open) {
                os.active = true;
                os.name = c->names[s];
                os.off = off;
            }
        }
        if (is_cont || is_open) {     // a piece of a stream encoded in pieces
            os.bytes += full;
            os.n_blocks += o.n_blocks;
            os.comb = o.combined_crc;
            os.lines += si[s].line_count;
            os.text_bytes += s == 0 ? new0 : si[s].text_len;
            if (is_open) {
                os.phase = (uint32_t)(bits & 7u);
                os.carry = carry;
                continue;
            }
        }
        starch_segment g{};
        g.line_count = is_cont ? os.lines : si[s].line_count;
        g.text_bytes = is_cont ? os.text_bytes : si[s].text_len;
        g.name_len = c->names[s].size();
        g.stream_offset = is_cont ? os.off : off;
        g.stream_bytes = is_cont ? os.bytes : o.bytes;
        g.n_blocks = is_cont ? os.n_blocks : o.n_blocks;
        g.combined_crc = o.combined_crc;
        g.unit = m.batches;
        m.segs.push_back(g);
        m.names.push_back(c->names[s]);
        if (is_cont) os.clear();
    }
    if (!open) os.rest_len = 0;
    ++m.batches;
    ++m.seq_commit;                   // (pieces start with every earlier batch appended)
    starch_stats x = stats_of(bst, ms_t, ms_all);
    x.n_lines = tr.n_lines - (ctx ? 1 : 0);
    x.text_bytes = tr.text_bytes - o_ctx;
    add_stats(m.stats, x);
    stream_flush(m);                 // batches after it that finished first
}

// append the next batch in hand-over order to the ready bytes (m.mu held)
void stream_append(starch_ctx::Streaming& m, const uint8_t* b, uint64_t nb, const std::vector<starch_segment>& segs,
                   const std::vector<std::string>& names, const starch_stats& x)
{
    m.ready.insert(m.ready.end(), b, b + nb);
    append_segments(m.segs, m.names, segs, names, m.stream_end);
    for (size_t s = m.segs.size() - segs.size(); s < m.segs.size(); ++s) m.segs[s].unit = m.batches;
    m.stream_end += nb;
    ++m.batches;
    ++m.seq_commit;
    add_stats(m.stats, x);
    stream_flush(m);
}

// the parked batches that are next in hand-over order (m.mu held)
void stream_flush(starch_ctx::Streaming& m)
{
    for (auto it = m.done.find(m.seq_commit); it != m.done.end(); it = m.done.find(m.seq_commit)) {
        starch_ctx::Streaming::Done d = std::move(it->second);
        m.done.erase(it);
        stream_append(m, d.bytes.data(), d.bytes.size(), d.segs, d.names, d.stats);
    }
}

// lane `lane`: encode the job's batch (segment boundary to segment boundary,
// or to the end) and append its streams in hand-over order
void stream_encode(starch_ctx* c, int lane, const starch_ctx::Streaming::Job& j)
{
    auto& m = c->sm;
    starch_ctx* L = lane ? c->lanes[lane - 1].get() : c;
    if (m.opt.reference_compat) {     // the reference writes only the magic (hpp:765-769)
        std::lock_guard<std::mutex> lk(m.mu);
        if (j.seq == m.seq_commit) stream_append(m, nullptr, 0, {}, {}, starch_stats{});
        else m.done[j.seq] = starch_ctx::Streaming::Done{};
        return;
    }
    const uint8_t* d = static_cast<const uint8_t*>(m.dbuf[j.bufi].p);
    // the batch's H2D (copy stream) must be done before any kernel of the
    // lane reads it -- the piece path (context line + open stream) included
    HIP_CHECK(hipStreamWaitEvent(L->st, m.buf_ev[j.bufi], 0));
    if (j.ctx || j.open || j.cont) {   // handed over with no other batch in flight, to lane 0
        if (lane) throw StarchError(STARCH_ERR_INTERNAL, "stream: piece batch on an extra lane");
        stream_encode_pieces(c, d, j.n, j.is, j.ip, j.ctx, j.open);
        return;
    }
    STRACE("stream batch %llu (lane %d): %llu bytes, encode", (unsigned long long)j.seq, lane, (unsigned long long)j.n);
    std::vector<UnitIn> u(1, UnitIn{0, j.n, j.is, j.ip, 0});
    encode_units(L, d, u, m.opt, L_STREAMS);
    STRACE("stream batch %llu: encoded, device %.3f ms", (unsigned long long)j.seq, L->stats.ms_total);
    uint8_t* part = static_cast<uint8_t*>(m.back[lane].get(L->part_bytes + 64));   // pinned: D2H at full PCIe rate
    if (L->part_bytes) HIP_CHECK(hipMemcpyAsync(part, L->part.p, L->part_bytes, hipMemcpyDeviceToHost, L->st));
    HIP_CHECK(hipStreamSynchronize(L->st));
    STRACE("stream batch %llu: streams read back", (unsigned long long)j.seq);
    std::unique_lock<std::mutex> lk(m.mu);
    if (j.seq == m.seq_commit) {
        stream_append(m, part, L->part_bytes, L->segs, L->names, L->stats);
    } else {                          // an earlier batch is still encoding on the other lane
        lk.unlock();
        starch_ctx::Streaming::Done dn;
        dn.bytes.assign(part, part + L->part_bytes);
        dn.segs = L->segs;
        dn.names = L->names;
        dn.stats = L->stats;
        lk.lock();
        if (j.seq == m.seq_commit) stream_append(m, dn.bytes.data(), dn.bytes.size(), dn.segs, dn.names, dn.stats);
        else m.done[j.seq] = std::move(dn);
    }
}

void stream_worker(starch_ctx* c, int lane)
{
    auto& m = c->sm;
    (void)hipSetDevice(c->device);
    for (;;) {
        starch_ctx::Streaming::Job j;
        {
            std::unique_lock<std::mutex> lk(m.mu);
            m.cv.wait(lk, [&] { return m.lj[lane].pending || m.stop; });
            if (!m.lj[lane].pending) return;
            j = m.lj[lane];
            m.lj[lane].pending = false;
            m.lj[lane].busy = true;
        }
        Caught err;
        err.run([&] { stream_encode(c, lane, j); });
        {
            std::lock_guard<std::mutex> lk(m.mu);
            m.lj[lane].busy = false;
            m.buf_busy[j.bufi] = false;
            if (err.code && !m.err) { m.err = err.code; m.err_msg = err.msg; }   // the session keeps its first error
        }
        m.cv.notify_all();
    }
}

bool lane_idle(const starch_ctx::Streaming& m, int i) { return !m.lj[i].pending && !m.lj[i].busy; }

// wait until every lane is idle; rethrow a lane's error
void stream_wait(starch_ctx* c)
{
    auto& m = c->sm;
    std::unique_lock<std::mutex> lk(m.mu);
    m.cv.wait(lk, [&] {
        for (int i = 0; i < starch_ctx::Streaming::NLANE; ++i)
            if (!lane_idle(m, i)) return false;
        return true;
    });
    if (m.err) throw StarchError(m.err, m.err_msg);
}

// a buffer other than buf[cur] that no lane holds (waits for one)
int stream_free_buf(starch_ctx* c)
{
    auto& m = c->sm;
    std::unique_lock<std::mutex> lk(m.mu);
    int o = -1;
    m.cv.wait(lk, [&] {
        if (m.err) return true;
        for (int i = 0; i < starch_ctx::Streaming::NBUF; ++i)
            if (i != m.cur && !m.buf_busy[i]) { o = i; return true; }
        return false;
    });
    if (m.err) throw StarchError(m.err, m.err_msg);
    return o;
}

// hand buf[cur][0, n) to a lane: its first m.ctx_len bytes are context
// (already counted), open: it ends inside a chromosome.  A batch cut inside a
// chromosome, and the one after it, depend on each other's state (the open
// bzip2 stream): they go to lane 0 with no other batch in flight; any other
// batch to the first idle lane
void stream_submit(starch_ctx* c, uint64_t n, bool open = false)
{
    auto& m = c->sm;
    const bool serial = m.ctx_len > 0 || open || m.last_open;
    HIP_CHECK(hipEventRecord(m.buf_ev[m.cur], c->cst));
    {
        std::unique_lock<std::mutex> lk(m.mu);
        int lane = -1;
        m.cv.wait(lk, [&] {
            if (m.err) return true;
            if (serial) {
                for (int i = 0; i < starch_ctx::Streaming::NLANE; ++i)
                    if (!lane_idle(m, i)) return false;
                lane = 0;
                return true;
            }
            for (int i = 0; i < starch_ctx::Streaming::NLANE; ++i)
                if (lane_idle(m, i)) { lane = i; return true; }
            return false;
        });
        if (m.err) throw StarchError(m.err, m.err_msg);
        auto& j = m.lj[lane];
        j.pending = true;
        j.bufi = m.cur;
        j.n = n;
        j.ctx = m.ctx_len;
        j.open = open;
        j.cont = m.last_open;
        j.is = m.init_start;
        j.ip = m.init_stop;
        j.seq = m.seq_next++;
        m.buf_busy[m.cur] = true;
        m.last_open = open;
        m.stats.input_bytes += n - m.ctx_len;
    }
    m.cv.notify_all();
}

// hand everything before the last segment boundary among the complete lines
// to the encoder thread; the tail moves to the other buffer
void stream_cut(starch_ctx* c)
{
    auto& m = c->sm;
    uint8_t* h = m.buf[m.cur];
    const void* nl = memrchr(h, '\n', m.held_n);
    std::vector<shard::Unit> u;
    if (nl) {
        const uint64_t lim = (uint64_t)(static_cast<const uint8_t*>(nl) - h) + 1;
        shard::plan_units_upto(h, lim, 4096, u, m.init_start, m.init_stop);   // commit cut the bytes at any 0xFF
    }
    if (u.size() < 2) {   // no chromosome boundary among the complete lines
        // bzip2 streams encode in pieces: a whole batch of one chromosome is
        // cut at its last complete line (STARCH_STREAM_HOLD=1: held whole)
        static const bool hold = [] { const char* e = getenv("STARCH_STREAM_HOLD"); return e && !strcmp(e, "1"); }();
        const bool pieces = !hold && m.opt.compression_method == STARCH_METHOD_BZIP2 && !m.opt.base_counts &&
                            !m.opt.reference_compat;
        uint64_t ls = 0, cut = 0;
        if (pieces && nl && m.held_n >= m.batch) {
            cut = (uint64_t)(static_cast<const uint8_t*>(nl) - h) + 1;
            ls = cut - 1;
            while (ls > 0 && h[ls - 1] != '\n') --ls;   // the last complete line [ls, cut): the next context
        }
        if (!pieces || ls <= m.ctx_len || ls == 0) {   // the held run continues
            m.try_at = m.held_n + m.batch / 2;
            return;
        }
        int64_t st = m.init_start, sp = m.init_stop;
        shard::values_before(h, 0, ls, &st, &sp);      // sscanf values current before the context line
        const uint64_t tail = m.held_n - ls;
        STRACE("stream cut inside a chromosome at %llu of %llu held", (unsigned long long)cut,
               (unsigned long long)m.held_n);
        stream_prepin_join(c);
        const int o = stream_free_buf(c);
        stream_reserve(c, o, std::max<uint64_t>(tail + m.batch + (m.batch >> 2), 1ull << 20));
        m.pool.copy(m.buf[o], h + ls, tail);
        HIP_CHECK(hipMemcpyAsync(m.dbuf[o].p, static_cast<uint8_t*>(m.dbuf[m.cur].p) + ls, tail,
                                 hipMemcpyDeviceToDevice, c->cst));
        stream_submit(c, cut, true);
        m.cur = o;
        m.held_n = tail;
        m.ctx_len = cut - ls;
        m.init_start = st;
        m.init_stop = sp;
        m.try_at = std::max(m.batch, tail + m.batch / 2);
        return;
    }
    const uint64_t cut = u.back().offset, tail = m.held_n - cut;
    stream_prepin_join(c);
    STRACE("stream cut at %llu of %llu held: wait for a free buffer", (unsigned long long)cut, (unsigned long long)m.held_n);
    const int o = stream_free_buf(c);
    STRACE("stream cut: buffer %d free", o);
    stream_reserve(c, o, std::max<uint64_t>(tail + m.batch + (m.batch >> 2), 1ull << 20));
    m.pool.copy(m.buf[o], h + cut, tail);
    if (tail)   // the tail's device bytes move with it (ordered after their H2D on cst)
        HIP_CHECK(hipMemcpyAsync(m.dbuf[o].p, static_cast<uint8_t*>(m.dbuf[m.cur].p) + cut, tail,
                                 hipMemcpyDeviceToDevice, c->cst));
    stream_submit(c, cut);
    m.cur = o;
    m.held_n = tail;
    m.ctx_len = 0;
    m.init_start = u.back().init_start;
    m.init_stop = u.back().init_stop;
    m.try_at = std::max(m.batch, tail + m.batch / 2);
}

}  // namespace

extern "C" {

int starch_stream_begin(starch_ctx* c, const starch_options* opt, uint64_t batch_bytes)
{
    GUARD(c)
    const starch_options o = options_of(opt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    c->stream_shutdown();                       // a session left open is abandoned
    auto& m = c->sm;
    if (!c->cst) HIP_CHECK(hipStreamCreateWithFlags(&c->cst, hipStreamNonBlocking));
    for (auto& e : m.buf_ev)
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (int i = 1; i < starch_ctx::Streaming::NLANE; ++i) lane_ctx(c, i);   // (created here, not in a worker)
    HIP_CHECK(hipStreamSynchronize(c->cst));
    m.active = true;
    m.eof = false;
    m.note = o.note ? o.note : "";
    m.opt = o;
    m.opt.note = o.note ? m.note.c_str() : nullptr;
    m.cur = 0;
    m.held_n = 0;
    m.ctx_len = 0;
    m.os.clear();                                // a session left open may have left a piece behind
    m.os.rest_len = 0;
    m.batch = batch_bytes ? batch_bytes : (256ull << 20);
    m.try_at = m.batch;
    m.batches = 0;
    m.init_start = m.init_stop = 0;
    for (auto& j : m.lj) j = starch_ctx::Streaming::Job{};
    for (auto& b : m.buf_busy) b = false;
    m.last_open = false;
    m.seq_next = m.seq_commit = 0;
    m.done.clear();
    m.err = 0;
    m.err_msg.clear();
    m.ready.assign(kMagic, kMagic + 4);
    m.ready_off = 0;
    m.stream_end = 4;
    m.segs.clear();
    m.names.clear();
    m.stats = starch_stats{};
    c->have = false;
    c->streamed = false;
    // the pinned buffers sized once for a batch plus a long held run (kept
    // across sessions: pinning is paid on the context's first session only):
    // the first now, the others on the prepin thread while the first fills
    // STARCH_PIN=eager (default): all three now; bg: the others on the prepin
    // thread; lazy: the others at their first use (stream_cut)
    static const int pin_mode = [] {
        const char* e = getenv("STARCH_PIN");
        return e && !strcmp(e, "bg") ? 1 : e && !strcmp(e, "lazy") ? 2 : 0;
    }();
    stream_reserve(c, 0, pin_mode ? m.batch + m.batch / 2 : 2 * m.batch);
    bool more = false;
    for (int i = 1; i < starch_ctx::Streaming::NBUF; ++i) more |= m.cap[i] < 2 * m.batch;
    if (more && pin_mode == 0)
        for (int i = 1; i < starch_ctx::Streaming::NBUF; ++i) stream_reserve(c, i, 2 * m.batch);
    else if (more && pin_mode == 1)
        m.prepin = std::thread([c]() {
            (void)hipSetDevice(c->device);
            try {
                for (int i = 1; i < starch_ctx::Streaming::NBUF; ++i) stream_prepin_one(c, i, 2 * c->sm.batch);
            } catch (const StarchError& e) {   // the next stream_reserve of that buffer retries and reports
                STRACE("prepin failed: %s", e.what());
            }
        });
    for (int i = 0; i < starch_ctx::Streaming::NLANE; ++i) m.workers[i] = std::thread(stream_worker, c, i);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_stream_window(starch_ctx* c, uint64_t min_bytes, void** ptr, uint64_t* cap)
{
    GUARD(c)
    auto& m = c->sm;
    if (!m.active) return STARCH_ERR_STATE;
    if (!ptr || !cap) return STARCH_ERR_ARG;
    {
        std::lock_guard<std::mutex> lk(m.mu);
        if (m.err) throw StarchError(m.err, m.err_msg);
    }
    stream_reserve(c, m.cur, m.held_n + std::max<uint64_t>(min_bytes, 1));
    *ptr = m.buf[m.cur] + m.held_n;
    *cap = m.cap[m.cur] - m.held_n;
    return STARCH_OK;
    END_GUARD(c)
}

// commit n window bytes of which the first k precede any 0xFF (0xFF reads as
// EOF, hpp:181); ff_known: k was found while copying (starch_stream_feed)
static int stream_commit_k(starch_ctx* c, uint64_t n, uint64_t k, bool ff_known)
{
    GUARD(c)
    auto& m = c->sm;
    if (!m.active) return STARCH_ERR_STATE;
    if (m.held_n + n > m.cap[m.cur]) return STARCH_ERR_ARG;
    if (m.eof || n == 0) return STARCH_OK;
    if (!ff_known) k = shard::input_limit(m.buf[m.cur] + m.held_n, n);
    if (k < n) m.eof = true;
    if (k && !m.opt.reference_compat)
        HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t*>(m.dbuf[m.cur].p) + m.held_n, m.buf[m.cur] + m.held_n, k,
                                 hipMemcpyHostToDevice, c->cst));
    m.held_n += k;
    if (m.held_n >= m.try_at) stream_cut(c);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_stream_commit(starch_ctx* c, uint64_t n) { return stream_commit_k(c, n, 0, false); }

int starch_stream_feed(starch_ctx* c, const void* bed, uint64_t n)
{
    if (!c) return STARCH_ERR_ARG;
    if (n && !bed) return STARCH_ERR_ARG;
    if (c->sm.eof || n == 0) return c->sm.active ? STARCH_OK : STARCH_ERR_STATE;
    void* w = nullptr;
    uint64_t cap = 0;
    int rc = starch_stream_window(c, n, &w, &cap);
    if (rc) return rc;
    const double t0 = tracing() ? trace_t0() : 0.0;
    const uint64_t k = c->sm.pool.copy_find_ff(static_cast<uint8_t*>(w), static_cast<const uint8_t*>(bed), n);
    const double t1 = tracing() ? trace_t0() : 0.0;
    rc = stream_commit_k(c, n, k, true);
    if (tracing()) {
        c->sm.t_copy += t1 - t0;
        c->sm.t_commit += trace_t0() - t1;
        c->sm.fed += n;
    }
    return rc;
}

int starch_stream_end(starch_ctx* c)
{
    GUARD(c)
    auto& m = c->sm;
    if (!m.active) return STARCH_ERR_STATE;
    try {
        stream_prepin_join(c);
        // the rest goes to a lane as soon as one is free (the other may still
        // be encoding); an open stream's last piece waits for its predecessor
        if (m.held_n > m.ctx_len || m.last_open) stream_submit(c, m.held_n);
        stream_wait(c);
    } catch (...) {
        c->stream_shutdown();
        throw;
    }
    c->stream_shutdown();
    STRACE("stream end: fed %.1f MB, copy %.1f ms (%.1f GB/s), commit+cut %.1f ms", m.fed / 1e6, m.t_copy,
           m.t_copy > 0 ? m.fed / m.t_copy / 1e6 : 0.0, m.t_commit);
    m.t_copy = m.t_commit = 0;
    m.fed = 0;
    m.held_n = 0;
    m.ctx_len = 0;
    uint64_t bytes = m.opt.reference_compat ? 4 : m.stream_end;
    if (m.opt.emit_index && !m.opt.reference_compat) {
        const std::string idx = index_of(m.segs, m.names, m.stream_end, m.opt);
        m.ready.insert(m.ready.end(), idx.begin(), idx.end());
        bytes += idx.size();
    }
    m.stats.n_segments = m.segs.size();
    install_archive(c, m.segs, m.names, m.stats, bytes);   // (the session's lists go to the context)
    c->streamed = true;                                     // the archive's bytes are read with starch_stream_read
    return STARCH_OK;
    END_GUARD(c)
}

int starch_stream_available(starch_ctx* c, uint64_t* n)
{
    if (!c || !n) return STARCH_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->sm.mu);
    *n = c->sm.ready.size() - c->sm.ready_off;
    return STARCH_OK;
}

int starch_stream_read(starch_ctx* c, void* dst, uint64_t cap, uint64_t* len)
{
    if (!c || !len || (cap && !dst)) return STARCH_ERR_ARG;
    auto& m = c->sm;
    std::lock_guard<std::mutex> lk(m.mu);
    const uint64_t k = std::min<uint64_t>(cap, m.ready.size() - m.ready_off);
    if (k) memcpy(dst, m.ready.data() + m.ready_off, k);
    m.ready_off += k;
    if (m.ready_off == m.ready.size()) {
        m.ready.clear();
        m.ready_off = 0;
    } else if (m.ready_off > (64ull << 20) && 2 * m.ready_off > m.ready.size()) {
        m.ready.erase(m.ready.begin(), m.ready.begin() + (std::ptrdiff_t)m.ready_off);
        m.ready_off = 0;
    }
    *len = k;
    return STARCH_OK;
}

}  // extern "C"
