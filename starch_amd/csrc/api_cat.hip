// starch_amd/csrc/api_cat.hip -- starchcat: merge archives (include/starch_amd.h).
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "api_int.hpp"

using namespace api;

namespace {

struct CatInput {
    const uint8_t* a = nullptr;
    uint64_t n = 0, index_off = 0;
    ArchiveInfo info;
    std::vector<IndexEntry> idx;
};

struct CatGroup {
    std::string name;
    std::vector<starch_cat_run> runs;
    bool merge = false;
    uint64_t lines = 0, text_bytes = 0;
};

starch_options cat_options(const starch_options* opt)
{
    const starch_options o = options_of(opt);
    if (o.block_size_100k < 1 || o.block_size_100k > 9)
        throw StarchError(STARCH_ERR_ARG, "cat: block_size_100k must be 1..9");
    if (o.emit_index != 1 || o.reference_compat != 0 || o.compression_method != STARCH_METHOD_BZIP2)
        throw StarchError(STARCH_ERR_ARG, "cat: wants emit_index 1, reference_compat 0 and the bzip2 method");
    return o;
}

// bytewise order of the names, a prefix before the longer name
bool name_less(const std::string& a, const std::string& b)
{
    const int c = memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
    return c < 0 || (c == 0 && a.size() < b.size());
}

// the one place that decides what is copied and what is merged
std::vector<CatGroup> cat_plan(const void* const* archives, const uint64_t* lens, uint64_t narch, const starch_options& o,
                               std::vector<CatInput>& in)
{
    if (!archives || !lens || narch == 0) throw StarchError(STARCH_ERR_ARG, "cat: no input archives");
    if (narch > 0xFFFFFFFFull) throw StarchError(STARCH_ERR_ARG, "cat: too many input archives");
    in.assign(narch, CatInput{});
    std::map<std::string, CatGroup, bool (*)(const std::string&, const std::string&)> by_name(name_less);
    for (uint64_t k = 0; k < narch; ++k) {
        CatInput& x = in[k];
        if (!archives[k]) throw StarchError(STARCH_ERR_ARG, "cat: input " + std::to_string(k) + " is NULL");
        x.a = static_cast<const uint8_t*>(archives[k]);
        x.n = lens[k];
        x.idx = read_index(x.a, x.n, &x.index_off, &x.info);
        if (x.info.format == "gzip")
            throw StarchError(STARCH_ERR_ARG, "cat: gzip archives are not decoded (compressionFormat \"gzip\")");
        if (x.info.format != "bzip2")
            throw StarchError(STARCH_ERR_ARG, "cat: input " + std::to_string(k) + " has no compressionFormat \"bzip2\"");
        check_bounds(x.idx, x.index_off);
        if (x.idx.size() > 0xFFFFFFFFull) throw StarchError(STARCH_ERR_ARG, "cat: too many streams in one input");
        for (size_t e = 0; e < x.idx.size(); ++e) {
            CatGroup& g = by_name[x.idx[e].chr];
            g.runs.push_back(starch_cat_run{(uint32_t)k, (uint32_t)e});
            g.lines += x.idx[e].line_count;
            g.text_bytes += x.idx[e].text_bytes;
        }
    }
    std::vector<CatGroup> groups;
    for (auto& kv : by_name) {
        CatGroup& g = kv.second;
        g.name = kv.first;
        const starch_cat_run r = g.runs[0];
        g.merge = !(g.runs.size() == 1 && in[r.input].info.block_size_100k == o.block_size_100k &&
                    (!o.base_counts || in[r.input].idx[r.entry].has_base_counts));
        groups.push_back(std::move(g));
    }
    return groups;
}

struct CatPiece {            // a group's stream in the output
    starch_segment seg{};
    const uint8_t* bytes = nullptr;
};

// decode, merge and encode the merge groups gs (one batch); their streams go to `hold`
void cat_batch(starch_ctx* c, const std::vector<CatInput>& in, const std::vector<CatGroup>& groups,
               const std::vector<size_t>& gs, const starch_options& o, std::vector<CatPiece>& piece,
               std::vector<std::unique_ptr<uint8_t[]>>& hold, starch_cat_stats& cs)
{
    struct Copy { const uint8_t* src; uint64_t dst, len; };
    std::vector<Copy> copies;
    std::vector<std::pair<size_t, starch_cat_run>> runs;   // (position in gs, run), in segment order
    uint64_t m = 0, lines = 0;
    for (size_t b = 0; b < gs.size(); ++b)
        for (const starch_cat_run& r : groups[gs[b]].runs) {
            const IndexEntry& en = in[r.input].idx[r.entry];
            const uint8_t* src = in[r.input].a + en.offset;
            if (!copies.empty() && copies.back().src + copies.back().len == src) copies.back().len += en.size;
            else copies.push_back(Copy{src, m, en.size});
            m += en.size;
            lines += en.line_count;
            runs.emplace_back(b, r);
        }
    if (lines >= 0xFFFFFFFFull) throw StarchError(STARCH_ERR_MEM, "2^32 lines or more in one batch");
    uint8_t* d = c->dec_in.as<uint8_t>(m + 256);
    for (const Copy& x : copies)
        if (x.len) HIP_CHECK(hipMemcpyAsync(d + x.dst, x.src, x.len, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemsetAsync(d + m, 0, 256, c->st));
    // the decoder's host view of the same bytes: the input itself for one copy, else a packed one
    std::vector<uint8_t> staging;
    const uint8_t* h_in = copies[0].src;
    if (copies.size() > 1) {
        staging.resize(m);
        for (const Copy& x : copies) memcpy(staging.data() + x.dst, x.src, x.len);
        h_in = staging.data();
    }
    const uint64_t tbytes = c->dec.decode(d, m, h_in, c->st, c->dec_out, c->dstreams);
    if (c->dstreams.size() != runs.size()) throw StarchError(STARCH_ERR_DATA, "archive: index and streams disagree");
    std::vector<ut::Untransform::Seg> segs;
    ut::Untransform::Merge mg;
    uint64_t pos = 0;
    for (size_t i = 0; i < runs.size(); ++i) {
        const starch_cat_run r = runs[i].second;
        const IndexEntry& en = in[r.input].idx[r.entry];
        const bz::DecStream& s = c->dstreams[i];
        if (s.in_beg != pos || s.in_end - s.in_beg != en.size)
            throw StarchError(STARCH_ERR_DATA, "archive: stream " + std::to_string(r.entry) + " of input " +
                                                   std::to_string(r.input) + " is not where the index says");
        pos += en.size;
        segs.push_back(ut::Untransform::Seg{s.out_off, s.out_len, en.chr});
        mg.group.push_back((uint32_t)runs[i].first);
    }
    const uint64_t bed = c->untf.run(c->tf, static_cast<const uint8_t*>(c->dec_out.p), tbytes, segs, c->st, c->ut_out,
                                     nullptr, &mg);
    if (mg.bad_seg != ut::Untransform::Merge::kNone) {
        const starch_cat_run r = runs[mg.bad_seg].second;
        std::string nm;
        json_str(nm, segs[mg.bad_seg].name.data(), segs[mg.bad_seg].name.size());
        throw StarchError(STARCH_ERR_DATA, "cat: input " + std::to_string(r.input) + ", chromosome " + nm + ": line " +
                                               std::to_string((uint64_t)mg.bad_line + 1) +
                                               " of its stream sorts before the line above it (inputs must be sorted)");
    }
    // the merged BED in ut_out is the encoder's input: the encode path reads it
    // (transform, base counts, names) and writes tf's buffers, its own and
    // c->part -- none of dec_out / ut_out, which nothing else touches meanwhile
    std::vector<UnitIn> u(1, UnitIn{0, bed, 0, 0, 0});
    encode_units(c, static_cast<const uint8_t*>(c->ut_out.p), u, o, L_STREAMS, false, true);
    c->have = false;   // a batch's streams are no result of the context
    if (c->segs.size() != gs.size()) throw StarchError(STARCH_ERR_INTERNAL, "cat: the merged BED did not give one stream per group");
    for (size_t b = 0; b < gs.size(); ++b)
        if (c->names[b] != groups[gs[b]].name)
            throw StarchError(STARCH_ERR_INTERNAL, "cat: the merged BED's chromosomes are not the groups'");
    hold.emplace_back(new uint8_t[c->part_bytes + 1]);
    uint8_t* h = hold.back().get();
    if (c->part_bytes) HIP_CHECK(hipMemcpyAsync(h, c->part.p, c->part_bytes, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    for (size_t b = 0; b < gs.size(); ++b) {
        const starch_segment& sg = c->segs[b];
        if (sg.stream_offset + sg.stream_bytes > c->part_bytes) throw StarchError(STARCH_ERR_INTERNAL, "cat: stream outside the batch");
        piece[gs[b]].seg = sg;
        piece[gs[b]].bytes = h + sg.stream_offset;
    }
    cs.groups_merged += gs.size();
    cs.runs_decoded += runs.size();
    cs.lines_merged += mg.lines_out;
    cs.bytes_decoded += m;
}

void cat_run(starch_ctx* c, const void* const* archives, const uint64_t* lens, uint64_t narch, const starch_options* opt,
             void** out, uint64_t* out_len)
{
    const starch_options o = cat_options(opt);
    std::vector<CatInput> in;
    const std::vector<CatGroup> groups = cat_plan(archives, lens, narch, o, in);
    std::vector<CatPiece> piece(groups.size());
    std::vector<std::unique_ptr<uint8_t[]>> hold;
    starch_cat_stats cs{};
    for (const CatInput& x : in) cs.streams_in += x.idx.size();
    std::vector<size_t> todo;
    for (size_t g = 0; g < groups.size(); ++g) {
        if (groups[g].merge) { todo.push_back(g); continue; }
        const starch_cat_run r = groups[g].runs[0];
        const IndexEntry& en = in[r.input].idx[r.entry];
        starch_segment& sg = piece[g].seg;
        sg.line_count = en.line_count;
        sg.text_bytes = en.text_bytes;
        sg.stream_bytes = en.size;
        sg.n_blocks = en.n_blocks;
        sg.combined_crc = en.combined_crc;
        sg.base_count_unique = en.base_unique;
        sg.base_count_nonunique = en.base_nonunique;
        piece[g].bytes = in[r.input].a + en.offset;
        ++cs.streams_copied;
        cs.bytes_copied += en.size;
    }
    if (!todo.empty()) {
        if (!c) throw StarchError(STARCH_ERR_ARG, "cat: a chromosome has to be merged or re-encoded: needs a context");
        Ctx guard(c);
        c->have_out = false;
        c->have = false;
        uint64_t budget = 1ull << 30;
        if (const char* e = getenv("STARCH_CAT_BATCH_BYTES"))
            if (*e) budget = strtoull(e, nullptr, 10);
        for (size_t k = 0; k < todo.size();) {
            std::vector<size_t> gs(1, todo[k]);
            uint64_t sum = groups[todo[k]].text_bytes;
            for (++k; k < todo.size() && sum + groups[todo[k]].text_bytes <= budget; ++k) {
                sum += groups[todo[k]].text_bytes;
                gs.push_back(todo[k]);
            }
            Caught e;
            e.run([&] { cat_batch(c, in, groups, gs, o, piece, hold, cs); });
            if (e.code) {
                c->have = false;
                const bool oom = e.code == STARCH_ERR_MEM ||
                                 (e.code == STARCH_ERR_DEVICE && strstr(e.msg.c_str(), "out of memory") != nullptr);
                if (!oom) e.rethrow();
                (void)hipGetLastError();
                std::string nm;
                json_str(nm, groups[gs[0]].name.data(), groups[gs[0]].name.size());
                throw StarchError(STARCH_ERR_MEM, "cat: the batch starting at chromosome " + nm + " does not fit (" +
                                                      e.msg + "); lower STARCH_CAT_BATCH_BYTES");
            }
        }
    }
    // layout: magic, streams in group order, index, footer
    const size_t ng = groups.size();
    std::vector<starch_segment> segs(ng);
    std::vector<const char*> np(ng);
    std::vector<uint64_t> nlen(ng);
    uint64_t pos = 4;
    for (size_t g = 0; g < ng; ++g) {
        segs[g] = piece[g].seg;
        segs[g].stream_offset = pos;
        segs[g].name_len = groups[g].name.size();
        segs[g].unit = 0;
        np[g] = groups[g].name.data();
        nlen[g] = groups[g].name.size();
        pos += segs[g].stream_bytes;
    }
    const std::string idx = build_index(segs.data(), np.data(), nlen.data(), ng, pos, o.note, o.block_size_100k,
                                        o.base_counts != 0, o.compression_method);
    const uint64_t total = pos + idx.size();
    uint8_t* res = static_cast<uint8_t*>(malloc(total));
    if (!res) throw StarchError(STARCH_ERR_MEM, "cat: no host memory for the archive");
    memcpy(res, kMagic, 4);
    for (size_t g = 0; g < ng; ++g)
        if (segs[g].stream_bytes) memcpy(res + segs[g].stream_offset, piece[g].bytes, segs[g].stream_bytes);
    memcpy(res + pos, idx.data(), idx.size());
    *out = res;
    *out_len = total;
    if (c) {
        c->cstats = cs;
        c->have_cstats = true;
    }
}

}  // namespace

extern "C" {

int starch_cat_plan(const void* const* archives, const uint64_t* lens, uint64_t narch, const starch_options* opt,
                    starch_cat_group* groups, uint64_t gcap, uint64_t* ngroups, starch_cat_run* runs, uint64_t rcap,
                    uint64_t* nruns, char* names, uint64_t names_cap, uint64_t* names_len)
{
    if (!ngroups) return STARCH_ERR_ARG;
    try {
        const starch_options o = cat_options(opt);
        std::vector<CatInput> in;
        const std::vector<CatGroup> gr = cat_plan(archives, lens, narch, o, in);
        uint64_t nr = 0, nb = 0;
        for (const CatGroup& g : gr) { nr += g.runs.size(); nb += g.name.size(); }
        *ngroups = gr.size();
        if (nruns) *nruns = nr;
        if (names_len) *names_len = nb;
        if (!groups && !runs && !names) return STARCH_OK;   // sizing call
        if ((groups && gcap < gr.size()) || (runs && rcap < nr) || (names && names_cap < nb)) return STARCH_ERR_MEM;
        uint64_t ro = 0, no = 0;
        for (size_t k = 0; k < gr.size(); ++k) {
            const CatGroup& g = gr[k];
            if (groups)
                groups[k] = starch_cat_group{no, g.name.size(), ro, (uint32_t)g.runs.size(), g.merge ? 1u : 0u, g.lines,
                                             g.text_bytes};
            if (runs) memcpy(runs + ro, g.runs.data(), g.runs.size() * sizeof(starch_cat_run));
            if (names && !g.name.empty()) memcpy(names + no, g.name.data(), g.name.size());
            ro += g.runs.size();
            no += g.name.size();
        }
        return STARCH_OK;
    } catch (const StarchError& e) {
        return e.code;
    } catch (const std::exception&) {
        return STARCH_ERR_INTERNAL;
    }
}

int starch_cat_host(starch_ctx* c, const void* const* archives, const uint64_t* lens, uint64_t narch,
                    const starch_options* opt, void** out, uint64_t* out_len)
{
    if (!out || !out_len) return STARCH_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    try {
        cat_run(c, archives, lens, narch, opt, out, out_len);
        return STARCH_OK;
    } catch (const StarchError& e) {
        if (c) c->err = e.what();
        return e.code;
    } catch (const std::exception& e) {
        if (c) c->err = e.what();
        return STARCH_ERR_INTERNAL;
    }
}

int starch_cat_get_stats(starch_ctx* c, starch_cat_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_cstats) return STARCH_ERR_STATE;
    *out = c->cstats;
    return STARCH_OK;
}

}  // extern "C"
