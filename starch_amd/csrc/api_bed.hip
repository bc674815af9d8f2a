// starch_amd/csrc/api_bed.hip -- the C ABI of sort-bed, bedops, bedmap, closest-features, bedmap-elements,
// bedmap-scores, convert2bed, sam2bed, psl2bed, rmsk2bed, bam2bed, bigwig2bed and bigbed2bed (with starch_bbi_info).  The four two-input tools go through pair_host,
// pair_device and pair_get_stats, the converters through text_call; a tool keeps its option check, its
// constants and the stats fields that are its own.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "api_int.hpp"
#include "bed_bbi.hpp"
#include "gz_adler.hpp"

using namespace api;

namespace {
// input k of a device call is d_bed[offs[k], offs[k + 1])
bool offs_ok(const void* d_bed, const uint64_t* offs, uint64_t ninputs)
{
    for (uint64_t k = 0; k < ninputs; ++k)
        if (offs[k + 1] < offs[k]) return false;
    return offs[ninputs] <= offs[0] || d_bed;
}
}  // namespace

// ---- sort-bed (include/starch_amd.h; kernels in sort_bed.hip) -----------------
namespace {
void sort_run(starch_ctx* c, const uint8_t* d, uint64_t n, bool check_only)
{
    c->have_sstats = false;
    if (!check_only) c->have_out = false;
    sb::SortResult r;
    c->sorter.run(d, n, c->st, check_only, c->sort_out, r);
    starch_sort_stats& s = c->sstats;
    s = starch_sort_stats{};
    s.input_bytes = n;
    s.n_lines = r.n_lines;
    s.n_chromosomes = r.n_chromosomes;
    s.already_sorted = r.already_sorted ? 1 : 0;
    s.first_unsorted_line = r.first_unsorted_line;
    s.radix_passes = r.radix_passes;
    s.ms_parse = r.ms_parse;
    s.ms_rank = r.ms_rank;
    s.ms_sort = r.ms_sort;
    s.ms_gather = r.ms_gather;
    s.ms_total = r.ms_total;
    c->have_sstats = true;
    if (check_only) return;
    publish(c, c->sort_out, r.out_bytes);
}
// bed[0, n) into c->input; a gzip input is inflated there, and n becomes its inflated size
const uint8_t* sort_upload(starch_ctx* c, const void* bed, uint64_t& n)
{
    if (gz::is_gzip(bed, n)) {
        n = gunzip_plan(c, static_cast<const uint8_t*>(bed), n);
        uint8_t* t = c->input.as<uint8_t>(n + 64);
        gunzip_into(c, t);
        return t;
    }
    uint8_t* d = c->input.as<uint8_t>(n + 64);
    HostRegistration reg(bed, n, 256ull << 20);
    reg.h2d(d, bed, n, c->st);
    HIP_CHECK(hipStreamSynchronize(c->st));
    return d;
}
}  // namespace

extern "C" {

int starch_sort_device(starch_ctx* c, const void* d_bed, uint64_t n)
{
    GUARD(c)
    if (n && !d_bed) return STARCH_ERR_ARG;
    sort_run(c, static_cast<const uint8_t*>(d_bed), n, false);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_sort_host(starch_ctx* c, const void* bed, uint64_t n)
{
    GUARD(c)
    if (n && !bed) return STARCH_ERR_ARG;
    const uint8_t* d = sort_upload(c, bed, n);
    sort_run(c, d, n, false);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_sort_check_host(starch_ctx* c, const void* bed, uint64_t n, uint64_t* first_unsorted_line)
{
    GUARD(c)
    if ((n && !bed) || !first_unsorted_line) return STARCH_ERR_ARG;
    const uint8_t* d = sort_upload(c, bed, n);
    sort_run(c, d, n, true);
    *first_unsorted_line = c->sstats.first_unsorted_line;
    return STARCH_OK;
    END_GUARD(c)
}

int starch_sort_encode_host(starch_ctx* c, const void* bed, uint64_t n, const starch_options* opt)
{
    GUARD(c)
    if (n && !bed) return STARCH_ERR_ARG;
    const starch_options o = options_of(opt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    c->have = false;
    const uint8_t* d = sort_upload(c, bed, n);
    sort_run(c, d, n, false);
    // the sorted text is in sort_out, which no encoder stage writes
    encode_device(c, c->out_dev, c->out_bytes, o);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_sort_get_stats(starch_ctx* c, starch_sort_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_sstats) return STARCH_ERR_STATE;
    *out = c->sstats;
    return STARCH_OK;
}

int starch_sort_constants(uint32_t* tile_lines, uint32_t* wave_copy_bytes)
{
    if (tile_lines) *tile_lines = (uint32_t)sb::kSortTile;
    if (wave_copy_bytes) *wave_copy_bytes = sb::kWaveCopyBytes;
    return STARCH_OK;
}

}  // extern "C"

// ---- bedops set operations (include/starch_amd.h; kernels in bed_setops.hip) ----
namespace {
// c->setop_in with room for `want` bytes, its first `used` bytes kept
uint8_t* setop_reserve(starch_ctx* c, uint64_t used, uint64_t want)
{
    DevBuf& b = c->setop_in;
    if (b.p && want <= b.cap) return static_cast<uint8_t*>(b.p);
    DevBuf nb;
    (void)nb.get(std::max<uint64_t>(want, 2 * (uint64_t)b.cap));
    if (used) {
        HIP_CHECK(hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
    }
    std::swap(b.p, nb.p);
    std::swap(b.cap, nb.cap);
    return static_cast<uint8_t*>(b.p);
}

void setop_run(starch_ctx* c, const so::BedopsOptions& opt, uint64_t len, const std::vector<uint64_t>& in_end, uint64_t archives,
               double ms_decode, const std::chrono::steady_clock::time_point& t0)
{
    so::SetopResult r;
    c->setop.run_bedops(c->sorter, opt, static_cast<const uint8_t*>(c->setop_in.p), len, in_end, c->st, c->setop_out, r);
    starch_setop_stats& s = c->ostats;
    s = starch_setop_stats{};
    s.n_inputs = in_end.size();
    s.input_bytes = len;
    s.n_lines = r.n_lines;
    s.n_chromosomes = r.n_chromosomes;
    s.runs_merged = r.runs_merged;
    s.groups = r.groups;
    s.lines_out = r.lines_out;
    s.output_bytes = r.out_bytes;
    s.archives_decoded = archives;
    s.radix_passes = r.radix_passes;
    s.ms_decode = (float)ms_decode;
    s.ms_parse = r.ms_parse;
    s.ms_merge = r.ms_merge;
    s.ms_sort = r.ms_sort;
    s.ms_sweep = r.ms_sweep;
    s.ms_format = r.ms_format;
    s.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->have_ostats = true;
    publish(c, c->setop_out, r.out_bytes);
}

// The inputs (BED text, archives or gzip / BGZF files of BED text, in host memory) back
// to back in c->setop_in, each non-empty one ending in '\n'.  Returns the bytes; in_end: where each ends.
uint64_t setop_load_host(starch_ctx* c, const starch_setop_input* inputs, uint64_t ninputs, const char* tool,
                         std::vector<uint64_t>& in_end, uint64_t* archives_out)
{
    uint64_t want = 64;
    for (uint64_t k = 0; k < ninputs; ++k) want += inputs[k].len + 1;
    uint8_t* d = setop_reserve(c, 0, want);
    uint64_t len = 0, archives = 0;
    for (uint64_t k = 0; k < ninputs; ++k) {
        const uint8_t* a = static_cast<const uint8_t*>(inputs[k].data);
        const uint64_t n = inputs[k].len;
        uint64_t m = n;
        uint8_t last = '\n';
        if (n >= 4 && memcmp(a, archive::kMagic, 4) == 0) {
            ++archives;
            m = unstarch_to_ut_out(c, a, n, tool);
            want += m;
            d = setop_reserve(c, len, want);
            if (m) {
                HIP_CHECK(hipMemcpyAsync(d + len, c->ut_out.p, m, hipMemcpyDeviceToDevice, c->st));
                HIP_CHECK(hipMemcpyAsync(&last, static_cast<const uint8_t*>(c->ut_out.p) + (m - 1), 1, hipMemcpyDeviceToHost,
                                         c->st));
                HIP_CHECK(hipStreamSynchronize(c->st));
            }
        } else if (gz::is_gzip(a, n)) {
            m = gunzip_plan(c, a, n);
            want += m;
            d = setop_reserve(c, len, want);
            gunzip_into(c, d + len);
            if (m) {
                HIP_CHECK(hipMemcpyAsync(&last, d + len + (m - 1), 1, hipMemcpyDeviceToHost, c->st));
                HIP_CHECK(hipStreamSynchronize(c->st));
            }
        } else if (n) {
            HIP_CHECK(hipMemcpyAsync(d + len, a, n, hipMemcpyHostToDevice, c->st));
            last = a[n - 1];
        }
        len += m;
        if (m && last != '\n') {
            HIP_CHECK(hipMemsetAsync(d + len, '\n', 1, c->st));
            ++len;
        }
        in_end.push_back(len);
    }
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (archives_out) *archives_out = archives;
    return len;
}

// The same for BED text in HBM: input k is d_bed[offs[k], offs[k + 1]).
uint64_t setop_load_device(starch_ctx* c, const void* d_bed, const uint64_t* offs, uint64_t ninputs,
                           std::vector<uint64_t>& in_end)
{
    const uint8_t* src = static_cast<const uint8_t*>(d_bed);
    uint8_t* d = setop_reserve(c, 0, offs[ninputs] - offs[0] + ninputs + 64);
    std::vector<uint8_t> last(ninputs, (uint8_t)'\n');
    for (uint64_t k = 0; k < ninputs; ++k)
        if (offs[k + 1] > offs[k])
            HIP_CHECK(hipMemcpyAsync(&last[k], src + offs[k + 1] - 1, 1, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    uint64_t len = 0;
    for (uint64_t k = 0; k < ninputs; ++k) {
        const uint64_t m = offs[k + 1] - offs[k];
        if (m) HIP_CHECK(hipMemcpyAsync(d + len, src + offs[k], m, hipMemcpyDeviceToDevice, c->st));
        len += m;
        if (m && last[k] != '\n') {
            HIP_CHECK(hipMemsetAsync(d + len, '\n', 1, c->st));
            ++len;
        }
        in_end.push_back(len);
    }
    return len;
}

bool setop_args_ok(int op, const void* inputs, uint64_t ninputs)
{
    return op >= STARCH_SETOP_MERGE && op <= STARCH_SETOP_COMPLEMENT && inputs && ninputs;
}

// starch_bedops_options checked into out; nothing here touches a device
bool bedops_options_ok(const starch_bedops_options* o, uint64_t ninputs, so::BedopsOptions* out)
{
    if (!o || o->op < STARCH_SETOP_MERGE || o->op > STARCH_SETOP_EVERYTHING || !ninputs) return false;
    *out = so::BedopsOptions{};
    out->op = o->op;
    if (o->op == STARCH_SETOP_ELEMENT_OF || o->op == STARCH_SETOP_NOT_ELEMENT_OF) {
        if (ninputs < 2 || o->threshold == 0 || (o->threshold_is_percent && o->threshold > 100)) return false;
        out->threshold = o->threshold;
        out->percent = o->threshold_is_percent != 0;
    }
    if (o->op == STARCH_SETOP_CHOP) {
        if (o->chop == 0) return false;
        out->chop = o->chop;
        out->stagger = o->stagger ? o->stagger : o->chop;
        out->exclude_short = o->exclude_short != 0;
    }
    return true;
}

so::BedopsOptions plain_op(int op)
{
    so::BedopsOptions o;
    o.op = op;
    return o;
}

int bedops_host(starch_ctx* c, const so::BedopsOptions& opt, const starch_setop_input* inputs, uint64_t ninputs)
{
    for (uint64_t k = 0; k < ninputs; ++k)
        if (inputs[k].len && !inputs[k].data) return STARCH_ERR_ARG;
    GUARD(c)
    c->have_out = false;
    c->have_ostats = false;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> in_end;
    uint64_t archives = 0;
    const uint64_t len = setop_load_host(c, inputs, ninputs, "bedops", in_end, &archives);
    const double ms_decode = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    setop_run(c, opt, len, in_end, archives, ms_decode, t0);
    return STARCH_OK;
    END_GUARD(c)
}

int bedops_device(starch_ctx* c, const so::BedopsOptions& opt, const void* d_bed, const uint64_t* offs, uint64_t ninputs)
{
    if (!offs_ok(d_bed, offs, ninputs)) return STARCH_ERR_ARG;
    GUARD(c)
    c->have_out = false;
    c->have_ostats = false;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> in_end;
    const uint64_t len = setop_load_device(c, d_bed, offs, ninputs, in_end);
    setop_run(c, opt, len, in_end, 0, 0.0, t0);
    return STARCH_OK;
    END_GUARD(c)
}
}  // namespace

extern "C" {

int starch_bedops_host(starch_ctx* c, const starch_bedops_options* o, const starch_setop_input* inputs, uint64_t ninputs)
{
    so::BedopsOptions opt;
    if (!c || !inputs || !bedops_options_ok(o, ninputs, &opt)) return STARCH_ERR_ARG;
    return bedops_host(c, opt, inputs, ninputs);
}

int starch_bedops_device(starch_ctx* c, const starch_bedops_options* o, const void* d_bed, const uint64_t* offs,
                         uint64_t ninputs)
{
    so::BedopsOptions opt;
    if (!c || !offs || !bedops_options_ok(o, ninputs, &opt)) return STARCH_ERR_ARG;
    return bedops_device(c, opt, d_bed, offs, ninputs);
}

int starch_bedops_constants(uint32_t* rmq_tile, uint32_t* expand_tile)
{
    if (rmq_tile) *rmq_tile = so::kRmqTile;
    if (expand_tile) *expand_tile = (uint32_t)so::kExpandTile;
    return STARCH_OK;
}

int starch_setop_host(starch_ctx* c, int op, const starch_setop_input* inputs, uint64_t ninputs)
{
    if (!c || !setop_args_ok(op, inputs, ninputs)) return STARCH_ERR_ARG;
    return bedops_host(c, plain_op(op), inputs, ninputs);
}

int starch_setop_device(starch_ctx* c, int op, const void* d_bed, const uint64_t* offs, uint64_t ninputs)
{
    if (!c || !setop_args_ok(op, offs, ninputs)) return STARCH_ERR_ARG;
    return bedops_device(c, plain_op(op), d_bed, offs, ninputs);
}

int starch_setop_get_stats(starch_ctx* c, starch_setop_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_ostats) return STARCH_ERR_STATE;
    *out = c->ostats;
    return STARCH_OK;
}

int starch_setop_constants(uint32_t* scan_tile_lines)
{
    if (scan_tile_lines) *scan_tile_lines = (uint32_t)so::kScanTile;
    return STARCH_OK;
}

}  // extern "C"

// ---- what bedmap, closest-features, bedmap-elements and bedmap-scores share ----------
// A tool T names its types (Options, Result, Stats), its slot in the context
// (stats, have), its name in messages, how it runs, and own(): the fields of
// its stats that no other tool has.
namespace {
template <class T>
void pair_run(starch_ctx* c, const typename T::Options& opt, uint64_t len, const std::vector<uint64_t>& in_end, double ms_decode,
              const std::chrono::steady_clock::time_point& t0)
{
    typename T::Result r;
    T::run(c, opt, static_cast<const uint8_t*>(c->setop_in.p), len, in_end, r);
    typename T::Stats& s = T::stats(c);
    s = typename T::Stats{};
    s.n_ref = r.n_ref;
    s.n_chromosomes = r.n_chromosomes;
    s.lines_out = r.lines_out;
    s.output_bytes = r.out_bytes;
    s.ms_decode = (float)ms_decode;
    s.ms_parse = r.ms_parse;
    s.ms_build = r.ms_build;
    s.ms_query = r.ms_query;
    s.ms_format = r.ms_format;
    T::own(s, r);
    s.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    T::have(c) = true;
    publish(c, c->setop_out, r.out_bytes);
}

// the reference and, unless it is NULL, the second input, in host memory; the arguments are checked
template <class T>
int pair_host(starch_ctx* c, const typename T::Options& opt, const starch_setop_input* ref, const starch_setop_input* second)
{
    GUARD(c)
    c->have_out = false;
    T::have(c) = false;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<starch_setop_input> inputs{*ref};
    if (second) inputs.push_back(*second);
    std::vector<uint64_t> in_end;
    const uint64_t len = setop_load_host(c, inputs.data(), inputs.size(), T::name(), in_end, nullptr);
    const double ms_decode = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    pair_run<T>(c, opt, len, in_end, ms_decode, t0);
    return STARCH_OK;
    END_GUARD(c)
}

template <class T>
int pair_device(starch_ctx* c, const typename T::Options& opt, const void* d_bed, const uint64_t* offs, uint64_t ninputs)
{
    if (!offs_ok(d_bed, offs, ninputs)) return STARCH_ERR_ARG;
    GUARD(c)
    c->have_out = false;
    T::have(c) = false;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> in_end;
    const uint64_t len = setop_load_device(c, d_bed, offs, ninputs, in_end);
    pair_run<T>(c, opt, len, in_end, 0.0, t0);
    return STARCH_OK;
    END_GUARD(c)
}

template <class T>
int pair_get_stats(starch_ctx* c, typename T::Stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!T::have(c)) return STARCH_ERR_STATE;
    *out = T::stats(c);
    return STARCH_OK;
}

bool input_ok(const starch_setop_input* in) { return !in || !in->len || in->data; }
}  // namespace

// ---- bedmap (include/starch_amd.h; kernels in bed_map.hip) -------------------------
namespace {
bool map_options_ok(const starch_map_options* o, bm::MapOptions* out)
{
    if (!o || o->ncols < 1 || o->ncols > 8 || o->delim_len < 1 || o->delim_len > 8) return false;
    uint32_t seen = 0;
    for (uint32_t k = 0; k < o->ncols; ++k) {
        if (o->cols[k] > STARCH_MAP_ECHO_REF_SIZE || ((seen >> o->cols[k]) & 1)) return false;
        seen |= 1u << o->cols[k];
        out->cols[k] = o->cols[k];
    }
    out->ncols = o->ncols;
    out->range = o->range;
    out->skip_unmapped = o->skip_unmapped ? 1 : 0;
    out->delim_len = o->delim_len;
    memcpy(out->delim, o->delim, o->delim_len);
    return true;
}

struct MapTool {
    typedef bm::MapOptions Options;
    typedef bm::MapResult Result;
    typedef starch_map_stats Stats;
    static const char* name() { return "bedmap"; }
    static Stats& stats(starch_ctx* c) { return c->mstats; }
    static bool& have(starch_ctx* c) { return c->have_mstats; }
    static void run(starch_ctx* c, const Options& o, const uint8_t* d, uint64_t len, const std::vector<uint64_t>& in_end, Result& r)
    {
        c->mapper.run(c->sorter, c->setop, o, d, len, in_end, c->st, c->setop_out, r);
    }
    static void own(Stats& s, const Result& r)
    {
        s.n_map = r.n_map;
        s.map_runs_merged = r.map_runs_merged;
        s.stops_sorted = r.stops_sorted;
    }
};
}  // namespace

extern "C" {

int starch_map_host(starch_ctx* c, const starch_setop_input* ref, const starch_setop_input* map, const starch_map_options* opt)
{
    bm::MapOptions mo;
    if (!c || !ref || !map_options_ok(opt, &mo)) return STARCH_ERR_ARG;
    if (!input_ok(ref) || !input_ok(map)) return STARCH_ERR_ARG;
    return pair_host<MapTool>(c, mo, ref, map);
}

int starch_map_device(starch_ctx* c, const void* d_bed, const uint64_t* offs, uint64_t ninputs, const starch_map_options* opt)
{
    bm::MapOptions mo;
    if (!c || !offs || ninputs < 1 || ninputs > 2 || !map_options_ok(opt, &mo)) return STARCH_ERR_ARG;
    return pair_device<MapTool>(c, mo, d_bed, offs, ninputs);
}

int starch_map_get_stats(starch_ctx* c, starch_map_stats* out)
{
    return pair_get_stats<MapTool>(c, out);
}

int starch_map_constants(uint32_t* tile_refs, uint32_t* lds_window)
{
    if (tile_refs) *tile_refs = (uint32_t)bm::kTileRefs;
    if (lds_window) *lds_window = bm::kLdsWindow;
    return STARCH_OK;
}

}  // extern "C"

// ---- closest-features (include/starch_amd.h; kernels in bed_closest.hip) -----------
namespace {
bool closest_options_ok(const starch_closest_options* o, bc::ClosestOptions* out)
{
    if (!o || o->delim_len < 1 || o->delim_len > 8) return false;
    if (o->closest > 1 || o->dist > 1 || o->no_overlaps > 1 || o->no_ref > 1) return false;
    out->closest = o->closest;
    out->dist = o->dist;
    out->no_overlaps = o->no_overlaps;
    out->no_ref = o->no_ref;
    out->delim_len = o->delim_len;
    memcpy(out->delim, o->delim, o->delim_len);
    return true;
}

struct ClosestTool {
    typedef bc::ClosestOptions Options;
    typedef bc::ClosestResult Result;
    typedef starch_closest_stats Stats;
    static const char* name() { return "closest-features"; }
    static Stats& stats(starch_ctx* c) { return c->kstats; }
    static bool& have(starch_ctx* c) { return c->have_kstats; }
    static void run(starch_ctx* c, const Options& o, const uint8_t* d, uint64_t len, const std::vector<uint64_t>& in_end, Result& r)
    {
        c->closer.run(c->sorter, c->setop, o, d, len, in_end, c->st, c->setop_out, r);
    }
    static void own(Stats& s, const Result& r)
    {
        s.n_query = r.n_query;
        s.stops_sorted = r.stops_sorted;
        s.left_na = r.left_na;
        s.right_na = r.right_na;
    }
};
}  // namespace

extern "C" {

int starch_closest_host(starch_ctx* c, const starch_setop_input* ref, const starch_setop_input* query,
                        const starch_closest_options* opt)
{
    bc::ClosestOptions co;
    if (!c || !ref || !query || !closest_options_ok(opt, &co)) return STARCH_ERR_ARG;
    if (!input_ok(ref) || !input_ok(query)) return STARCH_ERR_ARG;
    return pair_host<ClosestTool>(c, co, ref, query);
}

int starch_closest_device(starch_ctx* c, const void* d_bed, const uint64_t* offs, const starch_closest_options* opt)
{
    bc::ClosestOptions co;
    if (!c || !offs || !closest_options_ok(opt, &co)) return STARCH_ERR_ARG;
    return pair_device<ClosestTool>(c, co, d_bed, offs, 2);
}

int starch_closest_get_stats(starch_ctx* c, starch_closest_stats* out)
{
    return pair_get_stats<ClosestTool>(c, out);
}

int starch_closest_constants(uint32_t* tile_refs, uint32_t* fanout)
{
    if (tile_refs) *tile_refs = (uint32_t)bc::kTileRefs;
    if (fanout) *fanout = bc::kFanout;
    return STARCH_OK;
}

}  // extern "C"

// ---- bedmap-elements (include/starch_amd.h; kernels in bed_mapel.hip) ---------------
namespace {
// exactly one criterion: the fields of the others are 0 (shared with bedmap-scores)
bool mapel_criterion_ok(uint32_t c, uint64_t n, uint64_t range, uint64_t frac_num, uint32_t frac_digits, me::MapelOptions* out)
{
    if (c > STARCH_MAPEL_CRIT_EXACT) return false;
    const bool frac = c >= STARCH_MAPEL_CRIT_FRACTION_REF && c <= STARCH_MAPEL_CRIT_FRACTION_EITHER;
    if ((c == STARCH_MAPEL_CRIT_BP_OVR) != (n != 0)) return false;
    if (c != STARCH_MAPEL_CRIT_RANGE && range != 0) return false;
    if (!frac && (frac_num != 0 || frac_digits != 0)) return false;
    out->criterion = c;
    out->n = n;
    out->range = range;
    if (frac) {
        if (frac_digits > 9) return false;
        uint64_t den = 1;
        for (uint32_t k = 0; k < frac_digits; ++k) den *= 10;
        if (frac_num == 0 || frac_num > den) return false;
        out->frac_num = frac_num;
        out->frac_den = den;
    }
    return true;
}

bool mapel_options_ok(const starch_mapel_options* o, me::MapelOptions* out)
{
    if (!o || o->ncols < 1 || o->ncols > me::kMaxCols || o->delim_len < 1 || o->delim_len > 8 || o->multidelim_len < 1 ||
        o->multidelim_len > 8)
        return false;
    uint32_t seen = 0;
    for (uint32_t k = 0; k < o->ncols; ++k) {
        if (o->cols[k] > STARCH_MAPEL_ECHO_MAP_RANGE || ((seen >> o->cols[k]) & 1)) return false;
        seen |= 1u << o->cols[k];
        out->cols[k] = o->cols[k];
    }
    out->ncols = o->ncols;
    if (!mapel_criterion_ok(o->criterion, o->n, o->range, o->frac_num, o->frac_digits, out)) return false;
    out->skip_unmapped = o->skip_unmapped ? 1 : 0;
    out->delim_len = o->delim_len;
    memcpy(out->delim, o->delim, o->delim_len);
    out->multi_len = o->multidelim_len;
    memcpy(out->multi, o->multidelim, o->multidelim_len);
    return true;
}

struct MapelTool {
    typedef me::MapelOptions Options;
    typedef me::MapelResult Result;
    typedef starch_mapel_stats Stats;
    static const char* name() { return "bedmap-elements"; }
    static Stats& stats(starch_ctx* c) { return c->estats; }
    static bool& have(starch_ctx* c) { return c->have_estats; }
    static void run(starch_ctx* c, const Options& o, const uint8_t* d, uint64_t len, const std::vector<uint64_t>& in_end, Result& r)
    {
        c->mapel.run(c->sorter, c->setop, o, d, len, in_end, c->st, c->setop_out, r);
    }
    static void own(Stats& s, const Result& r)
    {
        s.n_map = r.n_map;
        s.hits = r.hits;
        s.heavy_lines = r.heavy_lines;
        s.walk_steps = r.walk_steps;
    }
};
}  // namespace

extern "C" {

int starch_mapel_host(starch_ctx* c, const starch_setop_input* ref, const starch_setop_input* map,
                      const starch_mapel_options* opt)
{
    me::MapelOptions mo;
    if (!c || !ref || !mapel_options_ok(opt, &mo)) return STARCH_ERR_ARG;
    if (!input_ok(ref) || !input_ok(map)) return STARCH_ERR_ARG;
    return pair_host<MapelTool>(c, mo, ref, map);
}

int starch_mapel_device(starch_ctx* c, const void* d_bed, const uint64_t* offs, uint64_t ninputs, const starch_mapel_options* opt)
{
    me::MapelOptions mo;
    if (!c || !offs || ninputs < 1 || ninputs > 2 || !mapel_options_ok(opt, &mo)) return STARCH_ERR_ARG;
    return pair_device<MapelTool>(c, mo, d_bed, offs, ninputs);
}

int starch_mapel_get_stats(starch_ctx* c, starch_mapel_stats* out)
{
    return pair_get_stats<MapelTool>(c, out);
}

int starch_mapel_constants(uint32_t* tile_refs, uint32_t* fanout, uint32_t* heavy_threshold, uint32_t* steps_per_hit_bound)
{
    if (tile_refs) *tile_refs = (uint32_t)me::kTileRefs;
    if (fanout) *fanout = bc::kFanout;
    if (heavy_threshold) *heavy_threshold = me::kHeavy;
    if (steps_per_hit_bound) *steps_per_hit_bound = me::kStepsPerHit;
    return STARCH_OK;
}

}  // extern "C"

// ---- bedmap-scores (include/starch_amd.h; kernels in bed_mapscore.hip) ---------------
namespace {
bool mapsc_options_ok(const starch_mapsc_options* o, ms::MapscOptions* out)
{
    if (!o || o->ncols < 1 || o->ncols > ms::kMaxCols || o->delim_len < 1 || o->delim_len > 8 || o->prec > 9) return false;
    uint32_t seen = 0;
    for (uint32_t k = 0; k < o->ncols; ++k) {
        if (o->cols[k] > STARCH_MAPSC_MAX_ELEMENT || ((seen >> o->cols[k]) & 1)) return false;
        seen |= 1u << o->cols[k];
        out->cols[k] = o->cols[k];
    }
    out->ncols = o->ncols;
    if (!mapel_criterion_ok(o->criterion, o->n, o->range, o->frac_num, o->frac_digits, &out->crit)) return false;
    if ((seen >> STARCH_MAPSC_KTH) & 1) {
        if (o->kth_digits > 9) return false;
        uint64_t den = 1;
        for (uint32_t k = 0; k < o->kth_digits; ++k) den *= 10;
        if (o->kth_num == 0 || o->kth_num > den) return false;
        out->kth_num = o->kth_num;
        out->kth_den = den;
    } else if (o->kth_num != 0 || o->kth_digits != 0) return false;
    out->prec = o->prec;
    out->skip_unmapped = o->skip_unmapped ? 1 : 0;
    out->delim_len = o->delim_len;
    memcpy(out->delim, o->delim, o->delim_len);
    return true;
}

struct MapscTool {
    typedef ms::MapscOptions Options;
    typedef ms::MapscResult Result;
    typedef starch_mapsc_stats Stats;
    static const char* name() { return "bedmap-scores"; }
    static Stats& stats(starch_ctx* c) { return c->scstats; }
    static bool& have(starch_ctx* c) { return c->have_scstats; }
    static void run(starch_ctx* c, const Options& o, const uint8_t* d, uint64_t len, const std::vector<uint64_t>& in_end, Result& r)
    {
        c->mapsc.run(c->sorter, c->setop, c->mapel, o, d, len, in_end, c->st, c->setop_out, r);
    }
    static void own(Stats& s, const Result& r)
    {
        s.n_map = r.n_map;
        s.hits = r.hits;
        s.straddling = r.straddling;
        s.sorted_hits = r.sorted_hits;
        s.radix_passes = r.radix_passes;
        s.ms_reduce = r.ms_reduce;
    }
};
}  // namespace

extern "C" {

int starch_mapsc_host(starch_ctx* c, const starch_setop_input* ref, const starch_setop_input* map,
                      const starch_mapsc_options* opt)
{
    ms::MapscOptions mo;
    if (!c || !ref || !mapsc_options_ok(opt, &mo)) return STARCH_ERR_ARG;
    if (!input_ok(ref) || !input_ok(map)) return STARCH_ERR_ARG;
    return pair_host<MapscTool>(c, mo, ref, map);
}

int starch_mapsc_device(starch_ctx* c, const void* d_bed, const uint64_t* offs, uint64_t ninputs, const starch_mapsc_options* opt)
{
    ms::MapscOptions mo;
    if (!c || !offs || ninputs < 1 || ninputs > 2 || !mapsc_options_ok(opt, &mo)) return STARCH_ERR_ARG;
    return pair_device<MapscTool>(c, mo, d_bed, offs, ninputs);
}

int starch_mapsc_get_stats(starch_ctx* c, starch_mapsc_stats* out)
{
    return pair_get_stats<MapscTool>(c, out);
}

int starch_mapsc_constants(uint32_t* tile_hits, uint32_t* wave_copy_threshold)
{
    if (tile_hits) *tile_hits = (uint32_t)ms::kTileHits;
    if (wave_copy_threshold) *wave_copy_threshold = sb::kWaveCopyBytes;
    return STARCH_OK;
}

}  // extern "C"

// ---- what convert2bed and sam2bed, psl2bed, rmsk2bed share ---------------------------
// A tool T is as above; run() converts d[0, n) into setop_out.
namespace {
// d[0, n) converted into setop_out and, unless no_sort, sorted from there into sort_out
template <class T>
void text_run(starch_ctx* c, const typename T::Options& opt, bool no_sort, const uint8_t* d, uint64_t n,
              const std::chrono::steady_clock::time_point& t0)
{
    typename T::Result r;
    T::run(c, opt, d, n, r);
    typename T::Stats& s = T::stats(c);
    s = typename T::Stats{};
    s.input_bytes = n;
    s.input_lines = r.n_lines;
    s.header_lines = r.header_lines;
    s.lines_out = r.lines_out;
    s.output_bytes = r.out_bytes;
    s.ms_frame = r.ms_frame;
    s.ms_parse = r.ms_parse;
    s.ms_write = r.ms_write;
    T::own(s, r);
    if (no_sort) publish(c, c->setop_out, r.out_bytes);
    else {
        sort_run(c, static_cast<const uint8_t*>(c->setop_out.p), r.out_bytes, false);
        s.sorted = 1;
        s.ms_sort = c->sstats.ms_total;
    }
    s.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    T::have(c) = true;
}

// the checked call: the text in HBM (host false) or in host memory; sopt: encode the sorted result with it
template <class T>
int text_call(starch_ctx* c, const typename T::Options& opt, bool no_sort, const void* data, uint64_t n, bool host,
              const starch_options* sopt)
{
    GUARD(c)
    if (sopt) c->have = false;
    c->have_out = false;
    T::have(c) = false;
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* d = host ? sort_upload(c, data, n) : static_cast<const uint8_t*>(data);
    text_run<T>(c, opt, no_sort, d, n, t0);
    // the sorted text is in sort_out, which no encoder stage writes
    if (sopt) encode_device(c, c->out_dev, c->out_bytes, *sopt);
    return STARCH_OK;
    END_GUARD(c)
}
}  // namespace

// ---- convert2bed (include/starch_amd.h; kernels in bed_convert.hip) ------------------
namespace {
bool convert_options_ok(const starch_convert_options* o, cv::ConvertOptions* out)
{
    if (!o || o->format > STARCH_CONVERT_WIG || o->vcf_class > STARCH_VCF_DELETIONS) return false;
    if (o->vcf_class != STARCH_VCF_ALL && o->format != STARCH_CONVERT_VCF) return false;
    out->format = o->format;
    out->vcf_class = o->vcf_class;
    out->keep_header = o->keep_header ? 1 : 0;
    return true;
}

struct ConvertTool {
    typedef cv::ConvertOptions Options;
    typedef cv::ConvertResult Result;
    typedef starch_convert_stats Stats;
    static Stats& stats(starch_ctx* c) { return c->vstats; }
    static bool& have(starch_ctx* c) { return c->have_vstats; }
    static void run(starch_ctx* c, const Options& o, const uint8_t* d, uint64_t n, Result& r)
    {
        c->converter.run(c->sorter, o, d, n, c->st, c->setop_out, r);
    }
    static void own(Stats& s, const Result& r)
    {
        s.data_lines = r.data_lines;
        s.declarations = r.declarations;
    }
};
}  // namespace

extern "C" {

int starch_convert_device(starch_ctx* c, const void* d_data, uint64_t n, const starch_convert_options* opt)
{
    cv::ConvertOptions co;
    if (!c || !convert_options_ok(opt, &co) || (n && !d_data)) return STARCH_ERR_ARG;
    return text_call<ConvertTool>(c, co, opt->no_sort != 0, d_data, n, false, nullptr);
}

int starch_convert_host(starch_ctx* c, const void* data, uint64_t n, const starch_convert_options* opt)
{
    cv::ConvertOptions co;
    if (!c || !convert_options_ok(opt, &co) || (n && !data)) return STARCH_ERR_ARG;
    return text_call<ConvertTool>(c, co, opt->no_sort != 0, data, n, true, nullptr);
}

int starch_convert_encode_host(starch_ctx* c, const void* data, uint64_t n, const starch_convert_options* copt,
                               const starch_options* sopt)
{
    cv::ConvertOptions co;
    if (!c || !convert_options_ok(copt, &co) || copt->no_sort || (n && !data)) return STARCH_ERR_ARG;
    const starch_options o = options_of(sopt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    return text_call<ConvertTool>(c, co, false, data, n, true, &o);
}

int starch_convert_get_stats(starch_ctx* c, starch_convert_stats* out)
{
    return pair_get_stats<ConvertTool>(c, out);
}

int starch_convert_constants(uint32_t* block_lines, uint32_t* wave_copy_bytes)
{
    if (block_lines) *block_lines = (uint32_t)cv::kThreads;
    if (wave_copy_bytes) *wave_copy_bytes = sb::kWaveCopyBytes;
    return STARCH_OK;
}

}  // extern "C"

// ---- sam2bed, psl2bed, rmsk2bed (include/starch_amd.h; kernels in bed_align.hip) -----
namespace {
bool align_options_ok(const starch_align_options* o, al::AlignOptions* out)
{
    if (!o || o->format > STARCH_ALIGN_RMSK) return false;
    if (o->split_deletions && !o->split) return false;
    if (o->format == STARCH_ALIGN_RMSK && o->split) return false;
    if (o->format != STARCH_ALIGN_SAM && (o->split_deletions || o->all_reads || o->reduced)) return false;
    out->format = o->format;
    out->split = o->split ? 1 : 0;
    out->split_deletions = o->split_deletions ? 1 : 0;
    out->all_reads = o->all_reads ? 1 : 0;
    out->reduced = o->reduced ? 1 : 0;
    out->keep_header = o->keep_header ? 1 : 0;
    return true;
}

struct AlignTool {
    typedef al::AlignOptions Options;
    typedef al::AlignResult Result;
    typedef starch_align_stats Stats;
    static Stats& stats(starch_ctx* c) { return c->astats; }
    static bool& have(starch_ctx* c) { return c->have_astats; }
    static void run(starch_ctx* c, const Options& o, const uint8_t* d, uint64_t n, Result& r)
    {
        c->aligner.run(c->sorter, o, d, n, c->st, c->setop_out, r);
    }
    static void own(Stats& s, const Result& r)
    {
        s.records = r.records;
        s.unmapped_dropped = r.unmapped_dropped;
    }
};
}  // namespace

extern "C" {

int starch_align_device(starch_ctx* c, const void* d_data, uint64_t n, const starch_align_options* opt)
{
    al::AlignOptions ao;
    if (!c || !align_options_ok(opt, &ao) || (n && !d_data)) return STARCH_ERR_ARG;
    return text_call<AlignTool>(c, ao, opt->no_sort != 0, d_data, n, false, nullptr);
}

int starch_align_host(starch_ctx* c, const void* data, uint64_t n, const starch_align_options* opt)
{
    al::AlignOptions ao;
    if (!c || !align_options_ok(opt, &ao) || (n && !data)) return STARCH_ERR_ARG;
    return text_call<AlignTool>(c, ao, opt->no_sort != 0, data, n, true, nullptr);
}

int starch_align_encode_host(starch_ctx* c, const void* data, uint64_t n, const starch_align_options* aopt,
                             const starch_options* sopt)
{
    al::AlignOptions ao;
    if (!c || !align_options_ok(aopt, &ao) || aopt->no_sort || (n && !data)) return STARCH_ERR_ARG;
    const starch_options o = options_of(sopt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    return text_call<AlignTool>(c, ao, false, data, n, true, &o);
}

int starch_align_get_stats(starch_ctx* c, starch_align_stats* out)
{
    return pair_get_stats<AlignTool>(c, out);
}

int starch_align_constants(uint32_t* block_lines, uint32_t* wave_copy_bytes)
{
    if (block_lines) *block_lines = (uint32_t)al::kThreads;
    if (wave_copy_bytes) *wave_copy_bytes = sb::kWaveCopyBytes;
    return STARCH_OK;
}

}  // extern "C"

// ---- bam2bed (include/starch_amd.h; kernels in bed_bam.hip) -----------------------------
namespace {
bool bam_options_ok(const starch_bam_options* o, bam::BamOptions* out)
{
    if (!o || (o->split_deletions && !o->split)) return false;
    out->split = o->split ? 1 : 0;
    out->split_deletions = o->split_deletions ? 1 : 0;
    out->all_reads = o->all_reads ? 1 : 0;
    out->reduced = o->reduced ? 1 : 0;
    out->keep_header = o->keep_header ? 1 : 0;
    return true;
}

// The checked call: BAM bytes in host memory (compressed or not), or inflated
// BAM in HBM (host false); converted into setop_out and, unless no_sort, sorted
// from there into sort_out; sopt: encode the sorted result with it.
int bam_call(starch_ctx* c, const bam::BamOptions& opt, bool no_sort, const void* data, uint64_t n, bool host, const starch_options* sopt)
{
    GUARD(c)
    if (sopt) c->have = false;
    c->have_out = false;
    c->have_bstats = false;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t input_bytes = n;
    const uint8_t* d = static_cast<const uint8_t*>(data);
    float ms_inflate = 0;
    if (host) {
        const bool gzip = gz::is_gzip(data, n);
        if (!gzip && !(n >= 4 && memcmp(data, "BAM\1", 4) == 0))
            throw StarchError(STARCH_ERR_DATA, "bam2bed: the input is neither gzip nor BAM (it does not begin BAM\\1)");
        d = sort_upload(c, data, n);   // a gzip input is inflated in HBM; n becomes its inflated size
        if (gzip) ms_inflate = c->gstats.ms_size + c->gstats.ms_inflate + c->gstats.ms_crc;
    }
    bam::BamResult r;
    c->bammer.run(opt, d, n, c->st, c->setop_out, r);
    starch_bam_stats& s = c->bstats;
    s = starch_bam_stats{};
    s.input_bytes = input_bytes;
    s.inflated_bytes = n;
    s.references = r.references;
    s.header_lines = r.header_lines;
    s.records = r.records;
    s.unmapped_dropped = r.unmapped_dropped;
    s.tiles = r.tiles;
    s.wave_records = r.wave_records;
    s.lines_out = r.lines_out;
    s.output_bytes = r.out_bytes;
    s.ms_inflate = ms_inflate;
    s.ms_frame = r.ms_frame;
    s.ms_parse = r.ms_parse;
    s.ms_write = r.ms_write;
    if (no_sort) publish(c, c->setop_out, r.out_bytes);
    else {
        sort_run(c, static_cast<const uint8_t*>(c->setop_out.p), r.out_bytes, false);
        s.sorted = 1;
        s.ms_sort = c->sstats.ms_total;
    }
    s.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->have_bstats = true;
    // the sorted text is in sort_out, which no encoder stage writes
    if (sopt) encode_device(c, c->out_dev, c->out_bytes, *sopt);
    return STARCH_OK;
    END_GUARD(c)
}
}  // namespace

extern "C" {

int starch_bam_device(starch_ctx* c, const void* d_data, uint64_t n, const starch_bam_options* opt)
{
    bam::BamOptions bo;
    if (!c || !bam_options_ok(opt, &bo) || (n && !d_data)) return STARCH_ERR_ARG;
    return bam_call(c, bo, opt->no_sort != 0, d_data, n, false, nullptr);
}

int starch_bam_host(starch_ctx* c, const void* data, uint64_t n, const starch_bam_options* opt)
{
    bam::BamOptions bo;
    if (!c || !bam_options_ok(opt, &bo) || (n && !data)) return STARCH_ERR_ARG;
    return bam_call(c, bo, opt->no_sort != 0, data, n, true, nullptr);
}

int starch_bam_encode_host(starch_ctx* c, const void* data, uint64_t n, const starch_bam_options* bopt, const starch_options* sopt)
{
    bam::BamOptions bo;
    if (!c || !bam_options_ok(bopt, &bo) || bopt->no_sort || (n && !data)) return STARCH_ERR_ARG;
    const starch_options o = options_of(sopt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    return bam_call(c, bo, false, data, n, true, &o);
}

int starch_bam_get_stats(starch_ctx* c, starch_bam_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_bstats) return STARCH_ERR_STATE;
    *out = c->bstats;
    return STARCH_OK;
}

int starch_bam_constants(uint32_t* tile_bytes, uint32_t* block_records, uint32_t* wave_threshold)
{
    if (tile_bytes) *tile_bytes = bam::kTileBytes;
    if (block_records) *block_records = (uint32_t)bam::kThreads;
    if (wave_threshold) *wave_threshold = bam::kWaveThreshold;
    return STARCH_OK;
}

}  // extern "C"

// ---- bigWig / bigBed files read on the host (include/starch_amd.h; bed_bbi.hip) ----------
namespace {
// a mismatch of kind and file is found once the file is read
bool bbi_query_ok(const starch_bbi_query* q, bbi::Region* out)
{
    if (!q || q->kind > STARCH_BBI_BIGBED || q->region > 2) return false;
    if (q->region && (!q->chrom || !q->chrom_len)) return false;
    if (q->region == 2 && q->start >= q->end) return false;
    out->any = q->region != 0;
    out->whole = q->region != 2;
    if (q->region) out->chrom.assign(q->chrom, q->chrom_len);
    out->start = q->start;
    out->end = q->end;
    return true;
}
}  // namespace

extern "C" {

int starch_bbi_info(const void* data, uint64_t n, const starch_bbi_query* q, starch_bbi_header* hdr, uint32_t* chrom_sizes,
                    uint64_t chrom_cap, char* names, uint64_t names_cap, starch_bbi_block* blocks, uint64_t* block_index,
                    uint64_t block_cap, char* err, uint64_t err_cap)
{
    if ((n && !data) || !hdr || (chrom_cap && !chrom_sizes) || (names_cap && !names) || (block_cap && !blocks)) return STARCH_ERR_ARG;
    if (err && err_cap) err[0] = 0;
    bbi::Region rg;
    if (q && !bbi_query_ok(q, &rg)) return STARCH_ERR_ARG;
    try {
        bbi::Info info;
        bbi::parse(static_cast<const uint8_t*>(data), n, info);
        if (q && q->kind != STARCH_BBI_AUTO && q->kind != info.kind)
            throw StarchError(STARCH_ERR_DATA, std::string("bbi: the file is a ") + (info.kind == bbi::KIND_BIGWIG ? "bigWig" : "bigBed") +
                                                   ", not the kind that was asked for");
        int64_t chrom_id = -1;
        const std::vector<uint64_t> sel = bbi::select(info, rg, &chrom_id);
        uint64_t names_bytes = 0;
        for (const bbi::Chrom& ch : info.chroms) names_bytes += ch.name.size() + 1;
        *hdr = starch_bbi_header{info.kind, info.version, info.zoom_levels, info.field_count, info.defined_field_count,
                                 info.uncompress_buf_size, info.chrom_tree_offset, info.full_data_offset, info.full_index_offset,
                                 info.chroms.size(), names_bytes, info.blocks.size(), sel.size()};
        bool small = false;
        if (chrom_sizes || chrom_cap) {
            if (chrom_cap < info.chroms.size()) small = true;
            else for (uint64_t k = 0; k < info.chroms.size(); ++k) chrom_sizes[k] = info.chroms[k].size;
        }
        if (names || names_cap) {
            if (names_cap < names_bytes) small = true;
            else {
                uint64_t at = 0;
                for (const bbi::Chrom& ch : info.chroms) {
                    memcpy(names + at, ch.name.c_str(), ch.name.size() + 1);
                    at += ch.name.size() + 1;
                }
            }
        }
        if (blocks || block_cap) {
            if (block_cap < sel.size()) small = true;
            else for (uint64_t k = 0; k < sel.size(); ++k) {
                const bbi::Block& b = info.blocks[sel[k]];
                blocks[k] = starch_bbi_block{b.start_chrom, b.start_base, b.end_chrom, b.end_base, b.data_offset, b.data_size};
                if (block_index) block_index[k] = sel[k];
            }
        }
        return small ? STARCH_ERR_MEM : STARCH_OK;
    } catch (const StarchError& e) {
        if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
        return e.code;
    } catch (const std::exception& e) {
        if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
        return STARCH_ERR_INTERNAL;
    }
}

int starch_bbi_adler32_host(const void* data, uint64_t n, uint32_t piece, uint32_t* adler)
{
    if ((n && !data) || !adler || piece < 1 || piece > gz::kAdlerMaxPiece) return STARCH_ERR_ARG;
    *adler = gz::adler32_pieces(static_cast<const uint8_t*>(data), n, piece);
    return STARCH_OK;
}

}  // extern "C"

// ---- bigwig2bed, bigbed2bed (include/starch_amd.h; kernels in bed_bbi_dev.hip, zlib blocks through gz_inflate.hip) ----
namespace {
constexpr uint32_t kBbiModestSlot = 1u << 20;   // an uncompressBufSize up to which every block gets a slot of that size ...
constexpr uint64_t kBbiModestArea = 1ull << 30;   // ... while all the slots together stay below this

struct BbiStaged {         // a file's selected blocks in HBM, inflated when the file is compressed
    bbidev::Input in;
    uint64_t uploaded = 0, inflated = 0, sized = 0, slot_bytes = 0;   // slot_bytes: the slots and the gaps behind them
    float ms_upload = 0, ms_size = 0, ms_inflate = 0, ms_adler = 0;
    bool compressed = false;
};

const char* bbi_tool(uint32_t kind) { return kind == bbi::KIND_BIGWIG ? "bigwig2bed" : "bigbed2bed"; }

[[noreturn]] void bbi_bad_block(uint32_t kind, uint64_t index, const std::string& why)
{
    throw StarchError(STARCH_ERR_DATA, std::string(bbi_tool(kind)) + ": block " + std::to_string(index) + ": " + why);
}

// The file read on the host, the blocks of q's region uploaded as one range (from
// the first selected block to the end of the last) into dec_in and, when the file
// is compressed, inflated into c->input: block k into a slot, `gap` bytes apart.
// The region's lines are chosen later, on the device.
void bbi_stage(starch_ctx* c, const uint8_t* file, uint64_t n, const starch_bbi_query* q, const bbi::Region& rg, uint32_t gap,
               BbiStaged& s)
{
    bbi::Info info;
    bbi::parse(file, n, info);
    if (q && q->kind != STARCH_BBI_AUTO && q->kind != info.kind)
        throw StarchError(STARCH_ERR_DATA, std::string("bbi: the file is a ") + (info.kind == bbi::KIND_BIGWIG ? "bigWig" : "bigBed") +
                                               ", not the kind that was asked for");
    int64_t chrom_id = -1;
    const std::vector<uint64_t> sel = bbi::select(info, rg, &chrom_id);
    bbidev::Input& in = s.in;
    in.kind = info.kind;
    for (const bbi::Chrom& ch : info.chroms) in.chroms.push_back(ch.name);
    in.rg = bbirec::Region{rg.any ? (rg.whole ? 1u : 2u) : 0u, chrom_id < 0 ? bbirec::kNoChrom : (uint32_t)chrom_id, rg.start, rg.end};
    in.index = sel;
    s.compressed = info.uncompress_buf_size != 0;
    if (sel.empty()) return;
    const uint64_t up0 = info.blocks[sel.front()].data_offset;
    const uint64_t up_n = info.blocks[sel.back()].data_offset + info.blocks[sel.back()].data_size - up0;
    uint8_t* d_in = c->dec_in.as<uint8_t>(up_n + gz::kInPad);   // 8-byte aligned, with the inflater's read-ahead padding
    {
        StageTimer<2> tm;
        tm.start(c->st);
        HostRegistration reg(file + up0, up_n, 256ull << 20);
        reg.h2d(d_in, file + up0, up_n, c->st);
        HIP_CHECK(hipMemsetAsync(d_in + up_n, 0, gz::kInPad, c->st));
        tm.finish(1, c->st, {&s.ms_upload});
    }
    s.uploaded = up_n;
    const uint64_t B = sel.size();
    in.off.resize(B);
    in.len.resize(B);
    if (!s.compressed) {
        for (uint64_t k = 0; k < B; ++k) {
            in.off[k] = info.blocks[sel[k]].data_offset - up0;
            in.len[k] = info.blocks[sel[k]].data_size;
        }
        in.d = d_in;
        return;
    }
    // zlib blocks (RFC 1950): the two header bytes are checked here, from the file's bytes
    const uint64_t ubs = info.uncompress_buf_size;
    std::vector<gz::Member> tab(B);
    for (uint64_t k = 0; k < B; ++k) {
        const bbi::Block& b = info.blocks[sel[k]];
        const uint8_t* p = file + b.data_offset;
        if (b.data_size < 6) bbi_bad_block(info.kind, sel[k], "shorter than a zlib header and trailer");
        if ((p[0] & 15u) != 8u) bbi_bad_block(info.kind, sel[k], "zlib compression method is not 8 (deflate)");
        if (((uint32_t)p[0] * 256u + p[1]) % 31u != 0) bbi_bad_block(info.kind, sel[k], "zlib header check fails (CMF * 256 + FLG is no multiple of 31)");
        if (p[1] & 0x20u) bbi_bad_block(info.kind, sel[k], "zlib preset dictionary (FDICT) is not supported");
        const uint8_t* t = p + b.data_size - 4;
        gz::Member m{};
        m.in_off = b.data_offset - up0;
        m.in_len = b.data_size;
        m.out_len = ubs;
        m.crc = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
        m.hdr_len = 2;
        tab[k] = m;
    }
    std::vector<gz::TableResult> res;
    auto check = [&] {
        for (uint64_t k = 0; k < B; ++k)
            if (res[k].err) bbi_bad_block(info.kind, sel[k], gz::inflate_error_text(res[k].err));
    };
    if (ubs > kBbiModestSlot || ubs * B > kBbiModestArea) {   // a declared size far above what blocks hold: the slots are what the blocks inflate to
        c->zinflater.run(d_in, up_n, tab, 4, false, false, nullptr, c->st, res);
        check();
        for (uint64_t k = 0; k < B; ++k) tab[k].out_len = res[k].produced;
        s.sized = 1;
        s.ms_size = c->zinflater.ms_inflate;
    }
    uint64_t total = 0;
    for (gz::Member& m : tab) {
        m.out_off = total;
        total += m.out_len + gap;
    }
    uint8_t* d_out = c->input.as<uint8_t>(total + 64);
    if (gap) HIP_CHECK(hipMemsetAsync(d_out, 0xA5, total, c->st));   // (starch_bbi_inflate_host: the guard behind every slot)
    c->zinflater.run(d_in, up_n, tab, 4, true, true, d_out, c->st, res);
    check();
    s.ms_inflate = c->zinflater.ms_inflate;
    s.ms_adler = c->zinflater.ms_check;
    for (uint64_t k = 0; k < B; ++k) {
        in.off[k] = tab[k].out_off;
        in.len[k] = res[k].produced;
        s.inflated += res[k].produced;
    }
    in.d = d_out;
    c->bbi_slot_off.assign(B, 0);
    for (uint64_t k = 0; k < B; ++k) c->bbi_slot_off[k] = tab[k].out_off;
    c->bbi_slot_len = in.len;
    s.slot_bytes = total;
}

// The checked call: the file's bytes in host memory; converted into setop_out
// and, unless no_sort, sorted from there into sort_out; sopt: encode the sorted
// result with it.
int bbi_call(starch_ctx* c, const void* data, uint64_t n, const starch_bbi_query* q, const bbi::Region& rg, bool no_sort,
             const starch_options* sopt)
{
    GUARD(c)
    if (sopt) c->have = false;
    c->have_out = false;
    c->have_bbstats = false;
    const auto t0 = std::chrono::steady_clock::now();
    BbiStaged sg;
    bbi_stage(c, static_cast<const uint8_t*>(data), n, q, rg, 0, sg);
    bbidev::Result r;
    c->bbier.run(sg.in, c->st, c->setop_out, r);
    starch_bbi_stats& s = c->bbstats;
    s = starch_bbi_stats{};
    s.input_bytes = n;
    s.uploaded_bytes = sg.uploaded;
    s.inflated_bytes = sg.compressed ? sg.inflated : sg.uploaded;
    s.kind = sg.in.kind;
    s.compressed = sg.compressed ? 1 : 0;
    s.blocks = r.blocks;
    s.sized = sg.sized;
    s.records = r.records;
    s.wave_records = r.wave_records;
    s.lines_out = r.lines_out;
    s.output_bytes = r.out_bytes;
    s.ms_upload = sg.ms_upload;
    s.ms_size = sg.ms_size;
    s.ms_inflate = sg.ms_inflate;
    s.ms_adler = sg.ms_adler;
    s.ms_frame = r.ms_frame;
    s.ms_parse = r.ms_parse;
    s.ms_write = r.ms_write;
    if (no_sort) publish(c, c->setop_out, r.out_bytes);
    else {
        sort_run(c, static_cast<const uint8_t*>(c->setop_out.p), r.out_bytes, false);
        s.sorted = 1;
        s.ms_sort = c->sstats.ms_total;
    }
    s.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->have_bbstats = true;
    // the sorted text is in sort_out, which no encoder stage writes
    if (sopt) encode_device(c, c->out_dev, c->out_bytes, *sopt);
    return STARCH_OK;
    END_GUARD(c)
}
}  // namespace

extern "C" {

int starch_bbi_host(starch_ctx* c, const void* data, uint64_t n, const starch_bbi_query* q, uint32_t no_sort)
{
    bbi::Region rg;
    if (!c || (n && !data) || (q && !bbi_query_ok(q, &rg))) return STARCH_ERR_ARG;
    return bbi_call(c, data, n, q, rg, no_sort != 0, nullptr);
}

int starch_bbi_device(starch_ctx* c, const void* d_data, uint64_t n, const starch_bbi_query* q, uint32_t no_sort)
{
    bbi::Region rg;
    if (!c || (n && !d_data) || (q && !bbi_query_ok(q, &rg))) return STARCH_ERR_ARG;
    std::vector<uint8_t> h(n);                 // the header and the trees are read on the host
    {
        GUARD(c)
        if (n) HIP_CHECK(hipMemcpyAsync(h.data(), d_data, n, hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
        END_GUARD(c)
    }
    return bbi_call(c, h.data(), n, q, rg, no_sort != 0, nullptr);
}

int starch_bbi_encode_host(starch_ctx* c, const void* data, uint64_t n, const starch_bbi_query* q, const starch_options* sopt)
{
    bbi::Region rg;
    if (!c || (n && !data) || (q && !bbi_query_ok(q, &rg))) return STARCH_ERR_ARG;
    const starch_options o = options_of(sopt);
    if (!options_ok(o)) return STARCH_ERR_ARG;
    return bbi_call(c, data, n, q, rg, false, &o);
}

int starch_bbi_get_stats(starch_ctx* c, starch_bbi_stats* out)
{
    if (!c || !out) return STARCH_ERR_ARG;
    if (!c->have_bbstats) return STARCH_ERR_STATE;
    *out = c->bbstats;
    return STARCH_OK;
}

int starch_bbi_constants(uint32_t* block_records, uint32_t* wave_rest, uint32_t* modest_slot, uint32_t* adler_piece)
{
    if (block_records) *block_records = (uint32_t)bbidev::kThreads;
    if (wave_rest) *wave_rest = bbidev::kWaveRest;
    if (modest_slot) *modest_slot = kBbiModestSlot;
    if (adler_piece) *adler_piece = gz::kAdlerPiece;
    return STARCH_OK;
}

int starch_bbi_inflate_host(starch_ctx* c, const void* data, uint64_t n, const starch_bbi_query* q, uint32_t gap)
{
    bbi::Region rg;
    if (!c || (n && !data) || (q && !bbi_query_ok(q, &rg))) return STARCH_ERR_ARG;
    GUARD(c)
    c->have_out = false;
    c->bbi_slot_off.clear();
    c->bbi_slot_len.clear();
    c->bbi_pad_ok = 0;
    BbiStaged sg;
    bbi_stage(c, static_cast<const uint8_t*>(data), n, q, rg, gap, sg);
    if (!sg.compressed) throw StarchError(STARCH_ERR_ARG, "bbi: the file's blocks are not compressed");
    if (sg.in.off.empty()) {
        publish(c, c->input, 0);
        c->bbi_pad_ok = 1;
        return STARCH_OK;
    }
    uint8_t pad[gz::kInPad];
    HIP_CHECK(hipMemcpyAsync(pad, static_cast<const uint8_t*>(c->dec_in.p) + sg.uploaded, sizeof pad, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->bbi_pad_ok = 1;
    for (uint8_t v : pad)
        if (v) c->bbi_pad_ok = 0;
    publish(c, c->input, sg.slot_bytes);
    return STARCH_OK;
    END_GUARD(c)
}

int starch_bbi_inflate_table(starch_ctx* c, uint64_t* off, uint64_t* len, uint64_t cap, uint64_t* n_blocks, uint64_t* input_pad_ok)
{
    if (!c || !n_blocks || (cap && (!off || !len))) return STARCH_ERR_ARG;
    if (!c->have_out) return STARCH_ERR_STATE;
    *n_blocks = c->bbi_slot_off.size();
    if (input_pad_ok) *input_pad_ok = c->bbi_pad_ok;
    if (cap < c->bbi_slot_off.size()) return STARCH_ERR_MEM;
    for (uint64_t k = 0; k < c->bbi_slot_off.size(); ++k) {
        off[k] = c->bbi_slot_off[k];
        len[k] = c->bbi_slot_len[k];
    }
    return STARCH_OK;
}

}  // extern "C"
