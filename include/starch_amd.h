/*
 * include/starch_amd.h -- C ABI of the MI355X Starch compressor
 * (libstarch_amd.so, built from starch_amd/csrc/ for gfx950).
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Every entry point returns an int status: STARCH_OK (0) or a negative code
 * (starch_strerror()).  Device pointers are HIP device pointers on the
 * context's device; host pointers are ordinary memory.  One context per
 * thread (a context owns its HIP stream and HBM workspace); contexts on
 * different devices are independent.
 *
 * What each entry point replaces in the reference (alexpreynolds/starch3):
 *   starch_encode_*      the whole starch3 pipeline: produce_line/consume_line
 *                        (include/starch3api.hpp:158-345), update_transformation_
 *                        state (hpp:428-504), per-chromosome flush
 *                        process_tf_buffer (hpp:393-407), and the libbz2
 *                        compressor the reference links for it (hpp:819-888,
 *                        initialize_bz_stream_ptr: BZ2_bzCompressInit(s, 9, .., 30))
 *   starch_transform_*   hpp:158-504 alone (the stderr "Content" text)
 *   starch_bz2_compress_* one BZ2_bzCompressInit + BZ2_bzCompress(BZ_FINISH)
 *                        stream (bz:bzlib.c:148-474), byte-identical
 *   starch_bz2_decompress_* / starch_unstarch_host
 *                        the decompression side: bzip2-1.0.6's
 *                        BZ2_bzDecompress (bz:decompress.c:106-646,
 *                        bz:bzlib.c:621-708) over concatenated streams, and the
 *                        inverse of hpp:428-504 (segment text -> BED lines),
 *                        which the reference does not ship (BEDOPS unstarch)
 *   the archive layout   magic bytes ca 5c ad 1a (hpp:765-769, 907-910), then
 *                        one bzip2 stream per chromosome segment, then a JSON
 *                        index and a 32-byte footer (DESIGN.md "Archive")
 * The patched-libbz2 streaming ABI (BZ2_bzCompress*) lives in
 * include/starch_bzlib.h.
 */
#ifndef STARCH_AMD_H_
#define STARCH_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STARCH_OK 0
#define STARCH_ERR_ARG (-2)        /* bad argument (bz: BZ_PARAM_ERROR) */
#define STARCH_ERR_MEM (-3)        /* allocation / capacity (bz: BZ_MEM_ERROR) */
#define STARCH_ERR_STATE (-4)      /* no result yet */
#define STARCH_ERR_DEVICE (-10)    /* HIP runtime error or no MI355X */
#define STARCH_ERR_INTERNAL (-11)
#define STARCH_ERR_DATA (-12)       /* malformed / corrupt compressed data (bz: BZ_DATA_ERROR, BZ_DATA_ERROR_MAGIC) */

typedef struct starch_ctx starch_ctx;

typedef struct {
    int block_size_100k;     /* bzip2 level, 1..9 (reference uses 9, hpp:837) */
    int emit_index;          /* 1: append JSON index + footer after the streams */
    int reference_compat;    /* 1: archive is exactly the reference's stdout (magic only) */
    const char* note;        /* --note text for the index (may be NULL) */
    int base_counts;         /* 1: per-segment base counts (hpp:61-62) in the segments and the index */
    int compression_method;  /* STARCH_METHOD_BZIP2 (0, default) or STARCH_METHOD_GZIP (1): the reference's
                              * compression_method_t (hpp:23-27); gzip there exits ENOSYS (hpp:777-779),
                              * here every segment is one gzip member (fixed-Huffman deflate on the GPU) */
} starch_options;

#define STARCH_METHOD_BZIP2 0
#define STARCH_METHOD_GZIP 1

typedef struct {
    uint64_t line_count;     /* transform_state_t.line_count at flush (hpp:395) */
    uint64_t text_bytes;     /* transformed bytes of this segment */
    uint64_t stream_offset;  /* byte offset of its bzip2 stream in the archive */
    uint64_t stream_bytes;
    uint64_t name_len;       /* chromosome name length (starch_segment_name) */
    uint32_t n_blocks;       /* bzip2 blocks in the stream */
    uint32_t combined_crc;   /* bzip2 combined stream CRC */
    uint64_t unit;           /* input unit the segment came from (archive order = unit order) */
    /* transform_state_t.base_count_unique / _nonunique (hpp:61-62; declared,
     * never computed by the reference), filled when starch_options.base_counts:
     * nonunique = sum of (stop - start) over the segment's lines, unique = sum
     * of max(0, stop - max(start, largest earlier stop)) = size of the union
     * of the intervals for a BED sorted by start; modulo 2^64. */
    int64_t base_count_unique;
    int64_t base_count_nonunique;
} starch_segment;

/* A unit: a byte range of the input whose first line starts a chromosome
 * segment, i.e. its chr token differs from the previous line's (hpp:325-342).
 * Units are encoded independently and their streams concatenate to the
 * whole input's.  init_start / init_stop are the sscanf values current before
 * the unit (a field that fails to parse keeps the previous line's value,
 * hpp:306-307); 0 for the first unit. */
typedef struct {
    uint64_t offset;
    uint64_t length;
    int64_t init_start;
    int64_t init_stop;
} starch_unit;

typedef struct {
    uint64_t input_bytes, n_lines, n_segments, text_bytes, archive_bytes;
    uint64_t n_blocks, rle_bytes, bwt_rounds, periodic_blocks;
    uint64_t bwt_tied;       /* rotations re-sorted by prefix-doubling rounds (ties of the packed key) */
    uint64_t dedup_blocks;   /* blocks that reused a byte-identical block's sort/MTF/tables */
    float ms_transform, ms_rle, ms_bwt, ms_mtf, ms_tables, ms_emit, ms_total;
} starch_stats;

int starch_version(void);                         /* 0x000100 = 0.1.0 */
const char* starch_strerror(int code);
const char* starch_last_error(starch_ctx* ctx);   /* detail text of the last failure */

int starch_create(int device, starch_ctx** out);
void starch_destroy(starch_ctx* ctx);
/* Run the context's work on an external hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream.  NULL (0) is the HIP null stream
 * itself: work the caller queued there (an H2D copy, a generator kernel) is
 * ordered before the encode with no host synchronisation.  The context still
 * uses private streams inside a call; they wait for the selected stream on
 * entry and the selected stream waits for them before the call returns. */
int starch_set_stream(starch_ctx* ctx, void* hip_stream);
/* Back to the context's own non-blocking stream (the default after
 * starch_create; not ordered with the null stream). */
int starch_use_own_stream(starch_ctx* ctx);
/* Encoder lanes of this context's device-path encodes (starch_encode_device,
 * starch_encode_host below its pipelined size, starch_encode_units_device):
 * after the one transform, the segments split into `lanes` contiguous runs of
 * about equal text, each encoded (RLE1 .. Huffman tables) by its own encoder
 * on its own stream and host thread, then emitted in order -- the archive
 * bytes do not depend on it.  1: one encoder; 2..8; 0: the default (the
 * STARCH_DEV_LANES environment variable, else 2).  Inputs under 16 MB of text
 * (STARCH_DEV_LANES_MIN) always take one.  Stage times in starch_stats are then
 * wall time during which any lane ran the stage. */
int starch_set_lanes(starch_ctx* ctx, int lanes);
void starch_options_init(starch_options* opt);

/* Whole pipeline.  Input BED bytes already in HBM (d_bed, n bytes).  The
 * archive stays in context-owned HBM until the next call. */
int starch_encode_device(starch_ctx* ctx, const void* d_bed, uint64_t n, const starch_options* opt);
/* Same, from host memory (copied to HBM first; the copy is not in ms_total). */
int starch_encode_host(starch_ctx* ctx, const void* bed, uint64_t n, const starch_options* opt);
/* Host bytes in, archive bytes out into the caller's host buffer out[0, cap)
 * (*out_len = its size; STARCH_ERR_MEM if cap is short, with *out_len = the
 * size needed and out's contents undefined -- finished batches may already
 * have been written into it).  For large pinned
 * inputs every chromosome batch's finished streams go device-to-host while
 * later batches still cross PCIe / encode, so the archive's PCIe trip
 * overlaps the work (pinned out recommended).  Same bytes as
 * starch_encode_host + starch_archive_copy; the archive also stays readable
 * through the accessors below.  (The reference writes its archive to stdout
 * from starch3.cpp's main loop, hpp:758-776.) */
int starch_encode_host_into(starch_ctx* ctx, const void* bed, uint64_t n, const starch_options* opt, void* out,
                            uint64_t cap, uint64_t* out_len);

/* ---- multi-GPU: per-chromosome units sharded across devices ----
 * Plan: split host BED bytes (up to the first 0xFF, hpp:181) into at most
 * max_units units (out must hold max_units entries) by galloping + bisection
 * over line starts -- the chromosome runs of a sorted BED, never a full scan. */
int starch_plan_units(const void* bed, uint64_t n, uint64_t max_units, starch_unit* out, uint64_t* nunits);
/* The same for bytes that continue an input: (init_start, init_stop) are the
 * sscanf values current before byte 0 (hpp:306-307; a batch that starts at a
 * chromosome change whose first lines do not parse keeps them). */
int starch_plan_units_from(const void* bed, uint64_t n, uint64_t max_units, int64_t init_start, int64_t init_stop,
                           starch_unit* out, uint64_t* nunits);
/* Longest-processing-time assignment of units to nshards (by byte length). */
int starch_assign_shards(const starch_unit* units, uint64_t nunits, int nshards, int32_t* shard_of);
/* One shard: encode units resident in HBM (offsets relative to d_base, in
 * input order; unit_ids = their global indices, NULL = 0..nunits-1).  The
 * result is the segments' bzip2 streams back to back (no magic, no index):
 * starch_streams_device/_copy; starch_segments gives each segment's unit and
 * stream_offset within the streams. */
int starch_encode_units_device(starch_ctx* ctx, const void* d_base, const starch_unit* units,
                               const uint64_t* unit_ids, uint64_t nunits, const starch_options* opt);
int starch_streams_device(starch_ctx* ctx, const void** d_ptr, uint64_t* n);
int starch_streams_copy(starch_ctx* ctx, void* dst, uint64_t cap);
/* Archive order of gathered segments (stable by unit) and their byte offsets
 * from base; *end = base + total stream bytes (the index offset). */
int starch_archive_layout(const uint64_t* unit_of, const uint64_t* bytes, uint64_t nseg, uint64_t base,
                          uint64_t* order, uint64_t* offset, uint64_t* end);
/* In-process multi-device encode of host bytes over nctx contexts (one host
 * thread per context; contexts may share a device -- "virtual shards").  The
 * finished streams are gathered into ctxs[0]'s HBM (hipMemcpyPeerAsync over
 * xGMI) and the archive is read through ctxs[0] as after starch_encode_host:
 * byte-identical to the one-context archive. */
int starch_encode_multi_host(starch_ctx* const* ctxs, int nctx, const void* bed, uint64_t n,
                             const starch_options* opt);

/* Same as starch_encode_units_device with the units in host memory (offsets
 * relative to bed): only the listed units are copied to HBM, packed. */
int starch_encode_units_host(starch_ctx* ctx, const void* bed, const starch_unit* units, const uint64_t* unit_ids,
                             uint64_t nunits, const starch_options* opt);

/* ---- the multi-rank gather (one process per GPU) ----------
 * Every rank encodes its units (starch_encode_units_*); starch_gather_archive
 * then collects all ranks' streams into rank 0's archive -- magic + streams in
 * unit order + index, byte-identical to the one-GPU archive -- with RCCL over
 * xGMI: an all-gather of segment counts, an all-gather of the segment records
 * and names, and grouped ncclSend/ncclRecv of the stream bytes straight into
 * their archive offsets.  Rank 0 reads the result through starch_archive_*,
 * starch_segments, starch_segment_name; other ranks see archive size 0.
 * Collective: every rank of the communicator calls it.  librccl is loaded on
 * first use (STARCH_ERR_DEVICE if absent). */
typedef struct starch_comm starch_comm;
#define STARCH_COMM_ID_BYTES 128
/* rank 0: a fresh RCCL unique id (ncclGetUniqueId) to hand to every rank */
int starch_comm_id(void* id);
/* one communicator per process, on the context's device */
int starch_comm_create(int device, int rank, int world, const void* id, starch_comm** out);
/* same, with the id handed out by rank 0 over TCP (rank 0 listens on port;
 * the others connect to host:port, retrying for up to 10 minutes) */
int starch_comm_create_tcp(int device, int rank, int world, const char* host, int port, starch_comm** out);
void starch_comm_destroy(starch_comm* comm);
/* Path of the librccl the gather uses (loaded on first use; "" when RCCL is
 * unavailable).  In a process that already loaded torch-ROCm's RCCL this is
 * that library: both resolve SONAME librccl.so.1 to one object. */
const char* starch_rccl_library(void);
const char* starch_comm_last_error(void);   /* detail of the last failed starch_comm_* / starch_gather_host */
int starch_gather_archive(starch_ctx* ctx, starch_comm* comm, const starch_options* opt);

/* The same gather over caller-supplied primitives on host memory (a test or
 * non-RCCL transport, e.g. torch.distributed gloo): all_gather(send, recv,
 * bytes) fills recv with world x bytes in rank order; send/recv post point-
 * to-point transfers whose order per peer pair matches on both sides and
 * which complete by the next group_end.  segs/names: this rank's segments
 * (stream_offset into streams; unit = global unit index).  Rank 0 receives
 * the archive in *archive (free with starch_free); elsewhere *archive = NULL. */
typedef struct {
    int rank, world;
    void* user;
    int (*all_gather)(void* user, const void* send, void* recv, uint64_t bytes);
    int (*send)(void* user, const void* buf, uint64_t n, int peer);
    int (*recv)(void* user, void* buf, uint64_t n, int peer);
    int (*group_end)(void* user);
} starch_host_comm;
int starch_gather_host(const starch_host_comm* comm, const starch_segment* segs, const char* const* names,
                       const uint64_t* name_lens, uint64_t nseg, const void* streams, const starch_options* opt,
                       void** archive, uint64_t* len);
void starch_free(void* p);
/* Page-lock [p, p + n) of caller memory (its whole pages) for the process,
 * so copies to and from it (starch_encode_host*, starch_transform_host*,
 * starch_text_read, the bzlib ABI's BZ2_bzCompress input) run by DMA at the
 * PCIe rate; a buffer reused across calls pays the pinning once (~0.03 s per
 * GB for memory already touched).  starch_host_unregister(p) with the same p
 * before the memory is freed (a read-only mapping is registered for reads
 * only: copies from it).  The library records the range and DMAs from it
 * only within it; a range overlapping one already registered (or one a
 * running call registered for itself) is refused with STARCH_ERR_ARG.
 * Memory page-locked by other means (hipHostMalloc, a framework's pinned
 * allocator) is used up to the end of its allocation.  No counterpart in the
 * reference (it has no device copies); the hpp's process_tf_buffer pool uses
 * them. */
int starch_host_register(const void* p, uint64_t n);
int starch_host_unregister(const void* p);

/* Streaming ingestion (replaces the reference's line-at-a-time
 * produce_line / consume_line hand-off, include/starch3api.hpp:158-345, and
 * the per-chromosome flush, hpp:393-407).  Feed host BED bytes in pieces of
 * any size (lines may straddle pieces); whenever at least batch_bytes
 * (0 = 256 MiB) are held, everything before the last chromosome change among
 * the complete lines is handed to the session's encoder thread (H2D, GPU
 * encode, D2H) while the caller keeps feeding into the other of two pinned
 * buffers; finished streams become readable with starch_stream_read (the
 * magic is readable at once).  Make no other calls on the context while a
 * session is open.
 * starch_stream_end encodes the rest and appends the index.  The bytes read
 * out, in order, are exactly the archive starch_encode_host gives for the
 * concatenated input.  A 0xFF byte ends the input (hpp:181): later bytes are
 * ignored.  After end, segments/stats describe the whole stream; the archive
 * accessors below report STARCH_ERR_STATE (the bytes went out by read). */
int starch_stream_begin(starch_ctx* ctx, const starch_options* opt, uint64_t batch_bytes);
int starch_stream_feed(starch_ctx* ctx, const void* bed, uint64_t n);
/* Zero-copy feed: a window of >= min_bytes in the session's pinned buffer to
 * read input into directly (e.g. read(2) from a file or pipe), then commit the
 * n bytes written there.  feed() = window + memcpy + commit. */
int starch_stream_window(starch_ctx* ctx, uint64_t min_bytes, void** ptr, uint64_t* cap);
int starch_stream_commit(starch_ctx* ctx, uint64_t n);
int starch_stream_end(starch_ctx* ctx);
int starch_stream_available(starch_ctx* ctx, uint64_t* n);
int starch_stream_read(starch_ctx* ctx, void* dst, uint64_t cap, uint64_t* len);

int starch_archive_size(starch_ctx* ctx, uint64_t* n);
int starch_archive_device(starch_ctx* ctx, const void** d_ptr);
int starch_archive_copy(starch_ctx* ctx, void* dst, uint64_t cap);
int starch_segment_count(starch_ctx* ctx, uint64_t* n);
int starch_segments(starch_ctx* ctx, starch_segment* out, uint64_t cap);
int starch_segment_name(starch_ctx* ctx, uint64_t i, char* buf, uint64_t cap, uint64_t* len);
int starch_get_stats(starch_ctx* ctx, starch_stats* out);

/* Transform stage only: afterwards starch_text_size/starch_text_copy give the
 * concatenated segment texts and starch_segments the per-segment counts. */
int starch_transform_host(starch_ctx* ctx, const void* bed, uint64_t n);
/* The same for bytes that start a segment of a longer input, with the sscanf
 * values current before them (a batch of whole chromosome runs). */
int starch_transform_host_init(starch_ctx* ctx, const void* bed, uint64_t n, int64_t init_start, int64_t init_stop);
int starch_transform_device(starch_ctx* ctx, const void* d_bed, uint64_t n);   /* BED bytes in HBM */
int starch_text_size(starch_ctx* ctx, uint64_t* n);
int starch_text_copy(starch_ctx* ctx, void* dst, uint64_t cap);
/* n bytes of that text from offset off (a segment's, at its stream_offset)
 * into dst: one chromosome's tf_buffer without a copy of the whole text. */
int starch_text_read(starch_ctx* ctx, uint64_t off, void* dst, uint64_t n);

/* One bzip2 stream (BZ_FINISH semantics) of n bytes; result to host. */
int starch_bz2_compress_host(starch_ctx* ctx, const void* in, uint64_t n, int block_size_100k, void* out,
                             uint64_t cap, uint64_t* out_len);
/* Block count and combined CRC of the (first) stream of the last
 * starch_bz2_compress_* call (the index fields of a process_tf_buffer hook). */
int starch_bz2_stream_info(starch_ctx* ctx, uint32_t* n_blocks, uint32_t* combined_crc);

/* Several independent bzip2 streams in one launch sequence (device memory):
 * stream k = d_in[offs[k] .. offs[k]+lens[k]); results packed back to back in
 * d_out (4-byte aligned), out_offs[k]/out_lens[k] filled. */
int starch_bz2_compress_many_device(starch_ctx* ctx, const void* d_in, const uint64_t* offs, const uint64_t* lens,
                                    uint64_t nstreams, int block_size_100k, void* d_out, uint64_t cap,
                                    uint64_t* out_offs, uint64_t* out_lens);

/* Synthetic hg38 BED generator (bench/tests): writes the lines of the given
 * chromosomes (indices into the 24 hg38 chromosomes in sort-bed order) into
 * dst; kind 0 = BED3 (cfg2), 1 = narrowPeak BED6+4 (cfg4), 2 = per-position
 * (cfg5).  total_lines is the whole-genome line count the per-chromosome
 * counts are derived from.  Returns bytes written via *len; pass dst = NULL to
 * size. */
int starch_gen_bed(int kind, uint64_t seed, uint64_t total_lines, const int32_t* chroms, int nchroms, void* dst,
                   uint64_t cap, uint64_t* len);
/* The per-position input (kind 2: "<chr>\t<p>\t<p+1>\n" for p in [first,
 * first + count)) of one chromosome written by the GPU into device memory
 * d_dst (cap bytes) on `stream` (asynchronous); *len = its byte count, which
 * d_dst = NULL returns alone (no GPU needed).  Same bytes as starch_gen_bed
 * kind 2 for that chromosome (cfg5's 73.6 GB input without the host). */
int starch_gen_perpos_device(int chrom, uint64_t first, uint64_t count, void* d_dst, uint64_t cap, uint64_t* len,
                             void* stream);
/* Per-chromosome byte counts of starch_gen_bed's output (sizes[k] for chroms[k]). */
int starch_gen_bed_sizes(int kind, uint64_t seed, uint64_t total_lines, const int32_t* chroms, int nchroms,
                         uint64_t* sizes);

/* Archive index writer: the JSON index + footer for a set of segments
 * (used by the multi-GPU gather to assemble rank 0's archive). */
int starch_build_index(const starch_segment* segs, const char* const* names, const uint64_t* name_lens,
                       uint64_t nseg, uint64_t index_offset, const char* note, int block_size_100k, char* dst,
                       uint64_t cap, uint64_t* len);
/* Same, with the index options taken from opt (note, block size, base counts). */
int starch_build_index_opt(const starch_segment* segs, const char* const* names, const uint64_t* name_lens,
                           uint64_t nseg, uint64_t index_offset, const starch_options* opt, char* dst, uint64_t cap,
                           uint64_t* len);

/* ---- decompression / unstarch -------------------------------
 * Results stay in the context: starch_output_size / _copy / _device. */
typedef struct {
    uint64_t in_beg, in_end;     /* the stream's bytes in the input */
    uint64_t out_off, out_len;   /* its decompressed bytes in the output */
    uint32_t level;              /* blockSize100k of its "BZh" header */
    uint32_t n_blocks;
    uint32_t combined_crc;       /* stored = recomputed (checked) */
} starch_dec_stream;

/* Every bzip2 stream of in[0, n) (concatenated streams, as bzip2 -d), decoded
 * on the GPU with every block CRC and stream CRC checked; STARCH_ERR_DATA on
 * malformed input or a CRC mismatch (bz: BZ_DATA_ERROR).  Randomised blocks
 * (bzip2 < 0.9.5) are refused. */
int starch_bz2_decompress_host(starch_ctx* ctx, const void* in, uint64_t n);
int starch_bz2_decompress_device(starch_ctx* ctx, const void* d_in, uint64_t n);
int starch_bz2_stream_count(starch_ctx* ctx, uint64_t* n);
int starch_bz2_streams(starch_ctx* ctx, starch_dec_stream* out, uint64_t cap);
/* Inverse transform of one segment's text: "chr\tstart\tstop[\trem]\n" lines.
 * Exact for canonical BED (decimal coordinates, stop >= start); a negative
 * p-value (whose newline the forward transform drops, hpp:440,452) or a
 * malformed line gives STARCH_ERR_DATA. */
int starch_untransform_host(starch_ctx* ctx, const void* text, uint64_t n, const char* chr, uint64_t chr_len);
/* A whole archive of this library (magic, streams, index, footer) back to BED:
 * every stream decoded and inverse-transformed on the GPU, in index order. */
int starch_unstarch_host(starch_ctx* ctx, const void* archive, uint64_t n);
/* ---- indexed extraction (BEDOPS `unstarch chr21 x.starch`) -----------------
 * A query is a list of regions: a chromosome name (exact bytes: "chr1" does
 * not match "chr10") and either the whole chromosome (whole != 0; start/stop
 * ignored) or the half-open range [start, stop), start < stop.  The result
 * (starch_output_*) is the lines starch_unstarch_host would give, in archive
 * order, each at most once, whose segment has a queried name and is either
 * queried whole or has line_start < stop && line_stop > start for one of its
 * regions (so a zero-length element x..x needs start < x < stop).  Only the
 * index entries with a queried name are read from the archive, decoded and
 * scanned; the coordinate filter runs on the GPU.  A chromosome revisited
 * later in the archive contributes every one of its segments.  nregions == 0:
 * the whole archive.  An absent chromosome or an empty result is STARCH_OK
 * with output size 0.  STARCH_ERR_ARG: start >= stop, a NULL name with a
 * non-zero length, or an archive whose index says compressionFormat "gzip"
 * (gzip members are not decoded; starch_archive_index still lists them). */
typedef struct {
    const char* chr;
    uint64_t chr_len;
    int64_t start, stop;
    int whole;
} starch_region;
int starch_extract_host(starch_ctx* ctx, const void* archive, uint64_t n, const starch_region* regions,
                        uint64_t nregions);
typedef struct {
    uint64_t streams_total;             /* index entries */
    uint64_t streams_decoded;           /* ... with a queried name */
    uint64_t compressed_bytes_decoded;  /* their stream bytes */
    uint64_t lines_scanned;             /* BED lines in the decoded segments */
    uint64_t lines_out;                 /* ... that were kept */
} starch_extract_stats;
int starch_extract_get_stats(starch_ctx* ctx, starch_extract_stats* out);

/* The archive's index as records (host only: no context, no GPU).  names
 * receives the chromosome names back to back (entry k: names[name_off,
 * name_off + name_len)).  out == NULL and names == NULL: *count / *names_len
 * alone.  STARCH_ERR_MEM when cap or names_cap is short; STARCH_ERR_DATA for
 * a damaged footer or index, or a stream outside [4, index offset).
 * compression_method: STARCH_METHOD_*. */
typedef struct {
    uint64_t name_off, name_len, offset, size, line_count, text_bytes;
    uint32_t n_blocks, combined_crc;
    int has_base_counts;
    int64_t base_count_unique, base_count_nonunique;
} starch_index_entry;
int starch_archive_index(const void* archive, uint64_t n, starch_index_entry* out, uint64_t cap, uint64_t* count,
                         char* names, uint64_t names_cap, uint64_t* names_len, int* compression_method,
                         int* block_size_100k);
/* The index's note as UTF-8 (buf == NULL: *len alone). */
int starch_archive_note(const void* archive, uint64_t n, char* buf, uint64_t cap, uint64_t* len);

/* ---- starchcat: merge archives (BEDOPS `starchcat a.starch b.starch`) -------
 * Inputs are narch >= 1 bzip2 archives of this library, in argument order.
 * All index entries with the same chromosome name (exact bytes) form a group;
 * its entries are its runs, ordered by input number, then by position in
 * that input's index.  The output holds one stream per group, the groups in
 * bytewise (memcmp, shorter first) order of their names.  A group is COPIED
 * when it has exactly one run, its archive's blockSize100k equals
 * opt->block_size_100k and, if opt->base_counts, its entry carries base
 * counts: the stream bytes and index fields are carried over and nothing of
 * it is decoded (so a damaged copied stream is not detected).  Every other
 * group is MERGED on the GPU: its runs are decoded, inverse-transformed,
 * merged by (start, stop) as signed 64-bit integers -- equal keys stay in run
 * order and, within a run, in their original order -- and encoded again.  In
 * a group with two or more runs every run must be non-decreasing in
 * (start, stop), as sort-bed writes it: a violation is STARCH_ERR_DATA and
 * starch_last_error names the input number (from 0), the chromosome and the
 * line (from 1, counting that stream's BED lines) of the first offending
 * line of the lowest offending run.  A single-run group that is re-encoded
 * only for its level or base counts keeps its order unchecked.  The result is
 * byte for byte the archive starch_encode_host writes for the merged BED
 * under the same options.
 * opt: emit_index must be 1, reference_compat 0 and compression_method
 * STARCH_METHOD_BZIP2 (NULL: the defaults); anything else, narch == 0 or an
 * input whose index says compressionFormat "gzip" is STARCH_ERR_ARG; a blob
 * that is not an archive is STARCH_ERR_DATA, as starch_archive_index has it. */
typedef struct {
    uint64_t name_off, name_len;   /* the chromosome, in `names` */
    uint64_t first_run;            /* its runs: runs[first_run, first_run + n_runs) */
    uint32_t n_runs;
    uint32_t merge;                /* 0 copy, 1 decode + encode */
    uint64_t lines, text_bytes;    /* sums over the runs, from the indexes */
} starch_cat_group;
typedef struct {
    uint32_t input, entry;         /* index entry `entry` of archive `input` */
} starch_cat_run;
/* The plan alone (host only: no context, no GPU): the groups in output order.
 * groups, runs and names all NULL: the three counts alone; STARCH_ERR_MEM
 * when a capacity is short (the counts are still set). */
int starch_cat_plan(const void* const* archives, const uint64_t* lens, uint64_t narch, const starch_options* opt,
                    starch_cat_group* groups, uint64_t gcap, uint64_t* ngroups, starch_cat_run* runs, uint64_t rcap,
                    uint64_t* nruns, char* names, uint64_t names_cap, uint64_t* names_len);
typedef struct {
    uint64_t streams_in;       /* index entries over all inputs */
    uint64_t streams_copied;   /* groups copied */
    uint64_t groups_merged;    /* groups decoded and encoded again */
    uint64_t runs_decoded;     /* their runs */
    uint64_t lines_merged;     /* BED lines of the merged groups */
    uint64_t bytes_copied;     /* stream bytes carried over */
    uint64_t bytes_decoded;    /* stream bytes decoded */
} starch_cat_stats;
/* The merged archive in *out (host memory; free with starch_free).  What is
 * copied is decided by starch_cat_plan and nothing else.  Merge groups go
 * through the GPU in batches, in output order: a batch takes groups while the
 * sum of their transformedBytes stays within 1 GiB (environment variable
 * STARCH_CAT_BATCH_BYTES overrides it), and always at least one; a batch of
 * 2^32 lines or more, or one whose buffers cannot be allocated, is
 * STARCH_ERR_MEM naming its first chromosome.  ctx may be NULL: a plan
 * without a merge group completes on the host alone, one with a merge group
 * is STARCH_ERR_ARG.  With a context, a plan without a merge group launches
 * nothing and leaves the context's results as they were.  When a merge group
 * runs, the call overwrites the decode and encode buffers: starch_output_* and
 * the encode accessors (starch_archive_*, starch_streams_*, starch_segment*)
 * report STARCH_ERR_STATE afterwards, as after a failed call, and
 * starch_get_stats holds the last batch's encode; the extract stats
 * (starch_extract_get_stats) are left untouched. */
int starch_cat_host(starch_ctx* ctx, const void* const* archives, const uint64_t* lens, uint64_t narch,
                    const starch_options* opt, void** out, uint64_t* out_len);
/* Of the last successful starch_cat_host on this context. */
int starch_cat_get_stats(starch_ctx* ctx, starch_cat_stats* out);

/* ---- sort-bed: BED lines into the order every other entry point expects ------
 * Input is BED as bytes, cut into lines at '\n'; a last line without '\n' is a
 * line, and every output line ends in '\n'.  A line is chrom TAB start TAB stop,
 * optionally TAB rest: chrom is one or more bytes that are neither TAB nor
 * '\n'; start and stop are 1 to 19 ASCII digits each with a value of at most
 * 2^63-1 (leading zeros stay in the bytes and do not count in the value).  The
 * output (starch_output_size / _copy / _device) is the same lines, byte for
 * byte, ordered by chrom (unsigned memcmp, a proper prefix first: the order of
 * starch_cat_host's groups), then start, then stop, both as numbers; lines
 * equal in all three keep their input order (starch_cat_host's rule for
 * ties; BEDOPS sort-bed orders such lines by the rest of the line instead).
 * Any other line -- an empty one, fewer than three fields, a non-digit or no
 * digit in a coordinate (so also the '\r' of a CRLF BED3 file), 20 or more
 * digits or a value above 2^63-1, a line that starts with '#' or is a `track`
 * header -- is STARCH_ERR_DATA: starch_last_error names the number (from 1) of
 * the first such line and what is wrong with it, and there is no output.
 * n == 0 gives an empty output.  2^32 lines or more in one call is
 * STARCH_ERR_ARG.  An input already in order is copied (plus a final '\n' if
 * it lacks one) and not sorted. */
int starch_sort_host(starch_ctx* ctx, const void* bed, uint64_t n);
int starch_sort_device(starch_ctx* ctx, const void* d_bed, uint64_t n);   /* BED bytes in HBM */
typedef struct {
    uint64_t input_bytes, n_lines, n_chromosomes;
    uint64_t already_sorted;        /* 1: the input was in order */
    uint64_t first_unsorted_line;   /* 1-based, 0: none: the first line whose key is below its predecessor's */
    uint32_t radix_passes;          /* key bytes that differ between lines (of 20) */
    float ms_parse, ms_rank, ms_sort, ms_gather, ms_total;
} starch_sort_stats;
/* Of the last successful starch_sort_* call on this context. */
int starch_sort_get_stats(starch_ctx* ctx, starch_sort_stats* out);
/* The order check alone (parse, chromosome ranks, one comparison pass): no
 * output is written and the context's output is left as it was. */
int starch_sort_check_host(starch_ctx* ctx, const void* bed, uint64_t n, uint64_t* first_unsorted_line);
/* starch_sort_host, then starch_encode_device of the sorted bytes while they
 * are in HBM: the archive is read as after starch_encode_host, and the sorted
 * BED stays readable through starch_output_*. */
int starch_sort_encode_host(starch_ctx* ctx, const void* bed, uint64_t n, const starch_options* opt);
/* Sizes the sort's kernels switch on: lines per radix tile, and the length
 * (with its '\n') from which an output line is copied by a whole wave. */
int starch_sort_constants(uint32_t* tile_lines, uint32_t* wave_copy_bytes);

/* ---- bedops: merge, intersect, difference, symmdiff, complement ---------------
 * The inputs are ninputs >= 1 sorted BED inputs, numbered from 0 in argument
 * order.  A line is what starch_sort_host accepts, and stop > start is also
 * required; columns after the third are ignored; a last line without '\n' is a
 * line; an empty input is valid and covers nothing.  S_k is the set of
 * (chrom, base) pairs covered by input k: base x is covered by a line when
 * start <= x < stop.  The result set R is
 *   merge        the union of all S_k;
 *   intersect    the intersection of all S_k;
 *   difference   S_0 minus the union of S_1 .. S_{N-1};
 *   symmdiff     the bases that lie in exactly one S_k;
 *   complement   per chromosome, the bases outside the union that lie between
 *                that chromosome's smallest start and its largest stop over all
 *                inputs (nothing is known about chromosome lengths).
 * With one input, merge, intersect, difference and symmdiff all give that input
 * merged.  The output (starch_output_size / _copy / _device) is BED3, chrom TAB
 * start TAB stop '\n' in plain decimal: one line for each maximal run of
 * consecutive bases of R on a chromosome, so abutting pieces are joined
 * ([0,10) and [10,20) become 0 20, wherever they came from); chromosomes in
 * starch_sort_host's order, lines within one by start.  It is itself valid
 * input for starch_encode_*, starch_sort_check_host and this call.
 * This is a definition by sets: it is believed to match BEDOPS' bedops for
 * these five options, but that is unverified against a BEDOPS binary.
 * Errors leave no output; starch_last_error names the input (from 0) and the
 * line (from 1, counted within that input; for an archive, its decoded BED
 * lines).  In this order: a malformed line, kinds and texts as in
 * starch_sort_host, is STARCH_ERR_DATA (the lowest (input, line)); then the
 * lowest (input, line) that has stop <= start, or whose key (chrom, start,
 * stop) is below the previous line of the same input, is STARCH_ERR_DATA, and
 * the text says which (the first line of an input is never compared with the
 * last line of the input before it); 2^31 lines or more over all inputs is
 * STARCH_ERR_ARG (every line gives two ends, indexed with 32 bits).
 * ninputs == 0, an unknown op or a NULL context or array is STARCH_ERR_ARG,
 * answered before anything touches a device.
 * An input whose first four bytes are the archive magic ca 5c ad 1a is an
 * archive of this library: its streams are decoded and inverse-transformed on
 * the GPU, as in starch_unstarch_host, and the BED stays in HBM; a gzip-method
 * archive is STARCH_ERR_ARG, as in starch_extract_host. */
#define STARCH_SETOP_MERGE 0
#define STARCH_SETOP_INTERSECT 1
#define STARCH_SETOP_DIFFERENCE 2
#define STARCH_SETOP_SYMMDIFF 3
#define STARCH_SETOP_COMPLEMENT 4
typedef struct {
    const void* data;   /* BED text or an archive */
    uint64_t len;
} starch_setop_input;
int starch_setop_host(starch_ctx* ctx, int op, const starch_setop_input* inputs, uint64_t ninputs);
/* BED text only, the inputs back to back in HBM: input k is
 * d_bed[offs[k], offs[k + 1]) (offs: ninputs + 1 host values, not decreasing). */
int starch_setop_device(starch_ctx* ctx, int op, const void* d_bed, const uint64_t* offs, uint64_t ninputs);
typedef struct {
    uint64_t n_inputs, input_bytes, n_lines, n_chromosomes;
    uint64_t runs_merged;      /* intervals left after the per-input merge, over all inputs */
    uint64_t groups;           /* distinct (chromosome, position) among their ends */
    uint64_t lines_out, output_bytes;
    uint64_t archives_decoded;
    uint32_t radix_passes;
    /* ms_decode (upload and archive decode) and ms_total are host clock, the others GPU events */
    float ms_decode, ms_parse, ms_merge, ms_sort, ms_sweep, ms_format, ms_total;
} starch_setop_stats;
/* Of the last successful starch_setop_* call on this context. */
int starch_setop_get_stats(starch_ctx* ctx, starch_setop_stats* out);
/* Lines per tile of the segmented max-scan (where its carry crosses). */
int starch_setop_constants(uint32_t* scan_tile_lines);

/* ---- bedops: element-of, not-element-of, partition, chop, everything ------------
 * starch_bedops_host / _device take every operation of the bedops command: ops 0
 * to 4 behave exactly as through starch_setop_*, and five more are defined here.
 * Inputs, line validity, errors and their order, archive inputs and the limit of
 * 2^31 lines are those of starch_setop_host: stop > start, each input in
 * starch_sort_host's order, error texts that name the input from 0 and the line
 * from 1.  A last line without '\n' is a line, and wherever it is echoed it gets
 * a '\n'.  These are definitions by sets: they are believed to match BEDOPS'
 * bedops for --everything, --element-of, --not-element-of, --partition and
 * --chop, but that is unverified against a BEDOPS binary.
 *   everything   Every line of every input, all of its columns, ordered by
 *                (chromosome bytewise, start, stop) as numbers; ties by (input
 *                number, line number).  For valid inputs this is what
 *                starch_sort_host gives for the inputs one after the other.
 *   element-of, not-element-of
 *                They take a threshold and at least two inputs (fewer is
 *                STARCH_ERR_ARG before a device is touched).  U is the set of
 *                maximal runs of the union of inputs 1 .. N-1; abutting runs are
 *                joined, as merge joins them.  For a line (c, s, e) of input 0, ov
 *                is the largest min(b, e) - max(a, s) over the runs [a, b) of U on
 *                c, 0 if none overlaps: deliberately the largest overlap with one
 *                run, not the total over several.  With a threshold in bases t
 *                (t >= 1) the line is selected when ov >= t; with a threshold in
 *                percent p (1 .. 100) when ov * 100 >= p * (e - s), exact for every
 *                64-bit length.  element-of writes the selected lines of input 0,
 *                whole, in input order; not-element-of writes the others.  The
 *                commands' default threshold is 100%.
 *   partition    All lines of all inputs together, not merged.  Per chromosome, P
 *                is the sorted set of distinct starts and stops; for consecutive
 *                p, q of P, BED3 `c p q` is written when at least one line covers
 *                [p, q).  Pieces are never joined, and a piece is written once
 *                however many lines cover it.
 *   chop         A width w >= 1, a stagger g >= 1 and an exclude flag.  U is the
 *                merge of all inputs.  For a run [a, b) of U and k = 0, 1, ...
 *                while a + k*g < b, the piece [a + k*g, min(a + k*g + w, b)) is
 *                written as BED3, in k order; with the flag, pieces shorter than w
 *                are left out.  Nothing wraps for coordinates up to 2^63-1.  A
 *                result of 2^32 pieces or more, or of 2^40 bytes or more, is
 *                refused: STARCH_ERR_ARG, "result too large", answered from the
 *                scanned counts before the pieces (or, for the bytes, the
 *                output) are allocated.
 * partition and chop write BED3 as the first five ops do, in starch_sort_host's
 * order.  A threshold of 0 bases or a percent outside 1 .. 100, chop == 0, an
 * unknown op, ninputs == 0 and a NULL pointer are STARCH_ERR_ARG, answered
 * before anything touches a device. */
#define STARCH_SETOP_ELEMENT_OF 5
#define STARCH_SETOP_NOT_ELEMENT_OF 6
#define STARCH_SETOP_PARTITION 7
#define STARCH_SETOP_CHOP 8
#define STARCH_SETOP_EVERYTHING 9
typedef struct {
    int32_t op;                      /* STARCH_SETOP_*, 0 to 9 */
    uint64_t threshold;              /* element-of, not-element-of */
    uint32_t threshold_is_percent;   /* threshold counts percent, not bases */
    uint64_t chop;                   /* chop: the width w */
    uint64_t stagger;                /* chop: g; 0 means equal to chop */
    uint32_t exclude_short;          /* chop: leave out pieces shorter than w */
} starch_bedops_options;             /* 48 bytes, every field naturally aligned */
/* Fields that the op does not use are not looked at. */
int starch_bedops_host(starch_ctx* ctx, const starch_bedops_options* opt, const starch_setop_input* inputs, uint64_t ninputs);
int starch_bedops_device(starch_ctx* ctx, const starch_bedops_options* opt, const void* d_bed, const uint64_t* offs,
                         uint64_t ninputs);
/* starch_setop_get_stats reports the last call through starch_setop_* or
 * starch_bedops_*: the fields that have a meaning for the op (runs_merged: the
 * runs of U for element-of, not-element-of and chop; groups: partition, chop)
 * and the rest 0. */
/* Sizes the new kernels switch on: runs per tile of element-of's range maximum,
 * and pieces per workgroup of chop's expansion (also the largest window of runs
 * it stages in LDS). */
int starch_bedops_constants(uint32_t* rmq_tile, uint32_t* expand_tile);

/* ---- bedmap: count and bases of map elements over reference intervals ----------
 * Two sorted BED inputs: the reference is input 0, the map input 1; with no map
 * the reference is mapped onto itself.  A line is what starch_setop_host
 * accepts: stop > start is required, and each input must be in
 * starch_sort_host's order; a last line without '\n' is a line; an empty input
 * is valid.  Either input may be a bzip2-method archive, recognised by its
 * magic and decoded on the GPU (a gzip-method archive is STARCH_ERR_ARG).
 * For a reference line (c, s, e) and range r the window is [s', e') =
 * [max(0, s - r), e + r) on c (e + r stops at 2^64-1).  A map line (c, a, b)
 * overlaps it when a < e' and b > s': BEDOPS' default of 1 bp of overlap.  The
 * columns:
 *   ECHO           the reference line's bytes, every column, without its '\n';
 *   COUNT          the number of overlapping map lines;
 *   BASES          the sum over the overlapping map lines of
 *                  min(b, e') - max(a, s');
 *   BASES_UNIQ     the number of bases of the window that at least one map line
 *                  covers;
 *   INDICATOR      1 if COUNT > 0, else 0;
 *   ECHO_REF_SIZE  e - s (without the range).
 * The output (starch_output_size / _copy / _device) is one line per reference
 * line, in reference order: the chosen columns (1 to 8 of them) in the order
 * given, joined by delim (1 to 8 bytes; bedmap's default is "|"), then '\n'.
 * Numbers are plain decimal.  With skip_unmapped, lines whose COUNT is 0 are
 * left out.  A reference line on a chromosome the map lacks gets zeros; map
 * lines on chromosomes the reference lacks are ignored.
 * All arithmetic is unsigned 64-bit, modulo 2^64 (the sums of map coordinates
 * that BASES is taken from wrap freely): the results are exact whenever the
 * true value fits in 64 bits, so coordinates up to 2^63-1 work.
 * This is believed to match BEDOPS' bedmap for --echo, --count, --bases,
 * --bases-uniq, --indicator, --echo-ref-size, --range, --delim and
 * --skip-unmapped, but that is unverified against a BEDOPS binary.
 * Errors leave no output and have the kinds, order and naming of
 * starch_setop_host: input number from 0, line number from 1; first the lowest
 * malformed (input, line), then the lowest with stop <= start or below its
 * predecessor, both STARCH_ERR_DATA.  2^32 lines or more over reference and map
 * (the reference twice when it is its own map) is STARCH_ERR_ARG.  A repeated
 * column, no columns or more than 8, an unknown code, an empty or over-long
 * delimiter and a NULL context, reference or options are STARCH_ERR_ARG,
 * answered before anything touches a device. */
#define STARCH_MAP_ECHO 0
#define STARCH_MAP_COUNT 1
#define STARCH_MAP_BASES 2
#define STARCH_MAP_BASES_UNIQ 3
#define STARCH_MAP_INDICATOR 4
#define STARCH_MAP_ECHO_REF_SIZE 5
typedef struct {
    uint32_t ncols;          /* 1 to 8 */
    uint8_t cols[8];         /* STARCH_MAP_*, none twice */
    uint64_t range;
    uint32_t skip_unmapped;
    uint32_t delim_len;      /* 1 to 8 */
    char delim[8];
} starch_map_options;
/* map_or_null == NULL: the reference is its own map. */
int starch_map_host(starch_ctx* ctx, const starch_setop_input* ref, const starch_setop_input* map_or_null,
                    const starch_map_options* opt);
/* BED text only, back to back in HBM: the reference is d_bed[offs[0], offs[1]),
 * the map d_bed[offs[1], offs[2]); ninputs is 1 (no map) or 2. */
int starch_map_device(starch_ctx* ctx, const void* d_bed, const uint64_t* offs, uint64_t ninputs,
                      const starch_map_options* opt);
typedef struct {
    uint64_t n_ref, n_map;     /* lines; n_map == n_ref when there is no map */
    uint64_t n_chromosomes;    /* over both inputs */
    uint64_t map_runs_merged;  /* disjoint runs of the map (0 unless BASES_UNIQ is asked for) */
    uint64_t stops_sorted;     /* 1: a map line is nested in another, so the stops were sorted */
    uint64_t lines_out, output_bytes;
    /* ms_decode (upload and archive decode) and ms_total are host clock, the others GPU events */
    float ms_decode, ms_parse, ms_build, ms_query, ms_format, ms_total;
} starch_map_stats;
/* Of the last successful starch_map_* call on this context. */
int starch_map_get_stats(starch_ctx* ctx, starch_map_stats* out);
/* Sizes the kernels switch on: reference lines per query workgroup (a window
 * into the map arrays is found once per workgroup and chromosome), and the
 * largest window, in elements, that is staged in LDS (0: there is no such path). */
int starch_map_constants(uint32_t* tile_refs, uint32_t* lds_window);

/* ---- closest-features: nearest query elements left and right ---------------------
 * Two sorted BED inputs, both required: the reference is input 0, the query
 * input 1.  Line validity, archive inputs and errors with their kinds, order and
 * naming are those of starch_map_host: stop > start, each input in
 * starch_sort_host's order, a last line without '\n' is a line, an empty input
 * is valid, a bzip2-method archive is decoded in HBM and a gzip-method archive is
 * STARCH_ERR_ARG.  Error texts begin "closest-features: input K, line N:".  2^32
 * lines or more over both inputs is STARCH_ERR_ARG.
 * Only lines of one chromosome relate to each other.  For a reference line
 * r = (c, s, e) and a query line q = (c, a, b):
 *   q overlaps r when a < e and b > s; then dist(q) = 0;
 *   when b <= s, dist(q) = -(s - b + 1): an abutting element to the left is at -1;
 *   when a >= e, dist(q) = a - e + 1: an abutting element to the right is at +1.
 * The left candidates are the query lines on c with (a, b) < (s, e)
 * lexicographically, as numbers; the right candidates those with
 * (a, b) >= (s, e), so a query line equal to the reference line is a right
 * candidate.  Every query line on c is a candidate on exactly one side; a left
 * candidate is never to the right of r and a right candidate never to its left.
 * With no_overlaps, overlapping lines are removed from both sides.
 *   left(r)   the left candidate with the greatest dist (the one nearest 0);
 *             ties go to the last in the query's order;
 *   right(r)  the right candidate with the least dist; ties go to the first in
 *             the query's order.
 * Either is NA when its side has no candidate; a chromosome the query lacks gives
 * NA on both sides.  With closest, the one of the two with the smaller |dist| is
 * kept, a tie goes to the left, an NA side loses to the other, and two NA give NA.
 * The output (starch_output_size / _copy / _device) is one line per reference
 * line, in reference order, its fields joined by delim (1 to 8 bytes;
 * closest-features' default is "|"), then '\n':
 *   the reference line, every column, without its '\n', unless no_ref is set;
 *   the left element: the query line's bytes, every column, or NA;
 *   with dist, the left element's distance as a signed decimal (-12, 0, 7), or NA;
 *   the same two fields for the right element.
 * With closest there is one element and one distance instead of two.  Distances
 * are exact for coordinates up to 2^63-1.
 * This is a definition by sets, modelled on BEDOPS' closest-features for
 * --closest, --dist, --no-overlaps, --no-ref and --delim, but it is unverified
 * against a BEDOPS binary.
 * Errors leave no output.  A NULL context, input or options, an empty or
 * over-long delimiter and a flag other than 0 or 1 are STARCH_ERR_ARG, answered
 * before anything touches a device. */
typedef struct {
    uint32_t closest;        /* 0 or 1: keep the nearer of left and right */
    uint32_t dist;           /* 0 or 1: a distance field after every element */
    uint32_t no_overlaps;    /* 0 or 1: overlapping query lines are no candidates */
    uint32_t no_ref;         /* 0 or 1: leave out the reference line */
    uint32_t delim_len;      /* 1 to 8 */
    char delim[8];
} starch_closest_options;
int starch_closest_host(starch_ctx* ctx, const starch_setop_input* ref, const starch_setop_input* query,
                        const starch_closest_options* opt);
/* BED text only, back to back in HBM: the reference is d_bed[offs[0], offs[1]),
 * the query d_bed[offs[1], offs[2]) (offs: three host values, not decreasing). */
int starch_closest_device(starch_ctx* ctx, const void* d_bed, const uint64_t* offs, const starch_closest_options* opt);
typedef struct {
    uint64_t n_ref, n_query;   /* lines */
    uint64_t n_chromosomes;    /* over both inputs */
    uint64_t stops_sorted;     /* 1: a query line is nested in another (with no_overlaps the stops were then sorted) */
    uint64_t left_na, right_na;   /* reference lines without a left / right element, before closest chooses */
    uint64_t lines_out, output_bytes;
    /* ms_decode (upload and archive decode) and ms_total are host clock, the others GPU events */
    float ms_decode, ms_parse, ms_build, ms_query, ms_format, ms_total;
} starch_closest_stats;
/* Of the last successful starch_closest_* call on this context. */
int starch_closest_get_stats(starch_ctx* ctx, starch_closest_stats* out);
/* Sizes the kernels switch on: reference lines per query workgroup, and the
 * fan-out of the hierarchy of maxima over the query stops (stops per tile, and
 * tiles per tile of the level above). */
int starch_closest_constants(uint32_t* tile_refs, uint32_t* fanout);

/* ---- bedmap-elements: the map lines that overlap each reference line ------------
 * bedmap's sibling for everything that needs the overlapping map lines one by
 * one: the --echo-map columns and the overlap criteria other than one base.
 * Inputs, line validity, archive inputs, the reference as its own map (no map
 * given) and errors with their kinds, order and naming are those of
 * starch_map_host.  Error texts begin "bedmap-elements: input K, line N:".
 * For a reference line (c, s, e) and range r the window is [s', e') =
 * [max(0, s - r), e + r) on c (e + r stops at 2^64-1).  For a map line (c, a, b)
 * ov = min(b, e') - max(a, s'); the line is a candidate when a < e' and b > s'.
 * Criterion: exactly one (BEDOPS: at most one overlap option; the commands'
 * default is BP_OVR with n = 1).  A candidate is a hit when
 *   BP_OVR n (n >= 1)   ov >= n;
 *   RANGE r             always (the only criterion with r > 0);
 *   FRACTION_REF f      ov / (e - s) >= f;
 *   FRACTION_MAP f      ov / (b - a) >= f;
 *   FRACTION_BOTH f     both of the two above;
 *   FRACTION_EITHER f   either of them;
 *   EXACT               a == s and b == e.
 * f is an exact decimal, frac_num / 10^frac_digits with frac_digits 0 to 9 and
 * 0 < f <= 1; the test is ov * 10^frac_digits >= frac_num * len in 128-bit
 * unsigned arithmetic, with no floating point anywhere.  The fields of a
 * criterion that is not the chosen one must be 0 (n, range, frac_num,
 * frac_digits): a second criterion, like n == 0 under BP_OVR, a fraction outside
 * (0, 1] or an unknown code, is STARCH_ERR_ARG.
 * Per-line columns:
 *   ECHO, COUNT (the number of hits), INDICATOR, ECHO_REF_SIZE as in bedmap;
 *   ECHO_REF_NAME     chrom:start-stop of the reference line;
 *   ECHO_REF_ROW_ID   id-N, N the reference line's number from 1.
 * Per-hit list columns: the hits' values in map order, joined by multidelim (1
 * to 8 bytes; the command's default is ";"), empty when there is no hit:
 *   ECHO_MAP            the whole map line, without its '\n';
 *   ECHO_MAP_ID         its column 4, byte for byte;
 *   ECHO_MAP_SCORE      its column 5, byte for byte;
 *   ECHO_MAP_SIZE       b - a, in decimal;
 *   ECHO_OVERLAP_SIZE   ov, in decimal.
 * ECHO_MAP_RANGE is no list: one BED3 `chrom TAB min a TAB max b` over the hits.
 * A hit that lacks the column ECHO_MAP_ID or ECHO_MAP_SCORE asks for (columns
 * are separated by TAB; an empty column is there) is STARCH_ERR_DATA naming
 * input 1 (0 when the reference is its own map) and the lowest such map line
 * that is a hit of some reference line; map lines that are never hits are not
 * checked.
 * The output is one line per reference line, in reference order: 1 to 12
 * columns, none twice, in the order given, joined by delim (1 to 8 bytes,
 * default "|"), then '\n'.  With skip_unmapped, lines with no hit are left out.
 * 2^32 hits or more in all, or 2^40 output bytes or more, is STARCH_ERR_ARG,
 * "result too large", answered from the scanned counts before the hit list (or,
 * for the bytes, the output) is allocated.
 * This is a definition by sets, modelled on BEDOPS' bedmap for the options
 * named, but it is unverified against a BEDOPS binary.  Known differences:
 * scores are copied, not reformatted; there is no --echo-map-id-uniq;
 * ECHO_MAP_RANGE is empty when there are no hits.
 * A repeated column, no columns or more than 12, an unknown code, an empty or
 * over-long delimiter or multi-delimiter and a NULL context, reference or
 * options are STARCH_ERR_ARG, answered before anything touches a device. */
#define STARCH_MAPEL_ECHO 0
#define STARCH_MAPEL_COUNT 1
#define STARCH_MAPEL_INDICATOR 2
#define STARCH_MAPEL_ECHO_REF_SIZE 3
#define STARCH_MAPEL_ECHO_REF_NAME 4
#define STARCH_MAPEL_ECHO_REF_ROW_ID 5
#define STARCH_MAPEL_ECHO_MAP 6
#define STARCH_MAPEL_ECHO_MAP_ID 7
#define STARCH_MAPEL_ECHO_MAP_SCORE 8
#define STARCH_MAPEL_ECHO_MAP_SIZE 9
#define STARCH_MAPEL_ECHO_OVERLAP_SIZE 10
#define STARCH_MAPEL_ECHO_MAP_RANGE 11
#define STARCH_MAPEL_CRIT_BP_OVR 0
#define STARCH_MAPEL_CRIT_RANGE 1
#define STARCH_MAPEL_CRIT_FRACTION_REF 2
#define STARCH_MAPEL_CRIT_FRACTION_MAP 3
#define STARCH_MAPEL_CRIT_FRACTION_BOTH 4
#define STARCH_MAPEL_CRIT_FRACTION_EITHER 5
#define STARCH_MAPEL_CRIT_EXACT 6
typedef struct {
    uint32_t ncols;          /* 1 to 12 */
    uint8_t cols[12];        /* STARCH_MAPEL_*, none twice */
    uint32_t criterion;      /* STARCH_MAPEL_CRIT_* */
    uint32_t frac_digits;    /* FRACTION_*: 0 to 9 */
    uint64_t n;              /* BP_OVR: 1 or more */
    uint64_t range;          /* RANGE */
    uint64_t frac_num;       /* FRACTION_*: f = frac_num / 10^frac_digits */
    uint32_t skip_unmapped;
    uint32_t delim_len;      /* 1 to 8 */
    uint32_t multidelim_len; /* 1 to 8 */
    char delim[8];
    char multidelim[8];
} starch_mapel_options;      /* 80 bytes, every field naturally aligned */
/* map_or_null == NULL: the reference is its own map. */
int starch_mapel_host(starch_ctx* ctx, const starch_setop_input* ref, const starch_setop_input* map_or_null,
                      const starch_mapel_options* opt);
/* BED text only, back to back in HBM: the reference is d_bed[offs[0], offs[1]),
 * the map d_bed[offs[1], offs[2]); ninputs is 1 (no map) or 2. */
int starch_mapel_device(starch_ctx* ctx, const void* d_bed, const uint64_t* offs, uint64_t ninputs,
                        const starch_mapel_options* opt);
typedef struct {
    uint64_t n_ref, n_map;     /* lines; n_map == n_ref when there is no map */
    uint64_t n_chromosomes;    /* over both inputs */
    uint64_t hits;             /* over all reference lines */
    uint64_t heavy_lines;      /* reference lines whose run of candidates was tested by a whole wave */
    uint64_t walk_steps;       /* probes of the binary searches and of the hierarchy while the hits were counted */
    uint64_t lines_out, output_bytes;
    /* ms_decode (upload and archive decode) and ms_total are host clock, the others GPU events */
    float ms_decode, ms_parse, ms_build, ms_query, ms_format, ms_total;
} starch_mapel_stats;
/* Of the last successful starch_mapel_* call on this context. */
int starch_mapel_get_stats(starch_ctx* ctx, starch_mapel_stats* out);
/* Sizes the kernels switch on: reference lines per workgroup of the passes that
 * find the hits; the fan-out of the hierarchy of maxima over the map stops;
 * heavy_threshold: a reference line takes the whole-wave path when the run of
 * its candidates that start inside the window has that many lines or more; and
 * the bound on walk_steps: at most steps_per_hit_bound for every reference line
 * plus as many for every candidate that starts before the window (each of
 * these is a hit under BP_OVR and RANGE), whatever lies between them. */
int starch_mapel_constants(uint32_t* tile_refs, uint32_t* fanout, uint32_t* heavy_threshold, uint32_t* steps_per_hit_bound);

/* ---- bedmap-scores: statistics of the scores of the hits of each reference line ----
 * bedmap-elements' sibling for the score operations.  Inputs, line validity,
 * archive inputs, the reference as its own map (no map given), the window, the
 * candidates, the seven criteria (STARCH_MAPEL_CRIT_*, the same codes and the
 * same rule that the fields of the criteria not chosen are 0) and errors with
 * their kinds, order and naming are those of starch_mapel_host.  Error texts
 * begin "bedmap-scores: input K, line N:".  The hits of a reference line are
 * in map order.  2^32 hits or more in all, or 2^40 output bytes or more, is
 * STARCH_ERR_ARG, "result too large", answered from the scanned counts before
 * the hit list (or, for the bytes, the output) is allocated.
 * Score.  The score of a hit is column 5 of its map line (columns are
 * separated by TAB), the whole of it:
 *   [+-]? D{1,9} ( '.' D{0,9} )?    or    [+-]? '.' D{1,9}
 * at most 9 digits before the point and at most 9 after it, no exponent, no
 * inf or nan, no spaces.  Its value is that exact decimal, held as a signed
 * 64-bit count of 10^-9 units of magnitude below 10^18.  When a column from SUM
 * on is asked for, a hit whose line has no column 5, or one outside this
 * grammar, is STARCH_ERR_DATA naming input 1 (0 when the reference is its own
 * map) and the lowest such map line that is a hit of some reference line; map
 * lines that are never hits are not checked.  There is no floating point
 * anywhere: every value below is an exact rational.
 * Columns, for a reference line with the hits' scores v_1..v_n in map order and
 * w_1 <= .. <= w_n the same values ascending:
 *   ECHO         the reference line;
 *   COUNT        n;
 *   INDICATOR    1 or 0;
 *   SUM          v_1 + .. + v_n;
 *   MEAN         SUM / n;
 *   MIN, MAX     the least and the greatest v_i;
 *   MEDIAN       w_((n+1)/2) for odd n, (w_(n/2) + w_(n/2+1)) / 2 for even n;
 *   KTH          w_k with k = ceil(f * n); f = kth_num / 10^kth_digits is an
 *                exact decimal with kth_digits 0 to 9 and 0 < f <= 1, like the
 *                fractions of bedmap-elements; kth_num and kth_digits must be 0
 *                when KTH is no column;
 *   MIN_ELEMENT  the whole map line, without its '\n', of the hit with the
 *                least score; among equal scores the first in map order;
 *   MAX_ELEMENT  the same for the greatest score.
 * With n = 0 the columns from SUM on are the three bytes NAN.  SUM to KTH are
 * written with prec decimals, prec 0 to 9 (the command's default is 6): for a
 * value x let m be the integer nearest to x * 10^prec, ties to even; the
 * output is '-' if m < 0, the decimal digits of |m| div 10^prec (at least 0)
 * and, if prec > 0, '.' and exactly prec digits.  A value that rounds to zero
 * carries no sign.  (A sum has magnitude below 2^32 * 10^18 < 2^92 units and is
 * kept in 128 bits; the mean's denominator n * 10^(9-prec) is below 2^62.)
 * The output is one line per reference line, in reference order: 1 to 12
 * columns, none twice, in the order given, joined by delim (1 to 8 bytes,
 * default "|"), then '\n'.  With skip_unmapped, lines with no hit are left out.
 * This is a definition by sets, modelled on BEDOPS' bedmap for the options
 * named, but it is unverified against a BEDOPS binary.  Known differences:
 * scores are exact decimals, not strtod doubles, so an exponent form or more
 * than 9+9 digits is a data error; rounding is exact on the rational, ties to
 * even, not printf of a double; there is no negative zero; element ties go to
 * map order; KTH is defined as above; --stdev, --variance, --cv, --mad,
 * --tmean, --wmean and --echo-map-id-uniq are not supported (they need square
 * roots or products beyond 128 bits).
 * A NULL context, reference or options, no columns or more than 12, a column
 * twice, an unknown code, prec above 9, a bad or stray kth, a second criterion
 * and an empty or over-long delimiter are STARCH_ERR_ARG, answered before
 * anything touches a device. */
#define STARCH_MAPSC_ECHO 0
#define STARCH_MAPSC_COUNT 1
#define STARCH_MAPSC_INDICATOR 2
#define STARCH_MAPSC_SUM 3
#define STARCH_MAPSC_MEAN 4
#define STARCH_MAPSC_MIN 5
#define STARCH_MAPSC_MAX 6
#define STARCH_MAPSC_MEDIAN 7
#define STARCH_MAPSC_KTH 8
#define STARCH_MAPSC_MIN_ELEMENT 9
#define STARCH_MAPSC_MAX_ELEMENT 10
typedef struct {
    uint32_t ncols;          /* 1 to 12 */
    uint8_t cols[12];        /* STARCH_MAPSC_*, none twice */
    uint32_t criterion;      /* STARCH_MAPEL_CRIT_* */
    uint32_t frac_digits;    /* FRACTION_*: 0 to 9 */
    uint64_t n;              /* BP_OVR: 1 or more */
    uint64_t range;          /* RANGE */
    uint64_t frac_num;       /* FRACTION_*: f = frac_num / 10^frac_digits */
    uint64_t kth_num;        /* KTH: f = kth_num / 10^kth_digits */
    uint32_t kth_digits;     /* KTH: 0 to 9 */
    uint32_t prec;           /* 0 to 9 */
    uint32_t skip_unmapped;
    uint32_t delim_len;      /* 1 to 8 */
    char delim[8];
} starch_mapsc_options;      /* 80 bytes, every field naturally aligned */
/* map_or_null == NULL: the reference is its own map. */
int starch_mapsc_host(starch_ctx* ctx, const starch_setop_input* ref, const starch_setop_input* map_or_null,
                      const starch_mapsc_options* opt);
/* BED text only, back to back in HBM: the reference is d_bed[offs[0], offs[1]),
 * the map d_bed[offs[1], offs[2]); ninputs is 1 (no map) or 2. */
int starch_mapsc_device(starch_ctx* ctx, const void* d_bed, const uint64_t* offs, uint64_t ninputs,
                        const starch_mapsc_options* opt);
typedef struct {
    uint64_t n_ref, n_map;     /* lines; n_map == n_ref when there is no map */
    uint64_t n_chromosomes;    /* over both inputs */
    uint64_t hits;             /* over all reference lines */
    uint64_t straddling;       /* reference lines whose hits lie in more than one tile: combined through atomics */
    uint64_t sorted_hits;      /* MEDIAN, KTH: hits when the radix stage ran, 0 when they were in order already */
    uint64_t radix_passes;     /* of that stage */
    uint64_t lines_out, output_bytes;
    /* ms_decode (upload and archive decode) and ms_total are host clock, the others GPU events */
    float ms_decode, ms_parse, ms_build, ms_query, ms_reduce, ms_format, ms_total;
} starch_mapsc_stats;
/* Of the last successful starch_mapsc_* call on this context. */
int starch_mapsc_get_stats(starch_ctx* ctx, starch_mapsc_stats* out);
/* Sizes the kernels switch on: contiguous hits per workgroup of the segmented
 * reduction (tile t holds the hits [t * tile_hits, (t + 1) * tile_hits) of the
 * hit list), and the bytes from which an echoed line is copied by a whole
 * wave. */
int starch_mapsc_constants(uint32_t* tile_hits, uint32_t* wave_copy_threshold);

/* ---- convert2bed: GFF3, GTF, VCF and WIG to BED ----------------------------------
 * Text in one of four formats becomes BED lines, one thread per input line, and
 * unless no_sort is set the lines then go through starch_sort_device unchanged,
 * without leaving HBM.  The definitions are modelled on BEDOPS' convert2bed but
 * are unverified against a BEDOPS binary; the known differences are marked (*).
 * Framing.  The input is cut into lines at '\n'; a last line without '\n' is a
 * line; '\r' is an ordinary byte.  Fields of GFF, GTF and VCF are separated by
 * TAB.  A coordinate is 1 to 19 ASCII digits with a value up to 2^63-1, as in
 * starch_sort_host, and is written as a plain decimal number.
 * Header lines.  An empty line and a line that begins with '#' are header lines;
 * in WIG also a line whose first token is track or browser.  They are dropped,
 * or with keep_header header line K (from 0, in input order) becomes
 *   _header TAB K TAB K+1 TAB <the line>
 * which the sort then orders as a chromosome named _header.
 * Errors.  Any other line that does not fit its format is STARCH_ERR_DATA: the
 * text is "convert2bed: line N: <what is wrong>" for the lowest such line (from
 * 1), and there is no output.
 *   gff   A line that is exactly ##FASTA ends the input: it and everything after
 *         it is ignored and is no header.  A record has exactly 9 fields, a
 *         non-empty first one, field 4 the start >= 1 and field 5 the end >=
 *         start.  Output: seqid, start-1, end, ID, score, strand, source, type,
 *         phase, attributes.  ID is the value of the first ';'-separated piece
 *         of the attributes that begins with ID=, up to the next ';'; '.' when
 *         there is none or the value is empty.  (*) BEDOPS adds a
 *         zero_length_insertion=True attribute when start equals end.
 *   gtf   As gff, without the ##FASTA rule.  ID is the value inside the first
 *         gene_id "..." whose gene_id stands at the start of the attributes or
 *         directly after ';' or a space; '.' when there is none, when it has no
 *         closing quote or when the value is empty.  (*) BEDOPS refuses a record
 *         without gene_id.
 *   vcf   A record has 8 or more fields, a non-empty CHROM, POS >= 1 and
 *         non-empty REF and ALT.  start = POS-1 and stop = start + len(REF): the
 *         REF-length rule (*: BEDOPS' rule has changed between releases); a stop
 *         above 2^63-1 is an error.  With STARCH_VCF_ALL one line per record:
 *         CHROM, start, stop, ID, QUAL, REF, ALT, FILTER, INFO, and every field
 *         after INFO unchanged.  With STARCH_VCF_SNVS, _INSERTIONS or _DELETIONS,
 *         ALT is split at ',' and one line is written per allele of the class, in
 *         allele order, its ALT column holding that allele alone: an snv has
 *         len(allele) == len(REF), an insertion is longer, a deletion shorter.  A
 *         record without such an allele writes nothing; an empty allele is an
 *         error.
 *   wig   Tokens are separated by runs of spaces and TABs.  A declaration is
 *         variableStep chrom=C [span=N] or fixedStep chrom=C start=N [step=N]
 *         [span=N], keys in any order; span and step default to 1; start, step
 *         and span are 1 to 2^63-1.  A missing or empty chrom, a missing start,
 *         a repeated key and an unknown key are errors.  A data line has 1, 2 or
 *         4 tokens.  pos score (pos >= 1) is valid only under variableStep:
 *         C, pos-1, pos-1+span.  score alone is valid only under fixedStep: the
 *         k-th such line since the declaration (k from 0) gives C,
 *         start-1+k*step, start-1+k*step+span.  chrom start stop score is valid
 *         anywhere, needs stop > start and is copied with its coordinates
 *         unchanged.  Every data line is named id-N, N its number among the data
 *         lines of the input from 1 (4-token lines count towards N, not towards
 *         k).  Output: chrom, start, stop, id-N, score.  (*) The score is copied
 *         byte for byte; BEDOPS re-parses it and prints it with %f.  A data line
 *         before any declaration (but for the 4-token form), one that does not
 *         fit the declaration in force, any other token count and a coordinate
 *         that would exceed 2^63-1 are errors on that line.
 * 2^32 input lines or more, or 2^32 output lines or more, is STARCH_ERR_ARG.  A
 * NULL context or options, an unknown format or class and a class other than
 * STARCH_VCF_ALL with a format other than VCF are STARCH_ERR_ARG, answered
 * before anything touches a device. */
#define STARCH_CONVERT_GFF 0
#define STARCH_CONVERT_GTF 1
#define STARCH_CONVERT_VCF 2
#define STARCH_CONVERT_WIG 3
#define STARCH_VCF_ALL 0
#define STARCH_VCF_SNVS 1
#define STARCH_VCF_INSERTIONS 2
#define STARCH_VCF_DELETIONS 3
typedef struct {
    uint32_t format;         /* STARCH_CONVERT_* */
    uint32_t vcf_class;      /* STARCH_VCF_* */
    uint32_t keep_header;    /* header lines become _header lines */
    uint32_t no_sort;        /* leave the lines in input order */
} starch_convert_options;
/* The BED is read through starch_output_size / _copy / _device. */
int starch_convert_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_convert_options* opt);
int starch_convert_device(starch_ctx* ctx, const void* d_data, uint64_t n, const starch_convert_options* opt);
/* Convert, sort (copt->no_sort is STARCH_ERR_ARG) and encode from the sorted bytes
 * while they are in HBM, as starch_sort_encode_host chains sort and encode: the
 * archive is read as after starch_encode_host, the sorted BED through
 * starch_output_*.  sopt == NULL: the defaults. */
int starch_convert_encode_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_convert_options* copt,
                               const starch_options* sopt);
typedef struct {
    uint64_t input_bytes, input_lines;   /* every line, those after ##FASTA too */
    uint64_t header_lines, data_lines;   /* before ##FASTA; data lines: records, WIG data lines */
    uint64_t declarations;               /* WIG */
    uint64_t lines_out, output_bytes;
    uint64_t sorted;                     /* 1: the sort ran */
    /* GPU events; ms_total is host clock and holds the upload too */
    float ms_frame, ms_parse, ms_write, ms_sort, ms_total;
} starch_convert_stats;
/* Of the last successful starch_convert_* call on this context. */
int starch_convert_get_stats(starch_ctx* ctx, starch_convert_stats* out);
/* Sizes the kernels switch on: threads per block of the per-line kernels (one
 * line each), and the bytes from which a copied tail (attributes, INFO and the
 * sample columns, a kept header line) is left to a whole wave. */
int starch_convert_constants(uint32_t* block_lines, uint32_t* wave_copy_bytes);

/* ---- sam2bed, psl2bed, rmsk2bed: SAM, PSL and RepeatMasker .out to BED -------------
 * The three remaining text formats of BEDOPS' convert2bed, converted as
 * starch_convert_* converts its four: one thread per input line, then the sort
 * unless no_sort is set, without leaving HBM.  The definitions are modelled on
 * BEDOPS' convert2bed (its sam2bed, psl2bed and rmsk2bed wrappers) but are
 * unverified against a BEDOPS binary; the known or possible differences are
 * marked (*).
 * Framing.  The input is cut into lines at '\n'; a last line without '\n' is a
 * line; '\r' is an ordinary byte.  A number is 1 to 19 ASCII digits with a value
 * up to 2^63-1; a coordinate is written as a plain decimal number, every other
 * column is copied byte for byte.
 * Header lines.  An empty line is a header line in all three formats; the others
 * are named per format.  They are dropped, or with keep_header header line K
 * (from 0, in input order) becomes
 *   _header TAB K TAB K+1 TAB <the line>
 * as starch_convert_* writes it.
 * Errors.  Any other line that does not fit its format is STARCH_ERR_DATA: the
 * text is "<command>: line N: <what is wrong>" (sam2bed, psl2bed or rmsk2bed) for
 * the lowest such line (from 1), and there is no output.
 *   sam   A line that begins with '@' is a header line.  A record is
 *         TAB-separated and needs its first six fields: QNAME, FLAG, RNAME, POS,
 *         MAPQ, CIGAR.  (*) What follows CIGAR (RNEXT to QUAL and the tags) is
 *         copied byte for byte and is neither counted nor checked; BEDOPS needs
 *         eleven fields.  FLAG is a decimal number from 0 to 65535.  A record
 *         with FLAG bit 4 is unmapped: it is dropped and counted, or with
 *         all_reads written as _unmapped, 0, 1 and then the columns of any
 *         record, its RNAME, POS and CIGAR unread.  A mapped record needs an
 *         RNAME that is neither empty nor *, and POS >= 1.  CIGAR is *, or one or
 *         more pieces of a count of 1 to 9 digits and an operator of MIDNSHP=X.
 *         The reference length is the sum of the counts of M D N = X, and
 *         stop = POS-1 + max(1, reference length): *, 5S and 10I give one base, as
 *         htslib's end position does.  A stop above 2^63-1 is an error.  Output:
 *         RNAME, POS-1, stop, QNAME, FLAG, strand ('-' when FLAG has bit 16, else
 *         '+'), MAPQ, then the bytes from CIGAR to the end of the line.  reduced
 *         writes the first six columns only.  split writes one line per maximal
 *         run of M D = X operations with a positive reference length: N ends a
 *         run, with split_deletions D ends one too and is in none; I S H P
 *         consume nothing and end nothing.  Each line has the run's own start and
 *         stop and otherwise the record's columns: (*) the whole CIGAR and the
 *         plain QNAME are kept, where BEDOPS may write a per-piece name.  A record
 *         without such a run, and an unmapped one, gets its unsplit line.
 *   psl   When line 1 begins with psLayout, every line up to and including the
 *         first line that begins with ----- is a header line; without such a
 *         line that is an error at line 1.  A file that does not begin with
 *         psLayout has no such header.  A record has exactly 21 TAB-separated
 *         non-empty fields, matches to tStarts in UCSC's order.  tSize, tStart,
 *         tEnd and blockCount are numbers, tStart < tEnd, and strand is +, -, or
 *         two characters each + or -.  Output: tName, tStart, tEnd, qName,
 *         matches, strand, qSize, misMatches, repMatches, nCount, qNumInsert,
 *         qBaseInsert, tNumInsert, tBaseInsert, qStart, qEnd, tSize, blockCount,
 *         blockSizes, qStarts, tStarts.  split writes one line per block k <
 *         blockCount: [t, t + blockSizes[k]) with t = tStarts[k], or, when the
 *         strand has two characters and the second is '-', [tSize - t -
 *         blockSizes[k], tSize - t) (UCSC's reverse-strand coordinates); the other
 *         columns are the record's.  With split, blockSizes and tStarts must hold
 *         exactly blockCount comma-terminated numbers, a block of size 0, one that
 *         exceeds tSize on the reverse strand and a stop above 2^63-1 are errors;
 *         (*) without split the lists are copied unread.
 *   rmsk  Tokens are separated by runs of spaces and TABs; leading and trailing
 *         blanks are ignored.  A line without a token, or whose first token is SW
 *         or score, is a header line.  A record has 15 tokens, or 16 with the last
 *         equal to *: SW score, %div, %del, %ins, query, begin, end, (left),
 *         strand (+ or C), repeat, class/family, three repeat positions, ID.
 *         begin >= 1 and end >= begin.  Output, TAB-joined: query, begin-1, end,
 *         repeat, score, strand (C becomes -), %div, %del, %ins, (left),
 *         class/family, the three positions as written, ID, and * when present.
 *         (*) The numbers other than begin and end are copied unread.
 * 2^32 input lines or more, or 2^32 output lines or more, is STARCH_ERR_ARG.  A
 * NULL context or options, an unknown format, split_deletions without split,
 * split for rmsk, and split_deletions, all_reads or reduced for a format other
 * than sam are STARCH_ERR_ARG, answered before anything touches a device. */
#define STARCH_ALIGN_SAM 0
#define STARCH_ALIGN_PSL 1
#define STARCH_ALIGN_RMSK 2
typedef struct {
    uint32_t format;            /* STARCH_ALIGN_* */
    uint32_t split;             /* sam: a line per run; psl: a line per block */
    uint32_t split_deletions;   /* sam, with split: D ends a run too */
    uint32_t all_reads;         /* sam: unmapped records become _unmapped lines */
    uint32_t reduced;           /* sam: the first six columns only */
    uint32_t keep_header;       /* header lines become _header lines */
    uint32_t no_sort;           /* leave the lines in input order */
} starch_align_options;
/* The BED is read through starch_output_size / _copy / _device. */
int starch_align_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_align_options* opt);
int starch_align_device(starch_ctx* ctx, const void* d_data, uint64_t n, const starch_align_options* opt);
/* Convert, sort (aopt->no_sort is STARCH_ERR_ARG) and encode from the sorted bytes
 * while they are in HBM, as starch_convert_encode_host does.  sopt == NULL: the
 * defaults. */
int starch_align_encode_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_align_options* aopt,
                             const starch_options* sopt);
typedef struct {
    uint64_t input_bytes, input_lines;
    uint64_t header_lines, records;      /* records: every other line, the unmapped ones too */
    uint64_t unmapped_dropped;           /* SAM records left out for FLAG bit 4 */
    uint64_t lines_out, output_bytes;
    uint64_t sorted;                     /* 1: the sort ran */
    /* GPU events; ms_total is host clock and holds the upload too */
    float ms_frame, ms_parse, ms_write, ms_sort, ms_total;
} starch_align_stats;
/* Of the last successful starch_align_* call on this context. */
int starch_align_get_stats(starch_ctx* ctx, starch_align_stats* out);
/* Sizes the kernels switch on: threads per block of the per-line kernels (one
 * line each), and the bytes from which a copied tail (CIGAR to the end of a SAM
 * line, blockCount to the end of a PSL line, a kept header line) is left to a
 * whole wave. */
int starch_align_constants(uint32_t* block_lines, uint32_t* wave_copy_bytes);

/* ---- bam2bed: BAM records to BED, read through BGZF ---------------------------------
 * The output for a BAM file B is, byte for byte, what starch_align_* with
 * format sam and the same options writes for the SAM text of B, that is, for
 * what  samtools view -h  prints: the definition of that text follows, the
 * rules of sam2bed above then hold on it unchanged.  The compressed bytes are
 * inflated in HBM, the records are found and formatted there, and the lines go
 * on to the sort and the encoder from there.  The points that are believed but
 * unverified against samtools or BEDOPS are marked (*).
 * Input.  An input that starch_is_gzip accepts is inflated as the gzip section
 * below says (BGZF wide, generic gzip serially; its errors are those of that
 * section).  An input that begins BAM\1 is taken as already inflated.  Anything
 * else is STARCH_ERR_DATA, and so is an inflated input that does not begin
 * BAM\1.  A missing BGZF EOF marker is not an error.
 * Header.  BAM\1, l_text (u32), the text, n_ref (u32), then per reference
 * l_name (u32), the NUL-terminated name and l_ref (u32); all little-endian.  A
 * truncated header, a name that is not NUL-terminated and an l_name of 0 are
 * STARCH_ERR_DATA.  The header lines are the lines of the text with its
 * trailing NUL bytes dropped, cut at '\n'; a last line without '\n' is a line.
 * They are dropped, or with keep_header written as _header lines exactly as
 * sam2bed writes them (an empty line is a header line there too).
 * Records.  A record is block_size (u32) and then block_size bytes, with
 * block_size >= 32: refID, pos (i32), l_read_name, mapq (u8), bin, n_cigar_op,
 * flag (u16), l_seq (u32), next_refID, next_pos, tlen (i32), the read name, the
 * CIGAR (u32 each: count << 4 | operator), SEQ (4 bits a base), QUAL, the tags.
 * The record must hold what its own counts announce: 32 + l_read_name +
 * 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size.  l_read_name >= 1 and
 * the name ends in NUL.  refID and next_refID lie in [-1, n_ref).  CIGAR
 * operators are 0 to 8.  The tag area parses exactly to the record's end: a tag
 * is two bytes, a type of A c C s S i I f Z H B and its value; B is a subtype of
 * c C s S i I f, a count (u32) and the elements; Z and H end in NUL inside the
 * record.  The chain of records must end exactly at the end of the input.  Any
 * violation is STARCH_ERR_DATA with the text
 *   bam2bed: record N: <what is wrong>
 * where N counts from 1 and the lowest bad record is named; nothing is written.
 * Every record is checked, a dropped one too.
 * SAM text of a record (SAM specification section 4.2).  QNAME (the name
 * without its NUL) and FLAG as written.  RNAME is the reference name, or * for
 * -1.  POS is pos + 1, MAPQ as written.  CIGAR is counts and MIDNSHP=X, or * when
 * there are no operators.  RNEXT is * for -1, = when it equals a non-negative
 * refID, otherwise the name.  PNEXT is next_pos + 1; TLEN is signed.  SEQ comes
 * from =ACMGRSVTWYHKDBN, or * when l_seq = 0.  QUAL is each byte plus 33, or *
 * when l_seq = 0 or the first byte is 0xFF.  Each tag is TG:t:value: A as its
 * byte, all six integer types as i: and a signed decimal, Z and H as their
 * bytes, B as B:s,v,v,...  An f value is C's %g of the float32 (6 significant
 * digits, trailing zeros stripped, exponent form below 1e-4 and from 1e6 up),
 * computed exactly in integer arithmetic on mantissa and exponent, with no
 * floating-point instruction, for every bit pattern; (*) infinities and NaNs
 * print inf, -inf and nan (a NaN of either sign).  The long-CIGAR convention is
 * honoured: when n_cigar_op = 2, the first operator is <l_seq>S, the second is N
 * and a CG:B:I tag is present, the first such tag's array is the CIGAR and that
 * tag is not printed.  (*) The name and the tag values are copied as they are:
 * a TAB, a newline or a NUL inside them is not escaped.
 * Semantics.  On that text the rules of sam2bed hold: the unmapped rule and
 * all_reads; stop = POS-1 + max(1, reference length); reduced, split and
 * split_deletions; a mapped record with refID -1 (or (*) a reference whose name
 * is empty or *) or with pos < 0 is bad, in sam2bed's words.  With reduced,
 * nothing after column 6 is formatted.
 * Framing (bed_bam.hip): tile t of the framing is the bytes
 * [t * T, (t + 1) * T) of the inflated file, header included.
 * 2^32 records or more, or 2^32 output lines or more, is STARCH_ERR_ARG.  A NULL
 * context or options, split_deletions without split, and no_sort with
 * starch_bam_encode_host are STARCH_ERR_ARG, answered before anything touches a
 * device. */
typedef struct {
    uint32_t split;             /* a line per run of M D = X */
    uint32_t split_deletions;   /* with split: D ends a run too */
    uint32_t all_reads;         /* unmapped records become _unmapped lines */
    uint32_t reduced;           /* the first six columns only */
    uint32_t keep_header;       /* header lines become _header lines */
    uint32_t no_sort;           /* leave the lines in input order */
} starch_bam_options;
/* BAM bytes in host memory, compressed (BGZF, gzip) or not.  The BED is read
 * through starch_output_size / _copy / _device. */
int starch_bam_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_bam_options* opt);
/* INFLATED BAM (it begins BAM\1) in HBM. */
int starch_bam_device(starch_ctx* ctx, const void* d_data, uint64_t n, const starch_bam_options* opt);
/* Convert, sort (bopt->no_sort is STARCH_ERR_ARG) and encode from the sorted bytes
 * while they are in HBM, as starch_align_encode_host does.  sopt == NULL: the
 * defaults. */
int starch_bam_encode_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_bam_options* bopt,
                           const starch_options* sopt);
typedef struct {
    uint64_t input_bytes, inflated_bytes;
    uint64_t references, header_lines, records;   /* records: the unmapped ones too */
    uint64_t unmapped_dropped;                    /* records left out for FLAG bit 4 */
    uint64_t tiles;                               /* of the framing */
    uint64_t wave_records;                        /* records whose l_seq or largest B count reaches the wave threshold */
    uint64_t lines_out, output_bytes;
    uint64_t sorted;                              /* 1: the sort ran */
    /* GPU events (ms_frame holds the header's round trip); ms_total is host clock and holds the upload too */
    float ms_inflate, ms_frame, ms_parse, ms_write, ms_sort, ms_total;
} starch_bam_stats;
/* Of the last successful starch_bam_* call on this context. */
int starch_bam_get_stats(starch_ctx* ctx, starch_bam_stats* out);
/* Sizes the kernels switch on: the bytes T of a framing tile, the threads per
 * block of the per-record kernels (one record each), and the l_seq or B count W
 * from which a record's SEQ, QUAL and arrays are left to a whole wave. */
int starch_bam_constants(uint32_t* tile_bytes, uint32_t* block_records, uint32_t* wave_threshold);

/* ---- bigWig and bigBed files: header, chromosomes and block table (bed_bbi.hip) ------
 * The host's reading of a bigWig / bigBed file: what a converter needs before it
 * touches a block.  No context and no GPU.  Modelled on UCSC's bbiFile layout;
 * unverified against UCSC's tools: what follows is the definition.  Only
 * full-resolution data is described; zoom levels, autoSql and the total summary
 * are skipped.
 * File.  All integers are little-endian; a file whose magic reads right only
 * byte-swapped is refused ("big-endian bigWig/bigBed is not supported").  Header
 * (64 bytes): magic u32 (0x888FFC26 bigWig, 0x8789F2EB bigBed), version u16,
 * zoomLevels u16, chromosomeTreeOffset, fullDataOffset, fullIndexOffset u64,
 * fieldCount, definedFieldCount u16, autoSqlOffset, totalSummaryOffset u64,
 * uncompressBufSize u32 (0: the blocks are not compressed), reserved u64.
 * Chromosome B+ tree at chromosomeTreeOffset: magic 0x78CA8C91, blockSize,
 * keySize, valSize (8) u32, itemCount, reserved u64; nodes are isLeaf u8,
 * reserved u8, count u16 and count items: key[keySize] then chromId, chromSize
 * u32 (leaf) or childOffset u64 (inner).  Ids are exactly 0..itemCount-1, each
 * once; a name is the key up to its first zero byte, not empty, without TAB or
 * newline.  R-tree at fullIndexOffset: a 48-byte header (magic 0x2468ACE0,
 * blockSize u32, itemCount u64, four u32 bounds, endFileOffset u64, itemsPerSlot,
 * reserved u32); nodes as above with leaf items startChromIx, startBase,
 * endChromIx, endBase u32, dataOffset, dataSize u64 and inner items the same four
 * u32 and childOffset u64.  The leaf items, ordered by dataOffset, are the block
 * table: blocks lie inside [fullDataOffset, fullIndexOffset), do not overlap and
 * have fewer than 2^32 bytes.  Both trees are walked with an explicit stack;
 * every offset and count is checked against the file size before use and a node
 * reached twice is an error.  The nodes of a tree are disjoint, so the bytes of
 * the nodes a walk visits (4 + count items each) may not exceed the file size:
 * a walk ends on any input, and its time and memory are bounded by the file's
 * bytes.
 * Region.  A chromosome, whole or [start, end) with start < end, chooses the
 * blocks whose R-tree box meets it: (startChromIx, startBase) < (id, end) and
 * (endChromIx, endBase) > (id, start), compared as pairs.  A chromosome the file
 * lacks chooses none.
 * Errors.  A malformed file is STARCH_ERR_DATA with the reason  bbi: <reason> .
 * A NULL header, a kind above 2, a region without a name and a range with
 * start >= end are STARCH_ERR_ARG; a forced kind that is not the file's is
 * STARCH_ERR_DATA. */
#define STARCH_BBI_AUTO 0
#define STARCH_BBI_BIGWIG 1
#define STARCH_BBI_BIGBED 2
typedef struct {
    uint32_t kind;              /* STARCH_BBI_*: AUTO takes the magic's word */
    uint32_t region;            /* 0: everything; 1: the chromosome; 2: [start, end) of it */
    const char* chrom;          /* region: the name, chrom_len bytes */
    uint64_t chrom_len;
    uint64_t start, end;
} starch_bbi_query;
typedef struct {
    uint32_t kind, version, zoom_levels, field_count, defined_field_count, uncompress_buf_size;
    uint64_t chrom_tree_offset, full_data_offset, full_index_offset;
    uint64_t n_chroms, names_bytes;               /* names_bytes: all names, each with its NUL */
    uint64_t n_blocks;                            /* of the whole table */
    uint64_t n_selected;                          /* blocks the query's region needs (all without one) */
} starch_bbi_header;
typedef struct {
    uint32_t start_chrom, start_base, end_chrom, end_base;
    uint64_t data_offset, data_size;
} starch_bbi_block;
/* hdr is always filled on success.  chrom_sizes[0, chrom_cap) and names[0,
 * names_cap) receive the sizes by chromId and the NUL-terminated names back to
 * back; blocks[0, block_cap) the blocks q's region needs (q may be NULL: all), in
 * table order, and block_index (may be NULL) their indices in the table.  A
 * short buffer is STARCH_ERR_MEM with hdr filled; NULL buffers with capacity 0
 * only fill hdr.  STARCH_ERR_DATA leaves the reason in err[0, err_cap) (may be
 * NULL). */
int starch_bbi_info(const void* data, uint64_t n, const starch_bbi_query* q, starch_bbi_header* hdr, uint32_t* chrom_sizes,
                    uint64_t chrom_cap, char* names, uint64_t names_cap, starch_bbi_block* blocks, uint64_t* block_index,
                    uint64_t block_cap, char* err, uint64_t err_cap);
/* Adler-32 (RFC 1950: the trailer of a compressed block of such a file) of
 * data[0, n), folded from pieces of `piece` bytes (1 to 2^20), each piece summed
 * in 64 interleaved shares: the arithmetic of starch_amd/csrc/gz_adler.hpp, which
 * is written to run unchanged in a kernel, run on the host.  No context and no
 * GPU.  A NULL adler, bytes announced and none given, and a piece outside its
 * range are STARCH_ERR_ARG. */
int starch_bbi_adler32_host(const void* data, uint64_t n, uint32_t piece, uint32_t* adler);

/* ---- bigwig2bed, bigbed2bed: the blocks of a bigWig / bigBed file to BED on the GPU ----
 * (bed_bbi_dev.hip; zlib blocks through gz_inflate.hip.)  Modelled on UCSC's
 * bigWigToBedGraph / bigBedToBed, unverified against UCSC's tools: what follows,
 * which tests/bbi_oracle.py formats independently, is the definition.
 * The file is read on the host as starch_bbi_info reads it.  The blocks that the
 * query's region needs are uploaded as one range of the file, from the first of
 * them to the end of the last, and nothing else of the file is.
 * Compressed files (uncompressBufSize != 0).  A block is a zlib stream (RFC
 * 1950): CMF, FLG, raw deflate data, Adler-32 big-endian.  From the bytes, on the
 * host: at least 6 bytes, CM = 8, (CMF * 256 + FLG) % 31 = 0, FDICT clear.  On
 * the device, one wave per block with the decoder of the gzip inflater: the
 * deflate data must end exactly at the trailer, and the Adler-32 of the output
 * (folded from pieces of 4096 bytes, starch_amd/csrc/gz_adler.hpp) must equal it.
 * Every block inflates into a slot of uncompressBufSize bytes; when that is
 * above 2^20, or the slots together above 2^30 bytes, a first walk over the
 * deflate symbols sizes the slots and nothing is copied until they are known.  A
 * block that would inflate past uncompressBufSize is an error and writes nothing
 * behind its slot.
 * bigWig.  A block is one section: chromId, chromStart, chromEnd, itemStep,
 * itemSpan u32, type u8 (1 bedGraph, 2 variableStep, 3 fixedStep), reserved u8,
 * itemCount u16, then items of 12 (start, end, value), 8 (start, value) or 4
 * (value) bytes; a value is a float32.  The section's size must be 24 +
 * itemCount * item bytes, its type 1 to 3, its chromId below the chromosome
 * count.  A record's end is start + itemSpan for types 2 and 3, a type 3 start
 * is chromStart + i * itemStep; both are kept in 64 bits.  start < end for every
 * record.  A record becomes  chrom TAB start TAB end TAB value , the value as C's
 * %g of the float32, computed exactly as bam2bed computes its f tags (inf, -inf,
 * nan for a NaN of either sign).
 * bigBed.  A block is records back to back: chromId, start, end u32, then the
 * rest of the line and a zero byte.  The first zero byte at 12 bytes or more from
 * a record's start ends it; the block must end exactly on such a byte.  chromId is
 * below the chromosome count, start <= end, the rest holds no newline.  A record
 * becomes  chrom TAB start TAB end , then TAB and the rest when it is not empty.
 * Region.  With a region only records on its chromosome are written, and of a
 * range only those with start < range end and end > range start; the others are
 * dropped on the GPU.
 * Order.  Block order, then record order; sorted as sort-bed sorts unless
 * no_sort.
 * Errors.  A bad block is STARCH_ERR_DATA with  bigwig2bed: block N: <reason>
 * (bigbed2bed: for a bigBed file), N being the block's number in the file's table
 * and the lowest bad block of the stage that found one (the zlib stage runs
 * before the records are looked at); nothing is written.  A malformed header or
 * tree is starch_bbi_info's  bbi: <reason> .  2^32 records or more is
 * STARCH_ERR_ARG.  q may be NULL: the whole file, of either kind. */
int starch_bbi_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_bbi_query* q, uint32_t no_sort);
/* The same for a file in HBM.  The whole file is read back to the host, where
 * the header and the trees are walked, and the selected blocks are copied again
 * into the context's padded input buffer, as starch_gunzip_device does. */
int starch_bbi_device(starch_ctx* ctx, const void* d_data, uint64_t n, const starch_bbi_query* q, uint32_t no_sort);
/* Convert, sort and encode from the sorted bytes while they are in HBM, as
 * starch_bam_encode_host does.  sopt == NULL: the defaults. */
int starch_bbi_encode_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_bbi_query* q, const starch_options* sopt);
typedef struct {
    uint64_t input_bytes, uploaded_bytes, inflated_bytes;
    uint64_t kind, compressed;                    /* STARCH_BBI_*; 1: zlib blocks */
    uint64_t blocks;                              /* selected and converted */
    uint64_t sized;                               /* 1: the slots came from the sizing walk */
    uint64_t records;                             /* of those blocks, dropped ones too */
    uint64_t wave_records;                        /* written bigBed records whose rest reaches the wave threshold */
    uint64_t lines_out, output_bytes;
    uint64_t sorted;                              /* 1: the sort ran */
    /* GPU events; ms_total is host clock and holds the host's reading of the file too */
    float ms_upload, ms_size, ms_inflate, ms_adler, ms_frame, ms_parse, ms_write, ms_sort, ms_total;
} starch_bbi_stats;
/* Of the last successful conversion on this context. */
int starch_bbi_get_stats(starch_ctx* ctx, starch_bbi_stats* out);
/* The threads per block of the per-record kernels (one record each), the bytes
 * of a bigBed rest from which its whole wave checks and copies it, the largest
 * uncompressBufSize that sizes the slots directly, and the bytes of an Adler-32
 * piece. */
int starch_bbi_constants(uint32_t* block_records, uint32_t* wave_rest, uint32_t* modest_slot, uint32_t* adler_piece);
/* The zlib stage alone, for a compressed file: the selected blocks inflated and
 * checked as above, block k into its slot and `gap` bytes of 0xA5 left behind
 * every slot.  The slots and gaps are read through starch_output_*;
 * starch_bbi_inflate_table gives, in table order, every slot's offset there and
 * the bytes its block inflated to, and whether the zero padding behind the
 * uploaded input is still zero.  A file that is not compressed is STARCH_ERR_ARG. */
int starch_bbi_inflate_host(starch_ctx* ctx, const void* data, uint64_t n, const starch_bbi_query* q, uint32_t gap);
int starch_bbi_inflate_table(starch_ctx* ctx, uint64_t* off, uint64_t* len, uint64_t cap, uint64_t* n_blocks, uint64_t* input_pad_ok);

/* ---- gzip and BGZF inputs: inflate on the GPU (gz_inflate.hip) ----
 * An input of at least 18 bytes that begins 1f 8b 08 is gzip: one or more
 * RFC 1952 members back to back.  When every member carries the BC extra
 * subfield (bgzip's BGZF: the member's compressed size is in its header and it
 * inflates to at most 65536 bytes) the member table is made on the host from
 * the headers alone and every member is inflated by a wave of its own, all in
 * one launch.  Any other gzip file (gzip, pigz, zlib's gzip framing) is generic:
 * its members are found by a sizing launch that walks the Huffman symbols of the
 * whole chain, so a one-member file is decoded by one wave -- correct and serial.
 * CRC-32 and ISIZE of every member are checked on the GPU.  FHCRC is skipped,
 * not verified.
 *
 * Errors.  A malformed header or deflate stream, a wrong CRC-32 or ISIZE, a
 * truncated member, a BGZF member that claims more than 65536 bytes or whose
 * BSIZE reaches past the input, and bytes after the last member that do not
 * begin a member are STARCH_ERR_DATA: starch_last_error names the member's
 * number (from 0), its byte offset in the input and the reason.  Nothing is
 * published from a failed call.
 *
 * The host entry points of sort-bed, bedops, bedmap, bedmap-elements,
 * bedmap-scores, closest-features, convert2bed and sam2bed / psl2bed / rmsk2bed
 * (starch_sort_host, starch_sort_check_host, starch_sort_encode_host, every
 * starch_setop_input of the two-input calls, starch_convert_host,
 * starch_convert_encode_host, starch_align_host, starch_align_encode_host)
 * recognise a gzip input in the same way and inflate it in HBM where the text is
 * wanted; the inflated bytes are then taken as text (a gzip of an archive is
 * not unwrapped).  starch_encode_host and the stream API take their bytes as
 * they are. */
typedef struct {
    uint64_t in_off, in_len;    /* the member: header, deflate data and trailer */
    uint64_t out_off;           /* exclusive sum of isize */
    uint32_t isize, crc;        /* the trailer */
} starch_gunzip_member;
int starch_gunzip_host(starch_ctx* ctx, const void* gz, uint64_t n);
/* The same for bytes in HBM.  The whole input is read back to the host, where
 * the headers are walked, and copied again into the context's padded, aligned
 * input buffer: two trips over the host link that starch_gunzip_host does not
 * make.  For a caller whose bytes are in HBM already and small beside the text. */
int starch_gunzip_device(starch_ctx* ctx, const void* d_gz, uint64_t n);
/* The plan of a BGZF input: host only, no GPU is opened.  *n_members members,
 * the first cap of them in out (out may be NULL with cap 0); generic gzip gives
 * *is_bgzf = 0 and *n_members = 0.  STARCH_ERR_DATA as above, for what the
 * headers show; STARCH_ERR_MEM when cap is short (the count is still set). */
int starch_gunzip_plan(const void* gz, uint64_t n, starch_gunzip_member* out, uint64_t cap, uint64_t* n_members,
                       int* is_bgzf);
typedef struct {
    uint64_t members, is_bgzf;
    uint64_t stored_blocks, fixed_blocks, dynamic_blocks;
    uint64_t bytes_in, bytes_out;
    /* ms_plan is host clock; the others are GPU events (ms_size: the sizing
     * launch of generic gzip, 0 for BGZF) */
    float ms_plan, ms_upload, ms_size, ms_inflate, ms_crc;
} starch_gunzip_stats;
/* Of the last inflate on this context (the last gzip input of a BED command counts). */
int starch_gunzip_get_stats(starch_ctx* ctx, starch_gunzip_stats* out);
/* The bytes of the LDS output window, the bits of the primary decode table,
 * the bytes of a match copied per round and the most a BGZF member inflates to. */
int starch_gunzip_constants(uint32_t* window_bytes, uint32_t* primary_bits, uint32_t* copy_width, uint32_t* bgzf_max);
/* 1 for an input that the commands above take as gzip */
int starch_is_gzip(const void* data, uint64_t n);

int starch_output_size(starch_ctx* ctx, uint64_t* n);
int starch_output_copy(starch_ctx* ctx, void* dst, uint64_t cap);
int starch_output_device(starch_ctx* ctx, const void** d_ptr);

#ifdef __cplusplus
}
#endif
#endif
