"""starch_amd -- host-side (Python) mirror of the Starch operator interface.

The compute lives in ``starch_amd/_build/libstarch_amd.so`` (HIP kernels for
gfx950 behind the C ABI of ``include/starch_amd.h``).  This module only loads
that library with ctypes and marshals arguments; there is no Python or CPU
fallback: if the library or an MI355X is missing, every call raises.

Names follow the reference (alexpreynolds/starch3): ``Starch`` mirrors
``starch3::Starch`` (include/starch3api.hpp:21-584) -- ``set_note``,
``set_compression_method``, ``initialize_header_magic_bytes`` -- and
``Starch.compress(bed)`` is the whole produce_line -> consume_line ->
update_transformation_state -> process_tf_buffer -> bzip2 path.
"""
import ctypes
import json
import os

__all__ = ["Starch", "StarchError", "load", "gen_bed", "build_index", "parse_archive", "plan_units", "assign_shards",
           "archive_layout", "compress_multi", "Unit", "Segment", "Comm", "gather_host", "MAGIC", "HG38", "HG38_LEN",
           "list_archive", "cat_plan", "cat_host", "sort_constants", "setop_constants", "SETOPS",
           "map_constants", "MAPCOLS", "BEDOPS_OPS", "bedops_constants", "closest_constants",
           "mapel_constants", "mapel_fraction", "MAPEL_COLS", "MAPEL_CRITERIA", "MapelOptions", "MapelStats",
           "mapsc_constants", "MAPSC_COLS", "MapscOptions", "MapscStats",
           "convert_constants", "CONVERT_FORMATS", "VCF_CLASSES", "ConvertOptions", "ConvertStats",
           "align_constants", "ALIGN_FORMATS", "AlignOptions", "AlignStats",
           "bam_constants", "BamOptions", "BamStats",
           "bbi_info", "BBI_KINDS", "BbiQuery", "BbiHeader", "BbiBlock", "BbiStats", "bbi_constants"]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STARCH_AMD_LIB") or os.path.join(_HERE, "_build", "libstarch_amd.so")
MAGIC = b"\xca\x5c\xad\x1a"          # hpp:907-910
HG38 = [  # sort-bed order; index = chromosome id used by gen_bed
    "chr1", "chr10", "chr11", "chr12", "chr13", "chr14", "chr15", "chr16", "chr17", "chr18", "chr19",
    "chr2", "chr20", "chr21", "chr22", "chr3", "chr4", "chr5", "chr6", "chr7", "chr8", "chr9", "chrX", "chrY",
]
HG38_LEN = [  # hg38 lengths, same order (per-position input has one line per base)
    248956422, 133797422, 135086622, 133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285,
    58617616, 242193529, 64444167, 46709983, 50818468, 198295559, 190214555, 181538259, 170805979, 159345973,
    145138636, 138394717, 156040895, 57227415,
]

# compression methods (hpp:23-27)
K_BZIP2, K_GZIP, K_UNDEFINED = 0, 1, 2


class StarchError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("starch error %d: %s" % (code, msg))
        self.code = code


class Segment(ctypes.Structure):
    _fields_ = [("line_count", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64),
                ("stream_offset", ctypes.c_uint64), ("stream_bytes", ctypes.c_uint64),
                ("name_len", ctypes.c_uint64), ("n_blocks", ctypes.c_uint32),
                ("combined_crc", ctypes.c_uint32), ("unit", ctypes.c_uint64),
                ("base_count_unique", ctypes.c_int64), ("base_count_nonunique", ctypes.c_int64)]


class Unit(ctypes.Structure):
    """starch_unit: an input byte range starting a chromosome segment, with the
    sscanf values current before it (hpp:306-307, 325-342)."""
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64),
                ("init_start", ctypes.c_int64), ("init_stop", ctypes.c_int64)]


class Options(ctypes.Structure):
    _fields_ = [("block_size_100k", ctypes.c_int), ("emit_index", ctypes.c_int),
                ("reference_compat", ctypes.c_int), ("note", ctypes.c_char_p), ("base_counts", ctypes.c_int),
                ("compression_method", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("input_bytes", "n_lines", "n_segments", "text_bytes",
                                               "archive_bytes", "n_blocks", "rle_bytes", "bwt_rounds",
                                               "periodic_blocks", "bwt_tied", "dedup_blocks")] + \
               [(n, ctypes.c_float) for n in ("ms_transform", "ms_rle", "ms_bwt", "ms_mtf", "ms_tables",
                                              "ms_emit", "ms_total")]


_lib = None

# starch_host_comm (include/starch_amd.h): the gather's four primitives
_AG_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)
_SEND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int)
_RECV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int)
_END_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)


class HostComm(ctypes.Structure):
    _fields_ = [("rank", ctypes.c_int), ("world", ctypes.c_int), ("user", ctypes.c_void_p),
                ("all_gather", _AG_FN), ("send", _SEND_FN), ("recv", _RECV_FN), ("group_end", _END_FN)]


class DecStream(ctypes.Structure):
    """starch_dec_stream: one decoded bzip2 stream."""
    _fields_ = [("in_beg", ctypes.c_uint64), ("in_end", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("out_len", ctypes.c_uint64), ("level", ctypes.c_uint32), ("n_blocks", ctypes.c_uint32),
                ("combined_crc", ctypes.c_uint32)]


class Region(ctypes.Structure):
    """starch_region: a chromosome, whole or the half-open range [start, stop)."""
    _fields_ = [("chr", ctypes.c_char_p), ("chr_len", ctypes.c_uint64), ("start", ctypes.c_int64),
                ("stop", ctypes.c_int64), ("whole", ctypes.c_int)]


class ExtractStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("streams_total", "streams_decoded", "compressed_bytes_decoded",
                                               "lines_scanned", "lines_out")]


class CatGroup(ctypes.Structure):
    """starch_cat_group: one output stream of a cat plan."""
    _fields_ = [("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint64), ("first_run", ctypes.c_uint64),
                ("n_runs", ctypes.c_uint32), ("merge", ctypes.c_uint32), ("lines", ctypes.c_uint64),
                ("text_bytes", ctypes.c_uint64)]


class CatRun(ctypes.Structure):
    _fields_ = [("input", ctypes.c_uint32), ("entry", ctypes.c_uint32)]


class CatStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("streams_in", "streams_copied", "groups_merged", "runs_decoded",
                                               "lines_merged", "bytes_copied", "bytes_decoded")]


SETOPS = {"merge": 0, "intersect": 1, "difference": 2, "symmdiff": 3, "complement": 4}   # STARCH_SETOP_*
# every op of starch_bedops_host (STARCH_SETOP_*, 0 to 9)
BEDOPS_OPS = dict(SETOPS, element_of=5, not_element_of=6, partition=7, chop=8, everything=9)


class BedopsOptions(ctypes.Structure):
    """starch_bedops_options."""
    _fields_ = [("op", ctypes.c_int32), ("threshold", ctypes.c_uint64), ("threshold_is_percent", ctypes.c_uint32),
                ("chop", ctypes.c_uint64), ("stagger", ctypes.c_uint64), ("exclude_short", ctypes.c_uint32)]


class SetopInput(ctypes.Structure):
    """starch_setop_input: BED text or an archive."""
    _fields_ = [("data", ctypes.c_char_p), ("len", ctypes.c_uint64)]


class SetopStats(ctypes.Structure):
    """starch_setop_stats: the last setop()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_inputs", "input_bytes", "n_lines", "n_chromosomes", "runs_merged",
                                               "groups", "lines_out", "output_bytes", "archives_decoded")] + \
               [("radix_passes", ctypes.c_uint32)] + \
               [(n, ctypes.c_float) for n in ("ms_decode", "ms_parse", "ms_merge", "ms_sort", "ms_sweep", "ms_format",
                                              "ms_total")]


MAPCOLS = {"echo": 0, "count": 1, "bases": 2, "bases_uniq": 3, "indicator": 4, "echo_ref_size": 5}   # STARCH_MAP_*


class MapOptions(ctypes.Structure):
    """starch_map_options: the columns, range, skip_unmapped and delimiter of bedmap()."""
    _fields_ = [("ncols", ctypes.c_uint32), ("cols", ctypes.c_uint8 * 8), ("range", ctypes.c_uint64),
                ("skip_unmapped", ctypes.c_uint32), ("delim_len", ctypes.c_uint32), ("delim", ctypes.c_char * 8)]


class MapStats(ctypes.Structure):
    """starch_map_stats: the last bedmap()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_ref", "n_map", "n_chromosomes", "map_runs_merged", "stops_sorted",
                                               "lines_out", "output_bytes")] + \
               [(n, ctypes.c_float) for n in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_format", "ms_total")]


class ClosestOptions(ctypes.Structure):
    """starch_closest_options: the flags and delimiter of closest_features()."""
    _fields_ = [("closest", ctypes.c_uint32), ("dist", ctypes.c_uint32), ("no_overlaps", ctypes.c_uint32),
                ("no_ref", ctypes.c_uint32), ("delim_len", ctypes.c_uint32), ("delim", ctypes.c_char * 8)]


class ClosestStats(ctypes.Structure):
    """starch_closest_stats: the last closest_features()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_ref", "n_query", "n_chromosomes", "stops_sorted", "left_na", "right_na",
                                               "lines_out", "output_bytes")] + \
               [(n, ctypes.c_float) for n in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_format", "ms_total")]


MAPEL_COLS = {"echo": 0, "count": 1, "indicator": 2, "echo_ref_size": 3, "echo_ref_name": 4, "echo_ref_row_id": 5,
              "echo_map": 6, "echo_map_id": 7, "echo_map_score": 8, "echo_map_size": 9, "echo_overlap_size": 10,
              "echo_map_range": 11}                                               # STARCH_MAPEL_*
MAPEL_CRITERIA = {"bp_ovr": 0, "range": 1, "fraction_ref": 2, "fraction_map": 3, "fraction_both": 4,
                  "fraction_either": 5, "exact": 6}                               # STARCH_MAPEL_CRIT_*


class MapelOptions(ctypes.Structure):
    """starch_mapel_options: the columns, criterion and delimiters of map_elements()."""
    _fields_ = [("ncols", ctypes.c_uint32), ("cols", ctypes.c_uint8 * 12), ("criterion", ctypes.c_uint32),
                ("frac_digits", ctypes.c_uint32), ("n", ctypes.c_uint64), ("range", ctypes.c_uint64),
                ("frac_num", ctypes.c_uint64), ("skip_unmapped", ctypes.c_uint32), ("delim_len", ctypes.c_uint32),
                ("multidelim_len", ctypes.c_uint32), ("delim", ctypes.c_char * 8), ("multidelim", ctypes.c_char * 8)]


class MapelStats(ctypes.Structure):
    """starch_mapel_stats: the last map_elements()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_ref", "n_map", "n_chromosomes", "hits", "heavy_lines", "walk_steps",
                                               "lines_out", "output_bytes")] + \
               [(n, ctypes.c_float) for n in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_format", "ms_total")]


MAPSC_COLS = {"echo": 0, "count": 1, "indicator": 2, "sum": 3, "mean": 4, "min": 5, "max": 6, "median": 7, "kth": 8,
              "min_element": 9, "max_element": 10}                                # STARCH_MAPSC_*


class MapscOptions(ctypes.Structure):
    """starch_mapsc_options: the columns, criterion, kth, precision and delimiter of map_scores()."""
    _fields_ = [("ncols", ctypes.c_uint32), ("cols", ctypes.c_uint8 * 12), ("criterion", ctypes.c_uint32),
                ("frac_digits", ctypes.c_uint32), ("n", ctypes.c_uint64), ("range", ctypes.c_uint64),
                ("frac_num", ctypes.c_uint64), ("kth_num", ctypes.c_uint64), ("kth_digits", ctypes.c_uint32),
                ("prec", ctypes.c_uint32), ("skip_unmapped", ctypes.c_uint32), ("delim_len", ctypes.c_uint32),
                ("delim", ctypes.c_char * 8)]


class MapscStats(ctypes.Structure):
    """starch_mapsc_stats: the last map_scores()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_ref", "n_map", "n_chromosomes", "hits", "straddling", "sorted_hits",
                                               "radix_passes", "lines_out", "output_bytes")] + \
               [(n, ctypes.c_float) for n in ("ms_decode", "ms_parse", "ms_build", "ms_query", "ms_reduce", "ms_format",
                                              "ms_total")]


CONVERT_FORMATS = {"gff": 0, "gtf": 1, "vcf": 2, "wig": 3}                       # STARCH_CONVERT_*
VCF_CLASSES = {"all": 0, "snvs": 1, "insertions": 2, "deletions": 3}              # STARCH_VCF_*


class ConvertOptions(ctypes.Structure):
    """starch_convert_options: the format, VCF class and flags of convert()."""
    _fields_ = [("format", ctypes.c_uint32), ("vcf_class", ctypes.c_uint32), ("keep_header", ctypes.c_uint32),
                ("no_sort", ctypes.c_uint32)]


class ConvertStats(ctypes.Structure):
    """starch_convert_stats: the last convert()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("input_bytes", "input_lines", "header_lines", "data_lines", "declarations",
                                               "lines_out", "output_bytes", "sorted")] + \
               [(n, ctypes.c_float) for n in ("ms_frame", "ms_parse", "ms_write", "ms_sort", "ms_total")]


ALIGN_FORMATS = {"sam": 0, "psl": 1, "rmsk": 2}                                  # STARCH_ALIGN_*


class AlignOptions(ctypes.Structure):
    """starch_align_options: the format and flags of align2bed()."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("format", "split", "split_deletions", "all_reads", "reduced", "keep_header",
                                               "no_sort")]


class AlignStats(ctypes.Structure):
    """starch_align_stats: the last align2bed()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("input_bytes", "input_lines", "header_lines", "records", "unmapped_dropped",
                                               "lines_out", "output_bytes", "sorted")] + \
               [(n, ctypes.c_float) for n in ("ms_frame", "ms_parse", "ms_write", "ms_sort", "ms_total")]


class BamOptions(ctypes.Structure):
    """starch_bam_options: the flags of bam2bed()."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("split", "split_deletions", "all_reads", "reduced", "keep_header", "no_sort")]


class BamStats(ctypes.Structure):
    """starch_bam_stats: the last bam2bed()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("input_bytes", "inflated_bytes", "references", "header_lines", "records",
                                               "unmapped_dropped", "tiles", "wave_records", "lines_out", "output_bytes",
                                               "sorted")] + \
               [(n, ctypes.c_float) for n in ("ms_inflate", "ms_frame", "ms_parse", "ms_write", "ms_sort", "ms_total")]


BBI_KINDS = {"auto": 0, "bigwig": 1, "bigbed": 2}                               # STARCH_BBI_*


class BbiQuery(ctypes.Structure):
    """starch_bbi_query: the kind and region of bbi_info()."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("kind", "region")] + \
               [("chrom", ctypes.c_char_p)] + [(n, ctypes.c_uint64) for n in ("chrom_len", "start", "end")]


class BbiHeader(ctypes.Structure):
    """starch_bbi_header: what bbi_info() reads of a file's header and trees."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("kind", "version", "zoom_levels", "field_count", "defined_field_count",
                                               "uncompress_buf_size")] + \
               [(n, ctypes.c_uint64) for n in ("chrom_tree_offset", "full_data_offset", "full_index_offset", "n_chroms",
                                               "names_bytes", "n_blocks", "n_selected")]


class BbiBlock(ctypes.Structure):
    """starch_bbi_block: a leaf item of the R-tree."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("start_chrom", "start_base", "end_chrom", "end_base")] + \
               [(n, ctypes.c_uint64) for n in ("data_offset", "data_size")]


class BbiStats(ctypes.Structure):
    """starch_bbi_stats: the last bbi2bed()."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("input_bytes", "uploaded_bytes", "inflated_bytes", "kind", "compressed", "blocks",
                                               "sized", "records", "wave_records", "lines_out", "output_bytes", "sorted")] + \
               [(n, ctypes.c_float) for n in ("ms_upload", "ms_size", "ms_inflate", "ms_adler", "ms_frame", "ms_parse", "ms_write",
                                              "ms_sort", "ms_total")]


class SortStats(ctypes.Structure):
    """starch_sort_stats: the last sort_bed / sort_check / compress_sorted."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("input_bytes", "n_lines", "n_chromosomes", "already_sorted",
                                               "first_unsorted_line")] + \
               [("radix_passes", ctypes.c_uint32)] + \
               [(n, ctypes.c_float) for n in ("ms_parse", "ms_rank", "ms_sort", "ms_gather", "ms_total")]


class GunzipMember(ctypes.Structure):
    """starch_gunzip_member: one member of a BGZF input's plan."""
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("isize", ctypes.c_uint32), ("crc", ctypes.c_uint32)]


class GunzipStats(ctypes.Structure):
    """starch_gunzip_stats: the last inflate on a context."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("members", "is_bgzf", "stored_blocks", "fixed_blocks", "dynamic_blocks",
                                               "bytes_in", "bytes_out")] + \
               [(n, ctypes.c_float) for n in ("ms_plan", "ms_upload", "ms_size", "ms_inflate", "ms_crc")]


class IndexEntry(ctypes.Structure):
    """starch_index_entry: one stream of an archive's index."""
    _fields_ = [("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("size", ctypes.c_uint64), ("line_count", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64),
                ("n_blocks", ctypes.c_uint32), ("combined_crc", ctypes.c_uint32), ("has_base_counts", ctypes.c_int),
                ("base_count_unique", ctypes.c_int64), ("base_count_nonunique", ctypes.c_int64)]


def load():
    """Load libstarch_amd.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StarchError(-10, "native library missing: %s (run __graft_entry__.build())" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64
    # (same soname as /opt/rocm's).  Loading torch first makes this library
    # bind to torch's copy, so the two share devices, streams and memory;
    # loading ours first and torch later leaves the process with a runtime
    # torch's device setup then breaks for this library (seen as
    # hipErrorNoDevice from starch_create).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, pu64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    sig = {
        "starch_version": ([], ctypes.c_int),
        "starch_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "starch_last_error": ([vp], ctypes.c_char_p),
        "starch_create": ([ctypes.c_int, ctypes.POINTER(vp)], ctypes.c_int),
        "starch_destroy": ([vp], None),
        "starch_set_stream": ([vp, vp], ctypes.c_int),
        "starch_use_own_stream": ([vp], ctypes.c_int),
        "starch_set_lanes": ([vp, ctypes.c_int], ctypes.c_int),
        "starch_options_init": ([ctypes.POINTER(Options)], None),
        "starch_encode_device": ([vp, vp, u64, ctypes.POINTER(Options)], ctypes.c_int),
        "starch_encode_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(Options)], ctypes.c_int),
        "starch_encode_host_into": ([vp, vp, u64, ctypes.POINTER(Options), vp, u64, ctypes.POINTER(u64)],
                                    ctypes.c_int),
        "starch_archive_size": ([vp, pu64], ctypes.c_int),
        "starch_archive_device": ([vp, ctypes.POINTER(vp)], ctypes.c_int),
        "starch_archive_copy": ([vp, vp, u64], ctypes.c_int),
        "starch_segment_count": ([vp, pu64], ctypes.c_int),
        "starch_segments": ([vp, ctypes.POINTER(Segment), u64], ctypes.c_int),
        "starch_segment_name": ([vp, u64, vp, u64, pu64], ctypes.c_int),
        "starch_get_stats": ([vp, ctypes.POINTER(Stats)], ctypes.c_int),
        "starch_transform_host": ([vp, ctypes.c_char_p, u64], ctypes.c_int),
        "starch_transform_device": ([vp, vp, u64], ctypes.c_int),
        "starch_text_size": ([vp, pu64], ctypes.c_int),
        "starch_text_copy": ([vp, vp, u64], ctypes.c_int),
        "starch_text_read": ([vp, u64, vp, u64], ctypes.c_int),
        "starch_bz2_compress_host": ([vp, ctypes.c_char_p, u64, ctypes.c_int, vp, u64, pu64], ctypes.c_int),
        "starch_bz2_compress_many_device": ([vp, vp, pu64, pu64, u64, ctypes.c_int, vp, u64, pu64, pu64],
                                            ctypes.c_int),
        "starch_gen_bed": ([ctypes.c_int, u64, u64, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, vp, u64, pu64],
                           ctypes.c_int),
        "starch_gen_perpos_device": ([ctypes.c_int, u64, u64, vp, u64, pu64, vp], ctypes.c_int),
        "starch_build_index": ([ctypes.POINTER(Segment), ctypes.POINTER(ctypes.c_char_p), pu64, u64, u64,
                                ctypes.c_char_p, ctypes.c_int, vp, u64, pu64], ctypes.c_int),
        "starch_build_index_opt": ([ctypes.POINTER(Segment), ctypes.POINTER(ctypes.c_char_p), pu64, u64, u64,
                                    ctypes.POINTER(Options), vp, u64, pu64], ctypes.c_int),
        "starch_gen_bed_sizes": ([ctypes.c_int, u64, u64, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, pu64],
                                 ctypes.c_int),
        "starch_plan_units": ([ctypes.c_char_p, u64, u64, ctypes.POINTER(Unit), pu64], ctypes.c_int),
        "starch_assign_shards": ([ctypes.POINTER(Unit), u64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)],
                                 ctypes.c_int),
        "starch_encode_units_device": ([vp, vp, ctypes.POINTER(Unit), pu64, u64, ctypes.POINTER(Options)],
                                       ctypes.c_int),
        "starch_streams_device": ([vp, ctypes.POINTER(vp), pu64], ctypes.c_int),
        "starch_streams_copy": ([vp, vp, u64], ctypes.c_int),
        "starch_archive_layout": ([pu64, pu64, u64, u64, pu64, pu64, pu64], ctypes.c_int),
        "starch_encode_multi_host": ([ctypes.POINTER(vp), ctypes.c_int, ctypes.c_char_p, u64,
                                      ctypes.POINTER(Options)], ctypes.c_int),
        "starch_stream_begin": ([vp, ctypes.POINTER(Options), u64], ctypes.c_int),
        "starch_stream_feed": ([vp, vp, u64], ctypes.c_int),
        "starch_stream_window": ([vp, u64, ctypes.POINTER(vp), pu64], ctypes.c_int),
        "starch_stream_commit": ([vp, u64], ctypes.c_int),
        "starch_stream_end": ([vp], ctypes.c_int),
        "starch_stream_available": ([vp, pu64], ctypes.c_int),
        "starch_stream_read": ([vp, vp, u64, pu64], ctypes.c_int),
        "starch_bz2_decompress_host": ([vp, ctypes.c_char_p, u64], ctypes.c_int),
        "starch_bz2_decompress_device": ([vp, vp, u64], ctypes.c_int),
        "starch_bz2_stream_count": ([vp, pu64], ctypes.c_int),
        "starch_bz2_streams": ([vp, ctypes.POINTER(DecStream), u64], ctypes.c_int),
        "starch_untransform_host": ([vp, ctypes.c_char_p, u64, ctypes.c_char_p, u64], ctypes.c_int),
        "starch_unstarch_host": ([vp, ctypes.c_char_p, u64], ctypes.c_int),
        "starch_extract_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(Region), u64], ctypes.c_int),
        "starch_extract_get_stats": ([vp, ctypes.POINTER(ExtractStats)], ctypes.c_int),
        "starch_archive_index": ([ctypes.c_char_p, u64, ctypes.POINTER(IndexEntry), u64, pu64, vp, u64, pu64,
                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "starch_archive_note": ([ctypes.c_char_p, u64, vp, u64, pu64], ctypes.c_int),
        "starch_cat_plan": ([ctypes.POINTER(ctypes.c_char_p), pu64, u64, ctypes.POINTER(Options),
                             ctypes.POINTER(CatGroup), u64, pu64, ctypes.POINTER(CatRun), u64, pu64, vp, u64, pu64],
                            ctypes.c_int),
        "starch_cat_host": ([vp, ctypes.POINTER(ctypes.c_char_p), pu64, u64, ctypes.POINTER(Options),
                             ctypes.POINTER(vp), pu64], ctypes.c_int),
        "starch_cat_get_stats": ([vp, ctypes.POINTER(CatStats)], ctypes.c_int),
        "starch_sort_host": ([vp, ctypes.c_char_p, u64], ctypes.c_int),
        "starch_sort_device": ([vp, vp, u64], ctypes.c_int),
        "starch_sort_get_stats": ([vp, ctypes.POINTER(SortStats)], ctypes.c_int),
        "starch_sort_check_host": ([vp, ctypes.c_char_p, u64, pu64], ctypes.c_int),
        "starch_sort_encode_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(Options)], ctypes.c_int),
        "starch_sort_constants": ([ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_setop_host": ([vp, ctypes.c_int, ctypes.POINTER(SetopInput), u64], ctypes.c_int),
        "starch_setop_device": ([vp, ctypes.c_int, vp, pu64, u64], ctypes.c_int),
        "starch_setop_get_stats": ([vp, ctypes.POINTER(SetopStats)], ctypes.c_int),
        "starch_setop_constants": ([ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_bedops_host": ([vp, ctypes.POINTER(BedopsOptions), ctypes.POINTER(SetopInput), u64], ctypes.c_int),
        "starch_bedops_device": ([vp, ctypes.POINTER(BedopsOptions), vp, pu64, u64], ctypes.c_int),
        "starch_bedops_constants": ([ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_map_host": ([vp, ctypes.POINTER(SetopInput), ctypes.POINTER(SetopInput), ctypes.POINTER(MapOptions)],
                            ctypes.c_int),
        "starch_map_device": ([vp, vp, pu64, u64, ctypes.POINTER(MapOptions)], ctypes.c_int),
        "starch_map_get_stats": ([vp, ctypes.POINTER(MapStats)], ctypes.c_int),
        "starch_map_constants": ([ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_closest_host": ([vp, ctypes.POINTER(SetopInput), ctypes.POINTER(SetopInput),
                                 ctypes.POINTER(ClosestOptions)], ctypes.c_int),
        "starch_closest_device": ([vp, vp, pu64, ctypes.POINTER(ClosestOptions)], ctypes.c_int),
        "starch_closest_get_stats": ([vp, ctypes.POINTER(ClosestStats)], ctypes.c_int),
        "starch_closest_constants": ([ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_mapel_host": ([vp, ctypes.POINTER(SetopInput), ctypes.POINTER(SetopInput), ctypes.POINTER(MapelOptions)],
                              ctypes.c_int),
        "starch_mapel_device": ([vp, vp, pu64, u64, ctypes.POINTER(MapelOptions)], ctypes.c_int),
        "starch_mapel_get_stats": ([vp, ctypes.POINTER(MapelStats)], ctypes.c_int),
        "starch_mapel_constants": ([ctypes.POINTER(ctypes.c_uint32)] * 4, ctypes.c_int),
        "starch_mapsc_host": ([vp, ctypes.POINTER(SetopInput), ctypes.POINTER(SetopInput), ctypes.POINTER(MapscOptions)],
                              ctypes.c_int),
        "starch_mapsc_device": ([vp, vp, pu64, u64, ctypes.POINTER(MapscOptions)], ctypes.c_int),
        "starch_mapsc_get_stats": ([vp, ctypes.POINTER(MapscStats)], ctypes.c_int),
        "starch_mapsc_constants": ([ctypes.POINTER(ctypes.c_uint32)] * 2, ctypes.c_int),
        "starch_convert_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(ConvertOptions)], ctypes.c_int),
        "starch_convert_device": ([vp, vp, u64, ctypes.POINTER(ConvertOptions)], ctypes.c_int),
        "starch_convert_encode_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(ConvertOptions), ctypes.POINTER(Options)],
                                       ctypes.c_int),
        "starch_convert_get_stats": ([vp, ctypes.POINTER(ConvertStats)], ctypes.c_int),
        "starch_convert_constants": ([ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_align_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(AlignOptions)], ctypes.c_int),
        "starch_align_device": ([vp, vp, u64, ctypes.POINTER(AlignOptions)], ctypes.c_int),
        "starch_align_encode_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(AlignOptions), ctypes.POINTER(Options)],
                                     ctypes.c_int),
        "starch_align_get_stats": ([vp, ctypes.POINTER(AlignStats)], ctypes.c_int),
        "starch_align_constants": ([ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_bam_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(BamOptions)], ctypes.c_int),
        "starch_bam_device": ([vp, vp, u64, ctypes.POINTER(BamOptions)], ctypes.c_int),
        "starch_bam_encode_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(BamOptions), ctypes.POINTER(Options)], ctypes.c_int),
        "starch_bam_get_stats": ([vp, ctypes.POINTER(BamStats)], ctypes.c_int),
        "starch_bam_constants": ([ctypes.POINTER(ctypes.c_uint32)] * 3, ctypes.c_int),
        "starch_bbi_info": ([ctypes.c_char_p, u64, ctypes.POINTER(BbiQuery), ctypes.POINTER(BbiHeader),
                             ctypes.POINTER(ctypes.c_uint32), u64, vp, u64, ctypes.POINTER(BbiBlock), pu64, u64, vp, u64],
                            ctypes.c_int),
        "starch_bbi_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(BbiQuery), ctypes.c_uint32], ctypes.c_int),
        "starch_bbi_device": ([vp, vp, u64, ctypes.POINTER(BbiQuery), ctypes.c_uint32], ctypes.c_int),
        "starch_bbi_encode_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(BbiQuery), ctypes.POINTER(Options)], ctypes.c_int),
        "starch_bbi_get_stats": ([vp, ctypes.POINTER(BbiStats)], ctypes.c_int),
        "starch_bbi_constants": ([ctypes.POINTER(ctypes.c_uint32)] * 4, ctypes.c_int),
        "starch_bbi_inflate_host": ([vp, ctypes.c_char_p, u64, ctypes.POINTER(BbiQuery), ctypes.c_uint32], ctypes.c_int),
        "starch_bbi_inflate_table": ([vp, pu64, pu64, u64, pu64, pu64], ctypes.c_int),
        "starch_bbi_adler32_host": ([ctypes.c_char_p, u64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "starch_gunzip_host": ([vp, ctypes.c_char_p, u64], ctypes.c_int),
        "starch_gunzip_device": ([vp, vp, u64], ctypes.c_int),
        "starch_gunzip_plan": ([ctypes.c_char_p, u64, ctypes.POINTER(GunzipMember), u64, pu64,
                                ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "starch_gunzip_get_stats": ([vp, ctypes.POINTER(GunzipStats)], ctypes.c_int),
        "starch_gunzip_constants": ([ctypes.POINTER(ctypes.c_uint32)] * 4, ctypes.c_int),
        "starch_is_gzip": ([ctypes.c_char_p, u64], ctypes.c_int),
        "starch_output_size": ([vp, pu64], ctypes.c_int),
        "starch_output_copy": ([vp, vp, u64], ctypes.c_int),
        "starch_output_device": ([vp, ctypes.POINTER(vp)], ctypes.c_int),
        "starch_encode_units_host": ([vp, vp, ctypes.POINTER(Unit), pu64, u64, ctypes.POINTER(Options)],
                                     ctypes.c_int),
        "starch_comm_id": ([vp], ctypes.c_int),
        "starch_comm_create": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(vp)], ctypes.c_int),
        "starch_comm_create_tcp": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                    ctypes.POINTER(vp)], ctypes.c_int),
        "starch_comm_destroy": ([vp], None),
        "starch_rccl_library": ([], ctypes.c_char_p),
        "starch_comm_last_error": ([], ctypes.c_char_p),
        "starch_gather_archive": ([vp, vp, ctypes.POINTER(Options)], ctypes.c_int),
        "starch_gather_host": ([ctypes.POINTER(HostComm), ctypes.POINTER(Segment), ctypes.POINTER(ctypes.c_char_p),
                                pu64, u64, vp, ctypes.POINTER(Options), ctypes.POINTER(vp), pu64], ctypes.c_int),
        "starch_free": ([vp], None),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def _check(rc, ctx=None):
    if rc != 0:
        L = load()
        detail = L.starch_last_error(ctx).decode(errors="replace") if ctx else ""
        raise StarchError(rc, (L.starch_strerror(rc) or b"").decode() + (": " + detail if detail else ""))


class Starch:
    """One compression context on one MI355X (``starch3::Starch``, hpp:21-584)."""

    client_name = "starch3"
    client_version = "0.1"

    def __init__(self, device=0):
        L = load()
        h = ctypes.c_void_p()
        _check(L.starch_create(device, ctypes.byref(h)))
        self._h = h
        self._L = L
        self._note = ""
        self._method = K_BZIP2
        self.block_size_100k = 9
        self.base_counts = False       # per-segment base counts in segments() and the index (hpp:61-62)
        self._magic = MAGIC

    def close(self):
        if getattr(self, "_h", None):
            self._L.starch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- starch3::Starch configuration surface -------------------------------
    def set_note(self, s):                      # hpp:807-809
        self._note = s

    def get_note(self):
        return self._note

    def set_compression_method(self, m):        # hpp:815-817
        if m not in (K_BZIP2, K_GZIP, K_UNDEFINED):
            raise StarchError(-2, "unknown compression method")
        self._method = m

    def get_compression_method(self):
        return self._method

    def initialize_header_magic_bytes(self):    # hpp:907-910
        self._magic = MAGIC
        return self._magic

    def set_stream(self, hip_stream_ptr):
        """Run on an external HIP stream; 0 is the HIP null stream (torch's default stream)."""
        _check(self._L.starch_set_stream(self._h, ctypes.c_void_p(hip_stream_ptr)), self._h)

    def set_lanes(self, lanes):
        """Encoder lanes of the device-path encodes (1..8; 0: the default, STARCH_DEV_LANES or 2)."""
        _check(self._L.starch_set_lanes(self._h, int(lanes)), self._h)

    def use_own_stream(self):
        """Back to the context's own non-blocking stream (the default)."""
        _check(self._L.starch_use_own_stream(self._h), self._h)

    # -- the hot path ----------------------------------------------------------
    def _opts(self, emit_index=True, reference_compat=False):
        if self._method == K_GZIP and reference_compat:
            raise StarchError(-38, "This method is unsupported at this time")      # hpp:777-779
        if self._method == K_UNDEFINED:
            raise StarchError(-38, "This method is undefined")                      # hpp:780-782
        o = Options()
        self._L.starch_options_init(ctypes.byref(o))
        o.block_size_100k = self.block_size_100k
        o.emit_index = 1 if emit_index else 0
        o.reference_compat = 1 if reference_compat else 0
        o.base_counts = 1 if self.base_counts else 0
        # gzip (-g): one gzip member per segment (deflate on the GPU: a block per 4 KiB,
        # fixed or dynamic Huffman codes, whichever is shorter);
        # the reference itself stops with ENOSYS (kept under reference_compat)
        o.compression_method = 1 if self._method == K_GZIP else 0
        self._note_b = self._note.encode() if self._note else None
        o.note = self._note_b
        return o

    def compress(self, bed: bytes, emit_index=True, reference_compat=False) -> bytes:
        """BED bytes (host) -> Starch archive bytes."""
        o = self._opts(emit_index, reference_compat)
        _check(self._L.starch_encode_host(self._h, bed, len(bed), ctypes.byref(o)), self._h)
        return self.archive()

    def compress_host_ptr(self, ptr: int, n: int, emit_index=True):
        """BED bytes at a host address (e.g. pinned memory) -> archive in HBM."""
        o = self._opts(emit_index)
        _check(self._L.starch_encode_host(self._h, ctypes.cast(ctypes.c_void_p(ptr), ctypes.c_char_p), n,
                                          ctypes.byref(o)), self._h)

    def compress_host_into(self, ptr: int, n: int, out_ptr: int, cap: int, emit_index=True) -> int:
        """BED bytes at a host address -> archive written to the host address
        out_ptr (cap bytes); finished batches go device-to-host while later
        ones encode (starch_encode_host_into).  Returns the archive size."""
        o = self._opts(emit_index)
        k = ctypes.c_uint64()
        _check(self._L.starch_encode_host_into(self._h, ctypes.c_void_p(ptr), n, ctypes.byref(o),
                                               ctypes.c_void_p(out_ptr), cap, ctypes.byref(k)), self._h)
        return k.value

    # -- streaming ingestion (starch_stream_*) ----------------------------------
    def stream_begin(self, batch_bytes=0, emit_index=True, reference_compat=False):
        """Start a streamed encode; feed pieces, read archive bytes as they finish."""
        self._stream_opts = self._opts(emit_index, reference_compat)
        _check(self._L.starch_stream_begin(self._h, ctypes.byref(self._stream_opts), batch_bytes), self._h)

    def stream_feed(self, piece, n=None):
        """Feed host bytes (bytes-like, or an address with n)."""
        if n is None:
            buf = ctypes.c_char_p(bytes(piece)) if not isinstance(piece, bytes) else ctypes.c_char_p(piece)
            _check(self._L.starch_stream_feed(self._h, ctypes.cast(buf, ctypes.c_void_p), len(piece)), self._h)
        else:
            _check(self._L.starch_stream_feed(self._h, ctypes.c_void_p(piece), n), self._h)

    def stream_end(self):
        _check(self._L.starch_stream_end(self._h), self._h)

    def stream_read(self, into=None, cap=None) -> bytes:
        """Drain the archive bytes ready so far (or copy up to cap into an address; returns the count)."""
        if into is not None:
            k = ctypes.c_uint64()
            _check(self._L.starch_stream_read(self._h, ctypes.c_void_p(into), cap, ctypes.byref(k)), self._h)
            return k.value
        n = ctypes.c_uint64()
        _check(self._L.starch_stream_available(self._h, ctypes.byref(n)), self._h)
        buf = ctypes.create_string_buffer(max(1, n.value))
        k = ctypes.c_uint64()
        _check(self._L.starch_stream_read(self._h, buf, n.value, ctypes.byref(k)), self._h)
        return buf.raw[:k.value]

    def compress_stream(self, pieces, batch_bytes=0, emit_index=True, reference_compat=False) -> bytes:
        """Iterable of BED byte pieces -> the archive (streamed encode)."""
        self.stream_begin(batch_bytes, emit_index, reference_compat)
        out = [self.stream_read()]
        for p in pieces:
            self.stream_feed(p)
            out.append(self.stream_read())
        self.stream_end()
        out.append(self.stream_read())
        return b"".join(out)

    def archive_into(self, ptr: int, cap: int) -> int:
        """Copy the archive to a host address; returns its size."""
        n = self.archive_size()
        _check(self._L.starch_archive_copy(self._h, ctypes.c_void_p(ptr), cap), self._h)
        return n

    def compress_device(self, d_ptr: int, n: int, emit_index=True):
        """BED bytes already in HBM (device pointer) -> archive stays in HBM."""
        o = self._opts(emit_index)
        _check(self._L.starch_encode_device(self._h, ctypes.c_void_p(d_ptr), n, ctypes.byref(o)), self._h)

    def encode_units_device(self, d_base: int, units, unit_ids=None, emit_index=False):
        """One shard: units resident in HBM (offsets relative to d_base) -> this
        context's streams (no magic / index); segments() carry each unit id."""
        o = self._opts(emit_index)
        k = len(units)
        U = (Unit * max(1, k))(*units)
        ids = (ctypes.c_uint64 * max(1, k))(*(unit_ids if unit_ids is not None else range(k)))
        _check(self._L.starch_encode_units_device(self._h, ctypes.c_void_p(d_base), U, ids, k, ctypes.byref(o)),
               self._h)

    def encode_units_host(self, bed, units, unit_ids=None, emit_index=False):
        """One shard from host bytes: only the listed units (offsets into bed)
        are copied to HBM, packed; then as encode_units_device."""
        o = self._opts(emit_index)
        k = len(units)
        U = (Unit * max(1, k))(*units)
        ids = (ctypes.c_uint64 * max(1, k))(*(unit_ids if unit_ids is not None else range(k)))
        ptr = bed if isinstance(bed, int) else ctypes.cast(ctypes.c_char_p(bed), ctypes.c_void_p).value
        _check(self._L.starch_encode_units_host(self._h, ctypes.c_void_p(ptr), U, ids, k, ctypes.byref(o)), self._h)

    def gather_archive(self, comm, emit_index=True):
        """Collective over comm (one rank per GPU): every rank's streams from
        its last encode_units_* into rank 0's archive (RCCL, starch_gather_archive)."""
        o = self._opts(emit_index)
        _check(self._L.starch_gather_archive(self._h, comm._h, ctypes.byref(o)), self._h)

    def streams_device(self):
        """(device pointer, bytes) of the last starch_encode_units_device result."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _check(self._L.starch_streams_device(self._h, ctypes.byref(p), ctypes.byref(n)), self._h)
        return p.value or 0, n.value

    def streams(self) -> bytes:
        n = self.streams_device()[1]
        buf = ctypes.create_string_buffer(max(1, n))
        _check(self._L.starch_streams_copy(self._h, buf, n), self._h)
        return buf.raw[:n]

    def archive_size(self):
        n = ctypes.c_uint64()
        _check(self._L.starch_archive_size(self._h, ctypes.byref(n)), self._h)
        return n.value

    def archive_device_ptr(self):
        p = ctypes.c_void_p()
        _check(self._L.starch_archive_device(self._h, ctypes.byref(p)), self._h)
        return p.value

    def archive(self) -> bytes:
        n = self.archive_size()
        buf = ctypes.create_string_buffer(max(1, n))
        _check(self._L.starch_archive_copy(self._h, buf, n), self._h)
        return buf.raw[:n]

    def segments(self):
        """[(chromosome bytes, Segment)] of the last call."""
        n = ctypes.c_uint64()
        _check(self._L.starch_segment_count(self._h, ctypes.byref(n)), self._h)
        arr = (Segment * max(1, n.value))()
        _check(self._L.starch_segments(self._h, arr, n.value), self._h)
        out = []
        for i in range(n.value):
            ln = ctypes.c_uint64()
            buf = ctypes.create_string_buffer(max(1, arr[i].name_len))
            _check(self._L.starch_segment_name(self._h, i, buf, arr[i].name_len, ctypes.byref(ln)), self._h)
            out.append((buf.raw[:ln.value], arr[i]))
        return out

    def stats(self):
        return self._stats(Stats, self._L.starch_get_stats)

    def transform(self, bed: bytes):
        """Transform stage only -> (text, [(chr, line_count, segment text)])."""
        _check(self._L.starch_transform_host(self._h, bed, len(bed)), self._h)
        n = ctypes.c_uint64()
        _check(self._L.starch_text_size(self._h, ctypes.byref(n)), self._h)
        buf = ctypes.create_string_buffer(max(1, n.value))
        _check(self._L.starch_text_copy(self._h, buf, n.value), self._h)
        text = buf.raw[:n.value]
        segs = []
        for name, s in self.segments():
            segs.append((name, s.line_count, text[s.stream_offset:s.stream_offset + s.text_bytes]))
        return text, segs

    def transform_device(self, d_ptr: int, n: int):
        """Transform stage only on BED bytes in HBM; the text stays in HBM
        (text_size / segments(); stats()["ms_transform"])."""
        _check(self._L.starch_transform_device(self._h, ctypes.c_void_p(d_ptr), n), self._h)

    def bz2_compress(self, data: bytes, level: int = 9) -> bytes:
        """One bzip2 stream, byte-identical to libbz2 BZ2_bzCompress(BZ_FINISH)."""
        cap = len(data) + len(data) // 50 + 4096
        buf = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint64()
        _check(self._L.starch_bz2_compress_host(self._h, data, len(data), level, buf, cap, ctypes.byref(n)),
               self._h)
        return buf.raw[:n.value]

    def bz2_compress_many_device(self, d_in, offs, lens, level, d_out, cap):
        k = len(offs)
        O = (ctypes.c_uint64 * max(1, k))(*offs)
        N = (ctypes.c_uint64 * max(1, k))(*lens)
        oo = (ctypes.c_uint64 * max(1, k))()
        ol = (ctypes.c_uint64 * max(1, k))()
        _check(self._L.starch_bz2_compress_many_device(self._h, ctypes.c_void_p(d_in), O, N, k, level,
                                                       ctypes.c_void_p(d_out), cap, oo, ol), self._h)
        return list(oo[:k]), list(ol[:k])


    # ---- decompression / unstarch ----
    def _output_size(self) -> int:
        k = ctypes.c_uint64()
        _check(self._L.starch_output_size(self._h, ctypes.byref(k)), self._h)
        return k.value

    def _output(self) -> bytes:
        n = self._output_size()
        buf = ctypes.create_string_buffer(max(1, n))
        _check(self._L.starch_output_copy(self._h, buf, n), self._h)
        return buf.raw[:n]

    def _stats(self, S, fn) -> dict:
        s = S()
        _check(fn(self._h, ctypes.byref(s)), self._h)
        return _as_dict(s)

    def bz2_decompress(self, data: bytes) -> bytes:
        """Concatenated bzip2 streams -> their bytes (GPU decode, CRCs checked)."""
        _check(self._L.starch_bz2_decompress_host(self._h, data, len(data)), self._h)
        return self._output()

    def bz2_decompress_device(self, d_ptr: int, n: int) -> int:
        """Device-resident streams; returns the output size (output_device_ptr())."""
        _check(self._L.starch_bz2_decompress_device(self._h, ctypes.c_void_p(d_ptr), n), self._h)
        return self._output_size()

    def output_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        _check(self._L.starch_output_device(self._h, ctypes.byref(p)), self._h)
        return p.value or 0

    def decoded_streams(self):
        n = ctypes.c_uint64()
        _check(self._L.starch_bz2_stream_count(self._h, ctypes.byref(n)), self._h)
        arr = (DecStream * max(1, n.value))()
        _check(self._L.starch_bz2_streams(self._h, arr, n.value), self._h)
        return [_as_dict(arr[i]) for i in range(n.value)]

    def untransform(self, text: bytes, chromosome: bytes) -> bytes:
        """One segment's transformed text -> its BED lines (inverse of hpp:428-504)."""
        _check(self._L.starch_untransform_host(self._h, text, len(text), chromosome, len(chromosome)), self._h)
        return self._output()

    def unstarch(self, archive: bytes) -> bytes:
        """An archive of this library back to BED (decode + inverse transform on the GPU)."""
        _check(self._L.starch_unstarch_host(self._h, archive, len(archive)), self._h)
        return self._output()

    def extract(self, archive: bytes, regions) -> bytes:
        """The archive's lines on the given regions, in archive order: a region
        is a chromosome name (``b"chr1"``: all of it) or ``(b"chr1", start,
        stop)``: the lines overlapping [start, stop).  Only the streams of the
        named chromosomes are decoded (the archive's index picks them); the
        coordinate filter runs on the GPU.  No regions: the whole archive."""
        regions = list(regions)
        arr = (Region * max(1, len(regions)))()
        names = []                                   # keeps the name bytes alive for the call
        for k, r in enumerate(regions):
            if isinstance(r, (bytes, bytearray)):
                names.append(bytes(r))
                arr[k] = Region(names[-1], len(names[-1]), 0, 0, 1)
            else:
                names.append(bytes(r[0]))
                arr[k] = Region(names[-1], len(names[-1]), int(r[1]), int(r[2]), 0)
        _check(self._L.starch_extract_host(self._h, archive, len(archive), arr, len(regions)), self._h)
        return self._output()

    def extract_stats(self) -> dict:
        """Of the last extract(): streams_total / streams_decoded /
        compressed_bytes_decoded / lines_scanned / lines_out."""
        return self._stats(ExtractStats, self._L.starch_extract_get_stats)

    # ---- gzip and BGZF inputs ----
    def gunzip(self, data: bytes) -> bytes:
        """A gzip or BGZF file -> its bytes, inflated on the GPU with every
        member's CRC-32 and ISIZE checked.  BGZF members are decoded all at
        once, a wave each; a generic gzip member is decoded by one wave.  A bad
        member is StarchError -12 naming its number, byte offset and the reason."""
        _check(self._L.starch_gunzip_host(self._h, data, len(data)), self._h)
        return self._output()

    def gunzip_device(self, d_ptr: int, n: int) -> int:
        """The same for bytes in HBM; returns the output size (output_device_ptr())."""
        _check(self._L.starch_gunzip_device(self._h, ctypes.c_void_p(d_ptr), n), self._h)
        return self._output_size()

    def gunzip_stats(self) -> dict:
        """Of the last inflate (gunzip(), or a gzip input of a BED method):
        members / is_bgzf / stored_blocks / fixed_blocks / dynamic_blocks /
        bytes_in / bytes_out / ms_plan / ms_upload / ms_size / ms_inflate / ms_crc."""
        return self._stats(GunzipStats, self._L.starch_gunzip_get_stats)

    # ---- sort-bed ----
    def sort_bed(self, bed: bytes) -> bytes:
        """BED lines in any order -> the same lines ordered by (chromosome
        bytes, start, stop); lines equal in all three keep their input order.
        A malformed line is StarchError -12 naming its number."""
        _check(self._L.starch_sort_host(self._h, bed, len(bed)), self._h)
        return self._output()

    def sort_bed_device(self, d_ptr: int, n: int) -> int:
        """The same for BED bytes in HBM; returns the output size (output_device_ptr())."""
        _check(self._L.starch_sort_device(self._h, ctypes.c_void_p(d_ptr), n), self._h)
        return self._output_size()

    def sort_check(self, bed: bytes) -> int:
        """0 if bed is sorted, else the number (from 1) of the first line that
        sorts before its predecessor.  Writes no output."""
        k = ctypes.c_uint64()
        _check(self._L.starch_sort_check_host(self._h, bed, len(bed), ctypes.byref(k)), self._h)
        return k.value

    def sort_stats(self) -> dict:
        """Of the last sort call: input_bytes / n_lines / n_chromosomes /
        already_sorted / first_unsorted_line / radix_passes / ms_*."""
        return self._stats(SortStats, self._L.starch_sort_get_stats)

    def compress_sorted(self, bed: bytes, emit_index=True) -> bytes:
        """sort_bed, then compress from the sorted bytes while they are in HBM:
        the archive compress(sort_bed(bed)) gives."""
        o = self._opts(emit_index)
        _check(self._L.starch_sort_encode_host(self._h, bed, len(bed), ctypes.byref(o)), self._h)
        return self.archive()

    # ---- bedops set operations ----
    def setop(self, op: str, inputs) -> bytes:
        """bedops --merge / --intersect / --difference / --symmdiff /
        --complement over sorted inputs (a list of bytes: BED text, or an
        archive, recognised by its magic) -> BED3, one line per maximal run of
        result bases.  The set definitions are in include/starch_amd.h.  A
        malformed or unsorted line is StarchError -12 naming input and line."""
        if op not in SETOPS:
            raise ValueError("setop: op must be one of %s" % ", ".join(SETOPS))
        arr, n = _inputs(inputs)
        _check(self._L.starch_setop_host(self._h, SETOPS[op], arr, n), self._h)
        return self._output()

    def setop_device(self, op: str, d_ptr: int, offs) -> int:
        """The same for BED text in HBM, input k at d_ptr + [offs[k], offs[k+1]);
        returns the output size (output_device_ptr())."""
        a, k = _offs(offs)
        _check(self._L.starch_setop_device(self._h, SETOPS[op], ctypes.c_void_p(d_ptr), a, k), self._h)
        return self._output_size()

    def merge(self, *inputs) -> bytes: return self.setop("merge", inputs)
    def intersect(self, *inputs) -> bytes: return self.setop("intersect", inputs)
    def difference(self, *inputs) -> bytes: return self.setop("difference", inputs)
    def symmdiff(self, *inputs) -> bytes: return self.setop("symmdiff", inputs)
    def complement(self, *inputs) -> bytes: return self.setop("complement", inputs)

    def bedops(self, op: str, inputs, threshold="100%", chop=1, stagger=None, exclude_short=False) -> bytes:
        """Any operation of the bedops command (a name of BEDOPS_OPS) over
        sorted inputs (a list of bytes: BED text or archives).  The five of
        setop() give BED3; "element_of" / "not_element_of" give the whole
        lines of inputs[0] whose largest overlap with one merged run of the
        other inputs reaches (or misses) ``threshold``, bases as an int or
        "7", percent as "50%"; "partition" gives the disjoint pieces between
        consecutive starts and stops that a line covers; "chop" cuts the
        merged regions into pieces of ``chop`` bases every ``stagger`` (None:
        ``chop``) bases, without the shorter ones if ``exclude_short``;
        "everything" gives every line of every input in sort-bed's order.
        The definitions are in include/starch_amd.h."""
        o = _bedops_options(op, threshold, chop, stagger, exclude_short)
        arr, n = _inputs(inputs)
        _check(self._L.starch_bedops_host(self._h, ctypes.byref(o), arr, n), self._h)
        return self._output()

    def bedops_device(self, op: str, d_ptr: int, offs, threshold="100%", chop=1, stagger=None, exclude_short=False) -> int:
        """The same for BED text in HBM, input k at d_ptr + [offs[k], offs[k+1]);
        returns the output size (output_device_ptr())."""
        o = _bedops_options(op, threshold, chop, stagger, exclude_short)
        a, k = _offs(offs)
        _check(self._L.starch_bedops_device(self._h, ctypes.byref(o), ctypes.c_void_p(d_ptr), a, k), self._h)
        return self._output_size()

    def element_of(self, ref, *others, threshold="100%") -> bytes:
        return self.bedops("element_of", (ref,) + others, threshold=threshold)

    def not_element_of(self, ref, *others, threshold="100%") -> bytes:
        return self.bedops("not_element_of", (ref,) + others, threshold=threshold)

    def partition(self, *inputs) -> bytes: return self.bedops("partition", inputs)

    def chop(self, *inputs, width=1, stagger=None, exclude_short=False) -> bytes:
        return self.bedops("chop", inputs, chop=width, stagger=stagger, exclude_short=exclude_short)

    def everything(self, *inputs) -> bytes: return self.bedops("everything", inputs)

    def setop_stats(self) -> dict:
        """Of the last setop() or bedops(): n_inputs / input_bytes / n_lines / n_chromosomes /
        runs_merged / groups / lines_out / output_bytes / archives_decoded /
        radix_passes / ms_*."""
        return self._stats(SetopStats, self._L.starch_setop_get_stats)

    # ---- bedmap ----
    def bedmap(self, ref, map=None, cols=("echo", "count"), range=0, skip_unmapped=False, delim=b"|") -> bytes:
        """bedmap: one line per line of the sorted reference ``ref`` with the
        columns ``cols`` (names of MAPCOLS, in this order, none twice) joined
        by ``delim``: the reference line, and the count, bases, distinct bases
        and indicator of the lines of the sorted ``map`` (None: ``ref``
        itself) that overlap it after padding it by ``range`` bases.  Either
        input is BED text or an archive.  The definitions are in
        include/starch_amd.h.  A malformed or unsorted line is StarchError -12
        naming input (ref 0, map 1) and line; a bad argument is -2."""
        o = _map_options(cols, range, skip_unmapped, delim)
        _check(self._L.starch_map_host(self._h, *_pair(ref, map), ctypes.byref(o)), self._h)
        return self._output()

    def bedmap_device(self, d_ptr: int, offs, cols=("echo", "count"), range=0, skip_unmapped=False, delim=b"|") -> int:
        """The same for BED text in HBM: the reference at d_ptr + [offs[0],
        offs[1]), the map (if offs has a third entry) at d_ptr + [offs[1],
        offs[2]); returns the output size (output_device_ptr())."""
        o = _map_options(cols, range, skip_unmapped, delim)
        a, k = _offs(offs)
        _check(self._L.starch_map_device(self._h, ctypes.c_void_p(d_ptr), a, k, ctypes.byref(o)), self._h)
        return self._output_size()

    def map_stats(self) -> dict:
        """Of the last bedmap(): n_ref / n_map / n_chromosomes / map_runs_merged /
        stops_sorted / lines_out / output_bytes / ms_*."""
        return self._stats(MapStats, self._L.starch_map_get_stats)

    # ---- closest-features ----
    def closest_features(self, ref, query, closest=False, dist=False, no_overlaps=False, no_ref=False, delim=b"|") -> bytes:
        """closest-features: one line per line of the sorted reference ``ref``:
        the line itself (unless ``no_ref``), then the nearest line of the
        sorted ``query`` to its left and the nearest to its right (``NA`` where
        a side has none), joined by ``delim``.  With ``dist`` every element is
        followed by its signed distance (0: it overlaps), with ``no_overlaps``
        overlapping lines are not considered, with ``closest`` only the nearer
        of the two is written (a tie goes to the left).  Either input is BED
        text or an archive.  The definitions are in include/starch_amd.h.  A
        malformed or unsorted line is StarchError -12 naming input (ref 0,
        query 1) and line; a bad argument is -2."""
        o = _closest_options(closest, dist, no_overlaps, no_ref, delim)
        _check(self._L.starch_closest_host(self._h, *_pair(ref, query), ctypes.byref(o)), self._h)
        return self._output()

    def closest_device(self, d_ptr: int, offs, closest=False, dist=False, no_overlaps=False, no_ref=False, delim=b"|") -> int:
        """The same for BED text in HBM: the reference at d_ptr + [offs[0],
        offs[1]), the query at d_ptr + [offs[1], offs[2]); returns the output
        size (output_device_ptr())."""
        o = _closest_options(closest, dist, no_overlaps, no_ref, delim)
        a, _ = _offs(offs, 3, "closest_device: offs holds three values")
        _check(self._L.starch_closest_device(self._h, ctypes.c_void_p(d_ptr), a, ctypes.byref(o)), self._h)
        return self._output_size()

    def closest_stats(self) -> dict:
        """Of the last closest_features(): n_ref / n_query / n_chromosomes /
        stops_sorted / left_na / right_na / lines_out / output_bytes / ms_*."""
        return self._stats(ClosestStats, self._L.starch_closest_get_stats)

    # ---- bedmap-elements ----
    def map_elements(self, ref, map=None, cols=("echo", "echo_map"), criterion=("bp_ovr", 1), skip_unmapped=False,
                     delim=b"|", multidelim=b";") -> bytes:
        """bedmap-elements: one line per line of the sorted reference ``ref``
        with the columns ``cols`` (names of MAPEL_COLS, in this order, none
        twice) joined by ``delim``.  The hits of a reference line are the
        lines of the sorted ``map`` (None: ``ref`` itself) that satisfy
        ``criterion``: ``("bp_ovr", N)``, ``("range", N)``, ``("exact",)`` or
        ``("fraction_ref" | "fraction_map" | "fraction_both" |
        "fraction_either", F)`` with F a string or decimal.Decimal such as
        "0.5" (never a float: the comparison is exact).  The echo_map columns
        list one value per hit, joined by ``multidelim``.  Either input is BED
        text or an archive.  The definitions are in include/starch_amd.h.  A
        malformed or unsorted line, or a hit without the column echo_map_id or
        echo_map_score asks for, is StarchError -12 naming input (ref 0, map
        1) and line; a bad argument is -2."""
        o = _mapel_options(cols, criterion, skip_unmapped, delim, multidelim)
        _check(self._L.starch_mapel_host(self._h, *_pair(ref, map), ctypes.byref(o)), self._h)
        return self._output()

    def map_elements_device(self, d_ptr: int, offs, cols=("echo", "echo_map"), criterion=("bp_ovr", 1), skip_unmapped=False,
                            delim=b"|", multidelim=b";") -> int:
        """The same for BED text in HBM: the reference at d_ptr + [offs[0],
        offs[1]), the map (if offs has a third entry) at d_ptr + [offs[1],
        offs[2]); returns the output size (output_device_ptr())."""
        o = _mapel_options(cols, criterion, skip_unmapped, delim, multidelim)
        a, k = _offs(offs)
        _check(self._L.starch_mapel_device(self._h, ctypes.c_void_p(d_ptr), a, k, ctypes.byref(o)), self._h)
        return self._output_size()

    def mapel_stats(self) -> dict:
        """Of the last map_elements(): n_ref / n_map / n_chromosomes / hits /
        heavy_lines / walk_steps / lines_out / output_bytes (also under the
        name out_bytes) / ms_*."""
        d = self._stats(MapelStats, self._L.starch_mapel_get_stats)
        d["out_bytes"] = d["output_bytes"]
        return d

    # ---- bedmap-scores ----
    def map_scores(self, ref, map=None, cols=("echo", "mean"), criterion=("bp_ovr", 1), prec=6, kth=None, skip_unmapped=False,
                   delim=b"|") -> bytes:
        """bedmap-scores: one line per line of the sorted reference ``ref``
        with the columns ``cols`` (names of MAPSC_COLS, in this order, none
        twice) joined by ``delim``.  The hits are those of map_elements()
        under the same ``criterion``; the score of a hit is column 5 of its
        map line, an exact decimal with up to 9 digits on either side of the
        point.  sum, mean, min, max, median and kth are exact and are written
        with ``prec`` (0 to 9) decimals, rounded once, ties to even; a line
        without a hit has NAN there.  ``kth`` is a string or decimal.Decimal
        in (0, 1] such as "0.5" (never a float), needed exactly when "kth" is
        a column.  The definitions are in include/starch_amd.h.  A malformed
        or unsorted line, or a hit without a valid score when a column from
        sum on is asked for, is StarchError -12 naming input (ref 0, map 1)
        and line; a bad argument is -2."""
        o = _mapsc_options(cols, criterion, prec, kth, skip_unmapped, delim)
        _check(self._L.starch_mapsc_host(self._h, *_pair(ref, map), ctypes.byref(o)), self._h)
        return self._output()

    def map_scores_device(self, d_ptr: int, offs, cols=("echo", "mean"), criterion=("bp_ovr", 1), prec=6, kth=None,
                          skip_unmapped=False, delim=b"|") -> int:
        """The same for BED text in HBM: the reference at d_ptr + [offs[0],
        offs[1]), the map (if offs has a third entry) at d_ptr + [offs[1],
        offs[2]); returns the output size (output_device_ptr())."""
        o = _mapsc_options(cols, criterion, prec, kth, skip_unmapped, delim)
        a, k = _offs(offs)
        _check(self._L.starch_mapsc_device(self._h, ctypes.c_void_p(d_ptr), a, k, ctypes.byref(o)), self._h)
        return self._output_size()

    def mapsc_stats(self) -> dict:
        """Of the last map_scores(): n_ref / n_map / n_chromosomes / hits /
        straddling / sorted_hits / radix_passes / lines_out / output_bytes /
        ms_*."""
        return self._stats(MapscStats, self._L.starch_mapsc_get_stats)

    # ---- convert2bed ----
    def convert(self, data: bytes, fmt: str, vcf_class="all", keep_header=False, sort=True) -> bytes:
        """convert2bed: text in format ``fmt`` (a name of CONVERT_FORMATS: GFF3,
        GTF, VCF or WIG) -> BED, in sort_bed()'s order unless ``sort`` is
        False.  ``vcf_class`` (a name of VCF_CLASSES, vcf only) splits ALT and
        keeps the alleles of one class; ``keep_header`` turns header lines
        into ``_header`` lines instead of dropping them.  The definitions are
        in include/starch_amd.h.  A line that does not fit its format is
        StarchError -12 naming its number; a bad argument is -2."""
        o = _convert_options(fmt, vcf_class, keep_header, sort)
        _check(self._L.starch_convert_host(self._h, data, len(data), ctypes.byref(o)), self._h)
        return self._output()

    def convert_device(self, d_ptr: int, n: int, fmt: str, vcf_class="all", keep_header=False, sort=True) -> int:
        """The same for text in HBM; returns the output size (output_device_ptr())."""
        o = _convert_options(fmt, vcf_class, keep_header, sort)
        _check(self._L.starch_convert_device(self._h, ctypes.c_void_p(d_ptr), n, ctypes.byref(o)), self._h)
        return self._output_size()

    def compress_converted(self, data: bytes, fmt: str, vcf_class="all", keep_header=False, emit_index=True) -> bytes:
        """convert, sort and compress without leaving HBM: the archive
        compress(convert(data, fmt, ...)) gives."""
        o = _convert_options(fmt, vcf_class, keep_header, True)
        so = self._opts(emit_index)
        _check(self._L.starch_convert_encode_host(self._h, data, len(data), ctypes.byref(o), ctypes.byref(so)), self._h)
        return self.archive()

    def convert_stats(self) -> dict:
        """Of the last convert(): input_bytes / input_lines / header_lines /
        data_lines / declarations / lines_out / output_bytes / sorted / ms_*."""
        return self._stats(ConvertStats, self._L.starch_convert_get_stats)

    # ---- sam2bed, psl2bed, rmsk2bed ----
    def align2bed(self, data: bytes, fmt: str, split=False, split_deletions=False, all_reads=False, reduced=False,
                  keep_header=False, sort=True) -> bytes:
        """sam2bed, psl2bed, rmsk2bed: text in format ``fmt`` (a name of
        ALIGN_FORMATS: SAM, PSL or RepeatMasker .out) -> BED, in sort_bed()'s
        order unless ``sort`` is False.  ``split`` writes a line per CIGAR run
        (sam) or per block (psl); ``split_deletions`` (sam, with split) lets D
        end a run too; ``all_reads`` (sam) keeps unmapped records as
        ``_unmapped`` lines; ``reduced`` (sam) writes six columns;
        ``keep_header`` turns header lines into ``_header`` lines.  The
        definitions are in include/starch_amd.h.  A line that does not fit its
        format is StarchError -12 naming its number; a bad argument is -2."""
        o = _align_options(fmt, split, split_deletions, all_reads, reduced, keep_header, sort)
        _check(self._L.starch_align_host(self._h, data, len(data), ctypes.byref(o)), self._h)
        return self._output()

    def align2bed_device(self, d_ptr: int, n: int, fmt: str, split=False, split_deletions=False, all_reads=False,
                         reduced=False, keep_header=False, sort=True) -> int:
        """The same for text in HBM; returns the output size (output_device_ptr())."""
        o = _align_options(fmt, split, split_deletions, all_reads, reduced, keep_header, sort)
        _check(self._L.starch_align_device(self._h, ctypes.c_void_p(d_ptr), n, ctypes.byref(o)), self._h)
        return self._output_size()

    def compress_aligned(self, data: bytes, fmt: str, split=False, split_deletions=False, all_reads=False, reduced=False,
                         keep_header=False, emit_index=True) -> bytes:
        """align2bed, sort and compress without leaving HBM: the archive
        compress(align2bed(data, fmt, ...)) gives."""
        o = _align_options(fmt, split, split_deletions, all_reads, reduced, keep_header, True)
        so = self._opts(emit_index)
        _check(self._L.starch_align_encode_host(self._h, data, len(data), ctypes.byref(o), ctypes.byref(so)), self._h)
        return self.archive()

    def align_stats(self) -> dict:
        """Of the last align2bed(): input_bytes / input_lines / header_lines /
        records / unmapped_dropped / lines_out / output_bytes / sorted / ms_*."""
        return self._stats(AlignStats, self._L.starch_align_get_stats)

    # ---- bam2bed ----
    def bam2bed(self, data: bytes, split=False, split_deletions=False, all_reads=False, reduced=False, keep_header=False,
                sort=True) -> bytes:
        """bam2bed: BAM (BGZF, any other gzip file of the same bytes, or
        inflated BAM) -> the BED that align2bed(..., "sam") with the same
        options gives for the file's SAM text, in sort_bed()'s order unless
        ``sort`` is False.  The bytes are inflated, cut into records and
        formatted in HBM; the definition is in include/starch_amd.h.  A record
        that does not fit it is StarchError -12 naming its number; a bad
        argument is -2."""
        o = _bam_options(split, split_deletions, all_reads, reduced, keep_header, sort)
        _check(self._L.starch_bam_host(self._h, data, len(data), ctypes.byref(o)), self._h)
        return self._output()

    def bam2bed_device(self, d_ptr: int, n: int, split=False, split_deletions=False, all_reads=False, reduced=False,
                       keep_header=False, sort=True) -> int:
        """The same for INFLATED BAM in HBM; returns the output size (output_device_ptr())."""
        o = _bam_options(split, split_deletions, all_reads, reduced, keep_header, sort)
        _check(self._L.starch_bam_device(self._h, ctypes.c_void_p(d_ptr), n, ctypes.byref(o)), self._h)
        return self._output_size()

    def compress_bam(self, data: bytes, split=False, split_deletions=False, all_reads=False, reduced=False, keep_header=False,
                     emit_index=True) -> bytes:
        """bam2bed, sort and compress without leaving HBM: the archive
        compress(bam2bed(data, ...)) gives."""
        o = _bam_options(split, split_deletions, all_reads, reduced, keep_header, True)
        so = self._opts(emit_index)
        _check(self._L.starch_bam_encode_host(self._h, data, len(data), ctypes.byref(o), ctypes.byref(so)), self._h)
        return self.archive()

    def bam_stats(self) -> dict:
        """Of the last bam2bed(): input_bytes / inflated_bytes / references /
        header_lines / records / unmapped_dropped / tiles / wave_records /
        lines_out / output_bytes / sorted / ms_*."""
        return self._stats(BamStats, self._L.starch_bam_get_stats)

    # ---- bigwig2bed, bigbed2bed ----
    def bbi2bed(self, data: bytes, region=None, sort=True, kind="auto") -> bytes:
        """bigwig2bed / bigbed2bed: a bigWig or bigBed file -> BED, in
        sort_bed()'s order unless ``sort`` is False (then in block order).
        bigWig gives chrom, start, end, value (%g of the float32); bigBed
        chrom, start, end and the rest of the record.  ``region`` (a name, or
        (name, start, end)) restricts the upload to the blocks it needs and the
        lines to the records that meet it.  The blocks are inflated, checked
        and formatted in HBM; the definition is in include/starch_amd.h.  A bad
        block is StarchError -12 naming its number; ``kind`` ("bigwig",
        "bigbed") refuses a file of the other kind."""
        q = _bbi_query(kind, region)
        _check(self._L.starch_bbi_host(self._h, data, len(data), ctypes.byref(q), 0 if sort else 1), self._h)
        return self._output()

    def bbi2bed_device(self, d_ptr: int, n: int, region=None, sort=True, kind="auto") -> int:
        """The same for a file in HBM (it is read back for the host's walk of its
        trees); returns the output size (output_device_ptr())."""
        q = _bbi_query(kind, region)
        _check(self._L.starch_bbi_device(self._h, ctypes.c_void_p(d_ptr), n, ctypes.byref(q), 0 if sort else 1), self._h)
        return self._output_size()

    def compress_bbi(self, data: bytes, region=None, emit_index=True, kind="auto") -> bytes:
        """bbi2bed, sort and compress without leaving HBM: the archive
        compress(bbi2bed(data, region)) gives."""
        q = _bbi_query(kind, region)
        so = self._opts(emit_index)
        _check(self._L.starch_bbi_encode_host(self._h, data, len(data), ctypes.byref(q), ctypes.byref(so)), self._h)
        return self.archive()

    def bbi_stats(self) -> dict:
        """Of the last bbi2bed(): input_bytes / uploaded_bytes / inflated_bytes /
        kind / compressed / blocks / sized / records / wave_records / lines_out /
        output_bytes / sorted / ms_*."""
        return self._stats(BbiStats, self._L.starch_bbi_get_stats)

    def bbi_inflate(self, data: bytes, region=None, gap=0):
        """The zlib stage of bbi2bed() alone, on a compressed file: (area,
        [(offset, length)], pad_ok).  Block k of the region's blocks inflated
        to area[offset:offset + length]; behind every slot lie ``gap`` bytes of
        0xA5; pad_ok: the zero padding behind the uploaded input is intact."""
        q = _bbi_query("auto", region)
        _check(self._L.starch_bbi_inflate_host(self._h, data, len(data), ctypes.byref(q), gap), self._h)
        area = self._output()
        n, ok = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._L.starch_bbi_inflate_table(self._h, None, None, 0, ctypes.byref(n), ctypes.byref(ok))
        if rc not in (0, -3):
            _check(rc, self._h)
        off, ln = (ctypes.c_uint64 * max(1, n.value))(), (ctypes.c_uint64 * max(1, n.value))()
        _check(self._L.starch_bbi_inflate_table(self._h, off, ln, n.value, ctypes.byref(n), ctypes.byref(ok)), self._h)
        return area, [(off[k], ln[k]) for k in range(n.value)], bool(ok.value)

    def cat(self, archives) -> bytes:
        """starchcat: the archives (bytes, in order) merged into one, with this
        instance's note, block_size_100k and base_counts.  A chromosome held
        by one input at the same level is copied byte for byte; the others
        are decoded, merged by (start, stop) and encoded again on the GPU.
        The result is the archive compress() writes for the merged BED."""
        return _cat(self._L, self._h, archives, self._opts())

    def cat_stats(self) -> dict:
        """Of the last cat(): streams_in / streams_copied / groups_merged /
        runs_decoded / lines_merged / bytes_copied / bytes_decoded."""
        return self._stats(CatStats, self._L.starch_cat_get_stats)


def _as_dict(s) -> dict:
    """A ctypes structure's fields by name."""
    return {k: getattr(s, k) for k, _ in s._fields_}


def _offs(offs, exact=None, why=None):
    """(uint64 array of the offsets, number of inputs they bound); exact: the only length allowed, else ValueError(why)."""
    offs = [int(x) for x in offs]
    if exact is not None and len(offs) != exact:
        raise ValueError(why)
    return (ctypes.c_uint64 * len(offs))(*offs), len(offs) - 1


def _inputs(inputs):
    """(SetopInput array, its length) of a list of bytes; the array keeps the bytes alive."""
    inputs = [bytes(b) for b in inputs]
    arr = (SetopInput * max(1, len(inputs)))()
    for k, b in enumerate(inputs):
        arr[k].data = b
        arr[k].len = len(b)
    return arr, len(inputs)


def _pair(ref, other):
    """The two SetopInput arguments of a call that takes a reference and a second input, which may be None."""
    return (ctypes.byref(SetopInput(bytes(ref), len(ref))),
            None if other is None else ctypes.byref(SetopInput(bytes(other), len(other))))


def _constants(fn, n):
    """The n uint32 values fn writes: the value for one, a tuple for several."""
    v = [ctypes.c_uint32() for _ in range(n)]
    _check(fn(*[ctypes.byref(x) for x in v]))
    return v[0].value if n == 1 else tuple(x.value for x in v)


def _named(cols, table, tool):
    """cols as a list, every one a name of table, else ValueError."""
    cols = list(cols)
    for c in cols:
        if c not in table:
            raise ValueError("%s: a column must be one of %s" % (tool, ", ".join(table)))
    return cols


def _fill_cols(o, cols, table):
    """ncols and as many of cols as the structure holds; too many are left to the library."""
    o.ncols = len(cols)
    for k, c in enumerate(cols[:len(o.cols)]):
        o.cols[k] = table[c]


def _put_delim(o, field, delim):
    """The delimiter field and its length; an over-long one is left to the library."""
    delim = bytes(delim)
    setattr(o, field + "_len", len(delim))
    ctypes.memmove(ctypes.addressof(o) + getattr(type(o), field).offset, delim, min(len(delim), 8))


def _criterion(o, criterion):
    """The five criterion fields of MapelOptions or MapscOptions; the messages name bedmap-elements for both."""
    criterion = (criterion,) if isinstance(criterion, str) else tuple(criterion)
    if not criterion or criterion[0] not in MAPEL_CRITERIA or len(criterion) != (1 if criterion[0] == "exact" else 2):
        raise ValueError("bedmap-elements: criterion is ('exact',) or (name, value) with a name of %s" % ", ".join(MAPEL_CRITERIA))
    o.criterion = MAPEL_CRITERIA[criterion[0]]
    if criterion[0] == "bp_ovr":
        o.n = int(criterion[1])
    elif criterion[0] == "range":
        o.range = int(criterion[1])
    elif criterion[0] != "exact":
        o.frac_num, o.frac_digits = mapel_fraction(criterion[1])


def is_gzip(data: bytes) -> bool:
    """True for an input the BED methods take as gzip: at least 18 bytes that begin 1f 8b 08."""
    return bool(load().starch_is_gzip(data, len(data)))


def gunzip_plan(data: bytes):
    """The plan of a gzip input from its headers; opens no GPU.  Returns
    (is_bgzf, members): for BGZF the member table as dicts (in_off, in_len,
    out_off, isize, crc), for generic gzip (False, [])."""
    L = load()
    n, bg = ctypes.c_uint64(), ctypes.c_int()
    _check(L.starch_gunzip_plan(data, len(data), None, 0, ctypes.byref(n), ctypes.byref(bg)))
    arr = (GunzipMember * max(1, n.value))()
    if n.value:
        _check(L.starch_gunzip_plan(data, len(data), arr, n.value, ctypes.byref(n), ctypes.byref(bg)))
    return bool(bg.value), [_as_dict(arr[i]) for i in range(n.value)]


def gunzip_constants():
    """window_bytes (the LDS output ring), primary_bits (codes decoded by one
    table lookup), copy_width (bytes of a match per round), bgzf_max."""
    return dict(zip(("window_bytes", "primary_bits", "copy_width", "bgzf_max"),
                    _constants(load().starch_gunzip_constants, 4)))


def sort_constants():
    """(lines per radix tile, bytes from which an output line is copied by a
    whole wave) of the sort's kernels; no GPU needed."""
    return _constants(load().starch_sort_constants, 2)


def setop_constants():
    """Lines per tile of the set operations' segmented max-scan; no GPU needed."""
    return _constants(load().starch_setop_constants, 1)


def bedops_constants():
    """(runs per tile of element-of's range maximum, pieces per workgroup of
    chop's expansion); no GPU needed."""
    return _constants(load().starch_bedops_constants, 2)


def _bedops_options(op, threshold, chop, stagger, exclude_short):
    """starch_bedops_options; an unknown op or a threshold that is no number is
    ValueError, every range is left to the library."""
    if op not in BEDOPS_OPS:
        raise ValueError("bedops: op must be one of %s" % ", ".join(BEDOPS_OPS))
    o = BedopsOptions()
    o.op = BEDOPS_OPS[op]
    t = threshold.decode("ascii") if isinstance(threshold, (bytes, bytearray)) else threshold
    if isinstance(t, str):
        pct = t.endswith("%")
        digits = t[:-1] if pct else t
        if not (digits.isascii() and digits.isdigit()):
            raise ValueError("bedops: threshold is a number of bases or a percentage such as '50%'")
        o.threshold, o.threshold_is_percent = int(digits), int(pct)
    else:
        o.threshold, o.threshold_is_percent = int(t), 0
    o.chop = int(chop)
    o.stagger = 0 if stagger is None else int(stagger)
    o.exclude_short = bool(exclude_short)
    return o


def map_constants():
    """(reference lines per query workgroup, largest map window in elements
    that is staged in LDS, 0 when there is no such path) of bedmap's query
    kernel; no GPU needed."""
    return _constants(load().starch_map_constants, 2)


def _map_options(cols, range_, skip_unmapped, delim):
    """starch_map_options; unknown names are ValueError, everything else is left to the library."""
    cols = _named(cols, MAPCOLS, "bedmap")
    o = MapOptions()
    _put_delim(o, "delim", delim)
    _fill_cols(o, cols, MAPCOLS)
    o.range = int(range_)
    o.skip_unmapped = bool(skip_unmapped)
    return o


def closest_constants():
    """(reference lines per query workgroup, fan-out of the hierarchy of maxima
    over the query stops) of closest-features' kernels; no GPU needed."""
    return _constants(load().starch_closest_constants, 2)


def _closest_options(closest, dist, no_overlaps, no_ref, delim):
    """starch_closest_options; the delimiter's length is left to the library."""
    o = ClosestOptions(bool(closest), bool(dist), bool(no_overlaps), bool(no_ref))
    _put_delim(o, "delim", delim)
    return o


def mapel_constants():
    """(reference lines per workgroup, fan-out of the hierarchy of maxima over
    the map stops, candidates from which a reference line's run is tested by a
    whole wave, bound on walk_steps per reference line and per hit) of
    bedmap-elements' kernels; no GPU needed."""
    return _constants(load().starch_mapel_constants, 4)


def mapel_fraction(f):
    """(numerator, digits) of the exact decimal ``f``, a str, bytes or
    decimal.Decimal: digits, optionally a point and up to 9 more digits, with a
    value above 0 and up to 1.  Anything else (a float, an exponent, 0, 1.01,
    ten digits) is ValueError."""
    import decimal
    import re
    if isinstance(f, decimal.Decimal):
        if not f.is_finite():
            raise ValueError("bedmap-elements: the fraction is not finite")
        f = format(f, "f")
    elif isinstance(f, (bytes, bytearray)):
        f = bytes(f).decode("ascii", "replace")
    if not isinstance(f, str):
        raise ValueError("bedmap-elements: a fraction is a str or decimal.Decimal such as '0.5', never a float")
    m = re.fullmatch(r"([0-9]*)(?:\.([0-9]*))?", f)
    if not m or not ((m.group(1) or "") + (m.group(2) or "")):
        raise ValueError("bedmap-elements: %r is no plain decimal" % f)
    frac = m.group(2) or ""
    if len(frac) > 9:
        raise ValueError("bedmap-elements: a fraction has at most 9 digits after the point")
    num = int(m.group(1) or "0") * 10 ** len(frac) + int(frac or "0")
    if not 0 < num <= 10 ** len(frac):
        raise ValueError("bedmap-elements: a fraction is above 0 and up to 1")
    return num, len(frac)


def _mapel_options(cols, criterion, skip_unmapped, delim, multidelim):
    """starch_mapel_options; unknown names and a fraction that is no exact
    decimal in (0, 1] are ValueError, everything else is left to the library."""
    cols = _named(cols, MAPEL_COLS, "bedmap-elements")
    o = MapelOptions()
    _criterion(o, criterion)
    _put_delim(o, "delim", delim)
    _put_delim(o, "multidelim", multidelim)
    _fill_cols(o, cols, MAPEL_COLS)
    o.skip_unmapped = bool(skip_unmapped)
    return o


def mapsc_constants():
    """(contiguous hits per workgroup of bedmap-scores' segmented reduction,
    bytes from which an echoed line is copied by a whole wave); no GPU
    needed."""
    return _constants(load().starch_mapsc_constants, 2)


def _mapsc_options(cols, criterion, prec, kth, skip_unmapped, delim):
    """starch_mapsc_options; unknown names, a criterion fraction or a kth that
    is no exact decimal in (0, 1], and a prec that is no integer are
    ValueError, everything else is left to the library."""
    cols = _named(cols, MAPSC_COLS, "bedmap-scores")
    if isinstance(prec, bool) or not isinstance(prec, int) or prec < 0:
        raise ValueError("bedmap-scores: prec is an integer from 0 to 9")
    o = MapscOptions()
    _criterion(o, criterion)
    _put_delim(o, "delim", delim)
    _fill_cols(o, cols, MAPSC_COLS)
    if kth is not None:
        o.kth_num, o.kth_digits = mapel_fraction(kth)
    o.prec = min(prec, 2 ** 32 - 1)
    o.skip_unmapped = bool(skip_unmapped)
    return o


def convert_constants():
    """(threads per block of convert2bed's per-line kernels, bytes from which a
    copied tail is left to a whole wave); no GPU needed."""
    return _constants(load().starch_convert_constants, 2)


def _convert_options(fmt, vcf_class, keep_header, sort):
    """starch_convert_options; unknown names are ValueError, their combination is left to the library."""
    fmt = fmt.lower() if isinstance(fmt, str) else fmt
    if fmt not in CONVERT_FORMATS:
        raise ValueError("convert: fmt must be one of %s" % ", ".join(CONVERT_FORMATS))
    if vcf_class not in VCF_CLASSES:
        raise ValueError("convert: vcf_class must be one of %s" % ", ".join(VCF_CLASSES))
    return ConvertOptions(CONVERT_FORMATS[fmt], VCF_CLASSES[vcf_class], bool(keep_header), not sort)


def align_constants():
    """(threads per block of the per-line kernels of sam2bed, psl2bed and
    rmsk2bed, bytes from which a copied tail is left to a whole wave); no GPU
    needed."""
    return _constants(load().starch_align_constants, 2)


def _align_options(fmt, split, split_deletions, all_reads, reduced, keep_header, sort):
    """starch_align_options; an unknown format name is ValueError, the combination of the flags is left to the library."""
    fmt = fmt.lower() if isinstance(fmt, str) else fmt
    if fmt not in ALIGN_FORMATS:
        raise ValueError("align2bed: fmt must be one of %s" % ", ".join(ALIGN_FORMATS))
    return AlignOptions(ALIGN_FORMATS[fmt], bool(split), bool(split_deletions), bool(all_reads), bool(reduced),
                        bool(keep_header), not sort)


def bam_constants():
    """(bytes of a tile of bam2bed's framing, threads per block of its
    per-record kernels, the l_seq or B count from which a record's columns are
    left to a whole wave); no GPU needed."""
    return _constants(load().starch_bam_constants, 3)


def _bam_options(split, split_deletions, all_reads, reduced, keep_header, sort):
    """starch_bam_options; the combination of the flags is left to the library."""
    return BamOptions(bool(split), bool(split_deletions), bool(all_reads), bool(reduced), bool(keep_header), not sort)


def bbi_constants():
    """(threads per block of bbi2bed's per-record kernels, the bytes of a bigBed
    rest from which its whole wave copies it, the largest uncompressBufSize
    that sizes the slots directly, the bytes of an Adler-32 piece); no GPU needed."""
    return _constants(load().starch_bbi_constants, 4)


def _bbi_query(kind, region):
    """starch_bbi_query; region: None, a name or (name, start, end).  The structure keeps the name alive."""
    o = BbiQuery(BBI_KINDS[kind], 0, None, 0, 0, 0)
    if region is not None:
        name = region if isinstance(region, (bytes, str)) else region[0]
        name = name.encode() if isinstance(name, str) else bytes(name)
        o.region, o.chrom, o.chrom_len = (1 if isinstance(region, (bytes, str)) else 2), name, len(name)
        if o.region == 2:
            o.start, o.end = int(region[1]), int(region[2])
    return o


def bbi_info(data: bytes, region=None) -> dict:
    """What the host reads of a bigWig / bigBed file; opens no GPU.  kind
    ("bigwig" or "bigbed"), version, uncompress_buf_size and the other header
    fields, chroms [(name, size)] by chromId, n_blocks, and blocks: the
    blocks ``region`` needs (all without one) as dicts with their index in the
    block table.  A malformed file is StarchError -12 with the reason."""
    L = load()
    o = _bbi_query("auto", region)
    h = BbiHeader()
    err = ctypes.create_string_buffer(512)

    def call(sizes, ncap, names, mcap, blocks, index, bcap):
        rc = L.starch_bbi_info(data, len(data), ctypes.byref(o), ctypes.byref(h), sizes, ncap, names, mcap, blocks, index, bcap,
                               err, len(err))
        if rc != 0:
            raise StarchError(rc, (L.starch_strerror(rc) or b"").decode() + ": " + err.value.decode(errors="replace"))

    call(None, 0, None, 0, None, None, 0)
    sizes = (ctypes.c_uint32 * max(1, h.n_chroms))()
    names = ctypes.create_string_buffer(max(1, h.names_bytes))
    blocks = (BbiBlock * max(1, h.n_selected))()
    index = (ctypes.c_uint64 * max(1, h.n_selected))()
    call(sizes, h.n_chroms, names, h.names_bytes, blocks, index, h.n_selected)
    out = _as_dict(h)
    out["kind"] = {1: "bigwig", 2: "bigbed"}[h.kind]
    nm = names.raw[:h.names_bytes].split(b"\0")[:h.n_chroms]
    out["chroms"] = [(nm[k], sizes[k]) for k in range(h.n_chroms)]
    out["blocks"] = [dict(_as_dict(blocks[k]), index=index[k]) for k in range(h.n_selected)]
    return out


def _cat_args(archives):
    archives = [bytes(a) for a in archives]
    n = len(archives)
    ptrs = (ctypes.c_char_p * max(1, n))(*archives)
    lens = (ctypes.c_uint64 * max(1, n))(*[len(a) for a in archives])
    return archives, ptrs, lens, n


def _cat_opts(L, note, level, base_counts):
    o = Options()
    L.starch_options_init(ctypes.byref(o))
    o.block_size_100k = int(level)
    o.base_counts = 1 if base_counts else 0
    note_b = note.encode() if isinstance(note, str) else note
    o.note = note_b or None
    return o, note_b


def _cat(L, h, archives, o) -> bytes:
    keep, ptrs, lens, n = _cat_args(archives)
    out, k = ctypes.c_void_p(), ctypes.c_uint64()
    _check(L.starch_cat_host(h, ptrs, lens, n, ctypes.byref(o), ctypes.byref(out), ctypes.byref(k)), h)
    try:
        return ctypes.string_at(out, k.value)
    finally:
        L.starch_free(out)


def cat_host(archives, note=None, level=9, base_counts=False) -> bytes:
    """starchcat without a context (and without a GPU): every chromosome must
    be a copy in cat_plan(); one that has to be merged or re-encoded is
    StarchError -2."""
    L = load()
    o, _keep = _cat_opts(L, note, level, base_counts)
    return _cat(L, None, archives, o)


def cat_plan(archives, level=9, base_counts=False):
    """What cat() would do, without a GPU (starch_cat_plan): the output's
    chromosomes in order as (name: bytes, "copy" | "merge", [(input, entry), ...])."""
    L = load()
    o, _keep = _cat_opts(L, None, level, base_counts)
    keep, ptrs, lens, n = _cat_args(archives)
    ng, nr, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(L.starch_cat_plan(ptrs, lens, n, ctypes.byref(o), None, 0, ctypes.byref(ng), None, 0, ctypes.byref(nr),
                             None, 0, ctypes.byref(nb)))
    groups = (CatGroup * max(1, ng.value))()
    runs = (CatRun * max(1, nr.value))()
    names = ctypes.create_string_buffer(max(1, nb.value))
    _check(L.starch_cat_plan(ptrs, lens, n, ctypes.byref(o), groups, ng.value, ctypes.byref(ng), runs, nr.value,
                             ctypes.byref(nr), names, nb.value, ctypes.byref(nb)))
    return [(names.raw[g.name_off:g.name_off + g.name_len], "merge" if g.merge else "copy",
             [(r.input, r.entry) for r in runs[g.first_run:g.first_run + g.n_runs]]) for g in groups[:ng.value]]


def list_archive(blob: bytes):
    """An archive's index without a GPU (starch_archive_index) ->
    (archive info, [entry dicts]), with the index's own JSON field names;
    chromosome names are bytes."""
    L = load()
    n, nb = ctypes.c_uint64(), ctypes.c_uint64()
    method, bs = ctypes.c_int(), ctypes.c_int()
    rc = L.starch_archive_index(blob, len(blob), None, 0, ctypes.byref(n), None, 0, ctypes.byref(nb),
                                ctypes.byref(method), ctypes.byref(bs))
    if rc:
        raise StarchError(rc, (L.starch_strerror(rc) or b"").decode())
    arr = (IndexEntry * max(1, n.value))()
    names = ctypes.create_string_buffer(max(1, nb.value))
    _check(L.starch_archive_index(blob, len(blob), arr, n.value, ctypes.byref(n), names, nb.value, ctypes.byref(nb),
                                  ctypes.byref(method), ctypes.byref(bs)))
    k = ctypes.c_uint64()
    _check(L.starch_archive_note(blob, len(blob), None, 0, ctypes.byref(k)))
    note = ctypes.create_string_buffer(max(1, k.value))
    _check(L.starch_archive_note(blob, len(blob), note, k.value, ctypes.byref(k)))
    info = {"compressionFormat": "gzip" if method.value == K_GZIP else "bzip2", "blockSize100k": bs.value,
            "note": note.raw[:k.value].decode("utf-8", errors="replace")}
    out = []
    for e in arr[:n.value]:
        d = {"chromosome": names.raw[e.name_off:e.name_off + e.name_len], "offset": e.offset, "size": e.size,
             "uncompressedLineCount": e.line_count, "transformedBytes": e.text_bytes, "blocks": e.n_blocks,
             "combinedCRC": e.combined_crc}
        if e.has_base_counts:
            d["uniqueBaseCount"] = e.base_count_unique
            d["nonUniqueBaseCount"] = e.base_count_nonunique
        out.append(d)
    return info, out


def gen_bed(kind, total_lines, chroms=None, seed=20261015, into=None):
    """Synthetic hg38 BED (kind 0 BED3 / 1 narrowPeak / 2 per-position) for the
    given chromosome ids; returns bytes, or writes into a ctypes buffer."""
    L = load()
    chroms = list(range(24)) if chroms is None else list(chroms)
    C = (ctypes.c_int32 * max(1, len(chroms)))(*chroms)
    n = ctypes.c_uint64()
    _check(L.starch_gen_bed(kind, seed, total_lines, C, len(chroms), None, 0, ctypes.byref(n)))
    if into is not None:
        _check(L.starch_gen_bed(kind, seed, total_lines, C, len(chroms), into, n.value, ctypes.byref(n)))
        return n.value
    buf = ctypes.create_string_buffer(max(1, n.value))
    _check(L.starch_gen_bed(kind, seed, total_lines, C, len(chroms), buf, n.value, ctypes.byref(n)))
    return buf.raw[:n.value]


def gen_perpos_device(chrom, d_ptr=None, cap=0, first=0, count=None, stream=None):
    """Per-position lines of one chromosome written by the GPU at d_ptr (or,
    d_ptr None, just the byte count) -> byte count."""
    L = load()
    count = HG38_LEN[chrom] - first if count is None else count
    n = ctypes.c_uint64()
    _check(L.starch_gen_perpos_device(chrom, first, count, ctypes.c_void_p(d_ptr) if d_ptr else None, cap,
                                      ctypes.byref(n), ctypes.c_void_p(stream) if stream else None))
    return n.value


def gen_bed_sizes(kind, total_lines, chroms=None, seed=20261015):
    """Byte count of each chromosome's lines in gen_bed's output."""
    L = load()
    chroms = list(range(24)) if chroms is None else list(chroms)
    C = (ctypes.c_int32 * max(1, len(chroms)))(*chroms)
    out = (ctypes.c_uint64 * max(1, len(chroms)))()
    _check(L.starch_gen_bed_sizes(kind, seed, total_lines, C, len(chroms), out))
    return list(out[:len(chroms)])


def build_index(segs, names, index_offset, note=None, level=9, base_counts=False):
    """JSON index + 32-byte footer for already-placed streams (multi-GPU gather)."""
    L = load()
    k = len(segs)
    arr = (Segment * max(1, k))(*segs)
    nm = (ctypes.c_char_p * max(1, k))(*names)
    nl = (ctypes.c_uint64 * max(1, k))(*[len(x) for x in names])
    n = ctypes.c_uint64()
    note_b = note.encode() if note else None
    o = Options()
    L.starch_options_init(ctypes.byref(o))
    o.block_size_100k, o.note, o.base_counts = level, note_b, 1 if base_counts else 0
    _check(L.starch_build_index_opt(arr, nm, nl, k, index_offset, ctypes.byref(o), None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(max(1, n.value))
    _check(L.starch_build_index_opt(arr, nm, nl, k, index_offset, ctypes.byref(o), buf, n.value, ctypes.byref(n)))
    return buf.raw[:n.value]


def plan_units(bed: bytes, max_units: int):
    """Split host BED bytes into <= max_units units whose boundaries are segment
    boundaries (starch_plan_units)."""
    L = load()
    out = (Unit * max(1, max_units))()
    n = ctypes.c_uint64()
    _check(L.starch_plan_units(bed, len(bed), max_units, out, ctypes.byref(n)))
    return [Unit(u.offset, u.length, u.init_start, u.init_stop) for u in out[:n.value]]


def assign_shards(units, nshards):
    """LPT assignment of units to shards -> list of shard indices."""
    L = load()
    k = len(units)
    U = (Unit * max(1, k))(*units)
    out = (ctypes.c_int32 * max(1, k))()
    _check(L.starch_assign_shards(U, k, nshards, out))
    return list(out[:k])


def archive_layout(unit_of, nbytes, base=4):
    """Archive order (stable by unit) and byte offsets of gathered segments ->
    (order, offsets, index offset)."""
    L = load()
    k = len(unit_of)
    A = (ctypes.c_uint64 * max(1, k))(*unit_of)
    B = (ctypes.c_uint64 * max(1, k))(*nbytes)
    o = (ctypes.c_uint64 * max(1, k))()
    f = (ctypes.c_uint64 * max(1, k))()
    end = ctypes.c_uint64()
    _check(L.starch_archive_layout(A, B, k, base, o, f, ctypes.byref(end)))
    return list(o[:k]), list(f[:k]), end.value


def compress_multi(ctxs, bed: bytes, emit_index=True, reference_compat=False) -> bytes:
    """In-process multi-device encode (starch_encode_multi_host): shards over
    the given contexts (they may share a device), archive read from ctxs[0]."""
    L = load()
    o = ctxs[0]._opts(emit_index, reference_compat)
    H = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    _check(L.starch_encode_multi_host(H, len(ctxs), bed, len(bed), ctypes.byref(o)), ctxs[0]._h)
    return ctxs[0].archive()


class Comm:
    """One RCCL communicator per process (starch_comm_*): rank 0 makes the id
    (``Comm.new_id()``) and every rank passes it, or use ``Comm.tcp``."""

    def __init__(self, device, rank, world, comm_id):
        L = load()
        h = ctypes.c_void_p()
        rc = L.starch_comm_create(device, rank, world, ctypes.c_char_p(bytes(comm_id)), ctypes.byref(h))
        if rc:
            raise StarchError(rc, L.starch_comm_last_error().decode(errors="replace"))
        self._h, self._L, self.rank, self.world = h, L, rank, world

    @staticmethod
    def new_id() -> bytes:
        L = load()
        buf = ctypes.create_string_buffer(128)
        rc = L.starch_comm_id(buf)
        if rc:
            raise StarchError(rc, L.starch_comm_last_error().decode(errors="replace"))
        return buf.raw

    @classmethod
    def tcp(cls, device, rank, world, host, port):
        self = cls.__new__(cls)
        L = load()
        h = ctypes.c_void_p()
        rc = L.starch_comm_create_tcp(device, rank, world, host.encode(), port, ctypes.byref(h))
        if rc:
            raise StarchError(rc, L.starch_comm_last_error().decode(errors="replace"))
        self._h, self._L, self.rank, self.world = h, L, rank, world
        return self

    @staticmethod
    def rccl_library() -> str:
        """Path of the librccl the gather runs on (dladdr of its symbols)."""
        return (load().starch_rccl_library() or b"").decode(errors="replace")

    def close(self):
        if getattr(self, "_h", None):
            self._L.starch_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gather_host(rank, world, all_gather, send, recv, group_end, segs, names, streams: bytes, note=None, level=9,
                emit_index=True, base_counts=False, reference_compat=False):
    """The library's gather (starch_gather_host) over caller primitives on host
    bytes: all_gather(bytes) -> [bytes per rank]; send(bytes, peer);
    recv(n, peer) -> a handle; group_end() -> {handle: bytes} for the recvs
    posted since the last group_end.  Returns the archive on rank 0, else None."""
    L = load()
    pending = {}

    def _ag(_u, sp, rp, n):
        try:
            parts = all_gather(ctypes.string_at(sp, n))
            for r, p in enumerate(parts):
                ctypes.memmove(rp + r * n, p, n)
            return 0
        except Exception:
            return 1

    def _send(_u, p, n, peer):
        try:
            send(ctypes.string_at(p, n), peer)
            return 0
        except Exception:
            return 1

    def _recv(_u, p, n, peer):
        try:
            pending[recv(n, peer)] = (p, n)
            return 0
        except Exception:
            return 1

    def _end(_u):
        try:
            got = group_end()
            for h, data in got.items():
                p, n = pending.pop(h)
                ctypes.memmove(p, data, n)
            return 0
        except Exception:
            return 1

    hc = HostComm(rank, world, None, _AG_FN(_ag), _SEND_FN(_send), _RECV_FN(_recv), _END_FN(_end))
    k = len(segs)
    arr = (Segment * max(1, k))(*segs)
    nm = (ctypes.c_char_p * max(1, k))(*names)
    nl = (ctypes.c_uint64 * max(1, k))(*[len(x) for x in names])
    o = Options()
    L.starch_options_init(ctypes.byref(o))
    note_b = note.encode() if note else None
    o.block_size_100k, o.note, o.base_counts = level, note_b, 1 if base_counts else 0
    o.emit_index, o.reference_compat = 1 if emit_index else 0, 1 if reference_compat else 0
    sbuf = ctypes.create_string_buffer(streams, max(1, len(streams)))
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    rc = L.starch_gather_host(ctypes.byref(hc), arr, nm, nl, k, sbuf, ctypes.byref(o), ctypes.byref(out),
                              ctypes.byref(n))
    if rc:
        raise StarchError(rc, L.starch_comm_last_error().decode(errors="replace"))
    if not out.value:
        return None
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        L.starch_free(out)


def parse_archive(blob: bytes):
    """Split an archive into (index dict, [stream bytes]) using its footer."""
    if blob[:4] != MAGIC:
        raise ValueError("bad magic")
    foot = blob[-32:]
    off = int(foot[:20])
    idx = json.loads(blob[off:-32].decode("utf-8"))
    streams = [blob[s["offset"]:s["offset"] + s["size"]] for s in idx["streams"]]
    return idx, streams
