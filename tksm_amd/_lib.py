"""ctypes binding of libtksmseq.so -- the C-ABI declared in include/tksmseq.h.

The shared library is the product; this module only loads it.  There is no fallback: if the
library is missing or was not built, importing the compute path raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("TKSMSEQ_LIB", "libtksmseq.so"))   # TKSMSEQ_LIB: diagnostic builds

OK, EINVAL, EIO, EDEVICE, ENOMEM, ESTATE, ELIMIT = range(7)
MODE_PERFECT, MODE_BADREAD = 0, 1


class BatchDesc(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_intervals", C.c_uint64), ("n_mods", C.c_uint64),
                ("n_literals", C.c_uint64), ("literal_bytes", C.c_uint64), ("id_bytes", C.c_uint64),
                ("reads", C.c_void_p), ("intervals", C.c_void_p), ("mods", C.c_void_p), ("literals", C.c_void_p),
                ("literal_pool", C.c_void_p), ("ids", C.c_void_p), ("id_pool", C.c_void_p)]


class RunParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_read_index", C.c_uint64), ("read_index_stride", C.c_uint64),
                ("mode", C.c_int32), ("fastq", C.c_int32), ("compute_qual", C.c_int32), ("collect_stats", C.c_int32),
                ("perfect_of_badread", C.c_int32), ("reserved", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("records", C.c_void_p), ("record_offsets", C.c_void_p), ("records_bytes", C.c_uint64),
                ("n_reads", C.c_uint64), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64),
                ("kernel_ms", C.c_float * 8)]


class GzipResult(C.Structure):            # tksmseq_gzip_result
    _fields_ = [("data", C.c_void_p), ("member_offsets", C.c_void_p), ("bytes", C.c_uint64), ("n_members", C.c_uint64),
                ("device_ms", C.c_float), ("reserved", C.c_float)]


GZIP_RAW, GZIP_FASTA, GZIP_FASTQ = 0, 1, 2


class TailModelDesc(C.Structure):            # tksmseq_tail_model
    _fields_ = [("n_lx", C.c_uint32), ("n_ly", C.c_uint32), ("lx", C.c_void_p), ("ly", C.c_void_p), ("grid", C.c_void_p),
                ("trans", C.c_double * 16), ("ratio", C.c_double), ("bases", C.c_uint8 * 4), ("pad", C.c_uint8 * 4)]


# every symbol include/tksmseq.h declares (checked by tests/test_abi.py without a GPU)
class PcrParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("target_count", C.c_uint64), ("cycles", C.c_int32), ("flags", C.c_int32),
                ("error_rate", C.c_double), ("efficiency", C.c_double), ("template_begin", C.c_uint64), ("template_end", C.c_uint64)]


class TrcParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_molecule_index", C.c_uint64), ("mode", C.c_int32), ("always_end", C.c_int32),
                ("kde_models_length", C.c_int32), ("flags", C.c_int32), ("mu", C.c_double), ("sigma", C.c_double),
                ("kde_model_path", C.c_char_p)]


TRC_NORMAL, TRC_LOGNORMAL, TRC_KDE = 0, 1, 2


class PolyaParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_molecule_index", C.c_uint64), ("dist", C.c_int32), ("flags", C.c_int32),
                ("a", C.c_double), ("b", C.c_double), ("min_length", C.c_int32), ("max_length", C.c_int32)]


class TagParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_molecule_index", C.c_uint64), ("format5", C.c_char_p), ("format3", C.c_char_p),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class ScbParams(C.Structure):
    _fields_ = [("keep_meta_barcodes", C.c_int32), ("flags", C.c_int32)]


class FlipParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_molecule_index", C.c_uint64), ("flip_probability", C.c_double), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


PLA_GAMMA, PLA_POISSON, PLA_WEIBULL, PLA_NORMAL = 0, 1, 2, 3


class FilterCond(C.Structure):               # tksmseq_filter_cond
    _fields_ = [("kind", C.c_int32), ("cmp", C.c_int32), ("text", C.c_char_p), ("value", C.c_int64), ("start", C.c_int64), ("end", C.c_int64),
                ("ranged", C.c_int32), ("reserved", C.c_int32)]


class FilterParams(C.Structure):             # tksmseq_filter_params
    _fields_ = [("conditions", C.POINTER(FilterCond)), ("n_conditions", C.c_uint64), ("negate", C.c_int32), ("flags", C.c_int32)]


FLT_TEXT, FLT_INFO, FLT_SIZE, FLT_LOCUS = 0, 1, 2, 3


class GlueParams(C.Structure):               # tksmseq_glue_params
    _fields_ = [("seed", C.c_uint64), ("first_molecule_index", C.c_uint64), ("probability", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


class ShuffleParams(C.Structure):            # tksmseq_shuffle_params
    _fields_ = [("seed", C.c_uint64), ("buffer_size", C.c_uint64), ("flags", C.c_int32), ("reserved", C.c_int32)]


class MutateParams(C.Structure):             # tksmseq_mutate_params
    _fields_ = [("flags", C.c_int32), ("reserved", C.c_int32)]


class WgsParams(C.Structure):                # tksmseq_wgs_params
    _fields_ = [("seed", C.c_uint64), ("dist", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("b", C.c_double),
                ("base_count", C.c_int64), ("first_candidate", C.c_uint64), ("n_candidates", C.c_uint64),
                ("molecules_before", C.c_uint64), ("bases_before", C.c_uint64)]


class WgsProgress(C.Structure):              # tksmseq_wgs_progress
    _fields_ = [("next_candidate", C.c_uint64), ("molecules", C.c_uint64), ("bases", C.c_uint64), ("reached", C.c_int32),
                ("reserved", C.c_int32)]


WGS_NORMAL, WGS_UNIFORM, WGS_LOGNORMAL, WGS_EXPONENTIAL = 0, 1, 2, 3
WGS_DISTS = {"normal": WGS_NORMAL, "uniform": WGS_UNIFORM, "lognormal": WGS_LOGNORMAL, "exponential": WGS_EXPONENTIAL}
MOL_NO_COMMENTS = 1


class NoiseParams(C.Structure):              # tksmseq_noise_params
    _fields_ = [("seed", C.c_uint64), ("first_molecule_index", C.c_uint64), ("dist", C.c_int32), ("palindromic", C.c_int32),
                ("mu", C.c_double), ("sigma", C.c_double), ("error_rate", C.c_double), ("alphabet", C.c_char_p), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


NOISE_NORMAL, NOISE_LOGNORMAL = 0, 1
NOISE_DISTS = {"normal": NOISE_NORMAL, "lognormal": NOISE_LOGNORMAL}

class TsbParams(C.Structure):                # tksmseq_tsb_params
    _fields_ = [("seed", C.c_uint64), ("molecule_count", C.c_int64), ("weight", C.c_double), ("first_row_index", C.c_uint64),
                ("use_whole_id", C.c_int32), ("reserved", C.c_int32), ("prefix", C.c_char_p)]


class KdeModelParams(C.Structure):           # tksmseq_kde_model_params
    _fields_ = [("seed", C.c_uint64), ("cv_samples", C.c_uint64), ("bandwidth", C.c_double), ("grid_start", C.c_int64),
                ("grid_end", C.c_int64), ("grid_step", C.c_int64), ("model_lengths", C.c_int32), ("reserved", C.c_int32),
                ("end_ratio", C.c_double)]


class AbundanceParams(C.Structure):        # tksmseq_abundance_params
    _fields_ = [("seed", C.c_uint64), ("em_iterations", C.c_int32), ("keep_hits", C.c_int32), ("cb_count", C.c_int64), ("cb_dropout", C.c_double),
                ("cb_mu", C.c_double), ("cb_sigma", C.c_double), ("cb_pattern", C.c_char_p), ("cb_txt_path", C.c_char_p), ("lr_br_path", C.c_char_p)]


class ModelSequenceParams(C.Structure):    # tksmseq_model_sequence_params
    _fields_ = [("error_k", C.c_int32), ("qscore_k", C.c_int32), ("max_alignments", C.c_int64), ("max_alt", C.c_int32), ("max_del", C.c_int32),
                ("min_occur", C.c_int64), ("max_output", C.c_int64), ("chunk_events", C.c_uint64)]


class ModelSequenceInfo(C.Structure):      # tksmseq_model_sequence_info
    _fields_ = [(n, C.c_uint64) for n in ("lines", "used", "skipped_no_cigar", "skipped_supplementary", "skipped_unknown_read", "skipped_unknown_target",
                                          "skipped_cigar_op", "counting_positions", "alternatives_too_long", "windows_max_del", "keys_too_long",
                                          "read_positions", "error_keys", "qscore_keys", "chunks", "events")] + \
               [("device_ms", C.c_float), ("stage_ms", C.c_float * 4), ("reserved", C.c_float), ("read_ms", C.c_double), ("upload_ms", C.c_double),
                ("write_ms", C.c_double)]


class BarcodeMatchParams(C.Structure):     # tksmseq_barcode_match_params
    _fields_ = [("adapter", C.c_char_p), ("window", C.c_int32), ("max_adapter_errors", C.c_int32), ("pad", C.c_int32), ("max_errors", C.c_int32),
                ("min_exact", C.c_int64), ("revcomp_barcodes", C.c_int32), ("reserved", C.c_int32), ("chunk_reads", C.c_uint64),
                ("segments_out", C.c_char_p), ("selected_out", C.c_char_p)]


class BarcodeMatchInfo(C.Structure):       # tksmseq_barcode_match_info
    _fields_ = [(n, C.c_uint64) for n in ("reads", "no_adapter", "forward", "reverse", "whitelist", "candidates", "no_barcode", "unique", "ambiguous",
                                          "pairs", "chunks")] + \
               [("device_ms", C.c_float), ("stage_ms", C.c_float * 4), ("reserved", C.c_float), ("read_ms", C.c_double), ("upload_ms", C.c_double),
                ("write_ms", C.c_double)]


class MapParams(C.Structure):              # tksmseq_map_params
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("max_occ", C.c_int32), ("max_gap", C.c_int32), ("bandwidth", C.c_int32), ("min_count", C.c_int32),
                ("min_score", C.c_int32), ("reserved", C.c_int32), ("secondary_ratio", C.c_double), ("max_secondary", C.c_int32), ("reserved2", C.c_int32),
                ("chunk_reads", C.c_uint64)]


class MapInfo(C.Structure):                # tksmseq_map_info
    _fields_ = [(n, C.c_uint64) for n in ("reads", "mapped", "unmapped", "lines", "secondary", "target_minimizers", "distinct_hashes", "dropped_hashes",
                                          "read_minimizers", "anchors", "groups", "chained_groups", "chunks")] + \
               [("device_ms", C.c_float), ("stage_ms", C.c_float * 5), ("read_ms", C.c_double), ("upload_ms", C.c_double), ("write_ms", C.c_double)]


class AlignParams(C.Structure):            # tksmseq_align_params
    _fields_ = [("band", C.c_int32), ("eqx", C.c_int32)]


class AlignInfo(C.Structure):              # tksmseq_align_info
    _fields_ = [(n, C.c_uint64) for n in ("lines", "segments", "longest_segment", "cells", "columns", "matches", "mismatches", "inserted", "deleted")] + \
               [("align_ms", C.c_float), ("reserved", C.c_float)]


class ExtendParams(C.Structure):           # tksmseq_extend_params
    _fields_ = [("band", C.c_int32), ("drop", C.c_int32), ("max_ext", C.c_int32), ("reserved", C.c_int32)]


class ExtendInfo(C.Structure):             # tksmseq_extend_info
    _fields_ = [(n, C.c_uint64) for n in ("lines", "ends_moved", "target_gained", "read_gained", "matches", "antidiagonals", "cells", "longest")] + \
               [("extend_ms", C.c_float), ("reserved", C.c_float)]


class SplitParams(C.Structure):            # tksmseq_split_params
    _fields_ = [("chains", C.c_int32), ("overlap", C.c_int32), ("segments", C.c_int32), ("reserved", C.c_int32)]


class SplitInfo(C.Structure):              # tksmseq_split_info
    _fields_ = [(n, C.c_uint64) for n in ("split_reads", "supplementary", "later_chains", "rounds", "rejected_overlap")] + \
               [("split_ms", C.c_float), ("reserved", C.c_float)]


class TargetsInfo(C.Structure):            # tksmseq_targets_info
    _fields_ = [(n, C.c_uint64) for n in ("transcripts", "targets", "letters", "exons", "skipped_empty", "skipped_unknown_contig", "skipped_bad_exon",
                                          "projectable", "image_vwords")] + \
               [("splice_ms", C.c_float), ("reserved", C.c_float)]


class MapTargetsParams(C.Structure):       # tksmseq_map_targets_params
    _fields_ = [("genome_coords", C.c_int32), ("reserved", C.c_int32)]


class ProjectInfo(C.Structure):            # tksmseq_project_info
    _fields_ = [(n, C.c_uint64) for n in ("lines", "projected", "unprojected", "junctions")]


BM_CAND_TILE = 256                           # candidates per workgroup row of the barcode match: a multiple of this (bm_kernels.h)
BM_TARGET_WAVES = 2048                       # ... split until about this many waves (bm_kernels.h)
BM_LIST = 8                                  # barcodes listed per read
ABUND_CHUNK = 1024                     # hits per chunk partial of the abundance sums (abund_kernels.h)
KDE_CHUNK = 4096                             # samples per partial grid of tksmseq_kde_grid (kde_kernels.h; doubled for large inputs)
KDE_BANDWIDTHS = tuple(range(50, 1000, 100))

SYMBOLS = [
    "tksmseq_create", "tksmseq_destroy", "tksmseq_last_error", "tksmseq_version", "tksmseq_set_stream",
    "tksmseq_synchronize", "tksmseq_reference_add_fasta", "tksmseq_reference_add_contig",
    "tksmseq_reference_contig_id", "tksmseq_reference_info", "tksmseq_load_error_model",
    "tksmseq_load_qscore_model", "tksmseq_set_identity", "tksmseq_get_error_model", "tksmseq_get_qscore_model",
    "tksmseq_get_identity", "tksmseq_batch_create", "tksmseq_batch_from_mdf_text", "tksmseq_batch_info",
    "tksmseq_batch_free", "tksmseq_run", "tksmseq_set_output_buffer", "tksmseq_set_timing",
    "tksmseq_prefetch_model", "tksmseq_prefetch_identity", "tksmseq_result_download", "tksmseq_result_download_range", "tksmseq_result_copy_device", "tksmseq_stats_download", "tksmseq_interleave_records", "tksmseq_sequence_main",
    "tksmseq_clone", "tksmseq_host_alloc", "tksmseq_host_free", "tksmseq_load_tail_model", "tksmseq_set_tail_model",
    "tksmseq_set_host_threads", "tksmseq_model_available",
    "tksmseq_device_alloc", "tksmseq_device_free", "tksmseq_copy_to_host", "tksmseq_pcr_preset", "tksmseq_pcr", "tksmseq_pcr_template_counts", "tksmseq_truncate", "tksmseq_batch_to_mdf_text", "tksmseq_text_free",
    "tksmseq_molecules_from_mdf_text", "tksmseq_pcr_main", "tksmseq_truncate_main", "tksmseq_run_diagnostics",
    "tksmseq_polya", "tksmseq_tag", "tksmseq_scb", "tksmseq_flip",
    "tksmseq_polya_main", "tksmseq_tag_main", "tksmseq_scb_main", "tksmseq_flip_main",
    "tksmseq_result_gzip", "tksmseq_gzip_device", "tksmseq_gzip_download_range", "tksmseq_gzip_download_offsets",
    "tksmseq_gzip_copy_device", "tksmseq_gzip_eof",
    "tksmseq_reference_declare_contig", "tksmseq_wgs", "tksmseq_random_wgs_main",
    "tksmseq_append_noise", "tksmseq_tail_noise_main",
    "tksmseq_kde_grid", "tksmseq_kde_cv_bandwidth", "tksmseq_model_truncation", "tksmseq_model_truncation_main",
    "tksmseq_transcripts_add_gtf", "tksmseq_transcripts_info", "tksmseq_transcripts_clear", "tksmseq_transcribe_plan_create",
    "tksmseq_transcribe_plan_clone", "tksmseq_transcribe_plan_info", "tksmseq_transcribe_plan_missing", "tksmseq_transcribe_plan_free",
    "tksmseq_transcribe", "tksmseq_transcribe_text", "tksmseq_transcribe_main", "tksmseq_transcribe_device_ms",
    "tksmseq_abundance", "tksmseq_abundance_info", "tksmseq_abundance_row", "tksmseq_abundance_vector", "tksmseq_abundance_transcript",
    "tksmseq_abundance_cell", "tksmseq_abundance_read", "tksmseq_abundance_hits", "tksmseq_abundance_device_ms", "tksmseq_abundance_write",
    "tksmseq_abundance_free", "tksmseq_abundance_main",
    "tksmseq_model_sequence", "tksmseq_model_sequence_main",
    "tksmseq_barcode_match", "tksmseq_barcode_match_main",
    "tksmseq_map", "tksmseq_map_main", "tksmseq_map_align", "tksmseq_map_extend", "tksmseq_map_split",
    "tksmseq_targets_from_transcripts", "tksmseq_targets_get", "tksmseq_targets_download", "tksmseq_targets_write_fasta", "tksmseq_targets_free", "tksmseq_map_targets",
    "tksmseq_filter", "tksmseq_concat", "tksmseq_filter_main",
    "tksmseq_glue", "tksmseq_glue_joins", "tksmseq_shuffle", "tksmseq_unsegment_main", "tksmseq_shuffle_main",
    "tksmseq_variants_load", "tksmseq_variants_info", "tksmseq_variants_free", "tksmseq_mutate", "tksmseq_mutate_main",
]

_lib = None


def load():
    """Loads libtksmseq.so (raises if it has not been built: there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C tksm_amd/csrc).  tksm_amd has no CPU fallback.")
    # (Several contexts in flight want a hardware queue each -- GPU_MAX_HW_QUEUES=16, read when the HIP runtime starts: the CLI and
    # bench.py set it for their own processes; a library import does not touch the environment of the application that embeds it --
    # INTEGRATION.md)
    lib = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int32
    P = C.POINTER
    sig = {
        "tksmseq_create": (C.c_int, [C.c_int, P(vp)]),
        "tksmseq_destroy": (None, [vp]),
        "tksmseq_last_error": (C.c_char_p, [vp]),
        "tksmseq_version": (C.c_char_p, []),
        "tksmseq_set_stream": (C.c_int, [vp, vp]),
        "tksmseq_clone": (C.c_int, [vp, C.POINTER(vp)]),
        "tksmseq_host_alloc": (C.c_int, [C.c_uint64, C.POINTER(vp)]),
        "tksmseq_host_free": (None, [vp]),
        "tksmseq_synchronize": (C.c_int, [vp]),
        "tksmseq_reference_add_fasta": (C.c_int, [vp, C.c_char_p]),
        "tksmseq_reference_add_contig": (C.c_int, [vp, C.c_char_p, vp, u64, C.c_int]),
        "tksmseq_reference_contig_id": (C.c_int, [vp, C.c_char_p]),
        "tksmseq_reference_info": (C.c_int, [vp, P(u64), P(u64), P(u64)]),
        "tksmseq_load_error_model": (C.c_int, [vp, C.c_char_p]),
        "tksmseq_load_qscore_model": (C.c_int, [vp, C.c_char_p]),
        "tksmseq_load_tail_model": (C.c_int, [vp, C.c_char_p]),
        "tksmseq_set_tail_model": (C.c_int, [vp, vp]),
        "tksmseq_set_host_threads": (C.c_int, [vp, C.c_int]),
        "tksmseq_pcr_preset": (C.c_int, [C.c_char_p, P(C.c_double), P(C.c_double)]),
        "tksmseq_pcr": (C.c_int, [vp, vp, vp, P(vp)]),
        "tksmseq_pcr_template_counts": (C.c_int, [vp, vp, vp, P(C.c_uint64)]),
        "tksmseq_truncate": (C.c_int, [vp, vp, vp, P(vp)]),
        "tksmseq_polya": (C.c_int, [vp, vp, P(PolyaParams), P(vp)]),
        "tksmseq_tag": (C.c_int, [vp, vp, P(TagParams), P(vp)]),
        "tksmseq_scb": (C.c_int, [vp, vp, P(ScbParams), P(vp)]),
        "tksmseq_flip": (C.c_int, [vp, vp, P(FlipParams), P(vp)]),
        "tksmseq_batch_to_mdf_text": (C.c_int, [vp, vp, P(vp), P(u64)]),
        "tksmseq_text_free": (None, [vp]),
        "tksmseq_molecules_from_mdf_text": (C.c_int, [vp, C.c_char_p, u64, P(vp)]),
        "tksmseq_model_available": (C.c_int, [C.c_char_p, C.c_char_p]),
        "tksmseq_set_identity": (C.c_int, [vp, C.c_double, C.c_double, C.c_double]),
        "tksmseq_get_error_model": (C.c_int, [vp, P(i32), P(i32), P(i32), vp, vp, vp]),
        "tksmseq_get_qscore_model": (C.c_int, [vp, P(i32), P(i32), P(u64), vp, vp, vp, vp, vp]),
        "tksmseq_get_identity": (C.c_int, [vp, P(i32), P(C.c_double), P(C.c_double), P(C.c_double), vp]),
        "tksmseq_batch_create": (C.c_int, [vp, P(BatchDesc), P(vp)]),
        "tksmseq_batch_from_mdf_text": (C.c_int, [vp, C.c_char_p, u64, P(vp)]),
        "tksmseq_batch_info": (C.c_int, [vp, P(u64), P(u64), P(u64)]),
        "tksmseq_batch_free": (None, [vp, vp]),
        "tksmseq_run": (C.c_int, [vp, vp, P(RunParams), P(Result)]),
        "tksmseq_set_output_buffer": (C.c_int, [vp, vp, u64]),
        "tksmseq_set_timing": (C.c_int, [vp, C.c_int]),
        "tksmseq_run_diagnostics": (C.c_int, [vp, P(C.c_uint32)]),
        "tksmseq_result_download": (C.c_int, [vp, vp, vp]),
        "tksmseq_prefetch_model": (C.c_int, [C.c_char_p, C.c_char_p]),
        "tksmseq_prefetch_identity": (C.c_int, [C.c_double, C.c_double, C.c_double]),
        "tksmseq_result_download_range": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.c_int]),
        "tksmseq_result_copy_device": (C.c_int, [vp, vp, vp]),
        "tksmseq_stats_download": (C.c_int, [vp, vp, vp]),
        "tksmseq_interleave_records": (C.c_int, [vp, C.c_int, P(vp), P(vp), P(u64), vp, u64, P(u64)]),
        "tksmseq_sequence_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_result_gzip": (C.c_int, [vp, P(GzipResult)]),
        "tksmseq_gzip_device": (C.c_int, [vp, vp, u64, C.c_int, P(GzipResult)]),
        "tksmseq_gzip_download_range": (C.c_int, [vp, vp, u64, u64, C.c_int]),
        "tksmseq_gzip_download_offsets": (C.c_int, [vp, vp]),
        "tksmseq_gzip_copy_device": (C.c_int, [vp, vp]),
        "tksmseq_gzip_eof": (C.c_int, [vp]),
        "tksmseq_reference_declare_contig": (C.c_int, [vp, C.c_char_p, u64]),
        "tksmseq_wgs": (C.c_int, [vp, P(WgsParams), P(vp), P(WgsProgress)]),
        "tksmseq_random_wgs_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_append_noise": (C.c_int, [vp, vp, P(NoiseParams), P(vp)]),
        "tksmseq_tail_noise_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_kde_grid": (C.c_int, [vp, vp, u64, vp, C.c_uint32, vp, C.c_uint32, C.c_double, vp]),
        "tksmseq_kde_cv_bandwidth": (C.c_int, [vp, vp, u64, u64, u64, P(C.c_double), vp]),
        "tksmseq_model_truncation": (C.c_int, [vp, P(KdeModelParams), C.c_char_p, C.c_char_p]),
        "tksmseq_model_truncation_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_transcripts_add_gtf": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "tksmseq_transcripts_info": (C.c_int, [vp, P(u64), P(u64)]),
        "tksmseq_transcripts_clear": (C.c_int, [vp]),
        "tksmseq_transcribe_plan_create": (C.c_int, [vp, C.c_char_p, C.c_char_p, u64, P(TsbParams), P(vp)]),
        "tksmseq_transcribe_plan_clone": (C.c_int, [vp, vp, P(vp)]),
        "tksmseq_transcribe_plan_info": (C.c_int, [vp, P(u64), P(u64), P(u64), P(u64)]),
        "tksmseq_transcribe_plan_missing": (C.c_int, [vp, u64, P(vp), P(u64)]),
        "tksmseq_transcribe_plan_free": (None, [vp]),
        "tksmseq_transcribe": (C.c_int, [vp, vp, u64, u64, i32, P(vp)]),
        "tksmseq_transcribe_text": (C.c_int, [vp, u64, u64, P(vp), P(u64)]),
        "tksmseq_transcribe_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_transcribe_device_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float)]),
        "tksmseq_abundance": (C.c_int, [vp, P(AbundanceParams), C.c_char_p, P(vp)]),
        "tksmseq_abundance_info": (C.c_int, [vp, P(u64), P(u64), P(u64), P(u64), P(u64)]),
        "tksmseq_abundance_row": (C.c_int, [vp, u64, P(C.c_char_p), P(C.c_char_p), P(C.c_double)]),
        "tksmseq_abundance_vector": (C.c_int, [vp, P(vp)]),
        "tksmseq_abundance_transcript": (C.c_int, [vp, u64, P(C.c_char_p)]),
        "tksmseq_abundance_cell": (C.c_int, [vp, u64, P(C.c_char_p)]),
        "tksmseq_abundance_read": (C.c_int, [vp, u64, P(C.c_char_p), P(i32)]),
        "tksmseq_abundance_hits": (C.c_int, [vp, P(vp), P(vp), P(vp), P(vp), P(vp)]),
        "tksmseq_abundance_device_ms": (C.c_int, [vp, P(C.c_float)]),
        "tksmseq_abundance_write": (C.c_int, [vp, C.c_char_p]),
        "tksmseq_abundance_free": (None, [vp]),
        "tksmseq_abundance_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_model_sequence": (C.c_int, [vp, P(ModelSequenceParams), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, P(ModelSequenceInfo)]),
        "tksmseq_model_sequence_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_barcode_match": (C.c_int, [vp, P(BarcodeMatchParams), C.c_char_p, C.c_char_p, C.c_char_p, P(BarcodeMatchInfo)]),
        "tksmseq_barcode_match_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_map": (C.c_int, [vp, P(MapParams), C.c_char_p, C.c_char_p, P(MapInfo)]),
        "tksmseq_map_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_map_align": (C.c_int, [vp, P(MapParams), P(AlignParams), C.c_char_p, C.c_char_p, P(MapInfo), P(AlignInfo)]),
        "tksmseq_map_extend": (C.c_int, [vp, P(MapParams), P(AlignParams), P(ExtendParams), C.c_char_p, C.c_char_p, P(MapInfo), P(AlignInfo), P(ExtendInfo)]),
        "tksmseq_map_split": (C.c_int, [vp, P(MapParams), P(AlignParams), P(ExtendParams), P(SplitParams), C.c_char_p, C.c_char_p, P(MapInfo), P(AlignInfo), P(ExtendInfo),
                                        P(SplitInfo)]),
        "tksmseq_targets_from_transcripts": (C.c_int, [vp, P(vp), P(TargetsInfo)]),
        "tksmseq_targets_get": (C.c_int, [vp, u64, P(C.c_char_p), P(C.c_uint32), P(u64), P(i32)]),
        "tksmseq_targets_download": (C.c_int, [vp, vp, vp, vp]),
        "tksmseq_targets_write_fasta": (C.c_int, [vp, vp, C.c_char_p, i32]),
        "tksmseq_targets_free": (None, [vp, vp]),
        "tksmseq_map_targets": (C.c_int, [vp, vp, P(MapTargetsParams), P(MapParams), P(AlignParams), P(ExtendParams), P(SplitParams), C.c_char_p, C.c_char_p, P(MapInfo),
                                          P(AlignInfo), P(ExtendInfo), P(SplitInfo), P(ProjectInfo)]),
        "tksmseq_filter": (C.c_int, [vp, vp, P(FilterParams), P(vp), P(vp)]),
        "tksmseq_concat": (C.c_int, [vp, P(vp), u64, i32, P(vp)]),
        "tksmseq_filter_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_glue": (C.c_int, [vp, vp, P(GlueParams), P(vp)]),
        "tksmseq_glue_joins": (C.c_int, [u64, C.c_double, u64]),
        "tksmseq_shuffle": (C.c_int, [vp, vp, P(ShuffleParams), P(vp)]),
        "tksmseq_unsegment_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_shuffle_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
        "tksmseq_variants_load": (C.c_int, [vp, C.c_char_p, C.c_char_p, u64, P(vp)]),
        "tksmseq_variants_info": (C.c_int, [vp, P(u64), P(u64), P(u64), P(u64), P(u64), P(u64)]),
        "tksmseq_variants_free": (None, [vp]),
        "tksmseq_mutate": (C.c_int, [vp, vp, vp, P(MutateParams), P(vp)]),
        "tksmseq_mutate_main": (C.c_int, [C.c_int, P(C.c_char_p)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    _lib = lib
    return lib
