"""ctypes binding of include/pantax_hip.h (libpantax_hip.so).

This is the same stub a Rust `extern "C"` block would mirror.  There is no CPU
fallback: if the library or a gfx950 device is missing, loading/`init` raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpantax_hip.so")
_lib = None

# every symbol include/pantax_hip.h declares
SYMBOLS = [
    "pantax_hip_init", "pantax_hip_destroy", "pantax_hip_last_error", "pantax_hip_version", "pantax_hip_set_option", "pantax_hip_lad_shape_name",
    "pantax_hip_db_upload", "pantax_hip_db_upload_parts", "pantax_hip_db_free", "pantax_hip_reads_upload", "pantax_hip_reads_free",
    "pantax_hip_bin_reads", "pantax_hip_species_profile", "pantax_hip_db_reset", "pantax_hip_abundance_filter",
    "pantax_hip_trio_index", "pantax_hip_trio_get", "pantax_hip_node_coverage",
    "pantax_hip_strain_profile", "pantax_hip_strain_node_stats", "pantax_hip_strain_hap_stats", "pantax_hip_strain_node_cov", "pantax_hip_pao_solve", "pantax_hip_pao_solve_batch", "pantax_hip_profile", "pantax_hip_profile_step", "pantax_hip_profile_step_enqueue", "pantax_hip_profile_step_collect", "pantax_hip_trio_index_prefetch", "pantax_hip_sort_rows",
    "pantax_hip_scan", "pantax_hip_radix_sort", "pantax_hip_fill",
    "pantax_hip_sample_ranks", "pantax_hip_chacha_block", "pantax_hip_gaf_filter", "pantax_hip_db_save_images", "pantax_hip_db_load_images",
    "pantax_hip_gaf_load", "pantax_hip_gaf_load_device", "pantax_hip_reads_load_gaf", "pantax_hip_reads_set_flags", "pantax_hip_gaf_view", "pantax_hip_gaf_ids", "pantax_hip_gaf_free",
    "pantax_hip_graph_load", "pantax_hip_graph_view", "pantax_hip_graph_free", "pantax_hip_format_f64",
    "pantax_hip_read_strains", "pantax_hip_strain_cov_track", "pantax_hip_strain_evidence", "pantax_hip_strain_read_support", "pantax_hip_strain_depth",
    "pantax_hip_depth_bin", "pantax_hip_depth_bin_range", "pantax_hip_depth_quantile", "pantax_hip_strain_near_miss", "pantax_hip_near_miss_rank",
    "pantax_hip_db_hap_pairs", "pantax_hip_db_pairs", "pantax_hip_strain_pair_evidence", "pantax_hip_strain_fit", "pantax_hip_profile_with_ext",
    "pantax_hip_strain_bootstrap", "pantax_hip_bootstrap_weight", "pantax_hip_bootstrap_summary", "pantax_hip_strain_dropout", "pantax_hip_dropout_substitute",
    "pantax_hip_strain_addin", "pantax_hip_addin_donor", "pantax_hip_strain_read_em", "pantax_hip_read_em",
    "pantax_hip_strain_segments", "pantax_hip_segment_chain",
    "pantax_hip_strain_mosaic", "pantax_hip_mosaic_walk", "pantax_hip_mosaic_top",
    "pantax_hip_strain_read_rescue", "pantax_hip_rescue_walk", "pantax_hip_rescue_rank",
    "pantax_hip_strain_links", "pantax_hip_link_crossings", "pantax_hip_link_top",
    "pantax_hip_strain_rarefy", "pantax_hip_rarefy_node_bases", "pantax_hip_rarefy_depth",
    "pantax_hip_fragment_key", "pantax_hip_fragment_mates", "pantax_hip_strain_fragments",
    "pantax_hip_strain_growth", "pantax_hip_growth_fit", "pantax_hip_growth_status_name",
    "pantax_hip_reads_route_pack", "pantax_hip_route_buffer", "pantax_hip_route_free", "pantax_hip_reads_from_routed",
    "pantax_hip_timing_enable", "pantax_hip_timing_filter", "pantax_hip_timing_reset", "pantax_hip_timing_get", "pantax_hip_sync",
]


E_LIMIT = -4   # pantax_hip_status values the binding itself looks at
SEGMENTS_PEAK_OFF = 0xFFFFFFFFFFFFFFFF   # PANTAX_HIP_SEGMENTS_PEAK_OFF
SEGMENT_CHAIN_N = 7   # PANTAX_HIP_SEGMENT_CHAIN_N
MOSAIC_TOP_OFF = 0xFFFFFFFFFFFFFFFF   # PANTAX_HIP_MOSAIC_TOP_OFF
MOSAIC_CLASSES = 6   # PANTAX_HIP_MOSAIC_CLASSES
RESCUE_CLASSES = 9   # PANTAX_HIP_RESCUE_CLASSES
LINK_SPECIES_N = 6   # PANTAX_HIP_LINK_SPECIES_N
LINK_HAP_N = 8       # PANTAX_HIP_LINK_HAP_N
MATE_NONE = 0xFFFFFFFF        # PANTAX_HIP_MATE_NONE
MATE_AMBIGUOUS = 0xFFFFFFFE   # PANTAX_HIP_MATE_AMBIGUOUS
FRAGMENT_CLASSES = 9   # PANTAX_HIP_FRAGMENT_CLASSES
GROWTH_MIN_WINDOWS = 20   # PANTAX_HIP_GROWTH_MIN_WINDOWS
GROWTH_MIN_DEPTH = 5.0    # PANTAX_HIP_GROWTH_MIN_DEPTH
DEPTH_BINS = 96   # PANTAX_HIP_DEPTH_BINS
DEPTH_NONE = 1    # PANTAX_HIP_DEPTH_NONE: pantax_hip_depth_quantile of a histogram without length


class PantaxHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pantax_hip error %d: %s" % (code, msg))
        self.code = code


class Graphs(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("range_start", C.c_void_p), ("range_end", C.c_void_p),
                ("node_off", C.c_void_p), ("node_len", C.c_void_p), ("hap_off", C.c_void_p),
                ("path_off", C.c_void_p), ("path_nodes", C.c_void_p)]


class GraphPart(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_haps", C.c_uint64), ("node_len", C.c_void_p), ("path_off", C.c_void_p), ("path_nodes", C.c_void_p)]


class PackedReads(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_steps", C.c_uint64), ("step_off", C.c_void_p), ("node_id", C.c_void_p),
                ("pstart", C.c_void_p), ("pend", C.c_void_p), ("qlen", C.c_void_p), ("mapq", C.c_void_p),
                ("flags", C.c_void_p)]


class GafIdsView(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("id_hash", C.c_void_p), ("id_off", C.c_void_p), ("id_len", C.c_void_p),
                ("ids_distinct", C.c_int32), ("id_check", C.c_int32), ("n_pieces", C.c_uint32), ("n_grow_r", C.c_uint32),
                ("n_grow_t", C.c_uint32)]


class HapMetrics(C.Structure):
    _fields_ = [("has", C.c_uint32), ("is_rescue", C.c_int32), ("unique_trio_nodes_fraction", C.c_double),
                ("frequencies_mean", C.c_double), ("path_cov_ratio", C.c_double), ("first_sol", C.c_double),
                ("divergence", C.c_double), ("second_sol", C.c_double), ("total_cov_diff", C.c_double)]


class StrainConfig(C.Structure):
    _fields_ = [("unique_trio_nodes_fraction", C.c_double), ("unique_trio_nodes_mean_count_f", C.c_double),
                ("single_cov_ratio", C.c_double), ("min_depth", C.c_int64), ("shift", C.c_int32),
                ("sample_nodes", C.c_int32), ("solver_semantics", C.c_int32)]


class StepConfig(C.Structure):
    _fields_ = [("unique_trio_nodes_fraction", C.c_double), ("unique_trio_nodes_mean_count_f", C.c_double),
                ("single_cov_ratio", C.c_double), ("single_cov_diff", C.c_double), ("min_cov", C.c_int64),
                ("min_depth", C.c_int64), ("shift", C.c_int32), ("filtered", C.c_int32), ("sample_nodes", C.c_int32),
                ("rebuild_trio", C.c_int32), ("solver_semantics", C.c_int32)]


class SolveInfo(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("status1", C.c_int32), ("status2", C.c_int32), ("iters1", C.c_int32),
                ("iters2", C.c_int32), ("n_rows", C.c_uint32), ("n_patterns", C.c_uint32), ("obj1", C.c_double),
                ("obj2", C.c_double)]


class SpeciesBatch(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("node_off", C.c_void_p), ("node_len", C.c_void_p), ("node_abundance", C.c_void_p),
                ("node_base_cov", C.c_void_p), ("hap_off", C.c_void_p), ("path_off", C.c_void_p), ("path_nodes", C.c_void_p),
                ("cand_off", C.c_void_p), ("cand_path_idx", C.c_void_p), ("fixed_zero", C.c_void_p)]


class SolutionBatch(C.Structure):
    _fields_ = [("x", C.c_void_p), ("path_cov_ratio", C.c_void_p), ("obj", C.c_void_p), ("status", C.c_void_p), ("iters", C.c_void_p)]


class ProfilingConfig(C.Structure):
    _fields_ = [("db", C.c_char_p), ("wd", C.c_char_p), ("output_dir", C.c_char_p), ("genomes_metadata", C.c_char_p),
                ("range_file", C.c_char_p), ("input_aln_file", C.c_char_p), ("species_len_file", C.c_char_p),
                ("out_binning_file", C.c_char_p), ("reads_binning_file", C.c_char_p),
                ("min_species_abundance", C.c_double), ("unique_trio_nodes_fraction", C.c_double),
                ("unique_trio_nodes_mean_count_f", C.c_double), ("single_cov_ratio", C.c_double),
                ("single_cov_diff", C.c_double), ("min_cov", C.c_int64), ("min_depth", C.c_int64),
                ("species", C.c_int32), ("strain", C.c_int32), ("shift", C.c_int32), ("filtered", C.c_int32),
                ("full", C.c_int32), ("force", C.c_int32), ("mode", C.c_int32), ("sample_nodes", C.c_int32),
                ("designated_species", C.c_char_p), ("zip", C.c_char_p), ("rank", C.c_int32), ("world_size", C.c_int32), ("image_cache", C.c_int32),
                ("allreduce_sum", C.c_void_p), ("comm_user", C.c_void_p), ("alltoallv", C.c_void_p), ("comm_device_buffers", C.c_int32),
                ("sample_test", C.c_int32), ("solver_semantics", C.c_int32), ("minimization_min_cov", C.c_double),
                ("read_strain_file", C.c_char_p), ("strain_coverage_file", C.c_char_p), ("strain_coverage_window", C.c_int64),
                ("strain_evidence_file", C.c_char_p), ("strain_read_support_file", C.c_char_p), ("strain_depth_file", C.c_char_p),
                ("strain_near_miss_file", C.c_char_p), ("strain_near_miss_top", C.c_int32), ("strain_pair_evidence_file", C.c_char_p)]


class ReadStrainSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("cand_off", C.c_void_p), ("cand_hap", C.c_void_p), ("cand_w", C.c_void_p)]


class ReadEmSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("cand_off", C.c_void_p), ("cand_hap", C.c_void_p), ("cand_len", C.c_void_p), ("max_iter", C.c_uint32),
                ("tol", C.c_double)]


class CovTrackSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p), ("window", C.c_uint64)]


class EvidenceSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p)]


class SegmentSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p), ("peak_depth", C.c_void_p), ("min_len", C.c_uint64)]


class FitSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p), ("sel_w", C.c_void_p)]


class ProfileExt(C.Structure):
    """pantax_hip_profile_ext12 laid out flat: the 16-byte pantax_hip_profile_ext (struct_size, strain_fit_file), the fields of pantax_hip_profile_ext2
    behind it (40 bytes), strain_dropout_file (48), the two fields of pantax_hip_profile_ext4 (64), the three of pantax_hip_profile_ext5 (88), the four
    of pantax_hip_profile_ext6 (120), the two of pantax_hip_profile_ext7 (136), the two of pantax_hip_profile_ext8 (152), the two of pantax_hip_profile_ext9 (168), the four of pantax_hip_profile_ext10 (200), the one of pantax_hip_profile_ext11 (208) and the four of pantax_hip_profile_ext12 (240); struct_size = ctypes.sizeof(ProfileExt)"""
    _fields_ = [("struct_size", C.c_uint64), ("strain_fit_file", C.c_char_p), ("strain_bootstrap_file", C.c_char_p),
                ("strain_bootstrap_replicates", C.c_uint64), ("strain_bootstrap_seed", C.c_uint64), ("strain_dropout_file", C.c_char_p),
                ("strain_addin_file", C.c_char_p), ("strain_addin_top", C.c_uint64),
                ("strain_em_file", C.c_char_p), ("strain_em_classes", C.c_uint64), ("strain_em_iterations", C.c_uint64),
                ("strain_segments_file", C.c_char_p), ("strain_segments_min", C.c_uint64), ("strain_segments_bridge", C.c_uint64),
                ("strain_segments_peak", C.c_uint64), ("strain_mosaic_file", C.c_char_p), ("strain_mosaic_top", C.c_uint64),
                ("strain_rescue_file", C.c_char_p), ("strain_rescue_top", C.c_uint64),
                ("strain_links_file", C.c_char_p), ("strain_links_top", C.c_uint64),
                ("strain_rarefy_file", C.c_char_p), ("strain_rarefy_levels", C.c_uint64), ("strain_rarefy_replicates", C.c_uint64),
                ("strain_rarefy_seed", C.c_uint64), ("strain_fragments_file", C.c_char_p),
                ("strain_growth_file", C.c_char_p), ("strain_growth_window", C.c_uint64), ("strain_growth_min_own_permille", C.c_uint64),
                ("strain_growth_trim_permille", C.c_uint64)]


class GrowthFitResult(C.Structure):
    """pantax_hip_growth_fit_result"""
    _fields_ = [("n_kept", C.c_uint64), ("n_zero", C.c_uint64), ("n_f", C.c_uint64), ("n_fit", C.c_uint64), ("own_len", C.c_uint64),
                ("median_depth", C.c_double), ("slope", C.c_double), ("intercept", C.c_double), ("r2", C.c_double), ("index", C.c_double),
                ("status", C.c_int32), ("pad", C.c_int32)]


class RarefySet(C.Structure):
    """pantax_hip_rarefy_set"""
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p), ("seed", C.c_uint64), ("n_levels", C.c_uint32),
                ("n_replicates", C.c_uint32)]


class BootstrapSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p), ("sp_key", C.c_void_p), ("seed", C.c_uint64),
                ("n_replicates", C.c_uint32)]


class NearMissSet(C.Structure):
    _fields_ = [("n_species", C.c_uint32), ("sel_off", C.c_void_p), ("sel_hap", C.c_void_p), ("cand_off", C.c_void_p), ("cand_hap", C.c_void_p)]


class DbPairsConfig(C.Structure):
    _fields_ = [("db", C.c_char_p), ("out_file", C.c_char_p), ("range_file", C.c_char_p), ("species", C.c_char_p), ("zip", C.c_char_p),
                ("max_distance", C.c_int64)]


# int (*allreduce_sum)(void *user, double *buf, uint64_t n)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_uint64)
# int (*alltoallv)(void *user, const void *send, const uint64_t *send_off, void *recv, const uint64_t *recv_off)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))


def load():
    """dlopen libpantax_hip.so (built by __graft_entry__.build() / make -C pantax_amd/csrc)."""
    global _lib
    if _lib is None:
        # PANTAX_HIP_LIB: another build of the SAME library (A/B measurements, a -DLAD_PROFILE build) without touching the product file
        path = os.environ.get("PANTAX_HIP_LIB") or LIB_PATH
        if not os.path.exists(path):
            raise ImportError("%s is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                              "pantax_amd has no CPU fallback" % path)
        _lib = C.CDLL(path)
        _lib.pantax_hip_last_error.restype = C.c_char_p
        _lib.pantax_hip_last_error.argtypes = [C.c_void_p]
        _lib.pantax_hip_version.restype = C.c_char_p
        _lib.pantax_hip_lad_shape_name.restype = C.c_char_p
        _lib.pantax_hip_lad_shape_name.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        _lib.pantax_hip_destroy.restype = None
        _lib.pantax_hip_db_free.restype = None
        _lib.pantax_hip_reads_free.restype = None
        _lib.pantax_hip_gaf_free.restype = None
        _lib.pantax_hip_graph_free.restype = None
        _lib.pantax_hip_route_free.restype = None
        _lib.pantax_hip_read_strains.restype = C.c_int
        _lib.pantax_hip_read_strains.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadStrainSet), C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_cov_track.restype = C.c_int
        _lib.pantax_hip_strain_cov_track.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CovTrackSet), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]
        _lib.pantax_hip_strain_growth.restype = C.c_int
        _lib.pantax_hip_strain_growth.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CovTrackSet), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        _lib.pantax_hip_growth_fit.restype = C.c_int
        _lib.pantax_hip_growth_fit.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.POINTER(GrowthFitResult)]
        _lib.pantax_hip_growth_status_name.restype = C.c_char_p
        _lib.pantax_hip_growth_status_name.argtypes = [C.c_int32]
        _lib.pantax_hip_strain_read_support.restype = C.c_int
        _lib.pantax_hip_strain_read_support.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadStrainSet), C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_uint64, C.c_void_p]
        _lib.pantax_hip_strain_evidence.restype = C.c_int
        _lib.pantax_hip_strain_evidence.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EvidenceSet), C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_depth.restype = C.c_int
        _lib.pantax_hip_strain_depth.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EvidenceSet), C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_near_miss.restype = C.c_int
        _lib.pantax_hip_strain_near_miss.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(NearMissSet), C.c_void_p, C.c_void_p]
        _lib.pantax_hip_db_hap_pairs.restype = C.c_int
        _lib.pantax_hip_db_hap_pairs.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EvidenceSet), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_pair_evidence.restype = C.c_int
        _lib.pantax_hip_strain_pair_evidence.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EvidenceSet), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_fit.restype = C.c_int
        _lib.pantax_hip_strain_fit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FitSet), C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_bootstrap.restype = C.c_int
        _lib.pantax_hip_strain_bootstrap.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BootstrapSet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_bootstrap_weight.restype = C.c_uint32
        _lib.pantax_hip_bootstrap_weight.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64]
        _lib.pantax_hip_bootstrap_summary.restype = C.c_int
        _lib.pantax_hip_bootstrap_summary.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_dropout.restype = C.c_int
        _lib.pantax_hip_strain_dropout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EvidenceSet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_dropout_substitute.restype = C.c_int
        _lib.pantax_hip_dropout_substitute.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_addin.restype = C.c_int
        _lib.pantax_hip_strain_addin.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(NearMissSet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_addin_donor.restype = C.c_int
        _lib.pantax_hip_addin_donor.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_read_em.restype = C.c_int
        _lib.pantax_hip_strain_read_em.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadEmSet), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_read_em.restype = C.c_int
        _lib.pantax_hip_read_em.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        _lib.pantax_hip_strain_segments.restype = C.c_int
        _lib.pantax_hip_strain_segments.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SegmentSet), C.c_void_p, C.c_uint64] + [C.c_void_p] * 10
        _lib.pantax_hip_segment_chain.restype = C.c_int
        _lib.pantax_hip_segment_chain.argtypes = [C.c_uint64] + [C.c_void_p] * 5 + [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)] + [C.c_void_p] * 4
        _lib.pantax_hip_strain_mosaic.restype = C.c_int
        _lib.pantax_hip_strain_mosaic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadStrainSet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib.pantax_hip_mosaic_walk.restype = C.c_int
        _lib.pantax_hip_mosaic_walk.argtypes = [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint64)]
        _lib.pantax_hip_mosaic_top.restype = C.c_int
        _lib.pantax_hip_mosaic_top.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
        _lib.pantax_hip_strain_read_rescue.restype = C.c_int
        _lib.pantax_hip_strain_read_rescue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NearMissSet)] + [C.c_void_p] * 4
        _lib.pantax_hip_rescue_walk.restype = C.c_int
        _lib.pantax_hip_rescue_walk.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p]
        _lib.pantax_hip_rescue_rank.restype = C.c_int
        _lib.pantax_hip_rescue_rank.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        _lib.pantax_hip_strain_links.restype = C.c_int
        _lib.pantax_hip_strain_links.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadStrainSet)] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 6
        _lib.pantax_hip_link_crossings.restype = C.c_int
        _lib.pantax_hip_link_crossings.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        _lib.pantax_hip_link_top.restype = C.c_int
        _lib.pantax_hip_link_top.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
        _lib.pantax_hip_strain_rarefy.restype = C.c_int
        _lib.pantax_hip_strain_rarefy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RarefySet)] + [C.c_void_p] * 6
        _lib.pantax_hip_rarefy_node_bases.restype = C.c_int
        _lib.pantax_hip_rarefy_node_bases.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib.pantax_hip_rarefy_depth.restype = C.c_uint32
        _lib.pantax_hip_rarefy_depth.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
        _lib.pantax_hip_fragment_key.restype = C.c_int
        _lib.pantax_hip_fragment_key.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]
        _lib.pantax_hip_fragment_mates.restype = C.c_int
        _lib.pantax_hip_fragment_mates.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.pantax_hip_strain_fragments.restype = C.c_int
        _lib.pantax_hip_strain_fragments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadStrainSet)] + [C.c_void_p] * 5 + [C.c_uint64] + [C.c_void_p] * 2
        _lib.pantax_hip_profile_with_ext.restype = C.c_int
        _lib.pantax_hip_profile_with_ext.argtypes = [C.c_void_p, C.POINTER(ProfilingConfig), C.POINTER(ProfileExt)]
        _lib.pantax_hip_db_pairs.restype = C.c_int
        _lib.pantax_hip_db_pairs.argtypes = [C.c_void_p, C.POINTER(DbPairsConfig)]
        _lib.pantax_hip_near_miss_rank.restype = C.c_int
        _lib.pantax_hip_near_miss_rank.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        _lib.pantax_hip_scan.restype = C.c_int
        _lib.pantax_hip_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.pantax_hip_radix_sort.restype = C.c_int
        _lib.pantax_hip_radix_sort.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.POINTER(C.c_int)]
        _lib.pantax_hip_fill.restype = C.c_int
        _lib.pantax_hip_fill.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        _lib.pantax_hip_depth_bin.restype = C.c_uint32
        _lib.pantax_hip_depth_bin.argtypes = [C.c_uint64]
        _lib.pantax_hip_depth_bin_range.restype = C.c_int
        _lib.pantax_hip_depth_bin_range.argtypes = [C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib.pantax_hip_depth_quantile.restype = C.c_int
        _lib.pantax_hip_depth_quantile.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return _lib


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def as_c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)
