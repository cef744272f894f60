"""ctypes binding of include/hairsplitter_hip.h (the C ABI of the MI355X HairSplitter hot path).

There is no Python/CPU implementation behind these calls: if the HIP library is missing, or there is no GPU,
they raise. Device buffers are torch CUDA tensors (PyTorch-ROCm is only the allocator / stream owner here);
their `data_ptr()` is what crosses the ABI.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from .dist import mean_of_positive_f32, stage4_error_rate, window_size_counts, window_size_from_counts

_ROOT = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_ROOT, "lib", "libhairsplitter_hip.so")
if os.environ.get("HS_LIB_AB"):      # (tools/gpu_ab_lib.sh: another build of the same library, for A/B timing of a code change on one box)
    LIB_PATH = os.environ["HS_LIB_AB"]

# every symbol declared in include/hairsplitter_hip.h
SYMBOLS = [
    "hs_cv_batch_set_ploidy", "hs_version", "hs_last_error", "hs_device_count", "hs_warmup", "hs_set_device", "hs_device_synchronize", "hs_malloc", "hs_free",
    "hs_memcpy_h2d", "hs_memcpy_d2h", "hs_memset", "hs_event_create", "hs_event_destroy", "hs_event_record",
    "hs_event_elapsed_ms", "hs_pileup", "hs_pileup_plan", "hs_free_host", "hs_tile_plan", "hs_column_stats_tiled", "hs_cv_column_pass_taps", "hs_cv_taps_destroy", "hs_cv_pileup_tap", "hs_cv_pileup_tap_destroy", "hs_sr_run_taps", "hs_sr_taps_destroy", "hs_exclusive_scan_i32", "hs_gaf_from_files", "hs_gaf_from_labels", "hs_gro_to_gaf_main", "hs_column_partition_test", "hs_column_partition_last_counts", "hs_loop_a_test", "hs_loop_a_result_destroy", "hs_partition_pair_distance", "hs_snp_planes", "hs_simdiff", "hs_read_graphs",
    "hs_edit_distance", "hs_cv_batch_create", "hs_cv_batch_destroy", "hs_cv_batch_aligned_bp", "hs_cv_run",
    "hs_cv_result_destroy", "hs_cv_select", "hs_cv_run_range", "hs_cv_selection_destroy", "hs_sr_run", "hs_sr_run_cv", "hs_sr_run_cv_range", "hs_pipeline_create", "hs_pipeline_select", "hs_pipeline_run", "hs_pipeline_destroy", "hs_pipeline_thread_devices", "hs_cv_batch_device", "hs_sr_result_destroy", "hs_sr_window_size", "hs_call_variants_main", "hs_call_variants_epilogue",
    "hs_pipeline_run_fused", "hs_realign_paf", "hs_pipeline_set_option", "hs_pipeline_groups", "hs_pipeline_group_range", "hs_pipeline_group_cv", "hs_pipeline_sparse_labels", "hs_separate_reads_main", "hs_main_process_exits", "hs_kernel_name", "hs_kernel_stats_reset", "hs_kernel_stats_get", "hs_kernel_stats_every", "hs_host_wait_stats", "hs_devices", "hs_cv_run_host", "hs_edlib_hw_align", "hs_edlib_align", "hs_edlib_align_bytes", "hs_alignment_to_cigar", "hs_reattach_ends", "hs_trim_polished", "hs_reattach_ends_bytes", "hs_trim_polished_bytes", "hs_free_strings", "hs_cut_gfa", "hs_gfa_to_fasta", "hs_cut_gfa_main", "hs_gfa2fa_main",
    "hs_polish_inputs", "hs_polish_inputs_from_files", "hs_polish_result_destroy", "hs_polish_inputs_main",
    "hs_consensus_default_params", "hs_polish_consensus", "hs_polish_consensus_arrays", "hs_polish_consensus_host", "hs_consensus_result_destroy",
    "hs_polish_haplotypes", "hs_polish_haplotypes_from_files", "hs_haplotypes_result_destroy", "hs_polish_consensus_planned_tap",
    "hs_polish_refine_plan_host", "hs_refine_plan_destroy", "hs_polish_haplotypes_refined", "hs_polish_refine_arrays", "hs_polish_haplotypes_refined_from_files",
    "hs_refined_result_destroy",
    "hs_moves_to_cigar", "hs_realign_intervals", "hs_realign_records_destroy", "hs_cv_batch_create_paf", "hs_cv_batch_create_sam",
    "hs_allele_table_destroy", "hs_alleles_text", "hs_alleles_lds_capacity", "hs_group_alleles_layout", "hs_group_alleles", "hs_haplotype_alleles", "hs_pipeline_alleles",
    "hs_recruit_params_default", "hs_recruit_table_destroy", "hs_recruit_reads", "hs_group_recruit_layout", "hs_group_recruit", "hs_recruit_apply", "hs_recruit_text",
    "hs_pipeline_recruits", "hs_pipeline_set_recruit_params",
    "hs_map_params_default", "hs_map_index_create", "hs_map_index_destroy", "hs_map_index_download", "hs_map_reads", "hs_map_result_destroy", "hs_map_lds_capacity",
    "hs_map_to_batch", "hs_map_text", "hs_map_files", "hs_map_main",
    "hs_map_split_params_default", "hs_map_reads_split", "hs_map_segments_destroy", "hs_map_split_to_batch", "hs_map_segments_text",
    "hs_map_anchor_params_default", "hs_map_reads_anchored", "hs_map_anchors_destroy", "hs_realign_intervals_anchored", "hs_map_to_batch_anchored",
    "hs_realign_cut_tap", "hs_anchor_join_tap",
]

HS_NKERNELS = 28


class HsError(RuntimeError):
    pass


class CvResult(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("mean_distance", C.POINTER(C.c_float)), ("depth", C.POINTER(C.c_float)),
                ("snp_off", C.POINTER(C.c_int64)), ("snp_pos", C.POINTER(C.c_int32)), ("snp_ref", C.POINTER(C.c_uint8)),
                ("snp_alt", C.POINTER(C.c_uint8)), ("snp_n_ref", C.POINTER(C.c_int32)), ("snp_n_alt", C.POINTER(C.c_int32)),
                ("col_off", C.POINTER(C.c_int64)), ("col_idx", C.POINTER(C.c_int32)),
                ("col_code", C.POINTER(C.c_uint8)), ("error_rate", C.c_float), ("n_contigs_with_error_rate", C.c_int32),
                ("t_device_ms", C.c_double), ("t_host_ms", C.c_double), ("t_kernel_ms", C.c_float * 4), ("t_kernel_k4_ms", C.c_float),
                ("n_columns_extracted", C.c_int64), ("n_columns_downloaded", C.c_int64), ("n_columns_downloaded_late", C.c_int64),
                ("entries_borrowed", C.c_int32)]


class KernelStats(C.Structure):
    _fields_ = [("ms", C.c_double * HS_NKERNELS), ("launches", C.c_int64 * HS_NKERNELS), ("bytes", C.c_int64 * HS_NKERNELS)]


class SrContig(C.Structure):
    _fields_ = [("length", C.c_int64), ("n_reads", C.c_int32), ("read_start", C.POINTER(C.c_int32)),
                ("read_end", C.POINTER(C.c_int32)), ("n_snps", C.c_int32), ("snp_pos", C.POINTER(C.c_int32)),
                ("snp_ref", C.POINTER(C.c_uint8)), ("snp_alt", C.POINTER(C.c_uint8)), ("col_off", C.POINTER(C.c_int64)),
                ("col_idx", C.POINTER(C.c_int32)), ("col_code", C.POINTER(C.c_uint8)), ("ploidy", C.c_int32)]


class SrResult(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("win_off", C.POINTER(C.c_int64)), ("win_start", C.POINTER(C.c_int32)),
                ("win_end", C.POINTER(C.c_int32)), ("label_off", C.POINTER(C.c_int64)), ("labels", C.POINTER(C.c_int32)),
                ("t_device_ms", C.c_double), ("t_host_ms", C.c_double), ("n_cw_instances", C.c_int64),
                ("t_kernel_ms", C.c_float * 4), ("t_kernel_graph_ms", C.c_float), ("n_graph_rows_host", C.c_int64), ("n_windows_finished_on_host", C.c_int64),
                ("n_cw_sweeps", C.c_int64), ("cw_bytes", C.c_int64), ("graph_nnz", C.c_int64), ("n_graph_rows", C.c_int64), ("simdiff_bytes", C.c_int64)]


class AlleleTable(C.Structure):
    """hs_allele_table"""
    _fields_ = [("n_windows", C.c_int64), ("n_snps", C.c_int64), ("n_groups", C.c_int64), ("n_cells", C.c_int64),
                ("win_contig", C.POINTER(C.c_int32)), ("win_start", C.POINTER(C.c_int32)), ("win_end", C.POINTER(C.c_int32)),
                ("win_group_off", C.POINTER(C.c_int64)), ("group_ids", C.POINTER(C.c_int32)), ("win_snp_off", C.POINTER(C.c_int64)),
                ("snp_contig", C.POINTER(C.c_int32)), ("snp_pos", C.POINTER(C.c_int32)), ("snp_ref", C.POINTER(C.c_uint8)), ("snp_alt", C.POINTER(C.c_uint8)),
                ("snp_n_calls", C.POINTER(C.c_int32)), ("snp_cell_off", C.POINTER(C.c_int64)), ("cells", C.c_void_p),
                ("t_kernel_ms", C.c_double), ("n_entries", C.c_int64), ("n_wide_columns", C.c_int64)]


class AlleleLayout(C.Structure):
    """hs_allele_layout: byte offsets of the parts of hs_group_alleles' work buffer"""
    _fields_ = [(k, C.c_int64) for k in ("snp_win", "grp_n", "win_snp_first", "win_snp_last", "cell_off", "grp_off", "n_calls", "grp_ids", "grp_pack",
                                         "internal", "total_bytes")]


class RecruitParams(C.Structure):
    """hs_recruit_params"""
    _fields_ = [(k, C.c_int32) for k in ("which", "min_informative", "min_margin", "mismatch_num", "mismatch_den")]


class RecruitTable(C.Structure):
    """hs_recruit_table"""
    _fields_ = [("n_windows", C.c_int64), ("n_rows", C.c_int64), ("n_assigned", C.c_int64),
                ("win_contig", C.POINTER(C.c_int32)), ("win_start", C.POINTER(C.c_int32)), ("win_end", C.POINTER(C.c_int32)),
                ("win_index", C.POINTER(C.c_int64)), ("win_row_off", C.POINTER(C.c_int64)), ("rows", C.c_void_p), ("params", RecruitParams),
                ("n_call_windows", C.c_int64), ("n_counter_words", C.c_int64), ("n_entries", C.c_int64), ("t_kernel_ms", C.c_double)]


class RecruitLayout(C.Structure):
    """hs_recruit_layout: byte offsets of the parts of hs_group_recruit's work buffer (the allele plan's in front)"""
    _fields_ = [("alleles", AlleleLayout)] + [(k, C.c_int64) for k in ("flag", "row_idx", "ctr_off", "win_row_off", "status", "internal", "total_bytes")]


class MapParams(C.Structure):
    """hs_map_params"""
    _fields_ = [(k, C.c_int32) for k in ("k", "w", "max_occ", "band_log2", "min_votes", "extend", "bucket_bits")]


MAP_FIELDS = ("contig", "strand", "qstart", "qend", "tstart", "tend", "votes", "second", "n_minimizers", "n_skipped", "n_hits")


class MapResult(C.Structure):
    """hs_map_result"""
    _fields_ = [("n_reads", C.c_int32), ("contig", C.POINTER(C.c_int32)), ("strand", C.POINTER(C.c_uint8)), ("qstart", C.POINTER(C.c_int32)), ("qend", C.POINTER(C.c_int32)),
                ("tstart", C.POINTER(C.c_int32)), ("tend", C.POINTER(C.c_int32)), ("votes", C.POINTER(C.c_int32)), ("second", C.POINTER(C.c_int32)),
                ("n_minimizers", C.POINTER(C.c_int32)), ("n_skipped", C.POINTER(C.c_int32)), ("n_hits", C.POINTER(C.c_int64)),
                ("n_wide", C.c_int64), ("total_minimizers", C.c_int64), ("total_hits", C.c_int64),
                ("t_minimizers_ms", C.c_double), ("t_hits_ms", C.c_double), ("t_vote_ms", C.c_double)]


class MapSplitParams(C.Structure):
    """hs_map_split_params"""
    _fields_ = [(k, C.c_int32) for k in ("max_segments", "min_votes", "min_span", "max_gap")]


MAP_SEG_FIELDS = ("read", "contig", "strand", "qstart", "qend", "tstart", "tend", "votes", "second", "round")
MAP_SEG_READ_FIELDS = ("n_minimizers", "n_skipped", "n_hits", "read_votes", "read_second")


class MapSegments(C.Structure):
    """hs_map_segments"""
    _fields_ = ([("n_reads", C.c_int32), ("n_segments", C.c_int64), ("seg_off", C.POINTER(C.c_int64))]
                + [(k, C.POINTER(C.c_uint8 if k == "strand" else C.c_int32)) for k in MAP_SEG_FIELDS]
                + [(k, C.POINTER(C.c_int64 if k == "n_hits" else C.c_int32)) for k in MAP_SEG_READ_FIELDS]
                + [("n_wide", C.c_int64), ("total_minimizers", C.c_int64), ("total_hits", C.c_int64),
                   ("t_minimizers_ms", C.c_double), ("t_hits_ms", C.c_double), ("t_vote_ms", C.c_double)])


class MapAnchorParams(C.Structure):
    """hs_map_anchor_params"""
    _fields_ = [("spacing", C.c_int32)]


class MapAnchors(C.Structure):
    """hs_map_anchors"""
    _fields_ = [("n_reads", C.c_int32), ("n_anchors", C.c_int64), ("anc_off", C.POINTER(C.c_int64)), ("anc_q", C.POINTER(C.c_int32)), ("anc_t", C.POINTER(C.c_int32)),
                ("n_best", C.POINTER(C.c_int32)), ("n_chain", C.POINTER(C.c_int32)), ("n_supported", C.POINTER(C.c_int32)), ("t_anchors_ms", C.c_double)]


HS_RECRUIT_ABSENT, HS_RECRUIT_UNCLUSTERED, HS_RECRUIT_LABELLED = 1, 2, 4
# hs_recruit_row (40 bytes)
RECRUIT_ROW = np.dtype([("read", "<i4"), ("label", "<i4"), ("best_group", "<i4"), ("second_group", "<i4"), ("m_best", "<u4"), ("x_best", "<u4"),
                        ("m_second", "<u4"), ("x_second", "<u4"), ("n_entries", "<u4"), ("assigned", "<i4")])
# hs_allele_cell (12 bytes)
ALLELE_CELL = np.dtype([("n", "<u2"), ("best", "<u2"), ("second", "<u2"), ("n_ref", "<u2"), ("n_alt", "<u2"), ("best_code", "u1"), ("call", "u1")])

_lib = None


def load() -> C.CDLL:
    """Loads the in-tree HIP library; raises if it is missing or lacks a declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so.7; whichever HIP runtime is mapped first serves the whole process, and
    # torch only finds the GPU through its own copy. Import torch first so that this library binds to the same runtime.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI itself
        pass
    if not os.path.exists(LIB_PATH):
        raise HsError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                      "there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise HsError("libhairsplitter_hip.so lacks symbols: " + ", ".join(missing))
    lib.hs_version.restype = C.c_char_p
    lib.hs_last_error.restype = C.c_char_p
    lib.hs_cv_batch_aligned_bp.restype = C.c_int64
    lib.hs_cv_batch_aligned_bp.argtypes = [C.c_void_p]
    lib.hs_cv_batch_destroy.argtypes = [C.c_void_p]
    lib.hs_cv_batch_destroy.restype = None
    lib.hs_cv_result_destroy.argtypes = [C.c_void_p]
    lib.hs_cv_result_destroy.restype = None
    lib.hs_pipeline_destroy.argtypes = [C.c_void_p]
    lib.hs_pipeline_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
    lib.hs_pipeline_destroy.restype = None
    lib.hs_cv_selection_destroy.argtypes = [C.c_void_p]
    lib.hs_cv_selection_destroy.restype = None
    lib.hs_free_host.argtypes = [C.c_void_p]
    lib.hs_free_host.restype = None
    lib.hs_sr_result_destroy.argtypes = [C.c_void_p]
    lib.hs_sr_result_destroy.restype = None
    lib.hs_cv_run.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.POINTER(C.POINTER(CvResult))]
    lib.hs_sr_run.argtypes = [C.POINTER(SrContig), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_uint32, C.c_int32,
                              C.POINTER(C.POINTER(SrResult))]
    lib.hs_sr_run_cv.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_int32,
                                 C.POINTER(C.POINTER(SrResult))]
    lib.hs_sr_window_size.argtypes = [C.POINTER(SrContig), C.c_int32, C.c_int32]
    lib.hs_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    lib.hs_event_record.argtypes = [C.c_void_p, C.c_void_p]
    lib.hs_event_destroy.argtypes = [C.c_void_p]
    lib.hs_kernel_name.restype = C.c_char_p
    lib.hs_kernel_name.argtypes = [C.c_int]
    lib.hs_kernel_stats_reset.restype = None
    lib.hs_kernel_stats_get.restype = None
    lib.hs_kernel_stats_get.argtypes = [C.POINTER(KernelStats)]
    lib.hs_realign_records_destroy.restype = None
    lib.hs_allele_table_destroy.restype = None
    lib.hs_allele_table_destroy.argtypes = [C.c_void_p]
    lib.hs_pipeline_alleles.restype = C.POINTER(AlleleTable)
    lib.hs_pipeline_alleles.argtypes = [C.c_void_p]
    lib.hs_haplotype_alleles.argtypes = [C.POINTER(SrContig), C.c_int32, C.POINTER(SrResult), C.POINTER(C.POINTER(AlleleTable))]
    lib.hs_alleles_lds_capacity.restype = C.c_int32
    lib.hs_recruit_params_default.restype = RecruitParams
    lib.hs_recruit_table_destroy.restype = None
    lib.hs_recruit_table_destroy.argtypes = [C.c_void_p]
    lib.hs_pipeline_recruits.restype = C.POINTER(RecruitTable)
    lib.hs_pipeline_recruits.argtypes = [C.c_void_p]
    lib.hs_pipeline_set_recruit_params.argtypes = [C.c_void_p, C.POINTER(RecruitParams)]
    lib.hs_recruit_reads.argtypes = [C.POINTER(SrContig), C.c_int32, C.POINTER(SrResult), C.POINTER(RecruitParams), C.POINTER(C.POINTER(AlleleTable)),
                                     C.POINTER(C.POINTER(RecruitTable))]
    lib.hs_recruit_apply.argtypes = [C.POINTER(RecruitTable), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.hs_recruit_text.argtypes = [C.POINTER(RecruitTable), C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)]
    lib.hs_map_params_default.restype = MapParams
    lib.hs_map_lds_capacity.restype = C.c_int32
    lib.hs_map_index_destroy.restype = None
    lib.hs_map_index_destroy.argtypes = [C.c_void_p]
    lib.hs_map_result_destroy.restype = None
    lib.hs_map_result_destroy.argtypes = [C.POINTER(MapResult)]
    lib.hs_map_index_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MapParams), C.POINTER(C.c_void_p)]
    lib.hs_map_index_download.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hs_map_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.POINTER(MapResult))]
    lib.hs_map_to_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                    C.POINTER(C.POINTER(RealignRecords)), C.POINTER(C.POINTER(MapResult))]
    lib.hs_map_text.argtypes = [C.POINTER(MapResult), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)]
    lib.hs_map_split_params_default.restype = MapSplitParams
    lib.hs_map_segments_destroy.restype = None
    lib.hs_map_segments_destroy.argtypes = [C.POINTER(MapSegments)]
    lib.hs_map_reads_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MapSplitParams), C.POINTER(C.POINTER(MapSegments))]
    lib.hs_map_split_to_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MapSplitParams),
                                          C.POINTER(C.c_void_p), C.POINTER(C.POINTER(RealignRecords)), C.POINTER(C.POINTER(MapSegments))]
    lib.hs_map_segments_text.argtypes = [C.POINTER(MapSegments), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)]
    lib.hs_map_anchor_params_default.restype = MapAnchorParams
    lib.hs_map_anchors_destroy.restype = None
    lib.hs_map_anchors_destroy.argtypes = [C.POINTER(MapAnchors)]
    lib.hs_map_reads_anchored.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MapAnchorParams), C.POINTER(C.POINTER(MapResult)), C.POINTER(C.POINTER(MapAnchors))]
    lib.hs_realign_intervals_anchored.argtypes = ([C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32, C.c_int32] + [C.c_void_p] * 3
                                                  + [C.POINTER(C.POINTER(RealignRecords)), C.POINTER(C.c_void_p)])
    lib.hs_map_to_batch_anchored.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MapAnchorParams), C.POINTER(C.c_void_p),
                                             C.POINTER(C.POINTER(RealignRecords)), C.POINTER(C.POINTER(MapResult)), C.POINTER(C.POINTER(MapAnchors))]
    _lib = lib
    return lib


def host_waits():
    """number of host waits for the device since the library was loaded"""
    n = C.c_int64(0); ms = C.c_double(0)
    lib = load()
    lib.hs_host_wait_stats.restype = None
    lib.hs_host_wait_stats(C.byref(n), C.byref(ms))
    return int(n.value)


def kernel_stats_reset():
    load().hs_kernel_stats_reset()


def kernel_stats_every(n: int):
    """Timing events on every n-th pipeline step only (counted from this call; 1 = every step, the default): hs_kernel_stats_every"""
    load().hs_kernel_stats_every(C.c_int32(int(n)))


def kernel_stats():
    """{kernel name: {"ms": summed launch durations (HIP events on the launch stream), "launches": n, "bytes": summed algorithmic bytes}}
    of everything the stage drivers launched since kernel_stats_reset()"""
    lib = load()
    st = KernelStats()
    lib.hs_kernel_stats_get(C.byref(st))
    out = {}
    for k in range(HS_NKERNELS):
        if st.launches[k]:
            out[lib.hs_kernel_name(k).decode()] = {"ms": float(st.ms[k]), "launches": int(st.launches[k]), "bytes": int(st.bytes[k])}
    return out


def _check(rc: int):
    if rc != 0:
        raise HsError(f"hairsplitter_hip error {rc}: {load().hs_last_error().decode()}")


def require_gpu():
    lib = load()
    if lib.hs_device_count() <= 0:
        raise HsError("no HIP device: the HairSplitter MI355X path has no CPU fallback")


def _p(t):
    """device pointer of a torch tensor (or None)"""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _hp(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


# ------------------------------------------------------------------------------------------------
# flat batch (the layout the C ABI takes) from synth.ContigData
# ------------------------------------------------------------------------------------------------
class FlatBatch:
    """Host-side flattening of contigs + reads + alignment records (what parse_reads / parse_assembly / parse_SAM
    of the reference produce, input_output.cpp:39-536), in the C-ABI layout."""

    def __init__(self, contigs):
        cseq, coff = [], [0]
        rseq, roff = [], [0]
        rec_read, rec_pos, rec_strand, cig, cig_off = [], [], [], [], [0]
        contig_rec_off = [0]
        n_reads = 0
        for c in contigs:
            cseq.append(c.seq)
            coff.append(coff[-1] + len(c.seq))
            for r in c.reads:
                rseq.append(r)
                roff.append(roff[-1] + len(r))
            for a in c.alns:
                rec_read.append(n_reads + a.read)
                rec_pos.append(a.pos)
                rec_strand.append(1 if a.strand else 0)
                cig.append(a.cigar)
                cig_off.append(cig_off[-1] + len(a.cigar))
            n_reads += len(c.reads)
            contig_rec_off.append(len(rec_read))
        self.contig_seq = _np(np.concatenate(cseq) if cseq else np.zeros(0), np.uint8)
        self.contig_off = _np(coff, np.int64)
        self.read_seq = _np(np.concatenate(rseq) if rseq else np.zeros(0), np.uint8)
        self.read_off = _np(roff, np.int64)
        self.rec_read = _np(rec_read, np.int32)
        self.rec_pos = _np(rec_pos, np.int32)
        self.rec_strand = _np(rec_strand, np.uint8)
        self.rec_cig_off = _np(cig_off, np.int64)
        self.cigar = _np(np.concatenate(cig) if cig else np.zeros(0), np.uint32)
        self.contig_rec_off = _np(contig_rec_off, np.int32)
        self.n_contigs = len(contigs)
        self.n_reads = n_reads
        self.n_rec = len(rec_read)
        # derived: contig of each record, reference span, pileup offsets (same rule as hs_cv_batch_create)
        self.rec_contig = _np(np.repeat(np.arange(self.n_contigs), np.diff(self.contig_rec_off)), np.int32)
        ops = self.cigar & 0xF
        lens = (self.cigar >> 4).astype(np.int64)
        refc = np.where((ops == 0) | (ops == 2) | (ops == 7) | (ops == 8), lens, 0)
        csum = np.concatenate(([0], np.cumsum(refc)))
        span = csum[self.rec_cig_off[1:]] - csum[self.rec_cig_off[:-1]]
        L = np.diff(self.contig_off)[self.rec_contig] if self.n_rec else np.zeros(0, np.int64)
        pos = self.rec_pos.astype(np.int64)
        self.rec_refspan = _np(span, np.int64)
        qend = np.where(pos >= L, pos, np.minimum(pos + span, L))
        self.rec_qend = _np(qend, np.int32)
        self.pile_off = _np(np.concatenate(([0], np.cumsum(qend - pos))), np.int64)
        self.aligned_bp = int(self.pile_off[-1])


    _ARRAYS = ("contig_seq", "contig_off", "read_seq", "read_off", "rec_read", "rec_pos", "rec_strand", "rec_cig_off", "cigar", "contig_rec_off",
               "rec_contig", "rec_refspan", "rec_qend", "pile_off")

    def save(self, path: str):
        """the flat arrays as one .npz (a job generated in one process, run in another)"""
        np.savez(path, **{k: getattr(self, k) for k in self._ARRAYS})

    @classmethod
    def load(cls, path: str) -> "FlatBatch":
        o = object.__new__(cls)
        with np.load(path) as z:
            for k in cls._ARRAYS:
                setattr(o, k, np.ascontiguousarray(z[k]))
        o.n_contigs = len(o.contig_off) - 1
        o.n_reads = len(o.read_off) - 1
        o.n_rec = len(o.rec_read)
        o.aligned_bp = int(o.pile_off[-1])
        return o


class CvBatch:
    """hs_cv_batch: a FlatBatch resident in HBM."""

    def __init__(self, flat: FlatBatch):
        require_gpu()
        lib = load()
        self.flat = flat
        h = C.c_void_p()
        import time
        t0 = time.perf_counter()
        _check(lib.hs_cv_batch_create(_hp(flat.contig_seq, C.c_uint8), _hp(flat.contig_off, C.c_int64), C.c_int32(flat.n_contigs),
                                      _hp(flat.read_seq, C.c_uint8), _hp(flat.read_off, C.c_int64), C.c_int32(flat.n_reads),
                                      _hp(flat.rec_read, C.c_int32), _hp(flat.rec_pos, C.c_int32), _hp(flat.rec_strand, C.c_uint8),
                                      _hp(flat.rec_cig_off, C.c_int64), _hp(flat.cigar, C.c_uint32),
                                      _hp(flat.contig_rec_off, C.c_int32), C.byref(h)))
        self.create_s = time.perf_counter() - t0      # host buffers -> HBM + the launch plans (CIGAR spans, tile plan, pileup tasks)
        self.handle = h

    @property
    def aligned_bp(self) -> int:
        return int(load().hs_cv_batch_aligned_bp(self.handle))

    def set_ploidy(self, ploidy: Optional[Sequence[int]]):
        """Ploidy of every contig (0 = none) for the in-memory stage 3 -> 4 paths (run_pipeline, PipelineGroups.run): what the
        <ploidy_of_contigs> file is to HS_separate_reads. None clears it."""
        if ploidy is None:
            _check(load().hs_cv_batch_set_ploidy(self.handle, None))
            return
        p = np.ascontiguousarray(ploidy, dtype=np.int32)
        assert p.size == self.flat.n_contigs
        _check(load().hs_cv_batch_set_ploidy(self.handle, _hp(p, C.c_int32)))

    def run(self, automatic_snp_threshold: float = 0.33, n_threads: int = 0) -> Dict:
        """Stage 3 on the resident batch == HS_call_variants without the file I/O (call_variants.cpp:1276-1381)."""
        lib = load()
        res = C.POINTER(CvResult)()
        _check(lib.hs_cv_run(self.handle, C.c_float(automatic_snp_threshold), C.c_int32(n_threads), C.byref(res)))
        r = res.contents
        Cn = r.n_contigs
        snp_off = np.ctypeslib.as_array(r.snp_off, (Cn + 1,)).copy()
        S = int(snp_off[-1])
        col_off = np.ctypeslib.as_array(r.col_off, (S + 1,)).copy()
        E = int(col_off[-1])
        out = {
            "mean_distance": np.ctypeslib.as_array(r.mean_distance, (Cn,)).copy() if Cn else np.zeros(0, np.float32),
            "depth": np.ctypeslib.as_array(r.depth, (Cn,)).copy() if Cn else np.zeros(0, np.float32),
            "snp_off": snp_off,
            "snp_pos": np.ctypeslib.as_array(r.snp_pos, (max(S, 1),))[:S].copy(),
            "snp_ref": np.ctypeslib.as_array(r.snp_ref, (max(S, 1),))[:S].copy(),
            "snp_alt": np.ctypeslib.as_array(r.snp_alt, (max(S, 1),))[:S].copy(),
            "col_off": col_off,
            "col_idx": np.ctypeslib.as_array(r.col_idx, (max(E, 1),))[:E].copy(),
            "col_code": np.ctypeslib.as_array(r.col_code, (max(E, 1),))[:E].copy(),
            "error_rate": float(r.error_rate),
            "t_device_ms": float(r.t_device_ms), "t_host_ms": float(r.t_host_ms),
            "t_kernel_ms": [float(x) for x in r.t_kernel_ms],
            "n_columns_extracted": int(r.n_columns_extracted), "n_columns_downloaded": int(r.n_columns_downloaded),
            "n_columns_downloaded_late": int(r.n_columns_downloaded_late),
        }
        lib.hs_cv_result_destroy(res)
        return out

    def run_pipeline(self, automatic_snp_threshold: float = 0.33, n_threads: int = 0, error_rate_fn=None,
                     rarest_strain_abundance: float = 0.01, low_memory: bool = False, amplicon: bool = False, seed: int = 12345,
                     window_size: int = 0):
        """Stage 3 then stage 4 in-process on the resident batch (hs_cv_run -> hs_sr_run_cv): no .col text round trip.
        `error_rate_fn(cv_dict)` maps the stage-3 result to the error rate handed to stage 4 (default: what
        hairsplitter.py does with error_rate.txt: 6 significant digits, capped at 0.15)."""
        lib = load()
        res = C.POINTER(CvResult)()
        _check(lib.hs_cv_run(self.handle, C.c_float(automatic_snp_threshold), C.c_int32(n_threads), C.byref(res)))
        try:
            r = res.contents
            Cn = r.n_contigs
            cv = {"mean_distance": np.ctypeslib.as_array(r.mean_distance, (max(Cn, 1),))[:Cn].copy(), "error_rate": float(r.error_rate),
                  "n_snps": int(np.ctypeslib.as_array(r.snp_off, (Cn + 1,))[-1]),
                  "t_device_ms": float(r.t_device_ms), "t_host_ms": float(r.t_host_ms), "t_kernel_ms": [float(x) for x in r.t_kernel_ms], "t_kernel_k4_ms": float(r.t_kernel_k4_ms),
                  "n_columns_extracted": int(r.n_columns_extracted), "n_columns_downloaded": int(r.n_columns_downloaded),
                  "n_columns_downloaded_late": int(r.n_columns_downloaded_late)}
            e = error_rate_fn(cv) if error_rate_fn is not None else stage4_error_rate(cv["error_rate"])
            sres = C.POINTER(SrResult)()
            _check(lib.hs_sr_run_cv(self.handle, res, C.c_float(e), C.c_float(rarest_strain_abundance), C.c_int32(1 if low_memory else 0),
                                    C.c_int32(1 if amplicon else 0), C.c_uint32(seed), C.c_int32(n_threads), C.c_int32(window_size),
                                    C.byref(sres)))
            sr = _sr_result_to_dict(sres, Cn)
            lib.hs_sr_result_destroy(sres)
        finally:
            lib.hs_cv_result_destroy(res)
        return cv, sr

    # -- the two halves of run_pipeline, for callers that drive several batches concurrently (run_pipeline_groups) --
    def _cv(self, automatic_snp_threshold, n_threads):
        lib = load()
        res = C.POINTER(CvResult)()
        _check(lib.hs_cv_run(self.handle, C.c_float(automatic_snp_threshold), C.c_int32(n_threads), C.byref(res)))
        r = res.contents
        Cn = r.n_contigs
        cv = {"mean_distance": np.ctypeslib.as_array(r.mean_distance, (max(Cn, 1),))[:Cn].copy(), "error_rate": float(r.error_rate),
              "n_snps": int(np.ctypeslib.as_array(r.snp_off, (Cn + 1,))[-1]),
              "t_device_ms": float(r.t_device_ms), "t_host_ms": float(r.t_host_ms), "t_kernel_ms": [float(x) for x in r.t_kernel_ms], "t_kernel_k4_ms": float(r.t_kernel_k4_ms),
                  "n_columns_extracted": int(r.n_columns_extracted), "n_columns_downloaded": int(r.n_columns_downloaded),
                  "n_columns_downloaded_late": int(r.n_columns_downloaded_late)}
        return res, cv

    def _sr(self, res, e, n_threads, rarest_strain_abundance, low_memory, amplicon, seed, window_size):
        lib = load()
        try:
            sres = C.POINTER(SrResult)()
            _check(lib.hs_sr_run_cv(self.handle, res, C.c_float(e), C.c_float(rarest_strain_abundance), C.c_int32(1 if low_memory else 0),
                                    C.c_int32(1 if amplicon else 0), C.c_uint32(seed), C.c_int32(n_threads), C.c_int32(window_size),
                                    C.byref(sres)))
            sr = _sr_result_to_dict(sres, res.contents.n_contigs)
            lib.hs_sr_result_destroy(sres)
        finally:
            lib.hs_cv_result_destroy(res)
        return sr

    @classmethod
    def _adopt(cls, handle, create_s, records=None) -> "CvBatch":
        """a batch the library made itself (no FlatBatch behind it: `flat` is None, `records` what it was made from)"""
        o = object.__new__(cls)
        o.flat = None
        o.handle = handle
        o.create_s = create_s
        o.records = records
        return o

    @classmethod
    def from_paf(cls, gfa: str, reads: str, paf: str, n_threads: int = 0) -> "CvBatch":
        """hs_cv_batch_create_paf: the files of hs_realign_paf -> a resident batch. Every PAF line's read segment is cut, aligned against
        its contig window and turned into CIGAR words on the device; no SAM in between. `records` holds the records and the phase times."""
        import time
        require_gpu()
        lib = load()
        h = C.c_void_p(); r = C.POINTER(RealignRecords)()
        t0 = time.perf_counter()
        _check(lib.hs_cv_batch_create_paf(gfa.encode(), reads.encode(), paf.encode(), C.c_int32(n_threads), C.byref(h), C.byref(r)))
        dt = time.perf_counter() - t0
        try:
            rec = _realign_records_to_dict(r)
        finally:
            lib.hs_realign_records_destroy(r)
        return cls._adopt(h, dt, rec)

    @classmethod
    def from_sam(cls, gfa: str, reads: str, sam: str, n_threads: int = 0) -> "CvBatch":
        """hs_cv_batch_create_sam: the three files of HS_call_variants -> a resident batch (its parser, then hs_cv_batch_create)"""
        import time
        require_gpu()
        h = C.c_void_p()
        t0 = time.perf_counter()
        _check(load().hs_cv_batch_create_sam(gfa.encode(), reads.encode(), sam.encode(), C.c_int32(n_threads), C.byref(h)))
        return cls._adopt(h, time.perf_counter() - t0)

    def close(self):
        if self.handle:
            load().hs_cv_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RealignRecords(C.Structure):
    _fields_ = [("n_intervals", C.c_int32), ("n_rec", C.c_int32), ("n_contigs", C.c_int32), ("contig_rec_off", C.POINTER(C.c_int32)),
                ("rec_interval", C.POINTER(C.c_int32)), ("rec_read", C.POINTER(C.c_int32)), ("rec_pos", C.POINTER(C.c_int32)), ("rec_dist", C.POINTER(C.c_int32)),
                ("rec_strand", C.POINTER(C.c_uint8)), ("rec_cig_off", C.POINTER(C.c_int64)), ("cigar", C.POINTER(C.c_uint32)),
                ("n_dropped", C.c_int64), ("dropped", C.POINTER(C.c_int32)),
                ("t_cut_ms", C.c_double), ("t_align_ms", C.c_double), ("t_cigar_ms", C.c_double), ("t_download_ms", C.c_double),
                ("n_rounds", C.c_int64), ("move_bytes", C.c_int64), ("cigar_words", C.c_int64), ("n_pieces", C.c_int64), ("t_join_ms", C.c_double)]


def _realign_records_to_dict(res) -> Dict:
    r = res.contents
    arr = lambda p, n: np.ctypeslib.as_array(p, (max(int(n), 1),))[:int(n)].copy()
    n = r.n_rec
    off = arr(r.rec_cig_off, n + 1)
    return {"n_intervals": int(r.n_intervals), "n_rec": int(n), "n_contigs": int(r.n_contigs), "contig_rec_off": arr(r.contig_rec_off, r.n_contigs + 1),
            "rec_interval": arr(r.rec_interval, n), "rec_read": arr(r.rec_read, n), "rec_pos": arr(r.rec_pos, n), "rec_dist": arr(r.rec_dist, n),
            "rec_strand": arr(r.rec_strand, n), "rec_cig_off": off, "cigar": arr(r.cigar, off[-1]), "n_dropped": int(r.n_dropped), "dropped": arr(r.dropped, r.n_dropped),
            "t_cut_ms": float(r.t_cut_ms), "t_align_ms": float(r.t_align_ms), "t_cigar_ms": float(r.t_cigar_ms), "t_download_ms": float(r.t_download_ms),
            "n_rounds": int(r.n_rounds), "move_bytes": int(r.move_bytes), "cigar_words": int(r.cigar_words), "n_pieces": int(r.n_pieces), "t_join_ms": float(r.t_join_ms)}


class CvSelection(C.Structure):
    _fields_ = [("n_selected", C.c_int64), ("t_kernel_ms", C.c_float * 4), ("t_device_ms", C.c_double), ("t_host_ms", C.c_double),
                ("impl", C.c_void_p)]


class PipelineStats(C.Structure):
    _fields_ = [("n_snps", C.c_int64), ("n_cw_instances", C.c_int64), ("n_graph_rows_host", C.c_int64),
                ("t_device_ms", C.c_double), ("t_host_ms", C.c_double), ("t_kernel_cv_ms", C.c_float * 4), ("t_kernel_k4_ms", C.c_float),
                ("t_kernel_sr_ms", C.c_float * 4), ("t_kernel_graph_ms", C.c_float),
                ("n_columns_extracted", C.c_int64), ("n_columns_downloaded", C.c_int64), ("n_columns_downloaded_late", C.c_int64),
                ("n_cw_sweeps", C.c_int64), ("cw_bytes", C.c_int64), ("graph_nnz", C.c_int64), ("n_graph_rows", C.c_int64), ("simdiff_bytes", C.c_int64)]


class PipelineGroups:
    """One resident batch whose contigs are processed as G consecutive groups (hs_pipeline_*). The streaming kernels (CIGAR scan,
    pileup, column statistics) run ONCE over the whole batch; everything after them runs per group, one persistent host
    thread and one HIP stream per group inside the library, so that the sequential host sections and device waits of one group
    overlap the work of the others. Contigs are independent in both stages (call_variants.cpp:1280, separate_reads.cpp:1508);
    the one cross-contig quantity, the error rate, is formed between the stages over ALL contigs in contig order, exactly as
    for a single call."""

    def __init__(self, contigs, n_groups):
        self.flat = contigs if isinstance(contigs, FlatBatch) else FlatBatch(contigs)
        self.batch = CvBatch(self.flat)
        self.handle = C.c_void_p()
        _check(load().hs_pipeline_create(self.batch.handle, C.c_int32(n_groups), C.byref(self.handle)))
        self.aligned_bp = self.flat.aligned_bp
        self.total_len = int(self.flat.contig_off[-1])
        self._owns_batch = True

    def keep_columns(self, on=True):
        """HS_PIPELINE_KEEP_COLUMNS: the entries of the SNP columns (.col's payload) are brought to the host inside every call too"""
        _check(load().hs_pipeline_set_option(self.handle, C.c_int32(1), C.c_int64(1 if on else 0)))

    def sparse_labels(self, on=True):
        """HS_PIPELINE_SPARSE_LABELS: results carry sr["sparse"] = (win_row_off, ids, labels) -- per window the reads it holds and their
        labels, what the .gro lists -- instead of the dense array sr["labels"] (None then). The arrays view the pipeline's memory and
        stay valid until its next call."""
        _check(load().hs_pipeline_set_option(self.handle, C.c_int32(2), C.c_int64(1 if on else 0)))
        self._sparse = bool(on)

    def alleles(self, on=True):
        """HS_PIPELINE_ALLELES: every call also returns sr["alleles"], the allele table of the call (a copy), formed by every contig group at the
        end of its own chain from the SNP columns on the device. HS_PIPELINE_KEEP_COLUMNS is not needed."""
        _check(load().hs_pipeline_set_option(self.handle, C.c_int32(4), C.c_int64(1 if on else 0)))
        self._alleles = bool(on)

    def recruits(self, on=True, params=None):
        """HS_PIPELINE_RECRUIT: every call also returns sr["recruits"], the recruit table of the call (a copy): every contig group crosses its
        windows' unlabelled reads with its allele cells on the device. params: a dict as recruit_params() gives it (None: what the pipeline
        has -- the defaults at first). The allele table comes along only under alleles(True)."""
        if params is not None:
            _check(load().hs_pipeline_set_recruit_params(self.handle, C.byref(_recruit_params(params))))
        _check(load().hs_pipeline_set_option(self.handle, C.c_int32(8), C.c_int64(1 if on else 0)))
        self._recruits = bool(on)

    def _attach_sparse(self, sr):
        if getattr(self, "_recruits", False):
            tb = load().hs_pipeline_recruits(self.handle)
            if not tb:
                raise HsError("hs_pipeline_recruits: no table")
            sr["recruits"] = _recruit_table_to_dict(tb)
        if getattr(self, "_alleles", False):
            tb = load().hs_pipeline_alleles(self.handle)
            if not tb:
                raise HsError("hs_pipeline_alleles: no table")
            sr["alleles"] = _allele_table_to_dict(tb)
        if not getattr(self, "_sparse", False):
            return sr
        off, ids, lab = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        nw, nr = C.c_int64(0), C.c_int64(0)
        _check(load().hs_pipeline_sparse_labels(self.handle, C.byref(off), C.byref(ids), C.byref(lab), C.byref(nw), C.byref(nr)))
        W, R = int(nw.value), int(nr.value)
        if R == 0:      # (an empty std::vector's data() may be NULL)
            sr["sparse"] = (np.ctypeslib.as_array(off, (W + 1,)), np.zeros(0, np.int32), np.zeros(0, np.int32))
            return sr
        sr["sparse"] = (np.ctypeslib.as_array(off, (W + 1,)), np.ctypeslib.as_array(ids, (R,)), np.ctypeslib.as_array(lab, (R,)))
        return sr

    def sibling(self, n_groups):
        """Another pipeline over the SAME resident batch with its own number of contig groups (bench.py: one group, where every
        kernel runs alone, to read the kernels' own durations next to those of the default run)."""
        o = object.__new__(PipelineGroups)
        o.flat, o.batch, o.aligned_bp, o.total_len = self.flat, self.batch, self.aligned_bp, self.total_len
        o.handle = C.c_void_p()
        o._owns_batch = False      # (the batch belongs to the pipeline it was made from: close() of the sibling leaves it alone)
        _check(load().hs_pipeline_create(self.batch.handle, C.c_int32(n_groups), C.byref(o.handle)))
        return o

    def run(self, automatic_snp_threshold=0.33, n_threads=0, error_rate_fn=None, rarest_strain_abundance=0.01, low_memory=False,
            amplicon=False, seed=12345, window_size=0):
        import time
        lib = load()
        Cn = self.flat.n_contigs
        md = np.zeros(max(Cn, 1), np.float32)
        st = PipelineStats()
        t_0 = time.perf_counter()
        _check(lib.hs_pipeline_select(self.handle, _hp(md, C.c_float), C.byref(st)))
        t_1 = time.perf_counter()
        md = md[:Cn]
        # call_variants.cpp:1312-1315,1377: float sum in contig order / number of contigs with a positive distance
        cv = {"mean_distance": md, "error_rate": mean_of_positive_f32(md)}
        e = error_rate_fn(cv) if error_rate_fn is not None else stage4_error_rate(cv["error_rate"])
        sres = C.POINTER(SrResult)()   # window_size <= 0: hs_pipeline_run chooses it over the whole batch (same rule as self.window_size())
        t_2 = time.perf_counter()
        _check(lib.hs_pipeline_run(self.handle, C.c_float(automatic_snp_threshold), C.c_float(e), C.c_float(rarest_strain_abundance),
                                   C.c_int32(1 if low_memory else 0), C.c_int32(1 if amplicon else 0), C.c_uint32(seed), C.c_int32(n_threads),
                                   C.c_int32(window_size), C.byref(sres), C.byref(st)))
        t_3 = time.perf_counter()
        cv.update({"n_snps": int(st.n_snps), "t_device_ms": float(st.t_device_ms), "t_host_ms": float(st.t_host_ms),
                   "t_kernel_ms": [float(x) for x in st.t_kernel_cv_ms], "t_kernel_k4_ms": float(st.t_kernel_k4_ms),
                   "n_columns_extracted": int(st.n_columns_extracted), "n_columns_downloaded": int(st.n_columns_downloaded),
                   "n_columns_downloaded_late": int(st.n_columns_downloaded_late)})
        sr = self._attach_sparse(_sr_result_to_dict(sres, Cn, take_ownership=True))   # the labels stay where the library put them
        sr["wall_ms"] = {"select": (t_1 - t_0) * 1e3, "between": (t_2 - t_1) * 1e3, "groups": (t_3 - t_2) * 1e3, "collect": (time.perf_counter() - t_3) * 1e3}
        return cv, sr

    def run_fused(self, automatic_snp_threshold=0.33, n_threads=0, rarest_strain_abundance=0.01, low_memory=False, amplicon=False, seed=12345,
                  window_size=0):
        """hs_pipeline_run_fused: the same job in one library call (single process: the error rate is formed inside)"""
        import time
        lib = load()
        Cn = self.flat.n_contigs
        md = np.zeros(max(Cn, 1), np.float32)
        st = PipelineStats()
        er = C.c_float(0)
        sres = C.POINTER(SrResult)()
        t_0 = time.perf_counter()
        _check(lib.hs_pipeline_run_fused(self.handle, C.c_float(automatic_snp_threshold), C.c_float(rarest_strain_abundance), C.c_int32(1 if low_memory else 0),
                                         C.c_int32(1 if amplicon else 0), C.c_uint32(seed), C.c_int32(n_threads), C.c_int32(window_size), _hp(md, C.c_float),
                                         C.byref(er), C.byref(sres), C.byref(st)))
        t_1 = time.perf_counter()
        cv = {"mean_distance": md[:Cn], "error_rate": float(er.value), "error_rate_is_final": True, "n_snps": int(st.n_snps), "t_device_ms": float(st.t_device_ms),
              "t_host_ms": float(st.t_host_ms), "t_kernel_ms": [float(x) for x in st.t_kernel_cv_ms], "t_kernel_k4_ms": float(st.t_kernel_k4_ms),
              "n_columns_extracted": int(st.n_columns_extracted), "n_columns_downloaded": int(st.n_columns_downloaded),
              "n_columns_downloaded_late": int(st.n_columns_downloaded_late)}
        sr = self._attach_sparse(_sr_result_to_dict(sres, Cn, take_ownership=True))
        sr["wall_ms"] = {"select": 0.0, "between": 0.0, "groups": (t_1 - t_0) * 1e3, "collect": (time.perf_counter() - t_1) * 1e3}
        return cv, sr

    def window_size(self, amplicon=False):
        """choose_window_size over the whole job (separate_reads.cpp:1466-1498): it depends on every read of every contig.
        READ limits are (POS-1, POS + reference span) (input_output.cpp:503-511), the length sum is a wrapping int."""
        f = self.flat
        if amplicon:
            return int(np.diff(f.contig_off).max()) if f.n_contigs else 0
        return window_size_from_counts(*window_size_counts(f.rec_refspan + 2))

    def close(self):
        if self.handle:
            load().hs_pipeline_destroy(self.handle)
            self.handle = None
        if getattr(self, "_owns_batch", True):
            self.batch.close()


class _SrResultOwner:
    """Frees an hs_sr_result when the last array that views its memory is gone"""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            load().hs_sr_result_destroy(self.res)
        except Exception:
            pass


class _SrTaps(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("win_contig", C.POINTER(C.c_int32)), ("win_start", C.POINTER(C.c_int32)), ("win_row0", C.POINTER(C.c_int64)),
                ("mask_ids", C.POINTER(C.c_int32)), ("run_begin", C.POINTER(C.c_int64)), ("run_snp", C.POINTER(C.c_int32)), ("run_off", C.POINTER(C.c_int64)),
                ("run_labels", C.POINTER(C.c_int32)), ("third", C.POINTER(C.c_int32)),
                ("g_n_windows", C.c_int32), ("g_win_contig", C.POINTER(C.c_int32)), ("g_win_kind", C.POINTER(C.c_int32)), ("g_win_row0", C.POINTER(C.c_int64)),
                ("g_mask_ids", C.POINTER(C.c_int32)), ("g_nbr_off", C.POINTER(C.c_int64)), ("g_nbr", C.POINTER(C.c_int32)), ("g_n_contigs", C.c_int32),
                ("g_plane_n", C.POINTER(C.c_int32)), ("g_words", C.POINTER(C.c_int32)), ("g_plane_off", C.POINTER(C.c_int64)), ("g_alt", C.POINTER(C.c_uint64)),
                ("g_ref", C.POINTER(C.c_uint64)), ("g_n_reads", C.POINTER(C.c_int32)), ("g_out_off", C.POINTER(C.c_int64)), ("g_read_base", C.POINTER(C.c_int64)),
                ("g_pos_orig", C.POINTER(C.c_int32)), ("g_n_pos_orig", C.c_int64), ("g_n_plane_words", C.c_int64), ("g_n_pairs", C.c_int64),
                ("g_matrix", C.POINTER(C.c_int32)), ("g_rows_on_host", C.c_int64), ("g_rows_late", C.c_int64), ("g_row_waves", C.c_int32),
                ("all_lanes", C.c_int32), ("cap_tail", C.c_int32), ("runs_lanes", C.c_int64), ("runs_overflow", C.c_int64), ("runs_rows", C.c_int64),
                ("units_rows", C.c_int64), ("runs_wave", C.c_int64), ("runs_wave_scratch", C.c_int64), ("tail_narrow", C.c_int64), ("tail_lds", C.c_int64),
                ("tail_scratch", C.c_int64)]


SR_ROUTE_COUNTERS = ("all_lanes", "runs_lanes", "runs_overflow", "runs_rows", "units_rows", "runs_wave", "runs_wave_scratch", "tail_narrow", "tail_lds",
                     "tail_scratch", "cap_tail")


SR_TAP_SENTINEL = -2 ** 31      # HS_SR_TAP_SENTINEL


def _sr_run_taps_fn(lib):
    lib.hs_sr_run_taps.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.POINTER(SrResult)),
                                   C.POINTER(C.POINTER(_SrTaps))]
    lib.hs_sr_taps_destroy.argtypes = [C.POINTER(_SrTaps)]; lib.hs_sr_taps_destroy.restype = None
    return lib.hs_sr_run_taps


def _graph_taps_to_dict(t):
    a = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, (max(n, 1),))[:n].astype(dt).copy()
    W, Cn = int(t.g_n_windows), int(t.g_n_contigs)
    row0 = a(t.g_win_row0, W + 1, np.int64)
    rows = int(row0[-1])
    noff = a(t.g_nbr_off, rows + 1, np.int64)
    return {"win_contig": a(t.g_win_contig, W, np.int32), "win_kind": a(t.g_win_kind, W, np.int32), "win_row0": row0, "mask_ids": a(t.g_mask_ids, rows, np.int32),
            "nbr_off": noff, "nbr": a(t.g_nbr, int(noff[-1]), np.int32),
            "plane_n": a(t.g_plane_n, Cn, np.int32), "words": a(t.g_words, Cn, np.int32), "plane_off": a(t.g_plane_off, Cn, np.int64),
            "alt": a(t.g_alt, int(t.g_n_plane_words), np.uint64), "ref": a(t.g_ref, int(t.g_n_plane_words), np.uint64),
            "n_reads": a(t.g_n_reads, Cn, np.int32), "out_off": a(t.g_out_off, Cn, np.int64), "read_base": a(t.g_read_base, Cn, np.int64),
            "pos_orig": a(t.g_pos_orig, int(t.g_n_pos_orig), np.int32), "matrix": a(t.g_matrix, 2 * int(t.g_n_pairs), np.int32).reshape(-1, 2),
            "rows_on_host": int(t.g_rows_on_host), "rows_late": int(t.g_rows_late), "row_waves": int(t.g_row_waves)}


def _sr_contig_array(contigs):
    """per-contig dicts (length, read_start, read_end, snp_pos, snp_ref, snp_alt, col_off, col_idx, col_code) -> (hs_sr_contig array, the numpy
    buffers it points into: keep them alive for the call)"""
    Cn = len(contigs)
    arr = (SrContig * max(Cn, 1))()
    keep = []
    for c, ctg in enumerate(contigs):
        rs, re = _np(ctg["read_start"], np.int32), _np(ctg["read_end"], np.int32)
        sp, sr, sa = _np(ctg["snp_pos"], np.int32), _np(ctg["snp_ref"], np.uint8), _np(ctg["snp_alt"], np.uint8)
        co, ci, cc = _np(ctg["col_off"], np.int64), _np(ctg["col_idx"], np.int32), _np(ctg["col_code"], np.uint8)
        if len(ci) == 0:
            ci, cc = np.zeros(1, np.int32), np.zeros(1, np.uint8)
        keep += [rs, re, sp, sr, sa, co, ci, cc]
        a = arr[c]
        a.length = int(ctg["length"]); a.n_reads = len(rs); a.n_snps = len(sp)
        a.read_start = _hp(rs, C.c_int32); a.read_end = _hp(re, C.c_int32)
        a.snp_pos = _hp(sp, C.c_int32); a.snp_ref = _hp(sr, C.c_uint8); a.snp_alt = _hp(sa, C.c_uint8)
        a.col_off = _hp(co, C.c_int64); a.col_idx = _hp(ci, C.c_int32); a.col_code = _hp(cc, C.c_uint8)
        a.ploidy = 0
    return arr, keep


def separate_reads_graph_taps(contigs: Sequence[Dict], window_size: int, error_rate: float, low_memory: bool = False, seed: int = 12345,
                              n_threads: int = 0) -> Dict:
    """hs_sr_run_taps in its graphs mode on stage-4 inputs given directly: one dict per contig with length, read_start, read_end, snp_pos, snp_ref,
    snp_alt, col_off, col_idx, col_code (what separate_reads(taps=...) leaves in out["contigs"]). The call runs hs_sr_run's own code up to the read
    graphs and returns what its kernels left (include/hairsplitter_hip.h: the g_ fields of hs_sr_taps); there is no clustering and no result."""
    require_gpu()
    lib = load()
    Cn = len(contigs)
    arr, keep = _sr_contig_array(contigs)
    res = C.POINTER(SrResult)()
    tp = C.POINTER(_SrTaps)()
    _check(_sr_run_taps_fn(lib)(C.cast(arr, C.c_void_p), C.c_int32(Cn), C.c_int32(int(window_size)), C.c_float(error_rate), C.c_int32(1 if low_memory else 0),
                                C.c_uint32(seed), C.c_int32(n_threads), C.c_int32(1), C.byref(res), C.byref(tp)))
    out = _graph_taps_to_dict(tp.contents)
    lib.hs_sr_taps_destroy(tp)
    return out


def _chain_taps_to_dict(t):
    a = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, (max(n, 1),))[:n].astype(dt).copy()
    Wc = int(t.n_windows)
    row0 = a(t.win_row0, Wc + 1, np.int64); rb = a(t.run_begin, Wc + 1, np.int64)
    n_runs = int(rb[-1]); ro = a(t.run_off, n_runs + 1, np.int64)
    out = {"win_contig": a(t.win_contig, Wc, np.int32), "win_start": a(t.win_start, Wc, np.int32), "win_row0": row0, "mask_ids": a(t.mask_ids, int(row0[-1]), np.int32),
           "run_begin": rb, "run_snp": a(t.run_snp, n_runs, np.int32), "run_off": ro, "run_labels": a(t.run_labels, int(ro[-1]), np.int32),
           "third": a(t.third, int(row0[-1]), np.int32)}
    for k in SR_ROUTE_COUNTERS:      # which kernel took which run / window (include/hairsplitter_hip.h)
        out[k] = int(getattr(t, k))
    return out


def separate_reads_chain_taps(contigs: Sequence[Dict], window_size: int, error_rate: float, low_memory: bool = False, seed: int = 12345,
                              n_threads: int = 0) -> Dict:
    """hs_sr_run_taps in its chain mode on stage-4 inputs given directly (per-contig dicts as separate_reads_graph_taps takes them): the result
    dict of the call plus "taps", as separate_reads(taps=True) returns them."""
    require_gpu()
    lib = load()
    Cn = len(contigs)
    arr, keep = _sr_contig_array(contigs)
    res = C.POINTER(SrResult)()
    tp = C.POINTER(_SrTaps)()
    _check(_sr_run_taps_fn(lib)(C.cast(arr, C.c_void_p), C.c_int32(Cn), C.c_int32(int(window_size)), C.c_float(error_rate), C.c_int32(1 if low_memory else 0),
                                C.c_uint32(seed), C.c_int32(n_threads), C.c_int32(0), C.byref(res), C.byref(tp)))
    out = _sr_result_to_dict(res, Cn)
    out["window_size"] = int(window_size)
    lib.hs_sr_result_destroy(res)
    out["taps"] = _chain_taps_to_dict(tp.contents)
    lib.hs_sr_taps_destroy(tp)
    return out


def _sr_result_to_dict(res, Cn, take_ownership=False):
    """take_ownership: the labels (tens of MB per batch) are returned as a view of the C result instead of a copy; the
    result is destroyed when that array (and every view of it) is gone, and the caller must not destroy it."""
    r = res.contents
    win_off = np.ctypeslib.as_array(r.win_off, (Cn + 1,)).copy()
    W = int(win_off[-1])
    label_off = np.ctypeslib.as_array(r.label_off, (W + 1,)).copy()
    NL = int(label_off[-1])
    return {
        "win_off": win_off,
        "win_start": np.ctypeslib.as_array(r.win_start, (max(W, 1),))[:W].copy(),
        "win_end": np.ctypeslib.as_array(r.win_end, (max(W, 1),))[:W].copy(),
        "label_off": label_off,
        "labels": (None if not r.labels else (_owned_view_i32(res, r.labels, NL) if take_ownership else np.ctypeslib.as_array(r.labels, (max(NL, 1),))[:NL].copy())),
        "_owner": (_SrResultOwner(res) if (take_ownership and not r.labels) else None),      # (no label array to carry the ownership: the dict does)
        "t_device_ms": float(r.t_device_ms), "t_host_ms": float(r.t_host_ms), "n_cw_instances": int(r.n_cw_instances),
        "t_kernel_ms": [float(x) for x in r.t_kernel_ms], "t_kernel_graph_ms": float(r.t_kernel_graph_ms),
        "n_graph_rows_host": int(r.n_graph_rows_host), "n_windows_finished_on_host": int(r.n_windows_finished_on_host),
        "n_cw_sweeps": int(r.n_cw_sweeps), "cw_bytes": int(r.cw_bytes), "graph_nnz": int(r.graph_nnz), "n_graph_rows": int(r.n_graph_rows),
        "simdiff_bytes": int(r.simdiff_bytes),
    }


def _owned_view_i32(res, ptr, n):
    buf = (C.c_int32 * max(n, 1)).from_address(C.addressof(ptr.contents))
    buf._hs_owner = _SrResultOwner(res)      # the ndarray's base is this ctypes array, which keeps the owner alive
    return np.ctypeslib.as_array(buf)[:n]


def separate_reads(cv_out: Dict, flat: FlatBatch, error_rate: float, low_memory: bool = False, amplicon: bool = False,
                   seed: int = 12345, n_threads: int = 0, ploidy: Optional[Sequence[int]] = None,
                   rarest_strain_abundance: float = 0.0, window_size: Optional[int] = None, taps: bool = False, alleles: bool = False,
                   recruit=False) -> Dict:
    """(recruit=True, or a dict of thresholds as recruit_params() gives it: out["recruits"] = the recruit table of the call, hs_recruit_reads
    on its labels and the SNPs it kept.)
    (alleles=True: out["alleles"] = the allele table of the call, hs_haplotype_alleles on its labels and the SNPs it kept.)
    (taps=True: through hs_sr_run_taps -- out["taps"] holds what the kernels of the clustering chain left, out["contigs"] the per-contig
    inputs as numpy arrays, for the tests. taps="graphs": the call stops behind the read graphs -- separate_reads_graph_taps on the same
    per-contig inputs; out = {"window_size", "contigs", "taps"}.)
    Stage 4 on the in-memory result of stage 3 == HS_separate_reads without the .col round trip
    (separate_reads.cpp:1440-1739). READ limits are (position_2_1, position_2_2) of the records
    (call_variants.cpp:1186-1189 -> separate_reads.cpp:176-179)."""
    require_gpu()
    lib = load()
    Cn = flat.n_contigs
    arr = (SrContig * Cn)()
    keep = []   # keep numpy buffers alive
    per_contig = []
    ops = flat.cigar & 0xF
    lens = (flat.cigar >> 4).astype(np.int64)
    refc = np.where((ops == 0) | (ops == 2) | (ops == 7) | (ops == 8), lens, 0)
    csum = np.concatenate(([0], np.cumsum(refc)))
    span = csum[flat.rec_cig_off[1:]] - csum[flat.rec_cig_off[:-1]]
    for c in range(Cn):
        r0, r1 = int(flat.contig_rec_off[c]), int(flat.contig_rec_off[c + 1])
        rs = _np(flat.rec_pos[r0:r1], np.int32)
        re = _np(flat.rec_pos[r0:r1].astype(np.int64) + 1 + span[r0:r1], np.int32)   # pos2_1 + length_contig
        s0, s1 = int(cv_out["snp_off"][c]), int(cv_out["snp_off"][c + 1])
        e0 = int(cv_out["col_off"][s0])
        snp_pos = _np(cv_out["snp_pos"][s0:s1], np.int32)
        snp_ref = _np(cv_out["snp_ref"][s0:s1], np.uint8)
        snp_alt = _np(cv_out["snp_alt"][s0:s1], np.uint8)
        col_off = _np(cv_out["col_off"][s0:s1 + 1] - e0, np.int64)
        e1 = e0 + int(col_off[-1])
        col_idx = _np(cv_out["col_idx"][e0:e1], np.int32)
        col_code = _np(cv_out["col_code"][e0:e1], np.uint8)
        if rarest_strain_abundance > 0 and s1 > s0:
            # parse_column_file drops SNPs whose second base is rarer than the threshold (separate_reads.cpp:167)
            seg = np.repeat(np.arange(s1 - s0), np.diff(col_off))
            n_ref = np.bincount(seg, weights=(col_code == snp_ref[seg]), minlength=s1 - s0)
            n_alt = np.bincount(seg, weights=(col_code == snp_alt[seg]) & (col_code != snp_ref[seg]), minlength=s1 - s0)
            keep_snp = n_alt.astype(np.float32) >= np.float32(rarest_strain_abundance) * (n_ref + n_alt).astype(np.float32)
            if not keep_snp.all():
                km = keep_snp[seg]
                lens = np.diff(col_off)[keep_snp]
                snp_pos, snp_ref, snp_alt = snp_pos[keep_snp], snp_ref[keep_snp], snp_alt[keep_snp]
                col_idx, col_code = _np(col_idx[km], np.int32), _np(col_code[km], np.uint8)
                col_off = _np(np.concatenate(([0], np.cumsum(lens))), np.int64)
                snp_pos, snp_ref, snp_alt = _np(snp_pos, np.int32), _np(snp_ref, np.uint8), _np(snp_alt, np.uint8)
                s1 = s0 + len(snp_pos)
        keep += [rs, re, snp_pos, snp_ref, snp_alt, col_off, col_idx, col_code]
        per_contig.append({"read_start": rs, "read_end": re, "snp_pos": snp_pos, "snp_ref": snp_ref, "snp_alt": snp_alt, "col_off": col_off, "col_idx": col_idx,
                           "col_code": col_code, "length": int(flat.contig_off[c + 1] - flat.contig_off[c])})
        a = arr[c]
        a.length = int(flat.contig_off[c + 1] - flat.contig_off[c])
        a.n_reads = r1 - r0
        a.read_start = _hp(rs, C.c_int32); a.read_end = _hp(re, C.c_int32)
        a.n_snps = s1 - s0
        a.snp_pos = _hp(snp_pos, C.c_int32); a.snp_ref = _hp(snp_ref, C.c_uint8); a.snp_alt = _hp(snp_alt, C.c_uint8)
        a.col_off = _hp(col_off, C.c_int64); a.col_idx = _hp(col_idx, C.c_int32); a.col_code = _hp(col_code, C.c_uint8)
        a.ploidy = int(ploidy[c]) if ploidy is not None else 0
    w = lib.hs_sr_window_size(arr, C.c_int32(Cn), C.c_int32(1 if amplicon else 0)) if window_size is None else int(window_size)
    if taps == "graphs":
        return {"window_size": int(w), "contigs": per_contig, "taps": separate_reads_graph_taps(per_contig, int(w), error_rate, low_memory, seed, n_threads)}
    res = C.POINTER(SrResult)()
    tp = C.POINTER(_SrTaps)()
    if taps:
        _check(_sr_run_taps_fn(lib)(C.cast(arr, C.c_void_p), C.c_int32(Cn), C.c_int32(w), C.c_float(error_rate), C.c_int32(1 if low_memory else 0),
                                    C.c_uint32(seed), C.c_int32(n_threads), C.c_int32(0), C.byref(res), C.byref(tp)))
    else:
        _check(lib.hs_sr_run(arr, C.c_int32(Cn), C.c_int32(w), C.c_float(error_rate), C.c_int32(1 if low_memory else 0),
                             C.c_uint32(seed), C.c_int32(n_threads), C.byref(res)))
    r = res.contents
    win_off = np.ctypeslib.as_array(r.win_off, (Cn + 1,)).copy()
    W = int(win_off[-1])
    label_off = np.ctypeslib.as_array(r.label_off, (W + 1,)).copy()
    NL = int(label_off[-1])
    out = {
        "window_size": int(w), "win_off": win_off,
        "win_start": np.ctypeslib.as_array(r.win_start, (max(W, 1),))[:W].copy(),
        "win_end": np.ctypeslib.as_array(r.win_end, (max(W, 1),))[:W].copy(),
        "label_off": label_off,
        "labels": np.ctypeslib.as_array(r.labels, (max(NL, 1),))[:NL].copy(),
        "t_device_ms": float(r.t_device_ms), "t_host_ms": float(r.t_host_ms), "n_cw_instances": int(r.n_cw_instances),
        "t_kernel_ms": [float(x) for x in r.t_kernel_ms], "t_kernel_graph_ms": float(r.t_kernel_graph_ms),
        "n_graph_rows_host": int(r.n_graph_rows_host), "n_windows_finished_on_host": int(r.n_windows_finished_on_host),
        "n_cw_sweeps": int(r.n_cw_sweeps), "cw_bytes": int(r.cw_bytes), "graph_nnz": int(r.graph_nnz), "n_graph_rows": int(r.n_graph_rows),
        "simdiff_bytes": int(r.simdiff_bytes),
    }
    if alleles:      # the allele table of the same call: its labels against the columns stage 4 just read
        tb = C.POINTER(AlleleTable)()
        _check(lib.hs_haplotype_alleles(arr, C.c_int32(Cn), res, C.byref(tb)))
        out["alleles"] = _allele_table_to_dict(tb)
        lib.hs_allele_table_destroy(tb)
    if recruit:
        rt = C.POINTER(RecruitTable)()
        prm = _recruit_params(recruit if isinstance(recruit, dict) else None)
        _check(lib.hs_recruit_reads(arr, C.c_int32(Cn), res, C.byref(prm), None, C.byref(rt)))
        out["recruits"] = _recruit_table_to_dict(rt)
        lib.hs_recruit_table_destroy(rt)
    lib.hs_sr_result_destroy(res)
    if taps:
        out["taps"] = _chain_taps_to_dict(tp.contents)
        out["contigs"] = per_contig
        lib.hs_sr_taps_destroy(tp)
    return out


# ------------------------------------------------------------------------------------------------
# per-group allele calls at every SNP (hs_allele_table)
# ------------------------------------------------------------------------------------------------
def alleles_lds_capacity() -> int:
    """entries of the deepest column the cell kernel sorts in LDS (deeper ones go through global scratch)"""
    return int(load().hs_alleles_lds_capacity())


def _table_array(ptr, n, dtype) -> np.ndarray:
    """a copy of the n elements a table's pointer field points to"""
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, (n,)).astype(dtype, copy=True)


def _allele_table_to_dict(tp) -> Dict:
    """a copy of an hs_allele_table as numpy arrays; "cells" has the dtype ALLELE_CELL"""
    t = tp.contents
    W, S, G, N = int(t.n_windows), int(t.n_snps), int(t.n_groups), int(t.n_cells)
    a = _table_array
    cells = np.zeros(N, ALLELE_CELL)
    if N:
        C.memmove(cells.ctypes.data, t.cells, N * ALLELE_CELL.itemsize)
    return {"win_contig": a(t.win_contig, W, np.int32), "win_start": a(t.win_start, W, np.int32), "win_end": a(t.win_end, W, np.int32),
            "win_group_off": a(t.win_group_off, W + 1, np.int64), "group_ids": a(t.group_ids, G, np.int32), "win_snp_off": a(t.win_snp_off, W + 1, np.int64),
            "snp_contig": a(t.snp_contig, S, np.int32), "snp_pos": a(t.snp_pos, S, np.int32), "snp_ref": a(t.snp_ref, S, np.uint8), "snp_alt": a(t.snp_alt, S, np.uint8),
            "snp_n_calls": a(t.snp_n_calls, S, np.int32), "snp_cell_off": a(t.snp_cell_off, S + 1, np.int64), "cells": cells,
            "t_kernel_ms": float(t.t_kernel_ms), "n_entries": int(t.n_entries), "n_wide_columns": int(t.n_wide_columns)}


def haplotype_alleles(contigs: Sequence[Dict], sr: Dict) -> Dict:
    """hs_haplotype_alleles: which allele every group of every window carries at every SNP of the window (separate_reads.cpp:1056-1113 on
    the final labels). contigs: one dict per contig as separate_reads_graph_taps takes them; sr: win_off, win_start, win_end, label_off and dense
    labels in the layout of a stage-4 result -- that call's own, or any labels (ids need not be 0..G-1)."""
    require_gpu()
    lib = load()
    arr, keep = _sr_contig_array(contigs)
    keep2 = []
    r = _sr_struct(sr, len(contigs), keep2)
    tb = C.POINTER(AlleleTable)()
    _check(lib.hs_haplotype_alleles(arr, C.c_int32(len(contigs)), C.byref(r), C.byref(tb)))
    out = _allele_table_to_dict(tb)
    lib.hs_allele_table_destroy(tb)
    del keep, keep2
    return out


def _group_call_inputs(contigs: Sequence[Dict], sr: Dict, dev: str):
    """the leading arguments hs_group_alleles and hs_group_recruit share -- the contigs' arrays one after the other on `dev`, the windows and labels
    of `sr`, with their counts --, the tensors behind them, and (S, W, n_labels)"""
    import torch
    depth = [np.diff(_np(c["col_off"], np.int64)) for c in contigs]
    col_off = np.concatenate([[0]] + [d for d in depth]).cumsum().astype(np.int64)
    def cat(key, dt):      # column entries from where the contig's col_off begins
        parts = [_np(c[key], dt)[int(c["col_off"][0]):int(c["col_off"][-1])] if key.startswith("col_") else _np(c[key], dt) for c in contigs]
        return np.concatenate([np.zeros(0, dt)] + parts).astype(dt)

    snp_contig = np.concatenate([np.zeros(0, np.int32)] + [np.full(len(c["snp_pos"]), k, np.int32) for k, c in enumerate(contigs)]).astype(np.int32)
    S, W, n_labels = len(snp_contig), len(sr["win_start"]), int(sr["label_off"][-1])
    up = lambda a, dt: torch.from_numpy(_np(a, dt) if len(a) else np.zeros(1, dt)).to(dev)
    d = [up(col_off, np.int64), up(cat("col_idx", np.int32), np.int32), up(cat("col_code", np.uint8), np.uint8), up(cat("snp_ref", np.uint8), np.uint8),
         up(cat("snp_alt", np.uint8), np.uint8), up(cat("snp_pos", np.int32), np.int32), up(snp_contig, np.int32)]
    w = [up(sr["win_off"], np.int64), up(sr["win_start"], np.int32), up(sr["win_end"], np.int32)]
    lab = [up(sr["label_off"], np.int64), up(sr["labels"], np.int32)]
    args = [_p(x) for x in d] + [C.c_int32(S)] + [_p(x) for x in w] + [C.c_int32(len(contigs)), C.c_int32(W)] + [_p(x) for x in lab] + [C.c_int64(n_labels)]
    return args, d + w + lab, (S, W, n_labels)


def group_alleles(contigs: Sequence[Dict], sr: Dict) -> Dict:
    """hs_group_alleles, the kernel-level call, in its two steps on torch tensors (inputs as haplotype_alleles takes them): the plan -- snp_win,
    grp_n, grp_off, grp_pack, win_snp_first, win_snp_last, cell_off over EVERY window and SNP of the call -- then cells and n_calls."""
    import torch
    require_gpu()
    lib = load()
    dev = "cuda:0"
    args, keep, (S, W, n_labels) = _group_call_inputs(contigs, sr, dev)
    L = AlleleLayout()
    _check(lib.hs_group_alleles_layout(C.c_int32(S), C.c_int32(W), C.c_int64(n_labels), C.byref(L)))
    work = torch.zeros(int(L.total_bytes), dtype=torch.uint8, device=dev)

    def call(cells, cap):
        _check(lib.hs_group_alleles(*args, _p(work), _p(cells), C.c_int64(cap), C.c_void_p(0)))
        torch.cuda.synchronize()

    call(None, 0)
    host = work[:int(L.grp_ids)].cpu().numpy()
    part = lambda off, n, dt: host[int(off):int(off) + n * np.dtype(dt).itemsize].view(dt).copy()
    out = {"snp_win": part(L.snp_win, S, np.int32), "grp_n": part(L.grp_n, W, np.int32), "win_snp_first": part(L.win_snp_first, W, np.int32),
           "win_snp_last": part(L.win_snp_last, W, np.int32), "cell_off": part(L.cell_off, S + 1, np.int64), "grp_off": part(L.grp_off, W + 1, np.int64)}
    n_groups, n_cells = int(out["grp_off"][-1]), int(out["cell_off"][-1])
    out["grp_pack"] = work[int(L.grp_pack):int(L.grp_pack) + 4 * n_groups].cpu().numpy().view(np.int32).copy()
    cells = torch.zeros(max(n_cells, 1) * ALLELE_CELL.itemsize, dtype=torch.uint8, device=dev)
    call(cells, n_cells)
    out["cells"] = cells[:n_cells * ALLELE_CELL.itemsize].cpu().numpy().view(ALLELE_CELL).copy()
    out["n_calls"] = work[int(L.n_calls):int(L.n_calls) + 4 * S].cpu().numpy().view(np.int32).copy()
    return out


# ------------------------------------------------------------------------------------------------
# a window's unlabelled reads recruited to its groups (hs_recruit_table)
# ------------------------------------------------------------------------------------------------
RECRUIT_PARAM_KEYS = ("which", "min_informative", "min_margin", "mismatch_num", "mismatch_den")


def recruit_params(**over) -> Dict:
    """hs_recruit_params_default() as a dict (placeholders of the interface, not validated figures), with `over` on top"""
    d = load().hs_recruit_params_default()
    out = {k: int(getattr(d, k)) for k in RECRUIT_PARAM_KEYS}
    out.update({k: int(v) for k, v in over.items()})
    return out


def _recruit_params(params) -> RecruitParams:
    d = recruit_params(**(params or {}))
    return RecruitParams(*[d[k] for k in RECRUIT_PARAM_KEYS])


def _recruit_table_to_dict(tp) -> Dict:
    """a copy of an hs_recruit_table as numpy arrays; "rows" has the dtype RECRUIT_ROW"""
    t = tp.contents
    W, R = int(t.n_windows), int(t.n_rows)
    a = _table_array
    rows = np.zeros(R, RECRUIT_ROW)
    if R:
        C.memmove(rows.ctypes.data, t.rows, R * RECRUIT_ROW.itemsize)
    return {"win_contig": a(t.win_contig, W, np.int32), "win_start": a(t.win_start, W, np.int32), "win_end": a(t.win_end, W, np.int32),
            "win_index": a(t.win_index, W, np.int64), "win_row_off": a(t.win_row_off, W + 1, np.int64), "rows": rows,
            "n_assigned": int(t.n_assigned), "params": {k: int(getattr(t.params, k)) for k in RECRUIT_PARAM_KEYS},
            "n_call_windows": int(t.n_call_windows), "n_counter_words": int(t.n_counter_words), "n_entries": int(t.n_entries),
            "t_kernel_ms": float(t.t_kernel_ms)}


def _recruit_table_from_dict(table: Dict, keep: list) -> RecruitTable:
    """an hs_recruit_table over the arrays of a dict of this module (for the device-free calls); `keep` holds the buffers"""
    t = RecruitTable()
    W, R = len(table["win_start"]), len(table["rows"])
    t.n_windows, t.n_rows, t.n_assigned = W, R, int(table.get("n_assigned", int((np.asarray(table["rows"])["assigned"] != 0).sum())))
    pad = lambda x, dt: _np(x if len(x) else np.zeros(1, dt), dt)
    wc, ws, we = pad(table["win_contig"], np.int32), pad(table["win_start"], np.int32), pad(table["win_end"], np.int32)
    wi, wo = pad(table["win_index"], np.int64), _np(table["win_row_off"], np.int64)
    rows = np.ascontiguousarray(np.asarray(table["rows"]).astype(RECRUIT_ROW)) if R else np.zeros(1, RECRUIT_ROW)
    keep += [wc, ws, we, wi, wo, rows]
    t.win_contig, t.win_start, t.win_end = _hp(wc, C.c_int32), _hp(ws, C.c_int32), _hp(we, C.c_int32)
    t.win_index, t.win_row_off, t.rows = _hp(wi, C.c_int64), _hp(wo, C.c_int64), rows.ctypes.data
    t.params = _recruit_params(table.get("params"))
    t.n_call_windows = int(table["n_call_windows"])
    return t


def _sr_struct(sr: Dict, Cn: int, keep: list) -> SrResult:
    wo, ws, we = _np(sr["win_off"], np.int64), _np(sr["win_start"], np.int32), _np(sr["win_end"], np.int32)
    lo, lab = _np(sr["label_off"], np.int64), _np(sr["labels"], np.int32)
    if len(ws) == 0:
        ws, we = np.zeros(1, np.int32), np.zeros(1, np.int32)
    if len(lab) == 0:
        lab = np.zeros(1, np.int32)
    keep += [wo, ws, we, lo, lab]
    r = SrResult()
    r.n_contigs = Cn
    r.win_off = _hp(wo, C.c_int64); r.win_start = _hp(ws, C.c_int32); r.win_end = _hp(we, C.c_int32)
    r.label_off = _hp(lo, C.c_int64); r.labels = _hp(lab, C.c_int32)
    return r


def recruit_reads(contigs: Sequence[Dict], sr: Dict, params: Optional[Dict] = None, with_alleles: bool = False):
    """hs_recruit_reads: which group of its window every read without a label there fits best, from the allele calls of the window's groups
    (inputs as haplotype_alleles takes them; params: recruit_params(), None = the defaults). Returns the table as a dict -- "rows" in the dtype
    RECRUIT_ROW, window-major, reads ascending -- or (table, allele table) with with_alleles=True."""
    require_gpu()
    lib = load()
    arr, keep = _sr_contig_array(contigs)
    keep2 = []
    r = _sr_struct(sr, len(contigs), keep2)
    prm = _recruit_params(params)
    rt, at = C.POINTER(RecruitTable)(), C.POINTER(AlleleTable)()
    _check(lib.hs_recruit_reads(arr, C.c_int32(len(contigs)), C.byref(r), C.byref(prm), C.byref(at) if with_alleles else None, C.byref(rt)))
    out = _recruit_table_to_dict(rt)
    lib.hs_recruit_table_destroy(rt)
    del keep, keep2
    if not with_alleles:
        return out
    alleles = _allele_table_to_dict(at)
    lib.hs_allele_table_destroy(at)
    return out, alleles


def recruit_apply(table: Dict, sr: Dict) -> np.ndarray:
    """hs_recruit_apply (no device): the dense labels of `sr` with every assigned row whose label is < 0 set to its best group"""
    lib = load()
    keep = []
    t = _recruit_table_from_dict(table, keep)
    lo, lab = _np(sr["label_off"], np.int64), _np(sr["labels"], np.int32)
    out = np.zeros(max(len(lab), 1), np.int32)
    src = lab if len(lab) else np.zeros(1, np.int32)
    _check(lib.hs_recruit_apply(C.byref(t), lo.ctypes.data, src.ctypes.data, out.ctypes.data, C.c_int64(len(lab))))
    return out[:len(lab)]


def recruit_text(table: Dict, names: Optional[Sequence[str]] = None) -> str:
    """hs_recruit_text: the text HS_separate_reads writes to <outfile>.recruit.tsv under HS_RECRUIT=1, from a table of this module"""
    lib = load()
    keep = []
    t = _recruit_table_from_dict(table, keep)
    arr = None
    if names is not None:
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    out = C.c_char_p()
    _check(lib.hs_recruit_text(C.byref(t), arr, C.c_int32(len(names) if names is not None else 0), C.byref(out)))
    text = out.value.decode()
    lib.hs_free_host(C.cast(out, C.c_void_p))
    return text


def group_recruit(contigs: Sequence[Dict], sr: Dict, params: Optional[Dict] = None, fill: int = 0, extra_rows: int = 0) -> Dict:
    """hs_group_recruit, the kernel-level call, in its two steps on torch tensors (inputs as recruit_reads takes them). The work buffer and
    the row buffer (extra_rows more rows than the plan counts) are filled with the byte `fill` first; returns the rows, win_row_off over all
    windows, status, the cells, and "rows_tail" -- the bytes of the row buffer behind the counted rows."""
    import torch
    require_gpu()
    lib = load()
    dev = "cuda:0"
    args, keep, (S, W, n_labels) = _group_call_inputs(contigs, sr, dev)
    L = RecruitLayout()
    _check(lib.hs_group_recruit_layout(C.c_int32(S), C.c_int32(W), C.c_int64(n_labels), C.byref(L)))
    work = torch.full((int(L.total_bytes),), fill, dtype=torch.uint8, device=dev)
    prm = _recruit_params(params)

    def call(cells, cap, ctr, ctr_cap, rows, rows_cap):
        _check(lib.hs_group_recruit(*args, C.byref(prm), _p(work), _p(cells), C.c_int64(cap), _p(ctr), C.c_int64(ctr_cap), _p(rows), C.c_int64(rows_cap), C.c_void_p(0)))
        torch.cuda.synchronize()

    call(None, 0, None, 0, None, 0)
    word = lambda off: int(work[int(off):int(off) + 8].cpu().numpy().view(np.int64)[0])
    n_cells = word(L.alleles.cell_off + 8 * S)
    n_rows, n_ctr = word(L.row_idx + 8 * n_labels), word(L.ctr_off + 8 * n_labels)
    cells = torch.zeros(max(n_cells, 1) * ALLELE_CELL.itemsize, dtype=torch.uint8, device=dev)
    ctr = torch.full((max(n_ctr, 1) * 4,), fill, dtype=torch.uint8, device=dev)
    rows = torch.full(((n_rows + extra_rows) * RECRUIT_ROW.itemsize + 8,), fill, dtype=torch.uint8, device=dev)
    call(cells, n_cells, ctr, n_ctr, rows, n_rows + extra_rows)
    host_rows = rows.cpu().numpy()
    part = lambda off, n, dt: work[int(off):int(off) + n * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
    return {"rows": host_rows[:n_rows * RECRUIT_ROW.itemsize].view(RECRUIT_ROW).copy(), "rows_tail": host_rows[n_rows * RECRUIT_ROW.itemsize:].copy(),
            "win_row_off": part(L.win_row_off, W + 1, np.int64), "status": int(part(L.status, 1, np.int32)[0]), "n_counter_words": n_ctr,
            "flag": part(L.flag, n_labels, np.int32), "cells": cells[:n_cells * ALLELE_CELL.itemsize].cpu().numpy().view(ALLELE_CELL).copy(),
            "win_snp_first": part(L.alleles.win_snp_first, W, np.int32), "win_snp_last": part(L.alleles.win_snp_last, W, np.int32),
            "work_gaps_untouched": _recruit_gaps_untouched(work, L, S, W, n_labels, fill)}


def _recruit_gaps_untouched(work, L, S, W, n_labels, fill) -> bool:
    """the alignment gaps behind the public parts of the recruit share of the work buffer still hold the fill byte (nothing wrote past a part)"""
    # (flag and the counter sizes behind it are cleared in one stretch, the gap between them included: not in this list)
    parts = [(int(L.row_idx), (n_labels + 1) * 8), (int(L.ctr_off), (n_labels + 1) * 8), (int(L.win_row_off), (W + 1) * 8), (int(L.status), 4)]
    host = work.cpu().numpy()
    for off, n in parts:
        end = off + max(n, 4)
        gap_end = (end + 255) & ~255
        if not np.all(host[end:min(gap_end, len(host))] == fill):
            return False
    return True


def allele_context(code: int) -> str:
    """the three bases a pileup code stands for (call_variants.cpp:25-31), "." for 0 / no code"""
    if code < 33 or code >= 33 + 125:
        return "."
    v = code - 33
    return "ACGT-"[(v % 25) // 5] + "ACGT-"[v % 5] + "ACGT-"[v // 25]


def alleles_text(table: Dict, names: Optional[Sequence[str]] = None) -> str:
    """the text HS_separate_reads writes to <outfile>.alleles.tsv under HS_ALLELES=1, from a table of this module"""
    out = []
    base = lambda code: "ACGT-"[(code - 33) % 5] if 33 <= code < 158 else "."
    for w in range(len(table["win_start"])):
        c = int(table["win_contig"][w])
        g0, g1 = int(table["win_group_off"][w]), int(table["win_group_off"][w + 1])
        ids = [int(x) for x in table["group_ids"][g0:g1]]
        name = names[c] if names is not None and 0 <= c < len(names) else str(c)
        out.append("WINDOW\t%s\t%d\t%d\t%s\n" % (name, table["win_start"][w], table["win_end"][w], "".join("%d," % g for g in ids)))
        for s in range(int(table["win_snp_off"][w]), int(table["win_snp_off"][w + 1])):
            line = "SNP\t%d\t%s\t%s\t%d" % (table["snp_pos"][s], base(int(table["snp_ref"][s])), base(int(table["snp_alt"][s])), table["snp_n_calls"][s])
            c0 = int(table["snp_cell_off"][s])
            for k, g in enumerate(ids):
                x = table["cells"][c0 + k]
                line += "\t%d:%d:%d:%d:%s" % (g, x["n"], x["n_ref"], x["n_alt"], allele_context(int(x["call"])))
            out.append(line + "\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------------
# kernel-level wrappers on torch CUDA tensors (used by the parity tests and bench.py's roofline leg)
# ------------------------------------------------------------------------------------------------
def device_tensors(flat: FlatBatch, device="cuda:0"):
    import torch
    t = {}
    for k in ("contig_seq", "contig_off", "read_seq", "read_off", "rec_read", "rec_contig", "rec_pos", "rec_strand",
              "rec_cig_off", "pile_off", "contig_rec_off", "rec_qend"):
        t[k] = torch.from_numpy(getattr(flat, k)).to(device)
    t["cigar"] = torch.from_numpy(flat.cigar.view(np.int32)).to(device)
    return t


def pileup_plan(flat: FlatBatch, ev_per_task: int = 4096):
    """hs_pileup_plan: (rec_chunk_off int64[n_rec+1], task_rec int32[], task_ev0 int32[])."""
    lib = load()
    chunk_off = np.zeros(flat.n_rec + 1, np.int64)
    n = C.c_int32(0)
    tr = C.POINTER(C.c_int32)(); te = C.POINTER(C.c_int32)()
    _check(lib.hs_pileup_plan(_hp(flat.rec_cig_off, C.c_int64), _hp(flat.cigar, C.c_uint32), C.c_int32(flat.n_rec), C.c_int32(ev_per_task),
                              _hp(chunk_off, C.c_int64), C.byref(n), C.byref(tr), C.byref(te)))
    nt = n.value
    task_rec = np.ctypeslib.as_array(tr, (max(nt, 1),))[:nt].copy()
    task_ev0 = np.ctypeslib.as_array(te, (max(nt, 1),))[:nt].copy()
    lib.hs_free_host(tr); lib.hs_free_host(te)
    return chunk_off, task_rec, task_ev0


def pileup(t, flat: FlatBatch, ev_per_task: int = 4096):
    """K0+K1 on device tensors; returns (pile u8[aligned_bp], rec_stats i32[n_rec,4])."""
    import torch
    require_gpu()
    dev = t["contig_seq"].device
    chunk_off, task_rec, task_ev0 = pileup_plan(flat, ev_per_task)
    d_co = torch.from_numpy(chunk_off).to(dev)
    d_tr = torch.from_numpy(task_rec if len(task_rec) else np.zeros(1, np.int32)).to(dev)
    d_te = torch.from_numpy(task_ev0 if len(task_ev0) else np.zeros(1, np.int32)).to(dev)
    scratch = torch.zeros(max(4 * int(chunk_off[-1]), 4), dtype=torch.int32, device=dev)
    pile = torch.zeros(max(flat.aligned_bp, 1), dtype=torch.uint8, device=dev)
    stats = torch.zeros((max(flat.n_rec, 1), 4), dtype=torch.int32, device=dev)
    _check(load().hs_pileup(_p(t["contig_seq"]), _p(t["contig_off"]), _p(t["read_seq"]), _p(t["read_off"]), _p(t["rec_read"]),
                            _p(t["rec_contig"]), _p(t["rec_pos"]), _p(t["rec_strand"]), _p(t["rec_cig_off"]), _p(t["cigar"]),
                            _p(t["pile_off"]), C.c_int32(flat.n_rec), _p(d_co), _p(scratch), _p(d_tr), _p(d_te),
                            C.c_int32(len(task_rec)), C.c_int32(ev_per_task), _p(pile), _p(stats), C.c_void_p(0)))
    torch.cuda.synchronize()
    return pile[:flat.aligned_bp], stats[:flat.n_rec]


def tile_plan(flat: FlatBatch, device="cuda:0"):
    """hs_tile_plan on the host arrays of a FlatBatch, uploaded: dict of device tensors (off int64, ent int64 [n,2] view of the 16-B entries, rec int32)"""
    import torch
    p_off = C.POINTER(C.c_int64)(); p_ent = C.c_void_p(); p_rec = C.POINTER(C.c_int32)(); n_tiles = C.c_int64(0)
    _check(load().hs_tile_plan(_hp(flat.contig_off, C.c_int64), C.c_int32(flat.n_contigs), _hp(flat.contig_rec_off, C.c_int32),
                               _hp(flat.rec_pos, C.c_int32), _hp(flat.rec_qend, C.c_int32), _hp(flat.pile_off, C.c_int64),
                               C.byref(p_off), C.byref(p_ent), C.byref(p_rec), C.byref(n_tiles)))
    nt = int(n_tiles.value)
    off = np.ctypeslib.as_array(p_off, shape=(nt + 1,)).copy()
    ne = int(off[-1])
    ent = np.ctypeslib.as_array(C.cast(p_ent, C.POINTER(C.c_int64)), shape=(max(ne, 1) * 2,)).copy()
    rec = np.ctypeslib.as_array(p_rec, shape=(max(ne, 1),)).copy()
    load().hs_free_host(p_off); load().hs_free_host(p_ent); load().hs_free_host(p_rec)
    return {"off": torch.from_numpy(off).to(device), "ent": torch.from_numpy(ent).to(device), "rec": torch.from_numpy(rec).to(device),
            "h_off": off, "h_ent": ent.view(np.int32).reshape(-1, 4), "h_rec": rec}


def column_stats(t, flat: FlatBatch, pile, min_second: int = 0, max_depth: int = 0, plan=None):
    """K2 in its full-statistics form on the tile plan (hs_column_stats_tiled); returns a numpy structured view: key u8[4], cnt u16[5],
    depth u16 per position (and, when min_second > 0, the compact selection -- second count > min_second, or == min_second with no
    third allele -- as sorted global positions + depths)."""
    import torch
    require_gpu()
    total = int(flat.contig_off[-1])
    dev = pile.device
    if plan is None:
        plan = tile_plan(flat, dev)
    out = torch.zeros((max(total, 1), 16), dtype=torch.uint8, device=dev)
    if min_second > 0:
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        gpos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
        dep = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
        args = (C.c_int32(min_second), _p(cnt), _p(gpos), _p(dep), C.c_int32(total))
    else:
        args = (C.c_int32(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_int32(0))
    _check(load().hs_column_stats_tiled(_p(pile), _p(plan["off"]), _p(plan["ent"]), C.c_int64(total), _p(out), *args, C.c_int32(max_depth), C.c_void_p(0)))
    torch.cuda.synchronize()
    dt = np.dtype([("key", np.uint8, 4), ("cnt", np.uint16, 5), ("depth", np.uint16)])
    st = out[:total].cpu().numpy().view(dt).reshape(-1)
    if min_second > 0:
        n = int(cnt.item())
        g = gpos[:n].cpu().numpy(); d = dep[:n].cpu().numpy()
        o = np.argsort(g, kind="stable")
        return st, g[o], d[o]
    return st


class _CandBits(C.Structure):
    _fields_ = [("wlo", C.c_int32), ("n_words", C.c_uint16), ("n_slots", C.c_uint16), ("idx_min", C.c_int32), ("idx_max", C.c_int32), ("reach", C.c_int32),
                ("n_entries", C.c_int32), ("word_off", C.c_int64)]


class _CvTaps(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("n_cols", C.c_int64), ("n_entries", C.c_int64), ("col_gpos", C.POINTER(C.c_int64)), ("col_rec", C.c_void_p),
                ("col_off", C.POINTER(C.c_int64)), ("col_idx", C.POINTER(C.c_int32)), ("col_code", C.POINTER(C.c_uint8)), ("n_cand", C.c_int64),
                ("cand_rec", C.c_void_p), ("cand_col", C.POINTER(C.c_int32)), ("cand_bits", C.POINTER(_CandBits)), ("cand_words", C.POINTER(C.c_uint64)),
                ("n_cand_words", C.c_int64), ("contig_n_cand", C.POINTER(C.c_int32)), ("contig_mean_distance", C.POINTER(C.c_float))]


COLREC_DTYPE = np.dtype([("pos", np.int32), ("contig", np.int32), ("c0", np.uint16), ("c1", np.uint16), ("k0", np.uint8), ("k1", np.uint8), ("flags", np.uint8), ("c2", np.uint8)])
CANDBITS_DTYPE = np.dtype([("wlo", np.int32), ("n_words", np.uint16), ("n_slots", np.uint16), ("idx_min", np.int32), ("idx_max", np.int32), ("reach", np.int32),
                           ("n_entries", np.int32), ("word_off", np.int64)])


def cv_column_pass_taps(batch: "CvBatch", c0: int, c1: int, automatic_snp_threshold: float = 0.33) -> Dict:
    """The column pass of stage 3 as the pipeline queues it (hs_cv_column_pass_taps), with what its kernels left on the device: the extracted
    columns (positions, records, CSR), the packed candidates, their bit sets, the contigs' candidate counts and mean distances."""
    lib = load()
    lib.hs_cv_column_pass_taps.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.POINTER(_CvTaps))]
    lib.hs_cv_taps_destroy.argtypes = [C.POINTER(_CvTaps)]
    lib.hs_cv_taps_destroy.restype = None
    tp = C.POINTER(_CvTaps)()
    _check(lib.hs_cv_column_pass_taps(batch.handle, C.c_int32(c0), C.c_int32(c1), C.c_float(automatic_snp_threshold), C.byref(tp)))
    t = tp.contents
    n, e, nc, Cn = int(t.n_cols), int(t.n_entries), int(t.n_cand), int(t.n_contigs)

    def arr(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype)
        return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
    out = {
        "col_gpos": arr(t.col_gpos, n, np.int64), "col_rec": arr(t.col_rec, n, COLREC_DTYPE), "col_off": arr(t.col_off, n + 1, np.int64),
        "col_idx": arr(t.col_idx, e, np.int32), "col_code": arr(t.col_code, e, np.uint8),
        "cand_rec": arr(t.cand_rec, nc, COLREC_DTYPE), "cand_col": arr(t.cand_col, nc, np.int32), "cand_bits": arr(t.cand_bits, nc, CANDBITS_DTYPE),
        "cand_words": arr(t.cand_words, int(t.n_cand_words), np.uint64),
        "contig_n_cand": arr(t.contig_n_cand, Cn, np.int32), "contig_mean_distance": arr(t.contig_mean_distance, Cn, np.float32),
    }
    lib.hs_cv_taps_destroy(tp)
    return out


class _CvPileupTaps(C.Structure):
    _fields_ = [("n_rec", C.c_int32), ("pile_lead", C.c_int32), ("pile_alloc_bytes", C.c_int64), ("n_chunks", C.c_int64), ("pile", C.POINTER(C.c_uint8)),
                ("pile_addr", C.POINTER(C.c_int64)), ("rec_stats", C.POINTER(C.c_int32)), ("rec_chunk_off", C.POINTER(C.c_int64)), ("chunk_table", C.POINTER(C.c_int32))]


def cv_pileup_tap(batch: "CvBatch", c0: int, c1: int, fill: int = 0xFF) -> Dict:
    """K0 + K1 of the contigs [c0, c1) as a contig group of the pipeline launches them on the resident batch (hs_cv_pileup_tap): the whole pile
    allocation is set to the byte `fill` first, rec_stats and the chunk table to 0xFF bytes. Returns what the device holds afterwards: "pile" (the whole
    allocation; "lead" bytes lie in front of the address 0 that "pile_addr" [n_rec + 1] counts from), "rec_stats" [n_rec, 4], "rec_chunk_off" [n_rec + 1],
    "chunk_table" [n_chunks, 4]. The batch's pileup is overwritten: take a fresh batch for anything else."""
    lib = load()
    lib.hs_cv_pileup_tap.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.POINTER(_CvPileupTaps))]
    lib.hs_cv_pileup_tap_destroy.argtypes = [C.POINTER(_CvPileupTaps)]
    lib.hs_cv_pileup_tap_destroy.restype = None
    tp = C.POINTER(_CvPileupTaps)()
    _check(lib.hs_cv_pileup_tap(batch.handle, C.c_int32(c0), C.c_int32(c1), C.c_int32(fill), C.byref(tp)))
    t = tp.contents
    n, nch = int(t.n_rec), int(t.n_chunks)

    def arr(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype)
        return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
    out = {"pile": arr(t.pile, int(t.pile_alloc_bytes), np.uint8), "lead": int(t.pile_lead), "pile_addr": arr(t.pile_addr, n + 1, np.int64),
           "rec_stats": arr(t.rec_stats, 4 * n, np.int32).reshape(n, 4), "rec_chunk_off": arr(t.rec_chunk_off, n + 1, np.int64),
           "chunk_table": arr(t.chunk_table, 4 * nch, np.int32).reshape(nch, 4)}
    lib.hs_cv_pileup_tap_destroy(tp)
    return out


def exclusive_scan(values):
    """n ints -> n + 1 offsets on the device (the scan behind the graph CSR and the selection list)"""
    import torch
    require_gpu()
    v = _np(values, np.int32)
    d_in = torch.from_numpy(v if v.size else np.zeros(1, np.int32)).to("cuda:0")
    d_out = torch.full((len(v) + 1,), -1, dtype=torch.int64, device="cuda:0")
    _check(load().hs_exclusive_scan_i32(_p(d_in), C.c_int32(len(v)), _p(d_out), C.c_void_p(0)))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def column_partition_test(col_off, col_idx, col_code, col_contig, col_k0, col_k1, col_c1, col_is_cand, part_off, part_state_off, part_state, n_reads):
    """K4: loops C/D of keep_only_robust_variants (call_variants.cpp:721-764); returns keep uint8 [n_cols]."""
    import torch
    require_gpu()
    dev = "cuda:0"
    n = len(col_contig)
    def up(a, dt):
        a = _np(a, dt)
        return torch.from_numpy(a if a.size else np.zeros(1, dt)).to(dev)
    d = [up(col_off, np.int64), up(col_idx, np.int32), up(col_code, np.uint8), up(col_contig, np.int32), up(col_k0, np.uint8), up(col_k1, np.uint8),
         up(col_c1, np.int32), up(col_is_cand, np.uint8)]
    q = [up(part_off, np.int32), up(part_state_off, np.int64), up(part_state, np.int8)]
    keep = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    nr = _np(n_reads, np.int32)
    _check(load().hs_column_partition_test(*[_p(x) for x in d], C.c_int32(n), *[_p(x) for x in q], _hp(nr, C.c_int32), C.c_int32(len(nr)), _p(keep), C.c_void_p(0)))
    torch.cuda.synchronize()
    return keep[:n].cpu().numpy()


def column_partition_last_counts():
    """what the kernels of this thread's last column_partition_test passed on: columns to k_column_partition_grouped, whole columns to
    k_column_partition_test, (column, partition) pairs to k_column_partition_pairs"""
    out = (C.c_int32 * 3)()
    load().hs_column_partition_last_counts(out)
    return {"to_grouped": int(out[0]), "whole_columns_to_exact": int(out[1]), "pairs_to_exact": int(out[2])}


class LoopAResult(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("on_device", C.POINTER(C.c_int32)), ("failed", C.POINTER(C.c_int32)), ("part_base", C.POINTER(C.c_int64)),
                ("rec", C.POINTER(C.c_int32)), ("state", C.POINTER(C.c_int8)), ("more", C.POINTER(C.c_int32)), ("less", C.POINTER(C.c_int32))]


LOOP_A_REC = ("left", "right", "n_occ", "n_corr", "lo", "hi", "reach", "w0", "w1")


def loop_a_test(contigs, form, cand_bound, pool_div=6, light=False):
    """Loop A of stage 3 on prescribed candidate columns (hs_loop_a_test). contigs: dicts of read_start, read_end [N], pos, k0 [S], off [S + 1], idx, code
    (CSR; read indices ascending inside a column). form: "host" (cv_build_cand_bits -> cv_phase_a_host) or "device" (the k_loop_a chain of stage 3 ->
    cv_phase_a_import; needs a GPU). Returns {"on_device": [C], "failed": [C], "contigs": [per contig {"rec": [P, 9] (LOOP_A_REC), "state", "more", "less":
    [P, N]}]}; a contig of the device form that was not planned for the device or was handed back has P = 0."""
    assert form in ("host", "device")
    if form == "device":
        require_gpu()
    lib = load()
    n = [len(c["read_start"]) for c in contigs]
    read_off = _np(np.concatenate([[0], np.cumsum(n)]), np.int32)
    col_base = _np(np.concatenate([[0], np.cumsum([len(c["pos"]) for c in contigs])]), np.int64)
    cat = lambda key, dt: _np(np.concatenate([np.asarray(c[key]) for c in contigs] + [np.zeros(1)]), dt)
    rs, re_, pos, k0, idx, code = cat("read_start", np.int32), cat("read_end", np.int32), cat("pos", np.int32), cat("k0", np.uint8), cat("idx", np.int32), cat("code", np.uint8)
    off = [np.zeros(1, np.int64)]
    e = 0
    for c in contigs:
        o = np.asarray(c["off"], np.int64)
        assert o[0] == 0 and o[-1] == len(c["idx"]) == len(c["code"])
        off.append(o[1:] + e); e += int(o[-1])
    off = _np(np.concatenate(off), np.int64)
    lib.hs_loop_a_test.argtypes = [C.c_int32] + [C.c_void_p] * 9 + [C.c_int32] * 4 + [C.POINTER(C.POINTER(LoopAResult)), C.c_void_p]
    lib.hs_loop_a_result_destroy.argtypes = [C.POINTER(LoopAResult)]; lib.hs_loop_a_result_destroy.restype = None
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    res = C.POINTER(LoopAResult)()
    _check(lib.hs_loop_a_test(C.c_int32(len(contigs)), hp(read_off), hp(rs), hp(re_), hp(col_base), hp(pos), hp(k0), hp(off), hp(idx), hp(code),
                              C.c_int32(0 if form == "host" else 1), C.c_int32(int(cand_bound)), C.c_int32(int(pool_div)), C.c_int32(1 if light else 0), C.byref(res), C.c_void_p(0)))
    r = res.contents
    Cn = len(contigs)
    a = lambda p, m, dt: np.ctypeslib.as_array(p, (max(m, 1),))[:m].astype(dt).copy()
    base = a(r.part_base, Cn + 1, np.int64)
    out = {"on_device": a(r.on_device, Cn, np.int32), "failed": a(r.failed, Cn, np.int32), "contigs": []}
    P = int(base[-1])
    rec = a(r.rec, 9 * P, np.int32).reshape(P, 9)
    D = int(sum(int(base[c + 1] - base[c]) * n[c] for c in range(Cn)))
    state, more, less = a(r.state, D, np.int8), a(r.more, D, np.int32), a(r.less, D, np.int32)
    d = 0
    for c in range(Cn):
        p = int(base[c + 1] - base[c])
        sl = slice(d, d + p * n[c])
        out["contigs"].append({"rec": rec[base[c]:base[c + 1]], "state": state[sl].reshape(p, n[c]), "more": more[sl].reshape(p, n[c]), "less": less[sl].reshape(p, n[c])})
        d += p * n[c]
    lib.hs_loop_a_result_destroy(res)
    return out


def partition_pair_distance(state, more, less, part_off, part_n, pair_a, pair_b, threshold_p=2):
    """V5 for a list of partition pairs (dense arrays, state 2 = absent): [n_pairs, 8] = n00, n01, n10, n11, phased, augmented, valid, comparable"""
    import torch
    require_gpu()
    dev = "cuda:0"
    n = len(pair_a)
    up = lambda a, dt: torch.from_numpy(_np(a, dt) if len(a) else np.zeros(1, dt)).to(dev)
    sigma3 = np.array([np.float32(0.5 * k + 3 * np.sqrt(k * 0.5 * (1 - 0.5))) for k in range(4096)], np.float32)
    d = [up(state, np.int8), up(more, np.int32), up(less, np.int32), up(part_off, np.int64), up(part_n, np.int32), up(pair_a, np.int32), up(pair_b, np.int32)]
    sg = up(sigma3, np.float32)
    out = torch.zeros((max(n, 1), 8), dtype=torch.int32, device=dev)
    _check(load().hs_partition_pair_distance(*[_p(x) for x in d], C.c_int32(n), C.c_int32(threshold_p), _p(sg), _p(out), C.c_void_p(0)))
    torch.cuda.synchronize()
    return out[:n].cpu().numpy()


def snp_planes(n_reads, snp_ref, snp_alt, col_off, col_idx, col_code):
    """K5a for one contig: returns (alt, ref) uint64 [N, words] bit-planes"""
    import torch
    require_gpu()
    dev = "cuda:0"
    S = len(snp_ref)
    W = (S + 63) // 64
    up = lambda a, dt: torch.from_numpy(_np(a, dt) if len(a) else np.zeros(1, dt)).to(dev)
    d = [up(col_off, np.int64), up(col_idx, np.int32), up(col_code, np.uint8), up(snp_ref, np.uint8), up(snp_alt, np.uint8),
         up(np.zeros(S, np.int32), np.int32), up(np.zeros(1, np.int64), np.int64), up(np.zeros(1, np.int64), np.int64), up(np.array([W], np.int32), np.int32)]
    # (not zeroed on purpose: the kernel writes every word of the rows)
    alt = torch.full((n_reads, max(W, 1)), -1, dtype=torch.int64, device=dev); ref = torch.full_like(alt, -1)
    hw = np.array([W], np.int32)
    _check(load().hs_snp_planes(*[_p(x) for x in d], _p(up(np.array([n_reads], np.int32), np.int32)), _hp(hw, C.c_int32), C.c_int32(1), C.c_int32(S), _p(alt), _p(ref), C.c_void_p(0)))
    torch.cuda.synchronize()
    return alt.cpu().numpy().view(np.uint64)[:, :W], ref.cpu().numpy().view(np.uint64)[:, :W]


def simdiff(alt_planes: np.ndarray, ref_planes: np.ndarray):
    """K5 for one contig: planes are uint64 [N, words]; returns (sim, diff) int32 [N, N]."""
    import torch
    require_gpu()
    N, W = alt_planes.shape
    dev = "cuda:0"
    a = torch.from_numpy(alt_planes.view(np.int64)).to(dev); r = torch.from_numpy(ref_planes.view(np.int64)).to(dev)
    po = torch.zeros(1, dtype=torch.int64, device=dev); oo = torch.zeros(1, dtype=torch.int64, device=dev)
    n = torch.tensor([N], dtype=torch.int32, device=dev); w = torch.tensor([W], dtype=torch.int32, device=dev)
    sim = torch.zeros((N, N), dtype=torch.int32, device=dev); diff = torch.zeros((N, N), dtype=torch.int32, device=dev)
    _check(load().hs_simdiff(_p(a), _p(r), _p(po), _p(n), _p(w), _p(oo), C.c_int32(1), _p(sim), _p(diff), C.c_void_p(0)))
    torch.cuda.synchronize()
    return sim.cpu().numpy(), diff.cpu().numpy()


def read_graphs(sim_list, diff_list, windows, error_rate):
    """K6: sim_list/diff_list = per-contig int32 [N, N] matrices (uploaded here); windows = [(contig, ascending masked read ids)].
    Returns (per window: dict read id -> sorted neighbour list, rows resolved on the host)."""
    import torch
    require_gpu()
    dev = "cuda:0"
    n = np.array([m.shape[0] for m in sim_list], np.int32)
    off = np.zeros(len(n), np.int64)
    if len(n) > 1:
        off[1:] = np.cumsum(n[:-1].astype(np.int64) ** 2)
    d_sim = torch.from_numpy(np.concatenate([np.ascontiguousarray(m, np.int32).ravel() for m in sim_list])).to(dev)
    d_diff = torch.from_numpy(np.concatenate([np.ascontiguousarray(m, np.int32).ravel() for m in diff_list])).to(dev)
    wc = np.array([w[0] for w in windows], np.int32)
    moff = np.zeros(len(windows) + 1, np.int64); moff[1:] = np.cumsum([len(w[1]) for w in windows])
    ids = _np(np.concatenate([np.asarray(w[1], np.int32) for w in windows]) if moff[-1] else np.zeros(1, np.int32), np.int32)
    p_off = C.POINTER(C.c_int64)(); p_nbr = C.POINTER(C.c_int32)(); n_host = C.c_int64(0)
    _check(load().hs_read_graphs(_p(d_sim), _p(d_diff), off.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), C.c_int32(len(n)),
                                 wc.ctypes.data_as(C.c_void_p), moff.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), C.c_int32(len(windows)),
                                 C.c_float(error_rate), C.byref(p_off), C.byref(p_nbr), C.byref(n_host), C.c_void_p(0)))
    rows = int(moff[-1])
    noff = np.ctypeslib.as_array(p_off, shape=(rows + 1,)).copy()
    nbr = np.ctypeslib.as_array(p_nbr, shape=(max(int(noff[-1]), 1),)).copy()
    load().hs_free_host(p_off); load().hs_free_host(p_nbr)
    out = []
    for w in range(len(windows)):
        out.append({int(ids[r]): nbr[noff[r]:noff[r + 1]].tolist() for r in range(int(moff[w]), int(moff[w + 1]))})
    return out, int(n_host.value)


def edit_distance(queries: Sequence[np.ndarray], targets: Sequence[np.ndarray], mode: str = "NW"):
    """A1 Myers bit-vector kernel; codes 0..3; mode NW | SHW | HW. Returns (distance, end) int32 arrays."""
    import torch
    require_gpu()
    dev = "cuda:0"
    m = {"NW": 0, "SHW": 1, "HW": 2}[mode]
    qo = np.zeros(len(queries) + 1, np.int64); qo[1:] = np.cumsum([len(q) for q in queries])
    to = np.zeros(len(targets) + 1, np.int64); to[1:] = np.cumsum([len(x) for x in targets])
    q = _np(np.concatenate(queries) if qo[-1] else np.zeros(1), np.uint8)
    tt = _np(np.concatenate(targets) if to[-1] else np.zeros(1), np.uint8)
    T = lambda a: torch.from_numpy(a).to(dev)
    d_q, d_qo, d_t, d_to = T(q), T(qo), T(tt), T(to)
    n = len(queries)
    dist = torch.zeros(n, dtype=torch.int32, device=dev); end = torch.zeros(n, dtype=torch.int32, device=dev)
    _check(load().hs_edit_distance(_p(d_q), _p(d_qo), _p(d_t), _p(d_to), C.c_int32(n), C.c_int32(m), _p(dist), _p(end), C.c_void_p(0)))
    torch.cuda.synchronize()
    return dist.cpu().numpy(), end.cpu().numpy()


# ---- next stage: the .gro consumer (host code; needs no device) -----------------------------------------
def gaf_from_files(gfa: str, reads: str, sam: str, gro: str, out_gaf: str, amplicon: bool = False, n_threads: int = 1) -> None:
    """parse_split_file + merge_intervals + output_GAF of the reference's stage 5 (create_new_contigs.cpp:1582-1590)."""
    _check(load().hs_gaf_from_files(gfa.encode(), reads.encode(), sam.encode(), gro.encode(), C.c_int32(1 if amplicon else 0),
                                    out_gaf.encode(), C.c_int32(n_threads)))


def gaf_from_labels(gfa: str, reads: str, sam: str, sr: Dict, out_gaf: str, contig_has_snps=None, amplicon: bool = False,
                    n_threads: int = 1) -> None:
    """Same, from a stage-4 result in memory (`sr` as returned by separate_reads / run_pipeline: win_off, win_start, win_end,
    label_off, labels) instead of the .gro text; contig_has_snps[c] = False for contigs the .gro writer would skip (default:
    the contigs without windows)."""
    win_off = _np(sr["win_off"], np.int64); win_start = _np(sr["win_start"], np.int32); win_end = _np(sr["win_end"], np.int32)
    label_off = _np(sr["label_off"], np.int64); labels = _np(sr["labels"], np.int32)
    has = None if contig_has_snps is None else _np(np.asarray(contig_has_snps).astype(np.uint8), np.uint8)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)
    _check(load().hs_gaf_from_labels(gfa.encode(), reads.encode(), sam.encode(), C.c_int32(1 if amplicon else 0), C.c_int32(len(win_off) - 1),
                                     ptr(win_off), ptr(win_start), ptr(win_end), ptr(label_off), ptr(labels), None if has is None else ptr(has),
                                     out_gaf.encode(), C.c_int32(n_threads)))


# ---- next stage: the polisher's inputs (device work on the resident batch) ---------------------------------
POLISH_START_BEYOND_SEQ = 2      # piece_flags bit: posOnReadStart lies beyond the read (the reference's substr throws there); the piece is empty
_POLISH_I32_BUNDLE = ("bundle_contig", "bundle_interval", "bundle_start", "bundle_end", "bundle_group", "bundle_left_to_polish",
                      "bundle_right_to_polish", "bundle_overhang_left", "bundle_overhang_right")
_POLISH_I32_PIECE = ("piece_rec", "piece_read_start", "piece_read_end", "piece_sam_pos", "piece_flags")


class PolishResult(C.Structure):
    _fields_ = ([("n_bundles", C.c_int64), ("n_pieces", C.c_int64), ("n_dropped", C.c_int64)] +
                [(k, C.POINTER(C.c_int32)) for k in _POLISH_I32_BUNDLE] +
                [("backbone_off", C.POINTER(C.c_int64)), ("backbone", C.POINTER(C.c_uint8)), ("piece_off", C.POINTER(C.c_int64))] +
                [(k, C.POINTER(C.c_int32)) for k in _POLISH_I32_PIECE] +
                [("base_off", C.POINTER(C.c_int64)), ("bases", C.POINTER(C.c_uint8)), ("cig_off", C.POINTER(C.c_int64)),
                 ("cigar", C.POINTER(C.c_uint32)), ("dropped", C.POINTER(C.c_int32)),
                 ("t_scan_ms", C.c_double), ("t_cut_ms", C.c_double), ("t_gather_ms", C.c_double), ("t_cigar_ms", C.c_double),
                 ("n_tasks", C.c_int64), ("n_rounds", C.c_int64), ("cut_ops_read", C.c_int64)])


def polish_inputs(batch_or_pipeline, sr: Dict, polish_everything: bool = False, c0: int = 0, c1: Optional[int] = None,
                  contig_has_snps=None) -> Dict:
    """The polisher's inputs of the reference's stage 5 (create_new_contigs.cpp:358-521) for the contigs [c0, c1) of a resident
    batch (a CvBatch or a PipelineGroups) from a stage-4 result `sr` (win_off, win_start, win_end, label_off, labels, as
    gaf_from_labels takes them). Returns numpy arrays: per bundle (one group of one merged interval) bundle_* and backbone_off /
    backbone (toPolish, text), piece_off; per piece piece_* , base_off / bases (text), cig_off / cigar (len << 4 | op); dropped
    [n][3] = (contig, interval, record) of the reads the walk drops; "stats" = kernel times and counts of the call."""
    batch = getattr(batch_or_pipeline, "batch", batch_or_pipeline)
    lib = load()
    win_off = _np(sr["win_off"], np.int64); win_start = _np(sr["win_start"], np.int32); win_end = _np(sr["win_end"], np.int32)
    label_off = _np(sr["label_off"], np.int64); labels = _np(sr["labels"], np.int32)
    has = None if contig_has_snps is None else _np(np.asarray(contig_has_snps).astype(np.uint8), np.uint8)
    if len(win_off) - 1 != batch.flat.n_contigs:
        raise HsError("polish_inputs: the result does not cover the contigs of the batch")
    if c1 is None:
        c1 = batch.flat.n_contigs

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)
    res = C.POINTER(PolishResult)()
    lib.hs_polish_inputs.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.POINTER(C.POINTER(PolishResult))]
    lib.hs_polish_result_destroy.argtypes = [C.c_void_p]
    lib.hs_polish_result_destroy.restype = None
    _check(lib.hs_polish_inputs(batch.handle, C.c_int32(c0), C.c_int32(c1), ptr(win_off), ptr(win_start), ptr(win_end), ptr(label_off), ptr(labels),
                                None if has is None else ptr(has), C.c_int32(1 if polish_everything else 0), C.byref(res)))
    try:
        out = _polish_result_dict(res.contents, True)
    finally:
        lib.hs_polish_result_destroy(res)
    return out


def _c_array(p, n, dtype):
    return np.ctypeslib.as_array(p, (n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)


def _polish_result_dict(r, with_text: bool) -> Dict:
    """a hs_polish_result as numpy arrays; with_text: backbone, bases and cigar too (hs_polish_haplotypes leaves them on the device)"""
    B, P, D = int(r.n_bundles), int(r.n_pieces), int(r.n_dropped)
    arr = _c_array
    out = {"n_bundles": B, "n_pieces": P}
    for k in _POLISH_I32_BUNDLE:
        out[k] = arr(getattr(r, k), B, np.int32)
    for k in _POLISH_I32_PIECE:
        out[k] = arr(getattr(r, k), P, np.int32)
    out["backbone_off"] = arr(r.backbone_off, B + 1, np.int64)
    out["piece_off"] = arr(r.piece_off, B + 1, np.int64)
    out["base_off"] = arr(r.base_off, P + 1, np.int64)
    out["cig_off"] = arr(r.cig_off, P + 1, np.int64)
    if with_text:
        out["backbone"] = arr(r.backbone, int(out["backbone_off"][-1]), np.uint8)
        out["bases"] = arr(r.bases, int(out["base_off"][-1]), np.uint8)
        out["cigar"] = arr(r.cigar, int(out["cig_off"][-1]), np.uint32)
    out["dropped"] = arr(r.dropped, 3 * D, np.int32).reshape(D, 3)
    out["stats"] = {"scan_ms": r.t_scan_ms, "cut_ms": r.t_cut_ms, "gather_ms": r.t_gather_ms, "cigar_ms": r.t_cigar_ms,
                    "n_tasks": int(r.n_tasks), "n_rounds": int(r.n_rounds), "cut_ops_read": int(r.cut_ops_read)}
    return out


def polish_inputs_from_files(gfa: str, reads: str, sam: str, gro: str, out_path: str, polish_everything: bool = False, n_threads: int = 1) -> None:
    """The same from the four files HS_create_new_contigs reads, written as the text of bin/hs_polish_inputs."""
    _check(load().hs_polish_inputs_from_files(gfa.encode(), reads.encode(), sam.encode(), gro.encode(), C.c_int32(1 if polish_everything else 0),
                                              out_path.encode(), C.c_int32(n_threads)))


def polish_cigar_string(words) -> str:
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=X"[int(w) & 15]) for w in words)


def polish_bundle_text(res: Dict, i: int, contig_name: Optional[str] = None) -> str:
    """Bundle i as bin/hs_polish_inputs writes it"""
    p0, p1 = int(res["piece_off"][i]), int(res["piece_off"][i + 1])
    head = [contig_name if contig_name is not None else str(int(res["bundle_contig"][i]))] + [
        str(int(res[k][i])) for k in ("bundle_start", "bundle_end", "bundle_group", "bundle_left_to_polish", "bundle_right_to_polish",
                                      "bundle_overhang_left", "bundle_overhang_right")] + [str(p1 - p0)]
    out = ["BUNDLE\t" + "\t".join(head), ">seq", res["backbone"][int(res["backbone_off"][i]):int(res["backbone_off"][i + 1])].tobytes().decode()]
    for p in range(p0, p1):
        b0, b1 = int(res["base_off"][p]), int(res["base_off"][p + 1])
        if b1 > b0:      # tools.cpp:357: empty pieces are left out
            out.append(">read%d %d %s" % (p - p0, int(res["piece_sam_pos"][p]), polish_cigar_string(res["cigar"][int(res["cig_off"][p]):int(res["cig_off"][p + 1])])))
            out.append(res["bases"][b0:b1].tobytes().decode())
    return "\n".join(out) + "\n"


def polish_bundle_files(res: Dict, i: int, dir: str, id: str = "0") -> Dict:
    """Bundle i as the files the reference's consensus_reads hands to its polisher (tools.cpp:351-361): unpolished_<id>.fasta and
    reads_<id>.fasta, plus mapped_<id>.sam built from the clipped CIGARs -- the SAM of the commented-out block at tools.cpp:383-392,
    which makes the minimap2 run of :374-380 unnecessary: `racon reads_<id>.fasta mapped_<id>.sam unpolished_<id>.fasta`."""
    p0, p1 = int(res["piece_off"][i]), int(res["piece_off"][i + 1])
    backbone = res["backbone"][int(res["backbone_off"][i]):int(res["backbone_off"][i + 1])].tobytes().decode()
    paths = {k: os.path.join(dir, "%s_%s.%s" % (k, id, ext)) for k, ext in (("unpolished", "fasta"), ("reads", "fasta"), ("mapped", "sam"))}
    with open(paths["unpolished"], "w") as f:
        f.write(">seq\n" + backbone + "\n")
    with open(paths["reads"], "w") as fr, open(paths["mapped"], "w") as fs:
        fs.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:seq\tLN:%d\n" % len(backbone))
        for p in range(p0, p1):
            b0, b1 = int(res["base_off"][p]), int(res["base_off"][p + 1])
            if b1 == b0:
                continue
            seq = res["bases"][b0:b1].tobytes().decode()
            fr.write(">read%d\n%s\n" % (p - p0, seq))
            fs.write("read%d\t0\tseq\t%d\t60\t%s\t*\t0\t0\t%s\t*\tAS:i:0\tXS:i:0\n" % (
                p - p0, int(res["piece_sam_pos"][p]), polish_cigar_string(res["cigar"][int(res["cig_off"][p]):int(res["cig_off"][p + 1])]), seq))
    return paths


# ---- the consensus of every bundle: a vote per backbone column and per insertion slot (the rule is ours: csrc/hs_consensus_host.h) ----
_CONSENSUS_I32 = ("trim_start", "trim_end", "n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped")


class ConsensusParams(C.Structure):
    _fields_ = [("min_cov", C.c_int32), ("max_ins", C.c_int32)]


class ConsensusResult(C.Structure):
    _fields_ = ([("n_bundles", C.c_int64), ("cons_off", C.POINTER(C.c_int64)), ("cons", C.POINTER(C.c_uint8))] + [(k, C.POINTER(C.c_int32)) for k in _CONSENSUS_I32] +
                [("t_rows_ms", C.c_double), ("t_columns_ms", C.c_double), ("t_ins_ms", C.c_double), ("t_emit_ms", C.c_double),
                 ("n_rounds", C.c_int64), ("n_ins_records", C.c_int64), ("n_ins_slots", C.c_int64)])


def consensus_params(**kw) -> ConsensusParams:
    """hs_consensus_default_params (min_cov 3, max_ins 32: PLACEHOLDERS, not tuned) with the given fields replaced"""
    lib = load()
    lib.hs_consensus_default_params.restype = ConsensusParams
    lib.hs_consensus_default_params.argtypes = []
    p = lib.hs_consensus_default_params()
    for k, v in kw.items():
        if k not in ("min_cov", "max_ins"):
            raise HsError("consensus_params: no field " + k)
        setattr(p, k, int(v))
    return p


_ARRAYS_ARGTYPES = [C.c_int64] + [C.c_void_p] * 11 + [C.POINTER(ConsensusParams)]      # n_bundles, the eleven arrays of a polishing job, the parameters


def polish_consensus(res: Dict, params: Optional[ConsensusParams] = None, form: str = "device") -> Dict:
    """The consensus of every bundle of `res`: the dict polish_inputs returns, or one of hand-built arrays with the keys backbone_off, backbone,
    bundle_overhang_left, bundle_overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar. form "device": the kernels
    (hs_polish_consensus_arrays); "host": the host half of the same rule (hs_polish_consensus_host, no device); "planned": the device again, but
    every piece planned by k_cons_plan as hs_polish_haplotypes plans it (hs_polish_consensus_planned_tap) -- the result then holds "plan",
    [n_pieces][4] = skipped, long_cigar, n_cols, n_ins as the device found them. Returns numpy arrays cons_off, cons
    (text), trim_start, trim_end, n_sub, n_del, n_ins_bases, n_low, n_skipped per bundle, and "stats"."""
    if form not in ("device", "host", "planned"):
        raise HsError("polish_consensus: form is 'device', 'host' or 'planned'")
    lib = load()
    B, P, args, keep = _consensus_arrays_args("polish_consensus", res, params)
    lib.hs_consensus_result_destroy.argtypes = [C.c_void_p]
    lib.hs_consensus_result_destroy.restype = None
    out_p = C.POINTER(ConsensusResult)()
    plan = None
    if form == "planned":
        plan = np.full((P, 4), -1, np.int32)
        fn = lib.hs_polish_consensus_planned_tap
        fn.argtypes = _ARRAYS_ARGTYPES + [C.c_void_p, C.POINTER(C.POINTER(ConsensusResult))]
        _check(fn(*(args + [plan.ctypes.data_as(C.c_void_p), C.byref(out_p)])))
    else:
        fn = lib.hs_polish_consensus_arrays if form == "device" else lib.hs_polish_consensus_host
        fn.argtypes = _ARRAYS_ARGTYPES + [C.POINTER(C.POINTER(ConsensusResult))]
        _check(fn(*(args + [C.byref(out_p)])))
    try:
        out = _consensus_result_dict(out_p.contents, B)
    finally:
        lib.hs_consensus_result_destroy(out_p)
    if plan is not None:
        out["plan"] = plan
    return out


def _consensus_result_dict(r, B: int) -> Dict:
    arr = _c_array
    out = {"n_bundles": int(r.n_bundles), "cons_off": arr(r.cons_off, B + 1, np.int64)}
    out["cons"] = arr(r.cons, int(out["cons_off"][-1]), np.uint8)
    for k in _CONSENSUS_I32:
        out[k] = arr(getattr(r, k), B, np.int32)
    out["stats"] = {"rows_ms": r.t_rows_ms, "columns_ms": r.t_columns_ms, "ins_ms": r.t_ins_ms, "emit_ms": r.t_emit_ms, "n_rounds": int(r.n_rounds),
                    "n_ins_records": int(r.n_ins_records), "n_ins_slots": int(r.n_ins_slots)}
    return out


def consensus_text(cons: Dict, i: int, trimmed: bool = False) -> str:
    """The consensus of bundle i of a polish_consensus result; trimmed: without the overhangs, cons[trim_start, trim_end)"""
    o = int(cons["cons_off"][i])
    a, b = (int(cons["trim_start"][i]), int(cons["trim_end"][i])) if trimmed else (0, int(cons["cons_off"][i + 1]) - o)
    return cons["cons"][o + a:o + max(a, b)].tobytes().decode()


# ---- from labels to haplotype sequences: the rounds of polish_inputs with the consensus as their sink, the pieces never leaving the device ----
class HaplotypesResult(C.Structure):
    _fields_ = [("inputs", C.POINTER(PolishResult)), ("consensus", C.POINTER(ConsensusResult)), ("n_rounds", C.c_int64), ("n_sub_rounds", C.c_int64),
                ("bytes_down", C.c_int64), ("bytes_up", C.c_int64), ("t_plan_ms", C.c_double)]


def _haplotypes_result_dict(h, refined=None) -> Dict:
    """A hs_haplotypes_result as one dict: the metadata of its inputs and the keys of its consensus, "stats" those of both with n_rounds (resident
    rounds), n_sub_rounds, bytes_down, bytes_up and plan_ms. Without inputs (polish_refine: the arrays were the caller's) the consensus keys alone,
    n_rounds the consensus's own. refined (a hs_refined_result): "passes" as well."""
    cons = _consensus_result_dict(h.consensus.contents, int(h.consensus.contents.n_bundles))
    if h.inputs:
        out = _polish_result_dict(h.inputs.contents, False)
        stats = dict(out["stats"], **cons.pop("stats"))
        out.update(cons)
        stats["n_rounds"] = int(h.n_rounds)
    else:
        out, stats = cons, cons["stats"]
    stats.update({"n_sub_rounds": int(h.n_sub_rounds), "bytes_down": int(h.bytes_down), "bytes_up": int(h.bytes_up), "plan_ms": h.t_plan_ms})
    out["stats"] = stats
    if refined is not None:
        out["passes"] = _refined_passes_dict(refined)
    return out


def polish_haplotypes(batch_or_pipeline, sr: Dict, polish_everything: bool = False, c0: int = 0, c1: Optional[int] = None, contig_has_snps=None,
                      params: Optional[ConsensusParams] = None, passes: int = 1) -> Dict:
    """polish_consensus(polish_inputs(...)) in one call (hs_polish_haplotypes): the arguments of polish_inputs and the consensus parameters. One
    dict: the metadata keys of polish_inputs (everything but backbone, bases and cigar, which stay on the device), the keys of polish_consensus,
    and "stats" = those of both, n_rounds (resident rounds), n_sub_rounds (consensus rounds), bytes_down, bytes_up and plan_ms.
    passes > 1 (hs_polish_haplotypes_refined): every piece is realigned to the consensus of the pass before and the vote is taken again, on the device;
    the consensus keys are the last pass's and "passes" holds the per-pass figures (see polish_refine). passes == 1 calls the one-pass entry."""
    batch = getattr(batch_or_pipeline, "batch", batch_or_pipeline)
    lib = load()
    win_off = _np(sr["win_off"], np.int64); win_start = _np(sr["win_start"], np.int32); win_end = _np(sr["win_end"], np.int32)
    label_off = _np(sr["label_off"], np.int64); labels = _np(sr["labels"], np.int32)
    has = None if contig_has_snps is None else _np(np.asarray(contig_has_snps).astype(np.uint8), np.uint8)
    if len(win_off) - 1 != batch.flat.n_contigs:
        raise HsError("polish_haplotypes: the result does not cover the contigs of the batch")
    if c1 is None:
        c1 = batch.flat.n_contigs

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)
    res = C.POINTER(HaplotypesResult)()
    refined = C.POINTER(RefinedResult)()
    labels_argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.POINTER(ConsensusParams)]
    lib.hs_polish_haplotypes.argtypes = labels_argtypes + [C.POINTER(C.POINTER(HaplotypesResult))]
    lib.hs_polish_haplotypes_refined.argtypes = labels_argtypes + [C.c_int32, C.POINTER(C.POINTER(RefinedResult))]
    lib.hs_haplotypes_result_destroy.argtypes = [C.c_void_p]
    lib.hs_haplotypes_result_destroy.restype = None
    lib.hs_refined_result_destroy.argtypes = [C.c_void_p]
    lib.hs_refined_result_destroy.restype = None
    args = [batch.handle, C.c_int32(c0), C.c_int32(c1), ptr(win_off), ptr(win_start), ptr(win_end), ptr(label_off), ptr(labels),
            None if has is None else ptr(has), C.c_int32(1 if polish_everything else 0), None if params is None else C.byref(params)]
    if passes == 1:
        _check(lib.hs_polish_haplotypes(*(args + [C.byref(res)])))
    else:
        _check(lib.hs_polish_haplotypes_refined(*(args + [C.c_int32(int(passes)), C.byref(refined)])))
        res = refined.contents.last
    try:
        return _haplotypes_result_dict(res.contents, refined.contents if refined else None)
    finally:
        if refined:
            lib.hs_refined_result_destroy(refined)
        else:
            lib.hs_haplotypes_result_destroy(res)


# ---- polishing passes: pieces realigned to the consensus of the pass before, then the vote again (the rule: csrc/hs_refine_host.h) ----
REFINE_MAX_PASSES = 8
_REFINE_I64 = ("n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped", "n_pairs", "n_unaligned", "sum_dist", "move_bytes", "cigar_words")
_REFINE_MS = ("t_windows_ms", "t_align_ms", "t_cigar_ms", "t_plan_ms", "t_consensus_ms")


class RefinedResult(C.Structure):
    _fields_ = ([("last", C.POINTER(HaplotypesResult)), ("n_passes", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_int64 * REFINE_MAX_PASSES) for k in _REFINE_I64] +
                [(k, C.c_double * REFINE_MAX_PASSES) for k in _REFINE_MS] + [("n_waits", C.c_int64 * REFINE_MAX_PASSES)])


class RefinePlan(C.Structure):
    _fields_ = [("consensus", C.POINTER(ConsensusResult)), ("n_bundles", C.c_int64), ("n_pieces", C.c_int64), ("col_off", C.POINTER(C.c_int64)),
                ("col_begin", C.POINTER(C.c_int32)), ("col_ins", C.POINTER(C.c_int32)), ("win_start", C.POINTER(C.c_int64)), ("win_end", C.POINTER(C.c_int64))]


def _refined_passes_dict(r) -> Dict:
    n = int(r.n_passes)
    out = {"n_passes": n}
    for k in _REFINE_I64 + ("n_waits",):
        out[k] = np.array(list(getattr(r, k))[:n], np.int64)
    for k in _REFINE_MS:
        out[k[2:]] = np.array(list(getattr(r, k))[:n], np.float64)
    return out


def _consensus_arrays_args(who: str, res: Dict, params: Optional[ConsensusParams] = None):
    """the arrays of a polishing job, converted and checked against each other, as the arguments _ARRAYS_ARGTYPES names: n_bundles, n_pieces, the
    argument list and the arrays it points into (to be kept alive over the call)"""
    a64 = [_np(res[k], np.int64) for k in ("backbone_off", "piece_off", "base_off", "cig_off")]
    a32 = [_np(res[k], np.int32) for k in ("bundle_overhang_left", "bundle_overhang_right", "piece_sam_pos", "piece_flags")]
    backbone, bases, cigar = _np(res["backbone"], np.uint8), _np(res["bases"], np.uint8), _np(res["cigar"], np.uint32)
    B = len(a64[0]) - 1
    if B < 0 or len(a64[1]) != B + 1 or len(a32[0]) != B or len(a32[1]) != B:
        raise HsError(who + ": the bundle arrays do not agree")
    P = int(a64[1][-1])
    if len(a64[2]) != P + 1 or len(a64[3]) != P + 1 or len(a32[2]) != P or len(a32[3]) != P:
        raise HsError(who + ": the piece arrays do not agree")
    if len(backbone) < int(a64[0][-1]) or len(bases) < int(a64[2][-1]) or len(cigar) < int(a64[3][-1]):
        raise HsError(who + ": the offsets run beyond the arrays")
    keep = a64 + a32 + [backbone, bases, cigar]

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)
    args = [C.c_int64(B), ptr(a64[0]), ptr(backbone), ptr(a32[0]), ptr(a32[1]), ptr(a64[1]), ptr(a32[2]), ptr(a32[3]), ptr(a64[2]), ptr(bases), ptr(a64[3]), ptr(cigar),
            None if params is None else C.byref(params)]
    return B, P, args, keep


def polish_refine(res: Dict, params: Optional[ConsensusParams] = None, passes: int = 2) -> Dict:
    """`passes` polishing passes over the bundles of `res` (the arrays polish_consensus takes) on the device (hs_polish_refine_arrays): the arrays go up
    whole, every pass from the second on realigns each piece to its window of the consensus just made (A1, NW with path) and votes again with that
    consensus as the backbone. Returns the keys of polish_consensus for the LAST pass and "passes": n_passes and, per pass, n_sub, n_del, n_ins_bases,
    n_low, n_skipped (sums over the bundles, each against that pass's backbone), n_pairs, n_unaligned, sum_dist, move_bytes, cigar_words (0 for pass 1),
    windows_ms, align_ms, cigar_ms, plan_ms, consensus_ms and n_waits."""
    lib = load()
    B, P, args, keep = _consensus_arrays_args("polish_refine", res, params)
    fn = lib.hs_polish_refine_arrays
    fn.argtypes = _ARRAYS_ARGTYPES + [C.c_int32, C.POINTER(C.POINTER(RefinedResult))]
    lib.hs_refined_result_destroy.argtypes = [C.c_void_p]
    lib.hs_refined_result_destroy.restype = None
    out_p = C.POINTER(RefinedResult)()
    _check(fn(*(args + [C.c_int32(int(passes)), C.byref(out_p)])))
    try:
        return _haplotypes_result_dict(out_p.contents.last.contents, out_p.contents)
    finally:
        lib.hs_refined_result_destroy(out_p)




def polish_refine_plan_host(res: Dict, params: Optional[ConsensusParams] = None) -> Dict:
    """One pass on the host and what the next pass needs of it (hs_polish_refine_plan_host, no device): the keys of polish_consensus(form="host"), then
    col_off [n_bundles + 1], col_begin and col_ins (L + 1 per bundle: where column t begins in the bundle's consensus, the inserted bases in front of
    it) and per piece win_start / win_end, its window in its bundle's consensus (-1 / -1: none)."""
    lib = load()
    B, P, args, keep = _consensus_arrays_args("polish_refine_plan_host", res, params)
    fn = lib.hs_polish_refine_plan_host
    fn.argtypes = _ARRAYS_ARGTYPES + [C.POINTER(C.POINTER(RefinePlan))]
    lib.hs_refine_plan_destroy.argtypes = [C.c_void_p]
    lib.hs_refine_plan_destroy.restype = None
    out_p = C.POINTER(RefinePlan)()
    _check(fn(*(args + [C.byref(out_p)])))
    try:
        r = out_p.contents
        out = _consensus_result_dict(r.consensus.contents, B)
        out["col_off"] = _c_array(r.col_off, B + 1, np.int64)
        n = int(out["col_off"][-1])
        out["col_begin"] = _c_array(r.col_begin, n, np.int32); out["col_ins"] = _c_array(r.col_ins, n, np.int32)
        out["win_start"] = _c_array(r.win_start, P, np.int64); out["win_end"] = _c_array(r.win_end, P, np.int64)
    finally:
        lib.hs_refine_plan_destroy(out_p)
    return out


def haplotype_text(res: Dict, i: int) -> str:
    """The sequence of bundle i of a polish_haplotypes result: its consensus without the overhangs"""
    return consensus_text(res, i, trimmed=True)


def haplotype_fasta_header(res: Dict, i: int, contig_name: Optional[str] = None) -> str:
    """The header bin/hs_polish_inputs writes for bundle i under HS_HAPLOTYPES=1 (without the '>')"""
    name = contig_name if contig_name is not None else str(int(res["bundle_contig"][i]))
    return "%s_%d_%d_%d" % (name, int(res["bundle_start"][i]), int(res["bundle_end"][i]), int(res["bundle_group"][i]))


def polish_haplotypes_from_files(gfa: str, reads: str, sam: str, gro: str, out_fasta: str, polish_everything: bool = False, params: Optional[ConsensusParams] = None,
                                 n_threads: int = 1, passes: int = 1) -> None:
    """The same from the four files HS_create_new_contigs reads, written as FASTA: a record ">contig_start_end_group" per bundle, its trimmed consensus
    on one line (hs_polish_haplotypes_from_files; what bin/hs_polish_inputs writes under HS_HAPLOTYPES=1)."""
    lib = load()
    if passes != 1:      # (hs_polish_haplotypes_refined_from_files; what HS_POLISH_PASSES asks of bin/hs_polish_inputs)
        lib.hs_polish_haplotypes_refined_from_files.argtypes = [C.c_char_p] * 4 + [C.c_int32, C.POINTER(ConsensusParams), C.c_int32, C.c_char_p, C.c_int32]
        _check(lib.hs_polish_haplotypes_refined_from_files(gfa.encode(), reads.encode(), sam.encode(), gro.encode(), C.c_int32(1 if polish_everything else 0),
                                                           None if params is None else C.byref(params), C.c_int32(int(passes)), out_fasta.encode(), C.c_int32(n_threads)))
        return
    lib.hs_polish_haplotypes_from_files.argtypes = [C.c_char_p] * 4 + [C.c_int32, C.POINTER(ConsensusParams), C.c_char_p, C.c_int32]
    _check(lib.hs_polish_haplotypes_from_files(gfa.encode(), reads.encode(), sam.encode(), gro.encode(), C.c_int32(1 if polish_everything else 0),
                                               None if params is None else C.byref(params), out_fasta.encode(), C.c_int32(n_threads)))


def edlib_hw_align(pairs, path=True):
    """A1 as stage 5 uses edlib (HW, k = -1, TASK_PATH): list of (query, target) strings over ACGT -> list of dicts
    {distance, start, end, ops (numpy uint8 of edlib move codes) or None}"""
    import torch
    require_gpu()
    dev = "cuda:0"
    code = np.full(256, 3, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    enc = lambda x: code[np.frombuffer(x.encode(), dtype=np.uint8)] if x else np.zeros(0, np.uint8)
    qs = [enc(q) for q, _ in pairs]; ts = [enc(t) for _, t in pairs]
    n = len(pairs)
    qo = np.zeros(n + 1, np.int64); to = np.zeros(n + 1, np.int64); oo = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in qs], out=qo[1:]); np.cumsum([len(x) for x in ts], out=to[1:]); np.cumsum([len(a) + len(b) for a, b in zip(qs, ts)], out=oo[1:])
    cat = lambda xs: np.concatenate(xs) if xs and sum(len(x) for x in xs) else np.zeros(1, np.uint8)
    dq = torch.from_numpy(cat(qs)).to(dev); dt = torch.from_numpy(cat(ts)).to(dev)
    dd = torch.zeros(max(n, 1), dtype=torch.int32, device=dev); ds = torch.zeros_like(dd); de = torch.zeros_like(dd); dl = torch.zeros_like(dd)
    dops = torch.zeros(max(int(oo[-1]), 1), dtype=torch.uint8, device=dev)
    _check(load().hs_edlib_hw_align(_p(dq), _hp(qo, C.c_int64), _p(dt), _hp(to, C.c_int64), C.c_int32(n), _p(dd), _p(ds), _p(de),
                                    _p(dops) if path else C.c_void_p(0), _hp(oo, C.c_int64), _p(dl), C.c_void_p(0)))
    torch.cuda.synchronize()
    dd, ds, de, dl, ops = dd.cpu().numpy(), ds.cpu().numpy(), de.cpu().numpy(), dl.cpu().numpy(), dops.cpu().numpy()
    out = []
    for i in range(n):
        out.append({"distance": int(dd[i]), "start": int(ds[i]), "end": int(de[i]),
                    "ops": ops[oo[i]:oo[i] + dl[i]].copy() if path and dl[i] >= 0 else None})
    return out


EDLIB_MODES = {"NW": 0, "SHW": 1, "HW": 2}
EDLIB_TASKS = {"distance": 0, "loc": 1, "path": 2}


def _edlib_codes(pairs):
    """(query, target) -> code arrays 0..3. Strings / bytes: one bijection per pair from its bytes to the codes, in order of first
    appearance (hs_stage5.cpp encode_pair): edlib compares bytes, so this keeps its results exactly. Arrays are codes already."""
    qs, ts = [], []
    for i, (q, t) in enumerate(pairs):
        if isinstance(q, (str, bytes)) and isinstance(t, (str, bytes)):
            qb = np.frombuffer(q.encode() if isinstance(q, str) else q, dtype=np.uint8)
            tb = np.frombuffer(t.encode() if isinstance(t, str) else t, dtype=np.uint8)
            seen = np.unique(np.concatenate((qb, tb)), return_index=True)
            if len(seen[0]) > 4:
                raise HsError(f"edlib_align: pair {i} has {len(seen[0])} distinct bytes; the kernel has four codes")
            code = np.zeros(256, np.uint8)
            code[seen[0][np.argsort(seen[1])]] = np.arange(len(seen[0]), dtype=np.uint8)
            qs.append(code[qb]); ts.append(code[tb])
        elif isinstance(q, (str, bytes)) or isinstance(t, (str, bytes)):
            raise HsError(f"edlib_align: pair {i} mixes a string with a code array")
        else:
            qa, ta = np.asarray(q), np.asarray(t)
            if (qa.size and (qa.min() < 0 or qa.max() > 3)) or (ta.size and (ta.min() < 0 or ta.max() > 3)):
                raise HsError(f"edlib_align: pair {i}: code arrays hold codes 0..3")
            qs.append(qa.astype(np.uint8).reshape(-1)); ts.append(ta.astype(np.uint8).reshape(-1))
    return qs, ts


def alignment_to_cigar(ops, fmt="extended"):
    """edlibAlignmentToCigar on host (hs_alignment_to_cigar): fmt "standard" (M I D) or "extended" (= X I D)."""
    lib = load()
    f = {"standard": 0, "extended": 1}[fmt]
    a = _np(ops if ops is not None else [], np.uint8)
    out = C.c_char_p()
    lib.hs_alignment_to_cigar.argtypes = [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_char_p)]
    _check(lib.hs_alignment_to_cigar(_hp(a, C.c_uint8), C.c_int32(len(a)), C.c_int32(f), C.byref(out)))
    s = C.cast(out, C.c_char_p).value.decode()
    lib.hs_free_host(C.cast(out, C.c_void_p))
    return s


def _edlib_bytes(pairs):
    """(query, target) -> uint8 arrays of the bytes as they are (str: its encoding; bytes; arrays of values 0..255)"""
    def one(x, i):
        if isinstance(x, str):
            x = x.encode()
        if isinstance(x, (bytes, bytearray)):
            return np.frombuffer(bytes(x), dtype=np.uint8)
        a = np.asarray(x)
        if a.size and (a.min() < 0 or a.max() > 255):
            raise HsError(f"edlib_align: pair {i}: byte arrays hold values 0..255")
        return a.astype(np.uint8).reshape(-1)
    return [one(q, i) for i, (q, _) in enumerate(pairs)], [one(t, i) for i, (_, t) in enumerate(pairs)]


def _equality_pairs(equalities):
    """[(a, b), ...] of one-character strings, bytes or ints -> uint8 array [n, 2] (hs_equality_pair, == EdlibEqualityPair)"""
    def byte(x):
        if isinstance(x, str):
            x = x.encode()
        if isinstance(x, (bytes, bytearray)):
            if len(x) != 1:
                raise HsError("edlib_align: an equality names single bytes")
            return x[0]
        if not 0 <= int(x) <= 255:
            raise HsError("edlib_align: an equality names bytes 0..255")
        return int(x)
    return np.array([[byte(a), byte(b)] for a, b in equalities], dtype=np.uint8).reshape(-1, 2)


def edlib_align(pairs, mode="NW", task="path", k=-1, cigar=None, alphabet=None, equalities=None):
    """edlibAlign(query, target, edlibNewAlignConfig(k, mode, task, equalities, len(equalities))) for every (query, target) pair, on
    the device. mode NW | SHW | HW; task "distance" | "loc" | "path"; k = -1: no bound.
    alphabet None (hs_edlib_align): strings / bytes with at most four distinct bytes per pair, or arrays of codes 0..3.
    alphabet "bytes" (hs_edlib_align_bytes): str, bytes and uint8 arrays as they are, any alphabet up to 256 distinct bytes.
    equalities: edlib's additionalEqualities, a list of 2-tuples of one-character strings, bytes or ints, e.g. [("N", "A"), ("N", "C"),
    ("N", "G"), ("N", "T")]; implies alphabet "bytes".
    -> one dict per pair: {distance (-1 beyond k), start, end (-1 when none), n_locations, ops (numpy uint8 of edlib move codes;
    None unless task "path"), cigar (None unless cigar = "standard" | "extended")}."""
    import torch
    require_gpu()
    dev = "cuda:0"
    m, tk = EDLIB_MODES[mode], EDLIB_TASKS[task]
    if cigar is not None and tk != 2:
        raise HsError("edlib_align: a CIGAR needs task 'path'")
    if alphabet not in (None, "bytes"):
        raise HsError("edlib_align: alphabet is None or 'bytes'")
    as_bytes = alphabet == "bytes" or equalities is not None
    qs, ts = _edlib_bytes(pairs) if as_bytes else _edlib_codes(pairs)
    n = len(pairs)
    qo = np.zeros(n + 1, np.int64); to = np.zeros(n + 1, np.int64); oo = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in qs], out=qo[1:]); np.cumsum([len(x) for x in ts], out=to[1:])
    np.cumsum([len(a) + len(b) for a, b in zip(qs, ts)], out=oo[1:])
    cat = lambda xs: np.concatenate(xs) if xs and sum(len(x) for x in xs) else np.zeros(1, np.uint8)
    dq = torch.from_numpy(cat(qs)).to(dev); dt = torch.from_numpy(cat(ts)).to(dev)
    dd = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    ds, de, dn, dl = (torch.zeros_like(dd) for _ in range(4))
    dops = torch.zeros(max(int(oo[-1]), 1), dtype=torch.uint8, device=dev) if tk == 2 else None
    outs = (_p(dd), _p(ds), _p(de), _p(dn), _p(dops), _hp(oo, C.c_int64) if tk == 2 else None, _p(dl) if tk == 2 else C.c_void_p(0), C.c_void_p(0))
    if as_bytes:
        eq = _equality_pairs(equalities if equalities is not None else [])
        _check(load().hs_edlib_align_bytes(_p(dq), _hp(qo, C.c_int64), _p(dt), _hp(to, C.c_int64), C.c_int32(n), C.c_int32(m), C.c_int32(tk),
                                           C.c_int32(int(k)), _hp(eq, C.c_uint8) if len(eq) else None, C.c_int32(len(eq)), *outs))
    else:
        _check(load().hs_edlib_align(_p(dq), _hp(qo, C.c_int64), _p(dt), _hp(to, C.c_int64), C.c_int32(n), C.c_int32(m), C.c_int32(tk),
                                     C.c_int32(int(k)), *outs))
    torch.cuda.synchronize()
    dd, ds, de, dn, dl = (x.cpu().numpy() for x in (dd, ds, de, dn, dl))
    ops = dops.cpu().numpy() if tk == 2 else None
    out = []
    for i in range(n):
        o = ops[oo[i]:oo[i] + dl[i]].copy() if tk == 2 and dl[i] >= 0 else None
        out.append({"distance": int(dd[i]), "start": int(ds[i]), "end": int(de[i]), "n_locations": int(dn[i]), "ops": o,
                    "cigar": alignment_to_cigar(o, cigar) if cigar is not None and o is not None else None})
    return out


def _string_batch(fn, lists, ints=()):
    lib = load()
    require_gpu()
    n = len(lists[0])
    arrs = [(C.c_char_p * max(n, 1))(*[x.encode() for x in l]) for l in lists]
    iarrs = [np.ascontiguousarray(v, np.int32) for v in ints]
    out = C.POINTER(C.c_char_p)()
    fn.argtypes = [C.POINTER(C.c_char_p)] * len(arrs) + [C.POINTER(C.c_int32)] * len(iarrs) + [C.c_int32, C.POINTER(C.POINTER(C.c_char_p))]
    _check(fn(*arrs, *[_hp(v, C.c_int32) for v in iarrs], C.c_int32(n), C.byref(out)))
    res = [out[i].decode() for i in range(n)]
    lib.hs_free_strings.argtypes = [C.POINTER(C.c_char_p), C.c_int32]
    lib.hs_free_strings.restype = None
    lib.hs_free_strings(out, C.c_int32(n))
    return res


def _stage5_fn(name, alphabet):
    if alphabet not in (None, "bytes"):
        raise HsError(name + ": alphabet is None or 'bytes'")
    return getattr(load(), name + ("_bytes" if alphabet == "bytes" else ""))


def reattach_ends(backbones, consensuses, alphabet=None):
    """tools.cpp:505-536, batched. alphabet None: at most four distinct bytes per aligned pair (hs_reattach_ends); "bytes": any
    bytes, compared as edlib compares them (hs_reattach_ends_bytes)"""
    return _string_batch(_stage5_fn("hs_reattach_ends", alphabet), [backbones, consensuses])


def trim_polished(to_polish, newcontigs, overhang_left, overhang_right, alphabet=None):
    """create_new_contigs.cpp:556-629, batched. alphabet as in reattach_ends (hs_trim_polished / hs_trim_polished_bytes)"""
    return _string_batch(_stage5_fn("hs_trim_polished", alphabet), [to_polish, newcontigs], [overhang_left, overhang_right])


def moves_to_cigar(moves_list, clips=None, spans=False, count_only=False, ops_len=None):
    """hs_moves_to_cigar: edlib move arrays (0 '=', 1 insertion, 2 deletion, 3 mismatch), one per pair, as hs_edlib_hw_align leaves them ->
    list of uint32 arrays of packed CIGAR words (len << 4 | op; M 0, I 1, D 2, S 4). An entry that is None stands for a pair without an
    alignment (ops_len -1): no words. clips: [(left, right), ...] soft clips around the runs, or None. spans=True: also an int32 array
    [n, 2] of reference and read spans. count_only=True: the word offsets [n + 1] instead of the words (no word is written).
    ops_len: the d_ops_len the call sees, where it is to differ from the arrays' lengths (a pair keeps its array's room)."""
    import torch
    require_gpu()
    dev = "cuda:0"
    n = len(moves_list)
    arrs = [np.zeros(0, np.uint8) if m is None else _np(m, np.uint8).reshape(-1) for m in moves_list]
    lens = np.array([-1 if m is None else len(a) for m, a in zip(moves_list, arrs)], np.int32)
    if ops_len is not None:
        lens = _np(ops_len, np.int32)
        assert len(lens) == n
    oo = np.zeros(n + 1, np.int64)
    np.cumsum([len(a) for a in arrs], out=oo[1:])
    flat = np.concatenate(arrs) if n and oo[-1] else np.zeros(1, np.uint8)
    d_ops = torch.from_numpy(flat).to(dev)
    d_len = torch.from_numpy(lens if n else np.zeros(1, np.int32)).to(dev)
    d_cl = d_cr = None
    if clips is not None:
        cl = _np([c[0] for c in clips], np.int32); cr = _np([c[1] for c in clips], np.int32)
        assert len(cl) == n
        d_cl = torch.from_numpy(cl if n else np.zeros(1, np.int32)).to(dev); d_cr = torch.from_numpy(cr if n else np.zeros(1, np.int32)).to(dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.zeros((max(n, 1), 2), dtype=torch.int32, device=dev) if spans else None
    total = C.c_int64(0)
    lib = load()
    call = lambda d_words, cap: lib.hs_moves_to_cigar(_p(d_ops), _hp(oo, C.c_int64), _p(d_len), _p(d_cl), _p(d_cr), C.c_int32(n), _p(d_off), _p(d_words), C.c_int64(cap),
                                                      _p(d_sp), C.byref(total), C.c_void_p(0))
    _check(call(None, 0))
    if not count_only:
        d_words = torch.zeros(max(int(total.value), 1), dtype=torch.int32, device=dev)
        _check(call(d_words, int(total.value)))
    torch.cuda.synchronize()
    off = d_off.cpu().numpy()
    if count_only:
        out = off
    else:
        w = d_words.cpu().numpy().view(np.uint32)
        out = [w[off[i]:off[i + 1]].copy() for i in range(n)]
    return (out, d_sp.cpu().numpy()[:n]) if spans else out


def _realign(who, flat_sequences, intervals, anchors, pad, want_batch):
    """the one body of realign_intervals (anchors None) and realign_intervals_anchored (anchors = (anc_off, anc_q, anc_t))"""
    import time
    require_gpu()
    lib = load()
    g = (lambda k: flat_sequences[k]) if isinstance(flat_sequences, dict) else (lambda k: getattr(flat_sequences, k))
    cseq, coff, rseq, roff = _np(g("contig_seq"), np.uint8), _np(g("contig_off"), np.int64), _np(g("read_seq"), np.uint8), _np(g("read_off"), np.int64)
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 7)
    if iv.size and (np.abs(iv).max() > 0x7fffffff):
        raise HsError(who + ": interval fields are 32-bit")
    col = [_np(iv[:, k], np.uint8 if k == 2 else np.int32) for k in range(7)]
    args = [_hp(cseq, C.c_uint8), _hp(coff, C.c_int64), C.c_int32(len(coff) - 1), _hp(rseq, C.c_uint8), _hp(roff, C.c_int64), C.c_int32(len(roff) - 1)]
    args += [_hp(c, C.c_uint8 if k == 2 else C.c_int32) for k, c in enumerate(col)] + [C.c_int32(len(iv)), C.c_int32(pad)]
    if anchors is not None:
        aoff, aq, at = _np(anchors[0], np.int64), _np(anchors[1], np.int32), _np(anchors[2], np.int32)
        if len(aoff) != len(iv) + 1 or len(aq) != len(at) or (len(aoff) and int(aoff[-1]) > len(aq)):
            raise HsError(who + ": anc_off has one entry per interval and one more, anc_q and anc_t anc_off[-1] entries")
        args += [_hp(aoff, C.c_int64), _hp(aq, C.c_int32), _hp(at, C.c_int32)]
    h = C.c_void_p(); r = C.POINTER(RealignRecords)()
    t0 = time.perf_counter()
    _check(getattr(lib, "hs_" + who)(*args, C.byref(r), C.byref(h) if want_batch else None))
    dt = time.perf_counter() - t0
    try:
        rec = _realign_records_to_dict(r)
    finally:
        lib.hs_realign_records_destroy(r)
    return rec, (CvBatch._adopt(h, dt, rec) if want_batch else None)


def realign_intervals(flat_sequences, intervals, pad: int = 100, want_batch: bool = True):
    """hs_realign_intervals: intervals held in memory -> alignment records with CIGARs (and the resident batch made from them).
    flat_sequences: anything with contig_seq / contig_off / read_seq / read_off as a FlatBatch has them (codes 0..3, one per byte).
    intervals: rows (read, contig, strand, qstart, qend, tstart, tend); strand 1 forward, 0 reverse; half-open, 0-based.
    Returns (records dict, CvBatch or None): records grouped by contig, input order inside a contig (rec_interval says which row)."""
    return _realign("realign_intervals", flat_sequences, intervals, None, pad, want_batch)


def realign_cut_tap(seq, off, src, rev=None, fill: int = 0xA5, out_cap: Optional[int] = None, m: Optional[int] = None) -> np.ndarray:
    """hs_realign_cut_tap: k_realign_cut through the job's own launch on the pieces (off [m + 1], src [m], rev [m] or None) of `seq`; returns all out_cap
    bytes (default: off[m] rounded up to 16, and 64 guard bytes behind), those behind the rounded length still `fill`. A refused table raises HsError."""
    require_gpu()
    seq, off, src = _np(seq, np.uint8), _np(off, np.int64), _np(src, np.int64)
    m = len(src) if m is None else int(m)
    if len(off) != m + 1 or len(src) < m or (rev is not None and len(rev) != m):
        raise HsError("realign_cut_tap: off has one entry per piece and one more, src and rev one per piece")
    rev = None if rev is None else _np(rev, np.uint8)
    if out_cap is None:
        out_cap = ((int(off[-1]) + 15) & ~15) + 64 if m >= 1 and 0 <= int(off[-1]) < (1 << 40) else 64
    out = np.empty(max(int(out_cap), 1), np.uint8)
    _check(load().hs_realign_cut_tap(_hp(seq, C.c_uint8), C.c_int64(len(seq)), _hp(off, C.c_int64), _hp(src, C.c_int64), _hp(rev, C.c_uint8) if rev is not None else None,
                                     C.c_int32(m), C.c_int32(fill), _hp(out, C.c_uint8), C.c_int64(out_cap)))
    return out[:int(out_cap)]


JOIN_TABLE = (("iv_piece", np.int32), ("iv_base", np.int32), ("join_off", np.int64), ("pc_kind", np.uint8), ("pc_idx", np.int32), ("pc_room", np.int32), ("pc_ops", np.int64))
JOIN_NUMBERS = ("dist", "start", "end", "len")


def anchor_join_tap(table: Dict, fill: int = 0xA5, joined_cap: Optional[int] = None) -> Dict:
    """hs_anchor_join_tap: k_anchor_join_plan and k_anchor_join through the job's own launches. table: the piece table of a round (iv_piece, iv_base,
    join_off, pc_kind, pc_idx, pc_room, pc_ops) and the aligner's side (ops; dist, start, end, len of equal length). Returns pc_at, out_len, out_dist,
    out_pos and `joined`: all joined_cap bytes (default: join_off[m] rounded up to 16, and 64 guard bytes behind). A refused table raises HsError."""
    require_gpu()
    t = {k: _np(table[k], dt) for k, dt in JOIN_TABLE}
    num = {k: _np(table[k], np.int32) for k in JOIN_NUMBERS}
    ops = _np(table["ops"], np.uint8)
    m, P, n_num = len(t["iv_base"]), len(t["pc_kind"]), len(num["dist"])
    if len(t["iv_piece"]) != m + 1 or len(t["join_off"]) != m + 1 or any(len(t[k]) != P for k in ("pc_idx", "pc_room", "pc_ops")) or any(len(v) != n_num for v in num.values()):
        raise HsError("anchor_join_tap: iv_piece and join_off have one entry per interval and one more, the pc_ arrays one per piece, the numbers one length")
    if m >= 1 and int(t["iv_piece"][-1]) > P:
        raise HsError("anchor_join_tap: iv_piece names %d pieces, the table has %d" % (int(t["iv_piece"][-1]), P))
    if joined_cap is None:
        joined_cap = ((int(t["join_off"][-1]) + 15) & ~15) + 64 if 0 <= int(t["join_off"][-1]) < (1 << 40) else 64
    one = lambda a: a if len(a) else np.zeros(1, a.dtype)      # (an empty array still has an address)
    outs = dict(pc_at=np.full(max(P, 1), -7, np.int32), out_len=np.full(max(m, 1), -7, np.int32), out_dist=np.full(max(m, 1), -7, np.int32), out_pos=np.full(max(m, 1), -7, np.int32),
                joined=np.empty(max(int(joined_cap), 1), np.uint8))
    args = [C.c_int32(m)] + [_hp(one(t[k]), C.c_int64 if dt is np.int64 else (C.c_uint8 if dt is np.uint8 else C.c_int32)) for k, dt in JOIN_TABLE]
    args += [_hp(one(ops), C.c_uint8), C.c_int64(len(ops))] + [_hp(one(num[k]), C.c_int32) for k in JOIN_NUMBERS] + [C.c_int32(n_num), C.c_int32(fill)]
    args += [_hp(outs[k], C.c_int32) for k in ("pc_at", "out_len", "out_dist", "out_pos")] + [_hp(outs["joined"], C.c_uint8), C.c_int64(joined_cap)]
    _check(load().hs_anchor_join_tap(*args))
    return dict(pc_at=outs["pc_at"][:P], out_len=outs["out_len"][:m], out_dist=outs["out_dist"][:m], out_pos=outs["out_pos"][:m], joined=outs["joined"][:int(joined_cap)])


# ---- the read mapper (hs_map_*): minimizer seeds against a resident index of the contigs, a vote over diagonal bins ----
def _params_with(default, who, kw):
    """a parameter struct of the library's defaults with the given fields replaced"""
    for k, v in kw.items():
        if k not in dict(type(default)._fields_):
            raise HsError(who + ": no field " + k)
        setattr(default, k, int(v))
    return default


def map_params(**kw) -> MapParams:
    """hs_map_params_default with the given fields replaced"""
    return _params_with(load().hs_map_params_default(), "map_params", kw)


def map_lds_capacity() -> int:
    return int(load().hs_map_lds_capacity())


def _flat(seqs):
    """list of code arrays -> (codes, offsets)"""
    off = np.zeros(len(seqs) + 1, np.int64)
    if len(seqs):
        np.cumsum([len(s) for s in seqs], out=off[1:])
    flat = np.concatenate([_np(s, np.uint8).reshape(-1) for s in seqs]) if len(seqs) and off[-1] else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat), off


def _reads_arg(reads):
    """a list of code arrays, or a (codes, offsets) pair -> (codes, offsets)"""
    return (_np(reads[0], np.uint8), _np(reads[1], np.int64)) if isinstance(reads, tuple) else _flat(reads)


class MapIndex:
    """hs_map_index: the contigs' minimizers, resident on the device until close(); serves any number of map_reads calls"""

    def __init__(self, handle, contig_seq, contig_off, params):
        self._h, self.contig_seq, self.contig_off, self.params = handle, contig_seq, contig_off, params

    def close(self):
        if self._h is not None:
            load().hs_map_index_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def entries(self) -> Dict:
        """hs_map_index_download: bucket_bits, bucket_off and the entries (hash, contig, t, strand bit) as the device holds them"""
        lib = load()
        n = C.c_int64(0); bits = C.c_int32(0)
        _check(lib.hs_map_index_download(self._h, C.byref(n), C.byref(bits), None, None, None, None))
        off = np.zeros((1 << bits.value) + 1, np.int64)
        h = np.zeros(max(n.value, 1), np.uint32); c = np.zeros(max(n.value, 1), np.int32); ts = np.zeros(max(n.value, 1), np.uint32)
        _check(lib.hs_map_index_download(self._h, None, None, off.ctypes.data, h.ctypes.data, c.ctypes.data, ts.ctypes.data))
        m = int(n.value)
        return {"bucket_bits": int(bits.value), "bucket_off": off, "hash": h[:m], "contig": c[:m], "t": (ts[:m] >> 1).astype(np.int64), "strand": (ts[:m] & 1).astype(np.uint8)}


def map_index(contigs, params: Optional[MapParams] = None) -> MapIndex:
    """hs_map_index_create. contigs: a list of code arrays (0..3), or a (codes, offsets) pair."""
    require_gpu()
    lib = load()
    cseq, coff = _reads_arg(contigs)
    prm = params if params is not None else lib.hs_map_params_default()
    h = C.c_void_p()
    _check(lib.hs_map_index_create(cseq.ctypes.data, coff.ctypes.data, C.c_int32(len(coff) - 1), C.byref(prm), C.byref(h)))
    return MapIndex(h, cseq, coff, prm)


def _map_call_stats(res, out):
    for k in ("n_wide", "total_minimizers", "total_hits"):
        out[k] = int(getattr(res, k))
    for k in ("t_minimizers_ms", "t_hits_ms", "t_vote_ms"):
        out[k] = float(getattr(res, k))
    return out


def _map_result_to_dict(r) -> Dict:
    res = r.contents
    n = int(res.n_reads)
    return _map_call_stats(res, {k: np.ctypeslib.as_array(getattr(res, k), shape=(n,)).copy() if n else np.zeros(0, np.int64) for k in MAP_FIELDS})


def map_reads(index: MapIndex, reads) -> Dict:
    """hs_map_reads: per read contig (-1 unmapped), strand, qstart, qend, tstart, tend, votes, second, n_minimizers, n_hits, n_skipped; per call n_wide.
    reads: a list of code arrays, or a (codes, offsets) pair."""
    lib = load()
    rseq, roff = _reads_arg(reads)
    r = C.POINTER(MapResult)()
    _check(lib.hs_map_reads(index._h, rseq.ctypes.data, roff.ctypes.data, C.c_int32(len(roff) - 1), C.byref(r)))
    try:
        return _map_result_to_dict(r)
    finally:
        lib.hs_map_result_destroy(r)


def map_intervals(res: Dict) -> np.ndarray:
    """the mapped reads of a map result as the rows realign_intervals takes: (read, contig, strand, qstart, qend, tstart, tend)"""
    m = np.flatnonzero(res["contig"] >= 0)
    return np.stack([m, res["contig"][m], res["strand"][m], res["qstart"][m], res["qend"][m], res["tstart"][m], res["tend"][m]], axis=1).astype(np.int64).reshape(-1, 7)


def _to_batch(fn, index, reads, pad, params, outs):
    """the one body of the three *_to_batch calls. params: () or (the call's parameter struct or None,); outs: (struct, its to-dict, its destroy) of
    every mapper output behind the records. Returns (CvBatch, records dict, one dict per output)."""
    import time
    lib = load()
    rseq, roff = _reads_arg(reads)
    h = C.c_void_p(); rec = C.POINTER(RealignRecords)()
    got = [C.POINTER(struct)() for struct, _, _ in outs]
    t0 = time.perf_counter()
    _check(getattr(lib, fn)(index._h, index.contig_seq.ctypes.data, index.contig_off.ctypes.data, C.c_int32(len(index.contig_off) - 1), rseq.ctypes.data, roff.ctypes.data,
                            C.c_int32(len(roff) - 1), C.c_int32(pad), *[C.byref(p) if p is not None else None for p in params], C.byref(h), C.byref(rec),
                            *[C.byref(p) for p in got]))
    dt = time.perf_counter() - t0
    try:
        records = _realign_records_to_dict(rec)
        dicts = [to_dict(p) for p, (_, to_dict, _) in zip(got, outs)]
    finally:
        lib.hs_realign_records_destroy(rec)
        for p, (_, _, destroy) in zip(got, outs):
            getattr(lib, destroy)(p)
    return (CvBatch._adopt(h, dt, records), records, *dicts)


def map_to_batch(index: MapIndex, reads, pad: int = 100):
    """hs_map_to_batch: map_reads, then realign_intervals on the mapped reads. Returns (CvBatch, records dict, map result dict)."""
    return _to_batch("hs_map_to_batch", index, reads, pad, (), [(MapResult, _map_result_to_dict, "hs_map_result_destroy")])


def _paf_text(fn, struct, n_reads, arrays, read_lengths, contig_lengths, read_names, contig_names):
    """the one PAF-text call: `struct` filled with n_reads and the arrays (name -> numpy array, kept alive here), the lengths as offsets, the names"""
    lib = load()
    struct.n_reads = n_reads
    for k, a in arrays.items():
        setattr(struct, k, a.ctypes.data_as(C.POINTER({np.dtype(np.uint8): C.c_uint8, np.dtype(np.int32): C.c_int32, np.dtype(np.int64): C.c_int64}[a.dtype])))
    roff = np.zeros(n_reads + 1, np.int64); np.cumsum(_np(read_lengths, np.int64), out=roff[1:])
    coff = np.zeros(len(contig_lengths) + 1, np.int64); np.cumsum(_np(contig_lengths, np.int64), out=coff[1:])
    names = lambda v: (C.c_char_p * len(v))(*[x.encode() for x in v]) if v is not None else None
    rn, cn = names(read_names), names(contig_names)
    text = C.c_char_p()
    _check(getattr(lib, fn)(C.byref(struct), rn, roff.ctypes.data, cn, coff.ctypes.data, C.c_int32(len(contig_lengths)), C.byref(text)))
    try:
        return text.value.decode()
    finally:
        lib.hs_free_host(text)


def map_text(res: Dict, read_lengths, contig_lengths, read_names=None, contig_names=None) -> str:
    """hs_map_text: the PAF lines of the mapped reads of a map result"""
    keep = {k: _np(res[k], np.uint8 if k == "strand" else np.int32) for k in ("contig", "strand", "qstart", "qend", "tstart", "tend", "votes", "second")}
    return _paf_text("hs_map_text", MapResult(), len(res["contig"]), keep, read_lengths, contig_lengths, read_names, contig_names)


def map_files(gfa: str, reads: str, out_paf: str, n_threads: int = 0, params: Optional[MapParams] = None):
    """hs_map_files: the job's files -> the PAF of the mapped reads (what bin/hs_map writes)"""
    require_gpu()
    _check(load().hs_map_files(gfa.encode(), reads.encode(), out_paf.encode(), C.c_int32(n_threads), C.byref(params) if params is not None else None))


# ---- split mappings (hs_map_reads_split): a read's parts on other contigs as further intervals ----
def map_split_params(**kw) -> MapSplitParams:
    """hs_map_split_params_default with the given fields replaced"""
    return _params_with(load().hs_map_split_params_default(), "map_split_params", kw)


def _map_segments_to_dict(g) -> Dict:
    res = g.contents
    n, s = int(res.n_reads), int(res.n_segments)
    out = {k: np.ctypeslib.as_array(getattr(res, k), shape=(s,)).copy() if s else np.zeros(0, np.int64) for k in MAP_SEG_FIELDS}
    out.update({k: np.ctypeslib.as_array(getattr(res, k), shape=(n,)).copy() if n else np.zeros(0, np.int64) for k in MAP_SEG_READ_FIELDS})
    out["seg_off"] = np.ctypeslib.as_array(res.seg_off, shape=(n + 1,)).copy()
    return _map_call_stats(res, out)


def map_reads_split(index: MapIndex, reads, split: Optional[MapSplitParams] = None) -> Dict:
    """hs_map_reads_split: seg_off [n_reads + 1]; per segment read, contig, strand, qstart, qend, tstart, tend, votes, second, round; per read n_minimizers,
    n_skipped, n_hits, read_votes, read_second; per call n_wide. reads: a list of code arrays, or a (codes, offsets) pair."""
    lib = load()
    rseq, roff = _reads_arg(reads)
    g = C.POINTER(MapSegments)()
    _check(lib.hs_map_reads_split(index._h, rseq.ctypes.data, roff.ctypes.data, C.c_int32(len(roff) - 1), C.byref(split) if split is not None else None, C.byref(g)))
    try:
        return _map_segments_to_dict(g)
    finally:
        lib.hs_map_segments_destroy(g)


def map_segment_intervals(res: Dict) -> np.ndarray:
    """the segments as the rows realign_intervals takes: (read, contig, strand, qstart, qend, tstart, tend)"""
    return np.stack([np.asarray(res[k], np.int64) for k in MAP_SEG_FIELDS[:7]], axis=1).reshape(-1, 7)


def map_split_to_batch(index: MapIndex, reads, split: Optional[MapSplitParams] = None, pad: int = 100):
    """hs_map_split_to_batch: map_reads_split, then realign_intervals with interval i = segment i. Returns (CvBatch, records dict, segments dict)."""
    return _to_batch("hs_map_split_to_batch", index, reads, pad, (split,), [(MapSegments, _map_segments_to_dict, "hs_map_segments_destroy")])


def map_segments_text(res: Dict, read_lengths, contig_lengths, read_names=None, contig_names=None) -> str:
    """hs_map_segments_text: one PAF line per segment of a map_reads_split result"""
    keep = {k: _np(res[k], np.uint8 if k == "strand" else np.int32) for k in MAP_SEG_FIELDS}
    keep["seg_off"] = _np(res["seg_off"], np.int64)
    g = MapSegments()
    g.n_segments = len(keep["read"])
    return _paf_text("hs_map_segments_text", g, len(keep["seg_off"]) - 1, keep, read_lengths, contig_lengths, read_names, contig_names)


# ---- anchored alignment (hs_map_reads_anchored, hs_realign_intervals_anchored): mapped reads cut at seed anchors before A1 ----
MAP_ANCHOR_READ_FIELDS = ("n_best", "n_chain", "n_supported")


def map_anchor_params(**kw) -> MapAnchorParams:
    """hs_map_anchor_params_default with the given fields replaced"""
    return _params_with(load().hs_map_anchor_params_default(), "map_anchor_params", kw)


def _map_anchors_to_dict(a) -> Dict:
    res = a.contents
    n, m = int(res.n_reads), int(res.n_anchors)
    out = {k: np.ctypeslib.as_array(getattr(res, k), shape=(m,)).copy() if m else np.zeros(0, np.int32) for k in ("anc_q", "anc_t")}
    out.update({k: np.ctypeslib.as_array(getattr(res, k), shape=(n,)).copy() if n else np.zeros(0, np.int32) for k in MAP_ANCHOR_READ_FIELDS})
    out["anc_off"] = np.ctypeslib.as_array(res.anc_off, shape=(n + 1,)).copy()
    out["t_anchors_ms"] = float(res.t_anchors_ms)
    return out


def map_reads_anchored(index: MapIndex, reads, params: Optional[MapAnchorParams] = None):
    """hs_map_reads_anchored: (map result dict as map_reads gives it, anchors dict): anc_off [n_reads + 1], anc_q (on the read as it aligns) and anc_t
    per anchor, n_best / n_chain / n_supported per read. reads: a list of code arrays, or a (codes, offsets) pair."""
    lib = load()
    rseq, roff = _reads_arg(reads)
    r = C.POINTER(MapResult)(); a = C.POINTER(MapAnchors)()
    _check(lib.hs_map_reads_anchored(index._h, rseq.ctypes.data, roff.ctypes.data, C.c_int32(len(roff) - 1), C.byref(params) if params is not None else None, C.byref(r), C.byref(a)))
    try:
        return _map_result_to_dict(r), _map_anchors_to_dict(a)
    finally:
        lib.hs_map_result_destroy(r)
        lib.hs_map_anchors_destroy(a)


def realign_intervals_anchored(flat_sequences, intervals, anc_off, anc_q, anc_t, pad: int = 100, want_batch: bool = True):
    """hs_realign_intervals_anchored: realign_intervals with the anchors of every interval given (anc_off [n_intervals + 1]; anc_q on the read as it
    aligns, anc_t on the contig). Every alignment is a cheapest one through its anchors, not edlib's HW optimum. Returns (records dict, CvBatch or None)."""
    return _realign("realign_intervals_anchored", flat_sequences, intervals, (anc_off, anc_q, anc_t), pad, want_batch)


def map_to_batch_anchored(index: MapIndex, reads, params: Optional[MapAnchorParams] = None, pad: int = 100):
    """hs_map_to_batch_anchored: map_reads_anchored, then realign_intervals_anchored on the mapped reads with their anchors. Returns (CvBatch, records
    dict, map result dict, anchors dict)."""
    return _to_batch("hs_map_to_batch_anchored", index, reads, pad, (params,),
                     [(MapResult, _map_result_to_dict, "hs_map_result_destroy"), (MapAnchors, _map_anchors_to_dict, "hs_map_anchors_destroy")])

