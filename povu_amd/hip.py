"""ctypes mirror of include/povu_hip.h.

Fails loudly when the HIP library is missing or no GPU is visible: there is no CPU
fallback on the product path (the CPU oracle lives under oracle/ and is test-only).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class HipUnavailable(RuntimeError):
    pass


class GuardBandError(RuntimeError):
    """A device-wide primitive wrote outside its output (raised by its unit-test hook, which guards every output)."""


# ops of povu_hip_debug_scan (include/povu_hip.h)
SCAN_SUM, SCAN_MAX, SCAN_U64, SCAN_U8, SCAN_DIFF, SCAN_XOR_PAIR, SCAN_XOR_U128, SCAN_DIFF_U8, SCAN_MIXED_PAIR, SCAN_DIFF_U8_U8, SCAN_INCLUSIVE = range(11)
SCAN_IN_PLACE, SCAN_N_DEV = 0x100, 0x200
# query kinds of povu_hip_debug_segtree
SEG_MIN, SEG_FIRST_LESS, SEG_LAST_LESS = range(3)


def lib_path() -> str:
    return os.path.join(_HERE, "lib", "libpovu_hip.so")


class _Opts(C.Structure):
    _fields_ = [("rank", C.c_uint32), ("world", C.c_uint32), ("flags", C.c_uint32)]


class _RankRecords(C.Structure):
    _fields_ = [("live", C.c_uint64), ("escaped", C.c_uint64), ("final_ranks", C.c_uint32), ("bucket_bits", C.c_uint32),
                ("delta_bits", C.c_uint32), ("partial_bits", C.c_uint32 * 2), ("hist", C.c_uint64 * (33 * 33))]


class _SubTree(C.Structure):
    _fields_ = [("n_total", C.c_uint32), ("n_flubble_like", C.c_uint32), ("n_concealed", C.c_uint32), ("n_midi", C.c_uint32),
                ("n_smothered", C.c_uint32), ("fam", C.POINTER(C.c_uint8)), ("or1", C.POINTER(C.c_uint8)),
                ("or2", C.POINTER(C.c_uint8)), ("route", C.POINTER(C.c_uint8)), ("id1", C.POINTER(C.c_uint32)),
                ("id2", C.POINTER(C.c_uint32)), ("child_off", C.POINTER(C.c_uint32)), ("child", C.POINTER(C.c_uint32))]


class _Tree(C.Structure):
    _fields_ = [("component_id", C.c_uint32), ("n_vtx", C.c_uint32), ("n_links", C.c_uint32),
                ("n_pvst", C.c_uint32), ("a_id", C.POINTER(C.c_uint32)), ("z_id", C.POINTER(C.c_uint32)),
                ("a_or", C.POINTER(C.c_uint8)), ("z_or", C.POINTER(C.c_uint8)), ("parent", C.POINTER(C.c_uint32)),
                ("n_hairpins", C.c_uint32), ("hairpins", C.POINTER(C.c_uint64))]


class _ShardInfo(C.Structure):
    _fields_ = [("n_vtx", C.c_uint32), ("n_links", C.c_uint32), ("n_components", C.c_uint32), ("weight", C.c_uint64),
                ("bytes", C.c_size_t), ("device_ptr", C.c_void_p)]


class _MultiRank(C.Structure):
    _fields_ = [("device", C.c_int), ("n_vtx", C.c_uint32), ("n_links", C.c_uint32), ("n_components", C.c_uint32),
                ("shard_bytes", C.c_uint64), ("recv_ms", C.c_double), ("csr_ms", C.c_double), ("decompose_ms", C.c_double),
                ("sink_ms", C.c_double), ("h2d", C.c_uint64), ("d2h", C.c_uint64), ("peer_out", C.c_uint64),
                ("peer_in", C.c_uint64)]


class _WalkOpts(C.Structure):
    _fields_ = [("max_walks", C.c_uint32), ("max_steps", C.c_uint32), ("max_expansions", C.c_uint32), ("flags", C.c_uint32)]


class _Walks(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_walks", C.c_uint64), ("n_steps", C.c_uint64),
                ("walk_off", C.POINTER(C.c_uint32)), ("step_off", C.POINTER(C.c_uint32)), ("step_id", C.POINTER(C.c_uint32)),
                ("step_or", C.POINTER(C.c_uint8)), ("status", C.POINTER(C.c_uint8)), ("n_tier2", C.c_uint64),
                ("device_ms", C.c_double)]


class _TravOpts(C.Structure):
    _fields_ = [("max_steps", C.c_uint32), ("flags", C.c_uint32)]


class _Traversals(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_traversals", C.c_uint64), ("n_alleles", C.c_uint64), ("n_steps", C.c_uint64),
                ("trav_off", C.POINTER(C.c_uint64)), ("allele_off", C.POINTER(C.c_uint64)), ("status", C.POINTER(C.c_uint8)),
                ("path", C.POINTER(C.c_uint32)), ("first", C.POINTER(C.c_uint32)), ("last", C.POINTER(C.c_uint32)),
                ("allele", C.POINTER(C.c_uint32)), ("reverse", C.POINTER(C.c_uint8)), ("step_off", C.POINTER(C.c_uint64)),
                ("step_id", C.POINTER(C.c_uint32)), ("step_or", C.POINTER(C.c_uint8)), ("n_tier2", C.c_uint64),
                ("n_hash_splits", C.c_uint64), ("device_ms", C.c_double)]


class _Sites(C.Structure):
    _fields_ = [("n", C.c_uint32), ("id1", C.POINTER(C.c_uint32)), ("id2", C.POINTER(C.c_uint32)), ("or1", C.POINTER(C.c_uint8)),
                ("or2", C.POINTER(C.c_uint8)), ("parent", C.POINTER(C.c_uint32)), ("height", C.POINTER(C.c_uint32)),
                ("family", C.POINTER(C.c_uint8)), ("tree", C.POINTER(C.c_uint32))]


class _CallRefs(C.Structure):
    _fields_ = [("n_refs", C.c_uint32), ("ref_path", C.POINTER(C.c_uint32)), ("n_slots", C.c_uint32), ("n_samples", C.c_uint32),
                ("sample_of_slot", C.POINTER(C.c_uint32))]


class _CallNames(C.Structure):
    _fields_ = [("refs", _CallRefs), ("n_paths", C.c_uint32), ("slot_of_path", C.POINTER(C.c_uint32)),
                ("sample", C.POINTER(C.c_char_p)), ("slot_hap", C.POINTER(C.c_int64))]


class _VcfDoc(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_samples", "n_records", "n_alleles", "n_steps", "n_text_bytes", "n_tasks", "n_id_bytes")] +
                [("sample", C.POINTER(C.c_char_p)), ("rec_line", C.POINTER(C.c_uint64)), ("rec_pos", C.POINTER(C.c_uint64)),
                 ("rec_id_off", C.POINTER(C.c_uint64)), ("ids", C.POINTER(C.c_uint8)), ("allele_off", C.POINTER(C.c_uint64)),
                 ("task_off", C.POINTER(C.c_uint64)), ("step_off", C.POINTER(C.c_uint64)), ("text_off", C.POINTER(C.c_uint64)),
                 ("allele_walk", C.POINTER(C.c_uint8)), ("step_id", C.POINTER(C.c_uint32)), ("step_or", C.POINTER(C.c_uint8)),
                 ("text", C.POINTER(C.c_uint8))] +
                [(k, C.POINTER(C.c_uint32)) for k in ("task_record", "task_allele", "task_col", "task_phase")] +
                [("n_chroms", C.c_uint64), ("chrom", C.POINTER(C.c_char_p)), ("rec_chrom", C.POINTER(C.c_uint32))])


# the counters of povu_hip_vcf_cmp behind its arrays (VcfComparison carries them under these names)
VCF_CMP_COUNTERS = ("n_shared", "n_only_a", "n_only_b", "n_skipped_a", "n_skipped_b", "n_samples_only_a", "n_samples_only_b", "n_tier2", "n_splits")


class _VcfOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32)]


class _VcfReport(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records", "n_tasks", "n_alleles")] +
                [(k, C.POINTER(C.c_uint8)) for k in ("task_status", "allele_spell", "rec_invalid", "rec_reason")] +
                [(k, C.POINTER(C.c_uint32)) for k in ("rec_allele", "rec_task")] +
                [("n_status", C.c_uint64 * 6), ("n_invalid", C.c_uint64), ("n_misspelled", C.c_uint64), ("n_tier2", C.c_uint64),
                 ("device_ms", C.c_double)])


class _VcfCmp(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_items_a", "n_items_b", "n_groups", "n_common_samples")] +
                [(k, C.POINTER(C.c_uint32)) for k in ("item_record_a", "item_record_b", "item_alt_a", "item_alt_b")] +
                [(k, C.POINTER(C.c_uint8)) for k in ("item_state_a", "item_state_b")] +
                [(k, C.POINTER(C.c_uint64)) for k in ("item_pos_a", "item_pos_b")] +
                [(k, C.POINTER(C.c_uint32)) for k in ("item_suffix_a", "item_suffix_b", "item_prefix_a", "item_prefix_b", "item_group_a",
                                                      "item_group_b")] +
                [("group_class", C.POINTER(C.c_uint8))] +
                [(k, C.POINTER(C.c_uint32)) for k in ("group_n_a", "group_n_b", "group_first", "sample_col_a", "sample_col_b")] +
                [(k, C.POINTER(C.c_uint64)) for k in ("sample_tp", "sample_fp", "sample_fn", "sample_gteq")] +
                [(k, C.c_uint64) for k in VCF_CMP_COUNTERS] + [("device_ms", C.c_double)])


# the counters of povu_hip_vcf_hap behind its arrays (HapComparison carries them under these names)
VCF_HAP_COUNTERS = ("n_inconsistent", "n_unplaced_a", "n_unplaced_b", "n_reach_capped", "n_tier2", "n_splits")
_HAP_ITEM_ARRAYS = (("item_record", C.c_uint32), ("item_alt", C.c_uint32), ("item_state", C.c_uint8), ("item_s", C.c_int64), ("item_e", C.c_int64),
                    ("item_suffix", C.c_uint32), ("item_prefix", C.c_uint32), ("item_left", C.c_uint32), ("item_right", C.c_uint32),
                    ("item_group", C.c_uint32))
_HAP_WIN_ARRAYS = (("win_chrom", C.c_uint32), ("win_lo", C.c_int64), ("win_hi", C.c_int64), ("win_n_a", C.c_uint32), ("win_n_b", C.c_uint32),
                   ("win_inconsistent", C.c_uint8), ("win_offender", C.c_uint32))
_HAP_CELL_ARRAYS = (("cell_window", C.c_uint32), ("cell_sample", C.c_uint32), ("cell_phase", C.c_uint32), ("cell_status", C.c_uint8),
                    ("cell_edits_a", C.c_uint32), ("cell_edits_b", C.c_uint32), ("cell_len_a", C.c_uint64), ("cell_len_b", C.c_uint64),
                    ("cell_first_diff", C.c_uint64))


class _VcfHapOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("max_reach", C.c_uint32)]


class _VcfHap(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records_a", "n_records_b", "n_items_a", "n_items_b", "n_groups", "n_windows", "n_cells",
                                           "n_common_samples")] +
                [(k, C.POINTER(C.c_uint8)) for k in ("rec_placed_a", "rec_placed_b")] +
                [(k, C.POINTER(C.c_uint32)) for k in ("rec_window_a", "rec_window_b")] +
                [(f"{k}_{side}", C.POINTER(t)) for k, t in _HAP_ITEM_ARRAYS[:2] for side in "ab"] +
                [(f"{k}_{side}", C.POINTER(t)) for k, t in _HAP_ITEM_ARRAYS[2:3] for side in "ab"] +
                [(f"{k}_{side}", C.POINTER(t)) for k, t in _HAP_ITEM_ARRAYS[3:5] for side in "ab"] +
                [(f"{k}_{side}", C.POINTER(t)) for k, t in _HAP_ITEM_ARRAYS[5:9] for side in "ab"] +
                [(f"{k}_{side}", C.POINTER(t)) for k, t in _HAP_ITEM_ARRAYS[9:] for side in "ab"] +
                [(k, C.POINTER(t)) for k, t in (_HAP_WIN_ARRAYS[0], _HAP_WIN_ARRAYS[1], _HAP_WIN_ARRAYS[2], _HAP_WIN_ARRAYS[3], _HAP_WIN_ARRAYS[4],
                                               _HAP_WIN_ARRAYS[5], _HAP_WIN_ARRAYS[6])] +
                [(k, C.POINTER(t)) for k, t in _HAP_CELL_ARRAYS] +
                [("sample_col_a", C.POINTER(C.c_uint32)), ("sample_col_b", C.POINTER(C.c_uint32)), ("sample_status", C.POINTER(C.c_uint64)),
                 ("n_status", C.c_uint64 * 10)] + [(k, C.c_uint64) for k in VCF_HAP_COUNTERS] +
                [("reference", C.c_uint32), ("device_ms", C.c_double)])


_CONS_ARRAYS = (("hap_chrom", C.c_uint32), ("hap_col", C.c_uint32), ("hap_phase", C.c_uint32), ("hap_len", C.c_uint64), ("hap_off", C.c_uint64),
                ("n_applied", C.c_uint32), ("n_duplicate", C.c_uint32), ("n_enclosed", C.c_uint32), ("n_overlap", C.c_uint32),
                ("n_unspelled", C.c_uint32), ("n_nocall", C.c_uint32), ("rt_status", C.c_uint8), ("rt_path", C.c_uint32),
                ("rt_path_len", C.c_uint64), ("rt_first_diff", C.c_uint64))


class _VcfConsOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("n_select", C.c_uint32), ("select_col", C.POINTER(C.c_uint32)), ("select_chrom", C.POINTER(C.c_uint32))]


class _VcfCons(C.Structure):
    _fields_ = ([("n_haps", C.c_uint64)] + [(k, C.POINTER(t)) for k, t in _CONS_ARRAYS] +
                [("text", C.POINTER(C.c_uint8)), ("n_text_bytes", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_tier2", C.c_uint64),
                 ("roundtrip", C.c_uint32), ("device_ms", C.c_double), ("write_ms", C.c_double)])


OFFREF_COUNTERS = ("n_offref_sites", "n_offref_records", "n_offref_hosted")  # of Calls
UNTANGLE_COUNTERS = ("n_unt_tasks", "n_unt_records", "n_unt_missing", "n_unt_extra", "n_unt_fallback")  # of Calls
REGION_COUNTERS = ("n_regions", "n_region_sites", "n_region_masked", "n_region_dropped")  # of Calls
REGION_NO_MASK = 1  # povu_hip_call_regions.flags: scan every site, select the records at the end only (tests)
CLUSTER_COUNTERS = ("n_cluster_sites", "n_clustered_sites", "n_cluster_vanished", "n_cluster_keys", "n_cluster_pairs", "n_cluster_pruned",
                    "n_cluster_tier2")  # of Calls
CLUSTER_NO_BOUND = 1  # povu_hip_call_cluster_opts.flags: no pair of bags is skipped by the weight bound (tests)
SPAN_COUNTERS = ("n_star_records", "n_star_entries")  # of Calls
MERGE_COUNTERS = ("n_merged_groups", "n_merged_members", "n_merge_splits", "n_ref_consistent", "n_gt_conflicts")  # of Calls, beside n_mrows


class _Calls(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records", "n_slots", "n_blocks", "n_spelled", "n_seq_bytes", "n_at_bytes", "n_refs")] +
                [(k, C.POINTER(C.c_uint32)) for k in ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "block")] +
                [("pos", C.POINTER(C.c_uint64)), ("flags", C.POINTER(C.c_uint8)), ("ac_off", C.POINTER(C.c_uint64)),
                 ("ac", C.POINTER(C.c_uint32)), ("gt", C.POINTER(C.c_uint16)), ("block_off", C.POINTER(C.c_uint64)),
                 ("seq_off", C.POINTER(C.c_uint64)), ("at_off", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint8)),
                 ("at", C.POINTER(C.c_uint8)), ("contig_len", C.POINTER(C.c_uint64)), ("device_ms", C.c_double),
                 ("n_steps", C.POINTER(C.c_uint32))] +
                [(k, C.c_uint64) for k in ("n_inv_records", "n_inv_heads", "n_inv_long", "n_inv_tier2")])


class _CallsNested(_Calls):
    """povu_hip_calls as povu_hip_call makes it now: the fields of "Nested calls" behind those above (povu_hip_calls_vcf, the
    entry of before, reads none of them; povu_hip_calls_vcf_profile does)."""
    _fields_ = ([("level", C.POINTER(C.c_uint32)), ("parent_query", C.POINTER(C.c_uint32)), ("ref_spelled", C.POINTER(C.c_uint64))] +
                [(k, C.c_uint64) for k in ("n_enclosed", "n_collapsed_sites", "n_popped", "n_rescued", "nested")] +
                # "Left-normalised calls"
                [("raw_pos", C.POINTER(C.c_uint64))] +
                [(k, C.POINTER(C.c_uint32)) for k in ("norm_block", "norm_shift", "norm_chop", "norm_trim")] +
                [(k, C.c_uint64) for k in ("n_normalized", "max_shift", "n_norm_compared")] +
                # "Decomposed calls"
                [("n_rows", C.c_uint64), ("row_record", C.POINTER(C.c_uint32)), ("row_alt", C.POINTER(C.c_uint32)),
                 ("row_kind", C.POINTER(C.c_uint8)), ("row_reason", C.POINTER(C.c_uint8)), ("row_index", C.POINTER(C.c_uint32)),
                 ("row_pos", C.POINTER(C.c_uint64))] +
                [(k, C.POINTER(C.c_uint32)) for k in ("row_ref_start", "row_ref_len", "row_alt_start", "row_alt_len")] +
                [("row_lead", C.POINTER(C.c_uint8))] +
                [(k, C.POINTER(C.c_uint32)) for k in ("row_ac", "row_an", "row_ns")] +
                [(k, C.c_uint64) for k in ("n_decomposed_alts", "n_passthrough_alts", "n_prim_tier2", "n_prim_cells")] +
                # "Merged primitives"
                [("merged", C.c_uint64), ("n_mrows", C.c_uint64), ("mrow_off", C.POINTER(C.c_uint64)),
                 ("mrow_member", C.POINTER(C.c_uint32)), ("mrow_gt", C.POINTER(C.c_uint8))] +
                [(k, C.POINTER(C.c_uint32)) for k in ("mrow_ac", "mrow_an", "mrow_ns")] +
                [(k, C.c_uint64) for k in MERGE_COUNTERS] +
                # "Off-reference calls"
                [("offref", C.c_uint64), ("rec_offref", C.POINTER(C.c_uint8)), ("host_query", C.POINTER(C.c_uint32)),
                 ("host_allele", C.POINTER(C.c_uint32)), ("n_off_contigs", C.c_uint64), ("off_contig_path", C.POINTER(C.c_uint32)),
                 ("off_contig_len", C.POINTER(C.c_uint64))] +
                [(k, C.c_uint64) for k in OFFREF_COUNTERS] +
                # "Untangled calls"
                [("untangled", C.c_uint64), ("rec_unt", C.POINTER(C.c_uint8)), ("lap", C.POINTER(C.c_uint32)),
                 ("n_laps", C.POINTER(C.c_uint32)), ("lap_count", C.POINTER(C.c_uint16))] +
                [(k, C.c_uint64) for k in UNTANGLE_COUNTERS] +
                # "Region calls"
                [(k, C.c_uint64) for k in REGION_COUNTERS] +
                # "Clustered calls"
                [("cluster_ppm", C.c_uint64), ("rec_clustered", C.POINTER(C.c_uint8)), ("cl_minsim", C.POINTER(C.c_uint32)),
                 ("cl_nx", C.POINTER(C.c_uint32))] +
                [(k, C.c_uint64) for k in CLUSTER_COUNTERS] +
                # "Spanning alleles"
                [("spanning", C.c_uint64), ("rec_star", C.POINTER(C.c_uint8))] +
                [(k, C.c_uint64) for k in SPAN_COUNTERS])


class _ClusterOpts(C.Structure):
    _fields_ = [("min_similarity_ppm", C.c_uint32), ("flags", C.c_uint32)]


class _Region(C.Structure):
    _fields_ = [("path", C.c_uint32), ("reserved", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64)]


class _CallRegions(C.Structure):
    _fields_ = [("n", C.c_uint32), ("flags", C.c_uint32), ("region", C.POINTER(_Region))]


class _ProfileOpts(C.Structure):
    _fields_ = [("profile", C.c_uint32), ("max_level", C.c_uint32), ("max_ref_length", C.c_uint64),
                ("max_allele_length", C.c_uint64)]


class _StageTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_double), ("launches", C.c_uint32)]


class _ArenaInfo(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("resident", C.c_int), ("bytes", C.c_uint64)]


class _Components(C.Structure):
    _fields_ = [("n_components", C.c_uint32), ("n_vtx", C.c_uint32), ("n_links", C.c_uint32),
                ("vtx_off", C.POINTER(C.c_uint32)), ("link_off", C.POINTER(C.c_uint32)), ("vtx_id", C.POINTER(C.c_uint32)),
                ("vtx_tip", C.POINTER(C.c_uint8)), ("l_v1", C.POINTER(C.c_uint32)), ("l_v2", C.POINTER(C.c_uint32)),
                ("l_s1", C.POINTER(C.c_uint8)), ("l_s2", C.POINTER(C.c_uint8))]


class _RowB(C.Structure):
    _fields_ = [("n_components", C.c_uint32), ("n_local_slots", C.c_uint32), ("stats0", C.c_uint32), ("path_bits", C.c_uint32),
                ("n_cross", C.c_uint32), ("voff", C.c_void_p), ("eoff", C.c_void_p), ("comp", C.c_void_p), ("pos", C.c_void_p),
                ("loff", C.c_void_p), ("ladj", C.c_void_p), ("lle", C.c_void_p), ("start_key", C.c_void_p)]


F_HAIRPINS = 1
F_SEQUENTIAL = 2
F_SEQ_TREE = 4
F_FORCE_REDO = 8
F_SORTED_ADJ = 16
F_NO_STAGE_TIMES = 32
F_BIG_CLASS_DFS = 64
F_SPARSE_SPLITTERS = 128
F_REDO_ODD = 256
F_ALL_VERTEX_CLASSES = 512
F_CHECK_LAMINAR = 1024
F_LEAF_SUBFLUBBLES = 2048
F_ASYNC = 4096
F_SUBFLUBBLES = 8192  # all five passes of -s (implies F_LEAF_SUBFLUBBLES): Forest.texts() then carry C / M / S lines

# HipDecomposer.debug_row_b: the path row B took (povu_hip_rowb.path_bits), and the two parts of a word of `lle`
ROWB_IDENTITY, ROWB_SORT_FREE, ROWB_LEAN_IDENTITY, ROWB_SELF_LOOPS, ROWB_DENSE_EDGES, ROWB_SPEC_KEPT = 1, 2, 4, 8, 16, 32
LLE_ID, LLE_TREE = 0x1FFFFFFF, 0x40000000

W_FORCE_TIER2 = 1  # HipDecomposer.walks: every query through the second-tier kernel (tests)
WALK_MORE, WALK_LONG, WALK_BUDGET = 1, 2, 4  # status bits of a query
T_FORCE_TIER2 = 1  # HipDecomposer.traversals: every scan through the wave-per-scan kernel (tests)
T_INVERSIONS = 2  # HipDecomposer.call: inversion (SUBR) records too (INTEGRATION.md "Inversion calls")
T_NESTED = 4  # HipDecomposer.call: alleles modulo enclosed sites, levels and parents by geometry (INTEGRATION.md "Nested calls")
# HipDecomposer.call under profile "decomposed" only: equal primitives merged into one row with joint genotypes (INTEGRATION.md
# "Merged primitives")
T_MERGE = 8
# HipDecomposer.call under profile "raw-graph" only, not with T_NESTED or T_MERGE: the sites no reference path crosses, called
# on the first path that traverses them (INTEGRATION.md "Off-reference calls")
T_OFFREF = 16
# HipDecomposer.call under profile "raw-graph" only, not with T_NESTED, T_MERGE or T_OFFREF: where a path walks a site more than
# once its laps are aligned with the reference's and every copy is genotyped on its own (INTEGRATION.md "Untangled calls")
T_UNTANGLE = 32
# HipDecomposer.call with T_NESTED or a profile that implies it only: a `*` ALT where an enclosing allele deletes the site
# (INTEGRATION.md "Spanning alleles"; HipDecomposer.call(..., spanning=True) sets it)
T_SPANNING = 64
TRAV_LONG, TRAV_STRAY, TRAV_OPEN = 1, 2, 4  # status bits of a query
PROFILES = {"raw-graph": 0, "top-level-only": 1, "popped": 2, "left-normalized": 3, "decomposed": 4}  # HipDecomposer.call(profile=...)
PRIM_MAX_LENGTH = 512  # `decomposed` profile: the longest allele that is aligned, and the most max_allele_length may ask for
# kind of a row of the `decomposed` profile (Calls.row_kind) and why a ROW_PASS row was kept whole (Calls.row_reason)
ROW_RAW, ROW_SNP, ROW_INS, ROW_DEL, ROW_PASS = 0, 1, 2, 3, 4
REASON_NONE, REASON_MAX_ALLELE_LENGTH, REASON_CONTIG_START, REASON_EMPTY_ALLELE, REASON_EQUALS_REF, REASON_SUBR = 0, 1, 2, 3, 4, 5

# "VCF checks" (HipDecomposer.check_vcf): the status of a task, V_MISSPELLED as a record's reason beside them; the spelling of an
# allele; the flags of povu_hip_vcf_check
V_FOUND_FWD, V_FOUND_REV, V_ABSENT, V_NO_AT, V_BAD_STEP, V_NO_SLOT, V_MISSPELLED = range(7)
V_STATUS_NAMES = ("found_fwd", "found_rev", "absent", "no_at", "bad_step", "no_slot", "misspelled")
V_SPELL_NONE, V_SPELL_WHOLE, V_SPELL_ANCHORED, V_SPELL_MISSPELLED = range(4)
V_FORWARD_ONLY, V_SPELLING, V_FORCE_TIER2 = 1, 2, 4
# "VCF comparison" (HipDecomposer.compare_vcfs): the state of an item, the class of a group
M_KEYED, M_SKIPPED = 0, 1
M_SHARED, M_ONLY_A, M_ONLY_B = 0, 1, 2
# "Haplotype comparison" (HipDecomposer.compare_haplotypes): the state of an item, the status of a cell
H_EDIT, H_UNSPELLED, H_UNPLACED = 0, 1, 2
(H_INCONSISTENT, H_NOCALL_A, H_NOCALL_B, H_UNSPELLED_A, H_UNSPELLED_B, H_CONFLICT_A, H_CONFLICT_B, H_EQUAL_REF, H_EQUAL, H_DIFFER) = range(10)
H_STATUS_NAMES = ("inconsistent", "nocall_a", "nocall_b", "unspelled_a", "unspelled_b", "conflict_a", "conflict_b", "equal_ref", "equal", "differ")
H_MAX_REACH_DEFAULT, H_MAX_REACH_MOST = 256, 65536
# "Consensus haplotypes" (HipDecomposer.consensus): the flags, the materialiser's tile, the round trip of a haplotype
C_ROUNDTRIP, C_NO_TEXT, C_TIME_WRITE = 1, 2, 8
C_TILE_BYTES = 4096
C_RT_NONE, C_RT_EQUAL, C_RT_DIFFER, C_RT_NO_PATH, C_RT_AMBIGUOUS = range(5)
C_RT_NAMES = ("none", "equal", "differ", "no_path", "ambiguous")

_lib = None


def load_lib():
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise HipUnavailable(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback)")
    l = C.CDLL(p)
    l.povu_hip_device_count.restype = C.c_int
    l.povu_hip_create.restype = C.c_void_p
    l.povu_hip_create.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    l.povu_hip_destroy.argtypes = [C.c_void_p]
    l.povu_hip_release_workspace.restype = C.c_int
    l.povu_hip_release_workspace.argtypes = [C.c_void_p]
    l.povu_hip_graph_upload.restype = C.c_int
    l.povu_hip_graph_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_last_upload_times.restype = C.c_int
    l.povu_hip_last_upload_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    l.povu_hip_decompose.restype = C.c_void_p
    l.povu_hip_decompose.argtypes = [C.c_void_p, C.POINTER(_Opts), C.c_char_p, C.c_size_t]
    l.povu_hip_forest_total_components.restype = C.c_uint32
    l.povu_hip_forest_total_components.argtypes = [C.c_void_p]
    l.povu_hip_forest_tree_count.restype = C.c_uint32
    l.povu_hip_forest_tree_count.argtypes = [C.c_void_p]
    l.povu_hip_forest_get.restype = C.c_int
    l.povu_hip_forest_get.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_Tree)]
    l.povu_hip_forest_free.argtypes = [C.c_void_p]
    l.povu_hip_forest_wait.restype = C.c_int
    l.povu_hip_forest_wait.argtypes = [C.c_void_p]
    l.povu_hip_forest_pass_ms.restype = C.c_double
    l.povu_hip_forest_pass_ms.argtypes = [C.c_void_p]
    l.povu_hip_forest_span_ms.restype = C.c_double
    l.povu_hip_forest_span_ms.argtypes = [C.c_void_p, C.c_void_p]
    l.povu_hip_forest_get_subtree.restype = C.c_int
    l.povu_hip_forest_get_subtree.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    l.povu_hip_forest_get_sub.restype = C.c_int
    l.povu_hip_forest_get_sub.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(C.c_uint32)),
                                          C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint8))]
    l.povu_hip_forest_raw.restype = C.c_int
    l.povu_hip_forest_raw.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
    l.povu_hip_forest_walks.restype = C.POINTER(_Walks)
    l.povu_hip_forest_walks.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_WalkOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_walks_free.argtypes = [C.POINTER(_Walks)]
    l.povu_hip_paths_upload.restype = C.c_int
    l.povu_hip_paths_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_forest_traversals.restype = C.POINTER(_Traversals)
    l.povu_hip_forest_traversals.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_TravOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_traversals_free.argtypes = [C.POINTER(_Traversals)]
    l.povu_hip_forest_first.restype = C.c_uint64
    l.povu_hip_segments_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_segments_upload.restype = C.c_int
    l.povu_hip_call.argtypes = [C.c_void_p, C.POINTER(_Sites), C.POINTER(_CallRefs), C.POINTER(C.c_uint32), C.POINTER(_TravOpts),
                                C.c_char_p, C.c_size_t]
    l.povu_hip_call.restype = C.POINTER(_CallsNested)
    l.povu_hip_call_profile.argtypes = [C.c_void_p, C.POINTER(_Sites), C.POINTER(_CallRefs), C.POINTER(C.c_uint32), C.POINTER(_TravOpts),
                                        C.POINTER(_ProfileOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_call_profile.restype = C.POINTER(_CallsNested)
    l.povu_hip_call_restricted.argtypes = [C.c_void_p, C.POINTER(_Sites), C.POINTER(_CallRefs), C.POINTER(C.c_uint32), C.POINTER(_TravOpts),
                                           C.POINTER(_ProfileOpts), C.POINTER(_CallRegions), C.c_char_p, C.c_size_t]
    l.povu_hip_call_restricted.restype = C.POINTER(_CallsNested)
    l.povu_hip_region_parse.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(_Region), C.c_char_p, C.c_size_t]
    l.povu_hip_region_parse.restype = C.c_int
    l.povu_hip_call_clustered.argtypes = [C.c_void_p, C.POINTER(_Sites), C.POINTER(_CallRefs), C.POINTER(C.c_uint32), C.POINTER(_TravOpts),
                                          C.POINTER(_ProfileOpts), C.POINTER(_CallRegions), C.POINTER(_ClusterOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_call_clustered.restype = C.POINTER(_CallsNested)
    l.povu_hip_cluster_parse.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    l.povu_hip_cluster_parse.restype = C.c_int
    l.povu_hip_calls_vcf_profile.argtypes = [C.POINTER(_CallsNested), C.POINTER(_Sites), C.POINTER(_CallNames), C.POINTER(C.c_char_p),
                                             C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]
    l.povu_hip_calls_vcf_profile.restype = C.c_void_p
    l.povu_hip_calls_vcf_rest.argtypes = [C.POINTER(_CallsNested), C.POINTER(_Sites), C.POINTER(_CallNames), C.POINTER(C.c_char_p),
                                          C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]
    l.povu_hip_calls_vcf_rest.restype = C.c_void_p
    l.povu_hip_calls_free.argtypes = [C.POINTER(_Calls)]
    l.povu_hip_call_names_make.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_char_p,
                                           C.c_size_t]
    l.povu_hip_call_names_make.restype = C.POINTER(_CallNames)
    l.povu_hip_call_names_free.argtypes = [C.POINTER(_CallNames)]
    l.povu_hip_sites_of_docs.argtypes = [C.c_void_p, C.c_uint32]  # (an array of povu_pvst_doc pointers)
    l.povu_hip_sites_of_docs.restype = C.POINTER(_Sites)
    l.povu_hip_forest_sites.argtypes = [C.c_void_p]
    l.povu_hip_forest_sites.restype = C.POINTER(_Sites)
    l.povu_hip_sites_free.argtypes = [C.POINTER(_Sites)]
    l.povu_hip_calls_vcf.argtypes = [C.POINTER(_Calls), C.POINTER(_Sites), C.POINTER(_CallNames), C.POINTER(C.c_char_p), C.c_char_p,
                                     C.c_char_p, C.c_uint32, C.POINTER(C.c_size_t)]
    l.povu_hip_calls_vcf.restype = C.c_void_p
    l.povu_hip_forest_first.argtypes = [C.c_void_p, C.c_uint32]
    l.povu_hip_vcf_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_char_p, C.c_size_t]
    l.povu_hip_vcf_parse.restype = C.POINTER(_VcfDoc)
    l.povu_hip_vcf_doc_free.argtypes = [C.POINTER(_VcfDoc)]
    l.povu_hip_vcf_names_make.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    l.povu_hip_vcf_names_make.restype = C.POINTER(_CallNames)
    l.povu_hip_vcf_columns.argtypes = [C.POINTER(_VcfDoc), C.POINTER(_CallNames), C.c_void_p, C.c_void_p]
    l.povu_hip_vcf_columns.restype = C.c_int
    l.povu_hip_vcf_check.argtypes = [C.c_void_p, C.POINTER(_VcfDoc), C.POINTER(_CallNames), C.POINTER(_VcfOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_vcf_check.restype = C.POINTER(_VcfReport)
    l.povu_hip_vcf_report_free.argtypes = [C.POINTER(_VcfReport)]
    l.povu_hip_vcf_report_text.argtypes = [C.POINTER(_VcfReport), C.POINTER(_VcfDoc), C.POINTER(_CallNames), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    l.povu_hip_vcf_report_text.restype = C.c_void_p
    l.povu_hip_vcf_compare.argtypes = [C.c_void_p, C.POINTER(_VcfDoc), C.POINTER(_VcfDoc), C.POINTER(_VcfOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_vcf_compare.restype = C.POINTER(_VcfCmp)
    l.povu_hip_vcf_cmp_free.argtypes = [C.POINTER(_VcfCmp)]
    l.povu_hip_vcf_cmp_text.argtypes = [C.POINTER(_VcfCmp), C.POINTER(_VcfDoc), C.POINTER(_VcfDoc), C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    l.povu_hip_vcf_cmp_text.restype = C.c_void_p
    l.povu_hip_vcf_haplotypes.argtypes = [C.c_void_p, C.POINTER(_VcfDoc), C.POINTER(_VcfDoc), C.POINTER(C.c_char_p), C.c_uint32,
                                          C.POINTER(_VcfHapOpts), C.c_char_p, C.c_size_t]
    l.povu_hip_vcf_haplotypes.restype = C.POINTER(_VcfHap)
    l.povu_hip_vcf_hap_free.argtypes = [C.POINTER(_VcfHap)]
    l.povu_hip_vcf_hap_text.argtypes = [C.POINTER(_VcfHap), C.POINTER(_VcfDoc), C.POINTER(_VcfDoc), C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    l.povu_hip_vcf_hap_text.restype = C.c_void_p
    l.povu_hip_vcf_consensus.argtypes = [C.c_void_p, C.POINTER(_VcfDoc), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(_VcfConsOpts), C.c_char_p,
                                         C.c_size_t]
    l.povu_hip_vcf_consensus.restype = C.POINTER(_VcfCons)
    l.povu_hip_vcf_cons_free.argtypes = [C.POINTER(_VcfCons)]
    l.povu_hip_vcf_cons_text.argtypes = [C.POINTER(_VcfCons), C.POINTER(_VcfDoc), C.POINTER(_CallNames), C.POINTER(C.c_char_p), C.c_uint32,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_size_t)]
    l.povu_hip_vcf_cons_text.restype = C.c_void_p
    l.povu_hip_forest_pvst_text.restype = C.c_void_p
    l.povu_hip_forest_pvst_text.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_size_t)]
    l.povu_hip_buffer_free.argtypes = [C.c_void_p]
    l.povu_hip_last_stage_times.restype = C.c_int
    l.povu_hip_last_stage_times.argtypes = [C.c_void_p, C.POINTER(_StageTime), C.c_int]
    l.povu_hip_arena_report.restype = C.c_int
    l.povu_hip_arena_report.argtypes = [C.c_void_p, C.POINTER(_ArenaInfo), C.c_int]
    l.povu_hip_last_seq_redo.restype = C.c_uint32
    l.povu_hip_last_seq_redo.argtypes = [C.c_void_p]
    l.povu_hip_last_links_processed.restype = C.c_uint64
    l.povu_hip_last_links_processed.argtypes = [C.c_void_p]
    l.povu_hip_debug_components.restype = C.c_int
    l.povu_hip_debug_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.povu_hip_debug_csr.restype = C.c_int
    l.povu_hip_debug_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    l.povu_hip_debug_row_b.restype = C.c_int
    l.povu_hip_debug_row_b.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_RowB)]
    l.povu_hip_componetize.restype = C.POINTER(_Components)
    l.povu_hip_componetize.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_components_free.restype = None
    l.povu_hip_components_free.argtypes = [C.POINTER(_Components)]
    l.povu_hip_debug_tree.restype = C.c_int
    l.povu_hip_debug_tree.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    l.povu_hip_last_narrow_counts.restype = C.c_int
    l.povu_hip_last_narrow_counts.argtypes = [C.c_void_p]
    l.povu_hip_wide_repeats.restype = C.c_uint64
    l.povu_hip_wide_repeats.argtypes = [C.c_void_p]
    l.povu_hip_last_black_only_classes.restype = C.c_int
    l.povu_hip_last_black_only_classes.argtypes = [C.c_void_p]
    l.povu_hip_last_crossings.restype = C.c_int
    l.povu_hip_last_crossings.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    l.povu_hip_last_lsz_field.restype = C.c_int
    l.povu_hip_last_lsz_field.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    l.povu_hip_last_laminar_check_ran.restype = C.c_int
    l.povu_hip_last_laminar_check_ran.argtypes = [C.c_void_p]
    l.povu_hip_debug_edge_ids.restype = C.c_int
    l.povu_hip_debug_edge_ids.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    l.povu_hip_debug_walk_words.restype = C.c_int
    l.povu_hip_debug_walk_words.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    l.povu_hip_debug_splice_pool.restype = C.c_int
    l.povu_hip_debug_splice_pool.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    l.povu_hip_debug_stack.restype = C.c_int
    l.povu_hip_debug_stack.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    l.povu_hip_version.restype = C.c_char_p
    l.povu_hip_debug_scan.restype = C.c_int
    l.povu_hip_debug_scan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                      C.c_size_t]
    l.povu_hip_debug_sort.restype = C.c_int
    l.povu_hip_debug_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p]
    l.povu_hip_debug_compact.restype = C.c_int
    l.povu_hip_debug_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
    l.povu_hip_debug_totals.restype = C.c_int
    l.povu_hip_debug_totals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    l.povu_hip_debug_segtree.restype = C.c_int
    l.povu_hip_debug_segtree.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_uint32)]
    l.povu_hip_last_prefix_records.restype = C.c_int
    l.povu_hip_last_prefix_records.argtypes = [C.c_void_p]
    l.povu_hip_debug_count_records.restype = C.c_int
    l.povu_hip_debug_count_records.argtypes = [C.c_void_p] + 2 * [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                  C.c_void_p, C.c_void_p] + [C.c_void_p]
    l.povu_hip_debug_bitrank.restype = C.c_int
    l.povu_hip_debug_bitrank.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    l.povu_hip_debug_append.restype = C.c_int
    l.povu_hip_debug_append.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
    l.povu_hip_debug_rank_escapes.restype = C.c_int
    l.povu_hip_debug_rank_escapes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    l.povu_hip_debug_list_rank.restype = C.c_int
    l.povu_hip_debug_list_rank.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    l.povu_hip_workspace_estimate.restype = C.c_uint64
    l.povu_hip_workspace_estimate.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    l.povu_hip_prewarm.restype = C.c_int
    l.povu_hip_prewarm.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    l.povu_hip_leaf_workspace_estimate.restype = C.c_uint64
    l.povu_hip_leaf_workspace_estimate.argtypes = [C.c_uint32, C.c_uint32]
    # ---- multi-GPU sharding
    l.povu_hip_lpt_assign.restype = C.c_int
    l.povu_hip_lpt_assign.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    l.povu_hip_shard_partition.restype = C.c_void_p
    l.povu_hip_shard_partition.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]
    l.povu_hip_shards_world.restype = C.c_uint32
    l.povu_hip_shards_world.argtypes = [C.c_void_p]
    l.povu_hip_shards_total_components.restype = C.c_uint32
    l.povu_hip_shards_total_components.argtypes = [C.c_void_p]
    l.povu_hip_shards_get.restype = C.c_int
    l.povu_hip_shards_get.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_ShardInfo)]
    l.povu_hip_shards_times.restype = C.c_int
    l.povu_hip_shards_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    l.povu_hip_shards_export.restype = C.c_int
    l.povu_hip_shards_export.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    l.povu_hip_shards_free.argtypes = [C.c_void_p]
    l.povu_hip_graph_upload_shard.restype = C.c_int
    l.povu_hip_graph_upload_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
    l.povu_hip_shard_total_components.restype = C.c_uint32
    l.povu_hip_shard_total_components.argtypes = [C.c_void_p]
    l.povu_hip_forest_globalize.restype = C.c_int
    l.povu_hip_forest_globalize.argtypes = [C.c_void_p, C.c_void_p]
    l.povu_hip_forest_pack_size.restype = C.c_size_t
    l.povu_hip_forest_pack_size.argtypes = [C.c_void_p]
    l.povu_hip_forest_pack.restype = C.c_int
    l.povu_hip_forest_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    l.povu_hip_forest_merge.restype = C.c_void_p
    l.povu_hip_forest_merge.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32, C.c_char_p,
                                        C.c_size_t]
    l.povu_hip_comm_unique_id.restype = C.c_int
    l.povu_hip_comm_unique_id.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    l.povu_hip_comm_create.restype = C.c_void_p
    l.povu_hip_comm_create.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    l.povu_hip_comm_destroy.argtypes = [C.c_void_p]
    l.povu_hip_comm_scatter.restype = C.c_int
    l.povu_hip_comm_scatter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_comm_gather.restype = C.c_void_p
    l.povu_hip_comm_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_comm_times.restype = C.c_int
    l.povu_hip_comm_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    l.povu_hip_share_results.restype = C.c_int
    l.povu_hip_share_results.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    l.povu_hip_forest_share.restype = C.c_int
    l.povu_hip_forest_share.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    l.povu_hip_forest_attach.restype = C.c_void_p
    l.povu_hip_forest_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint32, C.c_char_p,
                                         C.c_size_t]
    l.povu_hip_transfer_bytes.restype = C.c_int
    l.povu_hip_transfer_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    # ---- one process, N GPUs
    l.povu_hip_multi_create.restype = C.c_void_p
    l.povu_hip_multi_create.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.c_char_p, C.c_size_t]
    l.povu_hip_multi_destroy.argtypes = [C.c_void_p]
    l.povu_hip_multi_world.restype = C.c_uint32
    l.povu_hip_multi_world.argtypes = [C.c_void_p]
    l.povu_hip_multi_upload.restype = C.c_int
    l.povu_hip_multi_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_multi_scatter.restype = C.c_int
    l.povu_hip_multi_scatter.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    l.povu_hip_multi_decompose.restype = C.c_void_p
    l.povu_hip_multi_decompose.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    l.povu_hip_multi_rank.restype = C.c_int
    l.povu_hip_multi_rank.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_MultiRank)]
    l.povu_hip_multi_times.restype = C.c_int
    l.povu_hip_multi_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    l.povu_hip_multi_transport.restype = C.c_char_p
    l.povu_hip_multi_transport.argtypes = [C.c_void_p]
    l.povu_hip_gfa_write.restype = C.c_int
    l.povu_hip_gfa_write.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_char_p, C.c_size_t]
    _lib = l
    return l


def write_gfa(links, path: str) -> None:
    """GFA v1 text of a workloads.Links through the host library's writer (host only, no GPU needed)."""
    l = load_lib()
    vid = np.ascontiguousarray(links.vid, dtype=np.uint32)
    v1 = np.ascontiguousarray(links.v1, dtype=np.uint32)
    v2 = np.ascontiguousarray(links.v2, dtype=np.uint32)
    s1 = np.ascontiguousarray(links.s1, dtype=np.uint8)
    s2 = np.ascontiguousarray(links.s2, dtype=np.uint8)
    err = C.create_string_buffer(512)
    if l.povu_hip_gfa_write(path.encode(), len(vid), vid.ctypes.data, len(v1), v1.ctypes.data, s1.ctypes.data,
                            v2.ctypes.data, s2.ctypes.data, err, 512) != 0:
        raise RuntimeError(err.value.decode())


def lpt_assign(weights, world: int) -> np.ndarray:
    """The library's LPT rule (host only): heaviest first (stable), least loaded rank, +1 per item."""
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    out = np.zeros(len(w), dtype=np.uint32)
    if load_lib().povu_hip_lpt_assign(w.ctypes.data, len(w), world, out.ctypes.data) != 0:
        raise ValueError("bad LPT arguments")
    return out


@dataclass
class PvstTree:
    component_id: int
    n_vtx: int
    n_links: int
    a_id: np.ndarray
    z_id: np.ndarray
    a_or: np.ndarray
    z_or: np.ndarray
    parent: np.ndarray
    hairpins: np.ndarray
    text: Optional[str] = None


class Forest:
    """Result of one decompose call (host memory)."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.povu_hip_forest_free(self._h)
            self._h = None

    def wait(self) -> "Forest":
        """Completes a forest of a decompose with F_ASYNC (its arrays may still be on their way to the host)."""
        self._lib.povu_hip_forest_wait(self._h)
        return self

    def pass_ms(self) -> float:
        """HIP-event time of the pass that produced this forest: first kernel to last byte on the host (waits first)."""
        return float(self._lib.povu_hip_forest_pass_ms(self._h))

    def span_ms(self, last: "Forest") -> float:
        """HIP-event time from this forest's first kernel to the last byte of `last` (a later pass of the same context)."""
        return float(self._lib.povu_hip_forest_span_ms(self._h, last._h))

    @property
    def total_components(self) -> int:
        return self._lib.povu_hip_forest_total_components(self._h)

    def __len__(self) -> int:
        return self._lib.povu_hip_forest_tree_count(self._h)

    def pvst_sizes(self) -> List[int]:
        """PVST vertices of every tree (no array is copied)."""
        out = []
        t = _Tree()
        for i in range(len(self)):
            if self._lib.povu_hip_forest_get(self._h, i, C.byref(t)) != 0:
                raise IndexError(i)
            out.append(int(t.n_pvst))
        return out

    def tree(self, i: int, with_text: bool = False) -> PvstTree:
        t = _Tree()
        if self._lib.povu_hip_forest_get(self._h, i, C.byref(t)) != 0:
            raise IndexError(i)
        n = t.n_pvst
        arr = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)  # noqa: E731
        hp = (np.ctypeslib.as_array(t.hairpins, shape=(2 * t.n_hairpins,)).reshape(-1, 2).copy()
              if t.n_hairpins else np.zeros((0, 2), dtype=np.uint64))
        out = PvstTree(t.component_id, t.n_vtx, t.n_links, arr(t.a_id, np.uint32), arr(t.z_id, np.uint32),
                       arr(t.a_or, np.uint8), arr(t.z_or, np.uint8), arr(t.parent, np.uint32), hp)
        if with_text:
            out.text = self.text(i)
        return out

    def sub(self, i: int):
        """(ai, zi, line letters) of tree i after a decompose with F_LEAF_SUBFLUBBLES: compute_ai_zi's spanning-tree
        vertices (flubbles.cpp:264-290) and 'D' / 'F' / 'T' / 'O' per PVST vertex."""
        t = _Tree()
        if self._lib.povu_hip_forest_get(self._h, i, C.byref(t)) != 0:
            raise IndexError(i)
        ai, zi, fam = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        rc = self._lib.povu_hip_forest_get_sub(self._h, i, C.byref(ai), C.byref(zi), C.byref(fam))
        if rc != 0:
            raise RuntimeError(f"forest carries no subflubble labels (rc {rc})")
        n = t.n_pvst
        return (np.ctypeslib.as_array(ai, shape=(n,)).copy(), np.ctypeslib.as_array(zi, shape=(n,)).copy(),
                np.ctypeslib.as_array(fam, shape=(n,)).copy())

    def subtree(self, i: int):
        """Tree i after all five passes of -s (a decompose with F_SUBFLUBBLES): dict of n_total, n_flubble_like, n_concealed,
        n_midi, n_smothered, fam / or1 / or2 / route (uint8) and id1 / id2 (uint32) per vertex, child_off (uint32, relative) and
        child (uint32): children of vertex v = child[child_off[v]:child_off[v + 1]]."""
        st = _SubTree()
        rc = self._lib.povu_hip_forest_get_subtree(self._h, i, C.byref(st))
        if rc != 0:
            raise RuntimeError(f"forest carries no subflubble trees (rc {rc})")
        n = st.n_total
        a8 = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint8)
        a32 = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        off = np.ctypeslib.as_array(st.child_off, shape=(n + 1,)).copy()
        lo, hi = int(off[0]), int(off[-1])
        child = np.ctypeslib.as_array(st.child, shape=(max(hi, 1),))[lo:hi].copy()
        return dict(n_total=n, n_flubble_like=st.n_flubble_like, n_concealed=st.n_concealed, n_midi=st.n_midi,
                    n_smothered=st.n_smothered, fam=a8(st.fam), or1=a8(st.or1), or2=a8(st.or2), route=a8(st.route),
                    id1=a32(st.id1), id2=a32(st.id2), child_off=off - lo, child=child)

    def sites(self) -> "Sites":
        """The sites of this forest (povu_hip_forest_sites): every PVST vertex but the roots, the extended trees of -s when
        the forest carries them."""
        p = self._lib.povu_hip_forest_sites(self._h)
        if not p:
            raise RuntimeError("cannot build the sites of this forest")
        return Sites(self._lib, p)

    def raw(self):
        """Zero-copy view of the whole result: (uint8 block over the pinned host memory, total entries,
        byte offsets of a_id/z_id/parent/a_or/z_or, header int64 [n_trees, 3] = (component id, n_pvst, first))."""
        blk, nb, tot = C.c_void_p(), C.c_size_t(0), C.c_uint64(0)
        offs = (C.c_uint64 * 5)()
        if self._lib.povu_hip_forest_raw(self._h, C.byref(blk), C.byref(nb), C.byref(tot), offs) != 0:
            raise RuntimeError("forest has no raw block")
        n = len(self)
        hdr = np.zeros((n, 3), dtype=np.int64)
        t = _Tree()
        for i in range(n):
            self._lib.povu_hip_forest_get(self._h, i, C.byref(t))
            hdr[i] = (t.component_id, t.n_pvst, self._lib.povu_hip_forest_first(self._h, i))
        if nb.value == 0 or not blk.value:
            block = np.zeros(0, dtype=np.uint8)
        else:
            block = np.ctypeslib.as_array(C.cast(blk, C.POINTER(C.c_uint8)), shape=(nb.value,))
        return block, int(tot.value), [int(x) for x in offs], hdr

    def pack(self) -> np.ndarray:
        """The forest in its wire format (host bytes): what a transport other than RCCL ships."""
        n = self._lib.povu_hip_forest_pack_size(self._h)
        buf = np.zeros(n, dtype=np.uint8)
        if self._lib.povu_hip_forest_pack(self._h, buf.ctypes.data, n) != 0:
            raise RuntimeError("forest pack failed")
        return buf

    def share(self, rank: int) -> np.ndarray:
        """Descriptor (8 x uint64, word 7 = `rank`) of this forest's block in shared memory for the root of a multi-process
        job (povu_hip_forest_share; the context must have been put into shared-results mode)."""
        d = (C.c_uint64 * 8)()
        rc = self._lib.povu_hip_forest_share(self._h, d)
        if rc != 0:
            raise RuntimeError({2: "the forest's block is no shared segment: call HipDecomposer.share_results first",
                                4: "a MERGED forest with hairpin boundaries / subflubble labels cannot be shared: share its parts"}.get(rc, f"forest share failed ({rc})"))
        out = np.array(list(d), dtype=np.uint64)
        out[7] = rank
        return out

    def component_ids(self) -> List[int]:
        t = _Tree()
        out = []
        for i in range(len(self)):
            self._lib.povu_hip_forest_get(self._h, i, C.byref(t))
            out.append(int(t.component_id))
        return out

    def text(self, i: int) -> str:
        ln = C.c_size_t(0)
        p = self._lib.povu_hip_forest_pvst_text(self._h, i, C.byref(ln))
        if not p:
            raise IndexError(i)
        s = C.string_at(p, ln.value).decode()
        self._lib.povu_hip_buffer_free(p)
        return s

    def texts(self) -> Dict[int, str]:
        """{component_id: pvst text} -- what `povu decompose` writes as <id>.pvst."""
        out = {}
        for i in range(len(self)):
            t = _Tree()
            self._lib.povu_hip_forest_get(self._h, i, C.byref(t))
            out[t.component_id] = self.text(i)
        return out


def _view(p, n: int, dt):
    """numpy view of the n elements at C pointer p (an empty array when n is 0: p may then be null)."""
    return np.ctypeslib.as_array(p, shape=(n,)) if n else np.zeros(0, dt)


class _PerQuery:
    """Results of every query of a forest: queries are numbered in tree order, then PVST vertex order within the tree, each
    root skipped (first_query: query number of PVST vertex 1 of every tree, _query_firsts)."""

    def __init__(self, lib, ptr, forest: "Forest", first_query: List[int]):
        self._lib, self._p = lib, ptr
        self._first = first_query
        self._forest = forest

    def query(self, tree_index: int, pvst_vertex: int) -> int:
        """Query number of a PVST vertex (not the root)."""
        n = (self._first[tree_index + 1] if tree_index + 1 < len(self._first) else self.n_queries) - self._first[tree_index]
        if not 1 <= pvst_vertex <= n:
            raise IndexError((tree_index, pvst_vertex))
        return self._first[tree_index] + pvst_vertex - 1


class Walks(_PerQuery):
    """Walks of every query of a forest (HipDecomposer.walks): numpy views of the flat arrays of povu_hip_forest_walks --
    walk_off [n_queries + 1], step_off [n_walks + 1], step_id / step_or [n_steps], status [n_queries] -- valid as long as
    this object lives."""

    def __init__(self, lib, ptr, forest: "Forest", first_query: List[int]):
        super().__init__(lib, ptr, forest, first_query)
        w = ptr.contents
        self.n_queries, self.n_walks, self.n_steps = int(w.n_queries), int(w.n_walks), int(w.n_steps)
        self.n_tier2, self.device_ms = int(w.n_tier2), float(w.device_ms)
        self.walk_off = _view(w.walk_off, self.n_queries + 1, np.uint32)
        self.step_off = _view(w.step_off, self.n_walks + 1, np.uint32)
        self.step_id = _view(w.step_id, self.n_steps, np.uint32)
        self.step_or = _view(w.step_or, self.n_steps, np.uint8)
        self.status = _view(w.status, self.n_queries, np.uint8)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_walks_free(self._p)
            self._p = None

    def walks_of_query(self, q: int):
        out = []
        for w in range(int(self.walk_off[q]), int(self.walk_off[q + 1])):
            a, b = int(self.step_off[w]), int(self.step_off[w + 1])
            out.append([(int(i), ">" if o == 0 else "<") for i, o in zip(self.step_id[a:b].tolist(), self.step_or[a:b].tolist())])
        return out

    def of(self, tree_index: int, pvst_vertex: int):
        """([[(segment id, '>' | '<'), ...], ...], status bits) of PVST vertex `pvst_vertex` of tree `tree_index`."""
        q = self.query(tree_index, pvst_vertex)
        return self.walks_of_query(q), int(self.status[q])


def _query_firsts(lib, forest: "Forest") -> List[int]:
    """Query number of PVST vertex 1 of every tree (queries: tree order, then PVST vertex order, roots skipped)."""
    first, q = [], 0
    st = _SubTree()
    t = _Tree()
    for i in range(len(forest)):
        first.append(q)
        if lib.povu_hip_forest_get_subtree(forest._h, i, C.byref(st)) == 0:
            q += st.n_total - 1
        else:
            lib.povu_hip_forest_get(forest._h, i, C.byref(t))
            q += t.n_pvst - 1
    return first


class Traversals(_PerQuery):
    """Traversals of every query of a forest by the resident paths (HipDecomposer.traversals): numpy views of the flat
    arrays of povu_hip_forest_traversals -- trav_off / allele_off [n_queries + 1], status [n_queries], path / first / last /
    allele / reverse [n_traversals], step_off [n_alleles + 1], step_id / step_or [n_steps] -- valid as long as this object
    lives."""

    def __init__(self, lib, ptr, forest: "Forest", first_query: List[int]):
        super().__init__(lib, ptr, forest, first_query)
        t = ptr.contents
        self.n_queries, self.n_traversals = int(t.n_queries), int(t.n_traversals)
        self.n_alleles, self.n_steps = int(t.n_alleles), int(t.n_steps)
        self.n_tier2, self.n_hash_splits, self.device_ms = int(t.n_tier2), int(t.n_hash_splits), float(t.device_ms)
        self.trav_off = _view(t.trav_off, self.n_queries + 1, np.uint64)
        self.allele_off = _view(t.allele_off, self.n_queries + 1, np.uint64)
        self.status = _view(t.status, self.n_queries, np.uint8)
        self.path = _view(t.path, self.n_traversals, np.uint32)
        self.first = _view(t.first, self.n_traversals, np.uint32)
        self.last = _view(t.last, self.n_traversals, np.uint32)
        self.allele = _view(t.allele, self.n_traversals, np.uint32)
        self.reverse = _view(t.reverse, self.n_traversals, np.uint8)
        self.step_off = _view(t.step_off, self.n_alleles + 1, np.uint64)
        self.step_id = _view(t.step_id, self.n_steps, np.uint32)
        self.step_or = _view(t.step_or, self.n_steps, np.uint8)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_traversals_free(self._p)
            self._p = None

    def of_query(self, q: int):
        alleles = []
        for a in range(int(self.allele_off[q]), int(self.allele_off[q + 1])):
            b, e = int(self.step_off[a]), int(self.step_off[a + 1])
            alleles.append([(int(i), ">" if o == 0 else "<")
                            for i, o in zip(self.step_id[b:e].tolist(), self.step_or[b:e].tolist())])
        trav = []
        for t in range(int(self.trav_off[q]), int(self.trav_off[q + 1])):
            trav.append((int(self.path[t]), int(self.first[t]), int(self.last[t]), "-" if self.reverse[t] else "+",
                         int(self.allele[t])))
        return alleles, trav, int(self.status[q])

    def of(self, tree_index: int, pvst_vertex: int):
        """(alleles [[(segment id, '>' | '<'), ...], ...], traversals [(path, first, last, '+' | '-', allele), ...],
        status bits) of PVST vertex `pvst_vertex` of tree `tree_index`."""
        return self.of_query(self.query(tree_index, pvst_vertex))


class Shards:
    """Device-resident partition of a resident graph into per-rank packed shards (povu_hip_shard_partition)."""

    def __init__(self, lib, handle, owner):
        self._lib, self._h, self._owner = lib, handle, owner

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.povu_hip_shards_free(self._h)
            self._h = None

    @property
    def world(self) -> int:
        return self._lib.povu_hip_shards_world(self._h)

    @property
    def total_components(self) -> int:
        return self._lib.povu_hip_shards_total_components(self._h)

    def info(self, rank: int) -> dict:
        i = _ShardInfo()
        if self._lib.povu_hip_shards_get(self._h, rank, C.byref(i)) != 0:
            raise IndexError(rank)
        return dict(n_vtx=i.n_vtx, n_links=i.n_links, n_components=i.n_components, weight=int(i.weight), bytes=int(i.bytes),
                    device_ptr=i.device_ptr)

    def times(self) -> dict:
        t = (C.c_double * 3)()
        self._lib.povu_hip_shards_times(self._h, t)
        return dict(label_ms=t[0], lpt_ms=t[1], partition_ms=t[2])

    def export(self, rank: int) -> np.ndarray:
        """Packed shard `rank` as host bytes."""
        buf = np.zeros(self.info(rank)["bytes"], dtype=np.uint8)
        if self._lib.povu_hip_shards_export(self._h, self._owner._ctx, rank, buf.ctypes.data) != 0:
            raise RuntimeError("shard export failed")
        return buf


CALL_ANCHORED, CALL_TANGLED, CALL_INS, CALL_DEL = 1, 2, 4, 8
CALL_SUBR = 16  # an inversion record: query 0xFFFFFFFF, first / n_steps the inverted run of its reference path
CALL_COLLAPSED = 32  # nested: the site has fewer classes than exact alleles (TANGLED too)
CALL_RESCUED = 64  # `popped` profile: kept above max_level because its ancestors were popped
CALL_NORMALIZED = 128  # `left-normalized` profile: the record was changed (INTEGRATION.md "Left-normalised calls")
GT_MISSING = 0xFFFF


class Sites:
    """The sites of a forest (its queries; Forest.sites()): numpy views of the arrays of povu_hip_sites -- id1 / or1 / id2 / or2,
    parent (a query, 0xFFFFFFFF under the root), height, family (the line letter's byte), tree -- valid as long as this
    object lives."""

    def __init__(self, lib, ptr):
        self._lib, self._p = lib, ptr
        s = ptr.contents
        self.n = int(s.n)
        for k, dt in (("id1", np.uint32), ("id2", np.uint32), ("or1", np.uint8), ("or2", np.uint8), ("parent", np.uint32),
                      ("height", np.uint32), ("family", np.uint8), ("tree", np.uint32)):
            setattr(self, k, _view(getattr(s, k), self.n, dt))

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_sites_free(self._p)
            self._p = None


class Calls:
    """Variant calls (HipDecomposer.call): numpy views of the flat arrays of povu_hip_call, valid as long as this object
    lives, and vcf_text().  It keeps the names record (povu_hip_call_names) and the sites it was made from alive."""

    def __init__(self, lib, ptr, names, names_rec, name_array, sites, profile="raw-graph"):
        self._lib, self._p = lib, ptr
        self.profile = profile
        self._names_rec, self._name_array, self._sites = names_rec, name_array, sites
        c, nr = ptr.contents, names_rec.contents
        self.names = names
        self.refs = [int(nr.refs.ref_path[k]) for k in range(nr.refs.n_refs)]
        self.samples = [nr.sample[k].decode() for k in range(nr.refs.n_samples)]
        self.n_records, self.n_slots = int(c.n_records), int(c.n_slots)
        self.device_ms = float(c.device_ms)
        self.n_seq_bytes, self.n_at_bytes = int(c.n_seq_bytes), int(c.n_at_bytes)
        n, nb, nsp = self.n_records, int(c.n_blocks), int(c.n_spelled)
        for k in ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "block"):
            setattr(self, k, _view(getattr(c, k), n, np.uint32))
        self.pos = _view(c.pos, n, np.uint64)
        self.flags = _view(c.flags, n, np.uint8)
        self.ac_off = _view(c.ac_off, n + 1, np.uint64)
        self.ac = _view(c.ac, int(self.ac_off[-1]) if n else 0, np.uint32)
        self.gt = _view(c.gt, n * self.n_slots, np.uint16).reshape(n, self.n_slots)
        self.block_off = _view(c.block_off, nb + 1, np.uint64)
        self.seq_off = _view(c.seq_off, nsp + 1, np.uint64)
        self.at_off = _view(c.at_off, nsp + 1, np.uint64)
        self.seq = _view(c.seq, self.n_seq_bytes, np.uint8)
        self.at = _view(c.at, self.n_at_bytes, np.uint8)
        self.contig_len = _view(c.contig_len, len(self.refs), np.uint64)
        self.n_steps = _view(c.n_steps, n, np.uint32)
        self.n_inv_records, self.n_inv_heads = int(c.n_inv_records), int(c.n_inv_heads)
        self.n_inv_long, self.n_inv_tier2 = int(c.n_inv_long), int(c.n_inv_tier2)
        # "Nested calls": LV, the enclosing record's site (0xFFFFFFFF: none), REF among the spelled alleles; the counters
        self.level = _view(c.level, n, np.uint32)
        self.parent_query = _view(c.parent_query, n, np.uint32)
        self.ref_spelled = _view(c.ref_spelled, n, np.uint64)
        self.nested = bool(c.nested)
        self.n_enclosed, self.n_collapsed_sites = int(c.n_enclosed), int(c.n_collapsed_sites)
        self.n_popped, self.n_rescued = int(c.n_popped), int(c.n_rescued)
        # "Left-normalised calls": POS before the normalisation, the block of the normalised alleles (0xFFFFFFFF: unchanged),
        # shift s, chop r and trim u; the counters
        self.raw_pos = _view(c.raw_pos, n, np.uint64)
        for k in ("norm_block", "norm_shift", "norm_chop", "norm_trim"):
            setattr(self, k, _view(getattr(c, k), n, np.uint32))
        self.n_normalized, self.max_shift = int(c.n_normalized), int(c.max_shift)
        self.n_norm_compared = int(c.n_norm_compared)
        # "Decomposed calls": the rows (none outside the profile) and the counters
        m = self.n_rows = int(c.n_rows)
        for k in ("row_record", "row_alt", "row_index", "row_ref_start", "row_ref_len", "row_alt_start", "row_alt_len", "row_ac",
                  "row_an", "row_ns"):
            setattr(self, k, _view(getattr(c, k), m, np.uint32))
        for k in ("row_kind", "row_reason", "row_lead"):
            setattr(self, k, _view(getattr(c, k), m, np.uint8))
        self.row_pos = _view(c.row_pos, m, np.uint64)
        self.n_decomposed_alts, self.n_passthrough_alts = int(c.n_decomposed_alts), int(c.n_passthrough_alts)
        self.n_prim_tier2, self.n_prim_cells = int(c.n_prim_tier2), int(c.n_prim_cells)
        # "Merged primitives" (T_MERGE): the groups of equal rows (none without the flag), their joint genotypes (0, 1, 0xFF for
        # '.') and counts; the counters
        self.merged = bool(c.merged)
        g = self.n_mrows = int(c.n_mrows)
        self.mrow_off = _view(c.mrow_off, g + 1 if self.merged else 0, np.uint64)
        self.mrow_member = _view(c.mrow_member, m if self.merged else 0, np.uint32)
        self.mrow_gt = _view(c.mrow_gt, g * self.n_slots, np.uint8).reshape(g, self.n_slots)
        for k in ("mrow_ac", "mrow_an", "mrow_ns"):
            setattr(self, k, _view(getattr(c, k), g, np.uint32))
        for k in MERGE_COUNTERS:
            setattr(self, k, int(getattr(c, k)))
        # "Off-reference calls" (T_OFFREF): per record whether it is one, its host's site and allele (0xFFFFFFFF: none); the
        # surrogate paths that are no reference path, with their lengths; the counters.  Without the flag: empty, 0
        self.offref = bool(c.offref)
        k = n if self.offref else 0
        self.rec_offref = _view(c.rec_offref, k, np.uint8)
        self.host_query = _view(c.host_query, k, np.uint32)
        self.host_allele = _view(c.host_allele, k, np.uint32)
        self.off_contig_path = _view(c.off_contig_path, int(c.n_off_contigs), np.uint32)
        self.off_contig_len = _view(c.off_contig_len, int(c.n_off_contigs), np.uint64)
        for k in OFFREF_COUNTERS:
            setattr(self, k, int(getattr(c, k)))
        # "Untangled calls" (T_UNTANGLE): per record whether it is untangled, the reference's lap it is (from 1) and the
        # reference's laps; per (record, slot) the laps of the slot's paths; the counters.  Without the flag: empty, 0
        self.untangled = bool(c.untangled)
        k = n if self.untangled else 0
        self.rec_unt = _view(c.rec_unt, k, np.uint8)
        self.lap = _view(c.lap, k, np.uint32)
        self.n_laps = _view(c.n_laps, k, np.uint32)
        self.lap_count = _view(c.lap_count, k * self.n_slots, np.uint16).reshape(k, self.n_slots)
        for k in UNTANGLE_COUNTERS:
            setattr(self, k, int(getattr(c, k)))
        # "Region calls" (regions=...): the intervals after normalisation, the sites that pass, the sites whose scans were masked,
        # the flubble records the late filter dropped.  Without regions: 0
        for k in REGION_COUNTERS:
            setattr(self, k, int(getattr(c, k)))
        # "Clustered calls" (cluster=...): the threshold in ppm (0: not clustered); per record whether its site lost alleles and
        # the site's lowest similarity; per written allele of record r the exact alleles behind it, at ac_off[r] + r + i; the
        # counters.  Without a threshold: empty, 0
        self.cluster_ppm = int(c.cluster_ppm)
        k = n if self.cluster_ppm else 0
        self.rec_clustered = _view(c.rec_clustered, k, np.uint8)
        self.cl_minsim = _view(c.cl_minsim, k, np.uint32)
        self.cl_nx = _view(c.cl_nx, int(self.ac_off[-1]) + n if k else 0, np.uint32)
        for k in CLUSTER_COUNTERS:
            setattr(self, k, int(getattr(c, k)))
        # "Spanning alleles" (T_SPANNING): per record whether its last ALT is `*` (n_alleles counts it, the spanned entries of
        # gt carry n_alleles - 1); the records with one and the spanned entries.  Without the flag: empty, 0
        self.spanning = bool(c.spanning)
        self.rec_star = _view(c.rec_star, n if self.spanning else 0, np.uint8)
        for k in SPAN_COUNTERS:
            setattr(self, k, int(getattr(c, k)))

    def nx(self, i):
        """The exact alleles behind every written allele of record i of a clustered call, REF's cluster first."""
        at = int(self.ac_off[i]) + i
        return self.cl_nx[at:at + int(self.n_alleles[i])].tolist()

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_calls_free(self._p)
            self._p = None
        if getattr(self, "_names_rec", None):
            self._lib.povu_hip_call_names_free(self._names_rec)
            self._names_rec = None

    def vcf_text(self, date=None, only=None, threads: int = 1, profile=None) -> str:
        """One VCF of every reference path (povu_hip_calls_vcf_profile): header (fileDate today unless given), contig lines,
        records; with `only` those of the reference paths whose name starts with it.  profile: the one the call was made
        under unless given."""
        ln = C.c_size_t(0)
        p = self._lib.povu_hip_calls_vcf_profile(self._p, self._sites._p, self._names_rec, self._name_array,
                                                 None if date is None else str(date).encode(),
                                                 None if only is None else only.encode(), threads,
                                                 PROFILES[self.profile if profile is None else profile], C.byref(ln))
        if not p:
            raise RuntimeError("the calls, sites and names do not belong together")
        s = C.string_at(p, ln.value).decode()
        self._lib.povu_hip_buffer_free(p)
        return s

    def vcf_rest_text(self, prefixes, date=None, threads: int = 1) -> str:
        """The VCF of the records whose CHROM starts with none of `prefixes` (povu_hip_calls_vcf_rest): the off-reference.vcf of
        `povu call -o DIR --off-reference`."""
        ln = C.c_size_t(0)
        arr = (C.c_char_p * max(1, len(prefixes)))(*[x.encode() for x in prefixes])
        p = self._lib.povu_hip_calls_vcf_rest(self._p, self._sites._p, self._names_rec, self._name_array,
                                              None if date is None else str(date).encode(), arr, len(prefixes), threads,
                                              PROFILES[self.profile], C.byref(ln))
        if not p:
            raise RuntimeError("the calls, sites and names do not belong together")
        s = C.string_at(p, ln.value).decode()
        self._lib.povu_hip_buffer_free(p)
        return s


class VcfDoc:
    """A parsed VCF (parse_vcf; povu_hip_vcf_parse): numpy views of the arrays of povu_hip_vcf_doc, valid as long as this object
    lives -- samples (the column names), rec_line / rec_pos / rec_id per record, allele_off / task_off (per record), step_off /
    text_off / allele_walk (per allele; bit 0: AT holds a walk, bit 1: it has a text), step_id / step_or, text (bytes),
    task_record / task_allele / task_col / task_phase; chroms (the distinct CHROM strings in order of first appearance) and
    rec_chrom (per record, an index into them)."""

    def __init__(self, lib, ptr):
        self._lib, self._p = lib, ptr
        d = ptr.contents
        self.n_records, self.n_alleles, self.n_tasks = int(d.n_records), int(d.n_alleles), int(d.n_tasks)
        self.n_steps = int(d.n_steps)
        self.samples = [d.sample[k].decode() for k in range(d.n_samples)]
        n, na, nk = self.n_records, self.n_alleles, self.n_tasks
        self.rec_line, self.rec_pos = _view(d.rec_line, n, np.uint64), _view(d.rec_pos, n, np.uint64)
        self.rec_id_off = _view(d.rec_id_off, n + 1, np.uint64)
        ids = bytes(_view(d.ids, int(d.n_id_bytes), np.uint8))
        self.rec_id = [ids[int(self.rec_id_off[r]):int(self.rec_id_off[r + 1])].decode() for r in range(n)]
        self.allele_off, self.task_off = _view(d.allele_off, n + 1, np.uint64), _view(d.task_off, n + 1, np.uint64)
        self.step_off, self.text_off = _view(d.step_off, na + 1, np.uint64), _view(d.text_off, na + 1, np.uint64)
        self.allele_walk = _view(d.allele_walk, na, np.uint8)
        self.step_id, self.step_or = _view(d.step_id, self.n_steps, np.uint32), _view(d.step_or, self.n_steps, np.uint8)
        self.text = _view(d.text, int(d.n_text_bytes), np.uint8)
        for k in ("task_record", "task_allele", "task_col", "task_phase"):
            setattr(self, k, _view(getattr(d, k), nk, np.uint32))
        self.chroms = [d.chrom[k].decode() for k in range(d.n_chroms)]
        self.rec_chrom = _view(d.rec_chrom, n, np.uint32)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_vcf_doc_free(self._p)
            self._p = None


def parse_vcf(text, threads: int = 1) -> VcfDoc:
    """The records, alleles, walks and tasks of VCF text (INTEGRATION.md "VCF checks"; host only).  A malformed line is refused
    with its line number."""
    lib = load_lib()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    err = C.create_string_buffer(512)
    p = lib.povu_hip_vcf_parse(raw, len(raw), threads, err, 512)
    if not p:
        raise RuntimeError(err.value.decode())
    return VcfDoc(lib, p)


def _vcf_texts(lib, report_p, doc_p, names_p):
    """(report.tsv, summary.txt) of povu_hip_vcf_report_text."""
    ln, sl, sp = C.c_size_t(0), C.c_size_t(0), C.c_void_p(None)
    p = lib.povu_hip_vcf_report_text(report_p, doc_p, names_p, C.byref(ln), C.byref(sp), C.byref(sl))
    if not p:
        raise RuntimeError("the report, the document and the names do not belong together")
    out = C.string_at(p, ln.value).decode(), C.string_at(sp.value, sl.value).decode()
    lib.povu_hip_buffer_free(p)
    lib.povu_hip_buffer_free(sp)
    return out


class VcfReport:
    """What HipDecomposer.check_vcf found (povu_hip_vcf_report): numpy views, valid as long as this object lives -- task_status
    (V_FOUND_FWD .. V_NO_SLOT), allele_spell (V_SPELL_*), rec_invalid, and per invalid record its first failure: rec_reason (a
    status or V_MISSPELLED; 0xFF when valid), rec_allele (within the record), rec_task (0xFFFFFFFF for a misspelled allele); the
    counters n_records, n_tasks, n_status (per status), n_invalid, n_misspelled, n_tier2; device_ms.  `doc` is the parsed VCF."""

    def __init__(self, lib, ptr, doc: VcfDoc, names_rec):
        self._lib, self._p, self.doc, self._names_rec = lib, ptr, doc, names_rec
        r = ptr.contents
        self.n_records, self.n_tasks, self.n_alleles = int(r.n_records), int(r.n_tasks), int(r.n_alleles)
        self.task_status = _view(r.task_status, self.n_tasks, np.uint8)
        self.allele_spell = _view(r.allele_spell, self.n_alleles, np.uint8)
        for k in ("rec_invalid", "rec_reason"):
            setattr(self, k, _view(getattr(r, k), self.n_records, np.uint8))
        for k in ("rec_allele", "rec_task"):
            setattr(self, k, _view(getattr(r, k), self.n_records, np.uint32))
        self.n_status = [int(x) for x in r.n_status]
        self.n_invalid, self.n_misspelled, self.n_tier2 = int(r.n_invalid), int(r.n_misspelled), int(r.n_tier2)
        self.device_ms = float(r.device_ms)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_vcf_report_free(self._p)
            self._p = None
        if getattr(self, "_names_rec", None):
            self._lib.povu_hip_call_names_free(self._names_rec)
            self._names_rec = None

    def report_text(self) -> str:
        """report.tsv of `povu vcf --report`: a line per invalid record, for its first failure."""
        return _vcf_texts(self._lib, self._p, self.doc._p, self._names_rec)[0]

    def summary_text(self) -> str:
        """summary.txt: `No errors`, or the rate of invalid records."""
        return _vcf_texts(self._lib, self._p, self.doc._p, self._names_rec)[1]


class VcfComparison:
    """What HipDecomposer.compare_vcfs found (povu_hip_vcf_cmp): numpy views, valid as long as this object lives.  Per side
    (`_a`, `_b`) and item, in document order: item_record, item_alt (from 1), item_state (M_KEYED, M_SKIPPED), item_pos (POS'),
    item_suffix / item_prefix (the bytes the trims took), item_group (0xFFFFFFFF for a skipped item).  Per group, in the order of
    their first items: group_class (M_SHARED, M_ONLY_A, M_ONLY_B), group_n_a / group_n_b, group_first (an item of A, or n_items_a +
    an item of B).  Per common sample: sample_col_a / sample_col_b, sample_tp / _fp / _fn / _gteq.  The counters n_items_a,
    n_items_b, n_groups, n_common_samples and VCF_CMP_COUNTERS; device_ms.  `doc_a` and `doc_b` are the parsed VCFs."""

    def __init__(self, lib, ptr, doc_a: VcfDoc, doc_b: VcfDoc):
        self._lib, self._p, self.doc_a, self.doc_b = lib, ptr, doc_a, doc_b
        c = ptr.contents
        for k in ("n_items_a", "n_items_b", "n_groups", "n_common_samples") + VCF_CMP_COUNTERS:
            setattr(self, k, int(getattr(c, k)))
        for side, n in (("a", self.n_items_a), ("b", self.n_items_b)):
            for k, dt in (("item_record", np.uint32), ("item_alt", np.uint32), ("item_state", np.uint8), ("item_pos", np.uint64),
                          ("item_suffix", np.uint32), ("item_prefix", np.uint32), ("item_group", np.uint32)):
                setattr(self, f"{k}_{side}", _view(getattr(c, f"{k}_{side}"), n, dt))
        self.group_class = _view(c.group_class, self.n_groups, np.uint8)
        for k in ("group_n_a", "group_n_b", "group_first"):
            setattr(self, k, _view(getattr(c, k), self.n_groups, np.uint32))
        for k in ("sample_col_a", "sample_col_b"):
            setattr(self, k, _view(getattr(c, k), self.n_common_samples, np.uint32))
        for k in ("sample_tp", "sample_fp", "sample_fn", "sample_gteq"):
            setattr(self, k, _view(getattr(c, k), self.n_common_samples, np.uint64))
        self.device_ms = float(c.device_ms)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_vcf_cmp_free(self._p)
            self._p = None

    def _texts(self):
        ln, sl, sp = C.c_size_t(0), C.c_size_t(0), C.c_void_p(None)
        p = self._lib.povu_hip_vcf_cmp_text(self._p, self.doc_a._p, self.doc_b._p, C.byref(ln), C.byref(sp), C.byref(sl))
        if not p:
            raise RuntimeError("the comparison and the documents do not belong together")
        out = C.string_at(p, ln.value).decode(), C.string_at(sp.value, sl.value).decode()
        self._lib.povu_hip_buffer_free(p)
        self._lib.povu_hip_buffer_free(sp)
        return out

    def compare_text(self) -> str:
        """compare.tsv of `povu vcf --compare`: a line per group that only one side has, in group order."""
        return self._texts()[0]

    def summary_text(self) -> str:
        """summary.txt: the groups of every class, the cells of every class, their rates, a line per common sample."""
        return self._texts()[1]


class HapComparison:
    """What HipDecomposer.compare_haplotypes found (povu_hip_vcf_hap): numpy views, valid as long as this object lives.  Per side
    (`_a`, `_b`) and record: rec_placed, rec_window (0xFFFFFFFF when unplaced).  Per side and item, in document order:
    item_record, item_alt (from 1), item_state (H_EDIT, H_UNSPELLED, H_UNPLACED), item_s / item_e (0-based, half-open),
    item_suffix / item_prefix (the bytes the trims took), item_left / item_right (the reaches), item_group.  Per window:
    win_chrom (an index into `chroms`), win_lo / win_hi, win_n_a / win_n_b, win_inconsistent, win_offender.  Per cell, in
    (window, sample, phase) order: cell_window, cell_sample, cell_phase, cell_status (H_INCONSISTENT .. H_DIFFER),
    cell_edits_a / _b, cell_len_a / _b, cell_first_diff.  Per common sample: sample_col_a / sample_col_b and sample_status
    ([n_common_samples, 10]).  n_status (per status), the counters VCF_HAP_COUNTERS, reference, device_ms.  `doc_a` and `doc_b`
    are the parsed VCFs."""

    def __init__(self, lib, ptr, doc_a: VcfDoc, doc_b: VcfDoc):
        self._lib, self._p, self.doc_a, self.doc_b = lib, ptr, doc_a, doc_b
        h = ptr.contents
        for k in ("n_records_a", "n_records_b", "n_items_a", "n_items_b", "n_groups", "n_windows", "n_cells", "n_common_samples") + VCF_HAP_COUNTERS:
            setattr(self, k, int(getattr(h, k)))
        for side, nr, ni in (("a", self.n_records_a, self.n_items_a), ("b", self.n_records_b, self.n_items_b)):
            setattr(self, f"rec_placed_{side}", _view(getattr(h, f"rec_placed_{side}"), nr, np.uint8))
            setattr(self, f"rec_window_{side}", _view(getattr(h, f"rec_window_{side}"), nr, np.uint32))
            for k, t in _HAP_ITEM_ARRAYS:
                setattr(self, f"{k}_{side}", _view(getattr(h, f"{k}_{side}"), ni, np.dtype(t)))
        for k, t in _HAP_WIN_ARRAYS:
            setattr(self, k, _view(getattr(h, k), self.n_windows, np.dtype(t)))
        for k, t in _HAP_CELL_ARRAYS:
            setattr(self, k, _view(getattr(h, k), self.n_cells, np.dtype(t)))
        for k in ("sample_col_a", "sample_col_b"):
            setattr(self, k, _view(getattr(h, k), self.n_common_samples, np.uint32))
        self.sample_status = _view(h.sample_status, self.n_common_samples * 10, np.uint64).reshape(self.n_common_samples, 10)
        self.n_status = [int(x) for x in h.n_status]
        self.reference, self.device_ms = bool(h.reference), float(h.device_ms)
        self.chroms = list(doc_a.chroms) + [c for c in doc_b.chroms if c not in doc_a.chroms]

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_vcf_hap_free(self._p)
            self._p = None

    def _texts(self):
        ln, sl, sp = C.c_size_t(0), C.c_size_t(0), C.c_void_p(None)
        p = self._lib.povu_hip_vcf_hap_text(self._p, self.doc_a._p, self.doc_b._p, C.byref(ln), C.byref(sp), C.byref(sl))
        if not p:
            raise RuntimeError("the haplotype comparison and the documents do not belong together")
        out = C.string_at(p, ln.value).decode(), C.string_at(sp.value, sl.value).decode()
        self._lib.povu_hip_buffer_free(p)
        self._lib.povu_hip_buffer_free(sp)
        return out

    def haplotypes_text(self) -> str:
        """haplotypes.tsv of `povu vcf --compare --haplotypes`: a line per cell that is neither equal_ref nor equal."""
        return self._texts()[0]

    def summary_text(self) -> str:
        """hap_summary.txt: the windows, the cells of every status, both concordances, a line per common sample."""
        return self._texts()[1]


def cons_texts(lib, cons_p, doc_p, names, width: int = 60):
    """(consensus.fa, roundtrip.tsv, cons_summary.txt) of povu_hip_vcf_cons_text for a result (which may be hand-made), a parsed
    document and the path names."""
    name_array = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    err = C.create_string_buffer(512)
    nr = lib.povu_hip_vcf_names_make(len(names), name_array, err, 512)
    if not nr:
        raise RuntimeError(err.value.decode())
    try:
        fl, rl, sl, rp, sp = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_void_p(None), C.c_void_p(None)
        p = lib.povu_hip_vcf_cons_text(cons_p, doc_p, nr, name_array, width, C.byref(fl), C.byref(rp), C.byref(rl), C.byref(sp), C.byref(sl))
        if not p:
            raise RuntimeError("the consensus, the document and the names do not belong together")
        out = C.string_at(p, fl.value).decode(), C.string_at(rp.value, rl.value).decode(), C.string_at(sp.value, sl.value).decode()
        for b in (p, rp, sp):
            lib.povu_hip_buffer_free(b)
        return out
    finally:
        lib.povu_hip_call_names_free(nr)


class Consensus:
    """What HipDecomposer.consensus made (povu_hip_vcf_cons): numpy views, valid as long as this object lives.  Per haplotype,
    in (CHROM id, column, phase) order: hap_chrom (an index into doc.chroms), hap_col, hap_phase, hap_len, hap_off (into
    `text`), n_applied / n_duplicate / n_enclosed / n_overlap / n_unspelled / n_nocall, rt_status (C_RT_*), rt_path (0xFFFFFFFF:
    none), rt_path_len, rt_first_diff.  text (bytes; None under text=False), n_haps, n_text_bytes, n_unplaced, n_tier2,
    roundtrip, device_ms, write_ms (the materialiser alone, under time_write).  `doc` is the parsed VCF."""

    def __init__(self, lib, ptr, doc: VcfDoc, names):
        self._lib, self._p, self.doc, self._names = lib, ptr, doc, list(names)
        c = ptr.contents
        for k in ("n_haps", "n_text_bytes", "n_unplaced", "n_tier2"):
            setattr(self, k, int(getattr(c, k)))
        for k, t in _CONS_ARRAYS:
            setattr(self, k, _view(getattr(c, k), self.n_haps, np.dtype(t)))
        self.text = _view(c.text, self.n_text_bytes, np.uint8) if c.text else None
        self.roundtrip, self.device_ms, self.write_ms = bool(c.roundtrip), float(c.device_ms), float(c.write_ms)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.povu_hip_vcf_cons_free(self._p)
            self._p = None

    def sequence(self, i: int) -> str:
        """The text of haplotype i."""
        if self.text is None:
            raise RuntimeError("the consensus was made without its text (text=False)")
        at, n = int(self.hap_off[i]), int(self.hap_len[i])
        return bytes(self.text[at:at + n]).decode()

    def fasta_text(self, width: int = 60) -> str:
        """consensus.fa of `povu vcf --consensus`: `>{sample}#{hap}#{CHROM}` and the text in lines of `width` bytes (0: one)."""
        return cons_texts(self._lib, self._p, self.doc._p, self._names, width)[0]

    def roundtrip_text(self) -> str:
        """roundtrip.tsv: a line per haplotype whose round trip is not `equal`."""
        return cons_texts(self._lib, self._p, self.doc._p, self._names)[1]

    def summary_text(self) -> str:
        """cons_summary.txt: the haplotypes of every round-trip status, the edits of every kind."""
        return cons_texts(self._lib, self._p, self.doc._p, self._names)[2]


class HipDecomposer:
    """One context = one GPU, one stream, one workspace arena."""

    def __init__(self, device: int = 0):
        self._lib = load_lib()
        if self._lib.povu_hip_device_count() <= 0:
            raise HipUnavailable("no HIP device visible: the decompose path has no CPU fallback")
        err = C.create_string_buffer(512)
        self._ctx = self._lib.povu_hip_create(device, err, 512)
        if not self._ctx:
            raise HipUnavailable(err.value.decode())
        self._keep = None

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.povu_hip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    def release_workspace(self) -> None:
        """Gives every workspace arena back to the device (povu_hip_release_workspace); the resident graph, paths, sequences, a
        received shard and the packed shards stay, and the next call allocates what it needs again."""
        if self._lib.povu_hip_release_workspace(self._ctx) != 0:
            raise RuntimeError("no context")

    def arenas(self) -> List[dict]:
        """Every device arena of the context in declaration order: its name, whether release_workspace keeps it, the bytes it
        holds now (povu_hip_arena_report)."""
        n = self._lib.povu_hip_arena_report(self._ctx, None, 0)
        buf = (_ArenaInfo * n)()
        n = self._lib.povu_hip_arena_report(self._ctx, buf, n)
        return [dict(name=buf[i].name.decode(), resident=buf[i].resident, bytes=buf[i].bytes) for i in range(n)]

    def upload(self, links, tips=None):
        """links: povu_amd.workloads.Links (vertex idx based link arrays)."""
        vid = np.ascontiguousarray(links.vid, dtype=np.uint32)
        v1 = np.ascontiguousarray(links.v1, dtype=np.uint32)
        v2 = np.ascontiguousarray(links.v2, dtype=np.uint32)
        s1 = np.ascontiguousarray(links.s1, dtype=np.uint8)
        s2 = np.ascontiguousarray(links.s2, dtype=np.uint8)
        tp = None
        if tips is not None:
            tips = np.ascontiguousarray(tips, dtype=np.uint8)
            tp = tips.ctypes.data
        err = C.create_string_buffer(512)
        rc = self._lib.povu_hip_graph_upload(self._ctx, len(vid), vid.ctypes.data, len(v1), v1.ctypes.data,
                                             s1.ctypes.data, v2.ctypes.data, s2.ctypes.data, tp, err, 512)
        if rc != 0:
            raise RuntimeError(err.value.decode())

    def prewarm(self, n_vtx: int, n_links: int) -> None:
        """Reserve the device memory a graph of this size will need (povu_hip_prewarm; only on a context that holds nothing)."""
        err = C.create_string_buffer(512)
        if self._lib.povu_hip_prewarm(self._ctx, n_vtx, n_links, err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def upload_times(self) -> dict:
        """Device time of the last upload (HIP events, ms): host-to-device copies, CSR build, reverse-slot table."""
        t = (C.c_double * 3)()
        if self._lib.povu_hip_last_upload_times(self._ctx, t) != 0:
            raise RuntimeError("no graph resident")
        return dict(h2d_ms=t[0], csr_ms=t[1], twin_ms=t[2])

    # ---- multi-GPU sharding
    def partition(self, world: int) -> Shards:
        """Labels the resident graph's components, bin-packs them over `world` ranks and partitions the links on the
        device (povu_hip_shard_partition)."""
        err = C.create_string_buffer(512)
        h = self._lib.povu_hip_shard_partition(self._ctx, world, err, 512)
        if not h:
            raise RuntimeError(err.value.decode())
        return Shards(self._lib, h, self)

    def upload_shard(self, packed, nbytes: Optional[int] = None, on_device: bool = False):
        """Makes a packed shard the resident graph: host bytes (numpy uint8) or a device pointer (int) + size."""
        err = C.create_string_buffer(512)
        if on_device:
            ptr, n = int(packed), int(nbytes)
        else:
            packed = np.ascontiguousarray(packed, dtype=np.uint8)
            ptr, n = packed.ctypes.data, packed.size
        if self._lib.povu_hip_graph_upload_shard(self._ctx, ptr, n, 1 if on_device else 0, err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def share_results(self, tag: str) -> None:
        """From now on the PVST blocks of this context's forests are shared-memory segments "/povu.<tag>.<k>" (the
        multi-process convention: tag = "<job>.<rank>"), see povu_hip_share_results."""
        err = C.create_string_buffer(512)
        if self._lib.povu_hip_share_results(self._ctx, tag.encode(), err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def attach_forests(self, own: Optional["Forest"], own_rank: int, job_tag: str, descs) -> "Forest":
        """Root of a multi-process job: the merged forest of every rank's descriptor (Forest.share) and of its own forest,
        which it takes over.  No PVST array is copied: the other ranks' blocks are mapped where their GPUs put them."""
        d = np.ascontiguousarray(np.asarray(descs, dtype=np.uint64).reshape(-1, 8))
        err = C.create_string_buffer(512)
        h = self._lib.povu_hip_forest_attach(self._ctx, own._h if own is not None else None, own_rank, job_tag.encode(),
                                             d.ctypes.data, d.shape[0], err, 512)
        if not h:
            raise RuntimeError(err.value.decode())
        return Forest(self._lib, h)

    def transfer_bytes(self) -> dict:
        """Bytes this context moved since it was created: over PCIe in either direction, to and from other GPUs."""
        b = (C.c_uint64 * 4)()
        self._lib.povu_hip_transfer_bytes(self._ctx, b)
        return dict(h2d=int(b[0]), d2h=int(b[1]), peer_out=int(b[2]), peer_in=int(b[3]))

    def shard_total_components(self) -> int:
        return int(self._lib.povu_hip_shard_total_components(self._ctx))

    def merge_forests(self, packed_list) -> Forest:
        """Merges packed forests (Forest.pack() bytes) into one forest ordered by component id."""
        bufs = [np.ascontiguousarray(b, dtype=np.uint8) for b in packed_list]
        n = len(bufs)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        err = C.create_string_buffer(512)
        h = self._lib.povu_hip_forest_merge(self._ctx, ptrs, sizes, n, err, 512)
        if not h:
            raise RuntimeError(err.value.decode())
        return Forest(self._lib, h)

    def decompose_shard(self, flags: int = 0) -> Forest:
        """Decomposes the resident shard and rewrites the component ids to those of the whole graph; a rank that
        owns no component gets an empty forest."""
        if self.shard_total_components() == 0:
            raise RuntimeError("the resident graph is not a shard")
        err = C.create_string_buffer(512)
        o = _Opts(0, 1, flags)
        h = self._lib.povu_hip_decompose(self._ctx, C.byref(o), err, 512)
        if not h:
            raise RuntimeError(err.value.decode())
        f = Forest(self._lib, h)
        if self._lib.povu_hip_forest_globalize(h, self._ctx) != 0:
            raise RuntimeError("forest globalize failed")
        return f

    def decompose(self, rank: int = 0, world: int = 1, flags: int = 0) -> Forest:
        o = _Opts(rank, world, flags)
        err = C.create_string_buffer(512)
        h = self._lib.povu_hip_decompose(self._ctx, C.byref(o), err, 512)
        if not h:
            raise RuntimeError(err.value.decode())
        return Forest(self._lib, h)

    def walks(self, forest: Forest, max_walks: int = 64, max_steps: int = 1000, max_expansions: int = 65536,
              flags: int = 0) -> Walks:
        """The walks of every flubble of `forest` (a decompose of the graph now resident here), on the GPU."""
        for k, v in (("max_walks", max_walks), ("max_steps", max_steps), ("max_expansions", max_expansions)):
            if not 1 <= int(v) < 2 ** 32:
                raise ValueError(f"{k} must be in [1, 2^32)")
        o = _WalkOpts(max_walks, max_steps, max_expansions, flags)
        err = C.create_string_buffer(512)
        p = self._lib.povu_hip_forest_walks(self._ctx, forest._h, C.byref(o), err, 512)
        if not p:
            raise RuntimeError(err.value.decode())
        return Walks(self._lib, p, forest, _query_firsts(self._lib, forest))

    def upload_paths(self, paths) -> None:
        """Makes the paths of the graph now uploaded resident (povu_hip_paths_upload): a workloads.Paths record, or a
        list of step lists [(segment id, 0 '>' | 1 '<'), ...].  The next upload drops them."""
        self._path_names = list(paths.names) if hasattr(paths, "names") else [f"path{k}" for k in range(len(paths))]
        if hasattr(paths, "off"):
            off = np.ascontiguousarray(paths.off, dtype=np.uint64)
            ids = np.ascontiguousarray(paths.ids, dtype=np.uint32)
            rev = np.ascontiguousarray(paths.rev, dtype=np.uint8)
        else:
            lens = [len(p) for p in paths]
            off = np.zeros(len(lens) + 1, np.uint64)
            off[1:] = np.cumsum(lens, dtype=np.uint64)
            flat = [s for p in paths for s in p]
            ids = np.array([a for a, _ in flat], dtype=np.uint32)
            rev = np.array([b for _, b in flat], dtype=np.uint8)
        err = C.create_string_buffer(512)
        if self._lib.povu_hip_paths_upload(self._ctx, len(off) - 1, off.ctypes.data, ids.ctypes.data if ids.size else None,
                                           rev.ctypes.data if rev.size else None, err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def upload_sequences(self, seqs) -> None:
        """Makes the sequences of the graph now uploaded resident (povu_hip_segments_upload): {segment id: str} or a list
        indexed by vertex (ascending segment id).  The next upload drops them."""
        if isinstance(seqs, dict):
            seqs = [seqs[k] for k in sorted(seqs)]
        raw = [x.encode() if isinstance(x, str) else bytes(x) for x in seqs]
        if any(r == b"*" for r in raw):
            raise RuntimeError("a segment has no sequence ('*'): variant calls need every sequence")
        off = np.zeros(len(raw) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
        blob = np.frombuffer(b"".join(raw) + b"\0", np.uint8)
        err = C.create_string_buffer(512)
        if self._lib.povu_hip_segments_upload(self._ctx, len(raw), off.ctypes.data, blob.ctypes.data, err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def call(self, forest: Forest, refs, max_steps: int = 65536, flags: int = 0, profile=None, max_level: int = 0,
             max_ref_length: int = 0, max_allele_length: int = 0, regions=None, region_no_mask: bool = False, cluster=None,
             cluster_no_bound: bool = False, spanning: bool = False) -> Calls:
        """The variant calls of `forest` (INTEGRATION.md "Variant calls") with the resident paths whose names start with one
        of the prefixes `refs` as references, on the GPU (paths and sequences uploaded first).  flags: T_FORCE_TIER2,
        T_INVERSIONS (the SUBR records of "Inversion calls" merged in: Calls.n_steps, flags & CALL_SUBR, the n_inv_* counters),
        T_NESTED ("Nested calls": records count classes of alleles modulo enclosed sites; Calls.level, parent_query,
        ref_spelled, flags & CALL_COLLAPSED, the counters).  profile: None or one of PROFILES; "top-level-only" and "popped"
        imply T_NESTED and keep what INTEGRATION.md says ("popped": max_level, max_ref_length, max_allele_length, 0 = no
        limit); "left-normalized" implies nothing, keeps every record and left-normalises it ("Left-normalised calls":
        Calls.raw_pos, norm_block, norm_shift, norm_chop, norm_trim, flags & CALL_NORMALIZED, the counters); "decomposed"
        implies nothing either, keeps every record and writes every (REF, ALT) as the primitives of its alignment ("Decomposed
        calls": Calls.n_rows, row_*, the counters; max_allele_length is the longest text that is aligned, 0 = PRIM_MAX_LENGTH,
        more is refused; T_FORCE_TIER2 also sends every aligned pair through the striped kernel; with T_MERGE equal primitives
        are merged: Calls.merged, n_mrows, mrow_*, the counters, and vcf_text writes the merged rows).  T_OFFREF ("Off-reference
        calls"): the sites no reference path crosses are called on their surrogate path; Calls.offref, rec_offref, host_query,
        host_allele, off_contig_*, the counters.  T_UNTANGLE ("Untangled calls"): where a path walks a site more than once its
        laps are aligned with the reference's and every record takes the allele of the lap aligned with its own;
        Calls.untangled, rec_unt, lap, n_laps, lap_count, the UNTANGLE_COUNTERS, and vcf_text writes LN, LC and GT:CN.  regions
        ("Region calls"): strings "name:start-end" or tuples (name, start, end), the 1-based bases [start, end) of the resident
        path named exactly so; the records are those of the same call without regions for the sites with a boundary segment, and
        the inversions with an end step, that a region meets; the REGION_COUNTERS.  A call that is not nested masks the other
        sites in front of its scans; region_no_mask makes it scan every site and select the records at the end, as a nested call
        does (tests).  cluster ("Clustered calls"): the threshold F as decimal text ("0.9", at most six decimals, 0 < F <= 1) or
        as an integer of parts per million; the exact alleles of a site whose bags of inner segments are that similar are one
        allele, written as its first member; Calls.cluster_ppm, rec_clustered, cl_minsim, cl_nx (Calls.nx), the
        CLUSTER_COUNTERS, and vcf_text writes NX and MINSIM.  cluster_no_bound reads every pair of bags, whatever their weights
        say (tests).  spanning (or T_SPANNING in flags; "Spanning alleles"): an option of the nested call -- an entry whose
        slot has no traversal of the record's site but traverses the site of an enclosing record is written as a `*` ALT, the
        record's last, instead of '.'; Calls.spanning, rec_star, the SPAN_COUNTERS; refused without T_NESTED or a profile that
        implies it, and under "left-normalized" and "decomposed".  Which of the flags, the profiles, regions and cluster combine is declared once, as RULES of
        povu_amd/csrc/hip/call_modes.hpp, with the message a refused combination raises."""
        if profile is not None and profile not in PROFILES:
            raise ValueError(f"profile must be one of {sorted(PROFILES)}")
        names = self._path_names
        if isinstance(refs, str):
            refs = [refs]
        name_array = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        prefixes = (C.c_char_p * max(len(refs), 1))(*[p.encode() for p in refs])
        err = C.create_string_buffer(512)
        nr = self._lib.povu_hip_call_names_make(len(names), name_array, len(refs), prefixes, err, 512)
        if not nr:
            raise RuntimeError(err.value.decode())
        try:
            sites = forest.sites()
            o = _TravOpts(max_steps, flags | (T_SPANNING if spanning else 0))
            po = _ProfileOpts(PROFILES[profile or "raw-graph"], max_level, max_ref_length, max_allele_length)
            rg = self._regions(regions, names, name_array, region_no_mask)
            co = None
            if cluster is not None:
                ppm = C.c_uint32(0)
                if isinstance(cluster, str):
                    if self._lib.povu_hip_cluster_parse(cluster.encode(), C.byref(ppm), err, 512) != 0:
                        raise RuntimeError(err.value.decode())
                elif isinstance(cluster, int) and not isinstance(cluster, bool) and 1 <= cluster <= 10 ** 6:
                    ppm = C.c_uint32(cluster)
                else:
                    raise RuntimeError(f"cluster threshold '{cluster}': decimal text such as \"0.9\", or parts per million in 1 .. 10^6")
                co = C.byref(_ClusterOpts(ppm.value, CLUSTER_NO_BOUND if cluster_no_bound else 0))
            p = self._lib.povu_hip_call_clustered(self._ctx, sites._p, C.byref(nr.contents.refs), nr.contents.slot_of_path, C.byref(o),
                                                  C.byref(po) if profile is not None else None, rg, co, err, 512)
            if not p:
                raise RuntimeError(err.value.decode())
        except Exception:
            self._lib.povu_hip_call_names_free(nr)
            raise
        return Calls(self._lib, p, names, nr, name_array, sites, profile or "raw-graph")

    def _regions(self, regions, names, name_array, no_mask):
        """povu_hip_call_regions of `regions` (None for none): a string goes through povu_hip_region_parse, a tuple's name is
        looked up exactly."""
        if not regions:
            return None
        if isinstance(regions, (str, tuple)):
            regions = [regions]
        arr = (_Region * len(regions))()
        for k, r in enumerate(regions):
            if isinstance(r, str):
                err = C.create_string_buffer(512)
                if self._lib.povu_hip_region_parse(r.encode(), len(names), name_array, C.byref(arr[k]), err, 512) != 0:
                    raise RuntimeError(err.value.decode())
            else:
                name, start, end = r
                if name not in names:
                    raise RuntimeError(f"region '{name}:{start}-{end}': no path is named {name}")
                if not (0 <= int(start) < 2 ** 64 and 0 <= int(end) < 2 ** 64):
                    raise RuntimeError(f"region '{name}:{start}-{end}': start and end must be in [0, 2^64)")
                arr[k] = _Region(names.index(name), 0, int(start), int(end))
        rg = _CallRegions(len(regions), REGION_NO_MASK if no_mask else 0, arr)
        rg._keep = arr
        return C.byref(rg)

    def check_vcf(self, text, forward_only: bool = False, spelling: bool = False, force_tier2: bool = False, threads: int = 1) -> VcfReport:
        """Does the VCF `text` (or a VcfDoc of parse_vcf) still describe the graph (INTEGRATION.md "VCF checks")?  For every
        record and every haplotype that carries an allele, the allele's AT walk must occur in a resident path of that haplotype
        (paths uploaded first), forward or -- unless forward_only -- reversed; spelling: REF and ALT must also spell their walks
        (sequences uploaded first; meant for raw-graph output, rewritten records fail it); force_tier2: every search through
        the wave-per-unit kernel (tests)."""
        doc = text if isinstance(text, VcfDoc) else parse_vcf(text, threads)
        names = getattr(self, "_path_names", [])
        name_array = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        err = C.create_string_buffer(512)
        nr = self._lib.povu_hip_vcf_names_make(len(names), name_array, err, 512)
        if not nr:
            raise RuntimeError(err.value.decode())
        o = _VcfOpts((V_FORWARD_ONLY if forward_only else 0) | (V_SPELLING if spelling else 0) | (V_FORCE_TIER2 if force_tier2 else 0))
        p = self._lib.povu_hip_vcf_check(self._ctx, doc._p, nr, C.byref(o), err, 512)
        if not p:
            self._lib.povu_hip_call_names_free(nr)
            raise RuntimeError(err.value.decode())
        return VcfReport(self._lib, p, doc, nr)

    def compare_vcfs(self, a, b, force_tier2: bool = False, threads: int = 1) -> VcfComparison:
        """How do the calls of VCF `a` differ from those of `b` (text or a VcfDoc of parse_vcf each; INTEGRATION.md "VCF
        comparison")?  Every (record, ALT) is keyed by (CHROM, POS', REF', ALT') after the case fold and the suffix-then-prefix
        trim, equal keys form a group (shared, only A, only B), and per group and sample column of both documents the doses
        of both sides are compared (tp, fp, fn, gteq).  Needs no graph: a fresh context will do.  force_tier2: every item through
        the wave-per-item kernel (tests)."""
        doc_a = a if isinstance(a, VcfDoc) else parse_vcf(a, threads)
        doc_b = b if isinstance(b, VcfDoc) else parse_vcf(b, threads)
        err = C.create_string_buffer(512)
        o = _VcfOpts(V_FORCE_TIER2 if force_tier2 else 0)
        p = self._lib.povu_hip_vcf_compare(self._ctx, doc_a._p, doc_b._p, C.byref(o), err, 512)
        if not p:
            raise RuntimeError(err.value.decode())
        return VcfComparison(self._lib, p, doc_a, doc_b)

    def compare_haplotypes(self, a, b, reference: bool = False, max_reach: int = H_MAX_REACH_DEFAULT, force_tier2: bool = False,
                           threads: int = 1) -> HapComparison:
        """Per region, sample and phase: do VCF `a` and VCF `b` (text or a VcfDoc of parse_vcf each) spell the same bases
        (INTEGRATION.md "Haplotype comparison")?  Every (record, ALT) becomes an edit by the full suffix-then-prefix trim, the
        records of both fall into windows, and per (window, common sample, phase) the edits either side's GT entries name are
        applied to the window's text and the haplotypes compared.  reference: the resident paths and sequences are the reference
        (CHROM names a path; every indel reaches up to max_reach bases through its repeat), else the REF fields are and no graph
        is needed.  force_tier2: every item through the wave-per-item kernel (tests)."""
        doc_a = a if isinstance(a, VcfDoc) else parse_vcf(a, threads)
        doc_b = b if isinstance(b, VcfDoc) else parse_vcf(b, threads)
        if not 0 <= int(max_reach) < 2 ** 32:
            raise ValueError("max_reach must be in [0, 2^32)")
        err = C.create_string_buffer(512)
        o = _VcfHapOpts(V_FORCE_TIER2 if force_tier2 else 0, int(max_reach))
        names, name_array = [], None
        if reference:
            names = getattr(self, "_path_names", [])
            name_array = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        p = self._lib.povu_hip_vcf_haplotypes(self._ctx, doc_a._p, doc_b._p, name_array, len(names), C.byref(o), err, 512)
        if not p:
            raise RuntimeError(err.value.decode())
        return HapComparison(self._lib, p, doc_a, doc_b)

    def consensus(self, vcf, roundtrip: bool = False, text: bool = True, samples=None, chroms=None, force_tier2: bool = False,
                  threads: int = 1, time_write: bool = False) -> Consensus:
        """The haplotypes the calls of `vcf` (text or a VcfDoc of parse_vcf) spell on the resident paths their CHROMs name
        (INTEGRATION.md "Consensus haplotypes"; paths and sequences uploaded first): per (CHROM, sample column, phase) the
        path's bases with the edits of the named ALTs applied, an edit inside or across one in front of it dropped and counted.
        roundtrip: every haplotype is compared with the one path of its slot.  text=False: lengths, counts and the round trip
        only.  samples / chroms: names of the sample columns / CHROMs to restrict the call to.  force_tier2: every item through
        the wave-per-item kernel (tests).  time_write: Consensus.write_ms is measured (the call then waits for the materialiser)."""
        doc = vcf if isinstance(vcf, VcfDoc) else parse_vcf(vcf, threads)
        names = getattr(self, "_path_names", [])
        name_array = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        cols = chr_ids = None
        if samples is not None:
            missing = [x for x in samples if x not in doc.samples]
            if missing:
                raise ValueError(f"no sample column is named {missing[0]}")
            cols = sorted({c for c, n in enumerate(doc.samples) if n in samples})
        if chroms is not None:
            missing = [x for x in chroms if x not in doc.chroms]
            if missing:
                raise ValueError(f"no record has the CHROM {missing[0]}")
            chr_ids = sorted({doc.chroms.index(x) for x in chroms})
        # (the two lists have one length: the shorter is padded with its own first entry)
        n = max(len(cols or []), len(chr_ids or []))
        pad = lambda v: None if v is None else (C.c_uint32 * max(n, 1))(*(list(v) + [v[0]] * (n - len(v)) if v else []))  # noqa: E731
        if (cols is not None and not cols) or (chr_ids is not None and not chr_ids):
            raise ValueError("an empty selection")
        ca, ha = pad(cols), pad(chr_ids)
        o = _VcfConsOpts((C_ROUNDTRIP if roundtrip else 0) | (0 if text else C_NO_TEXT) | (V_FORCE_TIER2 if force_tier2 else 0) |
                         (C_TIME_WRITE if time_write else 0), n,
                         C.cast(ca, C.POINTER(C.c_uint32)) if ca is not None else None, C.cast(ha, C.POINTER(C.c_uint32)) if ha is not None else None)
        err = C.create_string_buffer(512)
        p = self._lib.povu_hip_vcf_consensus(self._ctx, doc._p, name_array, len(names), C.byref(o), err, 512)
        if not p:
            raise RuntimeError(err.value.decode())
        return Consensus(self._lib, p, doc, names)

    def traversals(self, forest: Forest, max_steps: int = 65536, flags: int = 0) -> Traversals:
        """The traversals of every flubble of `forest` by the resident paths, on the GPU."""
        if not 2 <= int(max_steps) < 2 ** 32:
            raise ValueError("max_steps must be in [2, 2^32)")
        o = _TravOpts(max_steps, flags)
        err = C.create_string_buffer(512)
        p = self._lib.povu_hip_forest_traversals(self._ctx, forest._h, C.byref(o), err, 512)
        if not p:
            raise RuntimeError(err.value.decode())
        return Traversals(self._lib, p, forest, _query_firsts(self._lib, forest))

    def stage_times(self) -> List[dict]:
        buf = (_StageTime * 64)()
        n = self._lib.povu_hip_last_stage_times(self._ctx, buf, 64)
        return [dict(name=buf[i].name.decode(), ms=buf[i].ms, launches=buf[i].launches) for i in range(min(n, 64))]

    def seq_redo_count(self) -> int:
        return int(self._lib.povu_hip_last_seq_redo(self._ctx))

    def links_processed(self) -> int:
        return int(self._lib.povu_hip_last_links_processed(self._ctx))

    # ---- parity hooks
    @staticmethod
    def _prim_rc(rc: int, primitive: str):
        """Return code of a primitive's unit-test hook: 5 = the primitive wrote outside its output."""
        if rc == 5:
            raise GuardBandError(f"{primitive}: a guard band around a device output changed")
        if rc:
            raise RuntimeError(f"{primitive}: debug hook failed ({rc})")

    def debug_scan(self, a, op: int = 0, b=None, in_place: bool = False):
        """Unit-test hook: exclusive scan of `a` on the device (op 0 sum, 1 running max, 2 sum of uint64 values);
        with `b`, an independent sum scan of `b` in the same launch.  `in_place`: the output is the input on the device."""
        a = np.ascontiguousarray(a, dtype=np.uint64 if op == 2 else np.uint32)
        out = np.empty_like(a)
        name = ("scan_exclusive_u32", "scan_exclusive_max_u32", "scan_exclusive_u64")[op]
        if b is None:
            rc = self._lib.povu_hip_debug_scan(self._ctx, op | (SCAN_IN_PLACE if in_place else 0), a.ctypes.data,
                                               out.ctypes.data, a.size, None, None, 0)
            self._prim_rc(rc, name + (" (in place)" if in_place else ""))
            return out
        b = np.ascontiguousarray(b, dtype=np.uint32)
        out2 = np.empty_like(b)
        rc = self._lib.povu_hip_debug_scan(self._ctx, op, a.ctypes.data, out.ctypes.data, a.size, b.ctypes.data,
                                           out2.ctypes.data, b.size)
        self._prim_rc(rc, "scan_exclusive_u32_pair" if op == 0 else name)
        return out, out2

    def debug_scan_inclusive(self, a):
        """Unit-test hook of scan_inclusive_u32: inclusive sums (mod 2^32) of the words `a`."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        out = np.empty_like(a)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_INCLUSIVE, a.ctypes.data, out.ctypes.data, a.size, None, None, 0)
        self._prim_rc(rc, "scan_inclusive_u32")
        return out

    def count_record_tiles(self) -> tuple:
        """Elements a tile of the count-record scan covers: (two-launch form, one-launch form)."""
        tile = (C.c_uint64 * 2)()
        self._lib.povu_hip_debug_count_records(None, None, 0, None, 0, None, None, None, None, 0, None, 0, None, None, None, tile)
        return int(tile[0]), int(tile[1])

    def debug_count_records(self, a, pos_a, b=None, pos_b=None):
        """Unit-test hook of the count records (scan_count_records_u8, cntrec_prefix, cntrec_count) over the bytes `a`
        and, in the same launch, `b`: per job (records, prefix, count) -- records = the (n + 11) // 12 records as rows
        (three words of count bytes, the sum in front), prefix[i] = the sum of the bytes in front of positions[i] (<
        n), count[i] = the byte at positions[i].  Without `b` one such triple, else a pair of them."""
        jobs, args = [], []
        for x, pos in ((a, pos_a), (b, pos_b)):
            if x is None:
                args += [None, 0, None, 0, None, None, None]
                continue
            x = np.ascontiguousarray(x, dtype=np.uint8)
            pos = np.ascontiguousarray(pos if pos is not None else [], dtype=np.uint32)
            rec = np.empty(((x.size + 11) // 12, 4), dtype=np.uint32)
            pre, cnt = np.empty(pos.size, dtype=np.uint32), np.empty(pos.size, dtype=np.uint32)
            jobs.append((x, pos, rec, pre, cnt))
            args += [x.ctypes.data, x.size, pos.ctypes.data, pos.size, rec.ctypes.data, pre.ctypes.data, cnt.ctypes.data]
        rc = self._lib.povu_hip_debug_count_records(self._ctx, *args, None)
        self._prim_rc(rc, "scan_count_records_u8")
        out = [(j[2], j[3], j[4]) for j in jobs]
        return out[0] if b is None else tuple(out)

    def debug_scan_u8(self, a, b=None):
        """Unit-test hook of scan_exclusive_u8: exclusive sums (uint32) of the bytes `a`; with `b`, of both in the same
        launch.  Either may be empty."""
        a = np.ascontiguousarray(a, dtype=np.uint8)
        out = np.empty(a.size, dtype=np.uint32)
        if b is None:
            rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_U8, a.ctypes.data, out.ctypes.data, a.size, None, None, 0)
            self._prim_rc(rc, "scan_exclusive_u8")
            return out
        b = np.ascontiguousarray(b, dtype=np.uint8)
        out2 = np.empty(b.size, dtype=np.uint32)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_U8, a.ctypes.data, out.ctypes.data, a.size, b.ctypes.data,
                                           out2.ctypes.data, b.size)
        self._prim_rc(rc, "scan_exclusive_u8 (two jobs)")
        return out, out2

    def debug_scan_diff(self, a, sub):
        """Unit-test hook of scan_exclusive_diff_u32: exclusive sums of a[i] - sub[i] mod 2^32."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        sub = np.ascontiguousarray(sub, dtype=np.uint32)
        assert a.size == sub.size
        out = np.empty_like(a)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_DIFF, a.ctypes.data, out.ctypes.data, a.size, sub.ctypes.data,
                                           None, sub.size)
        self._prim_rc(rc, "scan_exclusive_diff_u32")
        return out

    def debug_scan_diff_u8(self, a, sub):
        """Unit-test hook of scan_exclusive_diff_u8_u32: exclusive sums of a[i] - sub[i] mod 2^32, `a` bytes, `sub` words."""
        a = np.ascontiguousarray(a, dtype=np.uint8)
        sub = np.ascontiguousarray(sub, dtype=np.uint32)
        assert a.size == sub.size
        out = np.empty(a.size, dtype=np.uint32)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_DIFF_U8, a.ctypes.data, out.ctypes.data, a.size, sub.ctypes.data,
                                           None, sub.size)
        self._prim_rc(rc, "scan_exclusive_diff_u8_u32")
        return out

    def debug_scan_diff_u8_u8(self, a, sub):
        """Unit-test hook of scan_exclusive_diff_u8_u8: exclusive sums of a[i] - sub[i] mod 2^32, both bytes."""
        a = np.ascontiguousarray(a, dtype=np.uint8)
        sub = np.ascontiguousarray(sub, dtype=np.uint8)
        assert a.size == sub.size
        out = np.empty(a.size, dtype=np.uint32)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_DIFF_U8_U8, a.ctypes.data, out.ctypes.data, a.size, sub.ctypes.data,
                                           None, sub.size)
        self._prim_rc(rc, "scan_exclusive_diff_u8_u8")
        return out

    def debug_scan_mixed_pair(self, a, b):
        """Unit-test hook of scan_exclusive_u32_u8_pair: exclusive sums of the words `a` and of the bytes `b`, one launch."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint8)
        out, out2 = np.empty_like(a), np.empty(b.size, dtype=np.uint32)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_MIXED_PAIR, a.ctypes.data, out.ctypes.data, a.size, b.ctypes.data,
                                           out2.ctypes.data, b.size)
        self._prim_rc(rc, "scan_exclusive_u32_u8_pair")
        return out, out2

    def debug_scan_xor_pair(self, a, b):
        """Unit-test hook of scan_exclusive_xor_u32_pair: the exclusive running xor of `a` and of `b` (same length)."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        assert a.size == b.size
        out, out2 = np.empty_like(a), np.empty_like(b)
        rc = self._lib.povu_hip_debug_scan(self._ctx, SCAN_XOR_PAIR, a.ctypes.data, out.ctypes.data, a.size,
                                           b.ctypes.data, out2.ctypes.data, b.size)
        self._prim_rc(rc, "scan_exclusive_xor_u32_pair")
        return out, out2

    def debug_scan_xor_u128(self, a, n_dev=None):
        """Unit-test hook of scan_exclusive_xor_u128: the exclusive running xor of the 16-byte words a[i] (an (n, 2)
        array of uint64).  With `n_dev`, that value goes into a device word: only the first min(n_dev + 1, n) words
        exist, and only those are returned (the hook has checked that the rest of the output still holds its guard
        pattern)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        assert a.ndim == 2 and a.shape[1] == 2
        out = np.empty_like(a)
        op = SCAN_XOR_U128 | (SCAN_N_DEV if n_dev is not None else 0)
        rc = self._lib.povu_hip_debug_scan(self._ctx, op, a.ctypes.data, out.ctypes.data, a.shape[0], None, None,
                                           n_dev or 0)
        self._prim_rc(rc, "scan_exclusive_xor_u128")
        return out if n_dev is None else out[:min(n_dev + 1, a.shape[0])]

    def debug_sort(self, keys, vals, bits: int):
        """Unit-test hook of sort_pairs_u32: (keys, vals) in the stable order of the keys' low `bits` bits."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        assert keys.size == vals.size
        ko, vo = np.empty_like(keys), np.empty_like(vals)
        rc = self._lib.povu_hip_debug_sort(self._ctx, keys.ctypes.data, vals.ctypes.data, keys.size, bits,
                                           ko.ctypes.data, vo.ctypes.data)
        self._prim_rc(rc, "sort_pairs_u32")
        return ko, vo

    def debug_compact(self, flags):
        """Unit-test hook of compact_flagged_u8: the indices of the non-zero bytes of `flags`, ascending."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        out = np.empty(flags.size, dtype=np.uint32)
        cnt = C.c_uint32(0)
        rc = self._lib.povu_hip_debug_compact(self._ctx, flags.ctypes.data, flags.size, out.ctypes.data, C.byref(cnt))
        self._prim_rc(rc, "compact_flagged_u8")
        if cnt.value > flags.size:
            raise RuntimeError(f"compact_flagged_u8: count {cnt.value} of {flags.size} flags")
        return out[:cnt.value], int(cnt.value)

    def debug_totals(self, a, b=None):
        """Unit-test hook of totals_u32: the 64-bit sum of `a`, and of `b` (same length) when given."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        tot = (C.c_uint64 * 2)()
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.uint32)
            assert a.size == b.size
        rc = self._lib.povu_hip_debug_totals(self._ctx, a.ctypes.data, b.ctypes.data if b is not None else None, a.size, tot)
        self._prim_rc(rc, "totals_u32")
        return int(tot[0]) if b is None else (int(tot[0]), int(tot[1]))

    def debug_segtree(self, values, queries, want_tree: bool = False):
        """Unit-test hook of the coarse min segment tree (segtree.hpp): seg_build over `values`, then one lane per row
        (kind, l, r, x) of `queries` (kind SEG_MIN / SEG_FIRST_LESS / SEG_LAST_LESS; r <= len(values)).  Returns one
        word per query (0xFFFFFFFF: empty range, or no such index); with `want_tree` also the nodes [0, 2 P) of the
        built tree (node 1 the root, node 0 undefined) and P."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        queries = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 4)
        out = np.empty(queries.shape[0], dtype=np.uint32)
        P = 1
        while P * 16 < values.size:
            P *= 2
        tree = np.empty(2 * P, dtype=np.uint32) if want_tree else None
        p_dev = C.c_uint32(0)
        rc = self._lib.povu_hip_debug_segtree(self._ctx, values.ctypes.data, values.size, queries.ctypes.data, queries.shape[0],
                                              out.ctypes.data, tree.ctypes.data if want_tree else None, C.byref(p_dev))
        self._prim_rc(rc, "segment tree (seg_build / seg_min / seg_first_less / seg_last_less)")
        if p_dev.value != P:
            raise RuntimeError(f"segment tree: P = {p_dev.value} for {values.size} values, {P} expected")
        return (out, tree, P) if want_tree else out

    def debug_bitrank(self, flags, positions):
        """Unit-test hook of the bit-rank directory (bitrank_store_wave, bitrank_build, bitrank, bitrank_test) over the
        byte flags `flags`: (rank, test, records) -- rank[i] = set flags in front of positions[i] (<= len(flags)),
        test[i] = flag positions[i] as 0 / 1 (only where positions[i] < len(flags); other entries are meaningless),
        records = the len(flags) // 64 + 2 records as rows (bits 0..31, bits 32..63, set flags in front, 0)."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        rank, test = np.empty(positions.size, dtype=np.uint32), np.empty(positions.size, dtype=np.uint32)
        records = np.empty((flags.size // 64 + 2, 4), dtype=np.uint32)
        rc = self._lib.povu_hip_debug_bitrank(self._ctx, flags.ctypes.data, flags.size, positions.ctypes.data, positions.size,
                                              rank.ctypes.data, test.ctypes.data, records.ctypes.data)
        self._prim_rc(rc, "bit-rank directory (bitrank_store_wave / bitrank_build)")
        return rank, test, records

    def debug_append(self, flags):
        """Unit-test hook of append_in_order: the positions of the non-zero bytes of `flags` as workgroups of 256 lanes,
        each over 16 384 positions, append them to one list; (list, its length)."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        out = np.empty(flags.size, dtype=np.uint32)
        cnt = C.c_uint32(0)
        rc = self._lib.povu_hip_debug_append(self._ctx, flags.ctypes.data, flags.size, out.ctypes.data, C.byref(cnt))
        self._prim_rc(rc, "append_in_order")
        if cnt.value > flags.size:
            raise RuntimeError(f"append_in_order: length {cnt.value} of {flags.size} flags")
        return out[:cnt.value], int(cnt.value)

    def debug_list_rank(self, nxt, w, heads, events: bool = False, bits: int = 0):
        """Unit-test hook: the tree stage's list ranking of the lists `nxt` (NIL ends a list) headed by `heads`,
        ranks as its readers resolve them.  Suffix sums (inclusive, mod 2^32) of the 0/1 weights `w`; with
        `events`, the pair of sums of the pre-order events' weights (x % 3 == 0 enters).  `bits`: splitter
        bucket bits (0 = the default).  Elements in no list get no defined value."""
        nxt = np.ascontiguousarray(nxt, dtype=np.uint32)
        w = np.ascontiguousarray(w, dtype=np.uint8)
        heads = np.ascontiguousarray(heads, dtype=np.uint32)
        ra = np.zeros(nxt.size, dtype=np.uint32)
        rb = np.zeros(nxt.size, dtype=np.uint32)
        rc = self._lib.povu_hip_debug_list_rank(self._ctx, nxt.size, nxt.ctypes.data, w.ctypes.data,
                                                heads.ctypes.data if heads.size else None, heads.size,
                                                1 if events else 0, bits, ra.ctypes.data, rb.ctypes.data)
        if rc:
            raise RuntimeError(f"debug_list_rank failed ({rc})")
        self._last_list_rank_n = nxt.size
        return (ra, rb) if events else ra

    def debug_rank_escapes(self, which: str = "list_rank", flags: bool = False):
        """Read-only hook: what a level-0 walk left in its records.  `which`: "tour" / "events" of the last pass (run
        with POVU_HIP_RANK_STATS set), or "list_rank", the last debug_list_rank call.  A dict: live, escaped,
        final_ranks, bucket_bits, delta_bits, partial_bits, hist[33, 33] (delta bits x partial bits); with `flags`
        (list_rank only) also esc, one byte per element."""
        k = {"tour": 0, "events": 1, "list_rank": 2}[which]
        rec = _RankRecords()
        esc = np.zeros(self._last_list_rank_n if flags else 0, dtype=np.uint8)
        rc = self._lib.povu_hip_debug_rank_escapes(self._ctx, k, C.byref(rec), esc.ctypes.data if flags else None, esc.size)
        if rc:
            raise RuntimeError(f"debug_rank_escapes failed ({rc})")
        out = {"live": int(rec.live), "escaped": int(rec.escaped), "final_ranks": bool(rec.final_ranks),
               "bucket_bits": int(rec.bucket_bits), "delta_bits": int(rec.delta_bits),
               "partial_bits": (int(rec.partial_bits[0]), int(rec.partial_bits[1])),
               "hist": np.ctypeslib.as_array(rec.hist).reshape(33, 33).copy()}
        if flags:
            out["esc"] = esc
        return out

    def debug_components(self, n_vtx: int):
        comp = np.zeros(n_vtx, dtype=np.uint32)
        loc = np.zeros(n_vtx, dtype=np.uint32)
        if self._lib.povu_hip_debug_components(self._ctx, comp.ctypes.data, loc.ctypes.data) != 0:
            raise RuntimeError("no decompose state")
        return comp, loc

    def componetize(self) -> dict:
        """Row B on its own (povu_hip_componetize): the components as bd::VG::componetize builds them.  vtx_off / link_off
        [C + 1]; vtx_id / vtx_tip by local vertex order, component-major; the local links (v1, s1, v2, s2) in local link order,
        with LOCAL vertex indices."""
        err = C.create_string_buffer(512)
        p = self._lib.povu_hip_componetize(self._ctx, err, 512)
        if not p:
            raise RuntimeError(err.value.decode())
        try:
            c = p.contents
            nc, nv, ne = c.n_components, c.n_vtx, c.n_links
            return dict(n_components=nc, vtx_off=_view(c.vtx_off, nc + 1, np.uint32).copy(), link_off=_view(c.link_off, nc + 1, np.uint32).copy(),
                        vtx_id=_view(c.vtx_id, nv, np.uint32).copy(), vtx_tip=_view(c.vtx_tip, nv, np.uint8).copy(),
                        v1=_view(c.l_v1, ne, np.uint32).copy(), v2=_view(c.l_v2, ne, np.uint32).copy(),
                        s1=_view(c.l_s1, ne, np.uint8).copy(), s2=_view(c.l_s2, ne, np.uint8).copy())
        finally:
            self._lib.povu_hip_components_free(p)

    def debug_csr(self, n_vtx: int, n_links: int) -> dict:
        """What the last upload left (povu_hip_debug_csr): off, adj, aoth, atwin, tip, max_vdeg, n_empty_sides and slot_fill
        (True: slot fill + insertion sort built the lists; False: the radix sort)."""
        off = np.zeros(2 * n_vtx + 1, dtype=np.uint32)
        adj, aoth, atwin = (np.zeros(2 * n_links, dtype=np.uint32) for _ in range(3))
        tip = np.zeros(n_vtx, dtype=np.uint8)
        w = (C.c_uint32 * 4)()
        if self._lib.povu_hip_debug_csr(self._ctx, off.ctypes.data, adj.ctypes.data, aoth.ctypes.data, atwin.ctypes.data,
                                        tip.ctypes.data, w) != 0:
            raise RuntimeError("povu_hip_debug_csr failed")
        n = int(w[0])
        return dict(off=off, adj=adj[:n], aoth=aoth[:n], atwin=atwin[:n], tip=tip, n_slots=n, max_vdeg=int(w[1]),
                    n_empty_sides=int(w[2]), slot_fill=bool(w[3]))

    def debug_row_b(self, n_vtx: int, n_links: int, flags: int = 0) -> dict:
        """Runs the row-B step of a pass on the resident graph under the pass flags (povu_hip_debug_row_b) and returns what
        it left: C, voff, eoff, comp / pos of every segment, loff / ladj / lle over the local slots, start_key [C] (~0: no
        tip), stats0, the ROWB_* path bits and n_cross."""
        voff, eoff = np.zeros(n_vtx + 1, dtype=np.uint32), np.zeros(n_vtx + 1, dtype=np.uint32)
        comp, pos = np.zeros(n_vtx, dtype=np.uint32), np.zeros(n_vtx, dtype=np.uint32)
        loff = np.zeros(2 * n_vtx + 1, dtype=np.uint32)
        ladj, lle = np.zeros(2 * n_links, dtype=np.uint32), np.zeros(2 * n_links, dtype=np.uint32)
        key = np.zeros(n_vtx + 1, dtype=np.uint64)
        r = _RowB(0, 0, 0, 0, 0, voff.ctypes.data, eoff.ctypes.data, comp.ctypes.data, pos.ctypes.data, loff.ctypes.data,
                  ladj.ctypes.data, lle.ctypes.data, key.ctypes.data)
        rc = self._lib.povu_hip_debug_row_b(self._ctx, flags, C.byref(r))
        if rc != 0:
            raise RuntimeError(f"povu_hip_debug_row_b failed ({rc})")
        nc, n = r.n_components, r.n_local_slots
        return dict(C=nc, voff=voff[:nc + 1], eoff=eoff[:nc + 1], comp=comp, pos=pos, loff=loff, ladj=ladj[:n], lle=lle[:n],
                    start_key=key[:nc], stats0=r.stats0, bits=r.path_bits, n_cross=r.n_cross)

    def debug_tree(self, comp: int):
        n = C.c_uint32(0)
        if self._lib.povu_hip_debug_tree(self._ctx, comp, C.byref(n), None, None, None, None) != 0:
            raise RuntimeError("no decompose state")
        gid = np.zeros(n.value, dtype=np.uint32)
        typ = np.zeros(n.value, dtype=np.uint8)
        par = np.zeros(n.value, dtype=np.uint32)
        cls = np.zeros(n.value, dtype=np.uint32)
        self._lib.povu_hip_debug_tree(self._ctx, comp, C.byref(n), gid.ctypes.data, typ.ctypes.data, par.ctypes.data,
                                      cls.ctypes.data)
        return dict(gid=gid, typ=typ & 3, black=(typ >> 2) & 1, root=(typ >> 3) & 1, par=par, cls=cls)

    def last_narrow_counts(self) -> bool:
        """True when the last pass kept the bracket counts per tree vertex as bytes (no side with more than 253 links);
        False when the word kernels ran (a fat side, or POVU_HIP_WIDE_COUNTS=1 in the environment)."""
        return bool(self._lib.povu_hip_last_narrow_counts(self._ctx))

    def last_narrow_forms(self) -> tuple:
        """(ordcnt, srccnt, incnt): which of the three counts per tree vertex the last pass kept as bytes."""
        m = int(self._lib.povu_hip_last_narrow_counts(self._ctx))
        return bool(m & 1), bool(m & 2), bool(m & 4)

    def last_prefix_records(self) -> int:
        """Which prefix sums the class stage of the last pass read as packed count records instead of words: bit 0 = the
        sums of the in-counts, bit 1 = the range starts of the bracket lists (records exactly where the matching count is
        a byte, unless POVU_HIP_WORD_PREFIX in the environment says words: 1 = both, 2 = the first, 3 = the second)."""
        return int(self._lib.povu_hip_last_prefix_records(self._ctx))

    def wide_repeat_count(self) -> int:
        """Passes of this context that ran their tree and class stages again with word counts (a byte in-count at 255)."""
        return int(self._lib.povu_hip_wide_repeats(self._ctx))

    def last_black_only_classes(self) -> bool:
        """True when the last pass numbered the cycle classes of the black tree edges only (the fast path)."""
        return bool(self._lib.povu_hip_last_black_only_classes(self._ctx))

    def last_crossings(self):
        """(flagged, crossed): candidate-stack entries whose interval is crossed, and those of them whose class was no longer
        open (povu_hip_last_crossings); (0, 0) when the laminarity check did not run."""
        o = (C.c_uint32 * 2)()
        if self._lib.povu_hip_last_crossings(self._ctx, o) != 0:
            raise RuntimeError("povu_hip_last_crossings failed")
        return int(o[0]), int(o[1])

    def last_lsz_field(self):
        """(bits, saturated) of the last black-only class pass: the bits of the class sort's payload that carried an entry's
        bracket-list size (POVU_HIP_LSZ_FIELD in the environment caps them, 0 = none), and the candidate-stack entries whose
        size did not fit (>= 2^bits - 1) and was looked up instead (povu_hip_last_lsz_field); (0, 0) behind any other pass."""
        o = (C.c_uint32 * 2)()
        if self._lib.povu_hip_last_lsz_field(self._ctx, o) != 0:
            raise RuntimeError("povu_hip_last_lsz_field failed")
        return int(o[0]), int(o[1])

    def last_laminar_check_ran(self) -> bool:
        """True when the last pass ran the laminarity check (the literal hi_2 rule deviated somewhere, or it was forced)."""
        return bool(self._lib.povu_hip_last_laminar_check_ran(self._ctx))

    def debug_edge_ids(self, comp: int):
        """Id of the tree edge into every tree vertex ([0] = 0xFFFFFFFF), Tree::add_tree_edge's shared counter."""
        n = C.c_uint32(0)
        rc = self._lib.povu_hip_debug_edge_ids(self._ctx, comp, C.byref(n), None)
        if rc != 0:
            raise RuntimeError("no parallel-tree state" if rc == 3 else "no decompose state")
        ids = np.zeros(n.value, dtype=np.uint32)
        if self._lib.povu_hip_debug_edge_ids(self._ctx, comp, C.byref(n), ids.ctypes.data) != 0:
            raise RuntimeError("povu_hip_debug_edge_ids failed")
        return ids

    def debug_walk_words(self):
        """dict(n_entry, n_over, pool_top) of the last pass's class walks (povu_hip_debug_walk_words): classes of more than
        one side, classes handed from the one-lane walk to the wave walk, stack-pool entries the wave walks took."""
        o = (C.c_uint32 * 3)()
        rc = self._lib.povu_hip_debug_walk_words(self._ctx, o)
        if rc != 0:
            raise RuntimeError("no parallel-tree state" if rc in (3, 4) else "no decompose state")
        return dict(n_entry=int(o[0]), n_over=int(o[1]), pool_top=int(o[2]))

    def debug_splice_pool(self, comp: int):
        """(used, room) of component `comp` (0-based) in the children-vector pool of the last `-s` pass's splice
        (povu_hip_debug_splice_pool)"""
        o = (C.c_uint32 * 2)()
        rc = self._lib.povu_hip_debug_splice_pool(self._ctx, comp, o)
        if rc != 0:
            raise RuntimeError("the last pass ran no inserting passes" if rc == 3 else
                               f"the last pass had no component {comp}" if rc == 5 else "no decompose state")
        return int(o[0]), int(o[1])

    def debug_stack(self, comp: int):
        n = C.c_uint32(0)
        if self._lib.povu_hip_debug_stack(self._ctx, comp, C.byref(n), None, None, None) != 0:
            raise RuntimeError("no decompose state")
        vtx = np.zeros(n.value, dtype=np.uint32)
        cls = np.zeros(n.value, dtype=np.uint32)
        ns = np.zeros(n.value, dtype=np.uint32)
        self._lib.povu_hip_debug_stack(self._ctx, comp, C.byref(n), vtx.ctypes.data, cls.ctypes.data, ns.ctypes.data)
        return dict(tree_vtx=vtx, cls=cls, next_seen=ns)


class MultiDecomposer:
    """One process, N GPUs (povu_hip_multi_*): one context and one host thread per device; the root device partitions, the
    shards travel over xGMI (RCCL), every GPU lands its PVST block in host memory over its own PCIe link."""

    def __init__(self, devices):
        self._lib = load_lib()
        if self._lib.povu_hip_device_count() <= 0:
            raise HipUnavailable("no HIP device visible: the decompose path has no CPU fallback")
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        err = C.create_string_buffer(512)
        self._h = self._lib.povu_hip_multi_create(devs, len(devices), err, 512)
        if not self._h:
            raise HipUnavailable(err.value.decode())
        self.world = len(devices)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.povu_hip_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def transport(self) -> str:
        return self._lib.povu_hip_multi_transport(self._h).decode()

    def upload(self, links, tips=None):
        vid = np.ascontiguousarray(links.vid, dtype=np.uint32)
        v1 = np.ascontiguousarray(links.v1, dtype=np.uint32)
        v2 = np.ascontiguousarray(links.v2, dtype=np.uint32)
        s1 = np.ascontiguousarray(links.s1, dtype=np.uint8)
        s2 = np.ascontiguousarray(links.s2, dtype=np.uint8)
        tp = None
        if tips is not None:
            tips = np.ascontiguousarray(tips, dtype=np.uint8)
            tp = tips.ctypes.data
        err = C.create_string_buffer(512)
        if self._lib.povu_hip_multi_upload(self._h, len(vid), vid.ctypes.data, len(v1), v1.ctypes.data, s1.ctypes.data,
                                           v2.ctypes.data, s2.ctypes.data, tp, err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def scatter(self, keep_graph: bool = True):
        err = C.create_string_buffer(512)
        if self._lib.povu_hip_multi_scatter(self._h, 1 if keep_graph else 0, err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def decompose(self, flags: int = 0) -> Forest:
        err = C.create_string_buffer(512)
        h = self._lib.povu_hip_multi_decompose(self._h, flags, None, None, err, 512)
        if not h:
            raise RuntimeError(err.value.decode())
        return Forest(self._lib, h)

    def rank_info(self, rank: int) -> dict:
        r = _MultiRank()
        if self._lib.povu_hip_multi_rank(self._h, rank, C.byref(r)) != 0:
            raise IndexError(rank)
        return {k: getattr(r, k) for k, _ in _MultiRank._fields_}

    def times(self) -> dict:
        t = (C.c_double * 6)()
        self._lib.povu_hip_multi_times(self._h, t)
        return dict(label_ms=t[0], lpt_ms=t[1], partition_ms=t[2], scatter_wall_ms=t[3], decompose_wall_ms=t[4], merge_ms=t[5])
