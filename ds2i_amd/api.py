"""ctypes binding of libds2i_hip.so + a Python mirror of ds2i's Index / query-operator concepts.

Names follow the reference (queries.hpp): and_query, or_query, ranked_and_query, wand_query,
maxscore_query, ranked_or_query; an operator is called as op(index, terms) and ranked operators
expose topk(), exactly like queries.cpp:13-62 drives them. Batched entry points take a list of
queries (the batch boundary this framework inserts at queries.cpp:26).
"""
import ctypes as C
import os

import numpy as np

CODECS = {"block_optpfor": 0, "block_varint": 1, "block_interpolative": 2, "block_qmx": 3, "block_mixed": 4, "opt": 5,
          "ef": 6, "single": 7, "uniform": 8}
FREQ_INDEX_KINDS = ["opt", "ef", "single", "uniform"]  # freq_index<...> layouts (index_types.hpp:18-32)
BLOCK_CODECS = ["block_optpfor", "block_varint", "block_interpolative", "block_qmx", "block_mixed"]
OPS = {"and": 0, "and_freq": 1, "or": 2, "or_freq": 3, "ranked_and": 4, "wand": 5, "maxscore": 6, "ranked_or": 7}
REFERENCE_ORDER = 0x100
NO_COUNTERS = 0x200  # run the kernels compiled without the statistics counters (stats then carry kernel_ms only)
# ranked operators: return the doc-id of every top-k score as well (score descending, equal scores by doc-id ascending; on a tie at
# the k-th place the smaller doc-ids); such a batch reports no counters
TOPK_DOCS = 0x400
_RANKED = {4, 5, 6, 7}

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class Ds2iError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ds2i_hip error %d: %s" % (code, msg))
        self.code = code


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("docs_blocks_decoded", C.c_uint64), ("freqs_blocks_decoded", C.c_uint64),
                ("block_max_examined", C.c_uint64), ("algorithmic_bytes", C.c_uint64), ("postings_scored", C.c_uint64),
                ("rounds", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class GroupStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("lists", C.c_uint32), ("units", C.c_uint32), ("queries", C.c_uint32), ("pipelined_stream", C.c_int)]


def _class_groups(fn, handle, cls):
    n = C.c_uint32()
    _check(fn(handle, cls, None, 0, C.byref(n)))
    arr = (GroupStats * max(1, n.value))()
    _check(fn(handle, cls, arr, n.value, C.byref(n)))
    return [{"kernel_ms": g.kernel_ms, "lists": g.lists, "units": g.units, "queries": g.queries, "pipelined_stream": bool(g.pipelined_stream)}
            for g in arr[:n.value]]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("num_docs", C.c_uint32), ("num_terms", C.c_uint32), ("zipf_exp", C.c_double),
                ("top_df_frac", C.c_double), ("min_len", C.c_uint32), ("clustered_every", C.c_uint32),
                ("topics", C.c_uint32), ("topic_boost", C.c_uint32)]  # correlated terms (0, 0: independent lists)


class VerifyReport(C.Structure):
    """ds2i_hip_verify_report (include/ds2i_hip.h)"""
    _fields_ = [("what", C.c_int), ("list", C.c_uint64), ("position", C.c_uint64), ("got", C.c_uint64), ("expected", C.c_uint64),
                ("postings_checked", C.c_uint64)]


VERIFY_WHAT = ("ok", "num_docs", "lists", "length", "docid", "freq")


def library_path():
    # DS2I_LIB_VARIANT=name loads a diagnostic / A-B build of the same library (ds2i_amd/build.py, DS2I_BUILD_VARIANT)
    variant = os.environ.get("DS2I_LIB_VARIANT", "")
    if variant:
        return os.path.join(_HERE, "..", "profiles", "tmp_libs", "lib_%s.so" % variant)
    return os.path.join(_HERE, "libds2i_hip.so")


def lib():
    """Loads the shared library; raises loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError("libds2i_hip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the query path)")
        L = C.CDLL(path)
        vp, u32p, u64p, fp = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        L.ds2i_hip_last_error.restype = C.c_char_p
        L.ds2i_hip_set_option.argtypes = [C.c_char_p, C.c_char_p]
        L.ds2i_hip_index_open.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
        L.ds2i_hip_index_close.argtypes = [vp]
        L.ds2i_hip_index_close.restype = None
        for f in ("ds2i_hip_index_size", "ds2i_hip_index_num_docs", "ds2i_hip_index_device_bytes"):
            getattr(L, f).argtypes = [vp]
            getattr(L, f).restype = C.c_uint64
        L.ds2i_hip_index_get_info.argtypes = [vp, vp]
        L.ds2i_hip_list_size.argtypes = [vp, C.c_uint32, u64p]
        L.ds2i_hip_decode_list.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint64, u64p]
        L.ds2i_hip_query_batch.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(Stats)]
        L.ds2i_hip_batch_prepare.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_uint32, C.c_int, C.POINTER(vp)]
        L.ds2i_hip_batch_run.argtypes = [vp, C.POINTER(Stats)]
        L.ds2i_hip_batch_class_stats.argtypes = [vp, C.c_int, C.POINTER(Stats), u32p]
        L.ds2i_hip_batch_phase_cycles.argtypes = [vp, C.c_int, vp, C.c_int]
        L.ds2i_hip_batch_class_groups.argtypes = [vp, C.c_int, vp, C.c_uint32, u32p]
        L.ds2i_hip_pipeline_class_groups.argtypes = [vp, C.c_int, vp, C.c_uint32, u32p]
        L.ds2i_hip_batch_fetch.argtypes = [vp, vp, vp, vp, vp]
        L.ds2i_hip_batch_match_total.argtypes = [vp, u64p]
        L.ds2i_hip_batch_fetch_matches.argtypes = [vp, vp, vp]
        L.ds2i_hip_batch_free.argtypes = [vp]
        L.ds2i_hip_batch_free.restype = None
        L.ds2i_hip_batch_set_instrumented.argtypes = [vp, C.c_int]
        L.ds2i_hip_pipeline_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
        L.ds2i_hip_pipeline_destroy.argtypes = [vp]
        L.ds2i_hip_pipeline_destroy.restype = None
        L.ds2i_hip_pipeline_submit.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_uint32, u64p]
        L.ds2i_hip_pipeline_wait.argtypes = [vp, C.c_uint64, vp, vp, vp, C.POINTER(Stats)]
        L.ds2i_hip_pipeline_wait_docs.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(Stats)]
        L.ds2i_hip_query_batch_docs.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(Stats)]
        L.ds2i_hip_batch_fetch_topk_docs.argtypes = [vp, vp]
        L.ds2i_hip_pipeline_set_instrumented.argtypes = [vp, C.c_int]
        L.ds2i_hip_pipeline_class_stats.argtypes = [vp, C.c_int, C.POINTER(Stats), u32p]
        L.ds2i_hip_batch_enable_block_profile.argtypes = [vp]
        L.ds2i_hip_batch_block_profile.argtypes = [vp, vp, C.c_uint64, u64p]
        L.ds2i_hybrid_default_model.argtypes = [vp]
        L.ds2i_hybrid_default_model.restype = None
        L.ds2i_hybrid_create.argtypes = [C.c_uint64, vp, C.POINTER(vp)]
        L.ds2i_hybrid_add_posting_list.argtypes = [vp, C.c_uint64, vp, vp, vp]
        L.ds2i_hybrid_analyse.argtypes = [vp, C.c_int, u64p, u64p]
        L.ds2i_hybrid_freeze.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(C.c_double), u64p,
                                         C.POINTER(C.c_double), u64p]
        L.ds2i_synth_build_hybrid.argtypes = [vp, C.c_int, vp, vp, C.c_double, C.POINTER(vp), C.POINTER(vp), u64p, u64p]
        L.ds2i_hybrid_hull.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, vp, C.c_uint32, u32p]
        L.ds2i_hip_hybrid_analyse.argtypes = [vp, C.c_int, u64p, u64p, C.POINTER(C.c_double)]
        L.ds2i_hip_hybrid_freeze.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_double), u64p,
                                             C.POINTER(C.c_double), u64p, C.POINTER(C.c_double)]
        L.ds2i_hybrid_free.argtypes = [vp]
        L.ds2i_hybrid_free.restype = None
        L.ds2i_hip_calibration_read.argtypes = [vp, u64p]
        L.ds2i_hip_list_block_weights.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
        L.ds2i_hip_list_range_table.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p, u32p, fp]
        L.ds2i_hip_selftest_scan.argtypes = [C.c_int, vp, vp, C.c_uint32]
        L.ds2i_hip_selftest_bm25.argtypes = [C.c_int, vp, vp, vp, C.c_uint32]
        L.ds2i_hip_synth_encode.argtypes = [C.c_int, C.POINTER(SynthParams), C.c_int, C.POINTER(vp), C.POINTER(vp), u64p,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ds2i_hip_encode_index.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_encode_host_seconds.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_encode_host_seconds.restype = None
        L.ds2i_hip_encode_index_with.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_uint32, C.POINTER(vp),
                                                 C.POINTER(C.c_double)]
        L.ds2i_hip_encode_plan_ms.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_encode_plan_ms.restype = None
        L.ds2i_hip_opt_partition.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(vp),
                                             C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_opt_partition.argtypes = [C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.ds2i_hip_build_wand.argtypes = [C.c_int, vp, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_build_collection.argtypes = [C.c_int, C.c_int, vp, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(vp),
                                                C.POINTER(C.c_double)]
        L.ds2i_hip_index_verify.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(VerifyReport), C.POINTER(C.c_double)]
        L.ds2i_hip_verify_collection.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, C.c_uint64, C.c_uint64, vp, vp, vp,
                                                 C.POINTER(VerifyReport), C.POINTER(C.c_double)]
        L.ds2i_hip_verify_host_seconds.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_verify_host_seconds.restype = None
        L.ds2i_hip_index_extract.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_uint64, u64p, C.POINTER(C.c_double)]
        L.ds2i_hip_extract_collection.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, u64p, u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                  C.POINTER(C.c_double)]
        L.ds2i_hip_convert_index.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_extract_host_seconds.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_extract_host_seconds.restype = None
        L.ds2i_check_doc_map.argtypes = [vp, C.c_uint64]
        L.ds2i_remap_postings.argtypes = [C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.c_int]
        L.ds2i_remap_wand.argtypes = [vp, C.c_size_t, vp, C.c_uint64, C.POINTER(vp)]
        L.ds2i_hip_remap_class_bounds.argtypes = [u32p]
        L.ds2i_hip_remap_class_bounds.restype = None
        L.ds2i_hip_remap_postings.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]
        L.ds2i_hip_remap_index.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_remap_ms.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_remap_ms.restype = None
        L.ds2i_merge_postings.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_int, u64p, u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.ds2i_hip_merge_postings.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint64, u64p, u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                              C.POINTER(C.c_double)]
        L.ds2i_hip_merge_indexes.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_merge_ms.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_merge_ms.restype = None
        L.ds2i_split_postings.argtypes = [C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.c_uint32, C.c_int, C.POINTER(vp)]
        L.ds2i_split_free.argtypes = [vp, C.c_uint32]
        L.ds2i_split_free.restype = None
        L.ds2i_hip_split_postings.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_split_index.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(vp),
                                           C.POINTER(C.c_double)]
        L.ds2i_hip_image_shape.argtypes = [C.c_int, vp, C.c_size_t, u64p, u64p]
        L.ds2i_hip_split_ms.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_split_ms.restype = None
        L.ds2i_hip_split_window.argtypes = []
        L.ds2i_hip_split_window.restype = C.c_uint32
        L.ds2i_hip_split_grid_waves.argtypes = [C.c_uint32]
        L.ds2i_hip_split_grid_waves.restype = C.c_uint32
        L.ds2i_hip_index_set_collection_stats.argtypes = [vp, C.c_uint64, vp, C.c_uint64]
        L.ds2i_split_wand.argtypes = [vp, C.c_size_t, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(vp)]
        L.ds2i_wand_arrays.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(vp)]
        L.ds2i_merge_topk.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_int]
        L.ds2i_hip_merge_topk.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(C.c_double)]
        L.ds2i_hip_merge_topk_grid.argtypes = [C.c_uint32, C.c_uint32]
        L.ds2i_hip_merge_topk_grid.restype = C.c_uint32
        L.ds2i_hip_shard_set_open.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.POINTER(vp)]
        L.ds2i_hip_shard_set_query.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
        L.ds2i_hip_shard_set_close.argtypes = [vp]
        L.ds2i_hip_shard_set_close.restype = None
        L.ds2i_invert_documents.argtypes = [C.c_uint64, vp, vp, C.c_uint64, C.c_int] + [C.POINTER(vp)] * 4
        L.ds2i_transpose_postings.argtypes = [C.c_uint64, C.c_uint64, vp, vp, vp, C.c_int] + [C.POINTER(vp)] * 3
        L.ds2i_hip_invert_postings.argtypes = [C.c_int, C.c_uint64, vp, vp, C.c_uint64] + [C.POINTER(vp)] * 4 + [C.POINTER(C.c_double)]
        L.ds2i_hip_transpose_postings.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp] + [C.POINTER(vp)] * 3 + [C.POINTER(C.c_double)]
        L.ds2i_hip_invert_documents.argtypes = [C.c_int, C.c_int, C.c_uint64, vp, vp, C.c_uint64] + [C.POINTER(vp)] * 4 + [C.POINTER(C.c_double)]
        L.ds2i_hip_forward_index.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, u64p, u64p] + [C.POINTER(vp)] * 3 + [C.POINTER(C.c_double)]
        L.ds2i_hip_invert_ms.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_invert_ms.restype = None
        L.ds2i_hip_invert_window.argtypes = []
        L.ds2i_hip_invert_window.restype = C.c_uint32
        L.ds2i_order_postings.argtypes = [C.c_uint64, C.c_uint64, vp, vp, vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
        L.ds2i_order_log_table.argtypes = [C.c_uint64, vp]
        L.ds2i_postings_cost.argtypes = [C.c_uint64, vp, vp, u64p]
        L.ds2i_order_clamp_gain.argtypes = [C.c_int64]
        L.ds2i_order_clamp_gain.restype = C.c_int32
        L.ds2i_hip_order_postings.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_order_index.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_double)]
        L.ds2i_hip_order_ms.argtypes = [C.POINTER(C.c_double)]
        L.ds2i_hip_order_ms.restype = None
        # build side
        L.ds2i_blob_data.argtypes = [vp]
        L.ds2i_blob_data.restype = vp
        L.ds2i_blob_size.argtypes = [vp]
        L.ds2i_blob_size.restype = C.c_size_t
        L.ds2i_blob_free.argtypes = [vp]
        L.ds2i_blob_free.restype = None
        L.ds2i_builder_create.argtypes = [C.c_int, C.c_uint64, C.POINTER(vp)]
        L.ds2i_builder_add_posting_list.argtypes = [vp, C.c_uint64, vp, vp]
        L.ds2i_builder_freeze.argtypes = [vp, C.POINTER(vp)]
        L.ds2i_builder_free.argtypes = [vp]
        L.ds2i_builder_free.restype = None
        L.ds2i_wand_create.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
        L.ds2i_wand_add_list.argtypes = [vp, C.c_uint64, vp, vp]
        L.ds2i_wand_freeze.argtypes = [vp, C.POINTER(vp)]
        L.ds2i_wand_free.argtypes = [vp]
        L.ds2i_wand_free.restype = None
        L.ds2i_encode_block.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.ds2i_encode_vbyte.argtypes = [C.c_uint32, C.POINTER(vp)]
        L.ds2i_write_sequence.argtypes = [C.c_int, vp, C.c_uint64, C.c_uint64, vp, C.POINTER(vp), u64p]
        L.ds2i_encode_posting_list.argtypes = [C.c_int, C.c_uint32, vp, vp, C.POINTER(vp)]
        L.ds2i_opt_list_directory.argtypes = [vp, C.c_size_t, C.c_uint32, C.POINTER(vp), C.POINTER(vp), u64p]
        L.ds2i_freq_list_directory.argtypes = [C.c_int, vp, C.c_size_t, C.c_uint32, C.POINTER(vp), C.POINTER(vp), u64p]
        L.ds2i_synth_list_upper_bound.argtypes = [C.POINTER(SynthParams), C.c_uint32]
        L.ds2i_synth_list_upper_bound.restype = C.c_uint64
        L.ds2i_synth_list.argtypes = [C.POINTER(SynthParams), C.c_uint32, vp, vp, C.c_uint64, u64p]
        L.ds2i_synth_doc_sizes.argtypes = [C.POINTER(SynthParams), vp]
        L.ds2i_synth_queries.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]
        L.ds2i_synth_queries_topical.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]
        L.ds2i_synth_build.argtypes = [C.POINTER(SynthParams), C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), u64p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise Ds2iError(rc, lib().ds2i_hip_last_error().decode("utf-8", "replace"))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _take_blob(handle):
    L = lib()
    n = L.ds2i_blob_size(handle)
    # (c_char * n).raw handles images > 2 GiB (string_at takes a C int size)
    out = (C.c_char * n).from_address(L.ds2i_blob_data(handle)).raw if n else b""
    L.ds2i_blob_free(handle)
    return out


def _codec(c):
    return CODECS[c] if isinstance(c, str) else int(c)


# ---------------------------------------------------------------- build side (host, CPU)
def encode_block(codec, values, sum_of_values=0xFFFFFFFF):
    v = _u32(values)
    h = C.c_void_p()
    _check(lib().ds2i_encode_block(_codec(codec), _ptr(v), C.c_uint32(sum_of_values & 0xFFFFFFFF), len(v), C.byref(h)))
    return _take_blob(h)


def encode_vbyte(value):
    h = C.c_void_p()
    _check(lib().ds2i_encode_vbyte(value, C.byref(h)))
    return _take_blob(h)


SEQUENCE_KINDS = ("elias_fano", "ranked_bitvector", "indexed", "strict", "partitioned_indexed", "partitioned_strict",
                  "uniform_indexed", "uniform_strict")


def write_sequence(seq_kind, values, universe, params=None):
    """One sequence of the Elias-Fano family written into a fresh bit string (ds2i_write_sequence).
    Returns (u64 words, nbits). params = (ef_log_sampling0, ef_log_sampling1, rb_log_rank1_sampling,
    rb_log_sampling1, log_partition_size) or None for global_parameters' defaults."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    h = C.c_void_p()
    nbits = C.c_uint64()
    pp = None
    if params is not None:
        pp = np.asarray(params, dtype=np.uint8)
        assert pp.shape == (5,)
    _check(lib().ds2i_write_sequence(SEQUENCE_KINDS.index(seq_kind), _ptr(v), len(v), int(universe),
                                     _ptr(pp) if pp is not None else None, C.byref(h), C.byref(nbits)))
    return np.frombuffer(_take_blob(h), dtype=np.uint64), int(nbits.value)


def encode_posting_list(codec, docs, freqs):
    d, f = _u32(docs), _u32(freqs)
    h = C.c_void_p()
    _check(lib().ds2i_encode_posting_list(_codec(codec), len(d), _ptr(d), _ptr(f), C.byref(h)))
    return _take_blob(h)


def build_index(codec, num_docs, lists):
    """lists: iterable of (docs, freqs). Returns the frozen block_freq_index image (bytes)."""
    L = lib()
    b = C.c_void_p()
    _check(L.ds2i_builder_create(_codec(codec), num_docs, C.byref(b)))
    try:
        for docs, freqs in lists:
            d, f = _u32(docs), _u32(freqs)
            _check(L.ds2i_builder_add_posting_list(b, len(d), _ptr(d), _ptr(f)))
        h = C.c_void_p()
        _check(L.ds2i_builder_freeze(b, C.byref(h)))
        return _take_blob(h)
    finally:
        L.ds2i_builder_free(b)


def _csr(lists):
    """(number of lists, offsets uint64[n + 1], docs, freqs) -- the form posting lists cross the C ABI in"""
    lists = [(_u32(dd), _u32(ff)) for dd, ff in lists]
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    for i, (dd, _) in enumerate(lists):
        offs[i + 1] = offs[i] + len(dd)
    docs = np.concatenate([dd for dd, _ in lists]) if lists else np.zeros(1, np.uint32)
    freqs = np.concatenate([ff for _, ff in lists]) if lists else np.zeros(1, np.uint32)
    return len(lists), offs, docs, freqs


ENCODE_PLANS = {None: 0, "host": 1, "device": 2}  # DS2I_ENCODE_PLAN_* of ds2i_hip.h


def gpu_encode_index(num_docs, lists, device=0, codec="block_optpfor", plan=None):
    """The index image of `lists` (iterable of (docs, freqs)) encoded ON THE GPU (ds2i_hip_encode_index_with): byte-identical
    to build_index(codec, num_docs, lists). codec: "block_optpfor", "block_varint", "block_interpolative", or one of the
    Elias-Fano layouts "opt", "ef", "single", "uniform" (default global_parameters; doc-ids strictly increasing and
    < num_docs, freqs >= 1, checked on the host). plan: who plans the partitions of "opt" -- "host", "device" (the partition
    DP as HIP kernels) or None for the library's default; the image is the same, and the other codecs ignore it.
    Returns (image bytes, device milliseconds of the kernels)."""
    n, offs, docs, freqs = _csr(lists)
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_encode_index_with(device, _codec(codec), num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), ENCODE_PLANS[plan],
                                            C.byref(h), C.byref(ms)))
    return _take_blob(h), ms.value


def encode_plan_ms():
    """hipEvent milliseconds of the partition kernels in this thread's last GPU encode call (ds2i_hip_encode_plan_ms): 0.0 when the
    host planned or the codec has no partition DP."""
    ms = C.c_double()
    lib().ds2i_hip_encode_plan_ms(C.byref(ms))
    return ms.value


def _take_partitions(hs):
    de, do, fe, fo = (np.frombuffer(_take_blob(h), dtype=t) for h, t in zip(hs, (np.uint32, np.uint64, np.uint32, np.uint64)))
    return de, do, fe, fo


def opt_partition(num_docs, lists):
    """The partition end points the "opt" builder chooses for every list, planned ON THE HOST (ds2i_opt_partition): per side (docs:
    the doc-ids; freqs: the strict prefix sums of the freqs) the exclusive end index of every partition of every list back to back
    and len(lists) + 1 offsets into them. Returns (docs_ends uint32, docs_offs uint64, freqs_ends uint32, freqs_offs uint64)."""
    n, offs, docs, freqs = _csr(lists)
    hs = [C.c_void_p() for _ in range(4)]
    _check(lib().ds2i_opt_partition(num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), *[C.byref(h) for h in hs]))
    return _take_partitions(hs)


def gpu_opt_partition(num_docs, lists, device=0, scratch_bytes=0):
    """opt_partition planned ON THE GPU (ds2i_hip_opt_partition): the same four arrays, element for element. scratch_bytes: the DP
    scratch one group of consecutive lists may take (12 bytes per posting and side; 0 = the library's default)."""
    n, offs, docs, freqs = _csr(lists)
    hs = [C.c_void_p() for _ in range(4)]
    _check(lib().ds2i_hip_opt_partition(device, num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), scratch_bytes, *[C.byref(h) for h in hs],
                                        None))
    return _take_partitions(hs)


def gpu_build_wand(doc_sizes, lists, device=0):
    """The wand_data image of `lists` over documents of `doc_sizes` built ON THE GPU (ds2i_hip_build_wand): byte-identical
    to build_wand(doc_sizes, lists). Returns (image bytes, dict(device_ms))."""
    s = _u32(doc_sizes)
    n, offs, docs, freqs = _csr(lists)
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_build_wand(device, _ptr(s), len(s), n, _ptr(offs), _ptr(docs), _ptr(freqs), C.byref(h), C.byref(ms)))
    return _take_blob(h), {"device_ms": ms.value}


def gpu_build_collection(num_docs, doc_sizes, lists, codec="block_optpfor", device=0):
    """Index image and wand_data image of one collection from ONE staging on the GPU (ds2i_hip_build_collection): what
    gpu_encode_index and gpu_build_wand return, everything Index(codec, index, wand) needs. codec: as gpu_encode_index
    (the block codecs and "opt", "ef", "single", "uniform").
    Returns (index image, wand image, dict(device_ms))."""
    s = _u32(doc_sizes)
    if len(s) != num_docs:
        raise ValueError("doc_sizes holds %d lengths for %d documents" % (len(s), num_docs))
    n, offs, docs, freqs = _csr(lists)
    hi, hw, ms = C.c_void_p(), C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_build_collection(device, _codec(codec), _ptr(s), num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs),
                                           C.byref(hi), C.byref(hw), C.byref(ms)))
    return _take_blob(hi), _take_blob(hw), {"device_ms": ms.value}


def _verify_result(r, ms):
    return dict(ok=r.what == 0, what=VERIFY_WHAT[r.what], list=r.list, position=r.position, got=r.got, expected=r.expected,
                postings_checked=r.postings_checked, device_ms=ms.value)


def gpu_verify_collection(kind, image, num_docs, lists, device=0):
    """An index image checked against the collection it was built from, ON THE GPU (ds2i_hip_verify_collection): every list
    decoded by the on-disk decoders of `kind` in one launch and compared with `lists` (iterable of (docs, freqs)).
    Returns dict(ok, what, list, position, got, expected, postings_checked, device_ms); what is "ok" or names the first
    difference: "num_docs", "lists", "length" (these three are found on the host), "docid", "freq"."""
    n, offs, docs, freqs = _csr(lists)
    r, ms = VerifyReport(), C.c_double()
    _check(lib().ds2i_hip_verify_collection(device, _codec(kind), image, len(image), num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs),
                                            C.byref(r), C.byref(ms)))
    return _verify_result(r, ms)


def gpu_extract_collection(kind, image, device=0):
    """The collection an index image holds, decoded ON THE GPU in one launch (ds2i_hip_extract_collection): a bare upload of the
    image and the on-disk decoders of `kind` (any of the nine). List t is docs[offsets[t]:offsets[t + 1]] with the freqs beside
    it. Returns (num_docs, offsets uint64[lists + 1], docs uint32, freqs uint32, dict(device_ms)). An index holds no document
    sizes: they do not come back."""
    n, v, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    ho, hd, hf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(lib().ds2i_hip_extract_collection(device, _codec(kind), image, len(image), C.byref(n), C.byref(v), C.byref(ho), C.byref(hd),
                                             C.byref(hf), C.byref(ms)))
    offs, docs, freqs = (np.frombuffer(_take_blob(h), dtype=t) for h, t in ((ho, np.uint64), (hd, np.uint32), (hf, np.uint32)))
    return n.value, offs, docs, freqs, {"device_ms": ms.value}


def gpu_convert_index(from_kind, image, to_kind, device=0):
    """An index image of `from_kind` (any of the nine) as an image of `to_kind` (a kind gpu_encode_index writes), ON THE GPU
    (ds2i_hip_convert_index): extracted in one launch and encoded where the postings lie; byte-identical to
    build_index(to_kind, ...) over the same lists. Returns (image bytes, dict(device_ms))."""
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_convert_index(device, _codec(from_kind), image, len(image), _codec(to_kind), C.byref(h), C.byref(ms)))
    return _take_blob(h), {"device_ms": ms.value}


def check_doc_map(doc_map, num_docs=None):
    """Raises Ds2iError (-1) naming the first offending old doc-id unless `doc_map` is a permutation of [0, num_docs)
    (ds2i_check_doc_map; num_docs=None: of its own length)."""
    m = _u32(doc_map)
    _check(lib().ds2i_check_doc_map(_ptr(m), len(m) if num_docs is None else num_docs))


def _split(lists, offs, docs, freqs):
    return [(docs[int(offs[t]):int(offs[t + 1])], freqs[int(offs[t]):int(offs[t + 1])]) for t in range(len(lists))]


def remap_postings(num_docs, lists, doc_map, threads=0):
    """`lists` (iterable of (docs, freqs)) with the documents renumbered ON THE HOST (ds2i_remap_postings): new doc-id =
    doc_map[old doc-id], every list sorted again by its new doc-ids with its freqs. The host twin of gpu_remap_postings.
    Returns the new lists, in the same order."""
    lists = list(lists)
    m = _u32(doc_map)
    if len(m) != num_docs:
        raise ValueError("doc_map holds %d entries for %d documents" % (len(m), num_docs))
    n, offs, docs, freqs = _csr(lists)
    docs, freqs = docs.copy(), freqs.copy()
    _check(lib().ds2i_remap_postings(num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), _ptr(m), threads))
    return _split(lists, offs, docs, freqs)


def remap_class_bounds():
    """(W, L, T) as compiled (ds2i_hip_remap_class_bounds): gpu_remap_postings sorts a list of up to W postings in one wavefront, one
    of up to L in one workgroup, and the longer ones together in tiles of T postings."""
    b = (C.c_uint32 * 3)()
    lib().ds2i_hip_remap_class_bounds(b)
    return tuple(b)


def _remap_info(ms):
    parts = (C.c_double * 6)()
    lib().ds2i_hip_remap_ms(parts)
    return {"device_ms": ms.value, "map_ms": parts[0], "sort_ms": (parts[1], parts[2], parts[3]), "extract_ms": parts[4],
            "encode_ms": parts[5]}


def gpu_remap_postings(num_docs, lists, doc_map, device=0):
    """remap_postings ON THE GPU (ds2i_hip_remap_postings): a map kernel and a segmented sort in three classes by list length; the
    same lists, element for element. Returns (new lists, dict(device_ms, map_ms, sort_ms per class, ...))."""
    lists = list(lists)
    m = _u32(doc_map)
    if len(m) != num_docs:
        raise ValueError("doc_map holds %d entries for %d documents" % (len(m), num_docs))
    n, offs, docs, freqs = _csr(lists)
    od, of, ms = np.empty_like(docs), np.empty_like(freqs), C.c_double()
    _check(lib().ds2i_hip_remap_postings(device, num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), _ptr(m), _ptr(od), _ptr(of), C.byref(ms)))
    return _split(lists, offs, od, of), _remap_info(ms)


def gpu_remap_index(kind, image, doc_map, to_kind=None, device=0):
    """An index image of `kind` (any of the nine) as the image of `to_kind` (a kind gpu_encode_index writes; None: `kind`) of the
    collection with its documents renumbered, ON THE GPU (ds2i_hip_remap_index): extracted, mapped, sorted and encoded where the
    postings lie; byte-identical to build_index(to_kind, ...) over remap_postings' lists. An index holds no wand data: remap_wand
    renumbers that. Returns (image bytes, dict(device_ms, extract_ms, map_ms, sort_ms per class, encode_ms))."""
    m = _u32(doc_map)
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_remap_index(device, _codec(kind), image, len(image), _ptr(m), len(m), _codec(kind if to_kind is None else to_kind),
                                      C.byref(h), C.byref(ms)))
    return _take_blob(h), _remap_info(ms)


def remap_wand(wand_image, doc_map):
    """The wand_data image of the collection with its documents renumbered (ds2i_remap_wand): norm_lens permuted, max_term_weight
    copied, no pass over the postings; byte-identical to build_wand over the renumbered collection."""
    m = _u32(doc_map)
    h = C.c_void_p()
    _check(lib().ds2i_remap_wand(wand_image, len(wand_image), _ptr(m), len(m), C.byref(h)))
    return _take_blob(h)


class MergeSource(C.Structure):
    """ds2i_merge_source (include/ds2i_hip.h)"""
    _fields_ = [("kind", C.c_int), ("image", C.c_void_p), ("bytes", C.c_size_t), ("doc_map", C.c_void_p), ("map_len", C.c_uint64),
                ("term_map", C.c_void_p), ("terms_len", C.c_uint64)]


class MergePostingsSource(C.Structure):
    """ds2i_merge_postings_source (include/ds2i_build.h)"""
    _fields_ = [("num_docs", C.c_uint64), ("nlists", C.c_uint64), ("list_offsets", C.c_void_p), ("docs", C.c_void_p), ("freqs", C.c_void_p),
                ("doc_map", C.c_void_p), ("map_len", C.c_uint64), ("term_map", C.c_void_p), ("terms_len", C.c_uint64)]


def _merge_maps(src, rest, keep):
    """fills the map fields of one source from its optional (doc_map, term_map); `keep` holds the arrays while the call runs"""
    maps = [None if m is None else _u32(m) for m in rest] + [None, None]
    keep.extend(maps[:2])
    for name, length, m in (("doc_map", "map_len", maps[0]), ("term_map", "terms_len", maps[1])):
        setattr(src, name, None if m is None else m.ctypes.data)
        setattr(src, length, 0 if m is None else len(m))


def _merge_postings_sources(sources):
    """sources: iterable of (num_docs, lists[, doc_map[, term_map]]) -> (array of MergePostingsSource, what it points into)"""
    sources = list(sources)
    arr, keep = (MergePostingsSource * max(1, len(sources)))(), []
    for src, (num_docs, lists, *rest) in zip(arr, sources):
        n, offs, docs, freqs = _csr(lists)
        keep.extend((offs, docs, freqs))
        src.num_docs, src.nlists, src.list_offsets, src.docs, src.freqs = num_docs, n, offs.ctypes.data, docs.ctypes.data, freqs.ctypes.data
        _merge_maps(src, rest, keep)
    return arr, len(sources), keep


def _take_merged(n, v, ho, hd, hf):
    offs, docs, freqs = (np.frombuffer(_take_blob(h), dtype=t) for h, t in ((ho, np.uint64), (hd, np.uint32), (hf, np.uint32)))
    return n.value, [(docs[int(offs[t]):int(offs[t + 1])], freqs[int(offs[t]):int(offs[t + 1])]) for t in range(v.value)]


def merge_postings(sources, num_terms=None, threads=0):
    """Collections merged into one ON THE HOST (ds2i_merge_postings), the host twin of gpu_merge_postings. sources: iterable of
    (num_docs, lists[, doc_map[, term_map]]); doc_map gives the merged doc-id of each of the source's documents (None: after the
    documents of the earlier sources; all maps together a permutation of all documents), term_map the merged term of each of its lists
    (strictly increasing; None: the same term). num_terms: the merged number of lists (None: the smallest that holds every mapped
    term); every term must receive a list. Returns (num_docs, merged lists): each the union of the mapped postings sent to its term,
    sorted by doc-id with the freqs."""
    arr, nsrc, keep = _merge_postings_sources(sources)
    n, v = C.c_uint64(), C.c_uint64()
    ho, hd, hf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(lib().ds2i_merge_postings(arr, nsrc, num_terms or 0, threads, C.byref(n), C.byref(v), C.byref(ho), C.byref(hd), C.byref(hf)))
    return _take_merged(n, v, ho, hd, hf)


def _merge_info(ms):
    parts = (C.c_double * 8)()
    lib().ds2i_hip_merge_ms(parts)
    return {"device_ms": ms.value, "extract_ms": parts[0], "place_ms": parts[1], "sort_ms": parts[2], "encode_ms": parts[3]}


def gpu_merge_postings(sources, num_terms=None, device=0):
    """merge_postings ON THE GPU (ds2i_hip_merge_postings): every source copied up and placed among the merged postings by one kernel,
    then, unless the doc maps together are the identity, the segmented sort of gpu_remap_postings; the same lists, element for element.
    Returns (num_docs, merged lists, dict(device_ms, place_ms, sort_ms, ...))."""
    arr, nsrc, keep = _merge_postings_sources(sources)
    n, v, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    ho, hd, hf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(lib().ds2i_hip_merge_postings(device, arr, nsrc, num_terms or 0, C.byref(n), C.byref(v), C.byref(ho), C.byref(hd), C.byref(hf),
                                         C.byref(ms)))
    return _take_merged(n, v, ho, hd, hf) + (_merge_info(ms),)


def gpu_merge_indexes(sources, to_kind, num_terms=None, device=0):
    """Index images merged into one image of `to_kind` (a kind gpu_encode_index writes) ON THE GPU (ds2i_hip_merge_indexes). sources:
    iterable of (kind, image[, doc_map[, term_map]]), each of any of the nine kinds, the maps as merge_postings takes them. Every source
    in turn is extracted, placed among the merged postings and freed; the merged lists are sorted unless the doc maps together are the
    identity, and encoded where they lie: byte-identical to build_index(to_kind, ...) over merge_postings' lists. An index holds no
    wand data and none is merged: build it from the merged document sizes (gpu_build_wand).
    Returns (image bytes, dict(device_ms, extract_ms, place_ms, sort_ms, encode_ms))."""
    sources = list(sources)
    arr, keep = (MergeSource * max(1, len(sources)))(), []
    for src, (kind, image, *rest) in zip(arr, sources):
        keep.append(image)
        src.kind, src.image, src.bytes = _codec(kind), C.cast(C.c_char_p(image), C.c_void_p), len(image)
        _merge_maps(src, rest, keep)
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_merge_indexes(device, arr, len(sources), num_terms or 0, _codec(to_kind), C.byref(h), C.byref(ms)))
    return _take_blob(h), _merge_info(ms)


DROP = 0xFFFFFFFF  # DS2I_SPLIT_DROP (include/ds2i_build.h): the shard_of value that deletes a document


class SplitShard(C.Structure):
    """ds2i_split_shard (include/ds2i_build.h)"""
    _fields_ = [("num_docs", C.c_uint64), ("nlists", C.c_uint64), ("doc_map", C.c_void_p), ("term_map", C.c_void_p),
                ("list_offsets", C.c_void_p), ("docs", C.c_void_p), ("freqs", C.c_void_p), ("image", C.c_void_p)]


def _shard_of(shard_of, nshards):
    """(shard_of as uint32, nshards; None: the largest shard number plus one)"""
    m = _u32(shard_of)
    if nshards is None:
        live = m[m != DROP]
        nshards = int(live.max()) + 1 if len(live) else 1
    return m, nshards


def _copy_blob(handle, dtype=None):
    """a blob's bytes (or array); the blob stays its owner's"""
    L = lib()
    n = L.ds2i_blob_size(handle)
    raw = (C.c_char * n).from_address(L.ds2i_blob_data(handle)).raw if n else b""
    return raw if dtype is None else np.frombuffer(raw, dtype=dtype)


def _take_shards(handle, nshards, images):
    """the shards of a ds2i_split_shard array as tuples, the array freed"""
    try:
        arr = C.cast(handle, C.POINTER(SplitShard))
        out = []
        for s in range(nshards):
            sh = arr[s]
            maps = (_copy_blob(sh.doc_map, np.uint32), _copy_blob(sh.term_map, np.uint32))
            if images:
                out.append((_copy_blob(sh.image),) + maps)
                continue
            offs, docs, freqs = (_copy_blob(h, t) for h, t in ((sh.list_offsets, np.uint64), (sh.docs, np.uint32), (sh.freqs, np.uint32)))
            lists = [(docs[int(offs[t]):int(offs[t + 1])], freqs[int(offs[t]):int(offs[t + 1])]) for t in range(sh.nlists)]
            out.append((int(sh.num_docs), lists) + maps)
        return out
    finally:
        lib().ds2i_split_free(handle, nshards)


def image_shape(kind, image):
    """(num_docs, number of lists) of an index image from its host parse alone (ds2i_hip_image_shape): no device is needed"""
    n, v = C.c_uint64(), C.c_uint64()
    _check(lib().ds2i_hip_image_shape(_codec(kind), image, len(image), C.byref(n), C.byref(v)))
    return n.value, v.value


def split_window():
    """the postings of one window of the device split as compiled (ds2i_hip_split_window): a wavefront takes a window at a time"""
    return lib().ds2i_hip_split_window()


def split_grid_waves(compute_units):
    """the most wavefronts one launch of the device split has on a device of that many compute units (ds2i_hip_split_grid_waves); they
    stride over the windows"""
    return lib().ds2i_hip_split_grid_waves(compute_units)


def split_postings(num_docs, lists, shard_of, nshards=None, threads=0):
    """A collection cut into shards by documents ON THE HOST (ds2i_split_postings), the inverse of merge_postings and the host twin of
    gpu_split_postings. shard_of[d] is the shard of document d, or DROP to delete it; nshards=None: the largest shard number plus one.
    The documents of a shard keep their order (local id = rank among them), lists with no posting in a shard are dropped from it, and
    nothing is sorted. Returns a list of (num_docs, lists, doc_map, term_map), one per shard: what merge_postings takes as sources.
    doc_map gives the old id of every local document, term_map the old term of every list. Wand data is not split: build a shard's from
    sizes[doc_map] (gpu_build_wand); scores over a shard use the shard's own statistics."""
    m, nshards = _shard_of(shard_of, nshards)
    if len(m) != num_docs:
        raise ValueError("shard_of holds %d entries for %d documents" % (len(m), num_docs))
    n, offs, docs, freqs = _csr(lists)
    h = C.c_void_p()
    _check(lib().ds2i_split_postings(num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), _ptr(m), nshards, threads, C.byref(h)))
    return _take_shards(h, nshards, False)


def _split_info(ms):
    parts = (C.c_double * 8)()
    lib().ds2i_hip_split_ms(parts)
    return {"device_ms": ms.value, "extract_ms": parts[0], "count_ms": parts[1], "offsets_ms": parts[2], "scatter_ms": parts[3],
            "encode_ms": parts[4]}


def gpu_split_postings(num_docs, lists, shard_of, nshards=None, device=0):
    """split_postings ON THE GPU (ds2i_hip_split_postings): the collection copied up once, then per shard a count kernel, the scan of
    the window counts on the host, a scatter kernel and an offsets kernel; the same shards, element for element.
    Returns ([(num_docs, lists, doc_map, term_map), ...], dict(device_ms, count_ms, offsets_ms, scatter_ms, ...))."""
    m, nshards = _shard_of(shard_of, nshards)
    if len(m) != num_docs:
        raise ValueError("shard_of holds %d entries for %d documents" % (len(m), num_docs))
    n, offs, docs, freqs = _csr(lists)
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_split_postings(device, num_docs, n, _ptr(offs), _ptr(docs), _ptr(freqs), _ptr(m), nshards, C.byref(h), C.byref(ms)))
    return _take_shards(h, nshards, False), _split_info(ms)


def gpu_split_index(kind, image, shard_of, nshards=None, to_kind=None, device=0):
    """An index image of `kind` (any of the nine) cut into shards by documents ON THE GPU (ds2i_hip_split_index), each an image of
    `to_kind` (a kind gpu_encode_index writes; None: `kind`): extracted once, every shard in turn compacted out of the postings and
    encoded where it lies; every image byte-identical to build_index(to_kind, ...) over split_postings' lists. Every shard must be
    assigned a document and receive a posting. Returns ([(image, doc_map, term_map), ...], dict(device_ms, extract_ms, count_ms,
    offsets_ms, scatter_ms, encode_ms)): with the kind in front, what gpu_merge_indexes takes as sources. An index holds no wand data
    and none is split: build a shard's from sizes[doc_map] (gpu_build_wand)."""
    m, nshards = _shard_of(shard_of, nshards)
    h, ms = C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_split_index(device, _codec(kind), image, len(image), _ptr(m), len(m), nshards,
                                      _codec(kind if to_kind is None else to_kind), C.byref(h), C.byref(ms)))
    return _take_shards(h, nshards, True), _split_info(ms)


MAX_SHARDS = 64  # DS2I_HIP_MAX_SHARDS (include/ds2i_hip.h)


def split_wand(wand_image, doc_map, term_map):
    """A shard's wand_data image under the COLLECTION's normalisation (ds2i_split_wand): norm_lens gathered through doc_map,
    max_term_weight through term_map (the maps of split_postings / gpu_split_index), no pass over the postings. It is not the image
    build_wand gives over the shard: that one divides by the shard's own average document length."""
    dm, tm = _u32(doc_map), _u32(term_map)
    h = C.c_void_p()
    _check(lib().ds2i_split_wand(wand_image, len(wand_image), _ptr(dm), len(dm), _ptr(tm), len(tm), C.byref(h)))
    return _take_blob(h)


def wand_arrays(wand_image):
    """(norm_lens float32[num_docs], max_term_weight float32[terms]) of a wand_data image (ds2i_wand_arrays)"""
    a, b = C.c_void_p(), C.c_void_p()
    _check(lib().ds2i_wand_arrays(wand_image, len(wand_image), C.byref(a), C.byref(b)))
    return np.frombuffer(_take_blob(a), dtype=np.float32), np.frombuffer(_take_blob(b), dtype=np.float32)


class TopkRows(C.Structure):
    """ds2i_topk_rows (include/ds2i_build.h)"""
    _fields_ = [("scores", C.c_void_p), ("docs", C.c_void_p), ("lens", C.c_void_p), ("doc_map", C.c_void_p), ("map_len", C.c_uint64)]


def _topk_rows(rows, k):
    """rows: iterable of (scores float32[nq, k], docs uint32[nq, k], lens uint32[nq][, doc_map]) -> (array of TopkRows, nq, k, what it
    points into)"""
    rows = list(rows)
    arr, keep, nq = (TopkRows * max(1, len(rows)))(), [], None
    for dst, (scores, docs, lens, *rest) in zip(arr, rows):
        s = np.ascontiguousarray(scores, dtype=np.float32)
        dd, ll = _u32(docs), _u32(lens)
        if k is None:
            k = s.shape[1] if s.ndim == 2 else 0
        nq = len(ll) if nq is None else nq
        if len(ll) != nq or s.size != nq * k or dd.size != nq * k:
            raise ValueError("every row set holds nq lengths and nq * k scores and docs")
        m = _u32(rest[0]) if rest and rest[0] is not None else None
        keep.extend((s, dd, ll, m))
        dst.scores, dst.docs, dst.lens = s.ctypes.data, dd.ctypes.data, ll.ctypes.data
        dst.doc_map, dst.map_len = (None, 0) if m is None else (m.ctypes.data, len(m))
    return arr, len(rows), nq or 0, k or 0, keep


def _merge_out(nq, k):
    return (np.full((nq, max(k, 1)), -np.inf, dtype=np.float32), np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32),
            np.zeros(max(nq, 1), dtype=np.uint32))


def merge_topk(rows, k=None, threads=0):
    """The top-k rows several shards answered for the same queries merged ON THE HOST into the rows of the whole collection
    (ds2i_merge_topk), the host twin of gpu_merge_topk. rows: iterable of (scores[nq, k], docs[nq, k], lens[nq][, doc_map]); doc_map
    gives the collection doc-id of every local id (None: the ids are the collection's). Score descending, equal scores by collection
    doc-id ascending, the smaller ids on a tie at the k-th place. Returns (scores float32[nq, k], docs uint32[nq, k], lens uint32[nq])."""
    arr, n, nq, k, keep = _topk_rows(rows, k)
    s, dd, ll = _merge_out(nq, k)
    _check(lib().ds2i_merge_topk(arr, n, nq, k, _ptr(s), _ptr(dd), _ptr(ll), threads))
    return s[:, :k], dd[:, :k], ll[:nq]


def gpu_merge_topk(rows, k=None, device=0):
    """merge_topk ON THE GPU (ds2i_hip_merge_topk): one wavefront per query folds the row sets into a best-k buffer in LDS; the same
    rows, element for element. Returns (scores, docs, lens, dict(device_ms))."""
    arr, n, nq, k, keep = _topk_rows(rows, k)
    s, dd, ll = _merge_out(nq, k)
    ms = C.c_double()
    _check(lib().ds2i_hip_merge_topk(device, arr, n, nq, k, _ptr(s), _ptr(dd), _ptr(ll), C.byref(ms)))
    return s[:, :k], dd[:, :k], ll[:nq], {"device_ms": ms.value}


def merge_topk_grid(compute_units, k):
    """the most workgroups (one wavefront each, a query at a time) a launch of the device merge at that k has on a device of that many
    compute units (ds2i_hip_merge_topk_grid): what the units' LDS and wavefront slots hold; they stride over the queries"""
    return lib().ds2i_hip_merge_topk_grid(compute_units, k)


def invert_window():
    """the tokens of one window of the device inversion as compiled (ds2i_hip_invert_window): a wavefront takes a window at a time"""
    return lib().ds2i_hip_invert_window()


def _forward(docs):
    """documents as a list of u32 arrays, or as (doc_offsets, tokens) -> (num_docs, doc_offsets uint64[num_docs + 1], tokens uint32)"""
    if isinstance(docs, tuple) and len(docs) == 2:
        offs, tokens = np.ascontiguousarray(docs[0], dtype=np.uint64), _u32(docs[1])
    else:
        docs = [_u32(d) for d in docs]
        offs = np.zeros(len(docs) + 1, dtype=np.uint64)
        if docs:
            offs[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
        tokens = np.concatenate(docs) if docs else np.zeros(0, np.uint32)
    if len(offs) < 1:
        raise ValueError("doc_offsets holds no value")
    if len(tokens) < int(offs.max()):
        raise ValueError("doc_offsets reach %d, past the %d tokens" % (int(offs.max()), len(tokens)))
    if not len(tokens):
        tokens = np.zeros(1, np.uint32)  # (a pointer the library may check against NULL)
    return len(offs) - 1, offs, tokens


def _take_csr(handles):
    """(offsets uint64, ids uint32, values uint32[, more uint32 arrays]) of the blobs a CSR result comes back in"""
    return tuple(np.frombuffer(_take_blob(h), dtype=np.uint64 if i == 0 else np.uint32) for i, h in enumerate(handles))


def invert_documents(docs, nterms, threads=0):
    """Documents inverted into posting lists ON THE HOST (ds2i_invert_documents), the host twin of gpu_invert_postings. docs: a list of
    uint32 arrays of term ids < nterms (in any order, with repeats; empty documents are allowed), or (doc_offsets, tokens). Returns
    (list_offsets uint64[nterms + 1], docs uint32, freqs uint32, doc_sizes uint32[num_docs]): list t holds the documents in which term
    t occurs, strictly increasing, freq = its count in the document; terms that never occur have empty lists; doc_sizes are the token
    counts."""
    n, offs, tokens = _forward(docs)
    h = [C.c_void_p() for _ in range(4)]
    _check(lib().ds2i_invert_documents(n, _ptr(offs), _ptr(tokens), nterms, threads, *[C.byref(x) for x in h]))
    return _take_csr(h)


def transpose_postings(nrows, ncols, row_offsets, cols, vals, threads=0):
    """A CSR matrix (column ids strictly increasing within every row and < ncols, one uint32 value per entry) transposed ON THE HOST
    (ds2i_transpose_postings), the host twin of gpu_transpose_postings. Returns (col_offsets uint64[ncols + 1], rows uint32, vals uint32),
    the row ids strictly increasing within every column. The transpose of posting lists is the forward index, and back."""
    offs, c, v = np.ascontiguousarray(row_offsets, dtype=np.uint64), _u32(cols), _u32(vals)
    if len(offs) != nrows + 1 or len(c) != len(v) or len(c) < int(offs.max()):
        raise ValueError("row_offsets holds %d values for %d rows, over %d columns and %d values" % (len(offs), nrows, len(c), len(v)))
    if not len(c):
        c = v = np.zeros(1, np.uint32)
    h = [C.c_void_p() for _ in range(3)]
    _check(lib().ds2i_transpose_postings(nrows, ncols, _ptr(offs), _ptr(c), _ptr(v), threads, *[C.byref(x) for x in h]))
    return _take_csr(h)


INVERT_MS = ("check_ms", "doc_sort_ms", "count_ms", "scatter_ms", "transpose_ms", "column_sort_ms", "extract_ms", "encode_ms")


def _invert_info(ms):
    parts = (C.c_double * 8)()
    lib().ds2i_hip_invert_ms(parts)
    info = {"device_ms": ms.value}
    info.update(zip(INVERT_MS, parts))
    return info


def gpu_invert_postings(docs, nterms, device=0):
    """invert_documents ON THE GPU (ds2i_hip_invert_postings): the tokens checked, sorted within their documents, run-length compacted
    into the canonical forward index and transposed; the same arrays, element for element. Returns ((list_offsets, docs, freqs,
    doc_sizes), dict(device_ms, check_ms, doc_sort_ms, count_ms, scatter_ms, transpose_ms, column_sort_ms, ...))."""
    n, offs, tokens = _forward(docs)
    h, ms = [C.c_void_p() for _ in range(4)], C.c_double()
    _check(lib().ds2i_hip_invert_postings(device, n, _ptr(offs), _ptr(tokens), nterms, *[C.byref(x) for x in h], C.byref(ms)))
    return _take_csr(h), _invert_info(ms)


def gpu_transpose_postings(nrows, ncols, row_offsets, cols, vals, device=0):
    """transpose_postings ON THE GPU (ds2i_hip_transpose_postings): a histogram of the columns, a scatter through one cursor per
    column, and the segmented sort of gpu_remap_postings over the columns; the same arrays, element for element.
    Returns ((col_offsets, rows, vals), dict(device_ms, transpose_ms, column_sort_ms, ...))."""
    offs, c, v = np.ascontiguousarray(row_offsets, dtype=np.uint64), _u32(cols), _u32(vals)
    if len(offs) != nrows + 1 or len(c) != len(v) or len(c) < int(offs.max()):
        raise ValueError("row_offsets holds %d values for %d rows, over %d columns and %d values" % (len(offs), nrows, len(c), len(v)))
    if not len(c):
        c = v = np.zeros(1, np.uint32)
    h, ms = [C.c_void_p() for _ in range(3)], C.c_double()
    _check(lib().ds2i_hip_transpose_postings(device, nrows, ncols, _ptr(offs), _ptr(c), _ptr(v), *[C.byref(x) for x in h], C.byref(ms)))
    return _take_csr(h), _invert_info(ms)


def gpu_invert_documents(kind, docs, nterms, wand=True, device=0):
    """Documents indexed ON THE GPU (ds2i_hip_invert_documents): inverted as gpu_invert_postings does and encoded where the postings
    lie, with the wand data from the same staging. kind: a kind gpu_encode_index writes. Terms that never occur get no list: term_map
    (uint32, strictly increasing) gives the old term of every list of the image, the map gpu_merge_indexes takes; doc_sizes are the
    token counts. The image is byte-identical to build_index(kind, ...) over invert_documents' nonempty lists, the wand image (None
    with wand=False) to build_wand over them with doc_sizes.
    Returns ((image, wand, term_map, doc_sizes), dict(device_ms, check_ms, doc_sort_ms, count_ms, scatter_ms, transpose_ms,
    column_sort_ms, encode_ms, ...))."""
    n, offs, tokens = _forward(docs)
    hi, hw, ht, hs, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_invert_documents(device, _codec(kind), n, _ptr(offs), _ptr(tokens), nterms, C.byref(hi), C.byref(hw) if wand else None,
                                           C.byref(ht), C.byref(hs), C.byref(ms)))
    return (_take_blob(hi), _take_blob(hw) if wand else None, np.frombuffer(_take_blob(ht), dtype=np.uint32),
            np.frombuffer(_take_blob(hs), dtype=np.uint32)), _invert_info(ms)


def gpu_forward_index(kind, image, device=0):
    """The forward index of an index image of `kind` (any of the nine) ON THE GPU (ds2i_hip_forward_index): extracted in one launch
    and transposed. Document d holds the terms (list numbers) terms[doc_offsets[d]:doc_offsets[d + 1]], strictly increasing, with
    their freqs beside them. Returns ((num_docs, nterms, doc_offsets uint64[num_docs + 1], terms uint32, freqs uint32),
    dict(device_ms, extract_ms, transpose_ms, column_sort_ms, ...))."""
    n, v, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    h = [C.c_void_p() for _ in range(3)]
    _check(lib().ds2i_hip_forward_index(device, _codec(kind), image, len(image), C.byref(n), C.byref(v), *[C.byref(x) for x in h], C.byref(ms)))
    return (n.value, v.value) + _take_csr(h), _invert_info(ms)


class OrderParams(C.Structure):
    """ds2i_order_params: zero in a field means its default (iterations 20, min_half 16, max_levels 32)"""
    _fields_ = [("iterations", C.c_uint32), ("min_half", C.c_uint32), ("max_levels", C.c_uint32)]


ORDER_MS = ("extract_ms", "level_sort_ms", "runs_ms", "degrees_ms", "gains_ms", "gain_sort_ms", "swap_ms", "compose_ms")


def _order_lists(lists):
    """posting lists as an iterable of doc-id arrays or of (docs, freqs) -> (number of lists, offsets uint64, docs uint32)"""
    lists = [_u32(x[0] if isinstance(x, tuple) else x) for x in lists]
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    if lists:
        offs[1:] = np.cumsum([len(d) for d in lists], dtype=np.uint64)
    docs = np.concatenate(lists) if lists else np.zeros(0, np.uint32)
    if not len(docs):
        docs = np.zeros(1, np.uint32)  # (a pointer the library may check against NULL)
    return len(lists), offs, docs


def _order_info(ms):
    parts = (C.c_double * 8)()
    lib().ds2i_hip_order_ms(parts)
    info = {"device_ms": ms.value}
    info.update(zip(ORDER_MS, parts))
    return info


def _take_order(hm, ht):
    return np.frombuffer(_take_blob(hm), dtype=np.uint32), np.frombuffer(_take_blob(ht), dtype=np.uint64)


def order_log_table(n):
    """LOGQ[0 .. n) (ds2i_order_log_table): rint(log2(x) * 256) as uint32, LOGQ[0] = 0 -- the fixed-point logarithms of the ordering"""
    out = np.zeros(max(n, 1), dtype=np.uint32)
    _check(lib().ds2i_order_log_table(n, _ptr(out)))
    return out[:n]


def postings_cost(lists):
    """The sum of LOGQ[gap] over all postings of `lists` (doc-id arrays or (docs, freqs) pairs), a list's first gap being doc + 1
    (ds2i_postings_cost): the size of the collection under an ideal gap coder in 1/256 bits, an exact Python int."""
    n, offs, docs = _order_lists(lists)
    cost = C.c_uint64()
    _check(lib().ds2i_postings_cost(n, _ptr(offs), _ptr(docs), C.byref(cost)))
    return cost.value


def order_postings(num_docs, lists, iterations=0, min_half=0, max_levels=0, threads=0):
    """A document order for `lists` (doc-id arrays or (docs, freqs) pairs; doc-ids strictly increasing and < num_docs) by recursive
    graph bisection ON THE HOST (ds2i_order_postings), the host twin of gpu_order_postings. Zero in a parameter means its default
    (iterations 20, min_half 16, max_levels 32). Returns (doc_map uint32[num_docs] with new id = doc_map[old id], what remap_postings
    and Index.remap take; trace uint64, the exchanges of every (level, iteration) that ran)."""
    n, offs, docs = _order_lists(lists)
    prm, hm, ht = OrderParams(iterations, min_half, max_levels), C.c_void_p(), C.c_void_p()
    _check(lib().ds2i_order_postings(num_docs, n, _ptr(offs), _ptr(docs), C.byref(prm), threads, C.byref(hm), C.byref(ht)))
    return _take_order(hm, ht)


def gpu_order_postings(num_docs, lists, iterations=0, min_half=0, max_levels=0, device=0):
    """order_postings ON THE GPU (ds2i_hip_order_postings): degrees, gains and swaps as HIP kernels over the lists where they lie, the
    halves sorted by the segmented sort of gpu_remap_postings; the same map and trace, element for element.
    Returns ((doc_map, trace), dict(device_ms, level_sort_ms, runs_ms, degrees_ms, gains_ms, gain_sort_ms, swap_ms, compose_ms, ...))."""
    n, offs, docs = _order_lists(lists)
    prm, hm, ht, ms = OrderParams(iterations, min_half, max_levels), C.c_void_p(), C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_order_postings(device, num_docs, n, _ptr(offs), _ptr(docs), C.byref(prm), C.byref(hm), C.byref(ht), C.byref(ms)))
    return _take_order(hm, ht), _order_info(ms)


def gpu_order_index(kind, image, iterations=0, min_half=0, max_levels=0, device=0):
    """A document order for an index image of `kind` (any of the nine) ON THE GPU (ds2i_hip_order_index): extracted in one launch and
    ordered where the postings lie; order_postings' map and trace over the extracted lists.
    Returns ((doc_map, trace), dict(device_ms, extract_ms, ...)); gpu_remap_index(kind, image, doc_map) applies the map."""
    prm, hm, ht, ms = OrderParams(iterations, min_half, max_levels), C.c_void_p(), C.c_void_p(), C.c_double()
    _check(lib().ds2i_hip_order_index(device, _codec(kind), image, len(image), C.byref(prm), C.byref(hm), C.byref(ht), C.byref(ms)))
    return _take_order(hm, ht), _order_info(ms)


def synth_build_gpu(p, device=0, threads=0):
    """The synthetic collection as a block_optpfor index encoded on the GPU (ds2i_hip_synth_encode).
    -> (index image, wand image, postings, dict(generate_s, device_ms))"""
    hi, hw = C.c_void_p(), C.c_void_p()
    n, gs, ms = C.c_uint64(), C.c_double(), C.c_double()
    _check(lib().ds2i_hip_synth_encode(device, C.byref(p), threads, C.byref(hi), C.byref(hw), C.byref(n), C.byref(gs), C.byref(ms)))
    return _take_blob(hi), _take_blob(hw), n.value, {"generate_s": gs.value, "device_ms": ms.value}


def build_wand(doc_sizes, lists):
    L = lib()
    s = _u32(doc_sizes)
    w = C.c_void_p()
    _check(L.ds2i_wand_create(_ptr(s), len(s), C.byref(w)))
    try:
        for docs, freqs in lists:
            d, f = _u32(docs), _u32(freqs)
            _check(L.ds2i_wand_add_list(w, len(d), _ptr(d), _ptr(f)))
        h = C.c_void_p()
        _check(L.ds2i_wand_freeze(w, C.byref(h)))
        return _take_blob(h)
    finally:
        L.ds2i_wand_free(w)


class HybridModel(C.Structure):
    """MI355X decode cost per 128-value block, wave-level instructions (ds2i_hybrid_model)."""
    _fields_ = [(n, C.c_float) for n in ("pfor_base", "pfor_exc", "pfor_exc_many", "varint", "interp_base", "interp_node")]

    @classmethod
    def default(cls):
        m = cls()
        lib().ds2i_hybrid_default_model(C.byref(m))
        return m


HULL_POINT = np.dtype([("time", np.float32), ("space", np.uint16), ("type", np.uint8), ("b", np.int8)])


class HybridBuilder:
    """block_mixed space/time optimiser (ds2i_hybrid_*; reference optimal_hybrid_index.cpp)."""

    def __init__(self, num_docs, model=None):
        self._h = C.c_void_p()
        _check(lib().ds2i_hybrid_create(num_docs, C.byref(model) if model is not None else None, C.byref(self._h)))

    def add_posting_list(self, docs, freqs, access=None):
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        a = None
        if access is not None:
            a = np.ascontiguousarray(access, dtype=np.uint32).reshape(-1)
            assert a.size == 2 * ((len(d) + 127) // 128)
        _check(lib().ds2i_hybrid_add_posting_list(self._h, len(d), _ptr(d), _ptr(f), _ptr(a) if a is not None else None))

    def analyse(self, threads=0, device=None):
        """-> (min_space, max_space). device=None analyses on `threads` host threads, an integer on that GPU
        (ds2i_hip_hybrid_analyse; self.device_ms then holds the kernel time): the hulls are the same bit for bit."""
        lo, hi = C.c_uint64(), C.c_uint64()
        if device is None:
            _check(lib().ds2i_hybrid_analyse(self._h, threads, C.byref(lo), C.byref(hi)))
        else:
            ms = C.c_double()
            _check(lib().ds2i_hip_hybrid_analyse(self._h, int(device), C.byref(lo), C.byref(hi), C.byref(ms)))
            self.device_ms = ms.value
        return lo.value, hi.value

    def freeze(self, budget_bytes=None, threads=0, device=None):
        """-> (image bytes, dict(rate, space, model_time, type_counts)); with device=<int> the image is written on that
        GPU (ds2i_hip_hybrid_freeze), byte-identical, and the dict also holds device_ms"""
        h = C.c_void_p()
        rate, t, space = C.c_double(), C.c_double(), C.c_uint64()
        tc = (C.c_uint64 * 6)()
        budget = 0xFFFFFFFFFFFFFFFF if budget_bytes is None else int(budget_bytes)
        extra = {}
        if device is None:
            _check(lib().ds2i_hybrid_freeze(self._h, budget, threads, C.byref(h), C.byref(rate), C.byref(space), C.byref(t), tc))
        else:
            ms = C.c_double()
            _check(lib().ds2i_hip_hybrid_freeze(self._h, int(device), budget, C.byref(h), C.byref(rate), C.byref(space),
                                                C.byref(t), tc, C.byref(ms)))
            extra["device_ms"] = ms.value
        return _take_blob(h), dict({"rate": rate.value, "space": space.value, "model_time": t.value,
                                    "type_counts": {"docs": list(tc[0:3]), "freqs": list(tc[3:6])}}, **extra)

    def hull(self, list, block, side):
        """The lower convex hull of one part after analyse (ds2i_hybrid_hull): side 0 = docs, 1 = freqs. A structured array
        (HULL_POINT: time, space, type, b) by increasing space and decreasing time."""
        n = C.c_uint32()
        pts = np.zeros(24, dtype=HULL_POINT)  # a part has at most 19 candidates
        _check(lib().ds2i_hybrid_hull(self._h, int(list), int(block), int(side), _ptr(pts), len(pts), C.byref(n)))
        return pts[:n.value]

    def close(self):
        if self._h:
            lib().ds2i_hybrid_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def synth_build_hybrid(p, budget_frac=0.5, threads=0, access=None, model=None):
    """The synthetic collection as an optimised block_mixed index -> (index image, wand image, postings, type_counts)."""
    hi, hw = C.c_void_p(), C.c_void_p()
    n = C.c_uint64()
    tc = (C.c_uint64 * 6)()
    a = None if access is None else np.ascontiguousarray(access, dtype=np.uint32).reshape(-1)
    _check(lib().ds2i_synth_build_hybrid(C.byref(p), threads, C.byref(model) if model is not None else None,
                                         _ptr(a) if a is not None else None, float(budget_frac), C.byref(hi), C.byref(hw),
                                         C.byref(n), tc))
    return _take_blob(hi), _take_blob(hw), n.value, {"docs": list(tc[0:3]), "freqs": list(tc[3:6])}


def opt_list_directory(image, term, kind="opt"):
    """The chunk directory the GPU upload builds for one list of a freq_index image (inspection / tests)."""
    hc, hk = C.c_void_p(), C.c_void_p()
    info = (C.c_uint64 * 5)()
    _check(lib().ds2i_freq_list_directory(_codec(kind), image, len(image), term, C.byref(hc), C.byref(hk), info))
    cmax = np.frombuffer(_take_blob(hc), dtype=np.uint32)
    chunks = np.frombuffer(_take_blob(hk), dtype=np.uint32).reshape(-1, 12)
    return cmax, chunks, [int(x) for x in info]


def synth_list(p, term):
    cap = int(p.num_docs)
    d = np.empty(cap, dtype=np.uint32)
    f = np.empty(cap, dtype=np.uint32)
    n = C.c_uint64()
    _check(lib().ds2i_synth_list(C.byref(p), term, _ptr(d), _ptr(f), cap, C.byref(n)))
    return d[:n.value].copy(), f[:n.value].copy()


def synth_doc_sizes(p):
    s = np.empty(int(p.num_docs), dtype=np.uint32)
    _check(lib().ds2i_synth_doc_sizes(C.byref(p), _ptr(s)))
    return s


def set_option(name, value):
    """a DS2I_* tuning knob without the environment (ds2i_hip_set_option): read by the uploads after it (each index keeps its own)"""
    _check(lib().ds2i_hip_set_option(name.encode(), None if value is None else str(value).encode()))


def synth_queries(seed, num_terms, nq):
    t = np.empty(11 * nq + 1, dtype=np.uint32)
    o = np.empty(nq + 1, dtype=np.uint32)
    _check(lib().ds2i_synth_queries(seed, num_terms, nq, _ptr(t), _ptr(o)))
    return [t[o[i]:o[i + 1]].tolist() for i in range(nq)]


def synth_queries_topical(p, seed, nq, same_topic_pct=25):
    """synth_queries over a correlated collection (p.topics > 1): same_topic_pct percent of the multi-term queries take
    all their terms from one topic"""
    t = np.empty(11 * nq + 1, dtype=np.uint32)
    o = np.empty(nq + 1, dtype=np.uint32)
    _check(lib().ds2i_synth_queries_topical(C.byref(p), seed, nq, same_topic_pct, _ptr(t), _ptr(o)))
    return [t[o[i]:o[i + 1]].tolist() for i in range(nq)]


def synth_build(p, codec, threads=0):
    """Returns (index_image, wand_image, total_postings) for the synthetic collection p."""
    hi, hw = C.c_void_p(), C.c_void_p()
    tot = C.c_uint64()
    _check(lib().ds2i_synth_build(C.byref(p), _codec(codec), threads, C.byref(hi), C.byref(hw), C.byref(tot)))
    return _take_blob(hi), _take_blob(hw), tot.value


# ---------------------------------------------------------------- query side (GPU)
def _flatten(queries):
    offs = np.zeros(len(queries) + 1, dtype=np.uint32)
    for i, q in enumerate(queries):
        offs[i + 1] = offs[i] + len(q)
    terms = np.zeros(max(int(offs[-1]), 1), dtype=np.uint32)
    pos = 0
    for q in queries:
        terms[pos:pos + len(q)] = q
        pos += len(q)
    return terms, offs


def _op(op):
    return OPS[op] if isinstance(op, str) else int(op)


def _docs_op(op, with_docs):
    """op with TOPK_DOCS added when with_docs; the unranked operators have no top-k to name (refused here, before the library)"""
    o = _op(op) | (TOPK_DOCS if with_docs else 0)
    if (o & TOPK_DOCS) and (o & 0xFF) not in _RANKED:
        raise ValueError("doc-ids of the top-k exist for ranked operators only (ranked_and, wand, maxscore, ranked_or)")
    return o


class Batch:
    """A prepared query batch resident in HBM (ds2i_hip_batch_*)."""

    def __init__(self, index, op, queries, k=10, want_matches=False, reference_order=False, with_docs=False):
        self.index, self.nq, self.k = index, len(queries), k
        self.op = _docs_op(op, with_docs) | (REFERENCE_ORDER if reference_order else 0)
        terms, offs = _flatten(queries)
        self._h = C.c_void_p()
        _check(lib().ds2i_hip_batch_prepare(index._h, self.op, k, _ptr(terms), _ptr(offs), self.nq,
                                            1 if want_matches else 0, C.byref(self._h)))
        self.k = k if (self.op & 0xFF) in _RANKED else max(k, 1)

    def set_instrumented(self, on):
        """Statistics counters on (default) / off -- see ds2i_hip_batch_set_instrumented."""
        _check(lib().ds2i_hip_batch_set_instrumented(self._h, 1 if on else 0))

    def enable_block_profile(self):
        """Start counting per-block decodes (block indexes; instrumented runs accumulate)."""
        _check(lib().ds2i_hip_batch_enable_block_profile(self._h))

    def block_profile(self):
        """uint32[total_blocks, 2]: (docs decodes, freqs decodes) per block, lists in index order."""
        tot = C.c_uint64()
        _check(lib().ds2i_hip_batch_block_profile(self._h, None, 0, C.byref(tot)))
        out = np.zeros((max(tot.value, 1), 2), dtype=np.uint32)
        _check(lib().ds2i_hip_batch_block_profile(self._h, _ptr(out), out.size, C.byref(tot)))
        return out[:tot.value]

    def run(self):
        st = Stats()
        _check(lib().ds2i_hip_batch_run(self._h, C.byref(st)))
        return st

    def class_stats(self, cls):
        st, n = Stats(), C.c_uint32()
        _check(lib().ds2i_hip_batch_class_stats(self._h, cls, C.byref(st), C.byref(n)))
        return st, n.value

    def class_groups(self, cls):
        """launch groups of kernel class `cls` in the last run (ds2i_hip_batch_class_groups)"""
        return _class_groups(lib().ds2i_hip_batch_class_groups, self._h, cls)

    def phase_cycles(self, cls):
        names = ("total", "docs", "freqs", "find", "member", "score", "topk", "prolog", "probe", "insert", "stream", "prefetch", "floor", "unit",
                 "n_visit", "n_surv1", "n_surv2", "n_bdocs", "n_bfreqs", "n_heap", "n_liverounds", "n_alive", "n_gblocks")
        out = np.zeros(len(names), dtype=np.uint64)
        _check(lib().ds2i_hip_batch_phase_cycles(self._h, cls, _ptr(out), len(names)))
        return dict(zip(names, out.tolist()))

    def fetch(self):
        nq = max(self.nq, 1)
        count = np.zeros(nq, dtype=np.uint64)
        topk = np.full((nq, self.k), -np.inf, dtype=np.float32)
        tlen = np.zeros(nq, dtype=np.uint32)
        fsum = np.zeros(nq, dtype=np.uint64)
        _check(lib().ds2i_hip_batch_fetch(self._h, _ptr(count), _ptr(topk), _ptr(tlen), _ptr(fsum)))
        return count[:self.nq], topk[:self.nq], tlen[:self.nq], fsum[:self.nq]

    def fetch_topk_docs(self):
        """uint32[nq, k]: the doc-id of every top-k score of the last run (batches prepared with_docs; 0xFFFFFFFF past tlen)"""
        docs = np.full((max(self.nq, 1), self.k), 0xFFFFFFFF, dtype=np.uint32)
        _check(lib().ds2i_hip_batch_fetch_topk_docs(self._h, _ptr(docs)))
        return docs[:self.nq]

    def fetch_matches(self, counts):
        tot = C.c_uint64()
        _check(lib().ds2i_hip_batch_match_total(self._h, C.byref(tot)))
        offs = np.zeros(self.nq + 1, dtype=np.uint64)
        m = np.zeros(max(tot.value, 1), dtype=np.uint32)
        _check(lib().ds2i_hip_batch_fetch_matches(self._h, _ptr(offs), _ptr(m)))
        return [m[int(offs[i]):int(offs[i]) + int(counts[i])].copy() for i in range(self.nq)]

    def close(self):
        if self._h:
            lib().ds2i_hip_batch_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """Pipelined submit / wait over reusable batch slots (ds2i_hip_pipeline_*): submit() plans the batch on the host
    and enqueues upload + kernels + result copy without waiting for the device, so the next submit() overlaps with
    the kernels of this one. A serving loop keeps `depth` batches in flight."""

    def __init__(self, index, depth=3):
        self.index, self.depth = index, depth
        self._h = C.c_void_p()
        self._meta = {}
        _check(lib().ds2i_hip_pipeline_create(index._h, depth, C.byref(self._h)))

    def set_instrumented(self, on):
        _check(lib().ds2i_hip_pipeline_set_instrumented(self._h, 1 if on else 0))

    def submit(self, op, queries, k=10, with_docs=False):
        """queries: list of term lists, or an already flattened (terms uint32[], offsets uint32[nq+1]) pair.
        with_docs: the ticket also returns the doc-ids of the top-k (wait_docs)."""
        o = _docs_op(op, with_docs)
        terms, offs = queries if isinstance(queries, tuple) else _flatten(queries)
        nq = len(offs) - 1
        t = C.c_uint64()
        _check(lib().ds2i_hip_pipeline_submit(self._h, o, k, _ptr(terms), _ptr(offs), nq, C.byref(t)))
        self._meta[t.value] = (nq, k if (_op(op) & 0xFF) in _RANKED else 1)
        return t.value

    def wait(self, ticket, stats=False):
        nq, k = self._meta.pop(ticket, (0, 1))
        count = np.zeros(max(nq, 1), dtype=np.uint64)
        topk = np.full((max(nq, 1), k), -np.inf, dtype=np.float32)
        tlen = np.zeros(max(nq, 1), dtype=np.uint32)
        st = Stats()
        _check(lib().ds2i_hip_pipeline_wait(self._h, ticket, _ptr(count), _ptr(topk), _ptr(tlen), C.byref(st) if stats else None))
        return (count[:nq], topk[:nq], tlen[:nq], st) if stats else (count[:nq], topk[:nq], tlen[:nq])

    def wait_docs(self, ticket, stats=False):
        """wait() for a ticket submitted with_docs -> (count, topk, docs uint32[nq, k], tlen[, stats])"""
        nq, k = self._meta.get(ticket, (0, 1))
        count = np.zeros(max(nq, 1), dtype=np.uint64)
        topk = np.full((max(nq, 1), k), -np.inf, dtype=np.float32)
        docs = np.full((max(nq, 1), k), 0xFFFFFFFF, dtype=np.uint32)
        tlen = np.zeros(max(nq, 1), dtype=np.uint32)
        st = Stats()
        _check(lib().ds2i_hip_pipeline_wait_docs(self._h, ticket, _ptr(count), _ptr(topk), _ptr(docs), _ptr(tlen), C.byref(st) if stats else None))
        self._meta.pop(ticket, None)  # (a refused wait leaves the ticket in flight)
        r = (count[:nq], topk[:nq], docs[:nq], tlen[:nq])
        return r + (st,) if stats else r

    def class_stats(self, cls):
        """(Stats, queries) of kernel class `cls` for the ticket collected last."""
        st, n = Stats(), C.c_uint32()
        _check(lib().ds2i_hip_pipeline_class_stats(self._h, cls, C.byref(st), C.byref(n)))
        return st, n.value

    def class_groups(self, cls):
        """launch groups of kernel class `cls` for the ticket collected last (ds2i_hip_pipeline_class_groups)"""
        return _class_groups(lib().ds2i_hip_pipeline_class_groups, self._h, cls)

    def close(self):
        if self._h:
            lib().ds2i_hip_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def flatten_queries(queries):
    """(terms, offsets) arrays of a query batch -- the form that crosses the C ABI."""
    return _flatten(queries)


class IndexInfo(C.Structure):
    """ds2i_hip_index_info (include/ds2i_hip.h)"""
    _fields_ = [("index_bytes", C.c_uint64), ("skip_table_bytes", C.c_uint64), ("block_weight_bytes", C.c_uint64), ("range_table_bytes", C.c_uint64),
                ("norm_len_bytes", C.c_uint64), ("total_blocks", C.c_uint64), ("total_postings", C.c_uint64), ("has_block_weights", C.c_int),
                ("has_range_tables", C.c_int), ("has_bitmaps", C.c_int), ("has_membership_hints", C.c_int), ("range_table_entries_per_posting", C.c_int),
                ("side_table_bytes", C.c_uint64), ("has_side_tables", C.c_int), ("transcoded_from", C.c_int), ("table_budget_bytes", C.c_uint64)]


class Index:
    """block_freq_index resident in one GPU's HBM (Index concept: size(), num_docs(), operator[])."""

    def __init__(self, kind, index_image, wand_image=None, device=0):
        self._h = C.c_void_p()
        self.kind = _codec(kind)
        self.device = device
        self._image = index_image  # (a reference, for remap(): the handle holds no copy of the caller's bytes)
        wi = wand_image if wand_image is not None else None
        _check(lib().ds2i_hip_index_open(device, self.kind, index_image, len(index_image), wi,
                                         len(wand_image) if wand_image is not None else 0, C.byref(self._h)))

    def size(self):
        return lib().ds2i_hip_index_size(self._h)

    def num_docs(self):
        return lib().ds2i_hip_index_num_docs(self._h)

    def device_bytes(self):
        return lib().ds2i_hip_index_device_bytes(self._h)

    def set_collection_stats(self, num_docs=0, df=None):
        """Collection-wide BM25 statistics for an index that holds a shard (ds2i_hip_index_set_collection_stats): every batch planned
        afterwards weighs a term by query_term_weight(qtf, df[term], num_docs). df: one document frequency per list of this index.
        No arguments: cleared, the index scores by its own statistics again. Not to be called while another thread plans a batch on
        this index."""
        if df is None:
            _check(lib().ds2i_hip_index_set_collection_stats(self._h, num_docs, None, 0))
            return
        a = _u32(df)
        _check(lib().ds2i_hip_index_set_collection_stats(self._h, num_docs, _ptr(a), len(a)))

    def info(self):
        """what the upload put into HBM beside the index image (ds2i_hip_index_get_info), as a dict"""
        i = IndexInfo()
        _check(lib().ds2i_hip_index_get_info(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in IndexInfo._fields_}

    def list_size(self, term):
        n = C.c_uint64()
        _check(lib().ds2i_hip_list_size(self._h, term, C.byref(n)))
        return n.value

    def __getitem__(self, term):
        """index[term]: the whole list enumerated on the GPU -> (docs, freqs)."""
        n = self.list_size(term)
        d = np.empty(n, dtype=np.uint32)
        f = np.empty(n, dtype=np.uint32)
        got = C.c_uint64()
        _check(lib().ds2i_hip_decode_list(self._h, term, _ptr(d), _ptr(f), n, C.byref(got)))
        return d, f

    def verify(self, lists):
        """This index, as queries read it, against `lists` (iterable of (docs, freqs)) in one launch (ds2i_hip_index_verify);
        the dict of gpu_verify_collection."""
        n, offs, docs, freqs = _csr(lists)
        r, ms = VerifyReport(), C.c_double()
        _check(lib().ds2i_hip_index_verify(self._h, self.num_docs(), n, _ptr(offs), _ptr(docs), _ptr(freqs), C.byref(r), C.byref(ms)))
        return _verify_result(r, ms)

    def extract(self, begin=0, end=None):
        """The postings of lists [begin, end) (end=None: to the last list) in one launch (ds2i_hip_index_extract), as queries read
        this index. Returns (offsets uint64[end - begin + 1] from 0, docs uint32, freqs uint32, dict(device_ms))."""
        L = lib()
        end = self.size() if end is None else end
        offs = np.zeros(max(end - begin, 0) + 1, dtype=np.uint64)
        total, ms = C.c_uint64(), C.c_double()
        _check(L.ds2i_hip_index_extract(self._h, begin, end, _ptr(offs), None, None, 0, C.byref(total), None))  # the size query
        docs = np.empty(max(total.value, 1), dtype=np.uint32)
        freqs = np.empty(max(total.value, 1), dtype=np.uint32)
        _check(L.ds2i_hip_index_extract(self._h, begin, end, _ptr(offs), _ptr(docs), _ptr(freqs), total.value, C.byref(total), C.byref(ms)))
        return offs, docs[:total.value], freqs[:total.value], {"device_ms": ms.value}

    def remap(self, doc_map, to_kind=None):
        """The image this index was opened from with its documents renumbered, as an image of `to_kind` (None: the same kind), on
        this index's device (gpu_remap_index). Returns (image bytes, dict(device_ms, ...)); open it with remap_wand's wand data."""
        return gpu_remap_index(self.kind, self._image, doc_map, to_kind, device=self.device)

    def split(self, shard_of, nshards=None, to_kind=None):
        """The image this index was opened from cut into shards by documents, as images of `to_kind` (None: the same kind), on this
        index's device (gpu_split_index). Returns ([(image, doc_map, term_map), ...], dict(device_ms, ...))."""
        return gpu_split_index(self.kind, self._image, shard_of, nshards, to_kind, device=self.device)

    def forward(self):
        """The forward index of the image this index was opened from, on this index's device (gpu_forward_index).
        Returns ((num_docs, nterms, doc_offsets, terms, freqs), dict(device_ms, ...))."""
        return gpu_forward_index(self.kind, self._image, device=self.device)

    def order(self, **params):
        """A document order for the image this index was opened from, on this index's device (gpu_order_index; params: iterations,
        min_half, max_levels). Returns ((doc_map, trace), dict(device_ms, ...)); remap(doc_map) applies it."""
        return gpu_order_index(self.kind, self._image, device=self.device, **params)

    def calibration_read(self):
        n = C.c_uint64()
        _check(lib().ds2i_hip_calibration_read(self._h, C.byref(n)))
        return n.value

    def block_weights(self, term):
        """bmw[] of one list (ds2i_hip_list_block_weights): float32 per block, or an empty array without wand data"""
        n = C.c_uint64()
        out = np.zeros(int(self.list_size(term)) + 8, dtype=np.float32)  # (a chunk holds at least one posting)
        _check(lib().ds2i_hip_list_block_weights(self._h, term, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def range_table(self, term, level=1):
        """(bytes, shift, list_max) of one level of one list's doc-id-range table (ds2i_hip_list_range_table)"""
        n, sh, mx = C.c_uint64(), C.c_uint32(), C.c_float()
        out = np.zeros(int(self.num_docs()) + 64, dtype=np.uint8)
        _check(lib().ds2i_hip_list_range_table(self._h, term, level, _ptr(out), len(out), C.byref(n), C.byref(sh), C.byref(mx)))
        return out[:n.value].copy(), int(sh.value), float(mx.value)

    def query_batch(self, op, queries, k=10):
        terms, offs = queries if isinstance(queries, tuple) else _flatten(queries)
        nq = len(offs) - 1
        count = np.zeros(max(nq, 1), dtype=np.uint64)
        topk = np.full((max(nq, 1), max(k, 1)), -np.inf, dtype=np.float32)
        tlen = np.zeros(max(nq, 1), dtype=np.uint32)
        st = Stats()
        _check(lib().ds2i_hip_query_batch(self._h, _op(op), k, _ptr(terms), _ptr(offs), nq, _ptr(count), _ptr(topk),
                                          _ptr(tlen), C.byref(st)))
        return count[:nq], topk[:nq], tlen[:nq], st

    def query_batch_docs(self, op, queries, k=10):
        """query_batch with the doc-ids of the top-k (ranked operators) -> (count, topk, docs uint32[nq, k], tlen, stats)"""
        o = _docs_op(op, True)
        terms, offs = queries if isinstance(queries, tuple) else _flatten(queries)
        nq = len(offs) - 1
        count = np.zeros(max(nq, 1), dtype=np.uint64)
        topk = np.full((max(nq, 1), max(k, 1)), -np.inf, dtype=np.float32)
        docs = np.full((max(nq, 1), max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        tlen = np.zeros(max(nq, 1), dtype=np.uint32)
        st = Stats()
        _check(lib().ds2i_hip_query_batch_docs(self._h, o, k, _ptr(terms), _ptr(offs), nq, _ptr(count), _ptr(topk), _ptr(docs),
                                               _ptr(tlen), C.byref(st)))
        return count[:nq], topk[:nq], docs[:nq], tlen[:nq], st

    def close(self):
        if self._h:
            lib().ds2i_hip_index_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- query-operator concept
class ShardSource(C.Structure):
    """ds2i_shard_source (include/ds2i_hip.h)"""
    _fields_ = [("device", C.c_int), ("kind", C.c_int), ("image", C.c_void_p), ("bytes", C.c_size_t), ("wand_image", C.c_void_p),
                ("wand_bytes", C.c_size_t), ("doc_map", C.c_void_p), ("map_len", C.c_uint64), ("term_map", C.c_void_p), ("terms_len", C.c_uint64)]


class ShardStats(C.Structure):
    """ds2i_hip_shard_stats (include/ds2i_hip.h)"""
    _fields_ = [("kernel_ms", C.c_double * MAX_SHARDS), ("merge_ms", C.c_double), ("translate_ms", C.c_double), ("shards_open", C.c_uint32)]


class ShardSet:
    """Document shards queried as one index (ds2i_hip_shard_set_*): every shard an index on its own device with the collection's BM25
    statistics, a batch sent to all of them and their top-k rows merged on the device, in the collection's doc-ids.
    sources: iterable of (kind, image, wand_image or None, doc_map, term_map[, device]) -- wand_image is split_wand's.
    num_docs / df: the collection's statistics (None: the sums over the shards, which for a split with nothing dropped are the unsplit
    index's own)."""

    def __init__(self, sources, collection_docs, collection_terms, num_docs=None, df=None):
        self._h = C.c_void_p()
        sources = list(sources)
        arr, keep = (ShardSource * max(1, len(sources)))(), []
        for src, (kind, image, wand, doc_map, term_map, *rest) in zip(arr, sources):
            dm, tm = _u32(doc_map), _u32(term_map)
            keep.extend((image, wand, dm, tm))
            src.device, src.kind = (rest[0] if rest else 0), _codec(kind)
            src.image, src.bytes = C.cast(C.c_char_p(image), C.c_void_p), len(image)
            src.wand_image, src.wand_bytes = (None, 0) if wand is None else (C.cast(C.c_char_p(wand), C.c_void_p), len(wand))
            src.doc_map, src.map_len, src.term_map, src.terms_len = dm.ctypes.data, len(dm), tm.ctypes.data, len(tm)
        self.nsources = len(sources)
        a = None if df is None else _u32(df)
        if a is not None and len(a) != collection_terms:
            raise ValueError("df holds %d entries for %d collection terms" % (len(a), collection_terms))
        _check(lib().ds2i_hip_shard_set_open(arr, len(sources), collection_docs, collection_terms, num_docs or 0, None if a is None else _ptr(a),
                                             C.byref(self._h)))

    @classmethod
    def from_split(cls, kind, image, wand_image, shard_of, nshards=None, to_kind=None, devices=None, num_docs=None, df=None):
        """The image cut into shards on the GPU (gpu_split_index, on devices[0]), every shard given its wand data (split_wand) and
        opened on devices[s % len(devices)] (None: device 0). The collection's doc-ids are the image's."""
        devices = list(devices) if devices else [0]
        n, v = image_shape(kind, image)
        shards, _ = gpu_split_index(kind, image, shard_of, nshards, to_kind, device=devices[0])
        kind2 = kind if to_kind is None else to_kind
        sources = [(kind2, img, None if wand_image is None else split_wand(wand_image, dm, tm), dm, tm, devices[s % len(devices)])
                   for s, (img, dm, tm) in enumerate(shards)]
        return cls(sources, n, v, num_docs=num_docs, df=df)

    def _query(self, op, queries, k, ranked):
        terms, offs = queries if isinstance(queries, tuple) else _flatten(queries)
        nq = len(offs) - 1
        count = np.zeros(max(nq, 1), dtype=np.uint64)
        st = ShardStats()
        if not ranked:
            _check(lib().ds2i_hip_shard_set_query(self._h, _op(op), 0, _ptr(terms), _ptr(offs), nq, _ptr(count), None, None, None, C.byref(st)))
            return count[:nq], st
        topk = np.full((max(nq, 1), max(k, 1)), -np.inf, dtype=np.float32)
        docs = np.full((max(nq, 1), max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        tlen = np.zeros(max(nq, 1), dtype=np.uint32)
        _check(lib().ds2i_hip_shard_set_query(self._h, _op(op), k, _ptr(terms), _ptr(offs), nq, _ptr(count), _ptr(topk), _ptr(docs), _ptr(tlen),
                                              C.byref(st)))
        return count[:nq], topk[:nq], docs[:nq], tlen[:nq], st

    def query_batch_docs(self, op, queries, k=10):
        """a ranked operator over the set -> (count, topk float32[nq, k], collection doc-ids uint32[nq, k], tlen, ShardStats): what
        Index.query_batch_docs of the whole collection returns"""
        return self._query(op, queries, k, True)

    def query_counts(self, op, queries):
        """`and` / `or` over the set -> (count uint64[nq] = the sum of the shards' counts, ShardStats)"""
        return self._query(op, queries, 0, False)

    def close(self):
        if self._h:
            lib().ds2i_hip_shard_set_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _query_op:
    op = None
    ranked = False

    def __init__(self, wdata=None, k=10, with_docs=False):
        if with_docs and not self.ranked:
            raise ValueError("doc-ids of the top-k exist for ranked operators only (ranked_and, wand, maxscore, ranked_or)")
        self.k = k
        self.with_docs = with_docs
        self._topk = []
        self._topk_docs = []

    def __call__(self, index, terms):
        """uint64_t operator()(Index const&, term_id_vec) -- a batch of one query."""
        return int(self.batch(index, [list(terms)])[0])

    def batch(self, index, queries):
        if self.with_docs:
            count, topk, docs, tlen, _ = index.query_batch_docs(self.op, queries, self.k)
            self._topk_docs = [docs[i, :tlen[i]].copy() for i in range(len(queries))]
        else:
            count, topk, tlen, _ = index.query_batch(self.op, queries, self.k)
        if self.ranked:
            self._topk = [topk[i, :tlen[i]].copy() for i in range(len(queries))]
        return count

    def topk(self, i=-1):
        return self._topk[i]

    def topk_docs(self, i=-1):
        """doc-ids of topk(i), same order (operators constructed with_docs)"""
        if not self.with_docs:
            raise ValueError("the operator was constructed without with_docs")
        return self._topk_docs[i]


class and_query(_query_op):
    def __init__(self, with_freqs=False, with_docs=False):
        super().__init__(with_docs=with_docs)
        self.op = "and_freq" if with_freqs else "and"


class or_query(_query_op):
    def __init__(self, with_freqs=False, with_docs=False):
        super().__init__(with_docs=with_docs)
        self.op = "or_freq" if with_freqs else "or"


class ranked_and_query(_query_op):
    op, ranked = "ranked_and", True


class wand_query(_query_op):
    op, ranked = "wand", True


class maxscore_query(_query_op):
    op, ranked = "maxscore", True


class ranked_or_query(_query_op):
    op, ranked = "ranked_or", True
