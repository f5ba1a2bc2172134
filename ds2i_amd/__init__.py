"""ds2i_amd -- MI355X-native batched query path for ds2i block indexes.

The package is a thin ctypes mirror of the C ABI in include/ds2i_hip.h and
include/ds2i_build.h (libds2i_hip.so, built in-tree by ds2i_amd/build.py).
All query results come from the HIP kernels; there is no CPU fallback.
"""
from .api import (  # noqa: F401
    CODECS, BLOCK_CODECS, FREQ_INDEX_KINDS, OPS, REFERENCE_ORDER, NO_COUNTERS, TOPK_DOCS, Ds2iError, Index, Batch, Pipeline, flatten_queries, lib, library_path,
    encode_block, encode_vbyte, encode_posting_list, build_index, build_wand, gpu_encode_index, encode_plan_ms, opt_partition, gpu_opt_partition, gpu_build_wand, gpu_build_collection, gpu_verify_collection, gpu_extract_collection, gpu_convert_index, synth_build_gpu,
    check_doc_map, remap_postings, remap_class_bounds, gpu_remap_postings, gpu_remap_index, remap_wand,
    merge_postings, gpu_merge_postings, gpu_merge_indexes,
    invert_documents, transpose_postings, gpu_invert_postings, gpu_transpose_postings, gpu_invert_documents, gpu_forward_index, invert_window,
    order_postings, gpu_order_postings, gpu_order_index, postings_cost, order_log_table, OrderParams,
    DROP, split_postings, gpu_split_postings, gpu_split_index, split_window, split_grid_waves, image_shape,
    MAX_SHARDS, ShardSet, split_wand, wand_arrays, merge_topk, gpu_merge_topk, merge_topk_grid,
    SynthParams, HybridBuilder, HybridModel, HULL_POINT, opt_list_directory, synth_list, synth_doc_sizes, set_option, synth_queries, synth_queries_topical, synth_build, synth_build_hybrid,
    and_query, or_query, ranked_and_query, wand_query, maxscore_query, ranked_or_query,
)
