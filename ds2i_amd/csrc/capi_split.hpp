// the shards of a split as the array ds2i_split_postings (ds2i_build.h) and ds2i_hip_split_postings / ds2i_hip_split_index (ds2i_hip.h)
// hand out: one ds2i_split_shard per shard, every member a blob or null, freed together by ds2i_split_free. No output is written unless
// every shard is: an array under construction frees itself.
#pragma once
#include <memory>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "host_split.hpp"

struct SplitShardsFree {
    uint32_t n;
    void operator()(ds2i_split_shard* s) const { ds2i_split_free(s, n); }
};
using SplitShards = std::unique_ptr<ds2i_split_shard, SplitShardsFree>;

inline SplitShards new_split_shards(uint32_t nshards) {
    return SplitShards(new ds2i_split_shard[nshards](), SplitShardsFree{nshards}); // (all members zero)
}

// the shape and the two maps of a shard; postings: its lists too (the CSR forms)
inline void fill_split_shard(ds2i_split_shard& out, ds2i_host::split_shard const& sh, bool postings) {
    out.num_docs = sh.num_docs;
    out.nlists = sh.nlists;
    out.doc_map = ds2i_blob_of(sh.doc_map);
    out.term_map = ds2i_blob_of(sh.term_map);
    if (!postings) return;
    out.list_offsets = ds2i_blob_of(sh.offs);
    out.docs = ds2i_blob_of(sh.docs);
    out.freqs = ds2i_blob_of(sh.freqs);
}
