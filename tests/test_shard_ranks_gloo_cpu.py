"""Document shards over ranks, on CPU: two gloo processes on localhost, each holding the rows ONE shard answers -- here from the numpy
brute force over its shard view (shard_cases.py), under the collection's statistics -- and ds2i_amd.sharding.merge_topk_over_ranks,
which maps the ids, gathers every rank's rows and merges them on every rank (the host twin; on GPUs the same call merges with the HIP
kernel). For queries of at most two distinct terms the merge equals the whole collection's brute-force top-k, bit for bit; for all
other queries it equals numpy_merge_topk over the two shards' rows."""
import os
import sys

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import ds2i_amd as d
    import shard_cases as shc
    import split_cases as sc
    from ds2i_amd import sharding as sh
    from helpers import Collection, small_params
    rank_, _, world_, dist = sh.init_distributed("gloo")
    assert (rank_, world_) == (rank, world) and dist is not None
    coll = Collection(small_params(num_docs=8000, num_terms=120))
    shards = d.split_postings(coll.num_docs, coll.lists, sc.round_robin_assign(coll.num_docs, world, group=3))
    views = shc.shard_views(coll, shards)
    queries = [q for q in shc.set_queries(len(coll.lists)) if max(q) < len(coll.lists)][:60] + [[]]
    ok = True
    for conj in (True, False):
        mine = shc.view_rows(views[rank], shc.translate(queries, shards[rank][3], conj), K, conj)
        got = sh.merge_topk_over_ranks(dist, rank, world, *mine, doc_map=shards[rank][2])
        rows = [shc.view_rows(v, shc.translate(queries, s[3], conj), K, conj) + (s[2],) for v, s in zip(views, shards)]
        want = shc.numpy_merge_topk(rows, K)
        for g, w in zip(got, want):
            ok = ok and bool(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)))
        whole = shc.own_view(coll.num_docs, coll.lists, coll.norm_lens)
        small = 0
        for i, q in enumerate(queries):
            if shc.distinct_terms(q) > 2:
                continue
            small += 1
            ws, wd = shc.view_pairs(whole, q, K, conj)
            ok = ok and int(got[2][i]) == len(wd) and bool(np.array_equal(got[1][i, :len(wd)], wd)) and \
                bool(np.array_equal(shc.bits(got[0][i, :len(wd)]), shc.bits(ws)))
        ok = ok and small >= 20
    ret[rank] = ok
    dist.barrier()
    dist.destroy_process_group()


def test_merge_over_one_rank_is_the_merge(built_lib):
    import ds2i_amd as d
    import shard_cases as shc
    from ds2i_amd import sharding as sh
    rows = shc.merge_rows(("nq65", 3, 10, 65, "random", "few", "increasing"))
    s, dd, ll, m = rows[1]
    got = sh.merge_topk_over_ranks(None, 0, 1, s, dd, ll, doc_map=m)
    shc.assert_rows_equal(got, shc.numpy_merge_topk([rows[1]], 10))
    shc.assert_rows_equal(got, d.merge_topk([rows[1]], 10))


def test_a_ranks_rows_are_put_into_the_merges_order(built_lib):
    """Under a doc map that does not increase a shard's equal-score runs, in local-id order, are not in the order of the merge. The ids
    are gathered without their maps, so every rank puts its rows into key order first: whoever merges them may rely on it."""
    import shard_cases as shc
    from ds2i_amd import sharding as sh
    for name in ("equal_interleaved_permuted", "nq65p", "one_row_set"):
        shape = next(s for s in shc.merge_shapes(lambda k: 1 << 20) if s[0] == name)
        for s, dd, ll, m in shc.merge_rows(shape):
            got = sh.rows_in_collection_order(s, dd, ll, m)
            shc.assert_rows_equal(got, shc.numpy_merge_topk([(s, dd, ll, m)], shape[2]), name)
            live = np.arange(shape[2])[None, :] < ll[:, None]
            plain = np.where(live, m[np.where(live, dd, 0)], shc.NO_DOC)
            assert not np.array_equal(plain, got[1])  # mapping alone leaves another order
            key = ((np.uint64(0xFFFFFFFF) - shc.bits(got[0]).astype(np.uint64)) << np.uint64(32)) | got[1].astype(np.uint64)
            assert all(np.all(np.diff(key[q, :int(ll[q])].astype(object)) > 0) for q in range(min(len(ll), 8)))
    # no map: the ids are the collection's and the rows stay as they are
    s, dd, ll, _ = shc.merge_rows(("some_empty", 3, 65, 5, "some_empty", "few", None))[0]
    shc.assert_rows_equal(sh.rows_in_collection_order(s, dd, ll), (s, dd, ll))


def test_two_rank_gloo_document_shards(built_lib):
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 29900 + (os.getpid() % 90)
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    assert ret.get(0) is True and ret.get(1) is True
