"""Document shards queried as one index, on the GPU: the merge kernel against its twin and numpy; collection statistics on one index
against the shard-view brute force; a set of shards (of four index kinds) against the unsplit index, against numpy_merge_topk over the
shards' own answers, and across the union operators; k classes; ties across shards; terms absent from shards; deletions; a doc map that
does not increase; and the edges. shard_cases.py holds the references. Collections stay at 20 000 documents and 300 terms."""
import numpy as np
import pytest

import ds2i_amd as d
import shard_cases as shc
import split_cases as sc
from helpers import Collection, small_params
from topk_docs_ref import brute_pairs

pytestmark = pytest.mark.gpu

RANKED = ("ranked_and", "wand", "maxscore", "ranked_or")
KINDS4 = ("block_optpfor", "opt", "block_qmx", "block_mixed")
K = 10


def sources_of(name, coll, wand, shards, kinds):
    """(kind, image, wand image under the collection's normalisation, doc_map, term_map) per shard; the images are the host builder's"""
    out = []
    for s, sh in enumerate(shards):
        kind = kinds[s % len(kinds)]
        out.append((kind, sc.shard_image((name, s), coll, sh, kind), d.split_wand(wand, sh[2], sh[3]), sh[2], sh[3]))
    return out


def open_shards(sources, N, df):
    """every shard as an index of its own with the collection's statistics"""
    idx = []
    for kind, image, wand, _, term_map in sources:
        g = d.Index(kind, image, wand)
        g.set_collection_stats(N, np.asarray(df)[term_map])
        idx.append(g)
    return idx


def shard_rows(indexes, sources, op, queries, k):
    """numpy_merge_topk's input from the shards' own query_batch_docs over their translated queries"""
    rows = []
    for g, src in zip(indexes, sources):
        _, topk, docs, tlen, _ = g.query_batch_docs(op, shc.translate(queries, src[4], op == "ranked_and"), k)
        rows.append((topk, docs, tlen, src[3]))
    return rows


class Env:
    pass


@pytest.fixture(scope="module")
def env(built_lib):
    e = Env()
    e.coll = Collection(small_params())
    e.N, e.V = e.coll.num_docs, len(e.coll.lists)
    e.wand = e.coll.wand_image()
    e.queries = shc.set_queries(e.V)
    e.whole = d.Index("block_optpfor", e.coll.index_image("block_optpfor"), e.wand)
    e.range3 = d.split_postings(e.N, e.coll.lists, sc.range_assign(e.N, (7000, 13001)))
    e.range4 = d.split_postings(e.N, e.coll.lists, sc.range_assign(e.N, (4000, 9000, 15001)))
    e.rr2 = d.split_postings(e.N, e.coll.lists, sc.round_robin_assign(e.N, 2))
    e.df = shc.collection_df(e.range3, e.V)
    e.mixed_sources = sources_of("mixed4", e.coll, e.wand, e.range4, KINDS4)
    e.mixed = d.ShardSet(e.mixed_sources, e.N, e.V)
    e.small = np.array([shc.distinct_terms(q) <= 2 for q in e.queries])
    e.whole_rows = {}
    yield e
    e.mixed.close()
    e.whole.close()


def whole_rows(e, op, k=K):
    if (op, k) not in e.whole_rows:
        e.whole_rows[(op, k)] = e.whole.query_batch_docs(op, e.queries, k)[1:4]
    return e.whole_rows[(op, k)]


def assert_rows_close(got, want, what):
    """lengths equal, scores row-wise within 1e-5 relative (the project's tolerance for reordered float32 sums)"""
    assert np.array_equal(got[2], want[2]), what
    f = np.isfinite(want[0])
    assert np.array_equal(np.isfinite(got[0]), f), what
    np.testing.assert_allclose(got[0][f], want[0][f], rtol=1e-5, err_msg=str(what))


# ---------------------------------------------------------------- 1. the merge kernel
def test_merge_kernel_equals_twin_and_numpy(built_lib):
    for shape in shc.merge_shapes(lambda k: d.merge_topk_grid(256, k)):
        rows = shc.merge_rows(shape)
        k = shape[2]
        want = shc.numpy_merge_topk(rows, k)
        got = d.gpu_merge_topk(rows, k)
        shc.assert_rows_equal(got, want, shape)
        shc.assert_rows_equal(got, d.merge_topk(rows, k), shape)
        assert got[3]["device_ms"] > 0 or not want[2].any()


# ---------------------------------------------------------------- 2. statistics on one index
@pytest.mark.parametrize("how", ["range3", "rr2"])
def test_collection_stats_on_one_index(env, how):
    """This is the test that fails without the feature: with the collection's statistics a shard scores as the collection, bit for bit
    the shard-view brute force; cleared, it scores by its own again; and the two differ."""
    shards = getattr(env, how)
    sources = sources_of(how, env.coll, env.wand, shards, ("block_optpfor",))
    views = shc.shard_views(env.coll, shards)
    assert views[0].N == env.N and np.array_equal(shc.collection_df(shards, env.V), env.df)
    differ = 0
    for (kind, image, wand, doc_map, term_map), view, sh in zip(sources, views, shards):
        qs = shc.translate(env.queries, term_map, True)
        g = d.Index(kind, image, wand)
        before = g.query_batch_docs("ranked_and", qs, K)[1:4]
        g.set_collection_stats(env.N, env.df[term_map])
        got = g.query_batch_docs("ranked_and", qs, K)[1:4]
        shc.assert_rows_equal(got, shc.view_rows(view, qs, K, True), (how, "with statistics"))
        own = shc.ShardView(view.lists, view.norm_lens, sh[0], [len(dd) for dd, _ in view.lists])
        shc.assert_rows_equal(before, shc.view_rows(own, qs, K, True), (how, "without statistics"))
        differ += int(np.sum(np.any(shc.bits(got[0]) != shc.bits(before[0]), axis=1)))
        g.set_collection_stats()
        shc.assert_rows_equal(g.query_batch_docs("ranked_and", qs, K)[1:4], before, (how, "cleared"))
        with pytest.raises(d.Ds2iError) as err:  # nothing changes on an error
            g.set_collection_stats(env.N, env.df[term_map][:-1])
        assert err.value.code == -1
        with pytest.raises(d.Ds2iError) as err:
            g.set_collection_stats(sh[0] - 1, env.df[term_map])
        assert err.value.code == -1 and "smaller than the index" in str(err.value)
        low = env.df[term_map].copy()
        low[3] = len(view.lists[3][0]) - 1
        with pytest.raises(d.Ds2iError) as err:
            g.set_collection_stats(env.N, low)
        assert err.value.code == -1 and "term 3" in str(err.value)
        shc.assert_rows_equal(g.query_batch_docs("ranked_and", qs, K)[1:4], before, (how, "after refusals"))
        g.close()
    assert differ > 0


# ---------------------------------------------------------------- 3. the set against the whole index
def test_set_conditions_hold(env):
    small, large, full, multi = shc.set_conditions(env.coll, env.range4, env.queries, K)
    assert small >= 40 and large >= 40 and full >= 0.5 and multi >= 0.25, (small, large, full, multi)


def test_mixed_set_equals_the_whole_index(env):
    res = {op: env.mixed.query_batch_docs(op, env.queries, K) for op in RANKED}
    for op in RANKED:
        count, topk, docs, tlen, st = res[op]
        assert np.array_equal(count, tlen) and st.shards_open == 4 and st.merge_ms > 0
        assert_rows_close((topk, docs, tlen), whole_rows(env, op), op)
    for op in ("ranked_and", "ranked_or"):  # at most two distinct terms: a sum of two separately rounded products commutes
        w = whole_rows(env, op)
        shc.assert_rows_equal(tuple(a[env.small] for a in res[op][1:4]), tuple(a[env.small] for a in w), op)
    for op in ("wand", "maxscore"):         # the three union operators return the same rows
        shc.assert_rows_equal(res[op][1:4], res["ranked_or"][1:4], op)


def test_mixed_set_equals_numpy_merge_of_its_shards(env):
    indexes = open_shards(env.mixed_sources, env.N, env.df)
    try:
        for op in RANKED:
            rows = shard_rows(indexes, env.mixed_sources, op, env.queries, K)
            shc.assert_rows_equal(env.mixed.query_batch_docs(op, env.queries, K)[1:4], shc.numpy_merge_topk(rows, K), op)
    finally:
        for g in indexes:
            g.close()


# ---------------------------------------------------------------- 4. k
@pytest.mark.parametrize("k", [1, 10, 64, 65, 257])
def test_k_classes_on_one_set(env, k):
    for op in ("ranked_and", "wand"):
        got = env.mixed.query_batch_docs(op, env.queries, k)[1:4]
        w = whole_rows(env, op, k)
        assert_rows_close(got, w, (op, k))
        if op == "ranked_and":
            shc.assert_rows_equal(tuple(a[env.small] for a in got), tuple(a[env.small] for a in w), (op, k))


# ---------------------------------------------------------------- 5. ties
def test_ties_interleave_across_round_robin_shards(built_lib):
    coll = shc.small_tie_collection()
    qs = [q for q in shc.small_tie_queries() if shc.distinct_terms(q) <= 2]
    tied = 0
    for q in qs:
        s, _ = brute_pairs(coll, q, K + 1, True)
        tied += len(s) > K and s[K - 1] == s[K]
    assert tied >= len(qs) / 2, (tied, len(qs))
    wand = coll.wand_image()
    shards = d.split_postings(coll.num_docs, coll.lists, sc.round_robin_assign(coll.num_docs, 3))
    whole = d.Index("block_optpfor", coll.index_image("block_optpfor"), wand)
    s = d.ShardSet(sources_of("tie_rr3", coll, wand, shards, ("block_optpfor",)), coll.num_docs, len(coll.lists))
    try:
        for op in ("ranked_and", "ranked_or"):
            shc.assert_rows_equal(s.query_batch_docs(op, qs, K)[1:4], whole.query_batch_docs(op, qs, K)[1:4], op)
    finally:
        s.close()
        whole.close()


# ---------------------------------------------------------------- 6. terms absent from shards
def test_absent_terms_over_range_shards_of_short_lists(built_lib):
    coll = sc.short_lists_collection()
    n, V = coll.num_docs, len(coll.lists)
    rng = np.random.default_rng(0xAB5E)
    qs = [[int(t)] for t in rng.integers(0, V, 20)] + [[int(t) for t in rng.integers(0, V, m)] for m in (2,) * 30 + (3,) * 30 + (4, 6, 9, 16, 20) * 2]
    qs += [[5, 5], []]
    shards = d.split_postings(n, coll.lists, sc.range_assign(n, (1300, 2700)))
    assert all(len(sh[3]) < V for sh in shards)  # every shard lacks terms
    wand = coll.wand_image()
    whole = d.Index("block_optpfor", coll.index_image("block_optpfor"), wand)
    sources = sources_of("short_range3", coll, wand, shards, ("block_optpfor",))
    s = d.ShardSet(sources, n, V)
    indexes = open_shards(sources, n, shc.collection_df(shards, V))
    try:
        for op in ("and", "or"):
            assert np.array_equal(s.query_counts(op, qs)[0], whole.query_batch(op, qs)[0]), op
        got = s.query_batch_docs("ranked_or", qs, K)[1:4]
        w = whole.query_batch_docs("ranked_or", qs, K)[1:4]
        assert_rows_close(got, w, "ranked_or")
        small = np.array([shc.distinct_terms(q) <= 2 for q in qs])
        shc.assert_rows_equal(tuple(a[small] for a in got), tuple(a[small] for a in w), "ranked_or")
        shc.assert_rows_equal(got, shc.numpy_merge_topk(shard_rows(indexes, sources, "ranked_or", qs, K), K), "ranked_or")
    finally:
        for g in indexes:
            g.close()
        s.close()
        whole.close()


# ---------------------------------------------------------------- 7. deletions
def test_deletions_score_with_the_statistics_given(env):
    """about a tenth of the documents dropped; the set is told the statistics of the collection before the deletions, and equals the
    brute force over the surviving documents under those statistics"""
    shard_of = sc.random_assign(env.N, 3)
    shards = d.split_postings(env.N, env.coll.lists, shard_of, nshards=3)
    assert sum(sh[0] for sh in shards) < env.N
    df = np.array([len(dd) for dd, _ in env.coll.lists])
    views = shc.shard_views(env.coll, shards, N=env.N, df=df)
    s = d.ShardSet(sources_of("random3", env.coll, env.wand, shards, ("block_optpfor",)), env.N, env.V, num_docs=env.N, df=df)
    try:
        want, _ = shc.set_rows(env.coll, shards, views, env.queries, K, True)
        got = s.query_batch_docs("ranked_and", env.queries, K)[1:4]
        shc.assert_rows_equal(got, want, "ranked_and")
        live = got[1][got[1] != shc.NO_DOC]
        assert np.all(shard_of[live] != d.DROP)
    finally:
        s.close()


# ---------------------------------------------------------------- 8. a doc map that does not increase
def test_a_permuted_shard(env):
    shards = list(env.rr2)
    n1, lists1, dm1, tm1 = shards[1]
    perm = np.random.default_rng(0x9E77).permutation(n1).astype(np.uint32)
    new_map = np.empty(n1, dtype=np.uint32)
    new_map[perm] = dm1  # the document that was local id i is now perm[i]
    shards[1] = (n1, d.remap_postings(n1, lists1, perm), new_map, tm1)
    assert not np.all(np.diff(new_map.astype(np.int64)) > 0)
    sources = sources_of("rr2_permuted", env.coll, env.wand, shards, ("block_optpfor",))
    s = d.ShardSet(sources, env.N, env.V)
    indexes = open_shards(sources, env.N, env.df)
    try:
        for op in ("ranked_and", "ranked_or"):
            rows = shard_rows(indexes, sources, op, env.queries, K)
            got = s.query_batch_docs(op, env.queries, K)[1:4]
            shc.assert_rows_equal(got, shc.numpy_merge_topk(rows, K), op)
            assert_rows_close(got, whole_rows(env, op), op)
    finally:
        for g in indexes:
            g.close()
        s.close()


def test_a_permuted_rank_through_the_device_merge_over_ranks(env):
    """merge_topk_over_ranks with device=: a rank whose doc map does not increase hands the kernel collection ids without a map, so its
    rows must reach it in key order (sharding.rows_in_collection_order). One process stands for each rank in turn: the rows every rank
    would gather are put together here as the function does it, and the one-rank call goes through the whole function."""
    from ds2i_amd import sharding as sh
    for name in ("equal_interleaved_permuted", "nq65p", "full64"):
        shape = next(s for s in shc.merge_shapes(lambda k: 1 << 20) if s[0] == name)
        rows, k = shc.merge_rows(shape), shape[2]
        want = shc.numpy_merge_topk(rows, k)
        gathered = [sh.rows_in_collection_order(*r) for r in rows]
        shc.assert_rows_equal(d.gpu_merge_topk(gathered, k), want, name)
        one = sh.merge_topk_over_ranks(None, 0, 1, *rows[0], device=0)
        shc.assert_rows_equal(one, shc.numpy_merge_topk(rows[:1], k), name)
        shc.assert_rows_equal(one, sh.merge_topk_over_ranks(None, 0, 1, *rows[0]), name)
    # the shard of test 8: real rows of a remapped shard, through the device path
    shards = list(env.rr2)
    n1, lists1, dm1, tm1 = shards[1]
    perm = np.random.default_rng(0x9E77).permutation(n1).astype(np.uint32)
    new_map = np.empty(n1, dtype=np.uint32)
    new_map[perm] = dm1
    shards[1] = (n1, d.remap_postings(n1, lists1, perm), new_map, tm1)
    sources = sources_of("rr2_permuted", env.coll, env.wand, shards, ("block_optpfor",))
    indexes = open_shards(sources, env.N, env.df)
    try:
        rows = shard_rows(indexes, sources, "ranked_or", env.queries, K)
        gathered = [sh.rows_in_collection_order(*r) for r in rows]
        shc.assert_rows_equal(d.gpu_merge_topk(gathered, K), shc.numpy_merge_topk(rows, K), "ranked_or")
    finally:
        for g in indexes:
            g.close()


# ---------------------------------------------------------------- 9. edges
def test_edges(env):
    none = np.zeros(0, dtype=np.uint32)
    sources = [("block_optpfor", d.build_index("block_optpfor", 0, []), None, none, none)]      # no documents
    sources += sources_of("range3", env.coll, env.wand, env.range3, ("block_optpfor",))
    # a shard with documents and no lists: its documents are ids past the collection's, which no list holds
    sources.append(("opt", d.build_index("opt", 5, []), None, np.arange(env.N, env.N + 5, dtype=np.uint32), none))
    s = d.ShardSet(sources, env.N + 5, env.V, num_docs=env.N, df=env.df)
    try:
        qs = [[], [5, 5], [7, 3, 7, 3], [1, 2], list(range(1, 21)), [9]]
        for op in ("ranked_and", "ranked_or"):
            count, topk, docs, tlen, st = s.query_batch_docs(op, qs, K)
            assert st.shards_open == 3 and st.kernel_ms[0] == 0 and st.kernel_ms[4] == 0
            w = env.whole.query_batch_docs(op, qs, K)[1:4]
            assert_rows_close((topk, docs, tlen), w, op)
            assert tlen[0] == 0 and np.array_equal(docs[[1, 3, 5]], w[1][[1, 3, 5]]) and np.array_equal(shc.bits(topk[[1, 3, 5]]), shc.bits(w[0][[1, 3, 5]]))
        for op in ("and", "or"):
            assert np.array_equal(s.query_counts(op, qs)[0], env.whole.query_batch(op, qs)[0])
        for op in ("and_freq", "or_freq"):
            with pytest.raises(d.Ds2iError) as err:
                s.query_counts(op, qs)
            assert err.value.code == -1
        for call in (lambda: s.query_batch_docs(d.OPS["ranked_and"] | d.REFERENCE_ORDER, qs, K), lambda: s.query_batch_docs("ranked_and", qs, 1025),
                     lambda: s.query_batch_docs("ranked_and", qs, 0)):
            with pytest.raises(d.Ds2iError) as err:
                call()
            assert err.value.code == -1
        with pytest.raises(d.Ds2iError) as err:
            s.query_batch_docs("ranked_and", [[1, env.V]], K)
        assert err.value.code == -3
        assert len(s.query_batch_docs("wand", [], K)[0]) == 0
    finally:
        s.close()


def test_from_split_runs_the_split_and_scores_as_the_whole(env):
    s = d.ShardSet.from_split("block_optpfor", env.coll.index_image("block_optpfor"), env.wand, sc.range_assign(env.N, (7000, 13001)))
    try:
        got = s.query_batch_docs("ranked_and", env.queries, K)[1:4]
        w = whole_rows(env, "ranked_and")
        assert_rows_close(got, w, "from_split")
        shc.assert_rows_equal(tuple(a[env.small] for a in got), tuple(a[env.small] for a in w), "from_split")
    finally:
        s.close()
