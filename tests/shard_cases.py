"""The references and inputs of the shard-set tests (test_shard_abi_cpu.py, test_shard_ranks_gloo_cpu.py, test_gpu_shards.py).

numpy_merge_topk is stated from the key definition of include/ds2i_build.h, not from the twin: a candidate is entry i < lens[q] of a row
set, its key the u64 ((0xFFFFFFFF - bits(score)) << 32) | g with g = doc_map[doc] (or doc), and the output row holds the
min(k, number of candidates) smallest keys in ascending order, padded with -inf and 0xFFFFFFFF.

translate states how a query goes to a shard: a binary search of every term in the shard's term map, repeats kept; a conjunctive query
with a term the shard does not hold becomes the empty query, a union drops the absent terms.

ShardView is a shard as the index sees it once it has been given the collection's statistics: the shard's local lists, norm_lens =
coll.norm_lens[doc_map], and explicit N and df. view_pairs is the brute force over it: float32 products query weight x document weight
summed in the shard's own list order (stable by local length for ranked_and, term order for the unions), as helpers.brute_ranked does
for one collection. The query weight is the library's host bm25::query_term_weight (ds2i_bm25_query_term_weight, held bit for bit to
the golden file by test_bm25_cpu.py): the planner calls that very function, and numpy's float32 log is another implementation of
logf, which may round the last bit the other way."""
import ctypes as C

import numpy as np

import ds2i_amd as d
from helpers import _term_freqs, doc_term_weight
from topk_docs_ref import canonical_topk

NO_DOC = 0xFFFFFFFF
_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the merge
def numpy_merge_topk(rows, k):
    """rows: [(scores[nq, k], docs[nq, k], lens[nq][, doc_map or None])] -> (scores float32[nq, k], docs uint32[nq, k], lens uint32[nq])"""
    nq = len(rows[0][2])
    keys = []
    for scores, docs, lens, *rest in rows:
        s = np.ascontiguousarray(scores, dtype=np.float32).reshape(nq, k)
        dd = np.ascontiguousarray(docs, dtype=np.uint32).reshape(nq, k)
        live = np.arange(k)[None, :] < np.asarray(lens)[:, None]
        g = dd.astype(np.uint64)
        if rest and rest[0] is not None:
            m = np.asarray(rest[0], dtype=np.uint32)
            g = m[np.where(live, dd, 0)].astype(np.uint64) if len(m) else g
        key = ((np.uint64(0xFFFFFFFF) - bits(s).astype(np.uint64)) << np.uint64(32)) | g
        keys.append(np.where(live, key, np.uint64(0xFFFFFFFFFFFFFFFF)))  # (no candidate has this key: ids stay below 0xFFFFFFFF)
    total = np.minimum(k, sum(np.asarray(r[2], dtype=np.int64) for r in rows)).astype(np.uint32)
    allk = np.sort(np.concatenate(keys, axis=1), axis=1)[:, :k]
    have = np.arange(k)[None, :] < total[:, None]
    out_s = np.where(have, (np.uint64(0xFFFFFFFF) - (allk >> np.uint64(32))).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
    out_s = np.where(have, out_s, np.float32(-np.inf)).astype(np.float32)
    out_d = np.where(have, allk & np.uint64(0xFFFFFFFF), NO_DOC).astype(np.uint32)
    return out_s, out_d, total


def assert_rows_equal(got, want, what=""):
    for g, w, name in zip(got[:3], want, ("scores", "docs", "lens")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        same = np.array_equal(bits(g), bits(w)) if name == "scores" else np.array_equal(g, w)
        assert same, (what, name, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:3].tolist())


# the shape list of the merge: (name, nrows, k, nq, fill, scores, map). fill: "random" lengths 0 .. k, "some_empty" (every other row 0),
# "all_empty", "full"; scores: "few" (a handful of distinct values: ties everywhere) or "equal" (one value: the whole order rests on the
# ids, which interleave across the row sets: row set r holds the collection ids = r mod nrows); map: None (the ids are the
# collection's), "increasing", "permuted" (not increasing: the rows have to be sorted by key first); "high" (increasing, the ids end at
# 0xFFFFFFFE, far past 2^24)
MERGE_KS = (1, 2, 63, 64, 65, 256, 257, 1024)
MERGE_NROWS = (1, 2, 3, 64)


def merge_shapes(grid):
    """grid(k): the most workgroups a launch at that k has (a query a workgroup at a time): two shapes hold more queries than that"""
    shapes = []
    for nrows in MERGE_NROWS:
        for k in MERGE_KS:
            maps = ("increasing", "permuted") if (nrows * k) % 2 else ("permuted", None)
            for i, m in enumerate(maps):
                shapes.append(("grid", nrows, k, 1 if nrows * k > 4096 else 3, "random", "few" if i else "equal", m))
    shapes += [("nq65", 3, 10, 65, "random", "few", "increasing"), ("nq65p", 2, 65, 65, "some_empty", "few", "permuted"),
               ("wrap", 3, 2, grid(2) + 37, "random", "few", "permuted"), ("wrap_equal", 2, 1024, grid(1024) + 1, "full", "equal", "increasing"),
               ("all_empty", 3, 64, 3, "all_empty", "few", "increasing"), ("some_empty", 3, 65, 5, "some_empty", "few", None),
               ("full", 3, 257, 3, "full", "few", "increasing"), ("full64", 64, 64, 2, "full", "equal", "permuted"),
               ("equal_interleaved", 3, 64, 4, "full", "equal", "increasing"), ("equal_interleaved_permuted", 3, 64, 4, "full", "equal", "permuted"),
               ("high", 3, 65, 4, "random", "few", "high"), ("high_equal", 2, 256, 2, "full", "equal", "high"),
               ("one_row_set", 1, 1024, 2, "full", "few", "permuted")]
    return shapes


def merge_rows(shape, seed=0x5A4D):
    """the row sets of one shape: [(scores, docs, lens, doc_map or None)], valid as a shard returns them: every row sorted by score
    descending, its equal-score runs by LOCAL id ascending; no collection id twice in one query"""
    name, nrows, k, nq, fill, scores, how = shape

    def make():
        rng = np.random.default_rng([seed, nrows, k, nq, len(name)])
        M = max(2 * k, 64)  # local documents of a row set
        base = 0xFFFFFFFE - M * nrows + 1 if how == "high" else 7
        values = np.array([0.0, 0.25, 1.5, 1.5000001, 3.75, 11.0, 1e-30], dtype=np.float32)
        rows = []
        for r in range(nrows):
            coll_of_local = base + np.arange(M, dtype=np.int64) * nrows + r  # ids = r mod nrows (+ base), increasing in the local id
            if how == "permuted":
                coll_of_local = coll_of_local[rng.permutation(M)]
            s = np.full((nq, k), -np.inf, dtype=np.float32)
            dd = np.full((nq, k), NO_DOC, dtype=np.uint32)
            ll = np.zeros(nq, dtype=np.uint32)
            for q in range(nq):
                n = {"random": int(rng.integers(0, k + 1)), "some_empty": 0 if (q + r) % 2 else int(rng.integers(1, k + 1)),
                     "all_empty": 0, "full": k}[fill]
                local = np.sort(rng.choice(M, n, replace=False))
                if how == "high" and r == nrows - 1 and q == 0 and n:
                    local[-1] = M - 1  # the largest id of all, 0xFFFFFFFE
                    local = np.unique(local)
                    n = len(local)
                sc = np.full(n, 2.5, dtype=np.float32) if scores == "equal" else rng.choice(values, n)
                o = np.lexsort((local, -sc.astype(np.float64)))
                ll[q] = n
                s[q, :n] = sc[o]
                dd[q, :n] = local[o] if how is not None else coll_of_local[local[o]]
            rows.append((s, dd, ll, None if how is None else coll_of_local.astype(np.uint32)))
        return rows
    return _once(("merge_rows", shape, seed), make)


# ---------------------------------------------------------------- queries and shards
def translate(queries, term_map, conjunctive):
    """the queries as a shard with that term map receives them"""
    term_map = np.asarray(term_map, dtype=np.int64)
    out = []
    for q in queries:
        pos = np.searchsorted(term_map, np.asarray(q, dtype=np.int64))
        held = (pos < len(term_map)) & (term_map[np.minimum(pos, max(len(term_map) - 1, 0))] == np.asarray(q, dtype=np.int64)) if len(term_map) and len(q) else \
            np.zeros(len(q), dtype=bool)
        if conjunctive and not held.all():
            out.append([])
        else:
            out.append([int(p) for p in pos[held]])
    return out


def host_query_term_weight(qtf, df, num_docs):
    """bm25::query_term_weight as the planner computes it (ds2i_bm25_query_term_weight), one value"""
    q, f = np.array([qtf], dtype=np.uint64), np.array([df], dtype=np.uint64)
    out = np.zeros(1, dtype=np.float32)
    rc = d.lib().ds2i_bm25_query_term_weight(q.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), int(num_docs), 1, out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out[0]


class ShardView:
    """a shard with explicit statistics: local lists, the norm_lens of its documents, N and one df per local list"""

    def __init__(self, lists, norm_lens, N, df):
        self.lists, self.norm_lens, self.N, self.df = lists, np.asarray(norm_lens, dtype=np.float32), int(N), [int(x) for x in df]
        assert len(self.df) == len(self.lists)


def collection_df(shards, num_terms):
    """per collection term, the sum of the lengths of the shard lists mapped to it"""
    df = np.zeros(num_terms, dtype=np.int64)
    for _, lists, _, term_map in shards:
        for j, (dd, _) in enumerate(lists):
            df[int(term_map[j])] += len(dd)
    return df


def shard_views(coll, shards, N=None, df=None):
    """the views of the shards of a split (tuples (num_docs, lists, doc_map, term_map)) of `coll` under the statistics N / df (None: the
    sums over the shards)"""
    N = sum(s[0] for s in shards) if N is None else N
    df = collection_df(shards, len(coll.lists)) if df is None else df
    return [ShardView(lists, coll.norm_lens[doc_map], N, [df[int(t)] for t in term_map]) for _, lists, doc_map, term_map in shards]


def own_view(n, lists, norm_lens):
    """a collection under its own statistics, as an index without collection statistics scores"""
    return ShardView(lists, norm_lens, n, [len(dd) for dd, _ in lists])


def view_scored(view, terms, conjunctive):
    """(local doc-ids ascending, float32 scores) of the AND / OR of the local `terms` over a view"""
    tf = _term_freqs(terms)
    if not tf:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)
    ents = [(len(view.lists[t][0]), t, host_query_term_weight(qtf, view.df[t], view.N)) for t, qtf in tf]
    if conjunctive:
        ents.sort(key=lambda e: e[0])  # stable, by the shard's own list lengths
    docset = view.lists[tf[0][0]][0]
    for t, _ in tf[1:]:
        docset = np.intersect1d(docset, view.lists[t][0], assume_unique=True) if conjunctive else np.union1d(docset, view.lists[t][0])
    docset = docset.astype(np.uint32)
    score = np.zeros(len(docset), dtype=np.float32)
    if not len(docset):
        return docset, score
    nl = view.norm_lens[docset]
    for _, t, qw in ents:
        docs, freqs = view.lists[t]
        pos = np.minimum(np.searchsorted(docs, docset), len(docs) - 1)
        hit = docs[pos] == docset
        w = (qw * doc_term_weight(freqs[pos], nl)).astype(np.float32)
        score = np.where(hit, (score + w).astype(np.float32), score)
    return docset, score


def view_pairs(view, terms, k, conjunctive):
    """the canonical top-k of a view: (scores, local doc-ids)"""
    dd, s = view_scored(view, terms, conjunctive)
    return canonical_topk(dd, s, k)


def view_rows(view, queries, k, conjunctive):
    """the rows a shard returns for its (translated) queries: (scores[nq, k], docs[nq, k], lens[nq])"""
    nq = len(queries)
    s = np.full((nq, k), -np.inf, dtype=np.float32)
    dd = np.full((nq, k), NO_DOC, dtype=np.uint32)
    ll = np.zeros(nq, dtype=np.uint32)
    for i, q in enumerate(queries):
        a, b = view_pairs(view, q, k, conjunctive)
        ll[i] = len(a)
        s[i, :len(a)], dd[i, :len(a)] = a, b
    return s, dd, ll


def set_rows(coll, shards, views, queries, k, conjunctive):
    """the brute force of a whole set: every shard's rows over its translated queries, merged by numpy_merge_topk"""
    rows = [view_rows(v, translate(queries, sh[3], conjunctive), k, conjunctive) + (sh[2],) for v, sh in zip(views, shards)]
    return numpy_merge_topk(rows, k), rows


# ---------------------------------------------------------------- the query list of the set tests
def set_queries(num_terms, seed=0x5E70):
    """Queries over the high-df terms of a helpers.small_params collection (term 0, half of all documents, left out: its idf is
    near 0): 50 of at most two distinct terms (single terms, repeats, pairs among terms 1 .. 30), 46 of three to five among terms
    1 .. 9 (their conjunctions still hold dozens of documents), and a few wide ones of 6, 9 and 16 terms for the unions. No query has
    more than 16 distinct terms: one such query sends its whole batch to the one-document-per-step kernels (one kernel family per
    batch), which sum a document's terms in each operator's own order, so that wand and ranked_or of ONE index differ in a last bit
    there (test_gpu_topk_docs.py says so) and the stream kernels, which the sets are for, would not run at all. The query of more than
    16 terms is among the edges (test_gpu_shards.py::test_edges)."""
    rng = np.random.default_rng(seed)
    pick = lambda lo, hi, m: [int(t) for t in lo + rng.choice(hi - lo, m, replace=False)]  # noqa: E731
    qs = [[t] for t in (1, 2, 5, 17, 30)] + [[3, 3], [9, 9, 9], [4, 7, 4]]
    qs += [pick(1, 31, 2) for _ in range(42)]
    qs += [pick(1, 10, 3) for _ in range(30)] + [pick(1, 10, 4) for _ in range(10)] + [pick(1, 10, 5) for _ in range(6)]
    qs += [pick(1, min(num_terms, 41), m) for m in (6, 9, 16)]
    return qs


def distinct_terms(q):
    return len(set(q))


def set_conditions(coll, shards, queries, k):
    """what the issue asks of the query list, from the numpy reference alone: (queries of at most two distinct terms, queries of three or
    more, share of the ranked_and queries that return k results, share of all ranked_and rows whose top-k comes from more than one
    shard)"""
    from topk_docs_ref import brute_pairs
    shard_of_doc = np.full(coll.num_docs, -1, dtype=np.int64)
    for s, sh in enumerate(shards):
        shard_of_doc[sh[2]] = s
    small = sum(1 for q in queries if distinct_terms(q) <= 2)
    full = multi = 0
    for q in queries:
        _, docs = brute_pairs(coll, q, k, True)
        full += len(docs) == k
        multi += len(set(shard_of_doc[docs].tolist())) > 1
    return small, len(queries) - small, full / len(queries), multi / len(queries)


# ---------------------------------------------------------------- a small collection where equal scores are the norm
def small_tie_collection(seed=0x71E7):
    """6000 documents of three sizes, freqs from {1, 2, 3} (skewed to 1), 24 terms of 300 to 3000 postings over a common core: as
    helpers.tie_collection at a scale a test runs in a second. A query sees a few dozen distinct scores, so almost every k-th place is
    tied; cut round-robin, the equal scores interleave across the shards."""
    def make():
        from helpers import Collection
        rng = np.random.default_rng(seed)
        n = 6000
        sizes = rng.choice(np.array([60, 150, 400], dtype=np.uint32), n)
        fr = np.array([1, 1, 1, 2, 3], dtype=np.uint32)
        core = np.unique(rng.integers(0, n, 400))
        core_freq = rng.choice(fr, len(core))
        lists = []
        for i in range(24):
            m = int(round(300 * (10 ** (i / 23))))
            own = np.setdiff1d(np.unique(rng.integers(0, n, m)), core, assume_unique=True)
            docs = np.concatenate([core, own])
            freqs = np.concatenate([core_freq, rng.choice(fr, len(own))])
            o = np.argsort(docs, kind="stable")
            lists.append((docs[o], freqs[o]))
        return Collection.from_lists(n, lists, sizes)
    return _once(("small_tie", seed), make)


def small_tie_queries(seed=0x71E8):
    rng = np.random.default_rng(seed)
    qs = [[t] for t in (0, 5, 11, 23)] + [[7, 7], [2, 2, 19]]
    qs += [[int(t) for t in rng.choice(24, 2, replace=False)] for _ in range(40)]
    qs += [[int(t) for t in rng.choice(24, 3, replace=False)] for _ in range(6)]
    return qs
