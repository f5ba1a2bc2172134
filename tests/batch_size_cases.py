"""The batch dimension: one collection, about 150 distinct queries, and batches of every size at which the planner
(ds2i_amd/csrc/batch_plan.cpp) or the slot (capi_batch.cpp) changes what it does (SIZES), up to LARGE = 36 000 queries, whose list-stream records need a second launch
slice of 32768 (launch_list_streams). tests/test_batch_size_cases_cpu.py proves that the batches are what they claim,
tests/test_gpu_batch_sizes.py runs them.

A batch of nq queries is distinct[pick[i]] for a seeded array pick, so every reference is computed once per distinct query (reference())
and expanded by index. All references are CPU: oracle.Index.query_batch (counts, freq sums, top-k, lengths), helpers.brute_and / brute_or
(counts, doc-id lists) and topk_docs_ref.brute_pairs (ranked_and scores and doc-ids); none comes from the code under test.

Collection: 2^17 documents, 24 lists. Terms 0 .. 13 are sparse (3 .. 2047 postings: 64 * n < num_docs, no bitmap; 2047 is the last
length without one), terms 14 .. 19 short and dense (2048 .. 4096 postings: they carry bitmaps and are cheap to stream 36 000 times),
terms 20 .. 23 long (23 k .. 58 k postings, 180 .. 454 blocks: a small batch splits their queries into several units, a large one
leaves them whole). Every list of 127 postings and more holds a common core of 48 documents and every list of 17 and more a second
one of 5, so that conjunctions of many lists are not empty and some hold fewer than k documents. Document sizes as in
test_gpu_unit_taper._collection."""
import functools

import numpy as np

from helpers import Collection, brute_and, brute_or
from topk_docs_ref import brute_pairs

NUM_DOCS = 1 << 17
SPARSE_SIZES = [3, 17, 40, 64, 127, 128, 129, 200, 300, 513, 650, 777, 900, 2047]
DENSE_SIZES = [2048, 2300, 2700, 3100, 3600, 4096]
# (lengths at which numpy's float32 log gives the oracle's query weights bit for bit: the CPU test asserts it)
LONG_SIZES = [23000, 34000, 46000, 58000]
SIZES_OF_LISTS = SPARSE_SIZES + DENSE_SIZES + LONG_SIZES
SPARSE = list(range(0, 14))
DENSE = list(range(14, 20))
LONG = list(range(20, 24))
OPS = ["and", "and_freq", "or", "or_freq", "ranked_and", "wand", "maxscore", "ranked_or"]
UNION = ["wand", "maxscore", "ranked_or"]
KS = {"ranked_and": (10, 65, 257), "wand": (10, 65, 257), "maxscore": (10, 65), "ranked_or": (10, 65)}  # what reference() holds
K_MAX = 257
SLICE = 32768  # terms per launch of k_and_stream / k_freq_stream (launch_list_streams: grid.y is limited)
LARGE = 36000

# batch sizes, each beside the expression of batch_plan.cpp / capi_batch.cpp it straddles
SIZES = [
    0,     # the `nq == 0` and `nq ? nq : 1` guards (lay_out, copy_results): no query at all
    1,     # ... and the smallest batch there is
    2,
    63,    # one wavefront of queries less one (no planner expression: the kernels' own 64)
    64,
    65,
    511,   # cut_units: all_cost *= min(min(nq <= 512 ? 3 : 2, pool_batches), max(1, 4096 / nq))
    512,
    513,
    1023,  # plan_queries: nchunks = nq >= 1024 ? min(plan_threads, 16) : 1
    1024,
    1025,
    1535,  # cut_units: unit factor nq < 1536 ? 2.0 : 4.0, taper_batch = ... nq >= 1536
    1536,
    1537,
    2047,  # pipeline_launch: alt_streams = (slot & 1) && nq < 2048
    2048,
    2049,
    4095,  # cut_units: max(1, 4096 / nq) reaches 1
    4096,
    4097,
    LARGE,  # launch_list_streams: for (t0 = 0; t0 < n; t0 += 32768), over sterms and over qterms
]
THRESHOLDS = [64, 512, 1024, 1536, 2048, 4096]
CHUNKINGS = (3, 4, 16)      # DS2I_PLAN_THREADS of the uploads of the planning-chunk checks
CHUNKED_SIZES = (1024, 1025, LARGE)  # the batches that carry the special queries at their chunk boundaries


def has_bitmap(n, num_docs=NUM_DOCS):
    """RmwLevels::has_bitmap (ds2i_amd/csrc/device_enum.hpp): a list of one document in 64 or more carries its exact bitmap"""
    return 64 * n >= num_docs


@functools.lru_cache(maxsize=None)
def collection():
    rng = np.random.default_rng(0xBA7C4)
    core = np.sort(rng.choice(NUM_DOCS, 48, replace=False))
    core2 = np.sort(rng.choice(np.setdiff1d(np.arange(NUM_DOCS), core), 5, replace=False))
    lists = []
    for n in SIZES_OF_LISTS:
        fixed = np.concatenate([core if n >= 127 else core[:0], core2 if n >= 17 else core2[:0]])
        rest = rng.choice(np.setdiff1d(np.arange(NUM_DOCS), fixed), n - len(fixed), replace=False)
        docs = np.sort(np.concatenate([fixed, rest])).astype(np.uint32)
        lists.append((docs, rng.integers(1, 9, n).astype(np.uint32)))
    return Collection.from_lists(NUM_DOCS, lists, rng.integers(50, 500, NUM_DOCS))


# the three special queries of the chunk boundaries (indexes into distinct_queries() are looked up by value)
EMPTY = []
OVER16 = list(range(4, 21))               # 17 distinct terms
OVER16_DUP = list(range(2, 22)) + [7]     # 20 distinct terms, one of them twice
DUP = [3, 9, 3]
D4 = [14, 15, 16, 17]                     # the all-dense 4-term query LARGE's slice boundaries fall into


@functools.lru_cache(maxsize=None)
def distinct_queries():
    rng = np.random.default_rng(0xBA7C5)
    pick = lambda pool, m: [int(t) for t in rng.choice(pool, m, replace=False)]
    qs = [EMPTY]
    qs += [[t] for t in range(24)]                                                      # one term: sparse, dense, long
    qs += [[5, 5], [15, 15], DUP, [16, 8, 16], [21, 21], [14, 14, 17], [20, 13, 20, 13]]  # duplicated terms
    qs += [[14, 15], [16, 19], [17, 18], [14, 19], [15, 17]]                            # all dense: 2,
    qs += [[14, 16, 18], [15, 17, 19], [14, 15, 19], [16, 17, 18]]                      # 3
    qs += [D4, [16, 17, 18, 19], [14, 16, 18, 19]]                                      # and 4 terms
    # 2 .. 4 terms, the shortest list sparse and the others dense: a list stream for `and`, units for and_freq
    qs += [[12, 19], [0, 14], [1, 14], [13, 14], [9, 16, 18], [13, 15, 19], [4, 17, 18, 19], [12, 14, 15, 16]]
    qs += [[11, 12], [12, 13, 19], [8, 10, 17], [6, 7, 15, 16], [11, 12, 13, 14], [13, 12], [2, 3], [0, 1]]  # two sparse lists: units
    for n in range(5, 17):                                                              # every length 5 .. 16
        qs += [pick(list(range(4, 20)), n), pick(list(range(4, 24)), n)]
    qs += [OVER16, OVER16_DUP]                                                          # more than 16 terms
    # over the long lists: split by small batches
    qs += [[a, b] for i, a in enumerate(LONG) for b in LONG[i + 1:]]
    qs += [[20, 21, 22], [21, 22, 23], [20, 22, 23], [20, 21, 22, 23], [13, 23], [19, 22], [12, 20, 23], [18, 19, 21], [10, 17, 22, 23],
           [20, 21, 22, 23, 19], [13, 20, 21, 22, 23, 18]]
    while len(qs) < 150:                                                                # random fill, 2 .. 4 terms
        q = pick(list(range(24)), int(rng.integers(2, 5)))
        if q not in qs:
            qs.append(q)
    assert len({tuple(q) for q in qs}) == len(qs)
    return [list(q) for q in qs]


def index_of(q):
    return distinct_queries().index(list(q))


def stream_records(q, op):
    """records the planner adds to the list streams for query q of an `and` / and_freq batch (add_list_streams, cut_units): a one-term
    query gives one; a query of 2 .. 4 distinct terms whose lists (`and`: except its shortest) all carry a bitmap gives one (`and`) or
    one per distinct term (and_freq); every other query gives none, and gets work units"""
    ts = sorted(set(q), key=lambda t: (SIZES_OF_LISTS[t], t))
    if len(ts) == 1:
        return 1
    if 2 <= len(ts) <= 4 and all(has_bitmap(SIZES_OF_LISTS[t]) for t in (ts[1:] if op == "and" else ts)):
        return len(ts) if op == "and_freq" else 1
    return 0


def distinct_terms(q):
    """query terms the planner keeps for q (plan_range): or_freq streams one record per term of the batch"""
    return len(set(q))


def boundary_positions(nq):
    """both sides of every planning-chunk boundary nq * c / nchunks, nchunks in CHUNKINGS, and the batch's two ends"""
    pos = {0, nq - 1}
    for nchunks in CHUNKINGS:
        for c in range(1, nchunks):
            b = nq * c // nchunks
            pos.update((b - 1, b))
    return sorted(p for p in pos if 0 <= p < nq)


def _place_specials(pick):
    """the empty query, a query of more than 16 terms and a duplicated-term query, in turn, over boundary_positions: the two sides of a
    boundary get two different kinds, and over the boundaries every kind falls on either side"""
    kinds = [index_of(EMPTY), index_of(OVER16), index_of(DUP), index_of(EMPTY), index_of(OVER16_DUP), index_of(DUP)]
    for i, p in enumerate(boundary_positions(len(pick))):
        pick[p] = kinds[i % len(kinds)]  # (three kinds in turn over pairs of positions: every kind on either side)
    return pick


def _crossing(counts, at=SLICE):
    """(query holding record number at - 1, records before it, records up to and including it) for per-query record counts"""
    after = np.cumsum(counts)
    i = int(np.searchsorted(after, at - 1, side="right"))
    return i, int(after[i] - counts[i]), int(after[i])


def _straddle(pick, count_of, lo):
    """Puts D4 where the running count of records passes SLICE, and turns one-term sparse queries between lo and there into the
    all-dense two-term query [14, 15] (one record more for or_freq and for and_freq, the same number for `and`) until D4's records
    lie on both sides of the boundary: records SLICE - 1 and SLICE belong to it. Returns D4's position."""
    d4, two = index_of(D4), index_of([14, 15])
    special = set(boundary_positions(len(pick)))
    one_term = {index_of([t]) for t in SPARSE}
    i, before, _ = _crossing(count_of[pick])
    while i in special:
        i += 1
    pick[i] = d4
    need = (SLICE - 2) - int(np.sum(count_of[pick[:i]]))  # D4 then covers records SLICE - 2 .. SLICE + 1
    j = i - 1
    while need > 0:
        assert j > lo, "no one-term query left to widen"
        if j not in special and int(pick[j]) in one_term:
            pick[j] = two
            need -= 1
        j -= 1
    assert need == 0 or need == -1, need  # (-1: D4 covers SLICE - 1 .. SLICE + 2)
    return i


@functools.lru_cache(maxsize=None)
def pick_of(nq):
    """the seeded pick array of the batch of nq queries (read-only)"""
    qs = distinct_queries()
    rng = np.random.default_rng(0xBA7C6 + nq)
    if nq != LARGE:
        pick = rng.integers(0, len(qs), nq)
        if nq in CHUNKED_SIZES:
            _place_specials(pick)
    else:
        # 94 in 100 are queries every list-stream operator streams and that are cheap to stream: one short list, or 2 .. 4 short dense
        # ones (so that the records of `and`, one per such query, pass SLICE as well); the others are drawn from all distinct queries
        short = set(SPARSE + DENSE)
        cheap = np.array([i for i, q in enumerate(qs) if q and set(q) <= short and stream_records(q, "and_freq") > 0])
        pick = np.where(rng.random(nq) < 0.94, cheap[rng.integers(0, len(cheap), nq)], rng.integers(0, len(qs), nq))
        _place_specials(pick)
        terms = np.array([distinct_terms(q) for q in qs])
        records = np.array([stream_records(q, "and_freq") for q in qs])
        i1 = _straddle(pick, terms, 0)         # or_freq: every term of the batch is a record
        _straddle(pick, records, i1)           # and_freq: fewer records per query, so its boundary falls later
    pick = pick.astype(np.int64)
    pick.setflags(write=False)
    return pick


@functools.lru_cache(maxsize=None)
def batch(nq, over16="as drawn"):
    """(pick, queries, (terms, offsets)) of the batch of nq queries. over16 = "none": every query of more than 16 terms replaced by a
    16-term one; "last": then the last query of the batch replaced by OVER16 -- the only one, and in the last planning chunk."""
    qs = distinct_queries()
    pick = pick_of(nq)
    if over16 != "as drawn":
        pick = pick.copy()
        sixteen = next(i for i, q in enumerate(qs) if len(set(q)) == 16)
        pick[np.isin(pick, [index_of(OVER16), index_of(OVER16_DUP)])] = sixteen
        if over16 == "last" and nq:
            pick[-1] = index_of(OVER16)
        pick.setflags(write=False)
    queries = [qs[i] for i in pick]
    lens = np.array([len(q) for q in qs], dtype=np.int64)[pick] if nq else np.zeros(0, dtype=np.int64)
    offs = np.zeros(nq + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(lens)
    terms = np.array([t for q in queries for t in q] or [0], dtype=np.uint32)
    return pick, queries, (terms, offs)


def large_conditions():
    """What LARGE is built for, from the inputs alone: per operator (records in all, the query in which record SLICE - 1 falls, records
    before that query, records up to and including it, the query itself)."""
    qs = distinct_queries()
    pick = pick_of(LARGE)
    out = {}
    for op, count in (("or_freq", distinct_terms), ("and_freq", lambda q: stream_records(q, "and_freq")), ("and", lambda q: stream_records(q, "and"))):
        per = np.array([count(q) for q in qs])[pick]
        i, before, after = _crossing(per)
        out[op] = (int(per.sum()), i, before, after, qs[pick[i]])
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """Per distinct query, computed once and never changed: numpy's AND doc-id list, OR count and and_freq / or_freq sums; the oracle's
    (count, top-k, lengths) of every ranked operator at the ks of KS; brute_pairs' ranked_and (scores, doc-ids) at K_MAX (a top-k of a
    smaller k is its head). oracle_unranked holds the oracle's counts and freq sums beside numpy's: the CPU test compares the two."""
    import oracle as o
    coll, qs = collection(), distinct_queries()
    ref = {"and_docs": [brute_and(coll, q) for q in qs]}
    ref["and"] = np.array([len(m) for m in ref["and_docs"]], dtype=np.uint64)
    ref["or"] = np.array([len(brute_or(coll, q)) for q in qs], dtype=np.uint64)
    and_freq, or_freq = [], []
    for q, both in zip(qs, ref["and_docs"]):
        ts = sorted(set(q))
        and_freq.append(sum(int(coll.lists[t][1][np.searchsorted(coll.lists[t][0], both)].sum()) for t in ts) if len(both) else 0)
        or_freq.append(sum(int(coll.lists[t][1].sum(dtype=np.uint64)) for t in ts))
    ref["and_freq"], ref["or_freq"] = np.array(and_freq, dtype=np.uint64), np.array(or_freq, dtype=np.uint64)
    oidx = o.Index("block_optpfor", coll.index_image("block_optpfor"), coll.wand_image())
    ref["oracle_unranked"] = {}
    for op in ("and", "and_freq", "or", "or_freq"):
        count, _, _, fsum, _ = oidx.query_batch(op, qs)
        ref["oracle_unranked"][op] = (count.copy(), fsum.copy())
    for op, ks in KS.items():
        for k in ks:
            count, topk, tlen, _, _ = oidx.query_batch(op, qs, k=k)
            ref[(op, k)] = (count.copy(), topk.copy(), tlen.copy())
    oidx.close()
    ref["brute"] = [brute_pairs(coll, q, K_MAX, True) for q in qs]
    for v in ref.values():
        for a in (v if isinstance(v, (tuple, list)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def brute_docs(k):
    """uint32[distinct, k]: brute_pairs' ranked_and doc-ids, 0xFFFFFFFF past the length"""
    brute = reference()["brute"]
    docs = np.full((len(brute), k), 0xFFFFFFFF, dtype=np.uint32)
    for i, (_, bd) in enumerate(brute):
        n = min(k, len(bd))
        docs[i, :n] = bd[:n]
    docs.setflags(write=False)
    return docs
