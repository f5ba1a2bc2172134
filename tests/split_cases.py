"""The assignments and inputs of the split tests (test_split_abi_cpu.py, test_gpu_split.py), and the numpy reference of the semantics of
ds2i_split_postings: shard s holds the documents d with shard_of[d] == s in increasing old id (local id = rank among them, doc_map the
old ids), a list survives in a shard if one of its postings lies there (term_map the old terms), postings keep their order and freqs.
A shard is the tuple the API returns: (num_docs, lists, doc_map, term_map). merge_cases.range_shards / round_robin_shards state the same
semantics independently for range and round-robin assignments: from_merge_shards turns theirs into such tuples. Everything is integers
and every answer is unique: all comparisons are exact."""
import numpy as np

import merge_cases as mc
import remap_cases as rc
import verify_cases as cases
from helpers import Collection

DROP = 0xFFFFFFFF
EDGE_CUTS = (7300, 30001)  # (the first cut lies inside the run of 700 consecutive doc-ids)
FREQ_EDGE_CUTS = (70350, 600000)
_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def numpy_split(num_docs, lists, shard_of, nshards):
    """the reference: a list of (num_docs, lists, doc_map, term_map), one per shard"""
    shard_of = np.asarray(shard_of, dtype=np.uint32)
    assert len(shard_of) == num_docs
    out = []
    for s in range(nshards):
        mine = shard_of == s
        doc_map = np.flatnonzero(mine).astype(np.uint32)
        local = np.cumsum(mine) - 1
        kept, terms = [], []
        for t, (dd, ff) in enumerate(lists):
            keep = mine[dd]
            if keep.any():
                kept.append((local[dd[keep]].astype(np.uint32), np.asarray(ff, dtype=np.uint32)[keep]))
                terms.append(t)
        out.append((len(doc_map), kept, doc_map, np.array(terms, dtype=np.uint32)))
    return out


def assert_shards_equal(got, want):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "documents of shard %d" % s
        for k, what in ((2, "doc map"), (3, "term map")):
            assert g[k].dtype == np.uint32 and np.array_equal(g[k], w[k]), "%s of shard %d" % (what, s)
        rc.assert_lists_equal(g[1], w[1])


def range_assign(num_docs, cuts):
    return np.searchsorted(np.asarray(cuts), np.arange(num_docs), side="right").astype(np.uint32)


def round_robin_assign(num_docs, k, group=1):
    return ((np.arange(num_docs) // group) % k).astype(np.uint32)


def random_assign(num_docs, k, drop=0.1, seed=0x5B117):
    """seeded shard numbers, about `drop` of the documents deleted"""
    def make():
        rng = np.random.default_rng(seed)
        m = rng.integers(0, k, num_docs).astype(np.uint32)
        m[rng.random(num_docs) < drop] = DROP
        return m
    return _once(("random", num_docs, k, drop, seed), make)


def from_merge_shards(shards):
    """merge_cases' shards as split tuples; a default doc map is the range after the documents of the earlier shards"""
    base = mc.bases(shards)
    return [(s.num_docs, s.lists, s.doc_map if s.doc_map is not None else (np.arange(s.num_docs, dtype=np.int64) + base[i]).astype(np.uint32),
             s.term_map) for i, s in enumerate(shards)]


def merge_sources(shards):
    """split tuples as the `sources` of merge_postings"""
    return [(n, lists, doc_map, term_map) for n, lists, doc_map, term_map in shards]


def shard_image(name, coll, shard, kind):
    """the host builder's image of one shard (a split tuple) of `coll`; `name` says which shard of which split of which collection it
    is, e.g. ("edge", "range", 1): the shard's collection is built once under that name"""
    n, lists, doc_map, _ = shard
    return cases.image(_once(("shard collection",) + tuple(name), lambda: Collection.from_lists(n, lists, coll.sizes[doc_map])), kind)


# ---------------------------------------------------------------- many short lists
SHORT_LISTS = 6000
SHORT_NUM_DOCS = 4001


def short_lists_collection():
    """6000 lists of 1, 2 and 3 postings in turn (12 000 postings) whose doc-ids are drawn from all 4001 documents, odd and even alike:
    a window of W postings of the device split spans about W / 2 list starts, and the parity of the doc-id really splits them: a list
    of one posting lies in one of the two shards only."""
    def make():
        rng = np.random.default_rng(0x5407)
        lists = []
        for t in range(SHORT_LISTS):
            m = 1 + t % 3
            lists.append((np.sort(rng.choice(SHORT_NUM_DOCS, m, replace=False)).astype(np.uint32), rng.integers(1, 40, m).astype(np.uint32)))
        return Collection.from_lists(SHORT_NUM_DOCS, lists, rng.integers(20, 400, SHORT_NUM_DOCS).astype(np.uint32))
    return _once("short_lists", make)


def list_starts_per_window(lists, W):
    """how many lists start in every window of W postings of the concatenated postings"""
    starts = np.cumsum([0] + [len(dd) for dd, _ in lists])
    return np.bincount(starts[:-1] // W, minlength=-(-int(starts[-1]) // W))


# ---------------------------------------------------------------- the window edges of the device split
KEEPS = ("all", "none_in_one_window", "every_other", "first_lane", "last_lane", "last_of_window", "first_of_next_window")


def window_edge_lists(W, whole_windows):
    """(num_docs, lists): lists of 1, 63, 64, 65, W - 1, W, W + 1, 2 W + 1 and 3 W - 1 postings and an empty one between two of them.
    The list of W comes first, so the second list starts exactly on a window boundary as the first does; all others start in
    mid-window. whole_windows: one more list fills the last window, so that the end of the postings is a window boundary too.
    Posting i of the concatenation lies in document 2 i + 1: every posting has a document of its own, and every even document none."""
    def make():
        lengths = [W, 1, 63, 0, 64, 65, W - 1, W + 1, 2 * W + 1, 3 * W - 1]
        if whole_windows:
            lengths.append(-sum(lengths) % W or W)
        total = sum(lengths)
        assert (total % W == 0) == whole_windows
        starts = np.cumsum([0] + lengths)[:-1]
        assert sum(1 for s in starts if s % W == 0) >= 2 and sum(1 for s in starts if s % W) >= 6
        rng = np.random.default_rng(0x5E1D + W)
        lists, first = [], 0
        for n in lengths:
            i = np.arange(first, first + n)
            lists.append(((2 * i + 1).astype(np.uint32), rng.integers(1, 40, n).astype(np.uint32)))
            first += n
        return 2 * total + 3, lists
    return _once(("window_edges", W, whole_windows), make)


def window_edge_assign(W, num_docs, keep, nshards, drops):
    """shard_of for window_edge_lists: the posting positions `keep` names stay in shard 0, the other postings are dealt out among the
    other shards (dropped when there is none, and every fifth of them when `drops`); the documents without a posting are dealt out
    among all shards, so that every shard has documents."""
    total = (num_docs - 3) // 2
    i = np.arange(total)
    kept = {"all": np.ones(total, dtype=bool), "none_in_one_window": i // W != 1, "every_other": i % 2 == 0, "first_lane": i % 64 == 0,
            "last_lane": i % 64 == 63, "last_of_window": i % W == W - 1, "first_of_next_window": i % W == 0}[keep]
    of_posting = np.where(kept, 0, 1 + i % max(nshards - 1, 1)).astype(np.uint32)
    gone = ~kept & (i % 5 == 0) if drops and nshards > 1 else ~kept & (nshards == 1)
    of_posting[gone] = DROP
    shard_of = (np.arange(num_docs) // 2 % nshards).astype(np.uint32)
    shard_of[2 * i + 1] = of_posting
    return shard_of


# ---------------------------------------------------------------- doc-ids past 2^24
PAST_2_24 = mc.PAST_2_24


def past_2_24_case():
    """(num_docs, lists, shard_of): the three-posting lists of the first source of merge_cases.past_2_24_sources over 2^24 + 5
    documents; the documents past 2^24 alternate between two shards, those below are all shard 0's but two, one of them dropped"""
    def make():
        src = mc.past_2_24_sources(False)[0]
        shard_of = np.zeros(PAST_2_24, dtype=np.uint32)
        shard_of[1 << 24:] = np.arange(PAST_2_24 - (1 << 24)) % 2
        shard_of[(1 << 24) - 1] = 1
        shard_of[5] = DROP
        return src.num_docs, src.lists, shard_of
    return _once("past", make)
