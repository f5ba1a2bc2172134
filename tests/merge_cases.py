"""The shards and sources of the merge tests (test_merge_abi_cpu.py, test_gpu_merge.py), and the numpy reference: the mapped postings of
every source list sent to a term concatenated, then sorted by argsort. A source is a Shard: its number of documents, its lists, and the
two optional maps of the C ABI (doc_map None: after the documents of the earlier sources; term_map None: the same terms). Doc-ids are
distinct across sources, so every merged list is unique and every comparison is exact."""
import collections

import numpy as np

import remap_cases as rc
import verify_cases as cases
from helpers import Collection

Shard = collections.namedtuple("Shard", "num_docs lists doc_map term_map sizes")
_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _shard(num_docs, per_term, doc_map, sizes):
    """per_term: the shard's (docs, freqs) of every term of the whole collection, possibly empty: empty ones are dropped"""
    kept = [t for t, (dd, _) in enumerate(per_term) if len(dd)]
    assert kept, "every shard keeps at least one list"
    lists = [(per_term[t][0].astype(np.uint32), per_term[t][1].astype(np.uint32)) for t in kept]
    return Shard(int(num_docs), lists, doc_map, np.array(kept, dtype=np.uint32), np.asarray(sizes, dtype=np.uint32))


def _all_terms_survive(shards, num_terms):
    seen = np.zeros(num_terms, dtype=bool)
    for s in shards:
        seen[s.term_map] = True
    assert seen.all(), "every term survives in some shard"
    return shards


def range_shards(coll, cuts):
    """contiguous doc ranges [0, cuts[0]), [cuts[0], cuts[1]), ..., [cuts[-1], num_docs), each renumbered from 0; default doc maps.
    Terms with no posting in a shard are dropped from it: its term map says which stayed."""
    def make():
        edges = [0] + list(cuts) + [coll.num_docs]
        assert all(a < b for a, b in zip(edges, edges[1:]))
        shards = []
        for lo, hi in zip(edges, edges[1:]):
            per_term = []
            for dd, ff in coll.lists:
                a, b = np.searchsorted(dd, [lo, hi])
                per_term.append((dd[a:b] - np.uint32(lo), ff[a:b]))
            shards.append(_shard(hi - lo, per_term, None, coll.sizes[lo:hi]))
        return _all_terms_survive(shards, len(coll.lists))
    return _once(("range", id(coll), tuple(cuts)), make)


def round_robin_shards(coll, k, group=1):
    """document d goes to shard d % k as its document d // k; explicit doc maps (local id i of shard s -> i * k + s). group > 1 deals
    the documents out in groups of that many consecutive ids: shard (d // group) % k, the local ids in the order of the old ones."""
    def make():
        shards = []
        for s in range(k):
            doc_map = np.flatnonzero((np.arange(coll.num_docs) // group) % k == s).astype(np.uint32)
            per_term = []
            for dd, ff in coll.lists:
                keep = (dd // group) % k == s
                per_term.append((np.searchsorted(doc_map, dd[keep]), ff[keep]))
            shards.append(_shard(len(doc_map), per_term, doc_map, coll.sizes[doc_map]))
        return _all_terms_survive(shards, len(coll.lists))
    return _once(("rr", id(coll), k, group), make)


def bases(shards):
    return np.concatenate([[0], np.cumsum([s.num_docs for s in shards])]).astype(np.int64)


def num_terms(shards):
    return max(int(s.term_map[-1]) + 1 if s.term_map is not None else len(s.lists) for s in shards)


def numpy_merge(shards, terms=None):
    """(num_docs, merged lists): the reference"""
    terms = num_terms(shards) if terms is None else terms
    base = bases(shards)
    docs, freqs = [[] for _ in range(terms)], [[] for _ in range(terms)]
    for s, sh in enumerate(shards):
        for t, (dd, ff) in enumerate(sh.lists):
            to = t if sh.term_map is None else int(sh.term_map[t])
            new = sh.doc_map[dd] if sh.doc_map is not None else dd.astype(np.int64) + base[s]
            docs[to].append(np.asarray(new, dtype=np.int64))
            freqs[to].append(ff)
    out = []
    for dd, ff in zip(docs, freqs):
        dd, ff = np.concatenate(dd), np.concatenate(ff)
        order = np.argsort(dd, kind="stable")
        out.append((dd[order].astype(np.uint32), ff[order].astype(np.uint32)))
    return int(base[-1]), out


def api_sources(shards):
    """the `sources` of merge_postings / gpu_merge_postings"""
    return [(s.num_docs, s.lists, s.doc_map, s.term_map) for s in shards]


def shard_collection(shard):
    return _once(("coll", id(shard.lists)), lambda: Collection.from_lists(shard.num_docs, shard.lists, shard.sizes))


def image_sources(shards, kinds):
    """the `sources` of gpu_merge_indexes: shard i as a host-built image of kinds[i % len(kinds)]"""
    return [(kinds[i % len(kinds)], cases.image(shard_collection(s), kinds[i % len(kinds)]), s.doc_map, s.term_map) for i, s in enumerate(shards)]


def interleaved_maps(sizes):
    """explicit doc maps that interleave sources of any sizes, each keeping its own order: document d of a source of D goes by the key
    (d + 1/2) / D; with equal sizes this is round robin. Every merged list then is as many sorted runs as it has sources."""
    keys = np.concatenate([(np.arange(n, dtype=np.float64) + 0.5) / n for n in sizes])
    rank = np.empty(len(keys), dtype=np.uint32)
    rank[np.argsort(keys, kind="stable")] = np.arange(len(keys), dtype=np.uint32)
    cut = np.cumsum(sizes)[:-1]
    return np.split(rank, cut)


RUNS = ("1", "63", "64", "65", "127", "128", "129", "L", "L + 1", "2 T + 1")


def class_edge_sources(bounds, interleave):
    """Three sources over the lists of rc.class_edge_lists (their lengths: 1, 2, W - 1, W, W + 1, 127, 128, 129, L - 1, L, L + 1, L + T,
    2 T, 2 T + 1, 3 T - 1). Source 0 holds them all, so its runs have every length of RUNS; source 1 adds a single posting to the list
    of 2 T + 1, a run of L + 1 to the list of one posting and a run of 65 to the list of L; source 2 adds a run of 2 T + 1 to the list
    of 64 and one posting to the list of 3 T - 1. interleave: explicit interleaving doc maps, else the default ones."""
    def make():
        W, L, T = bounds
        whole = rc.class_edge_lists(bounds)
        lengths = [len(dd) for dd, _ in whole]
        for want in (1, 63, 64, 65, 127, 128, 129, L, L + 1, 2 * T + 1):
            assert want in lengths
        rng = np.random.default_rng(0x3E26E)

        def extra(num_docs, runs):
            terms = sorted(runs)
            lists = [(np.sort(rng.choice(num_docs, runs[t], replace=False)).astype(np.uint32), rng.integers(1, 40, runs[t]).astype(np.uint32))
                     for t in terms]
            return num_docs, lists, np.array(terms, dtype=np.uint32)

        n0 = rc.class_edge_num_docs(bounds)
        n1, lists1, terms1 = extra(3 * L, {lengths.index(2 * T + 1): 1, lengths.index(1): L + 1, lengths.index(L): 65})
        n2, lists2, terms2 = extra(4 * T + 7, {lengths.index(64): 2 * T + 1, lengths.index(3 * T - 1): 1})
        maps = interleaved_maps([n0, n1, n2]) if interleave else [None, None, None]
        ones = lambda n: np.ones(n, dtype=np.uint32)  # noqa: E731
        return [Shard(n0, whole, maps[0], None, ones(n0)), Shard(n1, lists1, maps[1], terms1, ones(n1)), Shard(n2, lists2, maps[2], terms2, ones(n2))]
    return _once(("class_edges", tuple(bounds), interleave), make)


PAST_2_24 = (1 << 24) + 5


def past_2_24_sources(reverse):
    """three-posting lists; the first source holds 2^24 + 5 documents, so with default maps every later base lies past 2^24. reverse:
    the reverse of the concatenation as explicit maps, which sends the later sources' documents to the bottom."""
    def make():
        f = np.array([1, 2, 3], dtype=np.uint32)
        sizes = [PAST_2_24, 100, 50]
        lists = [[(np.array([0, (1 << 24) - 1, PAST_2_24 - 1], dtype=np.uint32), f), (np.array([5, 1 << 24, (1 << 24) + 2], dtype=np.uint32), f + 3)],
                 [(np.array([0, 50, 99], dtype=np.uint32), f + 6), (np.array([1, 2, 3], dtype=np.uint32), f + 9)],
                 [(np.array([0, 1, 49], dtype=np.uint32), f + 12)]]
        total = sum(sizes)
        maps = [None, None, None]
        if reverse:
            maps = np.split((total - 1 - np.arange(total, dtype=np.int64)).astype(np.uint32), np.cumsum(sizes)[:-1])
        term_maps = [None, None, np.array([1], dtype=np.uint32)]
        return [Shard(n, ll, m, tm, None) for n, ll, m, tm in zip(sizes, lists, maps, term_maps)]
    return _once(("past", reverse), make)


def assert_merged_equal(got, want):
    assert got[0] == want[0]
    rc.assert_lists_equal(got[1], want[1])


def write_map(path, m):
    rc.write_map(path, m)
