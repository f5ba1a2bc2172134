"""The collections of the partition planner's tests (test_opt_partition_abi_cpu.py, test_gpu_opt_partition.py): the lists of
freq_encode_cases.py and the small synthetic collection, and `window_collection`: lists that drive the windows of the opt DP
(host_pef.hpp: optimal_partition) -- a window that never closes, windows of different classes that end at different places, a list
longer than 2^16, lengths around a wavefront, a list whose budget list breaks off early.

Every collection and the host planner's answer for it are built once per process (functools.lru_cache) and must not be modified."""
import functools

import numpy as np

import ds2i_amd as d
import freq_encode_cases as cases
from helpers import Collection, small_params

WINDOW_NUM_DOCS = 1 << 24
WINDOW_LENGTHS = (1, 2, 3, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def window_collection(seed=0x0B7A):
    """(collection over 2^24 documents, names: what a test asks for -> its term)"""
    rng = np.random.default_rng(seed)
    n = WINDOW_NUM_DOCS
    lists, names = [], {}

    def add(name, docs, freqs):
        names[name] = len(lists)
        lists.append((np.asarray(docs).astype(np.uint32), np.asarray(freqs, dtype=np.uint32)))

    def random_docs(lo, hi, m):
        return np.sort(rng.choice(hi - lo, m, replace=False)) + lo

    # a consecutive run costs fix_cost at any length: both sides are all ones and no window ever closes
    add("long_run", np.arange(123456, 123456 + 6000), np.ones(6000))
    add("run_in_sparse", np.concatenate([random_docs(0, 4000000, 500), np.arange(5000000, 5000000 + 3000), random_docs(6000000, n, 500)]),
        rng.integers(1, 6, 4000))
    # 100 times: 40 postings at gaps of 1-2, then 40 at gaps of 2000-4000 (4 000 such gaps end below 2^24; gaps of one width make
    # the DP cut the same two sizes over and over): many partitions of many sizes, and the windows of different classes end at
    # different places
    gaps = np.concatenate([np.concatenate([rng.integers(1, 3, 40), rng.integers(2000, 4001, 40)]) for _ in range(100)])
    add("clusters", np.cumsum(gaps), rng.integers(1, 6, 8000))
    add("long", random_docs(0, n, 70000), rng.integers(1, 6, 70000))  # longer than 2^16
    for m in WINDOW_LENGTHS:
        add("len%d" % m, random_docs(0, n, m), rng.integers(1, 40, m))
    add("few_classes", [1000, 1001, 1003], [1, 1, 2])  # cost(universe, n) is below most budgets: the budget list breaks off early
    return Collection.from_lists(n, lists, np.full(n, 100, dtype=np.uint32)), names


@functools.lru_cache(maxsize=None)
def edge_collection():
    return cases.edge_collection()


@functools.lru_cache(maxsize=None)
def dense_collection():
    return cases.dense_collection()


@functools.lru_cache(maxsize=None)
def small_collection():
    """the 300 synthetic lists of test_gpu_freq_encode.py, every fourth clustered"""
    return Collection(small_params(num_docs=20000, num_terms=300, clustered_every=4))


COLLECTIONS = {"window": lambda: window_collection()[0], "edge": lambda: edge_collection()[0], "dense": dense_collection,
               "small": small_collection}


@functools.lru_cache(maxsize=None)
def host_partitions(name):
    """opt_partition (the host DP) of COLLECTIONS[name]: (docs_ends, docs_offs, freqs_ends, freqs_offs)"""
    coll = COLLECTIONS[name]()
    return d.opt_partition(coll.num_docs, coll.lists)


def ends_of(parts, side, t):
    """the end points of list t on side 0 (docs) / 1 (freqs)"""
    ends, offs = parts[2 * side], parts[2 * side + 1]
    return ends[int(offs[t]):int(offs[t + 1])]
