"""The explicit collections of the Elias-Fano encoder's tests (test_gpu_freq_encode.py, test_freq_encode_abi_cpu.py): posting lists
that reach every branch of the layouts -- one-partition headers, all-ones / ranked-bitvector / Elias-Fano base sequences with and
without their sampled arrays, prefix sums past 2^32."""
import numpy as np

from helpers import Collection

NUM_DOCS = 1 << 20
EDGE_LENGTHS = (1, 2, 127, 128, 129, 256, 257)
DENSE_NUM_DOCS = 3000


def edge_collection(seed=0xEF0A):
    """(collection over 2^20 documents, names: what a test asks for -> its term)"""
    rng = np.random.default_rng(seed)
    n = NUM_DOCS
    lists, names = [], {}

    def add(name, docs, freqs):
        names[name] = len(lists)
        lists.append((np.sort(np.asarray(docs)).astype(np.uint32), np.asarray(freqs, dtype=np.uint32)))

    for m in EDGE_LENGTHS:
        add("len%d" % m, rng.choice(n, m, replace=False), rng.integers(1, 40, m))
    add("run", np.arange(70000, 70000 + 700), rng.integers(1, 5, 700))          # n == universe of its partitions: all ones
    add("every_second", np.arange(100, 100 + 3000, 2), rng.integers(1, 9, 1500))  # ranked bitvector: 3000 positions, 1500 ones
    add("sparse", rng.choice(1000000, 2000, replace=False), rng.integers(1, 6, 2000))  # Elias-Fano, both pointer arrays (ef / single)
    add("to_the_end", np.concatenate([rng.choice(n - 1, 299, replace=False), [n - 1]]), rng.integers(1, 4, 300))  # delta(0) header
    add("last_only", [n - 1], [1])
    add("ones", rng.choice(n, 1000, replace=False), np.ones(1000))               # strict all ones
    add("twos", rng.choice(n, 1500, replace=False), np.full(1500, 2))            # strict ranked bitvector with pointers1
    add("big_f", [5, 77, 900000], np.full(3, 1 << 31))                           # prefix sums pass 2^32
    return Collection.from_lists(n, lists, np.full(n, 100, dtype=np.uint32)), names


def dense_collection(seed=0xEF0B):
    """3 000 documents: lists dense enough in the WHOLE universe that `single` takes its ranked bitvector (with rank1_samples and
    pointers1) and its all-ones form, and that `ef` has no low bits"""
    rng = np.random.default_rng(seed)
    n = DENSE_NUM_DOCS
    lists = [(np.arange(0, n, 2), rng.integers(1, 4, n // 2)),
             (np.arange(n), np.ones(n)),
             (np.arange(1, n, 3), np.full(len(np.arange(1, n, 3)), 2)),
             (np.sort(rng.choice(n, 2000, replace=False)), rng.integers(1, 3, 2000))]
    return Collection.from_lists(n, lists, rng.integers(20, 400, n).astype(np.uint32))
