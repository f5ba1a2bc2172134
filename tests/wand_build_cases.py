"""The collections of the wand_data build tests (test_gpu_build_wand.py, test_build_wand_abi_cpu.py): explicit posting lists whose
maximum-weight posting sits where a per-block reduction can lose it, and a numpy restatement of wand_data's max_term_weight."""
import numpy as np

from helpers import Collection, doc_term_weight

NUM_DOCS = 70000
EDGE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 128 * 37 + 5)
FLAT = (1000, 4000)      # documents of one size: inside a list over them the freq alone orders the weights
FLAT_SIZE = 100
SHORT_DOCS = (0, 7, 31234)  # length 1: the smallest norm_len
LONG_DOC = NUM_DOCS - 1     # one very long document: the largest norm_len
# crafted lists over FLAT, freq 1 but for the named postings (freq 7): name -> (length, positions of the maximum)
PLACED = {"first": (300, (0,)), "tail_last": (128 * 2 + 37, (128 * 2 + 36,)), "full_block_last": (128 * 3 + 10, (255,)),
          "tie_two_blocks": (128 * 3, (5, 128 * 2 + 77))}

EDGE = 1 << 24
BIG_NUM_DOCS = EDGE + (1 << 18)
BIG_LONG = 320000


def max_term_weight(coll, t):
    """(maximum, positions that reach it) of list t: float32 arithmetic of bm25.hpp over the collection's float32 norm_lens"""
    docs, freqs = coll.lists[t]
    w = doc_term_weight(freqs, coll.norm_lens[docs])
    m = np.float32(max(np.float32(0), w.max()))
    return m, np.flatnonzero(w == m)


def image_max_term_weights(image, num_docs, nlists):
    """the max_term_weight array of a wand_data image: u64 N | float norm_lens[N] | u64 V | float max_term_weight[V]"""
    assert int(np.frombuffer(image[:8], dtype=np.uint64)[0]) == num_docs
    at = 8 + 4 * num_docs
    assert int(np.frombuffer(image[at:at + 8], dtype=np.uint64)[0]) == nlists and len(image) == at + 8 + 4 * nlists
    return np.frombuffer(image[at + 8:], dtype=np.float32)


def small_collection(seed=0x3A2D):
    """About 300 lists over 70 000 documents. Document lengths are skewed (log-normal; a few of length 1, one of three
    million), so norm_len runs from about 0.004 to about 10^4. Returns (collection, names): names maps what a test asks for to
    its term -- the lengths of EDGE_LENGTHS ("len<n>"), the crafted lists of PLACED, "ones" (freq 1 everywhere, holds the
    shortest and the longest document), "big_f" (freqs up to 2^31 - 2, as test_gpu_encode_is_byte_identical's list)."""
    rng = np.random.default_rng(seed)
    n = NUM_DOCS
    sizes = np.maximum(1, rng.lognormal(5.0, 1.2, n)).astype(np.uint32)
    sizes[FLAT[0]:FLAT[1]] = FLAT_SIZE
    sizes[list(SHORT_DOCS)] = 1
    sizes[LONG_DOC] = 3000000
    lists, names = [], {}

    def add(name, docs, freqs):
        if name:
            names[name] = len(lists)
        lists.append((np.sort(np.asarray(docs)).astype(np.uint32), np.asarray(freqs, dtype=np.uint32)))

    def draw(m):
        return rng.choice(n, m, replace=False)

    for m in EDGE_LENGTHS:
        add("len%d" % m, draw(m), rng.integers(1, 40, m))
    for name, (m, at) in PLACED.items():
        f = np.ones(m, dtype=np.uint32)
        f[list(at)] = 7
        add(name, FLAT[0] + rng.choice(FLAT[1] - FLAT[0], m, replace=False), f)
    ends = np.array(SHORT_DOCS + (LONG_DOC,))
    docs = np.union1d(draw(5000), ends)
    add("ones", docs, np.ones(len(docs), dtype=np.uint32))
    m = 128 * 3 + 5
    big_f = rng.integers(1, (1 << 31) - 2, m).astype(np.uint32)
    big_f[384:] = rng.integers(1, 1 << 20, m - 384)
    big_f[200] = (1 << 31) - 2
    add("big_f", draw(m), big_f)
    # the body: Zipf-like lengths from a few postings to most of the collection, small freqs; some hold the extreme documents
    while len(lists) < 300:
        m = int(min(n * 0.8, 3 + 40000 / (1 + len(lists) - len(names)) ** 0.9 * rng.uniform(0.5, 1.5)))
        docs = draw(m)
        if len(lists) % 9 == 0:
            docs = np.union1d(docs, ends)
        add(None, docs, rng.geometric(0.45, len(docs)))
    return Collection.from_lists(n, lists, sizes), names


def small_queries(coll, nq=64, seed=0x3A2E):
    """nq queries of 1 .. 4 distinct terms over the small collection"""
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.choice(len(coll.lists), int(rng.integers(1, 5)), replace=False)] for _ in range(nq)]


def big_collection(seed=0x3A2F):
    """2^24 + 2^18 documents of a few sizes (a cut-down helpers.tie_collection): one list of BIG_LONG postings over the whole
    universe (2 500 blocks, on both sides of 2^24), four lists in a window around 2^24, and `straddle`: the four neighbours
    2^24 - 1 .. 2^24 + 2 with freq 1, of which only 2^24 + 1 is short -- a doc-id that passed through a float32 would land on
    an even neighbour and on another norm_len. Returns (collection, names)."""
    rng = np.random.default_rng(seed)
    n = BIG_NUM_DOCS
    sizes = rng.choice(np.array([60, 150, 151, 400, 2000], dtype=np.uint32), n)
    sizes[EDGE - 1:EDGE + 3] = (400, 400, 3, 400)
    names = {"long": 0, "straddle": 1}
    lists = [(np.unique(rng.integers(0, n, BIG_LONG + 4000))[:BIG_LONG + 1000], None),
             (np.arange(EDGE - 1, EDGE + 3), None)]
    for m in (2000, 128 * 40, 20001, 60000):
        lists.append((np.unique(rng.integers(EDGE - 5000, n, m)), None))
    lists = [(dd, np.ones(len(dd), dtype=np.uint32) if i == 1 else rng.choice(np.array([1, 1, 1, 2, 3], dtype=np.uint32), len(dd)))
             for i, (dd, _) in enumerate(lists)]
    assert len(lists[0][0]) >= BIG_LONG and lists[0][0][0] < EDGE < lists[0][0][-1]
    return Collection.from_lists(n, lists, sizes), names
