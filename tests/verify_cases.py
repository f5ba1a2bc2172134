"""The collections of the index-verification tests (test_verify_abi_cpu.py, test_gpu_verify.py), ways to alter the EXPECTED postings
(never an image: an altered image can send a decoder anywhere), and a writer of the ds2i binary collection files the tool reads."""
import numpy as np

import freq_encode_cases as fcases
from helpers import Collection, small_params

KINDS = ("block_optpfor", "block_varint", "block_interpolative", "block_qmx", "block_mixed", "opt", "ef", "single", "uniform")
FREQ_KINDS = ("opt", "ef", "single", "uniform")
GPU_BUILT_KINDS = ("block_optpfor", "block_varint", "block_interpolative", "opt", "ef", "single", "uniform")
EDGE_LENGTHS = (1, 2, 127, 128, 129, 256, 257)
EDGE_NUM_DOCS = 50000
GARBAGE = bytes(range(1, 11))  # ten bytes that are no image of any kind
WHAT = ("ok", "num_docs", "lists", "length", "docid", "freq")

_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def small_collection():
    return _once("small", lambda: Collection(small_params(num_docs=20000, num_terms=300, clustered_every=4)))


def block_edge_collection(seed=0x7E21F1):
    """(collection, names): lists of the lengths around the 128-posting block, one run of 700 consecutive doc-ids, and last a list
    that ends with the last document; every freq < 40, so every block codec and the block_mixed policy take it. Every list
    but the run has gaps, so that a doc-id can be altered and the list stay strictly increasing."""
    def make():
        rng = np.random.default_rng(seed)
        n = EDGE_NUM_DOCS
        lists, names = [], {}

        def add(name, docs, freqs):
            names[name] = len(lists)
            lists.append((np.sort(np.asarray(docs)).astype(np.uint32), np.asarray(freqs, dtype=np.uint32)))

        for m in EDGE_LENGTHS:
            add("len%d" % m, 2 * rng.choice(n // 2 - 1, m, replace=False), rng.integers(1, 40, m))  # even doc-ids: a gap after each
        add("run", np.arange(7000, 7700), rng.integers(1, 5, 700))
        add("to_the_end", np.concatenate([2 * rng.choice(n // 2 - 1, 299, replace=False), [n - 1]]), rng.integers(1, 40, 300))
        return Collection.from_lists(n, lists, rng.integers(20, 400, n).astype(np.uint32)), names
    return _once("edge", make)


def freq_edge_collection():
    return _once("freq_edge", fcases.edge_collection)[0]


def freq_dense_collection():
    return _once("freq_dense", fcases.dense_collection)


def many_lists_collection(num_cus):
    """16 x CUs + 300 lists of 1, 1, 1, 2, 129 postings in turn: more blocks than the verification's launch grid holds, so every
    wave wraps, and most neighbouring lists are one block long (the worst case for the block -> list search)"""
    def make():
        rng = np.random.default_rng(0x3A17)
        n, count = 4000, 16 * num_cus + 300
        pool = np.sort(2 * rng.choice(n // 2, 129, replace=False)).astype(np.uint32)
        lists = []
        for i in range(count):
            m = (1, 1, 1, 2, 129)[i % 5]
            docs = pool[:m] + np.uint32(2 * (i % 7)) if m < 129 else pool
            lists.append((docs.astype(np.uint32), (1 + (np.arange(m) + i) % 7).astype(np.uint32)))
        return Collection.from_lists(n + 16, lists, np.full(n + 16, 50, dtype=np.uint32))
    return _once("many%d" % num_cus, make)


def postings(coll):
    return sum(len(dd) for dd, _ in coll.lists)


def clean_collections(kind):
    """the collections whose images of `kind` the clean-verification tests check"""
    if kind in FREQ_KINDS:  # (big_f of the freq edge lists: prefix sums past 2^32, which the block codecs are not built for)
        return [small_collection(), block_edge_collection()[0], freq_edge_collection(), freq_dense_collection()]
    return [small_collection(), block_edge_collection()[0]]


def image(coll, kind):
    """the host-built image of a collection, built once per (collection, kind)"""
    return _once(("image", id(coll), kind), lambda: coll.index_image(kind))


def altered(lists, changes):
    """a copy of `lists` with changes applied: (list, position, "docid" | "freq", new value)"""
    out = [(dd.copy(), ff.copy()) for dd, ff in lists]
    for t, i, what, v in changes:
        out[t][0 if what == "docid" else 1][i] = v
    for dd, _ in out:
        assert np.all(np.diff(dd.astype(np.int64)) > 0)  # the expected doc-ids stay strictly increasing
    return out


def write_collection(base, num_docs, lists, sizes):
    """<base>.docs / .freqs / .sizes: little-endian u32 streams of [len][len x u32] sequences, .docs led by [1][num_docs]"""
    with open(base + ".docs", "wb") as fd, open(base + ".freqs", "wb") as ff:
        np.array([1, num_docs], dtype=np.uint32).tofile(fd)
        for docs, freqs in lists:
            np.array([len(docs)], dtype=np.uint32).tofile(fd)
            np.asarray(docs, dtype=np.uint32).tofile(fd)
            np.array([len(freqs)], dtype=np.uint32).tofile(ff)
            np.asarray(freqs, dtype=np.uint32).tofile(ff)
    with open(base + ".sizes", "wb") as fs:
        np.array([num_docs], dtype=np.uint32).tofile(fs)
        np.asarray(sizes, dtype=np.uint32).tofile(fs)
