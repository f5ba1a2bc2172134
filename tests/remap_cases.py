"""The doc-id maps and collections of the remap tests (test_remap_abi_cpu.py, test_gpu_remap.py), and the numpy reference: every
doc-id through the map, every list sorted by argsort. All maps are closed-form or seeded; the doc-ids of a list are distinct, so the
remapped list is unique and every comparison is exact."""
import numpy as np

import verify_cases as cases
from helpers import Collection

MAPS = ("identity", "reverse", "rotation", "random")
_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def doc_map(name, n):
    """new doc-id of every old doc-id, uint32[n]"""
    def make():
        d = np.arange(n, dtype=np.int64)
        if name == "identity":
            m = d
        elif name == "reverse":  # every list fully reversed
            m = n - 1 - d
        elif name == "rotation":  # every list becomes two sorted runs
            m = (d + n // 2) % n
        else:
            m = np.random.default_rng(0x52E3A9).permutation(n)
        return m.astype(np.uint32)
    return _once(("map", name, n), make)


def inverse(m):
    inv = np.empty_like(m)
    inv[m] = np.arange(len(m), dtype=m.dtype)
    return inv


def numpy_remap(lists, m):
    out = []
    for docs, freqs in lists:
        new = m[docs]
        order = np.argsort(new, kind="stable")
        out.append((new[order].astype(np.uint32), np.asarray(freqs, dtype=np.uint32)[order]))
    return out


def remapped_collection(coll, name):
    """the collection with its documents renumbered by the map of that name, built from scratch: numpy-remapped lists, the sizes moved
    with their documents"""
    def make():
        m = doc_map(name, coll.num_docs)
        sizes = np.empty_like(coll.sizes)
        sizes[m] = coll.sizes
        return Collection.from_lists(coll.num_docs, numpy_remap(coll.lists, m), sizes)
    return _once(("remapped", id(coll), name), make)


def assert_lists_equal(got, want):
    assert len(got) == len(want)
    for t, ((gd, gf), (wd, wf)) in enumerate(zip(got, want)):
        assert gd.dtype == np.uint32 and gf.dtype == np.uint32
        assert np.array_equal(gd, wd), "doc-ids of list %d (%d postings)" % (t, len(wd))
        assert np.array_equal(gf, wf), "freqs of list %d (%d postings)" % (t, len(wd))


def class_edge_lengths(bounds):
    """lengths at the real edges of the three sort classes: one wavefront (<= W), one workgroup (<= L), tiles of T"""
    W, L, T = bounds
    lengths = [1, 2, W - 1, W, W + 1, 127, 128, 129, L - 1, L, L + 1, L + T]
    if 2 * T > L:
        lengths.append(2 * T)
    return lengths + [2 * T + 1, 3 * T - 1]


def class_edge_num_docs(bounds):
    """the key width is no multiple of the radix digit: 2^17 + 3 documents need 18 bits"""
    return max((1 << 17) + 3, 4 * max(class_edge_lengths(bounds)) + 3)


def class_edge_lists(bounds):
    """one seeded list per edge length, doc-ids drawn from all documents"""
    def make():
        rng = np.random.default_rng(0xC1A55)
        n = class_edge_num_docs(bounds)
        return [(np.sort(rng.choice(n, m, replace=False)).astype(np.uint32), rng.integers(1, 40, m).astype(np.uint32))
                for m in class_edge_lengths(bounds)]
    return _once(("edges", tuple(bounds)), make)


def preimage_lists(bounds, m):
    """lists whose NEW doc-ids are a contiguous range [c, c + n): all keys of a list share their high digits, the skew case of a radix
    sort (every posting of a pass lands in a few buckets). One list per class and one of 2 T + 1."""
    W, L, T = bounds
    inv = inverse(m)
    rng = np.random.default_rng(0x9E1A)
    lists = []
    for n, c in ((W, 5), (L, 1000), (L + 1, 70000), (2 * T + 1, len(m) - 2 * T - 1)):
        lists.append((np.sort(inv[c:c + n]).astype(np.uint32), rng.integers(1, 40, n).astype(np.uint32)))
    return lists


PAST_2_24 = (1 << 24) + 5


def past_2_24_lists(bounds):
    """three lists of 1, 200 and L + 1 postings whose doc-ids lie on both sides of 2^24, and so do their images under the reverse map"""
    L = bounds[1]
    n = PAST_2_24
    lists = [(np.array([(1 << 24) + 1], dtype=np.uint32), np.array([3], dtype=np.uint32))]
    for m in (200, L + 1):
        low = 1 + 7 * np.arange(m - 4, dtype=np.int64)                      # -> the top of the new doc-ids, past 2^24
        high = np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 2, n - 1])     # -> 5, 4, 2, 0
        docs = np.concatenate([low, high]).astype(np.uint32)
        lists.append((docs, (1 + np.arange(m) % 37).astype(np.uint32)))
    return lists


def reverse_map_past_2_24():
    return doc_map("reverse", PAST_2_24)


def small_collection():
    return cases.small_collection()


def block_edge_collection():
    return cases.block_edge_collection()[0]


def write_map(path, m):
    """one ds2i binary sequence: [len][len x u32], the layout of a .sizes file"""
    with open(path, "wb") as f:
        np.array([len(m)], dtype=np.uint32).tofile(f)
        np.asarray(m, dtype=np.uint32).tofile(f)
