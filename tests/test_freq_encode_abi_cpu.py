"""The GPU encoder of the Elias-Fano layouts (opt, ef, single, uniform) on a CPU-only box: ds2i_hip_encode_index and
ds2i_hip_build_collection check their input on the host, before anything is staged or any device is touched, and the explicit
lists of test_gpu_freq_encode.py are lists the host builder accepts and the oracle reads back."""
import ctypes as C

import numpy as np
import pytest

import ds2i_amd as d
import freq_encode_cases as cases
import oracle as o
from helpers import Collection, small_params

KINDS = [d.CODECS[k] for k in d.FREQ_INDEX_KINDS]


def test_the_freq_kinds_are_5_to_8():
    assert KINDS == [5, 6, 7, 8]


@pytest.mark.parametrize("kind", KINDS)
def test_host_side_checks_come_before_the_device(built_lib, kind):
    L = built_lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    sizes = np.full(10, 5, dtype=np.uint32)
    offs = np.array([0, 3], dtype=np.uint64)
    good_docs, good_freqs = np.array([1, 4, 9], dtype=np.uint32), np.array([1, 2, 1], dtype=np.uint32)
    bad = {b"doc id out of range": (offs, np.array([1, 4, 10], dtype=np.uint32), good_freqs),
           b"not strictly increasing": (offs, np.array([4, 4, 9], dtype=np.uint32), good_freqs),
           b"zero freq": (offs, good_docs, np.array([1, 0, 1], dtype=np.uint32)),
           b"List must be nonempty": (np.array([0, 0], dtype=np.uint64), good_docs, good_freqs)}
    h, h2, ms = C.c_void_p(), C.c_void_p(), C.c_double(-7.0)
    for device in (0, 99):  # the answer is the input's, whatever the device
        for text, (of, docs, freqs) in bad.items():
            assert L.ds2i_hip_encode_index(device, kind, 10, 1, p(of), p(docs), p(freqs), C.byref(h), C.byref(ms)) == -1, text
            assert text in L.ds2i_hip_last_error(), (text, L.ds2i_hip_last_error())
            assert L.ds2i_hip_build_collection(device, kind, p(sizes), 10, 1, p(of), p(docs), p(freqs), C.byref(h), C.byref(h2),
                                               C.byref(ms)) == -1, text
            assert text in L.ds2i_hip_last_error(), (text, L.ds2i_hip_last_error())
        # null outputs
        assert L.ds2i_hip_encode_index(device, kind, 10, 1, p(offs), p(good_docs), p(good_freqs), None, C.byref(ms)) == -1
        assert b"null argument" in L.ds2i_hip_last_error()
        assert L.ds2i_hip_build_collection(device, kind, p(sizes), 10, 1, p(offs), p(good_docs), p(good_freqs), None, C.byref(h2),
                                           C.byref(ms)) == -1
        assert b"bad argument" in L.ds2i_hip_last_error()
    assert h.value is None and h2.value is None and ms.value == -7.0


@pytest.mark.parametrize("kind", d.FREQ_INDEX_KINDS)
def test_the_host_builder_accepts_the_edge_lists(built_lib, kind):
    for coll in (cases.edge_collection()[0], cases.dense_collection()):
        idx = o.Index(kind, coll.index_image(kind))
        assert idx.size() == len(coll.lists) and idx.num_docs() == coll.num_docs
        for t, (docs, freqs) in enumerate(coll.lists):
            dd, ff = idx.enumerate(t)
            assert np.array_equal(dd, docs) and np.array_equal(ff, freqs), t


def test_the_edge_lists_are_what_their_names_say():
    coll, names = cases.edge_collection()
    n = coll.num_docs
    for m in cases.EDGE_LENGTHS:
        assert len(coll.lists[names["len%d" % m]][0]) == m
    docs, _ = coll.lists[names["run"]]
    assert len(docs) > 256 and int(docs[-1] - docs[0]) + 1 == len(docs)
    docs, _ = coll.lists[names["every_second"]]
    assert len(docs) > 256 and int(docs[-1] - docs[0]) + 1 > 512 and np.all(np.diff(docs) == 2)
    docs, _ = coll.lists[names["sparse"]]
    assert len(docs) == 2000 and int(docs[-1]) > 900000 and len(docs) >> 8 > 0 and (int(docs[-1]) >> 8) >> 9 > 0
    assert int(coll.lists[names["to_the_end"]][0][-1]) == n - 1 and int(coll.lists[names["last_only"]][0][0]) == n - 1
    assert int(coll.lists[names["ones"]][1].max()) == 1
    freqs = coll.lists[names["big_f"]][1]
    assert len(freqs) == 3 and int(freqs.astype(np.uint64).sum()) > 1 << 32


def test_the_small_collection_has_opt_partitions_of_many_sizes(built_lib):
    """what test_gpu_freq_encode.py's comparison on the small synthetic collection is worth for opt: the DP's partitions are neither
    all fixed-size nor all whole lists (a chunk of the upload directory is at most 128 postings inside one partition)"""
    coll = Collection(small_params(num_docs=20000, num_terms=300, clustered_every=4))
    opt = coll.index_image("opt")
    assert len(opt) < len(coll.index_image("uniform"))
    sizes = set()
    for t in range(0, len(coll.lists), 7):
        _, chunks, _ = d.opt_list_directory(opt, t)
        sizes.update(int(x) for x in chunks[:, 1] & 0xFF)
    assert len(sizes) > 20 and min(sizes) < 16 and max(sizes) == 128
