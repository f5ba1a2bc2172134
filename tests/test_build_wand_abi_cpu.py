"""The GPU wand_data builder's C ABI on a CPU-only box: the two symbols are exported and declared with the agreed arguments, the
host-side argument checks answer before any device work, and the fixture lists of test_gpu_build_wand.py place their maxima
where that file says they do (a numpy restatement of max_term_weight against the host builder's image)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ds2i_amd
import wand_build_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"ds2i_hip_build_wand": 9, "ds2i_hip_build_collection": 11}


def test_symbols_are_exported_and_declared(built_lib):
    src = open(os.path.join(ROOT, "include", "ds2i_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in ARGS.items():
        assert hasattr(built_lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        assert len(getattr(built_lib, name).argtypes) == nargs
    build_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds2i_build.h")).read(), flags=re.S)
    assert "ds2i_hip_" not in build_h  # nothing declared there touches the GPU
    assert ds2i_amd.gpu_build_wand and ds2i_amd.gpu_build_collection


def test_host_side_checks_come_before_the_device(built_lib):
    sizes = np.full(10, 5, dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    docs, freqs = np.array([1, 10], dtype=np.uint32), np.array([1, 1], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h, h2 = C.c_void_p(), C.c_void_p()
    L = built_lib
    # null arguments
    assert L.ds2i_hip_build_wand(0, None, 10, 1, p(offs), p(docs), p(freqs), C.byref(h), None) == -1
    assert L.ds2i_hip_build_wand(0, p(sizes), 10, 1, p(offs), p(docs), p(freqs), None, None) == -1
    assert L.ds2i_hip_build_collection(0, 0, p(sizes), 10, 1, p(offs), p(docs), p(freqs), None, C.byref(h2), None) == -1
    assert L.ds2i_hip_build_collection(0, 0, None, 10, 1, p(offs), p(docs), p(freqs), C.byref(h), C.byref(h2), None) == -1
    # doc-id 10 of 10 documents; an empty list; the kinds without a GPU encoder
    assert L.ds2i_hip_build_wand(0, p(sizes), 10, 1, p(offs), p(docs), p(freqs), C.byref(h), None) == -1
    assert b"doc id out of range" in L.ds2i_hip_last_error()
    assert L.ds2i_hip_build_collection(0, 0, p(sizes), 10, 1, p(offs), p(docs), p(freqs), C.byref(h), C.byref(h2), None) == -1
    offs0 = np.array([0, 0], dtype=np.uint64)
    assert L.ds2i_hip_build_wand(0, p(sizes), 10, 1, p(offs0), p(docs), p(freqs), C.byref(h), None) == -1
    assert b"List must be nonempty" in L.ds2i_hip_last_error()
    docs[1] = 9
    for kind in (ds2i_amd.CODECS["block_qmx"], ds2i_amd.CODECS["block_mixed"]):
        assert L.ds2i_hip_build_collection(0, kind, p(sizes), 10, 1, p(offs), p(docs), p(freqs), C.byref(h), C.byref(h2), None) == -1
    assert h.value is None and h2.value is None


@pytest.fixture(scope="module")
def small(built_lib):
    coll, names = cases.small_collection()
    return coll, names


def test_numpy_max_term_weight_agrees_with_the_host_image(small):
    coll, names = small
    got = cases.image_max_term_weights(coll.wand_image(), coll.num_docs, len(coll.lists))
    want = np.array([cases.max_term_weight(coll, t)[0] for t in range(len(coll.lists))], dtype=np.float32)
    assert got.tobytes() == want.tobytes()


def test_fixture_lists_place_their_maxima(small):
    coll, names = small
    for name, (n, at) in cases.PLACED.items():
        docs, _ = coll.lists[names[name]]
        _, where = cases.max_term_weight(coll, names[name])
        assert len(docs) == n and tuple(where) == at, name
    nb = lambda i: i // 128
    assert cases.PLACED["first"][1] == (0,)
    n, (at,) = cases.PLACED["tail_last"]
    assert at == n - 1 and n % 128 != 0                      # the last posting of a partial tail block
    n, (at,) = cases.PLACED["full_block_last"]
    assert at % 128 == 127 and nb(at) < nb(n - 1)            # the last posting of a full block that is not the last block
    a, b = cases.PLACED["tie_two_blocks"][1]
    assert nb(a) != nb(b)                                    # the same weight, bit for bit, in two blocks
    # the shortest documents carry the "ones" list's maximum, its first posting among them; the longest its minimum
    docs, freqs = coll.lists[names["ones"]]
    m, where = cases.max_term_weight(coll, names["ones"])
    assert set(int(x) for x in docs[where]) == set(cases.SHORT_DOCS) and where[0] == 0 and int(docs[-1]) == cases.LONG_DOC
    for n in cases.EDGE_LENGTHS:
        assert len(coll.lists[names["len%d" % n]][0]) == n


def test_big_collection_straddles_2_24():
    coll, names = cases.big_collection()
    assert coll.num_docs == (1 << 24) + (1 << 18)
    docs, _ = coll.lists[names["long"]]
    assert len(docs) >= 300000 and int(docs[0]) < (1 << 24) < int(docs[-1])
    _, where = cases.max_term_weight(coll, names["straddle"])
    sdocs = coll.lists[names["straddle"]][0]
    assert tuple(where) == (2,) and int(sdocs[2]) == (1 << 24) + 1
    # through a float32 the id would be an even neighbour's: another document length, another weight
    assert int(np.float32(sdocs[2])) != int(sdocs[2]) and coll.sizes[int(np.float32(sdocs[2]))] != coll.sizes[sdocs[2]]
