"""Renumbering documents on a CPU-only box: the host twin against numpy, the check of a doc-id map, the wand image of a renumbered
collection against a build from scratch, and every answer of the two device entry points that needs no device, in the order the header
states: null arguments, kinds, the host parse of the image, the map's length, the map, and only then the missing device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
import remap_cases as rc
import verify_cases as cases
from ds2i_amd.api import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "convert_index")
NO_DEVICE = 99
HIP_ARGS = {"ds2i_hip_remap_postings": 10, "ds2i_hip_remap_index": 9}
BUILD_ARGS = {"ds2i_check_doc_map": 2, "ds2i_remap_postings": 7, "ds2i_remap_wand": 5}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_are_exported_and_declared(built_lib):
    for header, table in (("ds2i_hip.h", HIP_ARGS), ("ds2i_build.h", BUILD_ARGS)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name, nargs in table.items():
            assert hasattr(built_lib, name), name
            decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
            assert decl, name
            assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
            assert len(getattr(built_lib, name).argtypes) == nargs
    assert d.check_doc_map and d.remap_postings and d.gpu_remap_postings and d.gpu_remap_index and d.remap_wand and d.Index.remap


def test_class_bounds_are_reported_as_compiled(built_lib):
    W, L, T = d.remap_class_bounds()
    assert W == 64                      # a wavefront
    assert W < L and 8 * L <= 80 << 10  # the pairs of a class 2 list fit a workgroup's LDS twice over in a compute unit's 160 KiB
    assert T >= 256


# ---------------------------------------------------------------- the host twin
@pytest.mark.parametrize("name", rc.MAPS)
@pytest.mark.parametrize("which", ["block_edge", "small"])
def test_host_twin_equals_numpy(built_lib, which, name):
    coll = rc.block_edge_collection() if which == "block_edge" else rc.small_collection()
    m = rc.doc_map(name, coll.num_docs)
    rc.assert_lists_equal(d.remap_postings(coll.num_docs, coll.lists, m), rc.numpy_remap(coll.lists, m))
    rc.assert_lists_equal(d.remap_postings(coll.num_docs, coll.lists, m, threads=3), rc.numpy_remap(coll.lists, m))


def test_host_twin_on_preimage_lists_and_past_2_24(built_lib):
    bounds = d.remap_class_bounds()
    m = rc.doc_map("random", rc.class_edge_num_docs(bounds))
    lists = rc.preimage_lists(bounds, m)
    got = d.remap_postings(len(m), lists, m)
    rc.assert_lists_equal(got, rc.numpy_remap(lists, m))
    for docs, _ in got:  # the new doc-ids of every list are one contiguous range
        assert int(docs[-1]) - int(docs[0]) == len(docs) - 1
    m = rc.reverse_map_past_2_24()
    lists = rc.past_2_24_lists(bounds)
    got = d.remap_postings(len(m), lists, m)
    rc.assert_lists_equal(got, rc.numpy_remap(lists, m))
    assert all(int(docs[0]) < 1 << 24 <= int(docs[-1]) for docs, _ in got[1:])


def test_host_twin_refuses_a_doc_id_outside_the_map(built_lib):
    L = built_lib
    m = rc.doc_map("reverse", 10)
    offs = np.array([0, 2], dtype=np.uint64)
    docs, freqs = np.array([3, 10], dtype=np.uint32), np.array([1, 1], dtype=np.uint32)
    assert L.ds2i_remap_postings(10, 1, ptr(offs), ptr(docs), ptr(freqs), ptr(m), 1) == -2
    assert b"outside the map" in L.ds2i_hip_last_error()
    assert L.ds2i_remap_postings(10, 1, None, ptr(docs), ptr(freqs), ptr(m), 1) == -1
    assert L.ds2i_remap_postings(10, 1, ptr(offs), ptr(docs), ptr(freqs), None, 1) == -1


# ---------------------------------------------------------------- the map check
@pytest.mark.parametrize("name", rc.MAPS)
def test_check_doc_map_accepts_every_map(built_lib, name):
    for n in (1, 2, 63, 64, 65, 50000):
        d.check_doc_map(rc.doc_map(name, n))


def test_check_doc_map_names_the_first_offending_document(built_lib):
    L = built_lib
    n = 1000
    m = rc.doc_map("random", n).copy()
    m[700], m[900] = n, n + 5  # a value == num_docs: the first one is named
    assert L.ds2i_check_doc_map(ptr(m), n) == -1
    msg = L.ds2i_hip_last_error().decode()
    assert "document 700 " in msg and " %d" % n in msg and "900" not in msg
    m = rc.doc_map("random", n).copy()
    m[400] = m[100]  # the SECOND document sent to an id already taken is the offender
    m[800] = m[200]
    assert L.ds2i_check_doc_map(ptr(m), n) == -1
    msg = L.ds2i_hip_last_error().decode()
    assert "document 400 " in msg and " %d" % int(m[100]) in msg and "800" not in msg
    with pytest.raises(d.Ds2iError) as e:
        d.check_doc_map(m)
    assert e.value.code == -1 and "document 400 " in str(e.value)
    m = rc.doc_map("identity", 64).copy()  # the last bit of a word
    m[63] = 62
    assert L.ds2i_check_doc_map(ptr(m), 64) == -1 and b"document 63 " in L.ds2i_hip_last_error()
    assert L.ds2i_check_doc_map(None, 5) == -1 and L.ds2i_check_doc_map(None, 0) == 0
    # a longer array is a map of its first num_docs entries only if those are a permutation
    assert L.ds2i_check_doc_map(ptr(rc.doc_map("identity", 64)), 10) == 0
    assert L.ds2i_check_doc_map(ptr(rc.doc_map("reverse", 64)), 10) == -1


# ---------------------------------------------------------------- wand data
@pytest.mark.parametrize("name", rc.MAPS)
@pytest.mark.parametrize("which", ["block_edge", "small"])
def test_remap_wand_is_the_build_from_scratch(built_lib, which, name):
    coll = rc.block_edge_collection() if which == "block_edge" else rc.small_collection()
    m = rc.doc_map(name, coll.num_docs)
    got = d.remap_wand(coll.wand_image(), m)
    assert got == rc.remapped_collection(coll, name).wand_image()
    if name == "identity":
        assert got == coll.wand_image()


def test_remap_wand_errors(built_lib):
    coll = rc.block_edge_collection()
    wand = coll.wand_image()
    for bad, code in ((rc.doc_map("random", coll.num_docs - 1), -1), (np.zeros(coll.num_docs, dtype=np.uint32), -1)):
        with pytest.raises(d.Ds2iError) as e:
            d.remap_wand(wand, bad)
        assert e.value.code == code
    with pytest.raises(d.Ds2iError) as e:
        d.remap_wand(cases.GARBAGE, rc.doc_map("random", coll.num_docs))
    assert e.value.code == -2


# ---------------------------------------------------------------- the device entry points, without a device
def remap_index(L, from_kind, img, m, to_kind, device=NO_DEVICE, image_null=False, map_null=False, out_null=False, map_len=None):
    h = C.c_void_p()
    rc_ = L.ds2i_hip_remap_index(device, from_kind, None if image_null else img, len(img), None if map_null else ptr(m),
                                 len(m) if map_len is None else map_len, to_kind, None if out_null else C.byref(h), None)
    assert not h.value
    return rc_


def remap_postings(L, coll, m, device=NO_DEVICE, skip=None):
    n, offs, docs, freqs = _csr(coll.lists)
    od, of = np.full_like(docs, 0xABCD), np.full_like(freqs, 0xABCD)
    args = [ptr(offs), ptr(docs), ptr(freqs), ptr(m), ptr(od), ptr(of)]
    if skip is not None:
        args[skip] = None
    rc_ = L.ds2i_hip_remap_postings(device, coll.num_docs, n, *args, None)
    assert np.all(od == 0xABCD) and np.all(of == 0xABCD)  # no output is written on an error
    return rc_


@pytest.fixture(scope="module")
def edge(built_lib):
    coll = rc.block_edge_collection()
    return coll, cases.image(coll, "block_optpfor"), rc.doc_map("random", coll.num_docs)


def test_null_arguments(built_lib, edge):
    L = built_lib
    coll, image, m = edge
    assert remap_index(L, 0, image, m, 0, image_null=True) == -1 and b"null argument" in L.ds2i_hip_last_error()
    assert remap_index(L, 0, image, m, 0, map_null=True) == -1 and b"null argument" in L.ds2i_hip_last_error()
    assert remap_index(L, 0, image, m, 0, out_null=True) == -1 and b"null argument" in L.ds2i_hip_last_error()
    assert remap_index(L, 99, cases.GARBAGE, m, 99, map_null=True) == -1 and b"null argument" in L.ds2i_hip_last_error()  # null comes first
    for skip in range(6):
        assert remap_postings(L, coll, m, skip=skip) == -1 and b"null argument" in L.ds2i_hip_last_error()


def test_unknown_kinds_come_before_the_image(built_lib, edge):
    L = built_lib
    _, image, m = edge
    for kind in (-1, 9, 99):
        for img in (image, cases.GARBAGE):
            assert remap_index(L, kind, img, m, 0) == -1 and b"unknown index kind" in L.ds2i_hip_last_error()
            assert remap_index(L, 0, img, m, kind) == -1


@pytest.mark.parametrize("to_kind", ["block_qmx", "block_mixed"])
def test_targets_without_an_encoder_are_refused_before_the_image_is_read(built_lib, edge, to_kind):
    L = built_lib
    _, image, m = edge
    for img in (image, cases.GARBAGE):
        assert remap_index(L, 0, img, m, d.CODECS[to_kind]) == -1
        for name in cases.GPU_BUILT_KINDS:
            assert name.encode() in L.ds2i_hip_last_error()


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_garbage_image_comes_before_the_map(built_lib, kind):
    bad_map = np.zeros(7, dtype=np.uint32)  # wrong length and no permutation: the image is looked at first
    assert remap_index(built_lib, d.CODECS[kind], cases.GARBAGE, bad_map, d.CODECS["block_optpfor"]) == -2


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_map_length_then_permutation_then_device(built_lib, kind):
    L = built_lib
    coll = rc.block_edge_collection()
    img, n = cases.image(coll, kind), coll.num_docs
    m = rc.doc_map("random", n)
    dup = m.copy()
    dup[n - 1] = dup[0]
    # a wrong length, although the entries it covers are no permutation either: the length is named
    assert remap_index(L, d.CODECS[kind], img, dup, 0, map_len=n - 1) == -1
    assert b"the map holds" in L.ds2i_hip_last_error()
    assert remap_index(L, d.CODECS[kind], img, np.concatenate([m, m]), 0) == -1 and b"the map holds" in L.ds2i_hip_last_error()
    # the right length, no permutation: the map check answers, before the device is looked for
    assert remap_index(L, d.CODECS[kind], img, dup, 0) == -1
    assert b"ds2i_check_doc_map: document %d " % (n - 1) in L.ds2i_hip_last_error()
    # all is well but the device
    assert remap_index(L, d.CODECS[kind], img, m, d.CODECS["block_varint"]) == -4 and b"no such HIP device" in L.ds2i_hip_last_error()
    for call in (lambda: d.gpu_remap_index(kind, img, m, device=NO_DEVICE) if kind != "opt" else d.gpu_remap_index(kind, img, m, "ef", device=NO_DEVICE),
                 lambda: d.gpu_remap_postings(n, coll.lists, m, device=NO_DEVICE)):
        with pytest.raises(d.Ds2iError) as e:
            call()
        assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_remap_index(kind, img, m, "block_mixed", device=NO_DEVICE)
    assert e.value.code == -1


def test_remap_postings_checks_the_map_before_the_device(built_lib, edge):
    L = built_lib
    coll, _, m = edge
    over = m.copy()
    over[5] = coll.num_docs
    assert remap_postings(L, coll, over) == -1 and b"document 5 " in L.ds2i_hip_last_error()
    assert remap_postings(L, coll, m) == -4 and b"no such HIP device" in L.ds2i_hip_last_error()


# ---------------------------------------------------------------- the tool
def test_tool_map_file_errors_without_a_device(built_lib, edge, tmp_path):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])

    def run(*args):
        p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return p.returncode, p.stdout, p.stderr

    coll, image, m = edge
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    open(src, "wb").write(image)
    good, short, empty = str(tmp_path / "map"), str(tmp_path / "short"), str(tmp_path / "empty")
    rc.write_map(good, m)
    open(short, "wb").write(open(good, "rb").read()[:-4])
    open(empty, "wb").close()
    for bad in (str(tmp_path / "missing"), short, empty):
        rcode, stdout, err = run("block_optpfor", src, "opt", out, "--remap", bad)
        assert rcode == 2 and stdout == "" and "usage" in err, (bad, err)
    assert run("block_optpfor", src, "opt", out, "--remap")[0] == 2                       # no file name
    assert run("block_optpfor", src, "--dump", out, "--remap", good)[0] == 2              # a dump is not renumbered
    assert run("block_optpfor", src, "opt", out, "--wand", src, out + ".wand")[0] == 2    # wand data without a map
    rcode, _, err = run("block_optpfor", src, "block_qmx", out, "--remap", good)
    assert rcode == 2 and all(name in err for name in cases.GPU_BUILT_KINDS)
    rcode, stdout, err = run("block_optpfor", src, "opt", out, "--remap", good, "--device", str(NO_DEVICE))
    assert rcode == 2 and stdout == "" and "no such HIP device" in err
    assert not os.path.exists(out) and not os.path.exists(out + ".wand")
