"""Merging collections on a CPU-only box: the host twin against numpy, and every answer of the merge entry points that needs no device,
in the order the headers state: null arguments, no source, the kinds, the host parse of the images, the maps' lengths, the concatenated
doc maps, the term maps, a merged term without a list, and only then the missing device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
import merge_cases as mc
import remap_cases as rc
import verify_cases as cases
from ds2i_amd.api import MergeSource, _merge_postings_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "merge_indexes")
NO_DEVICE = 99
HIP_ARGS = {"ds2i_hip_merge_indexes": 7, "ds2i_hip_merge_postings": 10}
BUILD_ARGS = {"ds2i_merge_postings": 9}
EDGE_CUTS = {2: (7300,), 3: (7300, 30001)}  # (the first cut lies inside the run of 700 consecutive doc-ids)


def edge_shards(how):
    coll = rc.block_edge_collection()
    return coll, (mc.round_robin_shards(coll, 3) if how == "rr3" else mc.range_shards(coll, EDGE_CUTS[how]))


def test_symbols_are_exported_and_declared(built_lib):
    for header, table in (("ds2i_hip.h", HIP_ARGS), ("ds2i_build.h", BUILD_ARGS)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name, nargs in table.items():
            assert hasattr(built_lib, name), name
            decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
            assert decl, name
            assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
            assert len(getattr(built_lib, name).argtypes) == nargs
        if header == "ds2i_hip.h":
            assert re.search(r"\bvoid\s+ds2i_hip_merge_ms\s*\(", src) and "ds2i_merge_source" in src
    assert hasattr(built_lib, "ds2i_hip_merge_ms")
    assert d.merge_postings and d.gpu_merge_postings and d.gpu_merge_indexes


# ---------------------------------------------------------------- the host twin
@pytest.mark.parametrize("how", [2, 3, "rr3"])
def test_host_twin_equals_numpy_on_block_edge_shards(built_lib, how):
    coll, shards = edge_shards(how)
    want = mc.numpy_merge(shards)
    rc.assert_lists_equal(want[1], coll.lists)  # the shards put together are the collection again
    assert want[0] == coll.num_docs
    mc.assert_merged_equal(d.merge_postings(mc.api_sources(shards)), want)
    mc.assert_merged_equal(d.merge_postings(mc.api_sources(shards), num_terms=len(coll.lists), threads=3), want)


def test_host_twin_equals_numpy_on_small_collection_shards(built_lib):
    coll = rc.small_collection()
    shards = mc.range_shards(coll, (5000, 5001, 12345))  # (one shard is a single document)
    want = mc.numpy_merge(shards)
    rc.assert_lists_equal(want[1], coll.lists)
    mc.assert_merged_equal(d.merge_postings(mc.api_sources(shards)), want)


def test_a_term_present_in_one_source_only(built_lib):
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    a = mc.Shard(10, [(one(1, 4), one(2, 3)), (one(0, 9), one(1, 1))], None, None, None)
    b = mc.Shard(5, [(one(2), one(7)), (one(0, 3), one(5, 6))], None, one(1, 2), None)  # term 0 only in a, term 2 only in b
    got = d.merge_postings(mc.api_sources([a, b]))
    mc.assert_merged_equal(got, mc.numpy_merge([a, b]))
    assert [dd.tolist() for dd, _ in got[1]] == [[1, 4], [0, 9, 12], [10, 13]] and got[0] == 15
    assert [ff.tolist() for _, ff in got[1]] == [[2, 3], [1, 1, 7], [5, 6]]


def test_host_twin_past_2_24_and_one_source(built_lib):
    for reverse in (False, True):
        shards = mc.past_2_24_sources(reverse)
        got = d.merge_postings(mc.api_sources(shards))
        mc.assert_merged_equal(got, mc.numpy_merge(shards))
        assert got[0] == mc.PAST_2_24 + 150
    coll = rc.block_edge_collection()
    mc.assert_merged_equal(d.merge_postings([(coll.num_docs, coll.lists)]), (coll.num_docs, coll.lists))
    m = rc.doc_map("random", coll.num_docs)
    mc.assert_merged_equal(d.merge_postings([(coll.num_docs, coll.lists, m)]), (coll.num_docs, rc.numpy_remap(coll.lists, m)))


# ---------------------------------------------------------------- refusals, without a device
def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def merge_postings_rc(L, sources, nlists=0, device=None, nsrc=None, null=None):
    """(code, message) of ds2i_merge_postings (device None) or ds2i_hip_merge_postings; no output is written on an error"""
    arr, n, keep = _merge_postings_sources(sources)
    nd, nl = C.c_uint64(77), C.c_uint64(77)
    hs = [C.c_void_p() for _ in range(3)]
    outs = [C.byref(nd), C.byref(nl)] + [C.byref(h) for h in hs]
    if null is not None:
        outs[null] = None
    n = n if nsrc is None else nsrc
    if device is None:
        code = L.ds2i_merge_postings(arr, n, nlists, 1, *outs)
    else:
        code = L.ds2i_hip_merge_postings(device, arr, n, nlists, *outs, None)
    assert code != 0 and nd.value == 77 and nl.value == 77 and not any(h.value for h in hs)
    return code, L.ds2i_hip_last_error().decode()


def merge_indexes_rc(L, sources, to_kind=0, nlists=0, device=NO_DEVICE, nsrc=None, src_null=False, out_null=False):
    arr, keep = (MergeSource * max(1, len(sources)))(), []
    for src, (kind, image, doc_map, term_map) in zip(arr, sources):
        keep.append(image)
        src.kind, src.bytes = kind, len(image) if image is not None else 0
        src.image = C.cast(C.c_char_p(image), C.c_void_p) if image is not None else None
        for name, length, m in (("doc_map", "map_len", doc_map), ("term_map", "terms_len", term_map)):
            if m is not None:
                m = np.ascontiguousarray(m, dtype=np.uint32)
                keep.append(m)
                setattr(src, name, m.ctypes.data)
                setattr(src, length, len(m))
    h = C.c_void_p()
    code = L.ds2i_hip_merge_indexes(device, None if src_null else arr, len(sources) if nsrc is None else nsrc, nlists, to_kind,
                                    None if out_null else C.byref(h), None)
    assert code != 0 and not h.value
    return code, L.ds2i_hip_last_error().decode()


@pytest.fixture(scope="module")
def edge(built_lib):
    """the three range shards of the block edge collection as block_optpfor, opt and block_varint images with their term maps"""
    coll, shards = edge_shards(3)
    kinds = ("block_optpfor", "opt", "block_varint")
    return coll, shards, [(d.CODECS[k], img, dm, tm) for k, img, dm, tm in mc.image_sources(shards, kinds)]


def test_null_arguments_and_no_source(built_lib, edge):
    L = built_lib
    coll, shards, srcs = edge
    for kw in (dict(src_null=True), dict(out_null=True)):
        code, msg = merge_indexes_rc(L, srcs, **kw)
        assert code == -1 and "null argument" in msg
    code, msg = merge_indexes_rc(L, [srcs[0], (0, None, None, None)], to_kind=99)  # a null image comes before the kinds
    assert code == -1 and "null argument" in msg
    code, msg = merge_indexes_rc(L, srcs, nsrc=0)
    assert code == -1 and "no source" in msg
    for device in (None, NO_DEVICE):
        for null in range(5):
            code, msg = merge_postings_rc(L, mc.api_sources(shards), device=device, null=null)
            assert code == -1 and "null argument" in msg
        code, msg = merge_postings_rc(L, mc.api_sources(shards), device=device, nsrc=0)
        assert code == -1 and "no source" in msg


def test_unknown_kinds_and_targets_without_an_encoder_come_before_the_images(built_lib, edge):
    L = built_lib
    _, _, srcs = edge
    garbage = (0, cases.GARBAGE, None, None)
    for kind in (-1, 9, 99):
        for second in (srcs[1], garbage):
            code, msg = merge_indexes_rc(L, [srcs[0], (kind,) + second[1:]])
            assert code == -1 and "unknown index kind" in msg
            assert merge_indexes_rc(L, [srcs[0], second], to_kind=kind)[0] == -1
    for to_kind in ("block_qmx", "block_mixed"):
        for second in (srcs[1], garbage):
            code, msg = merge_indexes_rc(L, [srcs[0], second], to_kind=d.CODECS[to_kind])
            assert code == -1 and all(name in msg for name in cases.GPU_BUILT_KINDS)


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_a_garbage_image_comes_before_the_maps(built_lib, edge, kind):
    _, _, srcs = edge
    bad = np.zeros(7, dtype=np.uint32)  # wrong lengths and no maps at all: the images are looked at first
    code, _ = merge_indexes_rc(built_lib, [(srcs[0][0], srcs[0][1], bad, bad), (d.CODECS[kind], cases.GARBAGE, None, None)])
    assert code == -2


def test_maps_then_device(built_lib, edge):
    """the same refusals from the twin, the device form over postings and the device form over images"""
    L = built_lib
    coll, shards, srcs = edge
    V = len(coll.lists)

    def both(change, nlists=0):
        """change(source index, doc_map, term_map, num_docs) -> (doc_map, term_map); returns the three (code, message)"""
        maps = [change(i, s.doc_map, s.term_map, s.num_docs) for i, s in enumerate(shards)]
        csr = [(s.num_docs, s.lists, dm, tm) for s, (dm, tm) in zip(shards, maps)]
        img = [(k, im, dm, tm) for (k, im, _, _), (dm, tm) in zip(srcs, maps)]
        return [merge_postings_rc(L, csr, nlists), merge_postings_rc(L, csr, nlists, device=NO_DEVICE), merge_indexes_rc(L, img, nlists=nlists)]

    base = mc.bases(shards)
    explicit = [(np.arange(s.num_docs, dtype=np.int64) + base[i]).astype(np.uint32) for i, s in enumerate(shards)]
    # a doc map of the wrong length, although what it holds is no permutation either: the length is named
    for code, msg in both(lambda i, dm, tm, n: (np.zeros(n - 1, dtype=np.uint32) if i == 1 else dm, tm)):
        assert code == -1 and "the doc map of source 1 holds" in msg
    for code, msg in both(lambda i, dm, tm, n: (dm, tm[:-1] if i == 2 else tm)):
        assert code == -1 and "the term map of source 2 holds" in msg
    # the concatenation is no permutation: the second document sent to an id already taken is named, numbered in the concatenation
    clash = explicit[1].copy()
    clash[3] = 5  # (document 5 of source 0 holds it by default)
    for code, msg in both(lambda i, dm, tm, n: (clash if i == 1 else dm, tm)):
        assert code == -1 and "no permutation" in msg and "document %d maps to 5," % (base[1] + 3) in msg
    over = explicit[2].copy()
    over[0] = coll.num_docs
    for code, msg in both(lambda i, dm, tm, n: (over if i == 2 else dm, tm)):
        assert code == -1 and "document %d maps to %d, outside" % (base[2], coll.num_docs) in msg
    # term maps: not increasing, out of range
    def swapped(tm):
        tm = tm.copy()
        tm[[1, 2]] = tm[[2, 1]]
        return tm
    for code, msg in both(lambda i, dm, tm, n: (dm, swapped(tm) if i == 0 else tm)):
        assert code == -1 and "the term map of source 0 does not increase at list 2" in msg
    for code, msg in both(lambda i, dm, tm, n: (dm, tm), nlists=V - 1):
        assert code == -1 and "outside the %d merged lists" % (V - 1) in msg
    # a merged term with no list: the first one is named, in the builder's words
    for code, msg in both(lambda i, dm, tm, n: (dm, np.where(tm >= 3, tm + 2, tm).astype(np.uint32)), nlists=V + 3):
        assert code == -1 and "merged term 3 receives no list" in msg and "List must be nonempty" in msg
    # all is well but the device: the twin merges, the device forms look for the device
    ok = lambda i, dm, tm, n: (explicit[i], tm)  # noqa: E731
    maps = [ok(i, None, s.term_map, None) for i, s in enumerate(shards)]
    got = d.merge_postings([(s.num_docs, s.lists, dm, tm) for s, (dm, tm) in zip(shards, maps)])
    mc.assert_merged_equal(got, (coll.num_docs, coll.lists))
    code, msg = merge_postings_rc(L, mc.api_sources(shards), device=NO_DEVICE)
    assert code == -4 and "no such HIP device" in msg
    code, msg = merge_indexes_rc(L, srcs, to_kind=d.CODECS["ef"])
    assert code == -4 and "no such HIP device" in msg
    for call in (lambda: d.gpu_merge_indexes(mc.image_sources(shards, ("opt",)), "block_optpfor", device=NO_DEVICE),
                 lambda: d.gpu_merge_postings(mc.api_sources(shards), device=NO_DEVICE)):
        with pytest.raises(d.Ds2iError) as e:
            call()
        assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_merge_indexes(mc.image_sources(shards, ("opt",)), "block_mixed", device=NO_DEVICE)
    assert e.value.code == -1


def test_too_many_documents(built_lib):
    """2^32 documents between the sources; no posting is looked at"""
    one = (np.array([0], dtype=np.uint32), np.array([1], dtype=np.uint32))
    for device in (None, NO_DEVICE):
        code, msg = merge_postings_rc(built_lib, [(1 << 31, [one]), (1 << 31, [one])], device=device)
        assert code == -1 and "2^32" in msg


def test_host_twin_refuses_a_doc_id_outside_a_source(built_lib):
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    code, msg = merge_postings_rc(built_lib, [(10, [(one(3, 9), one(1, 1))]), (5, [(one(2, 5), one(1, 1))])])
    assert code == -2 and "outside the map" in msg and "source 1" in msg


# ---------------------------------------------------------------- the host side under the sanitizers, as a program of its own
def test_twin_check_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """host_merge.hpp and tests/merge_twin_check.cpp (its own main) compiled with -fsanitize=address,undefined and run: nothing that is
    loaded into this interpreter runs under a sanitizer"""
    exe = str(tmp_path / "merge_twin_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread",  # (the runtimes inside the program: it asks nothing of its loader)
                           os.path.join(ROOT, "tests", "merge_twin_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and p.stdout == "OK\n" and p.stderr == "", (p.stdout, p.stderr)


# ---------------------------------------------------------------- the tool
def test_tool_usage_errors_without_a_device(built_lib, edge, tmp_path):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])

    def run(*args):
        p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return p.returncode, p.stdout, p.stderr

    _, shards, srcs = edge
    a, b, out = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "out")
    open(a, "wb").write(srcs[0][1])
    open(b, "wb").write(srcs[1][1])
    good, short = str(tmp_path / "terms"), str(tmp_path / "short")
    mc.write_map(good, shards[0].term_map)
    open(short, "wb").write(open(good, "rb").read()[:-4])
    for args in (("block_optpfor", out), ("block_optpfor", out, "block_optpfor"), ("block_optpfor", out, "block_optpfor", a, "opt"),
                 ("block_optpfor", out, "--terms", good, "block_optpfor", a),              # a map before any source
                 ("block_optpfor", out, "block_optpfor", a, "--terms"),                     # no file name
                 ("block_optpfor", out, "block_optpfor", a, "--terms", good, "--terms", good),
                 ("block_optpfor", out, "block_optpfor", a, "--frobnicate")):
        rcode, stdout, err = run(*args)
        assert rcode == 2 and stdout == "" and "usage" in err, (args, err)
    for bad in (str(tmp_path / "missing"), short):
        for flag in ("--docs", "--terms"):
            rcode, stdout, err = run("block_optpfor", out, "block_optpfor", a, flag, bad)
            assert rcode == 2 and stdout == "" and "usage" in err, (bad, err)
    assert run("nonsense", out, "block_optpfor", a)[0] == 2 and run("opt", out, "nonsense", a)[0] == 2
    rcode, _, err = run("block_qmx", out, "block_optpfor", a, "--terms", good)
    assert rcode == 2 and all(name in err for name in cases.GPU_BUILT_KINDS)
    # a term without a list is the library's answer, in the builder's words; so is the missing device once all is well
    rcode, stdout, err = run("opt", out, "block_optpfor", a, "opt", b, "--lists", "1000", "--device", str(NO_DEVICE))
    assert rcode == 2 and stdout == "" and "receives no list: List must be nonempty" in err
    rcode, stdout, err = run("opt", out, "--check", "block_optpfor", a, "--device", str(NO_DEVICE), "opt", b)  # (flags in any place)
    assert rcode == 2 and stdout == "" and "no such HIP device" in err
    assert not os.path.exists(out)
