"""Splitting collections on a CPU-only box: the host twin against numpy and against the shards of merge_cases, merge(split(x)) == x, and
every answer of the split entry points that needs no device, in the order the headers state: null arguments and the offsets, no shard,
2^32 documents, the kinds, the host parse of the image, the length of shard_of, its values, a shard without a document, and only then
the missing device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
import merge_cases as mc
import remap_cases as rc
import split_cases as sc
import verify_cases as cases
from ds2i_amd.api import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "split_index")
NO_DEVICE = 99
HIP_ARGS = {"ds2i_hip_split_index": 10, "ds2i_hip_split_postings": 10, "ds2i_hip_image_shape": 5}
BUILD_ARGS = {"ds2i_split_postings": 9}


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
            assert re.search(r"\bvoid\s+ds2i_hip_split_ms\s*\(", src) and re.search(r"\buint32_t\s+ds2i_hip_split_window\s*\(", src)
        else:
            assert re.search(r"\bvoid\s+ds2i_split_free\s*\(", src) and "ds2i_split_shard" in src and "DS2I_SPLIT_DROP" in src
            assert "is not offered" not in src
    for name in ("ds2i_hip_split_ms", "ds2i_hip_split_window", "ds2i_split_free"):
        assert hasattr(built_lib, name)
    assert d.split_postings and d.gpu_split_postings and d.gpu_split_index and d.Index.split and d.DROP == 0xFFFFFFFF
    W = d.split_window()
    assert W > 0 and W % 64 == 0


# ---------------------------------------------------------------- the host twin
def edge_assign(how, num_docs):
    if how == "range":
        return sc.range_assign(num_docs, sc.EDGE_CUTS), 3
    if how == "rr3":
        return sc.round_robin_assign(num_docs, 3), 3
    return sc.random_assign(num_docs, 5), 5


@pytest.mark.parametrize("how", ["range", "rr3", "random"])
def test_host_twin_equals_numpy_on_the_block_edge_collection(built_lib, how):
    coll = rc.block_edge_collection()
    shard_of, k = edge_assign(how, coll.num_docs)
    want = sc.numpy_split(coll.num_docs, coll.lists, shard_of, k)
    if how == "random":
        dropped = int(np.sum(shard_of == d.DROP))
        assert 0.05 * coll.num_docs < dropped < 0.15 * coll.num_docs and sum(s[0] for s in want) == coll.num_docs - dropped
    sc.assert_shards_equal(d.split_postings(coll.num_docs, coll.lists, shard_of), want)
    sc.assert_shards_equal(d.split_postings(coll.num_docs, coll.lists, shard_of, nshards=k, threads=3), want)


def test_host_twin_equals_the_shards_the_merge_tests_cut(built_lib):
    """merge_cases.range_shards and round_robin_shards state the same semantics on their own, maps included"""
    coll = rc.block_edge_collection()
    got = d.split_postings(coll.num_docs, coll.lists, sc.range_assign(coll.num_docs, sc.EDGE_CUTS))
    sc.assert_shards_equal(got, sc.from_merge_shards(mc.range_shards(coll, sc.EDGE_CUTS)))
    for k, group in ((3, 1), (2, 2)):
        got = d.split_postings(coll.num_docs, coll.lists, sc.round_robin_assign(coll.num_docs, k, group))
        sc.assert_shards_equal(got, sc.from_merge_shards(mc.round_robin_shards(coll, k, group)))
    small = rc.small_collection()
    got = d.split_postings(small.num_docs, small.lists, sc.range_assign(small.num_docs, (5000, 5001, 12345)))  # (one shard is a single document)
    sc.assert_shards_equal(got, sc.from_merge_shards(mc.range_shards(small, (5000, 5001, 12345))))
    assert got[1][0] == 1
    short = sc.short_lists_collection()  # thousands of lists of 1 to 3 postings by doc parity: most vanish from one shard or the other
    got = d.split_postings(short.num_docs, short.lists, sc.round_robin_assign(short.num_docs, 2))
    sc.assert_shards_equal(got, sc.from_merge_shards(mc.round_robin_shards(short, 2)))
    sc.assert_shards_equal(got, sc.numpy_split(short.num_docs, short.lists, sc.round_robin_assign(short.num_docs, 2), 2))


@pytest.mark.parametrize("how", ["range", "rr3"])
def test_merging_the_shards_gives_the_collection_back(built_lib, how):
    coll = rc.block_edge_collection()
    shard_of, _ = edge_assign(how, coll.num_docs)
    shards = d.split_postings(coll.num_docs, coll.lists, shard_of)
    mc.assert_merged_equal(d.merge_postings(sc.merge_sources(shards)), (coll.num_docs, coll.lists))


def test_twin_edge_cases(built_lib):
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    lists = [(one(0, 2, 5), one(1, 2, 3)), (one(), one()), (one(2), one(9)), (one(), one())]  # empty input lists
    # a shard of a single document (4), which no list holds: it comes back with zero lists
    got = d.split_postings(6, lists, [0, 0, 0, 2, 1, 2])
    sc.assert_shards_equal(got, sc.numpy_split(6, lists, [0, 0, 0, 2, 1, 2], 3))
    assert got[1][0] == 1 and got[1][1] == [] and got[1][2].tolist() == [4] and len(got[1][3]) == 0
    assert [dd.tolist() for dd, _ in got[0][1]] == [[0, 2], [2]] and got[0][3].tolist() == [0, 2]
    assert [dd.tolist() for dd, _ in got[2][1]] == [[1]] and [ff.tolist() for _, ff in got[2][1]] == [[3]] and got[2][2].tolist() == [3, 5]
    # one shard and nothing dropped: the identity, with identity maps, but for the empty lists
    coll = rc.block_edge_collection()
    (n, same, doc_map, term_map), = d.split_postings(coll.num_docs, coll.lists, np.zeros(coll.num_docs, dtype=np.uint32))
    assert n == coll.num_docs and np.array_equal(doc_map, np.arange(n)) and np.array_equal(term_map, np.arange(len(coll.lists)))
    rc.assert_lists_equal(same, coll.lists)
    # a shard nobody is sent to, and everything dropped
    got = d.split_postings(6, lists, [0, 0, 0, 0, 0, 0], nshards=2)
    assert got[1][0] == 0 and got[1][1] == [] and len(got[1][2]) == 0 and len(got[1][3]) == 0 and got[0][0] == 6
    got = d.split_postings(6, lists, [d.DROP] * 6)
    assert len(got) == 1 and got[0][0] == 0 and got[0][1] == [] and len(got[0][2]) == 0
    got = d.split_postings(6, lists, [d.DROP] * 6, nshards=3)
    assert len(got) == 3 and all(s[0] == 0 and s[1] == [] for s in got)


def test_host_twin_past_2_24(built_lib):
    num_docs, lists, shard_of = sc.past_2_24_case()
    assert num_docs == (1 << 24) + 5
    got = d.split_postings(num_docs, lists, shard_of)
    sc.assert_shards_equal(got, sc.numpy_split(num_docs, lists, shard_of, 2))
    assert int(got[0][2][-1]) > 1 << 24 and int(got[0][1][0][0][-1]) > (1 << 24) - 10  # old and local ids past 2^24


# ---------------------------------------------------------------- refusals, without a device
def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def split_postings_rc(L, num_docs, lists, shard_of, nshards, device=None, null=None, offs=None):
    """(code, message) of ds2i_split_postings (device None) or ds2i_hip_split_postings; no output is written on an error"""
    n, o, docs, freqs = _csr(lists)
    o = o if offs is None else np.asarray(offs, dtype=np.uint64)
    m = np.ascontiguousarray(shard_of, dtype=np.uint32)
    h = C.c_void_p()
    args = [ptr(o), ptr(docs), ptr(freqs), ptr(m)]
    out = C.byref(h)
    if null is not None:
        if null == 4:
            out = None
        else:
            args[null] = None
    if device is None:
        code = L.ds2i_split_postings(num_docs, n, *args, nshards, 1, out)
    else:
        code = L.ds2i_hip_split_postings(device, num_docs, n, *args, nshards, out, None)
    assert code != 0 and not h.value
    return code, L.ds2i_hip_last_error().decode()


def split_index_rc(L, kind, image, shard_of, nshards, to_kind=0, device=NO_DEVICE, null=None):
    m = np.ascontiguousarray(shard_of, dtype=np.uint32)
    h = C.c_void_p()
    code = L.ds2i_hip_split_index(device, kind, None if null == "image" else image, len(image), None if null == "map" else ptr(m), len(m), nshards,
                                  to_kind, None if null == "out" else C.byref(h), None)
    assert code != 0 and not h.value
    return code, L.ds2i_hip_last_error().decode()


@pytest.fixture(scope="module")
def edge(built_lib):
    coll = rc.block_edge_collection()
    return coll, sc.range_assign(coll.num_docs, sc.EDGE_CUTS), cases.image(coll, "block_optpfor")


def test_null_arguments_offsets_and_no_shard(built_lib, edge):
    L = built_lib
    coll, shard_of, image = edge
    for device in (None, NO_DEVICE):
        for null in range(5):
            code, msg = split_postings_rc(L, coll.num_docs, coll.lists, shard_of, 0, device=device, null=null)  # (before the missing shards)
            assert code == -1 and "null argument" in msg
        offs = _csr(coll.lists)[1]
        bad = offs.copy()
        bad[0] = 1
        code, msg = split_postings_rc(L, coll.num_docs, coll.lists, shard_of, 0, device=device, offs=bad)
        assert code == -1 and "must start at 0" in msg
        bad = offs.copy()
        bad[[2, 3]] = bad[[3, 2]]
        code, msg = split_postings_rc(L, coll.num_docs, coll.lists, shard_of, 0, device=device, offs=bad)
        assert code == -1 and "decrease" in msg
        code, msg = split_postings_rc(L, coll.num_docs, coll.lists, shard_of + 7, 0, device=device)  # (before the values)
        assert code == -1 and "no shard" in msg
    for null in ("image", "map", "out"):
        code, msg = split_index_rc(L, 99, image, shard_of, 0, to_kind=99, null=null)  # (before the shards and the kinds)
        assert code == -1 and "null argument" in msg
    code, msg = split_index_rc(L, 99, image, shard_of, 0, to_kind=99)  # (before the kinds)
    assert code == -1 and "no shard" in msg


def test_too_many_documents_or_lists(built_lib):
    """2^32 documents or lists, before any value of shard_of or any posting is looked at"""
    one = [(np.array([0], dtype=np.uint32), np.array([1], dtype=np.uint32))]
    for device in (None, NO_DEVICE):
        code, msg = split_postings_rc(built_lib, 1 << 32, one, [9], 2, device=device)
        assert code == -1 and "2^32" in msg


def test_kinds_come_before_the_image(built_lib, edge):
    L = built_lib
    coll, shard_of, image = edge
    for img in (image, cases.GARBAGE):
        for kind in (-1, 9, 99):
            code, msg = split_index_rc(L, kind, img, shard_of, 3)
            assert code == -1 and "unknown index kind" in msg
            assert split_index_rc(L, 0, img, shard_of, 3, to_kind=kind)[0] == -1
        for to_kind in ("block_qmx", "block_mixed"):
            code, msg = split_index_rc(L, 0, img, shard_of, 3, to_kind=d.CODECS[to_kind])
            assert code == -1 and all(name in msg for name in cases.GPU_BUILT_KINDS)
    for to_kind in ("block_qmx", "block_mixed"):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_split_index("block_optpfor", image, shard_of, to_kind=to_kind, device=NO_DEVICE)
        assert e.value.code == -1 and all(name in str(e.value) for name in cases.GPU_BUILT_KINDS)


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_a_garbage_image_comes_before_the_map(built_lib, kind):
    bad = np.full(7, 1000, dtype=np.uint32)  # a wrong length and values outside the shards: the image is looked at first
    code, _ = split_index_rc(built_lib, d.CODECS[kind], cases.GARBAGE, bad, 3)
    assert code == -2
    with pytest.raises(d.Ds2iError) as e:  # the host parse on its own says the same
        d.image_shape(kind, cases.GARBAGE)
    assert e.value.code == -2
    with pytest.raises(d.Ds2iError) as e:
        d.image_shape(9, cases.GARBAGE)
    assert e.value.code == -1 and "unknown index kind" in str(e.value)
    coll = rc.block_edge_collection()
    assert d.image_shape(kind, cases.image(coll, kind)) == (coll.num_docs, len(coll.lists))


def test_map_then_device(built_lib, edge):
    """the refusals over shard_of from the twin and both device forms, then the missing device"""
    L = built_lib
    coll, shard_of, image = edge
    n = coll.num_docs

    def all_three(m, nshards):
        return [split_postings_rc(L, n, coll.lists, m, nshards), split_postings_rc(L, n, coll.lists, m, nshards, device=NO_DEVICE),
                split_index_rc(L, 0, image, m, nshards)]

    # a wrong length, although what it holds lies outside the shards too: the length is named
    code, msg = split_index_rc(L, 0, image, np.full(n - 1, 1000, dtype=np.uint32), 3)
    assert code == -1 and "shard_of holds %d documents, the index %d" % (n - 1, n) in msg
    for call in (d.split_postings, d.gpu_split_postings):
        with pytest.raises(ValueError):
            call(n, coll.lists, shard_of[:-1])
    # a shard number >= nshards: the first document is named; the drop value is none
    bad = shard_of.copy()
    bad[[41, 77]] = [3, 9]
    for code, msg in all_three(bad, 3):
        assert code == -1 and "document 41 is sent to shard 3, outside the 3 shards" in msg
    bad[41] = d.DROP
    for code, msg in all_three(bad, 3):
        assert code == -1 and "document 77 is sent to shard 9" in msg
    # a shard with no document: the images' form names the first, before the device; the postings' forms hand it back empty
    code, msg = split_index_rc(L, 0, image, np.where(shard_of == 1, 3, shard_of).astype(np.uint32), 5)
    assert code == -1 and "shard 1 is assigned no document" in msg
    assert d.split_postings(n, coll.lists, shard_of, nshards=5)[4][0] == 0
    # all is well but the device
    for code, msg in (split_postings_rc(L, n, coll.lists, shard_of, 3, device=NO_DEVICE), split_index_rc(L, 0, image, shard_of, 3)):
        assert code == -4 and "no such HIP device" in msg
    for call in (lambda: d.gpu_split_postings(n, coll.lists, shard_of, device=NO_DEVICE),
                 lambda: d.gpu_split_index("block_optpfor", image, shard_of, to_kind="opt", device=NO_DEVICE)):
        with pytest.raises(d.Ds2iError) as e:
            call()
        assert e.value.code == -4


def test_host_twin_refuses_a_doc_id_outside_the_documents(built_lib):
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    code, msg = split_postings_rc(built_lib, 10, [(one(3, 9), one(1, 1)), (one(2, 10), one(1, 1))], np.arange(10) % 2, 2)
    assert code == -2 and "list 1 holds doc-id 10, outside the 10 documents" in msg


# ---------------------------------------------------------------- the host side under the sanitizers, as a program of its own
def test_twin_check_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """host_split.hpp and tests/split_twin_check.cpp (its own main) compiled with -fsanitize=address,undefined and run: nothing that is
    loaded into this interpreter runs under a sanitizer"""
    exe = str(tmp_path / "split_twin_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread",  # (the runtimes inside the program: it asks nothing of its loader)
                           os.path.join(ROOT, "tests", "split_twin_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and p.stdout == "OK\n" and p.stderr == "", (p.stdout, p.stderr)


# ---------------------------------------------------------------- the tool
def test_tool_usage_errors_without_a_device(built_lib, edge, tmp_path):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])

    def run(*args):
        p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return p.returncode, p.stdout, p.stderr

    coll, shard_of, image = edge
    a, out = str(tmp_path / "a"), str(tmp_path / "out")
    open(a, "wb").write(image)
    good, short = str(tmp_path / "assign"), str(tmp_path / "short")
    rc.write_map(good, shard_of)
    open(short, "wb").write(open(good, "rb").read()[:-4])
    base = ("block_optpfor", a, "opt", out)
    for args in (base, base[:3] + ("--assign", good), base + ("extra", "--assign", good), base + ("--assign",), base + ("--ranges",),
                 base + ("--assign", good, "--ranges", "5"),            # one or the other
                 base + ("--assign", good, "--assign", good),
                 base + ("--ranges", "7,7"), base + ("--ranges", "9,3"), base + ("--ranges", "0"), base + ("--ranges", "5,"), base + ("--ranges", "x"),
                 base + ("--assign", good, "--device", "-1"), base + ("--assign", good, "--frobnicate")):
        rcode, stdout, err = run(*args)
        assert rcode == 2 and stdout == "" and "usage" in err, (args, err)
    for bad in (str(tmp_path / "missing"), short):
        rcode, stdout, err = run(*base, "--assign", bad)
        assert rcode == 2 and stdout == "" and "usage" in err, (bad, err)
    assert run("nonsense", a, "opt", out, "--assign", good)[0] == 2 and run("opt", a, "nonsense", out, "--assign", good)[0] == 2
    rcode, _, err = run("block_optpfor", a, "block_qmx", out, "--assign", good)
    assert rcode == 2 and all(name in err for name in cases.GPU_BUILT_KINDS)
    # a cut at or past the last document is found on the host parse of the input: no device is looked for
    for cuts in ("7300,%d" % coll.num_docs, str(coll.num_docs + 5)):
        rcode, stdout, err = run(*base, "--ranges", cuts, "--device", str(NO_DEVICE))
        assert rcode == 2 and stdout == "" and "lies outside the %d documents" % coll.num_docs in err, err
    rcode, stdout, err = run(*base, "--ranges", "7300,30001", "--device", str(NO_DEVICE))
    assert rcode == 2 and stdout == "" and "no such HIP device" in err
    # a shard without a document is the library's answer; so is the missing device once all is well
    hole = str(tmp_path / "hole")
    rc.write_map(hole, np.where(shard_of == 1, 4, shard_of))
    rcode, stdout, err = run(*base, "--assign", hole, "--device", str(NO_DEVICE))
    assert rcode == 2 and stdout == "" and "shard 1 is assigned no document" in err
    rcode, stdout, err = run("--check", "block_optpfor", "--device", str(NO_DEVICE), a, "--assign", good, "opt", out)  # (flags in any place)
    assert rcode == 2 and stdout == "" and "no such HIP device" in err
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("out")]
