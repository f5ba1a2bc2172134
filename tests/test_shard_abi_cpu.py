"""Querying shards as one index, on a CPU-only box: the host twin of the merge against numpy over the shape list, split_wand against
wand_arrays and numpy, the references of shard_cases against each other (a set's brute force equals the whole collection's for queries
of at most two distinct terms), and every answer of the new entry points that needs no device, in the order the headers state, each
before the missing device is noticed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
import shard_cases as shc
import split_cases as sc
import verify_cases as cases
from ds2i_amd.api import ShardSource, TopkRows
from helpers import Collection, small_params
from test_host_parallel_cpu import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 99
HIP_ARGS = {"ds2i_hip_index_set_collection_stats": 4, "ds2i_hip_merge_topk": 9, "ds2i_hip_shard_set_open": 7, "ds2i_hip_shard_set_query": 11}
BUILD_ARGS = {"ds2i_split_wand": 7, "ds2i_wand_arrays": 4, "ds2i_merge_topk": 8}


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
    hip = open(os.path.join(ROOT, "include", "ds2i_hip.h")).read()
    build = open(os.path.join(ROOT, "include", "ds2i_build.h")).read()
    assert "#define DS2I_HIP_MAX_SHARDS 64" in hip and d.MAX_SHARDS == 64
    assert "must NOT run concurrently with planning" in hip           # set_collection_stats says so
    assert "NOT the image ds2i_wand_create gives over the shard" in build
    assert "Not split: wand data" not in build and "ds2i_split_wand" in build
    assert d.Index.set_collection_stats and d.ShardSet.from_split and d.split_wand and d.wand_arrays and d.merge_topk and d.gpu_merge_topk
    assert d.merge_topk_grid(256, 1024) == 5 * 256 and d.merge_topk_grid(256, 128) == d.merge_topk_grid(256, 1) == 32 * 256


# ---------------------------------------------------------------- the twin of the merge
def test_twin_equals_numpy_over_the_shape_list(built_lib):
    shapes = shc.merge_shapes(lambda k: d.merge_topk_grid(256, k))
    assert {s[1] for s in shapes} >= set(shc.MERGE_NROWS) and {s[2] for s in shapes} >= set(shc.MERGE_KS)
    assert any(s[3] == 65 for s in shapes) and sum(s[3] > d.merge_topk_grid(256, s[2]) for s in shapes) >= 2
    for shape in shapes:
        rows = shc.merge_rows(shape)
        k = shape[2]
        want = shc.numpy_merge_topk(rows, k)
        shc.assert_rows_equal(d.merge_topk(rows, k), want, shape)
        shc.assert_rows_equal(d.merge_topk(rows, k, threads=3), want, shape)
        if shape[0] in ("equal_interleaved", "equal_interleaved_permuted"):  # the whole order rests on the ids, across the row sets
            ids = want[1][0].astype(np.int64)
            assert np.all(np.diff(ids) > 0) and len({int(i - 7) % shape[1] for i in ids}) == shape[1]
        if shape[0] == "high":
            assert int(want[1].max(initial=0, where=want[1] != shc.NO_DOC)) > 1 << 24
    high = shc.merge_rows(next(s for s in shapes if s[0] == "high"))
    assert int(high[-1][3].max()) == 0xFFFFFFFE and int(high[-1][1][0, :int(high[-1][2][0])].max()) == len(high[-1][3]) - 1
    one = [(np.array([[1.0, 1.0]], np.float32), np.array([[0, 1]], np.uint32), np.array([2], np.uint32), np.array([0xFFFFFFFE, 1 << 31], np.uint32))]
    assert d.merge_topk(one, 2)[1].tolist() == [[1 << 31, 0xFFFFFFFE]] and shc.numpy_merge_topk(one, 2)[1].tolist() == [[1 << 31, 0xFFFFFFFE]]


def test_numpy_merge_is_the_definition_on_a_case_by_hand(built_lib):
    inf = -np.inf
    a = (np.array([[3.0, 1.0, inf]], np.float32), np.array([[4, 0, 9]], np.uint32), np.array([2], np.uint32), np.array([10, 11, 12, 13, 5], np.uint32))
    b = (np.array([[3.0, 3.0, 0.5]], np.float32), np.array([[2, 7, 1]], np.uint32), np.array([3], np.uint32), None)
    for merge in (shc.numpy_merge_topk, d.merge_topk):
        s, dd, ll = merge([a, b], 3)
        assert s.tolist() == [[3.0, 3.0, 3.0]] and dd.tolist() == [[2, 5, 7]] and ll.tolist() == [3]
    s, dd, ll = d.merge_topk([a], 3)
    assert s.tolist() == [[3.0, 1.0, inf]] and dd.tolist() == [[5, 10, 0xFFFFFFFF]] and ll.tolist() == [2]


def merge_rc(L, rows, nrows, nq, k, device=None, null=None, out_null=False):
    """(code, message) of ds2i_merge_topk (device None) or ds2i_hip_merge_topk; rows: TopkRows array or None"""
    s = np.zeros(max(nq * k, 1), np.float32)
    dd = np.zeros(max(nq * k, 1), np.uint32)
    ll = np.zeros(max(nq, 1), np.uint32)
    outs = [None if out_null else ptr(s), ptr(dd), ptr(ll)]
    if device is None:
        code = L.ds2i_merge_topk(rows, nrows, nq, k, *outs, 1)
    else:
        code = L.ds2i_hip_merge_topk(device, rows, nrows, nq, k, *outs, None)
    return code, L.ds2i_hip_last_error().decode()


def _rows_struct(rows):
    from ds2i_amd.api import _topk_rows
    return _topk_rows(rows, rows[0][0].shape[1])


@pytest.mark.parametrize("device", [None, NO_DEVICE])
def test_merge_argument_checks_in_order_before_any_device(built_lib, device):
    L = built_lib
    k, nq = 4, 3
    good = [(np.tile(np.array([3, 2, 1, 0.5], np.float32), (nq, 1)), np.tile(np.arange(4, dtype=np.uint32), (nq, 1)), np.full(nq, 4, np.uint32),
             np.arange(10, 20, dtype=np.uint32)) for _ in range(2)]
    arr, n, _, _, keep = _rows_struct(good)
    assert merge_rc(L, None, 0, nq, 0, device)[0] == -1 and "null argument" in merge_rc(L, None, 0, nq, 0, device)[1]
    code, msg = merge_rc(L, arr, 0, nq, 0, device, out_null=True)     # (before the number of row sets and k)
    assert code == -1 and "null argument" in msg
    code, msg = merge_rc(L, arr, 0, nq, 0, device)                    # (nrows before k)
    assert code == -1 and "row sets" in msg
    many = (TopkRows * 65)(*([arr[0]] * 65))
    code, msg = merge_rc(L, many, 65, nq, 0, device)
    assert code == -1 and "65 row sets" in msg
    for bad_k in (0, 1025):
        code, msg = merge_rc(L, arr, 2, nq, bad_k, device)
        assert code == -1 and "k = %d" % bad_k in msg
    # a length above k comes before a bad score, a bad score before a bad id
    bad = [tuple(np.copy(x) for x in r) for r in good]
    bad[1][2][2] = 5
    bad[0][0][0, 0] = -1.0
    bad[0][1][0, 0] = 10
    arr2, _, _, _, keep2 = _rows_struct(bad)
    code, msg = merge_rc(L, arr2, 2, nq, k, device)
    assert code == -1 and "row set 1, query 2" in msg and "above k" in msg
    bad[1][2][2] = 4
    for value in (-1.0, -0.0, np.inf, np.nan):
        bad[0][0][1, 2] = value
        bad[1][0][0, 0] = np.nan                                      # (a later row set: the first offender is named)
        arr2, _, _, _, keep2 = _rows_struct(bad)
        code, msg = merge_rc(L, arr2, 2, nq, k, device)
        assert code == -1 and "row set 0, query 0, position 0" in msg and "negative or not finite" in msg
        bad[0][0][0, 0] = 3.0
        arr2, _, _, _, keep2 = _rows_struct(bad)
        code, msg = merge_rc(L, arr2, 2, nq, k, device)
        assert code == -1 and "row set 0, query 1, position 2" in msg, (value, msg)
        bad[0][0][0, 0] = -1.0
    bad[0][0][0, 0], bad[0][0][1, 2], bad[1][0][0, 0] = 3.0, 1.0, 3.0
    arr2, _, _, _, keep2 = _rows_struct(bad)
    code, msg = merge_rc(L, arr2, 2, nq, k, device)
    assert code == -1 and "row set 0, query 0, position 0" in msg and "local doc-id 10 lies outside the map of 10" in msg
    # entries past a row's length are not looked at
    bad[0][1][0, 0] = 0
    bad[0][2][1] = 2
    bad[0][0][1, 2:], bad[0][1][1, 2:] = np.nan, 4000
    arr2, _, _, _, keep2 = _rows_struct(bad)
    code, msg = merge_rc(L, arr2, 2, nq, k, device)
    assert (code == 0) if device is None else (code == -4 and "no such HIP device" in msg), msg
    # no query: success, nothing written, no device needed
    assert merge_rc(L, arr, 2, 0, k, device)[0] == 0
    if device is not None:
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_merge_topk(good, device=NO_DEVICE)
        assert e.value.code == -4


def test_a_repeated_collection_id_is_kept_twice_and_nothing_else_moves(built_lib):
    """two candidates with one collection id are the caller's error: both may come back, in bounds"""
    a = (np.array([[2.0, 1.0]], np.float32), np.array([[3, 4]], np.uint32), np.array([2], np.uint32), None)
    s, dd, ll = d.merge_topk([a, a, a], 2)
    assert s.tolist() == [[2.0, 2.0]] and dd.tolist() == [[3, 3]] and ll.tolist() == [2]


# ---------------------------------------------------------------- wand data
@pytest.fixture(scope="module")
def small(built_lib):
    coll = Collection(small_params())
    shard_of = sc.range_assign(coll.num_docs, (7000, 13001))
    shards = d.split_postings(coll.num_docs, coll.lists, shard_of)
    return coll, shards, coll.wand_image()


def test_split_wand_gathers_the_collections_arrays(built_lib, small):
    coll, shards, wand = small
    nl, mw = d.wand_arrays(wand)
    assert nl.dtype == np.float32 and np.array_equal(shc.bits(nl), shc.bits(coll.norm_lens)) and len(mw) == len(coll.lists)
    for n, lists, doc_map, term_map in shards:
        img = d.split_wand(wand, doc_map, term_map)
        a, b = d.wand_arrays(img)
        assert np.array_equal(shc.bits(a), shc.bits(nl[doc_map])) and np.array_equal(shc.bits(b), shc.bits(mw[term_map]))
        own = d.build_wand(coll.sizes[doc_map], lists)                # the shard's own normalisation is another image
        assert own != img and len(own) == len(img)
        assert np.all(d.wand_arrays(own)[1] > 0)
    perm = np.random.default_rng(5).permutation(coll.num_docs).astype(np.uint32)[:100]  # the maps need not be increasing
    a, b = d.wand_arrays(d.split_wand(wand, perm, [7, 3, 3]))
    assert np.array_equal(shc.bits(a), shc.bits(nl[perm])) and np.array_equal(shc.bits(b), shc.bits(mw[[7, 3, 3]]))
    a, b = d.wand_arrays(d.split_wand(wand, [], []))
    assert len(a) == 0 and len(b) == 0


def test_split_wand_refusals(built_lib, small):
    L = built_lib
    coll, shards, wand = small
    V = len(coll.lists)
    h = C.c_void_p()
    m = np.arange(4, dtype=np.uint32)
    assert L.ds2i_split_wand(None, len(wand), ptr(m), 4, ptr(m), 4, C.byref(h)) == -1 and "null argument" in L.ds2i_hip_last_error().decode()
    assert L.ds2i_split_wand(wand, len(wand), None, 4, ptr(m), 4, C.byref(h)) == -1
    assert L.ds2i_split_wand(wand, len(wand), ptr(m), 4, ptr(m), 4, None) == -1
    for call, text in ((lambda: d.split_wand(wand, [0, coll.num_docs, coll.num_docs + 3], [V]), "doc_map[1] = %d" % coll.num_docs),
                       (lambda: d.split_wand(wand, [0, 1], [0, V + 2, V]), "term_map[1] = %d" % (V + 2))):
        with pytest.raises(d.Ds2iError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value)
    with pytest.raises(d.Ds2iError) as e:
        d.split_wand(cases.GARBAGE, [0], [0])
    assert e.value.code == -2
    with pytest.raises(d.Ds2iError) as e:
        d.wand_arrays(cases.GARBAGE)
    assert e.value.code == -2
    assert not h.value


# ---------------------------------------------------------------- the references against each other
def test_translate():
    tm = [2, 5, 9]
    qs = [[], [5], [5, 5, 2], [5, 7], [7], [9, 2, 9, 3]]
    assert shc.translate(qs, tm, True) == [[], [1], [1, 1, 0], [], [], []]
    assert shc.translate(qs, tm, False) == [[], [1], [1, 1, 0], [1], [], [2, 0, 2]]
    assert shc.translate(qs, [], False) == [[]] * 6


def test_the_query_list_meets_the_conditions_the_set_tests_rest_on(built_lib, small):
    coll, shards, _ = small
    qs = shc.set_queries(len(coll.lists))
    small_q, large_q, full, multi = shc.set_conditions(coll, shards, qs, 10)
    assert small_q >= 40 and large_q >= 40 and full >= 0.5 and multi >= 0.25, (small_q, large_q, full, multi)


@pytest.mark.parametrize("how", ["range", "rr2"])
def test_a_sets_brute_force_is_the_whole_collections_for_two_terms(built_lib, small, how):
    """with nothing dropped the default statistics are the collection's own, and a sum of two separately rounded products commutes"""
    coll, shards, _ = small
    if how == "rr2":
        shards = d.split_postings(coll.num_docs, coll.lists, sc.round_robin_assign(coll.num_docs, 2))
    views = shc.shard_views(coll, shards)
    whole = shc.own_view(coll.num_docs, coll.lists, coll.norm_lens)
    assert views[0].N == coll.num_docs and np.array_equal(shc.collection_df(shards, len(coll.lists)), [len(dd) for dd, _ in coll.lists])
    qs = [q for q in shc.set_queries(len(coll.lists)) if shc.distinct_terms(q) <= 2][:24]
    for conj in (True, False):
        (s, dd, ll), rows = shc.set_rows(coll, shards, views, qs, 10, conj)
        shc.assert_rows_equal(d.merge_topk(rows, 10), (s, dd, ll))
        for i, q in enumerate(qs):
            ws, wd = shc.view_pairs(whole, q, 10, conj)
            assert int(ll[i]) == len(wd) and np.array_equal(dd[i, :len(wd)], wd) and np.array_equal(shc.bits(s[i, :len(wd)]), shc.bits(ws)), (how, conj, q)


# ---------------------------------------------------------------- refusals of the statistics and of the set, without a device
def test_set_collection_stats_refuses_a_null_index(built_lib):
    df = np.ones(3, np.uint32)
    assert built_lib.ds2i_hip_index_set_collection_stats(None, 5, ptr(df), 3) == -1
    assert "null index" in built_lib.ds2i_hip_last_error().decode()
    assert built_lib.ds2i_hip_index_set_collection_stats(None, 0, None, 0) == -1


def open_rc(L, sources, collection_docs, collection_terms, num_docs=0, df=None, nshards=None, null=None):
    """(code, message) of ds2i_hip_shard_set_open over (kind, image, doc_map, term_map) sources on a device that does not exist"""
    arr, keep = (ShardSource * max(1, len(sources)))(), []
    for src, (kind, image, doc_map, term_map) in zip(arr, sources):
        dm, tm = np.ascontiguousarray(doc_map, np.uint32), np.ascontiguousarray(term_map, np.uint32)
        keep.extend((image, dm, tm))
        src.device, src.kind = NO_DEVICE, kind
        src.image, src.bytes = C.cast(C.c_char_p(image), C.c_void_p), len(image)
        src.doc_map, src.map_len, src.term_map, src.terms_len = dm.ctypes.data, len(dm), tm.ctypes.data, len(tm)
    if null == "image":
        arr[0].image = None
    if null == "map":
        arr[len(sources) - 1].doc_map = None
    h = C.c_void_p()
    a = None if df is None else np.ascontiguousarray(df, np.uint32)
    code = L.ds2i_hip_shard_set_open(None if null == "src" else arr, len(sources) if nshards is None else nshards, collection_docs, collection_terms,
                                     num_docs, None if a is None else ptr(a), None if null == "out" else C.byref(h))
    assert code != 0 and not h.value
    return code, L.ds2i_hip_last_error().decode()


def test_shard_set_open_checks_in_order_before_any_device(built_lib, small):
    L = built_lib
    coll, shards, _ = small
    N, V = coll.num_docs, len(coll.lists)
    good = [(0, sc.shard_image(("small", "range3", s), coll, sh, "block_optpfor"), sh[2], sh[3]) for s, sh in enumerate(shards)]
    for null in ("src", "out", "image", "map"):
        code, msg = open_rc(L, good, N, V, nshards=0 if null in ("src", "out") else None, null=null)  # (before the number of shards)
        assert code == -1 and "null argument" in msg, null
    for n in (0, 65):
        code, msg = open_rc(L, [(99, cases.GARBAGE, [], [])] * min(n, 64) or good, N, V, nshards=n)  # (before the kinds)
        assert code == -1 and "%d shards" % n in msg
    code, msg = open_rc(L, [good[0], (9, cases.GARBAGE, [], [])], N, V)                # the kinds before the images
    assert code == -1 and "shard 1: unknown index kind" in msg
    code, msg = open_rc(L, [good[0], (0, cases.GARBAGE, good[1][2][:-1], [])], N, V)   # an image before the lengths of the maps
    assert code == -2
    code, msg = open_rc(L, [good[0], good[1][:2] + (good[1][2][:-1], good[1][3][::-1])], N, V)  # the lengths before the values
    assert code == -1 and "shard 1: doc_map holds %d documents, the index %d" % (shards[1][0] - 1, shards[1][0]) in msg
    code, msg = open_rc(L, [good[0], good[1][:3] + (good[1][3][:-1],)], N, V)
    assert code == -1 and "shard 1: term_map holds" in msg
    # term maps: strictly increasing and inside the collection, before the doc maps
    twice = good[1][2].copy()
    twice[5] = good[0][2][3]
    tm = good[1][3].copy()
    tm[[4, 5]] = tm[[5, 4]]
    code, msg = open_rc(L, [good[0], (0, good[1][1], twice, tm)], N, V)
    assert code == -1 and "shard 1: term_map does not increase at entry 5" in msg
    code, msg = open_rc(L, [good[0], (0, good[1][1], twice, good[1][3])], N, int(good[1][3][-1]))
    assert code == -1 and "term_map[%d] = %d lies outside" % (len(good[1][3]) - 1, int(good[1][3][-1])) in msg
    # doc maps: inside the collection, no id twice across the set, the first offender named
    code, msg = open_rc(L, [good[0], (0, good[1][1], twice, good[1][3])], N, V)
    assert code == -1 and "shard 1: document 5 maps to %d, which an earlier document took" % int(twice[5]) in msg
    code, msg = open_rc(L, good, int(good[2][2][-1]), V)
    assert code == -1 and "shard 2: document %d maps to %d, outside" % (shards[2][0] - 1, int(good[2][2][-1])) in msg
    # the statistics: a df below the sum of the shard lists or above the documents, a collection smaller than its shards
    df = shc.collection_df(shards, V)
    low = df.copy()
    low[17] -= 1
    code, msg = open_rc(L, good, N, V, df=low)
    assert code == -1 and "term 17: df %d" % low[17] in msg
    high = df.copy()
    high[3] = N + 5
    code, msg = open_rc(L, good, N, V, num_docs=N + 4, df=high)
    assert code == -1 and "term 3: df %d" % (N + 5) in msg
    code, msg = open_rc(L, good[:1], N, V, num_docs=shards[0][0] - 1)
    assert code == -1 and ("smaller than shard 0" in msg or "df" in msg)
    # all is well but the device -- also with statistics larger than the sums
    for kw in ({}, {"num_docs": N + 100, "df": df + 1}):
        code, msg = open_rc(L, good, N, V, **kw)
        assert code == -4 and "no such HIP device" in msg
    with pytest.raises(d.Ds2iError) as e:
        d.ShardSet([(0, g[1], None, g[2], g[3], NO_DEVICE) for g in good], N, V)
    assert e.value.code == -4
    with pytest.raises(ValueError):
        d.ShardSet([(0, g[1], None, g[2], g[3], NO_DEVICE) for g in good], N, V, df=df[:-1])


def test_shard_set_query_and_close_take_a_null_set(built_lib):
    offs = np.zeros(2, np.uint32)
    assert built_lib.ds2i_hip_shard_set_query(None, 4, 10, None, ptr(offs), 1, None, None, None, None, None) == -1
    assert "null argument" in built_lib.ds2i_hip_last_error().decode()
    built_lib.ds2i_hip_shard_set_close(None)


# ---------------------------------------------------------------- the tools
def _run(tool, *args, stdin=""):
    exe = os.path.join(ROOT, "ds2i_amd", "tools", tool)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe), "-s"])
    p = subprocess.run([exe] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    return p.returncode, p.stdout, p.stderr


def test_split_index_wand_option_errors_without_a_device(built_lib, small, tmp_path):
    import remap_cases as rc
    coll, shards, wand = small
    a, w, out = str(tmp_path / "a"), str(tmp_path / "a.wand"), str(tmp_path / "out")
    open(a, "wb").write(cases.image(coll, "block_optpfor"))
    open(w, "wb").write(wand)
    other = str(tmp_path / "other.wand")
    open(other, "wb").write(d.split_wand(wand, np.arange(100), np.arange(len(coll.lists))))  # the wand data of 100 documents
    base = ("block_optpfor", a, "opt", out, "--ranges", "7000,13001")
    for args in (base + ("--wand",), base + ("--wand", w, "--wand", w), base + ("--wand", str(tmp_path / "missing"))):
        code, stdout, err = _run("split_index", *args)
        assert code == 2 and stdout == "" and "usage" in err and "--wand" in err, (args, err)
    code, stdout, err = _run("split_index", *base, "--wand", other, "--device", str(NO_DEVICE))
    assert code == 2 and stdout == "" and "--wand: the wand data holds 100 documents" in err
    code, stdout, err = _run("split_index", *base, "--wand", cases_garbage_file(tmp_path), "--device", str(NO_DEVICE))
    assert code == 2 and stdout == "" and "ds2i_wand_arrays failed" in err
    code, stdout, err = _run("split_index", *base, "--wand", w, "--device", str(NO_DEVICE))  # all is well but the device
    assert code == 2 and stdout == "" and "no such HIP device" in err
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("out")]
    assert rc.write_map  # (the maps of the shards below are written by the same helper the split tests use)


def cases_garbage_file(tmp_path):
    path = str(tmp_path / "garbage")
    open(path, "wb").write(cases.GARBAGE)
    return path


def test_shard_queries_errors_without_a_device(built_lib, small, tmp_path):
    import remap_cases as rc
    coll, shards, wand = small
    prefix = str(tmp_path / "sh")
    for s, sh in enumerate(shards):
        open("%s.%d" % (prefix, s), "wb").write(sc.shard_image(("small", "range3", s), coll, sh, "block_optpfor"))
        rc.write_map("%s.%d.docs" % (prefix, s), sh[2])
        rc.write_map("%s.%d.terms" % (prefix, s), sh[3])
    log = "1 2\n3\n"
    good = ("block_optpfor", "ranked_and", prefix, "3")
    for args in (good[:3], good + ("extra",), good[:3] + ("0",), good[:3] + ("65",), good[:3] + ("x",), good + ("--k", "0"), good + ("--k", "1025"),
                 good + ("--k",), good + ("--devices", "a"), good + ("--devices", "0,"), good + ("--devices", "-1"), good + ("--frobnicate",)):
        code, stdout, err = _run("shard_queries", *args, stdin=log)
        assert code == 2 and stdout == "" and "usage" in err, (args, err)
    code, stdout, err = _run("shard_queries", "nonsense", *good[1:], stdin=log)
    assert code == 2 and stdout == "" and "Unknown type" in err
    for op in ("and_freq", "ranked_and:or_freq", "frob"):
        code, stdout, err = _run("shard_queries", good[0], op, *good[2:], stdin=log)
        assert code == 2 and stdout == "" and "Unsupported query type over shards" in err
    code, stdout, err = _run("shard_queries", *good[:3], "4", stdin=log)                    # a shard that is not there
    assert code == 2 and stdout == "" and "cannot open" in err
    code, stdout, err = _run("shard_queries", *good, stdin=log)                             # a ranked operator without the wand files
    assert code == 2 and stdout == "" and "needs" in err and ".wand" in err
    open(prefix + ".1.docs", "ab").write(b"\0\0\0\0")
    code, stdout, err = _run("shard_queries", good[0], "and", *good[2:], stdin=log)         # a map file that is too long
    assert code == 2 and stdout == "" and "is no binary sequence" in err
    rc.write_map(prefix + ".1.docs", shards[1][2])
    for s, sh in enumerate(shards):
        open("%s.%d.wand" % (prefix, s), "wb").write(d.split_wand(wand, sh[2], sh[3]))
    for op in ("and", "ranked_and:wand"):                                                   # all is well but the device
        code, stdout, err = _run("shard_queries", good[0], op, *good[2:], "--devices", "%d,%d" % (NO_DEVICE, NO_DEVICE + 1), "--print", stdin=log)
        assert code == 2 and stdout == "" and "no such HIP device" in err, err


# ---------------------------------------------------------------- the host side under the sanitizers, as programs of their own
def test_twin_check_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """host_shard.hpp and tests/shard_twin_check.cpp (its own main) compiled with -fsanitize=address,undefined and run as a child
    process: nothing that is loaded into this interpreter runs under a sanitizer"""
    exe = str(tmp_path / "shard_twin_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread", os.path.join(ROOT, "tests", "shard_twin_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and p.stdout == "OK\n" and p.stderr == "", (p.stdout, p.stderr)


def test_plans_with_collection_statistics_hold_under_asan_ubsan(tmp_path):
    """tests/shard_plan_check.cpp with batch_plan.cpp by the host compiler alone: the same batches planned with and without statistics"""
    exe = str(tmp_path / "shard_plan_check")
    srcs = [os.path.join(ROOT, "tests", "shard_plan_check.cpp"), os.path.join(ROOT, "ds2i_amd", "csrc", "batch_plan.cpp")]
    built = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined"] + srcs + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-4000:]
    last = run.stdout.splitlines()[-1]
    assert last.startswith("shard_plan: ") and last.endswith(" plans hold") and int(last.split()[1]) >= 16, run.stdout[-2000:]
