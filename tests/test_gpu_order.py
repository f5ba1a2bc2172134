"""Ordering documents on the GPU (-m gpu): ds2i_hip_order_postings and ds2i_hip_order_index against the host twin (ds2i_order_postings),
map and trace, element for element with np.array_equal; Index.order() on images of three kinds, its map applied by Index.remap and
verified; and the order_documents tool feeding convert_index --remap. Everything is integers: no tolerance anywhere. A case that reaches
the int32 clamp of a gain needs a document of millions of terms and is left to the host helper (test_order_abi_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (the GPU suite runs where torch sees the device)

import ds2i_amd as d
import order_cases as oc
from helpers import Collection

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "ds2i_amd", "tools")
ORDER, CONVERT = os.path.join(TOOLS, "order_documents"), os.path.join(TOOLS, "convert_index")
PARTS = ("extract_ms", "level_sort_ms", "runs_ms", "degrees_ms", "gains_ms", "gain_sort_ms", "swap_ms", "compose_ms")
SMALL = {name: (n, lists, prm) for name, n, lists, prm in oc.small_cases()}


def check(name, n, lists, prm):
    """gpu_order_postings == the twin; device_ms is the sum of its parts; returns (map, trace, info)"""
    (m, tr), info = d.gpu_order_postings(n, lists, **prm)
    wm, wt = oc.twin(name, n, lists, prm)
    assert m.dtype == np.uint32 and tr.dtype == np.uint64 and len(m) == n
    same = np.array_equal(m, wm)
    if not np.array_equal(tr, wt) or not same:
        k = min(len(tr), len(wt))
        bad = np.flatnonzero(tr[:k] != wt[:k])
        print("%s: trace lengths %d / %d, first differing iteration %s; maps equal: %s" % (name, len(tr), len(wt), bad[:1].tolist(), same))
    assert np.array_equal(tr, wt), name
    assert same, name
    assert abs(info["device_ms"] - sum(info[p] for p in PARTS)) < 1e-6 and info["extract_ms"] == 0
    return m, tr, info


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_cases_equal_the_twin(built_lib, name):
    """0, 1, 2 * min_half - 1 and 2 * min_half documents; odd sizes; halves of 63 / 64 and 64 / 65 documents; 1000 documents with
    min_half = 1, down to halves of one and two documents; ties; iterations = 1, max_levels = 1, zeros as defaults; no list, empty lists"""
    n, lists, prm = SMALL[name]
    m, tr, info = check(name, n, lists, prm)
    d.check_doc_map(m, n)
    levels = oc.level_count(n, prm.get("min_half", 0), prm.get("max_levels", 0))
    assert len(tr) >= levels
    if not levels:
        assert np.array_equal(m, np.arange(n)) and info["device_ms"] == 0


def test_the_small_cases_are_what_they_claim(built_lib):
    assert oc.level_count(31) == 0 and oc.level_count(32) == 1 and oc.level_count(1000, min_half=1) == 9
    W = d.remap_class_bounds()[0]
    assert (127 >> 1, 127 - (127 >> 1)) == (W - 1, W) and (129 >> 1, 129 - (129 >> 1)) == (W, W + 1)
    _, tr, _ = check("identical", *SMALL["identical"])
    assert tr.tolist() == [0] * oc.level_count(110)  # every gain equal and not positive: one iteration a level, nothing exchanged
    _, tr, _ = check("identical, restless", *SMALL["identical, restless"])
    assert tr[0] == 0 and set(tr[1:21].tolist()) == {100} and len(tr) > 21  # level 1: all 2 * 50 pairs, in each of the 20 iterations
    m, tr, _ = check("two kinds", *SMALL["two kinds"])
    assert tr[0] > 0 and tr[1] == 0  # level 0 stops after its second iteration, long before `iterations`
    first = np.sort(m[SMALL["two kinds"][1][0]])
    assert np.array_equal(first, np.arange(128)) or np.array_equal(first, 128 + np.arange(128))  # the kinds are apart
    _, tr, _ = check("one iteration", *SMALL["one iteration"])
    assert len(tr) == oc.level_count(500)
    _, tr, info = check("one level only", *SMALL["one level only"])
    assert len(tr) <= 20 and info["level_sort_ms"] == 0
    assert np.array_equal(tr, check("zeros", *SMALL["zeros"])[1][:len(tr)])


def test_class3_halves_and_every_list_length(built_lib):
    """2 (2 T + 1) + 1 documents: the top halves longer than a workgroup sorts, where ties are kept in p0 order by sorting by p0 first;
    the levels below have halves of T + 1 and L, then down through W + 1 and W; duplicated documents, a term in every document and in
    one, empty lists, documents without terms, lists on both sides of W, L and T (the level-start sort of the lists)"""
    W, L, T = bounds = d.remap_class_bounds()
    n, lists = oc.class3(bounds)
    sizes = {int(((k + 1) * n >> lv) - (k * n >> lv)) for lv in range(1, 11) for k in range(1 << lv)}
    assert n == 2 * (2 * T + 1) + 1 and {2 * T + 1, 2 * T + 2, T + 1, L, W + 1, W} <= sizes and max(sizes) > L
    assert {len(x) for x in lists} >= {0, 1, n, W - 1, W, W + 1, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T + 1}
    m, tr, info = check("class3", n, lists, {})
    d.check_doc_map(m, n)
    assert oc.level_count(n) == 10 and len(tr) >= 10
    for p in PARTS[1:]:
        assert info[p] > 0, p


def test_two_runs_give_the_same_bytes(built_lib):
    n, lists = oc.topical(1000)
    (m1, t1), _ = d.gpu_order_postings(n, lists, min_half=4)
    (m2, t2), _ = d.gpu_order_postings(n, lists, min_half=4)
    assert m1.tobytes() == m2.tobytes() and t1.tobytes() == t2.tobytes()
    assert np.array_equal(m1, d.order_postings(n, lists, min_half=4)[0])


def test_a_better_order(built_lib):
    """not a check of the device against the twin but of the point of it all: the device's map lowers the integer cost of the gaps"""
    n, lists = oc.topical(1000)
    m, _, _ = check("to the last level", n, lists, {"min_half": 1})
    after = d.remap_postings(n, [(x, np.ones(len(x), np.uint32)) for x in lists], m)
    assert d.postings_cost([x for x, _ in after]) < d.postings_cost(lists)


# ---------------------------------------------------------------- images
def image_collection():
    def make():
        n, lists = oc.topical(2000)
        lists = [(x, 1 + (x % 3).astype(np.uint32)) for x in lists if len(x)]
        return Collection.from_lists(n, lists, np.full(n, 12, dtype=np.uint32))
    return oc._once("image collection", make)


@pytest.mark.parametrize("kind", ["block_optpfor", "opt", "block_qmx"])
def test_index_order_and_remap(built_lib, kind):
    coll = image_collection()
    docs = [x for x, _ in coll.lists]
    want = oc.twin("image collection", coll.num_docs, docs, {})
    idx = d.Index(kind, coll.index_image(kind))
    try:
        (m, tr), info = idx.order()
        assert np.array_equal(m, want[0]) and np.array_equal(tr, want[1])
        assert info["extract_ms"] > 0 and abs(info["device_ms"] - sum(info[p] for p in PARTS)) < 1e-6
        (m2, _), _ = idx.order(iterations=2, max_levels=3)
        assert np.array_equal(m2, d.order_postings(coll.num_docs, docs, iterations=2, max_levels=3)[0])
        to_kind = "block_optpfor" if kind == "block_qmx" else kind
        img, _ = idx.remap(m, to_kind)
    finally:
        idx.close()
    r = d.gpu_verify_collection(to_kind, img, coll.num_docs, d.remap_postings(coll.num_docs, coll.lists, m))
    assert r["ok"], r


def test_order_documents_then_convert_index(built_lib, tmp_path):
    coll = image_collection()
    base = str(tmp_path / "topical")
    open(base + ".opt", "wb").write(coll.index_image("opt"))
    p = subprocess.run([ORDER, "opt", base + ".opt", base + ".map", "--check"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert p.returncode == 0, p.stderr
    docs = [x for x, _ in coll.lists]
    m = oc.twin("image collection", coll.num_docs, docs, {})[0]
    after = d.postings_cost([x for x, _ in d.remap_postings(coll.num_docs, coll.lists, m)])
    assert p.stdout == "OK documents=%d cost_before=%d cost_after=%d\n" % (coll.num_docs, d.postings_cost(docs), after)
    words = np.fromfile(base + ".map", dtype=np.uint32)
    assert words[0] == coll.num_docs and np.array_equal(words[1:], m)
    p = subprocess.run([CONVERT, "opt", base + ".opt", "block_optpfor", base + ".out", "--remap", base + ".map", "--check"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith("OK lists=%d " % len(coll.lists))
    # the parameters reach the library
    p = subprocess.run([ORDER, "opt", base + ".opt", base + ".map2", "--iterations", "2", "--levels", "3", "--min-half", "8"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and p.stdout == "", p.stderr
    assert np.array_equal(np.fromfile(base + ".map2", dtype=np.uint32)[1:], d.order_postings(coll.num_docs, docs, 2, 8, 3)[0])
