"""Ordering documents on a CPU-only box: the host twin of recursive graph bisection against the numpy restatement (map and trace), the
maps it returns as permutations, the clamp of a gain, the integer cost of the gaps, every answer of the entry points that needs no
device in the order the headers state, the twin under the sanitizers as a program of its own, and the point of it all on a topical
collection in random order: a lower cost and a smaller opt image."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
import order_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "order_documents")
NO_DEVICE = 99
HIP_ARGS = {"ds2i_hip_order_postings": 9, "ds2i_hip_order_index": 8}
BUILD_ARGS = {"ds2i_order_postings": 8, "ds2i_order_log_table": 2, "ds2i_postings_cost": 4}


def test_symbols_are_exported_and_declared(built_lib):
    for header, table in (("ds2i_hip.h", HIP_ARGS), ("ds2i_build.h", BUILD_ARGS)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name, nargs in table.items():
            assert hasattr(built_lib, name), name
            decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
            assert decl, name
            assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
            assert len(getattr(built_lib, name).argtypes) == nargs
    src = open(os.path.join(ROOT, "include", "ds2i_hip.h")).read()
    assert re.search(r"\bvoid\s+ds2i_hip_order_ms\s*\(", src) and hasattr(built_lib, "ds2i_hip_order_ms")
    assert re.search(r"\bint32_t\s+ds2i_order_clamp_gain\s*\(", open(os.path.join(ROOT, "include", "ds2i_build.h")).read())
    assert d.order_postings and d.gpu_order_postings and d.gpu_order_index and d.Index.order and d.postings_cost and d.order_log_table
    assert C.sizeof(d.OrderParams) == 12


# ---------------------------------------------------------------- the twin
def test_log_table_is_the_stated_fixed_point(built_lib):
    t = d.order_log_table(5000)
    assert t.dtype == np.uint32 and t[0] == 0 and t[1] == 0 and t[2] == 256 and t[4] == 512 and t[1024] == 2560 and t[3] == 406
    x = np.arange(1, 5000)
    # (within half a unit and a libm's last bits of numpy's logarithm, and monotone; the restatement uses the table, not numpy's log2)
    assert np.all(np.abs(t[1:].astype(np.float64) - np.log2(x.astype(np.float64)) * 256) <= 0.5 + 1e-6) and np.all(np.diff(t.astype(np.int64)) >= 0)
    assert np.array_equal(t[1 << np.arange(13)], 256 * np.arange(13))
    assert len(d.order_log_table(0)) == 0


@pytest.mark.parametrize("case", list(oc.small_cases()), ids=lambda c: c[0])
def test_twin_equals_the_numpy_restatement(built_lib, case):
    name, n, lists, prm = case
    m, tr = oc.twin(name, n, lists, prm)
    wm, wt = oc.numpy_order(n, lists, **prm)
    assert m.dtype == np.uint32 and tr.dtype == np.uint64
    assert np.array_equal(tr, wt) and np.array_equal(m, wm)
    d.check_doc_map(m, n)
    assert len(tr) >= oc.level_count(n, prm.get("min_half", 0), prm.get("max_levels", 0))
    tm, tt = d.order_postings(n, lists, threads=3, **prm)
    assert np.array_equal(tm, m) and np.array_equal(tt, tr)


def test_twin_equals_the_numpy_restatement_where_ties_meet_long_halves(built_lib):
    n, lists = oc.class3(d.remap_class_bounds())
    m, tr = oc.twin("class3", n, lists, {})
    wm, wt = oc.numpy_order(n, lists)
    assert np.array_equal(tr, wt) and np.array_equal(m, wm)
    d.check_doc_map(m, n)


def test_the_tie_cases_are_what_they_claim(built_lib):
    cases = {name: (n, lists, prm) for name, n, lists, prm in oc.small_cases()}
    assert oc.twin("identical", *cases["identical"])[1].tolist() == [0, 0]
    tr = oc.twin("identical, restless", *cases["identical, restless"])[1]
    assert tr[0] == 0 and set(tr[1:21].tolist()) == {100}
    n, lists, _ = cases["two kinds"]
    m, tr = oc.twin("two kinds", n, lists, {})
    assert tr[0] > 0 and tr[1] == 0 and set(np.sort(m[lists[0]]) // 128) in ({0}, {1})
    assert np.array_equal(oc.twin("no level", *cases["no level"])[0], np.arange(31)) and len(oc.twin("no level", *cases["no level"])[1]) == 0


def test_clamp_at_both_int32_ends(built_lib):
    f = built_lib.ds2i_order_clamp_gain
    hi, lo = (1 << 31) - 1, -(1 << 31)
    for g, want in ((0, 0), (7, 7), (-7, -7), (hi, hi), (hi + 1, hi), (lo, lo), (lo - 1, lo), ((1 << 62), hi), (-(1 << 62), lo), (hi - 1, hi - 1), (lo + 1, lo + 1)):
        assert f(g) == want, g


def test_postings_cost(built_lib):
    t = d.order_log_table(70000)
    lists = [np.array([0, 1, 5, 69000], dtype=np.uint32), np.zeros(0, np.uint32), np.array([9], dtype=np.uint32)]
    assert d.postings_cost(lists) == int(t[1]) + int(t[1]) + int(t[4]) + int(t[68995]) + int(t[10])
    assert d.postings_cost([]) == 0
    assert d.postings_cost([np.array([0xFFFFFFFF], dtype=np.uint32)]) == 32 * 256  # the first gap is doc + 1 = 2^32
    with pytest.raises(d.Ds2iError) as e:
        d.postings_cost([np.array([3, 3], dtype=np.uint32)])
    assert e.value.code == -2 and "do not strictly increase" in str(e.value)


# ---------------------------------------------------------------- refusals, without a device
def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


U64 = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
U32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731


def call(L, name, num_docs, offs, docs, prm=(0, 0, 0), null=None, device=NO_DEVICE):
    """(code, message) of one of the two postings entry points with pointer `null` (0 offsets, 1 docs, 2 doc_map, 3 trace) null; no output
    is written on an error"""
    hm, ht, ms = C.c_void_p(), C.c_void_p(), C.c_double(-1.0)
    p = d.OrderParams(*prm)
    args = [num_docs, len(offs) - 1, None if null == 0 else ptr(offs), None if null == 1 else ptr(docs), C.byref(p)]
    outs = [None if null == 2 else C.byref(hm), None if null == 3 else C.byref(ht)]
    if name.startswith("ds2i_hip_"):
        rc = getattr(L, name)(device, *args, *outs, C.byref(ms))
    else:
        rc = getattr(L, name)(*args, 0, *outs)
    assert hm.value is None and ht.value is None and ms.value == -1.0
    return rc, L.ds2i_hip_last_error().decode()


@pytest.mark.parametrize("name", ["ds2i_order_postings", "ds2i_hip_order_postings"])
def test_refusals_in_the_documented_order(built_lib, name):
    L = built_lib
    good_o, good_d = U64(0, 2, 3), U32(1, 4, 0)
    for null in range(4):
        rc, msg = call(L, name, 5, U64(1, 0), U32(9), prm=(1 << 20, 0, 99), null=null)  # (every later fault is present too)
        assert rc == -1 and msg == name + ": null argument"
    rc, msg = call(L, name, 5, U64(1, 0), U32(9), prm=(1 << 20, 0, 99))
    assert rc == -1 and msg == name + ": list_offsets must start at 0"
    rc, msg = call(L, name, 5, U64(0, 2, 1), U32(9, 9, 9), prm=(1 << 20, 0, 99))
    assert rc == -1 and msg == name + ": list_offsets decrease"
    rc, msg = call(L, name, 4, good_o, good_d, prm=(1 << 20, 0, 99))
    assert rc == -2 and msg == name + ": list 0 holds doc-id 4, outside the 4 documents"
    rc, msg = call(L, name, 5, U64(0, 1, 4), U32(0, 1, 3, 3), prm=(1 << 20, 0, 99))
    assert rc == -2 and msg == name + ": the doc-ids of list 1 do not strictly increase at position 2"
    rc, msg = call(L, name, (1 << 32) - 2, good_o, good_d, prm=(1 << 20, 0, 99))
    assert rc == -1 and msg == name + ": 2^32 - 2 documents or more"
    rc, msg = call(L, name, 5, good_o, good_d, prm=((1 << 16) + 1, 0, 99))
    assert rc == -1 and msg == name + ": iterations above 65536"
    rc, msg = call(L, name, 5, good_o, good_d, prm=(1 << 16, 1 << 31, 33))
    assert rc == -1 and msg == name + ": max_levels above 32"
    if name.startswith("ds2i_hip_"):  # every argument is good: only now is a device looked for
        rc, msg = call(L, name, 5, good_o, good_d, prm=(1 << 16, 1 << 31, 32))
        assert rc == -4 and msg == name + ": no such HIP device"
        rc, msg = call(L, name, 5, good_o, good_d, device=-1)
        assert rc == -4
    else:
        hm, ht = C.c_void_p(), C.c_void_p()
        assert L.ds2i_order_postings(5, 2, ptr(good_o), ptr(good_d), None, 0, C.byref(hm), C.byref(ht)) == 0  # (null params: all defaults)
        assert np.array_equal(np.frombuffer(d.api._take_blob(hm), dtype=np.uint32), np.arange(5)) and d.api._take_blob(ht) == b""


def test_order_index_refusals_without_a_device(built_lib):
    L, name = built_lib, "ds2i_hip_order_index"
    n, lists = oc.topical(77)
    img = d.build_index("block_optpfor", n, [(x, np.ones(len(x), np.uint32)) for x in lists if len(x)])

    def run(kind, image, prm=(0, 0, 0), null=None, size=None):
        hm, ht, ms, p = C.c_void_p(), C.c_void_p(), C.c_double(-1.0), d.OrderParams(*prm)
        rc = L.ds2i_hip_order_index(NO_DEVICE, kind, None if null == 0 else image, len(image) if size is None else size, C.byref(p),
                                    None if null == 1 else C.byref(hm), None if null == 2 else C.byref(ht), C.byref(ms))
        assert hm.value is None and ht.value is None and ms.value == -1.0
        return rc, L.ds2i_hip_last_error().decode()

    for null in range(3):
        assert run(42, b"garbage!" * 8, prm=(1 << 20, 0, 99), null=null) == (-1, name + ": null argument")
    for kind in (-1, 9):
        assert run(kind, b"garbage!" * 8, prm=(1 << 20, 0, 99)) == (-1, name + ": unknown index kind")
    for kind in ("block_optpfor", "opt", "block_qmx"):
        assert run(d.CODECS[kind], b"garbage!" * 8, prm=(1 << 20, 0, 99))[0] == -2
    assert run(0, img, size=len(img) // 2, prm=(1 << 20, 0, 99))[0] == -2
    assert run(0, img, prm=((1 << 16) + 1, 0, 0)) == (-1, name + ": iterations above 65536")
    assert run(0, img, prm=(0, 0, 33)) == (-1, name + ": max_levels above 32")
    assert run(0, img) == (-4, name + ": no such HIP device")
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_order_index("block_optpfor", img, device=NO_DEVICE)
    assert e.value.code == -4


def test_cost_and_table_refusals(built_lib):
    L = built_lib
    cost = C.c_uint64(77)
    for args in ((None, ptr(U32(1)), C.byref(cost)), (ptr(U64(0, 1)), None, C.byref(cost)), (ptr(U64(0, 1)), ptr(U32(1)), None)):
        assert L.ds2i_postings_cost(1, *args) == -1 and L.ds2i_hip_last_error().decode() == "ds2i_postings_cost: null argument"
    assert L.ds2i_postings_cost(1, ptr(U64(1, 1)), ptr(U32(1)), C.byref(cost)) == -1
    assert L.ds2i_postings_cost(2, ptr(U64(0, 2, 1)), ptr(U32(1, 2)), C.byref(cost)) == -1
    assert cost.value == 77
    assert L.ds2i_order_log_table(4, None) == -1


# ---------------------------------------------------------------- the host side under the sanitizers, as a program of its own
def test_twin_check_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """host_order.hpp and tests/order_twin_check.cpp (its own main) compiled with -fsanitize=address,undefined and run: nothing that is
    loaded into this interpreter runs under a sanitizer"""
    exe = str(tmp_path / "order_twin_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread",  # (the runtimes inside the program: it asks nothing of its loader)
                           os.path.join(ROOT, "tests", "order_twin_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and p.stdout == "OK\n" and p.stderr == "", (p.stdout, p.stderr)


# ---------------------------------------------------------------- the tool, without a device
def test_tool_usage_errors_without_a_device(built_lib, tmp_path):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])

    def run(*args):
        p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return p.returncode, p.stdout, p.stderr

    out = str(tmp_path / "map")
    for args in ((), ("opt", "in"), ("opt", "in", out, "extra"), ("opt", "in", out, "--iterations"), ("opt", "in", out, "--iterations", "x"),
                 ("opt", "in", out, "--levels", "-1"), ("opt", "in", out, "--nonsense")):
        rc, so, se = run(*args)
        assert rc == 2 and so == "" and se.startswith("usage: ") and "--min-half" in se, args
    rc, so, se = run("nonsense", "in", out)
    assert rc == 2 and "Unknown type nonsense" in se
    rc, so, se = run("opt", str(tmp_path / "missing"), out)
    assert rc == 2 and "cannot open" in se and not os.path.exists(out)


# ---------------------------------------------------------------- a better order
def topical_fixture():
    """8192 documents and 300 terms of the synthetic collection with 4 topics (boost 16), its documents shuffled by a seeded
    permutation: the order a crawl might arrive in. Chosen on the CPU so that the twin alone wins both comparisons below."""
    def make():
        p = d.SynthParams(seed=0x70C1CA1, num_docs=8192, num_terms=300, zipf_exp=0.75, top_df_frac=0.3, min_len=16, clustered_every=0,
                          topics=4, topic_boost=16)
        lists = [x for x in (d.synth_list(p, t) for t in range(p.num_terms)) if len(x[0])]
        shuffle = np.random.default_rng(5).permutation(p.num_docs).astype(np.uint32)
        return int(p.num_docs), d.remap_postings(p.num_docs, lists, shuffle)
    return oc._once("topical fixture", make)


def test_the_order_is_better_on_a_topical_collection(built_lib):
    n, lists = topical_fixture()
    docs = [x for x, _ in lists]
    m, tr = d.order_postings(n, docs)
    d.check_doc_map(m, n)
    after = d.remap_postings(n, lists, m)
    before_cost, after_cost = d.postings_cost(docs), d.postings_cost([x for x, _ in after])
    before_size, after_size = len(d.build_index("opt", n, lists)), len(d.build_index("opt", n, after))
    print("cost %d -> %d (ratio %.4f), opt image %d -> %d bytes, %d iterations" % (before_cost, after_cost, after_cost / before_cost, before_size,
                                                                                   after_size, len(tr)))
    assert after_cost < before_cost
    assert after_size < before_size
