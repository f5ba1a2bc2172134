"""Indexing documents on the GPU (-m gpu): ds2i_hip_invert_postings and ds2i_hip_transpose_postings against the host twins and the numpy
references, ds2i_hip_invert_documents against the HOST builder's index and wand images, the loop through gpu_merge_indexes, the forward
index of every kind of image, and the index_documents tool. Everything is integers and every answer is unique: arrays are compared with
np.array_equal, images and files with == on bytes."""
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import ds2i_amd as d
import invert_cases as ic
import remap_cases as rc
import split_cases as sc
import verify_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "ds2i_amd", "tools")
INDEX = os.path.join(TOOLS, "index_documents")
MERGE = os.path.join(TOOLS, "merge_indexes")
INVERT_PARTS = ("check_ms", "doc_sort_ms", "count_ms", "scatter_ms", "transpose_ms", "column_sort_ms")


def check_postings(docs, nterms, reference=True):
    """gpu_invert_postings == the twin (and the numpy reference), element for element; returns (arrays, info)"""
    got, info = d.gpu_invert_postings(docs, nterms)
    ic.assert_csr_equal(got, d.invert_documents(docs, nterms), "the twin")
    if reference:
        ic.assert_csr_equal(got, ic.numpy_invert(docs[0], docs[1], nterms), "numpy")
    assert info["extract_ms"] == 0 and info["encode_ms"] == 0
    assert abs(info["device_ms"] - sum(info[p] for p in INVERT_PARTS)) < 1e-6
    return got, info


def postings_of(arrays, term):
    offs, docs, freqs = arrays[:3]
    return docs[int(offs[term]):int(offs[term + 1])], freqs[int(offs[term]):int(offs[term + 1])]


def assert_same_bytes(got, want, what):
    if got != want:
        k = min(len(got), len(want))
        bad = np.flatnonzero(np.frombuffer(got[:k], dtype=np.uint8) != np.frombuffer(want[:k], dtype=np.uint8))
        print("%s: lengths, first differing byte, differing bytes:" % what, len(got), len(want), int(bad[0]) if len(bad) else None, len(bad))
    assert got == want, what


# ---------------------------------------------------------------- the kernels, against the twin and numpy
def test_document_length_edges(built_lib):
    """documents of 0, 1, 2, 63, 64, 65, L - 1, L, L + 1, T - 1, T, T + 1 and 2 T + 1 tokens drawn with replacement from 300 terms: every
    class of the segmented sort, over keys that repeat"""
    W, L, T = d.remap_class_bounds()
    lengths, docs = ic.length_edge_documents((W, L, T))
    assert set(lengths) == {0, 1, 2, 63, 64, 65, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T + 1}
    assert lengths[0] == 0 and lengths[-1] == 0 and 0 in lengths[1:-1] and np.array_equal(np.diff(docs[0].astype(np.int64)), lengths)
    got, info = check_postings(docs, 300)
    assert np.array_equal(got[3], lengths) and int((got[2] > 1).sum()) > 1000  # (freqs > 1 are common)
    assert info["doc_sort_ms"] > 0 and info["count_ms"] > 0 and info["scatter_ms"] > 0 and info["transpose_ms"] > 0


@pytest.mark.parametrize("whole_windows", [False, True])
def test_run_edges(built_lib, whole_windows):
    """documents that are n copies of one term, n = 1, 63, 64, 65, V - 1, V, V + 1, 2 V + 1, 3 V - 1, on window boundaries and in
    mid-window: a run spans lanes, steps, windows and whole windows; neighbours that share a term across lane 63 | 0 and across a window
    edge do not fuse"""
    V = d.invert_window()
    runs, docs, nterms = ic.run_edge_documents(V, whole_windows)
    assert {n for _, _, n in runs} >= {1, 63, 64, 65, V - 1, V, V + 1, 2 * V + 1, 3 * V - 1}
    starts = docs[0][:-1].astype(np.int64)
    assert (int(docs[0][-1]) % V == 0) == whole_windows and np.sum(starts % V == 0) >= 3 and np.sum(starts % V != 0) >= 8
    got, _ = check_postings(docs, nterms)
    for doc, term, n in runs:
        dd, ff = postings_of(got, term)
        at = int(np.searchsorted(dd, doc))
        assert dd[at] == doc and ff[at] == n, (doc, term, n)
    shared = [(doc, n) for doc, term, n in runs if term == ic.RUN_TERM]
    dd, ff = postings_of(got, ic.RUN_TERM)
    assert dd.tolist() == [doc for doc, _ in shared] and ff.tolist() == [n for _, n in shared] == [64, 3, 7, V + 2]
    lane63, edge = int(docs[0][shared[1][0]]), int(docs[0][shared[3][0]])  # where the second document of each pair starts
    assert lane63 % 64 == 0 and lane63 % V != 0 and edge % V == 0 and shared[1][0] == shared[0][0] + 1 and shared[3][0] == shared[2][0] + 1


def test_a_term_in_every_document(built_lib, capsys):
    """20 000 documents that all hold term 0: every add of the transposition's scatter to that column's cursor lands on one word. Terms
    that occur once, and terms that never occur: the postings form keeps their empty lists, the image form's term_map skips them."""
    o, t, nterms = ic.every_document_case()
    num_docs = len(o) - 1
    sizes = np.diff(o.astype(np.int64))
    assert num_docs == 20000 and sizes.min() >= 3 and sizes.max() <= 41
    t0 = time.perf_counter()
    want = d.invert_documents((o, t), nterms)
    twin_s = time.perf_counter() - t0
    got, info = check_postings((o, t), nterms)
    dd, _ = postings_of(got, 0)
    assert np.array_equal(dd, np.arange(num_docs))
    lens = np.diff(got[0].astype(np.int64))
    assert np.all(lens[200:400] == 1) and np.all(lens[400:] == 0) and np.all(got[2][got[0][200]:got[0][400]] == 1)
    (image, wand, term_map, doc_sizes), iinfo = d.gpu_invert_documents("block_optpfor", (o, t), nterms)
    assert np.array_equal(term_map, np.arange(400)) and np.array_equal(doc_sizes, sizes)
    lists = [postings_of(want, term) for term in range(400)]
    assert_same_bytes(image, d.build_index("block_optpfor", num_docs, lists), "image")
    assert_same_bytes(wand, d.build_wand(doc_sizes, lists), "wand")
    with capsys.disabled():
        print("\ninversion of %d tokens in %d documents, term 0 in every document: %s; transpose count + scatter %.3f ms, column sort %.3f ms; "
              "host twin %.1f ms" % (len(t), num_docs, ", ".join("%s %.3f" % (p[:-3], info[p]) for p in INVERT_PARTS), info["transpose_ms"],
                                     info["column_sort_ms"], 1e3 * twin_s))


def test_the_grid_wraps(built_lib, capsys):
    """a launch has at most split_grid_waves(CUs) wavefronts, a window of V tokens each at a time: twice that many windows, five more
    and 17 tokens make every wavefront of the count and scatter launches take a second window and some a third"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    V, waves = d.invert_window(), d.split_grid_waves(cus)
    n = (2 * waves + 5) * V + 17
    rng = np.random.default_rng(0x6A1D)
    lengths = rng.integers(0, 120, 2 * n // 119 + 100)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), n))]
    lengths = np.concatenate([lengths, [n - int(lengths.sum())]])  # (the last document takes what is left)
    o = np.zeros(len(lengths) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(lengths)
    t = rng.integers(0, 5000, n).astype(np.uint32)
    assert int(o[-1]) == n and n // V >= 2 * waves
    t0 = time.perf_counter()
    want = d.invert_documents((o, t), 5000)
    twin_s = time.perf_counter() - t0
    got, info = d.gpu_invert_postings((o, t), 5000)
    ic.assert_csr_equal(got, want)
    assert int(got[2].sum()) == n
    with capsys.disabled():
        print("\ninversion of %d tokens in %d documents on %d CUs: %s, sum %.3f ms; host twin %.1f ms"
              % (n, len(lengths), cus, ", ".join("%s %.3f" % (p[:-3], info[p]) for p in INVERT_PARTS), info["device_ms"], 1e3 * twin_s))


def test_ids_past_2_24(built_lib):
    o, t, nterms = ic.past_2_24_documents()
    assert len(o) - 1 == (1 << 24) + 5 and nterms == 50
    got, _ = check_postings((o, t), nterms)
    full = np.flatnonzero(np.diff(o.astype(np.int64)))
    assert 30 <= len(full) <= 80 and np.sum(full < 1 << 24) >= 10 and np.sum(full >= 1 << 24) >= 5
    assert int(got[1].max()) == (1 << 24) + 4 and set(got[1].tolist()) == set(full.tolist())
    o, t, nterms = ic.past_2_24_terms()
    assert nterms == (1 << 24) + 5 and np.sum(t < 1 << 24) > 100 and np.sum(t >= 1 << 24) > 100
    got, _ = check_postings((o, t), nterms)
    assert int(got[0][1 << 24]) < int(got[0][-1]) and int((got[2] > 1).sum()) > 50


def test_transposition(built_lib):
    coll = rc.block_edge_collection()
    V, n = len(coll.lists), coll.num_docs
    lists = ic.csr_of(coll)
    fwd, info = d.gpu_transpose_postings(V, n, *lists)
    ic.assert_csr_equal(fwd, ic.numpy_transpose(V, n, *lists))
    ic.assert_csr_equal(fwd, d.transpose_postings(V, n, *lists))
    assert info["transpose_ms"] > 0 and info["column_sort_ms"] > 0 and info["check_ms"] == 0 and info["encode_ms"] == 0
    assert abs(info["device_ms"] - info["transpose_ms"] - info["column_sort_ms"]) < 1e-6
    back, _ = d.gpu_transpose_postings(n, V, *fwd)
    ic.assert_csr_equal(back, lists)  # twice gives the input back
    offs, cols, vals = np.array([0, 0, 2, 2, 3, 3], dtype=np.uint64), np.array([1, 4, 4], dtype=np.uint32), np.array([7, 8, 9], dtype=np.uint32)
    got, _ = d.gpu_transpose_postings(5, 6, offs, cols, vals)  # empty rows, and columns 0, 2, 3 and 5 empty
    assert got[0].tolist() == [0, 0, 1, 1, 1, 3, 3] and got[1].tolist() == [1, 1, 3] and got[2].tolist() == [7, 8, 9]
    none, info = d.gpu_transpose_postings(3, 2, [0, 0, 0, 0], [], [])
    assert none[0].tolist() == [0, 0, 0] and len(none[1]) == 0 and info["device_ms"] == 0


# ---------------------------------------------------------------- images: == the host builder's, on bytes
@pytest.mark.parametrize("to_kind", cases.GPU_BUILT_KINDS)
def test_documents_become_every_gpu_built_kind(built_lib, to_kind):
    coll = rc.block_edge_collection()
    with_sizes = ic.with_token_sizes(coll)  # coll': the sizes are the token counts
    (image, wand, term_map, doc_sizes), info = d.gpu_invert_documents(to_kind, ic.forward_of(coll), len(coll.lists))
    assert_same_bytes(image, cases.image(with_sizes, to_kind), "image")
    assert_same_bytes(wand, with_sizes.wand_image(), "wand")
    twin = d.invert_documents(ic.forward_of(coll), len(coll.lists))
    assert term_map.dtype == np.uint32 and np.array_equal(term_map, np.flatnonzero(np.diff(twin[0].astype(np.int64))))
    assert np.array_equal(doc_sizes, twin[3]) and np.array_equal(doc_sizes, with_sizes.sizes)
    used = INVERT_PARTS + ("encode_ms",)
    for part in used:
        assert info[part] > 0, part
    assert info["extract_ms"] == 0 and abs(info["device_ms"] - sum(info[p] for p in used)) < 1e-6
    (again, none, _, _), _ = d.gpu_invert_documents(to_kind, ic.forward_of(coll), len(coll.lists), wand=False)
    assert none is None and again == image


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_the_loop_closes(built_lib, kind):
    """the documents cut into three batches, each indexed on its own; merging the three images with their term maps and the default doc
    maps is the host builder's image of the whole collection"""
    coll = rc.block_edge_collection()
    o, t = ic.forward_of(coll)
    edges = [0] + list(sc.EDGE_CUTS) + [coll.num_docs]
    sources = []
    for lo, hi in zip(edges, edges[1:]):
        batch = (o[lo:hi + 1] - o[lo], t[int(o[lo]):int(o[hi])])
        (image, _, term_map, doc_sizes), _ = d.gpu_invert_documents(kind, batch, len(coll.lists), wand=False)
        assert len(doc_sizes) == hi - lo and 0 < len(term_map) <= len(coll.lists)
        sources.append((kind, image, None, term_map))
    assert any(len(s[3]) < len(coll.lists) for s in sources)  # (a batch lacks a term: its map is no identity)
    merged, _ = d.gpu_merge_indexes(sources, kind, num_terms=len(coll.lists))
    assert_same_bytes(merged, cases.image(coll, kind), "merged")


@pytest.mark.parametrize("kind", cases.KINDS)
def test_forward_and_back(built_lib, kind):
    coll = rc.block_edge_collection()
    V, n = len(coll.lists), coll.num_docs
    image = cases.image(coll, kind)
    (num_docs, nterms, offs, terms, freqs), info = d.gpu_forward_index(kind, image)
    assert (num_docs, nterms) == (n, V)
    ic.assert_csr_equal((offs, terms, freqs), ic.numpy_transpose(V, n, *ic.csr_of(coll)))
    assert info["extract_ms"] > 0 and info["transpose_ms"] > 0 and info["column_sort_ms"] > 0 and info["check_ms"] == 0 and info["encode_ms"] == 0
    assert abs(info["device_ms"] - info["extract_ms"] - info["transpose_ms"] - info["column_sort_ms"]) < 1e-6
    to_kind = kind if kind in cases.GPU_BUILT_KINDS else "block_optpfor"
    (back, _, term_map, _), _ = d.gpu_invert_documents(to_kind, ic.expand(offs, terms, freqs), V, wand=False)
    assert np.array_equal(term_map, np.arange(V))
    assert_same_bytes(back, cases.image(coll, to_kind), "the image back")
    idx = d.Index(kind, image)
    try:
        (n2, v2, o2, t2, f2), _ = idx.forward()
    finally:
        idx.close()
    assert (n2, v2) == (n, V)
    ic.assert_csr_equal((o2, t2, f2), (offs, terms, freqs))


# ---------------------------------------------------------------- errors on the device
def test_no_such_device(built_lib):
    o, t = ic.small_edges()
    image = cases.image(rc.block_edge_collection(), "block_optpfor")
    for make in (lambda: d.gpu_invert_postings((o, t), 12, device=99), lambda: d.gpu_invert_documents("opt", (o, t), 12, device=99),
                 lambda: d.gpu_transpose_postings(len(o) - 1, 12, o, t, t, device=99), lambda: d.gpu_forward_index("block_optpfor", image, device=99)):
        with pytest.raises(d.Ds2iError) as e:
            make()
        assert e.value.code == -4


def test_a_token_or_a_column_out_of_range_is_a_format_error(built_lib):
    """the stage kernel (the transposition's count kernel) flags it and indexes nothing by it; the call refuses and writes no output"""
    C = d.api.C
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L = built_lib
    o, t = ic.small_edges()
    bad = t.copy()
    bad[6] = 12  # == nterms
    for make in (lambda: d.gpu_invert_postings((o, bad), 12), lambda: d.gpu_invert_documents("block_optpfor", (o, bad), 12)):
        with pytest.raises(d.Ds2iError) as e:
            make()
        assert e.value.code == -2 and "outside the 12 terms" in str(e.value)
    hs, ms = [C.c_void_p() for _ in range(4)], C.c_double(-1.0)
    code = L.ds2i_hip_invert_postings(0, len(o) - 1, ptr(o), ptr(bad), 12, *[C.byref(h) for h in hs], C.byref(ms))
    assert code == -2 and not any(h.value for h in hs) and ms.value == -1.0 and "outside the 12 terms" in L.ds2i_hip_last_error().decode()
    code = L.ds2i_hip_invert_documents(0, 0, len(o) - 1, ptr(o), ptr(bad), 12, *[C.byref(h) for h in hs], C.byref(ms))
    assert code == -2 and not any(h.value for h in hs) and ms.value == -1.0
    # the transposition: a column == ncols, and a row whose columns do not strictly increase
    offs, vals = np.array([0, 2, 2, 5], dtype=np.uint64), np.ones(5, dtype=np.uint32)
    for cols in ([1, 3, 0, 2, 4], [1, 3, 0, 2, 2]):
        cols = np.array(cols, dtype=np.uint32)
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_transpose_postings(3, 4, offs, cols, vals)
        assert e.value.code == -2 and "outside the 4 columns" in str(e.value)
        hs3 = [C.c_void_p() for _ in range(3)]
        code = L.ds2i_hip_transpose_postings(0, 3, 4, ptr(offs), ptr(cols), ptr(vals), *[C.byref(h) for h in hs3], C.byref(ms))
        assert code == -2 and not any(h.value for h in hs3) and ms.value == -1.0
    good, _ = d.gpu_transpose_postings(3, 4, offs, np.array([1, 3, 0, 2, 3], dtype=np.uint32), vals)
    assert good[0].tolist() == [0, 1, 2, 3, 5]


# ---------------------------------------------------------------- the tool
def test_tool_indexes_checks_and_feeds_the_merge(built_lib, tmp_path):
    if not (os.path.exists(INDEX) and os.path.exists(MERGE)):
        subprocess.check_call(["make", "-C", TOOLS, "-s"])
    coll = rc.block_edge_collection()
    V = len(coll.lists)
    o, t = ic.forward_of(coll)
    cut = sc.EDGE_CUTS[1]
    batches = [(o[:cut + 1], t[:int(o[cut])]), (o[cut:] - o[cut], t[int(o[cut]):])]

    def run(*args):
        return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)

    for k, batch in enumerate(batches):
        fwd, out, wand_path = str(tmp_path / ("fwd%d" % k)), str(tmp_path / ("index%d" % k)), str(tmp_path / ("wand%d" % k))
        ic.write_forward(fwd, *batch)
        p = run(INDEX, "block_optpfor", fwd, str(V), out, wand_path, "--check")
        assert p.returncode == 0, p.stderr
        twin = d.invert_documents(batch, V)
        assert p.stdout == "OK lists=%d postings=%d\n" % (int(np.sum(np.diff(twin[0].astype(np.int64)) > 0)), len(twin[1])), p.stdout
        (image, wand, term_map, doc_sizes), _ = d.gpu_invert_documents("block_optpfor", batch, V)
        assert open(out, "rb").read() == image and open(wand_path, "rb").read() == wand
        for path, m in ((out + ".terms", term_map), (out + ".sizes", doc_sizes)):
            words = np.fromfile(path, dtype=np.uint32)
            assert words[0] == len(m) and np.array_equal(words[1:], m), path
    p = run(INDEX, "opt", str(tmp_path / "fwd0"), str(V), str(tmp_path / "plain"), "--gpu-only")
    assert p.returncode == 0 and p.stdout == "" and not os.path.exists(str(tmp_path / "plain.wand")), p.stderr
    assert open(str(tmp_path / "plain"), "rb").read() == d.gpu_invert_documents("opt", batches[0], V, wand=False)[0][0]
    merged = str(tmp_path / "merged")
    p = run(MERGE, "block_optpfor", merged, "block_optpfor", str(tmp_path / "index0"), "--terms", str(tmp_path / "index0.terms"),
            "block_optpfor", str(tmp_path / "index1"), "--terms", str(tmp_path / "index1.terms"))
    assert p.returncode == 0, p.stderr
    assert open(merged, "rb").read() == cases.image(coll, "block_optpfor")
