"""Renumbering documents on the GPU (-m gpu): ds2i_hip_remap_postings against the host twin, ds2i_hip_remap_index against the HOST
builder's image of the numpy-remapped collection, and the convert_index tool. Everything is integers and the doc-ids of a list are
distinct, so the answer is unique: lists are compared with np.array_equal, images and files with == on bytes. Only the scores of the
wand query carry the project's 1e-5."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ds2i_amd as d
import remap_cases as rc
import verify_cases as cases
from helpers import queries_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "ds2i_amd", "tools")
CONVERT, CREATE = os.path.join(TOOLS, "convert_index"), os.path.join(TOOLS, "create_freq_index")


@pytest.fixture(scope="module")
def bounds(built_lib):
    return d.remap_class_bounds()


def check_postings(num_docs, lists, m):
    got, info = d.gpu_remap_postings(num_docs, lists, m)
    assert info["device_ms"] > 0 and info["map_ms"] > 0
    rc.assert_lists_equal(got, d.remap_postings(num_docs, lists, m))
    return info


# ---------------------------------------------------------------- the sort itself
@pytest.mark.parametrize("name", rc.MAPS)
def test_class_edges_equal_the_host_twin(bounds, name):
    """lengths at W, L and T as compiled; 18 key bits: three radix passes, the last over two bits, ending in the second buffer pair"""
    n = rc.class_edge_num_docs(bounds)
    info = check_postings(n, rc.class_edge_lists(bounds), rc.doc_map(name, n))
    assert all(ms > 0 for ms in info["sort_ms"])  # every class had lists


def test_preimage_lists_share_their_high_digits(bounds):
    """the new doc-ids of each list are a contiguous range: every posting of a late radix pass lands in one or two buckets"""
    m = rc.doc_map("random", rc.class_edge_num_docs(bounds))
    check_postings(len(m), rc.preimage_lists(bounds, m), m)


def test_short_lists_only_need_no_second_buffer(bounds):
    W, L, _ = bounds
    lists = [ll for ll in rc.class_edge_lists(bounds) if len(ll[0]) <= L]
    n = rc.class_edge_num_docs(bounds)
    info = check_postings(n, lists, rc.doc_map("random", n))
    assert info["sort_ms"][2] == 0.0


def test_the_grid_wraps():
    """16 x CUs + 300 lists of 1, 1, 1, 2, 129 postings: more class 1 lists than waves and more class 2 lists than workgroups in their
    grids, and neighbouring lists a wave long: a store past a list's end lands in its neighbour and shows"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    coll = cases.many_lists_collection(cus)
    ones = sum(len(dd) <= 64 for dd, _ in coll.lists)
    assert ones > 8 * cus and len(coll.lists) - ones > 2 * cus  # (capi_remap.cpp: 2 workgroups a compute unit for either class)
    check_postings(coll.num_docs, coll.lists, rc.doc_map("random", coll.num_docs))


def test_doc_ids_past_2_24(bounds):
    """25 key bits: four passes, the top digit one bit wide; no key loses its high bits on the way"""
    m = rc.reverse_map_past_2_24()
    lists = rc.past_2_24_lists(bounds)
    got, _ = d.gpu_remap_postings(len(m), lists, m)
    rc.assert_lists_equal(got, d.remap_postings(len(m), lists, m))
    for (docs, freqs), (old, oldf) in zip(got, lists):  # the reverse map in closed form
        assert np.array_equal(docs, (len(m) - 1 - old.astype(np.int64))[::-1]) and np.array_equal(freqs, oldf[::-1])


def test_a_doc_id_outside_the_map_is_a_format_error(bounds):
    """the map kernel flags it and reads nothing past the map; the call refuses the result"""
    n = 1000
    lists = [(np.array([1, 5, 999], dtype=np.uint32), np.ones(3, dtype=np.uint32)),
             (np.array([7, 1000], dtype=np.uint32), np.ones(2, dtype=np.uint32))]
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_remap_postings(n, lists, rc.doc_map("reverse", n))
    assert e.value.code == -2 and "outside the map" in str(e.value)


# ---------------------------------------------------------------- images: == the host builder's, on bytes
def check_image(coll, from_kind, to_kind, name="random"):
    m = rc.doc_map(name, coll.num_docs)
    img, info = d.gpu_remap_index(from_kind, cases.image(coll, from_kind), m, to_kind)
    assert info["device_ms"] > 0 and info["extract_ms"] > 0 and info["encode_ms"] > 0
    want = cases.image(rc.remapped_collection(coll, name), to_kind)
    if img != want:
        k = min(len(img), len(want))
        bad = np.flatnonzero(np.frombuffer(img[:k], dtype=np.uint8) != np.frombuffer(want[:k], dtype=np.uint8))
        print("lengths, first differing byte, differing bytes:", len(img), len(want), int(bad[0]) if len(bad) else None, len(bad))
    assert img == want


@pytest.mark.parametrize("from_kind", cases.KINDS)
def test_every_kind_remaps_to_block_optpfor(built_lib, from_kind):
    check_image(rc.block_edge_collection(), from_kind, "block_optpfor")


@pytest.mark.parametrize("to_kind", cases.GPU_BUILT_KINDS)
def test_block_optpfor_remaps_to_every_gpu_built_kind(built_lib, to_kind):
    check_image(rc.block_edge_collection(), "block_optpfor", to_kind)


@pytest.mark.parametrize("from_kind", cases.FREQ_KINDS)
def test_freq_kinds_remap_the_freq_edge_collection_to_opt(built_lib, from_kind):
    check_image(cases.freq_edge_collection(), from_kind, "opt")


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_round_trip_through_the_inverse_map(built_lib, kind):
    coll = rc.block_edge_collection()
    p = rc.doc_map("random", coll.num_docs)
    there, _ = d.gpu_remap_index(kind, cases.image(coll, kind), p)  # (to_kind=None: the same kind)
    assert there != cases.image(coll, kind)
    back, _ = d.gpu_remap_index(kind, there, rc.inverse(p), kind)
    assert back == cases.image(coll, kind)


def test_remap_errors(built_lib):
    coll = rc.block_edge_collection()
    img, m = cases.image(coll, "opt"), rc.doc_map("random", coll.num_docs)
    for to_kind in ("block_qmx", "block_mixed"):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_remap_index("opt", img, m, to_kind)
        assert e.value.code == -1 and all(name in str(e.value) for name in cases.GPU_BUILT_KINDS)
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_remap_index("opt", cases.GARBAGE, m, "block_optpfor")
    assert e.value.code == -2
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_remap_index("opt", img, m[:-1], "block_optpfor")
    assert e.value.code == -1


# ---------------------------------------------------------------- a remapped index answers queries
def test_a_remapped_index_answers_queries(built_lib):
    """Index.remap + remap_wand against the index it came from. The doc-ids of the top-k are not compared: ties are broken by doc-id,
    which the map changes; the score rows are, and the whole match lists of `and`."""
    coll = cases.small_collection()
    m = rc.doc_map("random", coll.num_docs)
    wand = coll.wand_image()
    queries = queries_for(coll, nq=48)
    built = d.Index("block_optpfor", cases.image(coll, "block_optpfor"), wand)
    try:
        img, _ = built.remap(m)
        remapped = d.Index("block_optpfor", img, d.remap_wand(wand, m))
        try:
            def matches(idx):
                b = d.Batch(idx, "and", queries, want_matches=True)
                try:
                    b.run()
                    count = b.fetch()[0]
                    return count, b.fetch_matches(count)
                finally:
                    b.close()
            count, got = matches(remapped)
            rcount, ref = matches(built)
            assert np.array_equal(count, rcount) and int(count.sum()) > 0
            for q, g, r in zip(queries, got, ref):
                assert np.array_equal(g, np.sort(m[r])), q
            _, topk, tlen, _ = remapped.query_batch("ranked_and", queries, k=10)
            _, rtopk, rtlen, _ = built.query_batch("ranked_and", queries, k=10)
            assert np.array_equal(tlen, rtlen) and int(tlen.sum()) > 0 and topk.tobytes() == rtopk.tobytes()
            _, topk, tlen, _ = remapped.query_batch("wand", queries, k=10)
            _, rtopk, rtlen, _ = built.query_batch("wand", queries, k=10)
            assert np.array_equal(tlen, rtlen) and int(tlen.sum()) > 0
            for i in range(len(queries)):
                np.testing.assert_allclose(topk[i, :tlen[i]], rtopk[i, :rtlen[i]], rtol=1e-5, err_msg=str(queries[i]))
        finally:
            remapped.close()
    finally:
        built.close()


# ---------------------------------------------------------------- the tool
def test_tool_remaps_checks_and_writes_the_python_paths_files(built_lib, tmp_path):
    if not (os.path.exists(CONVERT) and os.path.exists(CREATE)):
        subprocess.check_call(["make", "-C", TOOLS, "-s"])
    coll = rc.block_edge_collection()
    m = rc.doc_map("random", coll.num_docs)
    base = str(tmp_path / "edge")
    open(base + ".opt", "wb").write(cases.image(coll, "opt"))
    open(base + ".wand", "wb").write(coll.wand_image())
    rc.write_map(base + ".map", m)
    out = base + ".remapped"
    p = subprocess.run([CONVERT, "opt", base + ".opt", "block_optpfor", out, "--remap", base + ".map", "--wand", base + ".wand", out + ".wand",
                        "--check"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout == "OK lists=%d postings=%d\n" % (len(coll.lists), cases.postings(coll))
    assert open(out, "rb").read() == d.gpu_remap_index("opt", cases.image(coll, "opt"), m, "block_optpfor")[0]
    assert open(out + ".wand", "rb").read() == d.remap_wand(coll.wand_image(), m)
