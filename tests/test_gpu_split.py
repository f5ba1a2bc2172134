"""Splitting indexes on the GPU (-m gpu): ds2i_hip_split_postings against the host twin, ds2i_hip_split_index against the HOST builder's
image of every shard, merge(split(x)) == x on bytes, shards that answer queries, and the split_index tool. Everything is integers and
every answer is unique: lists are compared with np.array_equal, images and files with == on bytes."""
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import ds2i_amd as d
import merge_cases as mc
import remap_cases as rc
import split_cases as sc
import verify_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "ds2i_amd", "tools")
SPLIT = os.path.join(TOOLS, "split_index")
MERGE = os.path.join(TOOLS, "merge_indexes")


def check_postings(num_docs, lists, shard_of, nshards=None):
    """gpu_split_postings == the twin, element for element; returns (shards, info)"""
    shards, info = d.gpu_split_postings(num_docs, lists, shard_of, nshards)
    total = sum(len(dd) for dd, _ in lists)
    assert info["extract_ms"] == 0 and info["encode_ms"] == 0 and info["offsets_ms"] > 0 and (info["count_ms"] > 0) == (total > 0)
    assert abs(info["device_ms"] - (info["count_ms"] + info["offsets_ms"] + info["scatter_ms"])) < 1e-6
    sc.assert_shards_equal(shards, d.split_postings(num_docs, lists, shard_of, nshards))
    return shards, info


# ---------------------------------------------------------------- the kernels, against the twin
@pytest.mark.parametrize("nshards", [1, 2, 3, 64])
@pytest.mark.parametrize("keep", sc.KEEPS)
def test_window_edges(built_lib, keep, nshards):
    """lists of 1, 63, 64, 65, W - 1, W, W + 1, 2 W + 1 and 3 W - 1 postings and an empty one, starting on window boundaries and in
    mid-window, with the postings ending in mid-window and on a boundary; shard 0 keeps what `keep` names, with and without drops"""
    W = d.split_window()
    for whole_windows in (False, True):
        num_docs, lists = sc.window_edge_lists(W, whole_windows)
        assert {len(dd) for dd, _ in lists} >= {0, 1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1, 3 * W - 1}
        for drops in (False, True):
            shard_of = sc.window_edge_assign(W, num_docs, keep, nshards, drops)
            shards, _ = check_postings(num_docs, lists, shard_of, nshards)
            assert len(shards) == nshards and all(s[0] > 0 for s in shards)
            if keep == "all":
                rc.assert_lists_equal([(shards[0][2][dd], ff) for dd, ff in shards[0][1]], [ll for ll in lists if len(ll[0])])  # (old ids through doc_map)
                assert all(s[1] == [] for s in shards[1:])
    sc.assert_shards_equal(shards, sc.numpy_split(num_docs, lists, shard_of, nshards))  # (the twin itself, once per case)


def test_the_grid_wraps_inside_a_list_of_millions(built_lib, capsys):
    """a launch has at most split_grid_waves(CUs) wavefronts, a window of W postings each at a time: a list of twice that many windows,
    five more and 17 postings makes every wavefront take a second window and some a third, all inside one list; split by doc parity"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, waves = d.split_window(), d.split_grid_waves(cus)
    n = (2 * waves + 5) * W + 17
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    lists = [(np.arange(n, dtype=np.uint32), (1 + np.arange(n) % 9).astype(np.uint32)), (one(7, 8, n - 1), one(3, 4, 5))]
    shard_of = sc.round_robin_assign(n, 2)
    t0 = time.perf_counter()
    want = d.split_postings(n, lists, shard_of)
    twin_s = time.perf_counter() - t0
    shards, info = d.gpu_split_postings(n, lists, shard_of)
    sc.assert_shards_equal(shards, want)
    assert [len(s[1][0][0]) for s in shards] == [(n + 1) // 2, n // 2]
    assert np.array_equal(shards[1][1][0][0], np.arange(n // 2)) and np.array_equal(shards[0][1][0][1], lists[0][1][::2])
    with capsys.disabled():
        print("\nsplit of %d postings in 2 shards on %d CUs: count %.3f ms, offsets %.3f ms, scatter %.3f ms; host twin %.1f ms"
              % (n + 3, cus, info["count_ms"], info["offsets_ms"], info["scatter_ms"], 1e3 * twin_s))


def test_many_short_lists_split_by_doc_parity(built_lib):
    """6000 lists of 1, 2 and 3 postings split by the parity of the doc-id: every full window spans hundreds of list starts (W / 2 on
    average, so k_split_offsets counts many starts inside one window), and the lists that keep nothing vanish in long runs from either
    shard: a list of one posting lies in one shard only"""
    coll = sc.short_lists_collection()
    W = d.split_window()
    assert {len(dd) for dd, _ in coll.lists} == {1, 2, 3} and len(coll.lists) >= 5000
    assert any(np.any(dd % 2 == 0) for dd, _ in coll.lists) and any(np.any(dd % 2 == 1) for dd, _ in coll.lists)
    per_window = sc.list_starts_per_window(coll.lists, W)
    assert len(per_window) >= 8 and np.all(per_window[:-1] >= max(200, W // 3)), per_window  # (hundreds of starts in every full window)
    shard_of = sc.round_robin_assign(coll.num_docs, 2)
    shards, _ = check_postings(coll.num_docs, coll.lists, shard_of)
    sc.assert_shards_equal(shards, sc.numpy_split(coll.num_docs, coll.lists, shard_of, 2))
    sc.assert_shards_equal(shards, sc.from_merge_shards(mc.round_robin_shards(coll, 2)))
    # every list of one posting vanishes from exactly one shard, the longer ones from at most one: that alone is a third of the lists
    ones = sum(1 for dd, _ in coll.lists if len(dd) == 1)
    gone = [len(coll.lists) - len(s[1]) for s in shards]
    assert ones == len(coll.lists) // 3 and sum(gone) >= ones and min(gone) >= ones // 4, gone
    for s in shards:  # and they vanish side by side: somewhere four lists in a row are missing
        assert np.max(np.diff(np.concatenate([[-1], s[3].astype(np.int64), [len(coll.lists)]]))) >= 5


def test_doc_ids_past_2_24(built_lib):
    num_docs, lists, shard_of = sc.past_2_24_case()
    shards, _ = check_postings(num_docs, lists, shard_of)
    sc.assert_shards_equal(shards, sc.numpy_split(num_docs, lists, shard_of, 2))
    assert int(shards[0][2][-1]) > 1 << 24 and int(shards[0][1][0][0][-1]) > (1 << 24) - 10


# ---------------------------------------------------------------- images: == the host builder's image of every shard, on bytes
def assign(coll, how, cuts):
    return sc.range_assign(coll.num_docs, cuts) if how == "range" else sc.round_robin_assign(coll.num_docs, 3)


def check_images(name, coll, kind, to_kind, how, cuts=sc.EDGE_CUTS):
    shard_of = assign(coll, how, cuts)
    got, info = d.gpu_split_index(kind, cases.image(coll, kind), shard_of, to_kind=to_kind)
    for part in ("extract_ms", "count_ms", "offsets_ms", "scatter_ms", "encode_ms"):
        assert info[part] > 0, part
    assert abs(info["device_ms"] - sum(info[p] for p in ("extract_ms", "count_ms", "offsets_ms", "scatter_ms", "encode_ms"))) < 1e-6
    want = d.split_postings(coll.num_docs, coll.lists, shard_of)
    assert len(got) == len(want) == 3
    for s, ((img, doc_map, term_map), shard) in enumerate(zip(got, want)):
        assert np.array_equal(doc_map, shard[2]) and np.array_equal(term_map, shard[3]), s
        expected = sc.shard_image((name, how, s), coll, shard, to_kind)
        if img != expected:
            k = min(len(img), len(expected))
            bad = np.flatnonzero(np.frombuffer(img[:k], dtype=np.uint8) != np.frombuffer(expected[:k], dtype=np.uint8))
            print("shard, lengths, first differing byte, differing bytes:", s, len(img), len(expected), int(bad[0]) if len(bad) else None, len(bad))
        assert img == expected, s
    return got


@pytest.mark.parametrize("how", ["range", "rr3"])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_every_kind_splits_to_block_optpfor(built_lib, kind, how):
    check_images("edge", rc.block_edge_collection(), kind, "block_optpfor", how)


@pytest.mark.parametrize("how", ["range", "rr3"])
@pytest.mark.parametrize("to_kind", cases.GPU_BUILT_KINDS)
def test_block_optpfor_splits_to_every_gpu_built_kind(built_lib, to_kind, how):
    check_images("edge", rc.block_edge_collection(), "block_optpfor", to_kind, how)


@pytest.mark.parametrize("how", ["range", "rr3"])
@pytest.mark.parametrize("to_kind", cases.FREQ_KINDS)
def test_the_freq_edge_collection_splits_to_the_elias_fano_kinds(built_lib, to_kind, how):
    """(prefix sums of freqs past 2^32, which the block codecs are not built for: the source is an opt image)"""
    check_images("freq_edge", cases.freq_edge_collection(), "opt", to_kind, how, cuts=sc.FREQ_EDGE_CUTS)


@pytest.mark.parametrize("how", ["range", "rr3"])
@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_the_loop_closes(built_lib, kind, how):
    """gpu_merge_indexes over gpu_split_index's output, fed back unchanged, is the original image; round robin takes merge's sort path"""
    coll = rc.block_edge_collection()
    image = cases.image(coll, kind)
    shards, _ = d.gpu_split_index(kind, image, assign(coll, how, sc.EDGE_CUTS))
    merged, info = d.gpu_merge_indexes([(kind,) + s for s in shards], kind)
    assert (info["sort_ms"] > 0) == (how == "rr3")
    assert merged == image


@pytest.mark.parametrize("how", ["rr3", "deletion"])
def test_a_shard_answers_queries(built_lib, how):
    """`and` with want_matches over a shard == the original index's match lists filtered to the shard's documents and renumbered
    through doc_map. Counts and ids only: no scores. deletion: one shard, a tenth of the documents dropped."""
    coll = rc.small_collection()
    n = coll.num_docs
    if how == "rr3":
        shard_of = sc.round_robin_assign(n, 3)
    else:
        shard_of = np.where(np.random.default_rng(0xDE1).random(n) < 0.1, d.DROP, 0).astype(np.uint32)
    queries = [[a, b] for a in range(8) for b in range(a + 1, 8)] + [[0, 1, 2], [1, 3, 5, 7], [0, 299], [298, 299], [5]]
    whole = d.Index("block_optpfor", cases.image(coll, "block_optpfor"))
    try:
        b = d.Batch(whole, "and", queries, want_matches=True)
        b.run()
        matches = b.fetch_matches(b.fetch()[0])
        b.close()
        shards, _ = whole.split(shard_of)
    finally:
        whole.close()
    assert sum(len(m) for m in matches) > 1000
    for s, (image, doc_map, term_map) in enumerate(shards):
        assert np.array_equal(doc_map, np.flatnonzero(shard_of == s))
        local_term = {int(t): i for i, t in enumerate(term_map)}
        want = [np.searchsorted(doc_map, m[shard_of[m] == s]).astype(np.uint32) for m in matches]
        asked = [i for i, q in enumerate(queries) if all(t in local_term for t in q)]
        for i in set(range(len(queries))) - set(asked):
            assert len(want[i]) == 0  # (a term the shard lacks: nothing to find there)
        idx = d.Index("block_optpfor", image)
        try:
            assert idx.num_docs() == len(doc_map) and idx.size() == len(term_map)
            b = d.Batch(idx, "and", [[local_term[t] for t in queries[i]] for i in asked], want_matches=True)
            b.run()
            count = b.fetch()[0]
            got = b.fetch_matches(count)
            b.close()
        finally:
            idx.close()
        for i, c, m in zip(asked, count, got):
            assert int(c) == len(want[i]) and np.array_equal(m, want[i]), (s, queries[i])


# ---------------------------------------------------------------- errors on the device
def test_split_errors(built_lib):
    coll = rc.block_edge_collection()
    image = cases.image(coll, "block_optpfor")
    shard_of = sc.range_assign(coll.num_docs, sc.EDGE_CUTS)
    for call in (lambda: d.gpu_split_index("block_optpfor", image, shard_of, device=99), lambda: d.gpu_split_postings(coll.num_docs, coll.lists, shard_of, device=99)):
        with pytest.raises(d.Ds2iError) as e:
            call()
        assert e.value.code == -4
    # a shard with documents and no posting: every doc-id of the lists but the last document's is even or lies in the run
    lonely = shard_of.copy()
    lonely[[1, 3, 5]] = 3
    assert not any(np.isin([1, 3, 5], dd).any() for dd, _ in coll.lists)
    L = built_lib
    h = d.api.C.c_void_p()
    code = L.ds2i_hip_split_index(0, 0, image, len(image), lonely.ctypes.data_as(d.api.C.c_void_p), len(lonely), 4, 0, d.api.C.byref(h), None)
    msg = L.ds2i_hip_last_error().decode()
    assert code == -1 and not h.value and "shard 3 receives no posting: List must be nonempty" in msg
    assert d.gpu_split_postings(coll.num_docs, coll.lists, lonely)[0][3][1] == []  # (the postings form hands it back without a list)


def test_a_doc_id_outside_the_documents_is_a_format_error(built_lib):
    """the count kernel flags it and reads nothing past shard_of; the call refuses the result and writes no output"""
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    lists = [(one(3, 9), one(1, 1)), (one(2, 10), one(1, 1))]  # ten documents
    shard_of = (np.arange(10) % 2).astype(np.uint32)
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_split_postings(10, lists, shard_of)
    assert e.value.code == -2 and "outside the 10 documents" in str(e.value)
    # the C entry point itself: the code, and the output handle and the time left as they were
    C = d.api.C
    n, offs, docs, freqs = d.api._csr(lists)
    h, ms = C.c_void_p(), C.c_double(-1.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    code = built_lib.ds2i_hip_split_postings(0, 10, n, ptr(offs), ptr(docs), ptr(freqs), ptr(shard_of), 2, C.byref(h), C.byref(ms))
    assert code == -2 and not h.value and "outside the 10 documents" in built_lib.ds2i_hip_last_error().decode()


# ---------------------------------------------------------------- the tool
def test_tool_splits_checks_and_prints_the_merge_that_undoes_it(built_lib, tmp_path):
    if not (os.path.exists(SPLIT) and os.path.exists(MERGE)):
        subprocess.check_call(["make", "-C", TOOLS, "-s"])
    coll = rc.block_edge_collection()
    image = cases.image(coll, "block_optpfor")
    src, out, assign_file = str(tmp_path / "index"), str(tmp_path / "shard"), str(tmp_path / "assign")
    open(src, "wb").write(image)
    shard_of = sc.round_robin_assign(coll.num_docs, 3)
    rc.write_map(assign_file, shard_of)

    def run(*args):
        return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)

    p = run(SPLIT, "block_optpfor", src, "block_optpfor", out, "--assign", assign_file, "--check")
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    want = d.split_postings(coll.num_docs, coll.lists, shard_of)
    assert lines[1:] == ["OK lists=%d postings=%d" % (len(s[1]), sum(len(dd) for dd, _ in s[1])) for s in want]
    got, _ = d.gpu_split_index("block_optpfor", image, shard_of)
    for s, (img, doc_map, term_map) in enumerate(got):
        base = "%s.%d" % (out, s)
        assert open(base, "rb").read() == img
        for path, m in ((base + ".docs", doc_map), (base + ".terms", term_map)):
            words = np.fromfile(path, dtype=np.uint32)
            assert words[0] == len(m) and np.array_equal(words[1:], m)
    # the printed command puts the input back, byte for byte
    words = lines[0].split()
    assert words[0] == "merge_indexes" and words[2] == out + ".merged"
    p = run(MERGE, *words[1:])
    assert p.returncode == 0, p.stderr
    assert open(out + ".merged", "rb").read() == image
    # --ranges cuts the same shards as the range assignment
    p = run(SPLIT, "block_optpfor", src, "opt", out + "r", "--ranges", ",".join(map(str, sc.EDGE_CUTS)), "--check")
    assert p.returncode == 0 and len(p.stdout.splitlines()) == 4, (p.stdout, p.stderr)
    ranged, _ = d.gpu_split_index("block_optpfor", image, sc.range_assign(coll.num_docs, sc.EDGE_CUTS), to_kind="opt")
    assert [open("%sr.%d" % (out, s), "rb").read() for s in range(3)] == [img for img, _, _ in ranged]
