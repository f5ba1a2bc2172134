"""Merging indexes on the GPU (-m gpu): ds2i_hip_merge_postings against the host twin, ds2i_hip_merge_indexes against the HOST builder's
image of the whole collection its shards were cut from, and the merge_indexes tool. Everything is integers and doc-ids are distinct
across sources, so the answer is unique: lists are compared with np.array_equal, images and files with == on bytes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ds2i_amd as d
import merge_cases as mc
import remap_cases as rc
import verify_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "ds2i_amd", "tools")
MERGE = os.path.join(TOOLS, "merge_indexes")
EDGE_CUTS = (7300, 30001)  # (the first cut lies inside the run of 700 consecutive doc-ids)


@pytest.fixture(scope="module")
def bounds(built_lib):
    return d.remap_class_bounds()


def check_postings(shards):
    num_docs, lists, info = d.gpu_merge_postings(mc.api_sources(shards))
    assert info["device_ms"] > 0 and info["place_ms"] > 0 and info["extract_ms"] == 0 and info["encode_ms"] == 0
    mc.assert_merged_equal((num_docs, lists), d.merge_postings(mc.api_sources(shards)))
    return lists, info


# ---------------------------------------------------------------- the placement, against the twin
def test_class_edge_runs_with_default_maps_sort_nothing(bounds):
    """source runs of 1, 63, 64, 65, 127, 128, 129, L, L + 1 and 2 T + 1 postings (windows inside one list, windows over many lists); one
    source adds a single posting to the list of 2 T + 1; every merged list is sorted as placed"""
    W, L, T = bounds
    shards = mc.class_edge_sources(bounds, interleave=False)
    runs = {len(dd) for s in shards for dd, _ in s.lists}
    assert {1, 63, 64, 65, 127, 128, 129, L, L + 1, 2 * T + 1} <= runs
    lists, info = check_postings(shards)
    assert info["sort_ms"] == 0.0
    assert 2 * T + 2 in {len(dd) for dd, _ in lists}
    for dd, _ in lists:
        assert np.all(np.diff(dd.astype(np.int64)) > 0)


def test_class_edge_runs_with_interleaving_maps_sort_every_class(bounds):
    W, L, T = bounds
    shards = mc.class_edge_sources(bounds, interleave=True)
    lists, info = check_postings(shards)
    assert info["sort_ms"] > 0
    merged = [len(dd) for dd, _ in lists]
    assert min(merged) <= W < max(m for m in merged if m <= L) and max(merged) > L  # every sort class had lists
    for dd, _ in lists:
        assert np.all(np.diff(dd.astype(np.int64)) > 0)


def test_many_lists_split_by_doc_parity():
    """16 x CUs + 300 lists of 1, 1, 1, 2, 129 postings split by doc parity: nearly every window of the placement spans hundreds of
    source lists one posting long, and a store past a run's end lands in a neighbour's and shows. (Every doc-id of that collection is
    even, so the parity is that of d // 2: the split by d % 2 would leave one shard without a list.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    coll = cases.many_lists_collection(cus)
    assert all(np.all(dd % 2 == 0) for dd, _ in coll.lists)
    shards = mc.round_robin_shards(coll, 2, group=2)
    lists, _ = check_postings(shards)
    rc.assert_lists_equal(lists, coll.lists)


def test_the_grid_wraps_inside_a_list_of_millions():
    """the placement's grid is min(windows / 4, 8 x CUs) workgroups of four wavefronts, a window of 1024 postings each at a time: a list
    of 32 x CUs + 5 windows and 17 postings makes every wavefront take a second window, all but the last inside that one list"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (32 * cus + 5) * 1024 + 17
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    a = mc.Shard(2 * n, [(np.arange(n, dtype=np.uint32) * 2, (1 + np.arange(n) % 9).astype(np.uint32)), (one(7), one(3))], None, None, None)
    b = mc.Shard(11, [(one(0, 10), one(2, 2))], None, one(1), None)
    lists, info = check_postings([a, b])
    assert info["sort_ms"] == 0.0 and len(lists[0][0]) == n and lists[1][0].tolist() == [7, 2 * n, 2 * n + 10]


def test_doc_ids_past_2_24():
    """default maps: every base lies past 2^24; then the reverse of the concatenation as explicit maps"""
    for reverse in (False, True):
        shards = mc.past_2_24_sources(reverse)
        lists, info = check_postings(shards)
        mc.assert_merged_equal((mc.PAST_2_24 + 150, lists), mc.numpy_merge(shards))
        assert (info["sort_ms"] > 0) == reverse
        assert all(int(dd[-1]) > 1 << 24 for dd, _ in lists)


def test_a_doc_id_outside_a_sources_map_is_a_format_error():
    """the placement kernel flags it, stores nothing for it and reads nothing past the map; the call refuses the result"""
    one = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    lists = [[(one(3, 9), one(1, 1))], [(one(2, 5), one(1, 1))]]  # the second source holds five documents
    for maps in ((None, None), (np.arange(10, dtype=np.uint32) + np.uint32(5), np.arange(5, dtype=np.uint32))):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_merge_postings([(10, lists[0], maps[0]), (5, lists[1], maps[1])])
        assert e.value.code == -2 and "outside the map" in str(e.value) and "source 1" in str(e.value)


# ---------------------------------------------------------------- images: == the host builder's image of the whole collection, on bytes
def check_image(coll, shards, kinds, to_kind, sorted_=False):
    img, info = d.gpu_merge_indexes(mc.image_sources(shards, kinds), to_kind, num_terms=len(coll.lists))
    assert info["device_ms"] > 0 and info["extract_ms"] > 0 and info["place_ms"] > 0 and info["encode_ms"] > 0
    assert (info["sort_ms"] > 0) == sorted_
    want = cases.image(coll, to_kind)
    if img != want:
        k = min(len(img), len(want))
        bad = np.flatnonzero(np.frombuffer(img[:k], dtype=np.uint8) != np.frombuffer(want[:k], dtype=np.uint8))
        print("lengths, first differing byte, differing bytes:", len(img), len(want), int(bad[0]) if len(bad) else None, len(bad))
    assert img == want
    return img


@pytest.mark.parametrize("rotation", [0, 1, 2])
def test_range_shards_of_every_kind_merge_to_block_optpfor(built_lib, rotation):
    """three range shards whose kinds rotate through all nine"""
    coll = rc.block_edge_collection()
    kinds = cases.KINDS[3 * rotation:3 * rotation + 3]
    check_image(coll, mc.range_shards(coll, EDGE_CUTS), kinds, "block_optpfor")


@pytest.mark.parametrize("to_kind", cases.GPU_BUILT_KINDS)
def test_block_optpfor_shards_merge_to_every_gpu_built_kind(built_lib, to_kind):
    coll = rc.block_edge_collection()
    img = check_image(coll, mc.range_shards(coll, EDGE_CUTS), ("block_optpfor",), to_kind)
    if to_kind == "block_optpfor":
        idx = d.Index(to_kind, img)
        try:
            r = idx.verify(coll.lists)
            assert r["ok"] and r["postings_checked"] == cases.postings(coll)
        finally:
            idx.close()


def test_freq_edge_shards_merge_to_opt(built_lib):
    coll = cases.freq_edge_collection()
    shards = mc.range_shards(coll, (70350, 600000))  # (the first cut lies inside the run of consecutive doc-ids)
    check_image(coll, shards, cases.FREQ_KINDS, "opt")


@pytest.mark.parametrize("to_kind", ["block_optpfor", "opt"])
def test_round_robin_shards_merge_through_the_sort(built_lib, to_kind):
    coll = rc.block_edge_collection()
    check_image(coll, mc.round_robin_shards(coll, 3), ("opt", "block_varint", "block_optpfor"), to_kind, sorted_=True)


def test_one_source_without_maps_is_a_conversion(built_lib):
    coll = rc.block_edge_collection()
    src = cases.image(coll, "opt")
    img, info = d.gpu_merge_indexes([("opt", src)], "block_varint")
    assert info["sort_ms"] == 0.0
    assert img == d.gpu_convert_index("opt", src, "block_varint")[0] == cases.image(coll, "block_varint")


def test_merge_errors(built_lib):
    coll = rc.block_edge_collection()
    srcs = mc.image_sources(mc.range_shards(coll, EDGE_CUTS), ("opt",))
    for to_kind in ("block_qmx", "block_mixed"):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_merge_indexes(srcs, to_kind)
        assert e.value.code == -1 and all(name in str(e.value) for name in cases.GPU_BUILT_KINDS)
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_merge_indexes(srcs[:2] + [("opt", cases.GARBAGE)], "block_optpfor")
    assert e.value.code == -2
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_merge_indexes(srcs, "block_optpfor", num_terms=len(coll.lists) + 1)
    assert e.value.code == -1 and "List must be nonempty" in str(e.value)


# ---------------------------------------------------------------- the tool
def test_tool_merges_checks_and_writes_the_python_paths_file(built_lib, tmp_path):
    if not os.path.exists(MERGE):
        subprocess.check_call(["make", "-C", TOOLS, "-s"])
    coll = rc.block_edge_collection()
    shards = mc.round_robin_shards(coll, 3)
    kinds = ("opt", "block_varint", "block_qmx")
    srcs = mc.image_sources(shards, kinds)
    args, out = [], str(tmp_path / "merged")
    for i, (kind, image, doc_map, term_map) in enumerate(srcs):
        base = str(tmp_path / ("shard%d" % i))
        open(base, "wb").write(image)
        mc.write_map(base + ".docs", doc_map)
        mc.write_map(base + ".terms", term_map)
        args += [kind, base, "--docs", base + ".docs", "--terms", base + ".terms"]

    def run(*flags):
        return subprocess.run([MERGE, "block_optpfor", out] + args + list(flags), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              universal_newlines=True, timeout=120)

    p = run("--check")
    assert p.returncode == 0, p.stderr
    assert p.stdout == "OK lists=%d postings=%d\n" % (len(coll.lists), cases.postings(coll))
    written = open(out, "rb").read()
    assert written == d.gpu_merge_indexes(srcs, "block_optpfor")[0] == cases.image(coll, "block_optpfor")
    # one source file altered (a shard built again with one freq changed, never an image's bytes): the written file no longer matches
    t = len(shards[1].lists) - 1
    lists = cases.altered(shards[1].lists, [(t, 0, "freq", int(shards[1].lists[t][1][0]) + 2)])
    open(str(tmp_path / "shard1"), "wb").write(d.build_index("block_varint", shards[1].num_docs, lists))
    p = run("--check-only")
    assert p.returncode == 1 and p.stdout.startswith("MISMATCH freq list=%d " % int(shards[1].term_map[t])), (p.stdout, p.stderr)
    assert open(out, "rb").read() == written  # --check-only writes nothing
