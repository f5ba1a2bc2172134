"""wand_data built on the GPU (-m gpu): ds2i_hip_build_wand and the one-call ds2i_hip_build_collection. The reference of every
comparison is the HOST builder (build_wand / build_index), and every comparison is == on bytes: a maximum has no rounding of
its own, the weights come from the scoring code's doc_term_weight (pinned bit for bit to the reference's bm25.hpp by
test_device_bm25_equals_reference_fixture) and norm_lens are computed by the host's own compute_norm_lens."""
import numpy as np
import pytest

import ds2i_amd as d
import wand_build_cases as cases

pytestmark = pytest.mark.gpu

GPU_KINDS = ("block_optpfor", "block_varint", "block_interpolative")


@pytest.fixture(scope="module")
def small(built_lib):
    coll, names = cases.small_collection()
    return coll, names, coll.wand_image()


@pytest.fixture(scope="module")
def small_gpu_wand(small):
    coll, _, _ = small
    return d.gpu_build_wand(coll.sizes, coll.lists)


@pytest.fixture(scope="module")
def big(built_lib):
    coll, names = cases.big_collection()
    return coll, names, coll.wand_image()


def test_wand_image_equals_the_host_builders(small, small_gpu_wand):
    coll, names, host = small
    img, info = small_gpu_wand
    assert info["device_ms"] > 0
    if img != host:  # name the lists before the byte comparison fails
        got = cases.image_max_term_weights(img, coll.num_docs, len(coll.lists))
        want = cases.image_max_term_weights(host, coll.num_docs, len(coll.lists))
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        by_term = {t: n for n, t in names.items()}
        print([(int(t), by_term.get(int(t)), len(coll.lists[t][0]), float(got[t]), float(want[t])) for t in bad[:20]])
    assert img == host


def test_every_shape_is_in_the_collection(small):
    """what the byte comparison above is worth: the lengths, the placed maxima, both ends of norm_len, both freq regimes"""
    coll, names, host = small
    for n in cases.EDGE_LENGTHS:
        assert len(coll.lists[names["len%d" % n]][0]) == n
    for name, (n, at) in cases.PLACED.items():
        _, where = cases.max_term_weight(coll, names[name])
        assert len(coll.lists[names[name]][0]) == n and tuple(where) == at
    hit = np.unique(np.concatenate([dd for dd, _ in coll.lists]))
    assert coll.norm_lens[hit].min() == coll.norm_lens.min() and coll.norm_lens[hit].max() == coll.norm_lens.max()
    assert int(coll.sizes.min()) == 1 and int(coll.sizes.max()) == 3000000
    assert int(coll.lists[names["ones"]][1].max()) == 1 and int(coll.lists[names["big_f"]][1].max()) == (1 << 31) - 2
    assert 280 <= len(coll.lists) <= 320 and coll.num_docs == cases.NUM_DOCS


@pytest.mark.parametrize("codec", GPU_KINDS)
def test_build_collection_is_encode_index_and_build_wand(small, small_gpu_wand, codec):
    coll, _, host_wand = small
    index, wand, info = d.gpu_build_collection(coll.num_docs, coll.sizes, coll.lists, codec=codec)
    assert info["device_ms"] > 0
    assert index == d.gpu_encode_index(coll.num_docs, coll.lists, codec=codec)[0]
    assert wand == small_gpu_wand[0]
    assert index == d.build_index(codec, coll.num_docs, coll.lists)
    assert wand == host_wand


def test_long_list_and_doc_ids_past_2_24(big):
    coll, names, host_wand = big
    assert coll.num_docs == (1 << 24) + (1 << 18) and len(coll.lists[names["long"]][0]) >= 300000
    m, where = cases.max_term_weight(coll, names["straddle"])
    assert tuple(where) == (2,) and int(coll.lists[names["straddle"]][0][2]) == (1 << 24) + 1
    img, info = d.gpu_build_wand(coll.sizes, coll.lists)
    assert info["device_ms"] > 0
    got = cases.image_max_term_weights(img, coll.num_docs, len(coll.lists))
    assert got[names["straddle"]] == m
    assert img == host_wand
    index, wand, _ = d.gpu_build_collection(coll.num_docs, coll.sizes, coll.lists)
    assert wand == host_wand and index == d.build_index("block_optpfor", coll.num_docs, coll.lists)


def test_gpu_built_images_answer_ranked_queries(small):
    coll, _, host_wand = small
    queries = cases.small_queries(coll, 64)
    index, wand, _ = d.gpu_build_collection(coll.num_docs, coll.sizes, coll.lists)
    gpu_built = d.Index("block_optpfor", index, wand)
    host_built = d.Index("block_optpfor", coll.index_image("block_optpfor"), host_wand)
    for op in ("ranked_and", "wand"):
        _, topk, tlen, _ = gpu_built.query_batch(op, queries, k=10)
        _, rtopk, rtlen, _ = host_built.query_batch(op, queries, k=10)
        assert np.array_equal(tlen, rtlen) and int(tlen.sum()) > 0
        assert topk.tobytes() == rtopk.tobytes()


def test_errors(small):
    coll, _, _ = small
    some = coll.lists[:3]
    empty = some + [(np.zeros(0, np.uint32), np.zeros(0, np.uint32))]
    past = some + [(np.array([5, coll.num_docs], np.uint32), np.array([1, 1], np.uint32))]
    for lists in (empty, past):  # "List must be nonempty"; a doc-id the gather would read past norm_lens for
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_build_wand(coll.sizes, lists)
        assert e.value.code == -1
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_build_collection(coll.num_docs, coll.sizes, lists)
        assert e.value.code == -1
    for codec in ("block_qmx", "block_mixed"):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_build_collection(coll.num_docs, coll.sizes, some, codec=codec)
        assert e.value.code == -1
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_build_wand(coll.sizes, some, device=99)
    assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_build_collection(coll.num_docs, coll.sizes, some, device=99)
    assert e.value.code == -4
