"""The Elias-Fano layouts -- opt, ef, single, uniform -- encoded on the GPU (-m gpu): ds2i_hip_encode_index and
ds2i_hip_build_collection for the four freq_index kinds. The reference of every image comparison is the HOST builder
(build_index) and every comparison is == on bytes: the layouts are integers throughout, there is no tolerance."""
import numpy as np
import pytest

import ds2i_amd as d
import freq_encode_cases as cases
from helpers import Collection, queries_for, small_params

pytestmark = pytest.mark.gpu

KINDS = list(d.FREQ_INDEX_KINDS)


@pytest.fixture(scope="module")
def small(built_lib):
    """a few hundred synthetic lists, every fourth clustered: the opt DP cuts partitions of many sizes"""
    coll = Collection(small_params(num_docs=20000, num_terms=300, clustered_every=4))
    return coll, coll.wand_image()


@pytest.fixture(scope="module")
def small_host(small):
    coll, _ = small
    return {kind: coll.index_image(kind) for kind in KINDS}


@pytest.fixture(scope="module")
def small_gpu(small):
    coll, _ = small
    return {kind: d.gpu_encode_index(coll.num_docs, coll.lists, codec=kind) for kind in KINDS}


@pytest.fixture(scope="module")
def edge(built_lib):
    return cases.edge_collection()


def first_difference(a, b):
    m = min(len(a), len(b))
    x, y = np.frombuffer(a[:m], dtype=np.uint8), np.frombuffer(b[:m], dtype=np.uint8)
    bad = np.flatnonzero(x != y)
    return (len(a), len(b), int(bad[0]) if len(bad) else None, len(bad))


@pytest.mark.parametrize("kind", KINDS)
def test_small_collection_image_equals_the_host_builders(small_host, small_gpu, kind):
    img, ms = small_gpu[kind]
    assert ms > 0
    if img != small_host[kind]:
        print("lengths, first differing byte, differing bytes:", first_difference(img, small_host[kind]))
    assert img == small_host[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_edge_lists_in_one_image(edge, kind):
    coll, _ = edge
    img, _ = d.gpu_encode_index(coll.num_docs, coll.lists, codec=kind)
    host = coll.index_image(kind)
    if img != host:
        print("lengths, first differing byte, differing bytes:", first_difference(img, host))
    assert img == host  # (images only: the freqs of big_f sum past 2^32)


@pytest.mark.parametrize("kind", KINDS)
def test_dense_lists_in_a_small_universe(built_lib, kind):
    coll = cases.dense_collection()
    img, _ = d.gpu_encode_index(coll.num_docs, coll.lists, codec=kind)
    assert img == coll.index_image(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip(small, small_host, small_gpu, kind):
    coll, wand = small
    gpu_built = d.Index(kind, small_gpu[kind][0], wand)
    longest = int(np.argmax([len(dd) for dd, _ in coll.lists]))
    for t in (0, len(coll.lists) - 1, longest):
        docs, freqs = gpu_built[t]
        assert np.array_equal(docs, coll.lists[t][0]) and np.array_equal(freqs, coll.lists[t][1]), t
    queries = queries_for(coll, nq=48)
    host_built = d.Index(kind, small_host[kind], wand)
    _, topk, tlen, _ = gpu_built.query_batch("ranked_and", queries, k=10)
    _, rtopk, rtlen, _ = host_built.query_batch("ranked_and", queries, k=10)
    assert np.array_equal(tlen, rtlen) and int(tlen.sum()) > 0
    assert topk.tobytes() == rtopk.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_build_collection_is_encode_index_and_build_wand(small, small_gpu, kind):
    coll, host_wand = small
    index, wand, info = d.gpu_build_collection(coll.num_docs, coll.sizes, coll.lists, codec=kind)
    assert info["device_ms"] > 0
    assert index == small_gpu[kind][0]
    assert wand == d.gpu_build_wand(coll.sizes, coll.lists)[0]
    assert wand == host_wand


@pytest.mark.parametrize("kind", KINDS)
def test_errors(small, kind):
    coll, _ = small
    some = coll.lists[:3]
    zero = some + [(np.array([5, 9], np.uint32), np.array([1, 0], np.uint32))]
    unsorted = some + [(np.array([9, 5], np.uint32), np.array([1, 1], np.uint32))]
    for lists in (zero, unsorted):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_encode_index(coll.num_docs, lists, codec=kind)
        assert e.value.code == -1
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_build_collection(coll.num_docs, coll.sizes, lists, codec=kind)
        assert e.value.code == -1
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_encode_index(coll.num_docs, some, device=99, codec=kind)
    assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_build_collection(coll.num_docs, coll.sizes, some, device=99, codec=kind)
    assert e.value.code == -4
