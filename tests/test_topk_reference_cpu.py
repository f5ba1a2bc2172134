"""The float64 top-k BM25 of tests/helpers.py (topk64) against the oracle, on the CPU: the GPU matrix (test_gpu_modes.py) holds
the kernels to both, so the two references must agree with each other first -- and the oracle's topk_queue gets tested at the
k boundaries of the kernels (64 | 65, 256 | 257, 1024) on result sets of exactly k - 1, k and k + 1 documents and on ties
at the k-th place."""
import numpy as np
import pytest

import oracle as o
from helpers import (BOUNDARY_SIZES, Collection, boundary_collection, boundary_queries, edge_queries, queries_for, small_params,
                     topk64)

RTOL = 1e-5
K64 = (1, 65, 257, 1024)
RANKED = ("ranked_and", "wand", "maxscore", "ranked_or")


@pytest.fixture(scope="module", params=["boundary", "synth"])
def world(request, built_lib):
    if request.param == "boundary":
        coll = boundary_collection()
        qs = boundary_queries(coll)
    else:
        coll = Collection(small_params(num_docs=20000, num_terms=300))
        qs = queries_for(coll, 120) + edge_queries(coll.p.num_terms)
    oidx = o.Index("block_optpfor", coll.index_image("block_optpfor"), coll.wand_image())
    ref = {conj: [topk64(coll, q, max(K64), conj) for q in qs] for conj in (True, False)}
    return coll, qs, oidx, ref


def test_boundary_collection_result_sizes(built_lib):
    """the crafted collection has the result sizes it is built for: every size of BOUNDARY_SIZES (and k - 1 / k / k + 1 of
    every k boundary) as an AND and as an OR size, ties across the k-th place, doc ids 0 and num_docs - 1"""
    coll = boundary_collection()
    qs = boundary_queries(coll)
    and_n = {topk64(coll, q, 1, True)[1] for q in qs}
    or_n = {topk64(coll, q, 1, False)[1] for q in qs}
    assert set(BOUNDARY_SIZES) <= and_n and set(BOUNDARY_SIZES) <= or_n and coll.num_docs in or_n
    assert all(len(q) != 1 or topk64(coll, q, 1, True)[1] == len(coll.lists[q[0]][0]) for q in qs)
    assert {len(set(q)) for q in qs} >= set(range(0, 17)) and max(len(set(q)) for q in qs) > 16
    assert any(0 in dd and coll.num_docs - 1 in dd for dd, _ in coll.lists[1:])
    s, n = topk64(coll, [len(coll.lists) - 1], 1024, True)
    assert n == 300 and np.all(s == s[0])                   # one score for the whole tie group
    s, n = topk64(coll, [0, len(coll.lists) - 1], 1024, True)
    assert n == 300 and np.all(s == s[0])


@pytest.mark.parametrize("k", K64)
def test_float64_reference_equals_oracle(world, k):
    coll, qs, oidx, ref = world
    oc, _, _, _, _ = oidx.query_batch("and", qs)
    assert np.array_equal(oc, [r[1] for r in ref[True]])
    oc, _, _, _, _ = oidx.query_batch("or", qs)
    assert np.array_equal(oc, [r[1] for r in ref[False]])
    for op in RANKED:
        _, otopk, otlen, _, _ = oidx.query_batch(op, qs, k=k)
        for i, q in enumerate(qs):
            s, n = ref[op == "ranked_and"][i]
            assert otlen[i] == min(n, k), (op, k, q)
            np.testing.assert_allclose(otopk[i, :otlen[i]], s[:min(n, k)], rtol=RTOL, err_msg=str((op, k, q)))
            assert np.all(np.isneginf(otopk[i, otlen[i]:]))
