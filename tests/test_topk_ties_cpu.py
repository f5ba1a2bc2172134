"""The tie collection and the signature checks without a GPU (tests/test_gpu_topk_ties.py uses both on the kernels): the
collection is what its docstring says, the canonical answer of the brute force passes the three checks, an answer with one k-th-place
tie decided the wrong way fails them, and the oracle's ranked_and scores are the brute force's bits on at least the share of rows
the GPU test's exact comparison relies on."""
import numpy as np
import pytest

import oracle as o
from helpers import (TIE_CORE, TIE_EDGE, TIE_FREQS, TIE_HALF, TIE_NUM_DOCS, TIE_SIZES, TIE_STRADDLE, TIE_WINDOW_LO, tie_collection,
                     tie_ladder, tie_queries)
from topk_docs_ref import (TieRef, brute_pairs, canonical_topk, closed_within_signature, nothing_better_left_out,
                           same_signature_same_bits, signature_keys)

KS = (1, 10, 64, 65, 256, 257, 1024)
BIT_EQUAL_SHARE = 0.9  # (of the rows with a result: what test_gpu_topk_ties.py requires of the kernels)


@pytest.fixture(scope="module")
def coll():
    return tie_collection()


@pytest.fixture(scope="module")
def queries(coll):
    return tie_queries(coll)


def test_collection_is_what_it_says(coll):
    n = coll.num_docs
    assert n == TIE_NUM_DOCS == (1 << 24) + (1 << 18) and len(coll.lists) == 2 * TIE_HALF + 1
    assert set(np.unique(coll.sizes).tolist()) == set(TIE_SIZES)
    total = sum(len(dd) for dd, _ in coll.lists)
    assert 5e6 <= total <= 10e6, total
    for half, (lo, hi) in enumerate(((2000, 2000000), (2000, 128000))):
        lens = [len(coll.lists[half * TIE_HALF + i][0]) for i in range(TIE_HALF)]
        want = tie_ladder(lo, hi)
        assert all(0.75 * w <= m <= w for m, w in zip(lens, want)), (lens, want)  # (a draw with replacement: up to a fifth less in the window)
        assert all(1.15 <= b / a <= 1.7 for a, b in zip(lens, lens[1:])), lens     # a geometric ladder
        core = coll.lists[half * TIE_HALF][0]
        for i in range(1, TIE_HALF):
            core = np.intersect1d(core, coll.lists[half * TIE_HALF + i][0], assume_unique=True)
        assert len(core) >= 0.95 * TIE_CORE
        if half:
            assert set(TIE_STRADDLE) <= set(core.tolist())
    assert len(coll.lists[TIE_HALF - 1][0]) > 320 * 128 * 4  # the longest list: many units of the default planner (96 / 320 blocks each)
    for t in range(2 * TIE_HALF + 1):
        dd, ff = coll.lists[t]
        assert set(np.unique(ff).tolist()) == set(TIE_FREQS), t
        assert np.count_nonzero(ff == 1) > len(ff) // 2, t         # skewed to 1
        if t < TIE_HALF:
            assert dd[0] < n // 64 and dd[-1] >= TIE_EDGE, t       # spread over the universe, to both sides of 2^24
        elif t < 2 * TIE_HALF:
            assert TIE_WINDOW_LO <= dd[0] < TIE_EDGE < dd[-1], t   # the window straddles 2^24
            assert np.count_nonzero(dd >= TIE_EDGE) > len(dd) // 2, t
    dense = coll.lists[2 * TIE_HALF][0]
    assert dense[0] == 0 and dense[-1] == n - 1
    assert np.all(np.diff(dense[:1 << 15]) == 1) and np.all(np.diff(dense[-(1 << 15):]) == 1)
    assert coll.sizes[list(TIE_STRADDLE)].tolist() == [150] * 4


def test_queries_cover_the_shapes(coll, queries):
    assert [] in queries
    lens = [len(set(q)) for q in queries]
    assert sum(1 for n in lens if n > 16) == 2 and lens[-1] > 16 and lens[-2] > 16
    assert any(len(q) > len(set(q)) for q in queries)  # duplicated terms
    for half in range(2):
        inside = [q for q in queries if q and all(half * TIE_HALF <= t < (half + 1) * TIE_HALF for t in q)]
        assert set(len(set(q)) for q in inside) >= set(range(1, 17)), half
    assert any(min(q) < TIE_HALF <= max(q) < 2 * TIE_HALF for q in queries if q)  # mixed halves
    assert any(2 * TIE_HALF in q for q in queries)
    assert queries == tie_queries(coll)                # fixed seeds


def test_signature_is_size_and_freqs(coll):
    q = [20, 3, 20, 2 * TIE_HALF]
    docs = np.array([0, 5, TIE_EDGE - 1, TIE_EDGE, TIE_EDGE + 1, coll.num_docs - 1], dtype=np.uint32)
    docs = np.union1d(docs, coll.lists[20][0][:300]).astype(np.uint32)
    key = signature_keys(coll, q, docs)
    sig = {}
    for i, doc in enumerate(docs.tolist()):
        s = [int(coll.sizes[doc])]
        for t in sorted(set(q)):
            dd, ff = coll.lists[t]
            p = int(np.searchsorted(dd, doc))
            s.append(int(ff[p]) if p < len(dd) and dd[p] == doc else 0)
        sig.setdefault(int(key[i]), set()).add(tuple(s))
    assert all(len(v) == 1 for v in sig.values())                                   # one key, one signature
    assert len(set(next(iter(v)) for v in sig.values())) == len(sig)                # one signature, one key


def _some(queries, step=3):
    return [q for q in queries if q and len(set(q)) <= 16][::step]


@pytest.mark.parametrize("conj", [True, False])
def test_canonical_answer_passes_and_a_wrong_tie_fails(coll, queries, conj):
    """the three checks on canonical_topk of the brute force; then the same answer with the kept and the dropped document of its
    k-th-place tie swapped (closed_within_signature must refuse it), with a score bit flipped (same_signature_same_bits) and with
    its best document replaced by one from further down (nothing_better_left_out)"""
    swapped = 0
    for q in _some(queries) if conj else [q for q in _some(queries) if all(t >= TIE_HALF for t in q)]:
        ref = TieRef(coll, q, conj)
        s_all, d_all = brute_pairs(coll, q, 1025, conj, order="size" if conj else "term")
        assert ref.n >= len(d_all)
        for k in KS:
            s, dd = s_all[:k], d_all[:k]
            assert same_signature_same_bits(ref, dd, s) is None, (conj, q, k)
            assert closed_within_signature(ref, dd) is None, (conj, q, k)
            assert nothing_better_left_out(ref, dd, k) is None, (conj, q, k)
            if len(dd):
                assert nothing_better_left_out(ref, dd[:-1], k) is not None, (conj, q, k)  # a row one short
            if len(d_all) > k and s_all[k] == s_all[k - 1] and \
                    signature_keys(coll, q, d_all[k - 1:k])[0] == signature_keys(coll, q, d_all[k:k + 1])[0]:
                assert ref.tied_at(k), (conj, q, k)
                wrong = dd.copy()
                wrong[-1] = d_all[k]  # the dropped document of the tie instead of the kept one
                msg = closed_within_signature(ref, wrong)
                assert msg is not None and str(int(dd[-1])) in msg and str(int(d_all[k])) in msg, (conj, q, k, msg)
                swapped += 1
            if len(dd) >= 2 and s[0] == s[1] and signature_keys(coll, q, dd[:1])[0] == signature_keys(coll, q, dd[1:2])[0]:
                flipped = s.copy()
                flipped.view(np.uint32)[1] ^= 1
                assert same_signature_same_bits(ref, dd, flipped) is not None, (conj, q, k)
            if len(d_all) > k and ref.top64[k] < ref.top64[0] * (1 - 1e-4):
                worse = np.concatenate([dd[1:], d_all[k:k + 1]])
                assert nothing_better_left_out(ref, worse, k) is not None, (conj, q, k)
    assert swapped >= 50, swapped


def test_canonical_order_agrees_with_the_reference_summary(coll, queries):
    """TieRef keeps the smallest doc-ids of a signature only: its float64 order names the same documents as the whole result set's"""
    from topk_docs_ref import doc_scores64, scored_docs
    for q in _some(queries, 9):
        for conj in (True, False):
            ref = TieRef(coll, q, conj)
            docs, _ = scored_docs(coll, q, conj)
            assert ref.n == len(docs)
            s64 = doc_scores64(coll, q, docs)
            _, want = canonical_topk(docs, s64, 1025)
            assert np.array_equal(ref.docs[ref.by_score[:1025]], want), (q, conj)
            assert np.array_equal(ref.top64, np.sort(s64)[::-1][:1025]), (q, conj)


def test_oracle_ranked_and_is_the_brute_force_bit_for_bit(coll, queries, capsys):
    """the share of ranked_and rows whose score bits are the float32 brute force's: the GPU test compares ids exactly on those rows and
    requires the same share of the kernels"""
    oidx = o.Index("block_optpfor", coll.index_image("block_optpfor"), coll.wand_image())
    qs = [q for q in queries if q]
    rows = equal = 0
    for k in (10, 1024):
        _, topk, tlen, _, _ = oidx.query_batch("ranked_and", qs, k=k)
        for i, q in enumerate(qs):
            s, _ = brute_pairs(coll, q, k, True, order="size")
            assert int(tlen[i]) == len(s), (q, k)
            if len(s):
                rows += 1
                equal += np.array_equal(np.ascontiguousarray(topk[i, :len(s)]).view(np.uint32), s.view(np.uint32))
    oidx.close()
    with capsys.disabled():
        print("\noracle ranked_and rows bit-equal to the float32 brute force: %d of %d (%.1f %%)" % (equal, rows, 100.0 * equal / rows))
    assert equal >= BIT_EQUAL_SHARE * rows, (equal, rows)
