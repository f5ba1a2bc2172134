"""tests/batch_size_cases.py is what it claims (no GPU): the collection's three kinds of lists, the distinct queries' shapes, the oracle
and the brute force agreeing on every distinct query, the table of sizes around every threshold, the special queries on both sides of
every planning-chunk boundary, and the three conditions LARGE is built for -- from the inputs alone."""
import numpy as np

import batch_size_cases as bc
from test_gpu_topk_docs import _bits


def test_collection():
    coll = bc.collection()
    assert coll.num_docs == bc.NUM_DOCS and [len(dd) for dd, _ in coll.lists] == bc.SIZES_OF_LISTS and len(coll.lists) == 24
    for t in bc.SPARSE:
        assert 3 <= len(coll.lists[t][0]) and not bc.has_bitmap(len(coll.lists[t][0]))
    for t in bc.DENSE:
        assert bc.has_bitmap(len(coll.lists[t][0])) and bc.NUM_DOCS // 64 <= len(coll.lists[t][0]) <= 4200
    for t in bc.LONG:
        assert 20000 <= len(coll.lists[t][0]) <= 60000 and 160 <= (len(coll.lists[t][0]) + 127) // 128 <= 470
    assert not bc.has_bitmap(2047) and bc.has_bitmap(2048)  # (the edge itself is among the lists)


def test_distinct_queries():
    qs = bc.distinct_queries()
    assert 140 <= len(qs) <= 160 and qs[0] == []
    nd = [len(set(q)) for q in qs]
    assert set(range(0, 17)) <= set(nd) and sum(n > 16 for n in nd) == 2
    assert all([t] in qs for t in range(24))
    assert sum(len(q) > len(set(q)) for q in qs) >= 5  # duplicated terms
    dense = set(bc.DENSE)
    assert {len(q) for q in qs if q and set(q) <= dense and len(set(q)) == len(q)} >= {1, 2, 3, 4}  # all dense
    mixed = [q for q in qs if 2 <= len(set(q)) <= 4 and set(q) & dense and set(q) & set(bc.SPARSE)]
    assert {len(set(q)) for q in mixed} == {2, 3, 4}
    # the two kinds of mixed query: a list stream for `and` but not for and_freq, and units for both
    assert any(bc.stream_records(q, "and") == 1 and bc.stream_records(q, "and_freq") == 0 for q in mixed)
    assert any(bc.stream_records(q, "and") == 0 for q in mixed)
    assert sum(bool(set(q) & set(bc.LONG)) for q in qs) >= 20  # over the long lists
    assert bc.stream_records(bc.D4, "and_freq") == 4 and bc.stream_records(bc.D4, "and") == 1
    assert bc.stream_records([], "and") == 0 and bc.stream_records(bc.OVER16, "and_freq") == 0 and bc.stream_records(bc.DUP[:1] * 2, "and") == 1


def test_oracle_and_brute_force_agree():
    coll, qs, ref = bc.collection(), bc.distinct_queries(), bc.reference()
    for op in ("and", "and_freq", "or", "or_freq"):
        count, fsum = ref["oracle_unranked"][op]
        assert np.array_equal(count, ref[op[:3].rstrip("_")]), op
        if op.endswith("freq"):
            assert np.array_equal(fsum, ref[op]), op
    for k in bc.KS["ranked_and"]:
        count, topk, tlen = ref[("ranked_and", k)]
        assert np.array_equal(count, np.minimum(ref["and"], k))  # (a ranked operator's count is its top-k's length)
        for i, q in enumerate(qs):
            bs, bd = ref["brute"][i]
            n = min(k, len(bd))
            assert n == tlen[i] == min(k, len(ref["and_docs"][i])), (k, q)
            assert np.array_equal(_bits(bs[:n]), _bits(topk[i, :n])), (k, q)  # the oracle and the brute force agree
            assert np.all(np.isneginf(topk[i, n:])), (k, q)
        assert np.array_equal(bc.brute_docs(k)[:, :1] != 0xFFFFFFFF, (tlen > 0)[:, None])
    for op in bc.UNION:  # the union operators: the oracle's three agree on the lengths, and with the size of the union
        for k in bc.KS[op]:
            _, topk, tlen = ref[(op, k)]
            assert np.array_equal(tlen, np.minimum(ref["or"], k)), (op, k)
            np.testing.assert_allclose(topk, ref[("wand", k)][1], rtol=1e-5)
    _, _, tlen = ref[("ranked_and", 10)]
    assert np.any((tlen > 0) & (tlen < 10)) and np.any(tlen == 10) and np.any(tlen == 0)
    assert sum(1 for i, q in enumerate(qs) if len(set(q)) >= 5 and tlen[i] == 10) >= 10  # (the common core: many-list conjunctions are not empty)


def test_sizes_straddle_every_threshold():
    assert bc.SIZES == sorted(set(bc.SIZES)) and bc.SIZES[0] == 0 and bc.SIZES[-1] == bc.LARGE == 36000
    for t in bc.THRESHOLDS:
        assert {t - 1, t, t + 1} <= set(bc.SIZES), t
    assert bc.LARGE > bc.SLICE


def test_batches_are_seeded_picks():
    qs = bc.distinct_queries()
    for nq in bc.SIZES:
        pick, queries, (terms, offs) = bc.batch(nq)
        assert len(pick) == len(queries) == nq == len(offs) - 1
        assert all(queries[i] == qs[pick[i]] for i in range(0, nq, max(1, nq // 97)))
        assert offs[-1] == sum(len(q) for q in queries) and (nq == 0 or terms[:offs[-1]].tolist() == [t for q in queries for t in q])
    assert len(set(bc.pick_of(4097).tolist())) == len(qs)  # a batch of that size holds every distinct query


def test_special_queries_sit_on_both_sides_of_every_chunk_boundary():
    qs = bc.distinct_queries()
    kinds = {"empty": lambda q: not q, "over16": lambda q: len(set(q)) > 16, "dup": lambda q: len(q) > len(set(q)) and len(set(q)) <= 16}
    for nq in bc.CHUNKED_SIZES:
        pick = bc.pick_of(nq)
        seen = set()
        for nchunks in bc.CHUNKINGS:
            for c in range(1, nchunks):
                b = nq * c // nchunks
                for side, p in ((0, b - 1), (1, b)):
                    q = qs[pick[p]]
                    name = [n for n, f in kinds.items() if f(q)]
                    assert len(name) == 1, (nq, nchunks, c, side, q)  # every such position holds one of the three
                    seen.add((name[0], side))
                assert qs[pick[b - 1]] != qs[pick[b]], (nq, nchunks, c)
        assert seen == {(n, s) for n in kinds for s in (0, 1)}, (nq, sorted(seen))  # each kind ends a chunk somewhere and starts one
    for nq in (1, 1023, 1025, 4097):
        assert not any(len(set(q)) > 16 for q in bc.batch(nq, "none")[1])
        last = bc.batch(nq, "last")[1]
        assert [i for i, q in enumerate(last) if len(set(q)) > 16] == [nq - 1]


def test_large_passes_the_slice_inside_a_query():
    cond = bc.large_conditions()
    total, i, before, after, q = cond["or_freq"]
    assert total >= 34000 and before < bc.SLICE < after and len(set(q)) >= 3, cond["or_freq"]
    total, j, before, after, q = cond["and_freq"]
    assert total > bc.SLICE and before < bc.SLICE < after, cond["and_freq"]
    assert len(set(q)) in (3, 4) and all(bc.has_bitmap(bc.SIZES_OF_LISTS[t]) for t in q), cond["and_freq"]
    assert j > i
    total, _, _, _, _ = cond["and"]
    assert total > bc.SLICE, cond["and"]
    # most of LARGE's queries are one-term or all-dense, and the others are all there: units beside the streams
    qs, pick = bc.distinct_queries(), bc.pick_of(bc.LARGE)
    assert len(set(pick.tolist())) == len(qs)
    assert sum(bc.stream_records(qs[p], "and") for p in pick) == total
