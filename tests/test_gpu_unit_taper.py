"""Tapering work units of ranked_and (-m gpu): cut_units cuts a split query of a large batch into a few large parts and then small ones
(ds2i_amd/csrc/unit_cut.hpp) instead of equal parts. The answer must not depend on the cut.

Collection: 2^17 documents, 12 lists of 8 k .. 64 k postings (64 .. 512 blocks). Queries of 2, 3, 4, 6, 8 and 9 lists whose shortest list
has at least 18 k postings, some with fewer than k matches (the many-list ones), some with matches in every part (the densest lists),
repeated to 1600 queries: tapering applies from 1536 queries on. DS2I_UNIT_FACTOR=1000000 puts every class's target at its floor (256,
48 for 9-16 lists), where a query's part count no longer depends on the batch -- so the same queries in two batches of 800 show what the
equal cut gives at the same factor.

ranked_and is compared bit for bit with the oracle (scores, lengths, counts) and with the float32 brute force (doc-ids), at k = 10 and
k = 100, as a one-shot batch, a prepared batch and through a depth-3 pipeline, and once more with DS2I_UNIT_CAP=8 (where the unit count
must be at least the sum of ceil(blocks / 8): the knob bounds every unit, tapering or not); wand and `and` are the bits of an index
uploaded without the knobs. The empty query is in every batch: at k = 100 it gets no unit, and its row must still be the empty answer
(count 0, length 0, scores -inf, doc-ids 0xFFFFFFFF) however the results leave the library."""
import itertools

import numpy as np
import pytest

import ds2i_amd as d
import oracle as o
from helpers import Collection
from test_gpu_topk_docs import Env, _bits
from topk_docs_ref import brute_pairs

pytestmark = pytest.mark.gpu
NUM_DOCS = 1 << 17
# (list sizes at which numpy's float32 log gives the oracle's query weights bit for bit -- the fixture asserts it: at 52000 it is 1 ulp off)
SIZES = [8192, 11000, 14000, 18000, 23000, 28000, 34000, 40000, 46000, 51000, 58000, 65536]
CAPACITIES = {2, 4, 6, 8, 16}
FACTOR = "DS2I_UNIT_FACTOR=1000000"
NQ = 1600  # (tapering: batches of 1536 queries and more)
KS = (10, 100)


def _collection():
    rng = np.random.default_rng(0x7A9E2)
    lists = []
    for n in SIZES:
        docs = np.sort(rng.choice(NUM_DOCS, n, replace=False)).astype(np.uint32)
        lists.append((docs, rng.integers(1, 9, n).astype(np.uint32)))
    return Collection.from_lists(NUM_DOCS, lists, rng.integers(50, 500, NUM_DOCS))


def _distinct_queries():
    """every query's shortest list is list 3 (18 k postings, 141 blocks) or longer: at the floor targets each is cut into 4 parts and more"""
    qs = [[a, b] for a, b in itertools.combinations(range(6, 12), 2)]                # 2 lists; [10, 11]: 29 k matches, some in every part
    qs += [[6, 8, 11], [7, 9, 10], [9, 10, 11], [6, 7, 8]]                            # 3
    qs += [[6, 7, 9, 11], [8, 9, 10, 11], [6, 8, 10, 11]]                             # 4
    qs += [[6, 7, 8, 9, 10, 11], [4, 6, 7, 9, 10, 11], [5, 6, 8, 9, 10, 11]]          # 6
    qs += [[4, 5, 6, 7, 8, 9, 10, 11], [3, 5, 6, 7, 8, 9, 10, 11]]                    # 8
    qs += [[3, 4, 5, 6, 7, 8, 9, 10, 11], [3, 4, 5, 6, 7, 8, 9, 10, 11, 11]]          # 9 (a repeated term: its query weight counts twice)
    qs += [[]]  # the empty query: at k > 64 it has no unit, and its row is the empty answer padded like every other row
    return qs


@pytest.fixture(scope="module")
def env():
    e = Env(_collection())
    e.distinct = _distinct_queries()
    e.pick = np.arange(NQ) % len(e.distinct)
    e.queries = [e.distinct[i] for i in e.pick]
    e.images["block_optpfor"] = e.coll.index_image("block_optpfor")
    oidx = o.Index("block_optpfor", e.images["block_optpfor"], e.wand)
    e.ref = {}
    for k in KS:
        count, topk, tlen, _, _ = oidx.query_batch("ranked_and", e.distinct, k=k)
        docs = np.full((len(e.distinct), k), 0xFFFFFFFF, dtype=np.uint32)
        for i, q in enumerate(e.distinct):
            bs, bd = brute_pairs(e.coll, q, k, True)
            assert len(bd) == tlen[i] and np.array_equal(_bits(bs), _bits(topk[i, :len(bd)])), (k, q)  # the oracle and the brute force agree
            docs[i, :len(bd)] = bd
        e.ref[k] = (count.copy(), topk.copy(), tlen.copy(), docs)
    e.ref_and = oidx.query_batch("and", e.distinct)[0].copy()
    oidx.close()
    yield e
    e.close()


def _check(e, k, count, topk, tlen, docs=None, where=""):
    rc, rt, rl, rd = e.ref[k]
    assert np.array_equal(count, rc[e.pick]), where
    assert np.array_equal(tlen, rl[e.pick]), where
    live = np.arange(k)[None, :] < rl[e.pick][:, None]
    assert np.array_equal(_bits(topk)[live], _bits(rt[e.pick])[live]), where
    assert np.all(np.isneginf(topk[~live])), where  # (a row no kernel wrote included: the empty query)
    if docs is not None:
        assert np.array_equal(docs, rd[e.pick]), where


def _groups(b):
    return [g for c in range(5) for g in b.class_groups(c)]


def _units(groups):
    return sum(g["units"] for g in groups)


def test_the_collection_is_what_the_cases_need(env):
    _, _, tlen10, _ = env.ref[10]
    _, _, tlen100, _ = env.ref[100]
    assert np.any((tlen10 < 10) & (tlen10 > 0)) and np.any((tlen100 < 100) & (tlen100 > 0)) and np.any(tlen100 == 100)
    assert sorted({len(set(q)) for q in env.distinct}) == [0, 2, 3, 4, 6, 8, 9]
    a, b = env.coll.lists[10][0], env.coll.lists[11][0]
    both = np.intersect1d(a, b)
    blocks = np.searchsorted(a, both) // 128  # blocks of the shorter list with a match
    assert len(np.unique(blocks)) == (len(a) + 127) // 128  # ... all of them: every part of [10, 11] holds matches


@pytest.mark.parametrize("knobs", [(FACTOR,), (FACTOR, "DS2I_UNIT_CAP=8")], ids=["factor", "factor+cap8"])
def test_ranked_and_does_not_depend_on_the_cut(env, knobs):
    g = env.index("block_optpfor", knobs)
    for k in KS:
        count, topk, tlen, _ = g.query_batch("ranked_and", env.queries, k)
        _check(env, k, count, topk, tlen, where=("one-shot", k, knobs))
        count, topk, docs, tlen, _ = g.query_batch_docs("ranked_and", env.queries, k)
        _check(env, k, count, topk, tlen, docs, where=("one-shot with docs", k, knobs))
        for with_docs in (False, True):
            b = d.Batch(g, "ranked_and", env.queries, k=k, with_docs=with_docs)
            b.run()
            count, topk, tlen, _ = b.fetch()
            _check(env, k, count, topk, tlen, b.fetch_topk_docs() if with_docs else None, where=("prepared", k, with_docs, knobs))
            groups = _groups(b)
            b.close()
            assert _units(groups) > NQ, (k, knobs)
            if len(knobs) > 1:  # DS2I_UNIT_CAP=8: no unit holds more than 8 blocks of its query's shortest list, tapering or not
                nb0 = [(min(len(env.coll.lists[t][0]) for t in q) + 127) // 128 for q in env.queries if q]
                assert _units(groups) >= sum((n + 7) // 8 for n in nb0), (k, knobs)
            assert {gr["lists"] for gr in groups if gr["pipelined_stream"]} == CAPACITIES, (k, knobs, groups)
        pipe = d.Pipeline(g, depth=3)
        tickets = [pipe.submit("ranked_and", env.queries, k=k, with_docs=i == 1) for i in range(3)]
        for i, t in enumerate(tickets):
            if i == 1:
                count, topk, docs, tlen = pipe.wait_docs(t)
            else:
                (count, topk, tlen), docs = pipe.wait(t), None
            _check(env, k, count, topk, tlen, docs, where=("pipeline", k, i, knobs))
        pipe.close()


def test_tapering_splits_and_makes_fewer_units_than_the_equal_cut(env):
    """at least 4 parts per query, fewer than the equal cut of the same queries at the same factor (two batches of 800: below 1536 queries
    the cut is equal, and at the floor targets a query's part count does not depend on its batch)"""
    g = env.index("block_optpfor", (FACTOR,))
    for k in KS:
        units = {}
        for name, batches in (("taper", [env.queries]), ("equal", [env.queries[:NQ // 2], env.queries[NQ // 2:]])):
            units[name] = {}
            for qs in batches:
                b = d.Batch(g, "ranked_and", qs, k=k)
                b.run()
                for gr in _groups(b):
                    if not gr["pipelined_stream"]:  # (k <= 64: the empty query's unit runs the class kernel)
                        continue
                    assert gr["lists"] in CAPACITIES, gr
                    u = units[name].setdefault(gr["lists"], [0, 0])
                    u[0] += gr["units"]
                    u[1] += gr["queries"]
                b.close()
        print("k = %d: units / queries per list capacity: tapering %s, equal %s" % (k, units["taper"], units["equal"]))
        assert set(units["taper"]) == set(units["equal"]) == CAPACITIES
        for cap in CAPACITIES:
            (tu, tq), (eu, eq) = units["taper"][cap], units["equal"][cap]
            assert tq == eq and tu >= 4 * tq and tu > tq, (k, cap, tu, tq)
            assert tu < eu, (k, cap, tu, eu)


@pytest.mark.parametrize("op", ["wand", "and"])
def test_other_operators_are_unchanged(env, op):
    g0, g = env.index("block_optpfor"), env.index("block_optpfor", (FACTOR,))
    c0, t0, l0, _ = g0.query_batch(op, env.queries, 10)
    c1, t1, l1, _ = g.query_batch(op, env.queries, 10)
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1) and np.array_equal(_bits(t0), _bits(t1)), op
    if op == "and":
        assert np.array_equal(c1, env.ref_and[env.pick])
