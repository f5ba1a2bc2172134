"""The 3-4-list stream kernel (k_ranked_stream<4>, ranked_stream.hip) after its footprint was cut (-m gpu): values that used to
sit in registers across stage C now wait in lanes of `cold` or in LDS areas that are dead at that moment, and stage C's staging
block shares its bytes with list 1's gathered bytes. A slip there shows where a block is exactly full, a list ends inside a unit,
a survivor walks every further list, or a unit starts in the middle of a query -- so this collection is built around those:

  lists of 127 / 128 / 129 postings (no bitmap: fewer than num_docs / 64) and of 300 (a partial last block), one of exactly five
  blocks, three of 20 and more blocks (the shortest lists of the queries that get cut), a dense one (every even document), one that lives in the first seventh of the collection (as list 1
  it ends the unit: `finished`), and a core of documents common to all of them (their survivors visit every further list).

Every 3- and 4-list query (a one-term and two 2-list queries ride in the same batch) runs as ranked_and with k = 1, 10, 64 and 65
(65: the four-scores-per-lane build), with and without DS2I_OP_TOPK_DOCS, with and without counters, and as and / and_freq; whole,
and cut into parts of at most eight blocks (DS2I_UNIT_CAP=8); with and without the dense lists' bitmaps. The answer is the class
kernel's (k_conjunctive, DS2I_NO_RANKED_STREAM) bit for bit, and the oracle's within 1e-5."""
import numpy as np
import pytest

import ds2i_amd as d
import oracle as o
from helpers import Collection

pytestmark = pytest.mark.gpu
N = 10000
KS = (1, 10, 64, 65)
CLASS_KERNEL = ("DS2I_NO_RANKED_STREAM",)
STREAM_UPLOADS = [(), ("DS2I_UNIT_CAP=8",), ("DS2I_NO_BITMAPS",), ("DS2I_NO_BITMAPS", "DS2I_UNIT_CAP=8")]
T_DENSE, T127, T128, T129, T300, T640, T700, T_LOW, T1000, T2500, T3000, T4000 = range(12)


def _collection():
    rng = np.random.default_rng(0x45F17)
    core = np.unique(np.concatenate([[0, 1, N - 2], rng.choice(np.arange(2, N - 2, 2), 37, replace=False)]))  # 40 documents, in every list

    def lst(n, pool):
        rest = np.setdiff1d(pool, core)
        docs = np.sort(np.concatenate([core[np.isin(core, pool)], rng.choice(rest, n - int(np.isin(core, pool).sum()), replace=False)]))
        assert len(docs) == n
        return docs, rng.integers(1, 9, n).astype(np.uint32)

    everything = np.arange(N)
    dense = np.union1d(np.arange(0, N, 2), core)
    lists = [(dense, rng.integers(1, 9, len(dense)).astype(np.uint32))]
    lists += [lst(n, everything) for n in (127, 128, 129, 300, 640, 700)]
    lists.append(lst(200, np.arange(0, N // 7)))  # T_LOW: nothing beyond the first seventh
    lists += [lst(n, everything) for n in (1000, 2500, 3000, 4000)]  # (2500 and more: the shortest list of a query that DS2I_UNIT_CAP=8 cuts)
    return Collection.from_lists(N, lists, rng.integers(20, 400, N).astype(np.uint32))


def _queries():
    rng = np.random.default_rng(0x45F18)
    three = [[T127, T128, T129], [T127, T300, T_DENSE], [T128, T640, T1000], [T129, T700, T_DENSE], [T300, T640, T700], [T127, T_LOW, T_DENSE],
             [T640, T700, T1000], [T128, T_LOW, T1000], [T640, T_DENSE, T1000], [T300, T_LOW, T640], [T2500, T3000, T_DENSE], [T2500, T4000, T3000]]
    four = [[T127, T128, T129, T300], [T127, T300, T640, T_DENSE], [T128, T640, T700, T1000], [T300, T640, T700, T_DENSE], [T127, T_LOW, T_DENSE, T1000],
            [T640, T700, T1000, T_DENSE], [T129, T_LOW, T640, T700], [T127, T128, T129, T_DENSE], [T300, T_LOW, T700, T1000], [T2500, T3000, T4000, T_DENSE],
            [T3000, T_LOW, T4000, T_DENSE]]
    some = [sorted(int(t) for t in rng.choice(12, n, replace=False)) for n in (3, 4) for _ in range(8)]
    return three + four + some + [[T300], [T127, T_DENSE], [T640, T700]]


class Env:
    def __init__(self):
        self.coll = _collection()
        self.qs = _queries()
        self.image, self.wand = self.coll.index_image("block_optpfor"), self.coll.wand_image()
        self.oracle = o.Index("block_optpfor", self.image, self.wand)
        self.idx, self.ref = {}, {}

    def index(self, knobs):
        if knobs not in self.idx:
            try:
                for kn in knobs:
                    name, _, val = kn.partition("=")
                    d.set_option(name, val or "1")
                self.idx[knobs] = d.Index("block_optpfor", self.image, self.wand)
            finally:
                for kn in knobs:
                    d.set_option(kn.partition("=")[0], None)
        return self.idx[knobs]

    def run(self, knobs, op, k, with_docs=False, instrumented=True):
        """-> (count, topk, tlen, fsum, docs or None, launch groups)"""
        b = d.Batch(self.index(knobs), op, self.qs, k=k, with_docs=with_docs)
        b.set_instrumented(instrumented)
        b.run()
        out = b.fetch() + (b.fetch_topk_docs() if with_docs else None, [g for c in range(4) for g in b.class_groups(c)])
        b.close()
        return out

    def reference(self, op, k):
        """the class kernel's answer, checked against the oracle once (computed once, shared, never changed)"""
        if (op, k) not in self.ref:
            count, topk, tlen, fsum, docs, groups = self.run(CLASS_KERNEL, op, k, with_docs=op == "ranked_and")
            assert not any(g["pipelined_stream"] for g in groups)
            oc, otopk, otlen, ofsum, _ = self.oracle.query_batch(op, self.qs, k=k)
            assert np.array_equal(count, oc) and np.array_equal(tlen, otlen), (op, k)
            if op == "and_freq":
                assert np.array_equal(fsum, ofsum)
            if op == "ranked_and":
                for i in range(len(self.qs)):
                    np.testing.assert_allclose(topk[i, :tlen[i]], otopk[i, :tlen[i]], rtol=1e-5, err_msg=str((k, self.qs[i])))
            for a in (count, topk, tlen, fsum, docs):
                if a is not None:
                    a.setflags(write=False)
            self.ref[(op, k)] = (count, topk, tlen, fsum, docs)
        return self.ref[(op, k)]

    def close(self):
        for g in self.idx.values():
            g.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _streamed(groups, knobs, ranked):
    g4 = [g for g in groups if g["lists"] == 4]
    assert g4 and all(g["pipelined_stream"] for g in g4), groups
    if ranked and any(kn.startswith("DS2I_UNIT_CAP") for kn in knobs):  # (the knob cuts ranked conjunctions only)
        assert sum(g["units"] for g in g4) > sum(g["queries"] for g in g4), groups


def test_collection_has_the_cases(env):
    """the shapes the module is about are really there: intersections through every list, a list that ends early, block edges"""
    c, qs = env.coll, env.qs
    assert [len(c.lists[t][0]) for t in (T127, T128, T129, T300, T640)] == [127, 128, 129, 300, 640]
    assert len(c.lists[T129][0]) * 64 < N <= len(c.lists[T300][0]) * 64  # no bitmap | bitmap
    assert int(c.lists[T_LOW][0][-1]) < N // 7 < int(c.lists[T127][0][-1])
    count = env.reference("and", 10)[0]
    n34 = [i for i, q in enumerate(qs) if len(q) in (3, 4)]
    assert len(n34) >= 30 and all(count[i] >= 2 for i in n34)  # (documents 0 and 1 at the least)
    assert any(len(q) == 1 for q in qs) and any(len(q) == 2 for q in qs)


@pytest.mark.parametrize("knobs", STREAM_UPLOADS, ids=lambda kn: "+".join(kn) or "default")
@pytest.mark.parametrize("k", KS)
def test_ranked_and_bit_identical_to_class_kernel(env, knobs, k):
    rc, rtopk, rtlen, _, rdocs = env.reference("ranked_and", k)
    for with_docs in (False, True):
        for instrumented in (True, False) if not with_docs else (False,):  # (the docs kernels carry no counters)
            count, topk, tlen, _, docs, groups = env.run(knobs, "ranked_and", k, with_docs, instrumented)
            where = (knobs, k, with_docs, instrumented)
            _streamed(groups, knobs, True)
            assert np.array_equal(count, rc) and np.array_equal(tlen, rtlen), where
            bad = np.argwhere(_bits(topk) != _bits(rtopk))
            assert len(bad) == 0, (where, [env.qs[i] for i in np.unique(bad[:, 0])[:4]])
            if with_docs:
                assert np.array_equal(docs, rdocs), where


@pytest.mark.parametrize("knobs", STREAM_UPLOADS, ids=lambda kn: "+".join(kn) or "default")
@pytest.mark.parametrize("op", ["and", "and_freq"])
def test_and_counts_and_freq_sums(env, knobs, op):
    rc, _, _, rfsum, _ = env.reference(op, 10)
    for instrumented in (True, False):
        count, _, _, fsum, _, groups = env.run(knobs, op, 10, False, instrumented)
        _streamed(groups, knobs, False)
        assert np.array_equal(count, rc), (knobs, op, instrumented, np.argwhere(count != rc)[:4])
        if op == "and_freq":
            assert np.array_equal(fsum, rfsum), (knobs, instrumented)
