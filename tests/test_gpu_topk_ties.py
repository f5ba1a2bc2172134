"""The tie rule of DS2I_OP_TOPK_DOCS where ties are the norm (-m gpu): helpers.tie_collection has a few dozen distinct scores per
query, 2^24 + 2^18 documents and lists of up to 2 M postings, so almost every k-th place is tied, the tied documents sit in different
blocks, units and partial heaps of a split query, and most rows hold doc-ids past 2^24.

Every row is held to three exact checks that need no model of a kernel's arithmetic (topk_docs_ref: same_signature_same_bits,
closed_within_signature -- the k-th-place rule at every rank --, nothing_better_left_out); ranked_and rows whose score bits are the float32
brute force's are compared with its ids exactly, and at least 90 % of the non-empty rows must be such rows (tests/test_topk_ties_cpu.py
shows the oracle meets that share). A failure names (operator, upload, k, query), the rank and the two doc-ids. One exception: the reference's
wand and maxscore traversals (k_daat / k_daat_long: reference order, more than 16 terms, k > 64 off block_optpfor) add a document's terms in
the order the lists stand in, so a signature does not fix the last bit there; those rows keep the order rule, the lengths and the float64 checks.

The coverage the file relies on is asserted, not assumed: per operator family and k <= 300, at least half of the rows with more than k
results are tied at the k-th place and at least a quarter hold an id >= 2^24; the default planner splits the batch and runs every list
capacity 2 | 4 | 6 | 8 | 16."""
import numpy as np
import pytest

import ds2i_amd as d
from helpers import TIE_EDGE, tie_collection, tie_queries
from test_gpu_topk_docs import Env, _bits, _order, _structure, run_pair
from topk_docs_ref import TieRef, brute_pairs, closed_within_signature, nothing_better_left_out, same_signature_same_bits

pytestmark = pytest.mark.gpu
UNION = ["wand", "maxscore", "ranked_or"]
KS = [1, 10, 64, 65, 256, 257, 1024]
CAPACITIES = {2, 4, 6, 8, 16}
BIT_EQUAL_SHARE = 0.9
# the uploads beside block_optpfor (the stream kernels): the class kernels, opt transcoded and native, block_mixed native
OTHER_UPLOADS = [("block_qmx", None), ("opt", None), ("opt", "DS2I_PEF_NATIVE"), ("block_mixed", "DS2I_MIXED_NATIVE")]


@pytest.fixture(scope="module")
def tie():
    e = Env(tie_collection())
    qs = tie_queries(e.coll)
    e.queries = [q for q in qs if len(set(q)) <= 16]
    e.long_queries = [q for q in qs if len(set(q)) > 16]
    e.subset = e.queries[::3]  # (the empty query, every family of tie_queries and every list capacity are in it)
    # for the uploads that answer k > 64 one document at a time (a wave walks every posting of a ranked_or): no list beyond 2^17 postings
    e.thin = [q for q in e.queries if all(len(e.coll.lists[t][0]) <= 1 << 17 for t in q)][::2]
    e.refs, e.brute = {}, {}
    yield e
    e.close()


def _ref(env, q, conj):
    key = (tuple(q), conj)
    if key not in env.refs:
        env.refs[key] = TieRef(env.coll, q, conj)
    return env.refs[key]


def _brute(env, q):
    if tuple(q) not in env.brute:
        env.brute[tuple(q)] = brute_pairs(env.coll, q, 1024, True, order="size")
    return env.brute[tuple(q)]


class Coverage:
    """rows with more than k results, how many of them are tied at the k-th place and hold an id >= 2^24; ranked_and rows with a result
    and how many of them are the brute force's bits"""

    def __init__(self):
        self.rows, self.tied, self.high, self.nonempty, self.bit_equal = {}, {}, {}, 0, 0

    def add(self, k, ref, ids):
        if ref.n > k:
            self.rows[k] = self.rows.get(k, 0) + 1
            self.tied[k] = self.tied.get(k, 0) + bool(ref.tied_at(k))
            self.high[k] = self.high.get(k, 0) + bool(np.any(ids >= TIE_EDGE))

    def check(self, what, ks):
        print("\n%s: k: rows with > k results / tied at the k-th place / with an id >= 2^24: %s" % (
            what, ", ".join("%d: %d / %d / %d" % (k, self.rows[k], self.tied[k], self.high[k]) for k in ks)))
        for k in ks:
            if k <= 300:
                assert self.rows[k] >= 40, (what, k, self.rows[k])
                assert 2 * self.tied[k] >= self.rows[k], (what, k, self.tied[k], self.rows[k])
                assert 4 * self.high[k] >= self.rows[k], (what, k, self.high[k], self.rows[k])

    def check_bit_equal(self, what):
        print("%s: ranked_and rows bit-equal to the float32 brute force: %d of %d" % (what, self.bit_equal, self.nonempty))
        assert self.bit_equal >= BIT_EQUAL_SHARE * self.nonempty, (what, self.bit_equal, self.nonempty)


def check_rows(env, op, upload, k, qs, topk, docs, tlen, cov=None, signatures=True):
    """the three signature checks and the float64 scores of every row; ranked_and: the brute force's ids wherever the bits are its bits"""
    conj = op == "ranked_and"
    for i, q in enumerate(qs):
        ref = _ref(env, q, conj)
        n = int(tlen[i])
        ids, s = docs[i, :n], topk[i, :n]
        where = (op, upload, k, q)
        for msg in (nothing_better_left_out(ref, ids, k),) + ((same_signature_same_bits(ref, ids, s), closed_within_signature(ref, ids)) if signatures else ()):
            assert msg is None, where + (msg,)
        if n:
            np.testing.assert_allclose(ref.s64[ref.locate(ids)], s, rtol=1e-5, err_msg=str(where))
        if cov is not None:
            cov.add(k, ref, ids)
        if conj:
            bs, bd = _brute(env, q)
            assert n == min(k, len(bd)), where
            if n and cov is not None:
                cov.nonempty += 1
            if n and np.array_equal(_bits(s), _bits(bs[:n])):
                if cov is not None:
                    cov.bit_equal += 1
                if not np.array_equal(ids, bd[:n]):
                    r = int(np.flatnonzero(ids != bd[:n])[0])
                    raise AssertionError(where + ("rank %d: doc %d returned, the brute force has doc %d" % (r, int(ids[r]), int(bd[r])),))


def _batch(g, op, qs, k, **kw):
    """a prepared batch run twice -> (topk, docs, tlen, launch groups of the last run)"""
    b = d.Batch(g, op, qs, k=k, with_docs=True, **kw)
    out = []
    for _ in range(2):
        b.run()
        _, t, l, _ = b.fetch()
        out.append((t.copy(), b.fetch_topk_docs().copy(), l.copy()))
    groups = [gr for cls in range(5) for gr in b.class_groups(cls)]
    b.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]), (op, k)
    return out[1] + (groups,)


def _split_and_every_capacity(groups, nq, where):
    """the default planner cut queries into several units, and every list capacity of the stream kernels ran at least one query"""
    assert sum(gr["units"] for gr in groups) > nq, where
    ran = {gr["lists"] for gr in groups if gr["pipelined_stream"] and gr["queries"] >= 1}
    assert CAPACITIES <= ran, (where, sorted(ran))


def test_ranked_and_on_the_stream_kernels(tie):
    """block_optpfor, default planner, every query, every k: one-shot and prepared batch"""
    g = tie.index("block_optpfor")
    qs, cov = tie.queries, Coverage()
    for k in KS:
        _, topk, docs, tlen = run_pair(g, "ranked_and", qs, k, tie.coll.num_docs)
        check_rows(tie, "ranked_and", "block_optpfor", k, qs, topk, docs, tlen, cov)
        t, dd, l, groups = _batch(g, "ranked_and", qs, k)
        assert np.array_equal(_bits(t), _bits(topk)) and np.array_equal(dd, docs) and np.array_equal(l, tlen), k
        _split_and_every_capacity(groups, len(qs), ("ranked_and", k))
    cov.check("ranked_and", KS)
    cov.check_bit_equal("block_optpfor")


def test_union_operators_on_the_stream_kernels(tie):
    """block_optpfor, default planner, every query, every k: wand, maxscore and ranked_or give the same ids and score bits"""
    g = tie.index("block_optpfor")
    qs, cov = tie.queries, Coverage()
    for k in KS:
        res = {op: run_pair(g, op, qs, k, tie.coll.num_docs) for op in UNION}
        _, topk, docs, tlen = res["wand"]
        for op in UNION[1:]:
            for i, q in enumerate(qs):
                assert np.array_equal(_bits(res[op][1][i]), _bits(topk[i])) and np.array_equal(res[op][2][i], docs[i]) \
                    and res[op][3][i] == tlen[i], (op, "block_optpfor", k, q)
        check_rows(tie, "wand", "block_optpfor", k, qs, topk, docs, tlen, cov)
        for op in UNION:
            t, dd, l, groups = _batch(g, op, qs, k)
            assert np.array_equal(_bits(t), _bits(topk)) and np.array_equal(dd, docs) and np.array_equal(l, tlen), (op, k)
            _split_and_every_capacity(groups, len(qs), (op, k))
    cov.check("wand = maxscore = ranked_or", KS)


@pytest.mark.parametrize("codec,knob", OTHER_UPLOADS)
def test_other_uploads(tie, codec, knob):
    """the class kernels and the native opt / block_mixed kernels, on the queries of tie.thin. Beyond k = 64 these uploads answer with
    k_daat_long, the reference's traversals one document at a time: its wand and maxscore add a document's terms in the order the lists
    stand in (kernels_daat.inc), so two documents of one signature may differ by one ulp there and those rows are held to the order
    rule (run_pair), the lengths and the float64 checks; every other row to the signature checks too. The scores with ids are the
    scores-only bits everywhere (run_pair): this file found that they were not for wand and maxscore beyond k = 64 (CHANGELOG)."""
    g = tie.index(codec, [knob] if knob else [])
    upload, qs, cov = codec + ("+" + knob if knob else ""), tie.thin, Coverage()
    by_signature = lambda op, k: codec == "opt" and not knob or k <= 64 or op in ("ranked_and", "ranked_or")  # (opt transcoded: the stream kernels)
    for k in KS:
        for op in ["ranked_and"] + UNION:
            _, topk, docs, tlen = run_pair(g, op, qs, k, tie.coll.num_docs)
            check_rows(tie, op, upload, k, qs, topk, docs, tlen, cov if op == "ranked_and" else None, signatures=by_signature(op, k))
    cov.check_bit_equal(upload)


def test_finely_split(tie):
    """DS2I_UNIT_CAP=8, DS2I_UT_BLOCKS=1: every query in as many units as its lists allow, the tied documents in different partial heaps"""
    g0 = tie.index("block_optpfor")
    g = tie.index("block_optpfor", ["DS2I_UNIT_CAP=8", "DS2I_UT_BLOCKS=1"])
    qs = tie.subset
    for k in (10, 65, 300):
        for op in ("ranked_and", "wand"):
            topk, docs, tlen, groups = _batch(g, op, qs, k)
            assert sum(gr["units"] for gr in groups) > 8 * len(qs), (op, k)
            _structure(docs, tlen, tie.coll.num_docs, k)
            _order(topk, docs, tlen)
            check_rows(tie, op, "block_optpfor+DS2I_UNIT_CAP=8+DS2I_UT_BLOCKS=1", k, qs, topk, docs, tlen)
            _, t0, d0, l0 = run_pair(g0, op, qs, k, tie.coll.num_docs)  # the default planner's answer: the ids do not depend on the cut
            assert np.array_equal(_bits(topk), _bits(t0)) and np.array_equal(docs, d0) and np.array_equal(tlen, l0), (op, k)


def test_every_form_gives_the_one_shot_ids(tie):
    """depth-3 pipeline with k and with_docs changing from slot to slot, and reference_order (the prepared batch run twice is in the
    stream-kernel tests above)"""
    g = tie.index("block_optpfor")
    qs = tie.subset
    ref = {(op, k): run_pair(g, op, qs, k, tie.coll.num_docs) for op in ("ranked_and", "wand") for k in (10, 65, 300)}
    p = d.Pipeline(g, depth=3)
    plan = [("ranked_and", 10, True), ("wand", 65, False), ("wand", 300, True), ("ranked_and", 65, True), ("ranked_and", 300, False),
            ("wand", 10, True), ("ranked_and", 300, True), ("wand", 65, True), ("ranked_and", 10, False)]
    inflight = []

    def collect(item):
        op, k, with_docs, t = item
        c0, t0, d0, l0 = ref[(op, k)]
        if with_docs:
            c, topk, dd, tlen = p.wait_docs(t)
            assert np.array_equal(dd, d0), (op, k)
        else:
            c, topk, tlen = p.wait(t)
        assert np.array_equal(_bits(topk), _bits(t0)) and np.array_equal(tlen, l0) and np.array_equal(c, c0), (op, k, with_docs)

    for op, k, with_docs in plan:
        inflight.append((op, k, with_docs, p.submit(op, qs, k=k, with_docs=with_docs)))
        if len(inflight) == 3:
            collect(inflight.pop(0))
    while inflight:
        collect(inflight.pop(0))
    p.close()
    for (op, k), (c0, t0, d0, l0) in ref.items():
        topk, docs, tlen, _ = _batch(g, op, qs, k, reference_order=True)
        _structure(docs, tlen, tie.coll.num_docs, k)
        _order(topk, docs, tlen)
        # The reference's wand sums a document's terms in the order its lists stand in at that moment (sorted by current doc-id, ties
        # as the traversal left them), so there two documents of one signature may differ in the last bit: measured on the MI355X,
        # query [0, 12, 11, 1, 4, 15] at k = 1024, 64 returned documents of one signature carry the bits 0x426fc0ba and 0x426fc0bb.
        # A signature does not fix the score in that traversal, and a document that the one-shot run returns may score one ulp
        # lower here and leave a row whose k returned scores are the same bits in both runs (seen at wand, k = 10). So its union rows
        # are held to the order rule, the lengths and the float64 checks; ranked_and to everything, the one-shot bits and ids included.
        check_rows(tie, op, "block_optpfor+reference_order", k, qs, topk, docs, tlen, signatures=op == "ranked_and")
        assert np.array_equal(tlen, l0), (op, k)
        if op == "ranked_and":
            assert np.array_equal(_bits(topk), _bits(t0)) and np.array_equal(docs, d0), (op, k)


def test_more_than_16_terms(tie):
    """k_daat_long (one unit per query, global scratch), with shorter queries in the same batch. Its wand and maxscore are the
    reference's traversals, which add a document's terms in the order the lists stand in (kernels_daat.inc): two documents of one
    signature may differ by one ulp there (seen: docs 16807785 and 16800625, bits 4349db10 and 4349db11), so those two operators are held
    to the order rule and the float64 checks; ranked_and and ranked_or, which add in list order, to the signature checks too."""
    g = tie.index("block_optpfor")
    qs = tie.long_queries + tie.thin[:12]  # (at k > 64 the whole union batch goes one document at a time)
    assert len(tie.long_queries) == 2
    for k in (10, 100):
        for op in ["ranked_and"] + UNION:
            _, topk, docs, tlen = run_pair(g, op, qs, k, tie.coll.num_docs)
            check_rows(tie, op, "block_optpfor", k, qs, topk, docs, tlen, signatures=op in ("ranked_and", "ranked_or"))
            # (check_rows holds the lengths to the result sets; here: the long queries have answers -- the first one's AND a few dozen
            # documents, the second one's, across the halves, none)
            assert tlen[0] >= 10 and (op == "ranked_and" or (tlen[0] == k and tlen[1] == k)), (op, k)
