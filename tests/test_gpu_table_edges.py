"""The membership hints, bitmaps and range tables at their edges (-m gpu): every upload kind and knob set that changes what the tables
hold or which kernel reads them, on the one crafted collection of tests/table_edge_cases.py -- a candidate on the alias of a lone
posting's hint code at shift 8, 9 and 10, on every byte and word edge of a bitmap, in the last, partial range, in ranges whose weights
round to less than one 255th of the list maximum, and with one doc-id per entry. tests/test_table_edges_cpu.py proves that the
collection holds those candidates in numbers (the census) and that the oracle answers its queries like numpy.

Every answer is compared with numpy (exact for counts, freq sums and doc-id lists; RTOL against the float64 top-k) and the ranked scores
with the oracle. A failure names the upload, the operator and the query; a wrong `and` list also the first differing document and what
it is to every list of the query (its census category)."""
import numpy as np
import pytest

import ds2i_amd as d
import oracle as o
import table_edge_cases as tc
from helpers import check_pruning_tables
from table_edge_cases import NAMES
from test_gpu_topk_docs import Env, _bits, run_pair
from topk_docs_ref import brute_pairs

pytestmark = pytest.mark.gpu
RTOL = 1e-5
UNION = ["wand", "maxscore", "ranked_or"]
KS_AND, KS_UNION = (1, 10, 64, 65), (10, 64)
NCLS = 5
UPLOADS = [("block_optpfor", ()), ("block_optpfor", ("DS2I_RMW_G=2",)), ("block_optpfor", ("DS2I_RMW_G=1",)), ("block_optpfor", ("DS2I_NO_RMH=1",)),
           ("block_optpfor", ("DS2I_NO_BITMAPS=1",)), ("block_optpfor", ("DS2I_NO_RANKED_STREAM=1",)), ("block_optpfor", ("DS2I_NO_UNION_RSTREAM=1",)),
           ("block_optpfor", ("DS2I_UNIT_CAP=8",)), ("opt", ("DS2I_PEF_NATIVE",)), ("block_mixed", ("DS2I_MIXED_NATIVE",)), ("block_qmx", ())]
IDS = ["+".join((c,) + k) for c, k in UPLOADS]


def _g_of(knobs):
    return {"DS2I_RMW_G=2": 2, "DS2I_RMW_G=1": 1}.get(knobs[0] if knobs else "", 4)


@pytest.fixture(scope="module")
def edge():
    e = Env(tc.collection())
    e.queries, e.ref = tc.queries(), tc.reference()
    oidx = o.Index("block_optpfor", e.coll.index_image("block_optpfor"), e.wand)
    e.oracle = {(op, k): oidx.query_batch(op, e.queries, k=k)[1:3] for op, ks in (("ranked_and", KS_AND), ("wand", KS_UNION), ("maxscore", KS_UNION),
                                                                                  ("ranked_or", KS_UNION)) for k in ks}
    oidx.close()
    e.brute = [brute_pairs(e.coll, q, max(KS_AND), True, order="size") for q in e.queries]
    yield e
    e.close()


def _name(q):
    return "[" + " ".join(NAMES[t] for t in q) + "]"


def _explain(coll, q, doc, G):
    """what `doc` is to every list the query probes"""
    ts = sorted(set(q), key=lambda t: (len(coll.lists[t][0]), t))
    return "; ".join(tc.category_of(coll, ts[0], t, G, doc) for t in ts[1:])


@pytest.mark.parametrize("codec,knobs", UPLOADS, ids=IDS)
def test_tables(edge, codec, knobs):
    """the shift of every list, and every assertion of test_gpu.py::test_pruning_tables_are_exact_maxima, on every list of the collection:
    the last entry of every level-1 table, the last bitmap byte and the tiny-weight-only ranges' non-zero bytes are among them"""
    g, G, up = edge.index(codec, knobs), _g_of(knobs), "+".join((codec,) + knobs)
    info = g.info()
    assert info["has_range_tables"] and info["range_table_entries_per_posting"] == G, up
    assert bool(info["has_membership_hints"]) == ("DS2I_NO_RMH=1" not in knobs) and bool(info["has_bitmaps"]) == ("DS2I_NO_BITMAPS=1" not in knobs), up
    coll = edge.coll
    for t, (docs, freqs) in enumerate(coll.lists):
        tab, sh, mx = g.range_table(t)
        assert sh == tc.expected_shift(len(docs), G), (up, NAMES[t], sh)
        assert len(tab) == (coll.num_docs >> sh) + 1, (up, NAMES[t])
    check_pruning_tables(g, coll, range(len(coll.lists)), codec, G=G, hints="DS2I_NO_RMH=1" not in knobs, bitmaps="DS2I_NO_BITMAPS=1" not in knobs, where=up)
    # said once more for the weight edge: every range of C that holds only postings below 1/255 of the list maximum has a non-zero byte
    from helpers import doc_term_weight
    docs, freqs = coll.lists[tc.HEAVY_ANCHOR]
    w = doc_term_weight(freqs, coll.norm_lens[docs])
    tab, sh, mx = g.range_table(tc.HEAVY_ANCHOR)
    rmax = np.zeros(len(tab), dtype=np.float32)
    np.maximum.at(rmax, docs >> sh, w)
    tiny = (rmax > 0) & (rmax < np.float32(mx) / np.float32(255.0))
    assert np.count_nonzero(tiny) >= 100 and np.all(tab[tiny] != 0), (up, np.count_nonzero(tiny))


@pytest.mark.parametrize("codec,knobs", UPLOADS, ids=IDS)
def test_unranked_operators(edge, codec, knobs):
    """and / and_freq: counts, freq sums and doc-id lists = numpy; or / or_freq: counts and sums = numpy"""
    g, G, up = edge.index(codec, knobs), _g_of(knobs), "+".join((codec,) + knobs)
    qs, ref = edge.queries, edge.ref
    for op in ("and", "and_freq"):
        for want in (True, False):  # (the doc-id lists first: a wrong list names its first wrong document)
            b = d.Batch(g, op, qs, want_matches=want)
            b.run()
            count, _, _, fsum = b.fetch()
            got = b.fetch_matches(count) if want else None
            b.close()
            for i, q in enumerate(qs):
                exp = ref[i]["and"]
                if want and not np.array_equal(got[i], exp):
                    extra, lost = np.setdiff1d(got[i], exp), np.setdiff1d(exp, got[i])
                    doc = int(min(list(extra[:1]) + list(lost[:1]))) if len(extra) + len(lost) else -1
                    raise AssertionError("%s %s %s: %d documents for %d; first difference: document %d %s -- %s" % (
                        up, op, _name(q), len(got[i]), len(exp), doc, "returned, not in the intersection" if doc in extra else "missing",
                        _explain(edge.coll, q, doc, G) if doc >= 0 and len(set(q)) > 1 else "order"))
                assert int(count[i]) == len(exp), "%s %s %s (want_matches=%s): count %d, numpy %d" % (up, op, _name(q), want, int(count[i]), len(exp))
                if op == "and_freq":
                    assert int(fsum[i]) == ref[i]["and_freq"], "%s %s %s: freq sum %d, numpy %d" % (up, op, _name(q), int(fsum[i]), ref[i]["and_freq"])
    for op in ("or", "or_freq"):
        count, _, _, _ = g.query_batch(op, qs)
        b = d.Batch(g, op, qs)
        b.run()
        bcount, _, _, fsum = b.fetch()
        b.close()
        for i, q in enumerate(qs):
            assert int(count[i]) == int(bcount[i]) == ref[i]["or"], "%s %s %s: count %d / %d, numpy %d" % (up, op, _name(q), int(count[i]), int(bcount[i]), ref[i]["or"])
            if op == "or_freq":
                assert int(fsum[i]) == ref[i]["or_freq"], "%s %s %s: freq sum %d, numpy %d" % (up, op, _name(q), int(fsum[i]), ref[i]["or_freq"])


@pytest.mark.parametrize("codec,knobs", UPLOADS, ids=IDS)
def test_ranked_and(edge, codec, knobs):
    """k = 1, 10, 64, 65: lengths exact, scores the oracle's bits and within RTOL of the float64 top-k; the ids the brute force's wherever
    the score bits are its bits"""
    g, up = edge.index(codec, knobs), "+".join((codec,) + knobs)
    qs, ref = edge.queries, edge.ref
    for k in KS_AND:
        _, topk, docs, tlen = run_pair(g, "ranked_and", qs, k, edge.coll.num_docs)
        otopk, otlen = edge.oracle[("ranked_and", k)]
        for i, q in enumerate(qs):
            where = "%s ranked_and k = %d %s" % (up, k, _name(q))
            want = ref[i]["top_and"][:k]
            n = int(tlen[i])
            assert n == len(want) == int(otlen[i]), "%s: %d scores, numpy %d" % (where, n, len(want))
            np.testing.assert_allclose(topk[i, :n], want, rtol=RTOL, err_msg=where)
            assert np.array_equal(_bits(topk[i, :n]), _bits(otopk[i, :n])), "%s: not the oracle's bits: %s / %s" % (where, topk[i, :n][:4], otopk[i, :n][:4])
            bs, bd = edge.brute[i]
            if np.array_equal(_bits(topk[i, :n]), _bits(bs[:n])):
                assert np.array_equal(docs[i, :n], bd[:n]), "%s: ids %s, brute force %s" % (where, docs[i, :n][:8], bd[:n][:8])


@pytest.mark.parametrize("codec,knobs", UPLOADS, ids=IDS)
def test_union_operators(edge, codec, knobs):
    """wand, maxscore, ranked_or at k = 10 and 64: lengths exact, within RTOL of the oracle and of the float64 top-k, the three bit-identical"""
    g, up = edge.index(codec, knobs), "+".join((codec,) + knobs)
    qs, ref = edge.queries, edge.ref
    for k in KS_UNION:
        res = {op: g.query_batch(op, qs, k) for op in UNION}
        for op in UNION:
            _, topk, tlen, _ = res[op]
            otopk, otlen = edge.oracle[(op, k)]
            for i, q in enumerate(qs):
                where = "%s %s k = %d %s" % (up, op, k, _name(q))
                want = ref[i]["top_or"][:k]
                n = int(tlen[i])
                assert n == len(want) == int(otlen[i]), "%s: %d scores, numpy %d" % (where, n, len(want))
                np.testing.assert_allclose(topk[i, :n], want, rtol=RTOL, err_msg=where)
                np.testing.assert_allclose(topk[i, :n], otopk[i, :n], rtol=RTOL, err_msg=where + " (oracle)")
                assert np.array_equal(_bits(topk[i]), _bits(res["wand"][1][i])), "%s: not wand's bits" % where


def _groups(g, op, qs, k=10):
    b = d.Batch(g, op, qs, k=k)
    b.run()
    groups = [gr for c in range(NCLS) for gr in b.class_groups(c)]
    b.close()
    return groups


def test_kernel_family(edge):
    """default knobs: `and` and ranked_and run pipelined_stream groups of list capacity 2, 4 and above; DS2I_NO_RANKED_STREAM=1: none"""
    qs = edge.queries
    for op in ("and", "ranked_and"):
        ran = {gr["lists"] for gr in _groups(edge.index("block_optpfor"), op, qs) if gr["pipelined_stream"] and gr["queries"] >= 1}
        assert 2 in ran and 4 in ran and max(ran) > 4, (op, sorted(ran))
        assert not any(gr["pipelined_stream"] for gr in _groups(edge.index("block_optpfor", ("DS2I_NO_RANKED_STREAM=1",)), op, qs)), op
