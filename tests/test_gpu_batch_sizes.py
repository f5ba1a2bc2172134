"""Every operator across batch sizes (-m gpu): the batches of tests/batch_size_cases.py -- one collection, about 150 distinct queries,
every size at which the planner of capi_batch.cpp changes what it does, up to 36 000 queries, whose list-stream records need a second
launch slice of 32768 -- must give, row for row, the answers of the CPU references, however the batch is cut into units, planned in
chunks, launched in slices, prepared, pipelined or encoded. tests/test_batch_size_cases_cpu.py proves the batches are what they claim.

The rules (check): and / and_freq / or / or_freq -- counts and freq sums exact (numpy; the oracle agrees), doc-id lists exact;
ranked_and -- counts, lengths and score bits the oracle's, -inf past the length, doc-ids the float32 brute force's and 0xFFFFFFFF past
the length; wand / maxscore / ranked_or -- lengths exact, scores within 1e-5 relative of the oracle, and the three
bit-equal to each other on every row that the block-synchronous or stream kernels answer (a query of more than 16 terms, and a k > 64
batch that holds one, run the one-document-per-step traversal, which sums in each operator's own order: section 5). Within one batch
all copies of one distinct query carry identical bits, for every operator. Every row of every batch is checked."""
import numpy as np
import pytest

import batch_size_cases as bc
import ds2i_amd as d
from batch_size_cases import LARGE, OPS, UNION
from test_gpu_topk_docs import Env, _bits

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
RTOL = 1e-5  # the project's tolerance of the union operators against the oracle
NCLS = 5
MATCH_SIZES = {1, 1025, 4097}             # `and` with want_matches: the doc-id lists
DOCS_SIZES = {1, 513, 1537, 4097, LARGE}  # ranked_and with_docs: the doc-ids of the top-k
GROUPS = {"0-513": [s for s in bc.SIZES if s <= 513], "1023-1537": [s for s in bc.SIZES if 1023 <= s <= 1537],
          "2047-2049": [2047, 2048, 2049], "4095-4097": [4095, 4096, 4097], "large": [LARGE]}
OP_SETS = {"and": ["and"], "and_freq": ["and_freq"], "or": ["or"], "or_freq": ["or_freq"], "ranked_and": ["ranked_and"], "union": UNION}
PLAN_KNOBS = [("DS2I_PLAN_THREADS=1",), ("DS2I_PLAN_THREADS=3",), ("DS2I_PLAN_THREADS=16",)]


@pytest.fixture(scope="module")
def env():
    e = Env(bc.collection())
    e.ref = bc.reference()
    e.nterms = np.array([len(set(q)) for q in bc.distinct_queries()])
    yield e
    e.close()


def run(g, op, nq, k=10, over16="as drawn", with_docs=False, want_matches=False):
    """the batch of nq queries through the one-shot entry points (a prepared batch where only that returns the freq sums or the
    doc-id lists) -> dict(count, topk, tlen[, fsum][, docs][, matches])"""
    _, queries, flat = bc.batch(nq, over16)
    if op in ("and_freq", "or_freq") or want_matches:
        b = d.Batch(g, op, queries, k=k, want_matches=want_matches)
        b.run()
        count, topk, tlen, fsum = b.fetch()
        res = dict(count=count, topk=topk, tlen=tlen, fsum=fsum)
        if want_matches:
            res["matches"] = b.fetch_matches(count)
        b.close()
        return res
    if with_docs:
        count, topk, docs, tlen, _ = g.query_batch_docs(op, flat, k)
        return dict(count=count, topk=topk, tlen=tlen, docs=docs)
    count, topk, tlen, _ = g.query_batch(op, flat, k)
    return dict(count=count, topk=topk, tlen=tlen)


def check(e, op, k, pick, res, where):
    """every row of one result against the references, by the rules of the module's docstring"""
    nq = len(pick)
    count, topk, tlen = res["count"], res["topk"], res["tlen"]
    assert count.shape == (nq,) and tlen.shape == (nq,) and topk.shape[0] == nq, where  # (nq = 0: empty arrays, no error)
    if op in ("and", "and_freq", "or", "or_freq"):
        assert np.array_equal(count, e.ref[op.split("_")[0]][pick]), where
        if "fsum" in res and op.endswith("freq"):
            assert np.array_equal(res["fsum"], e.ref[op][pick]), where
        if "matches" in res:
            assert len(res["matches"]) == nq, where
            for i in range(nq):
                assert np.array_equal(res["matches"][i], e.ref["and_docs"][pick[i]]), (where, i)
        return
    assert topk.shape == (nq, k), where
    rc, rt, rl = e.ref[(op, k)]
    assert np.array_equal(tlen, rl[pick]), where
    live = np.arange(k)[None, :] < rl[pick][:, None]
    assert np.all(np.isneginf(topk[~live])), where  # (a row no kernel wrote included)
    if op == "ranked_and":
        assert np.array_equal(count, rc[pick]), where
        assert np.array_equal(_bits(topk)[live], _bits(rt[pick])[live]), where
        if "docs" in res:
            assert np.array_equal(res["docs"], bc.brute_docs(k)[pick]), where
    else:
        got, want = topk[live].astype(np.float64), rt[pick][live].astype(np.float64)
        assert np.all(np.abs(got - want) <= RTOL * np.abs(want)), (where, float(np.max(np.abs(got - want) / np.abs(want))) if len(want) else 0.0)
        if "docs" in res:
            assert np.all((res["docs"] == NONE) == ~live), where
    # all copies of one distinct query: identical bits
    if nq:
        first = np.zeros(len(e.nterms), dtype=np.int64)
        first[pick[::-1]] = np.arange(nq)[::-1]
        assert np.array_equal(_bits(topk), _bits(topk)[first[pick]]), where
        if "docs" in res:
            assert np.array_equal(res["docs"], res["docs"][first[pick]]), where


def check_union_agree(e, k, pick, results, where, stream_batch=True):
    """wand == maxscore == ranked_or bit for bit, on the rows the block-synchronous and stream kernels answer: every query of up to 16
    terms, unless the batch is a k > 64 one that a query of more than 16 terms sent to the one-document-per-step traversal"""
    if not stream_batch:
        return
    rows = e.nterms[pick] <= 16
    for op in UNION[1:]:
        assert np.array_equal(_bits(results[op]["topk"])[rows], _bits(results["wand"]["topk"])[rows]), (where, op)
        assert np.array_equal(results[op]["tlen"], results["wand"]["tlen"]), (where, op)


def same_bits(a, b):
    return all(np.array_equal(_bits(a[key]) if key == "topk" else a[key], _bits(b[key]) if key == "topk" else b[key]) for key in a if key != "matches")


def run_ops(e, g, ops, nq, k=10, over16="as drawn", where=""):
    pick = bc.batch(nq, over16)[0]
    results = {}
    for op in ops:
        res = run(g, op, nq, k, over16, with_docs=op == "ranked_and" and nq in DOCS_SIZES)
        check(e, op, k, pick, res, (where, op, nq, k, over16))
        results[op] = res
        if op == "and" and nq in MATCH_SIZES:
            check(e, op, k, pick, run(g, op, nq, want_matches=True), (where, op, nq, "matches"))
    if ops == UNION:
        over = bool(np.any(e.nterms[pick] > 16))
        check_union_agree(e, k, pick, results, (where, nq, k), stream_batch=k <= 64 or not over)
    return results


# ---------------------------------------------------------------- 1. every size, every operator, one-shot, block_optpfor
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("ops", list(OP_SETS))
def test_every_size(env, ops, group):
    g = env.index("block_optpfor")
    for nq in GROUPS[group]:
        run_ops(env, g, OP_SETS[ops], nq, where="one-shot")


# ---------------------------------------------------------------- 2. the 32768-term slices
def _groups(b):
    return [gr for c in range(NCLS) for gr in b.class_groups(c)]


@pytest.mark.parametrize("op", ["and", "and_freq", "or_freq", "or"])
def test_large_runs_a_second_slice_of_the_list_streams(env, op):
    """LARGE on the default upload and on one without the list streams (DS2I_NO_LIST_STREAMS=1): both equal the reference.

    That the default run took the streams, and so launched a second slice of 32768 records: for and / and_freq the planner gives a query
    it hands to k_and_stream no work unit (cut_units), and Batch.class_groups counts the queries that have units -- on the default
    upload exactly the queries batch_size_cases.stream_records predicts are missing from the groups, on the knob's upload none is;
    stream_records counts 35 124 (`and`) and 57 619 (and_freq) records for LARGE, more than 32768, and record 32768 of and_freq lies
    inside an all-dense four-term query (test_batch_size_cases_cpu.py). or_freq has no such count: k_freq_stream runs whenever plan_route
    sets freq_stream -- block_optpfor, side tables (asserted here from Index.info), no DS2I_NO_LIST_STREAMS, no reference_order -- over
    every term of the batch, 64 486 for LARGE, with record 32768 inside a four-term query; a slice launched with the wrong qterm_q would
    add those freqs to other queries' sums. `or` takes no list stream: it is here as the half of or_freq that the union kernels answer."""
    pick, queries, _ = bc.batch(LARGE)
    qs = bc.distinct_queries()
    g0, g1 = env.index("block_optpfor"), env.index("block_optpfor", ("DS2I_NO_LIST_STREAMS=1",))
    assert g0.info()["has_side_tables"] and g0.info()["has_bitmaps"] and g0.info()["transcoded_from"] == g1.info()["transcoded_from"]
    with_units = {}
    for name, g in (("default", g0), ("no list streams", g1)):
        b = d.Batch(g, op, queries)
        b.run()
        count, topk, tlen, fsum = b.fetch()
        with_units[name] = sum(gr["queries"] for gr in _groups(b))
        b.close()
        check(env, op, 10, pick, dict(count=count, topk=topk, tlen=tlen, fsum=fsum), (name, op))
    assert with_units["no list streams"] == LARGE, with_units
    if op in ("and", "and_freq"):
        streamed = int(np.count_nonzero(np.array([bc.stream_records(q, op) for q in qs])[pick]))
        records = int(np.sum(np.array([bc.stream_records(q, op) for q in qs])[pick]))
        assert records > bc.SLICE and with_units["default"] == LARGE - streamed, (op, with_units, streamed, records)
    else:
        assert with_units["default"] == LARGE, with_units  # (the union kernels count every query's documents)


# ---------------------------------------------------------------- 3. planning chunks
@pytest.mark.parametrize("ops", list(OP_SETS))
def test_planning_chunks_give_the_same_rows(env, ops):
    """DS2I_PLAN_THREADS = 1, 3 and 16: one chunk below 1024 queries, that many from 1024 on; the special queries sit on both sides of
    every chunk boundary (batch_size_cases._place_specials)"""
    for nq in (1023, 1024, 1025, LARGE):
        results = [run_ops(env, env.index("block_optpfor", knobs), OP_SETS[ops], nq, where=knobs) for knobs in PLAN_KNOBS]
        for knobs, r in zip(PLAN_KNOBS[1:], results[1:]):
            for op in OP_SETS[ops]:
                assert same_bits(r[op], results[0][op]), (op, nq, knobs)


@pytest.mark.parametrize("over16", ["none", "last"])
@pytest.mark.parametrize("k", [65, 257])
@pytest.mark.parametrize("op", ["ranked_and", "wand"])
def test_planning_chunks_beyond_64_scores(env, op, k, over16):
    """k > 64: without a query of more than 16 terms the batch stays on the k-wide stream kernels; with one, in the last planning chunk
    only, a union batch is planned a second time (plan_queries, attempt == 1) over all the chunks"""
    for nq in (1, 1023, 1025, 4097):
        results = [run_ops(env, env.index("block_optpfor", knobs), [op], nq, k, over16, where=knobs) for knobs in PLAN_KNOBS]
        for knobs, r in zip(PLAN_KNOBS[1:], results[1:]):
            assert same_bits(r[op], results[0][op]), (op, k, nq, over16, knobs)


# ---------------------------------------------------------------- 4. prepared batch and pipeline
@pytest.mark.parametrize("op", OPS)
def test_a_prepared_batch_gives_the_same_bits_twice(env, op):
    g = env.index("block_optpfor")
    for nq in (0, 513, 1537, 4097):
        pick, queries, _ = bc.batch(nq)
        with_docs = op == "ranked_and"
        b = d.Batch(g, op, queries, k=10, with_docs=with_docs)
        runs = []
        for _ in range(2):
            b.run()
            count, topk, tlen, fsum = b.fetch()
            res = dict(count=count.copy(), topk=topk.copy(), tlen=tlen.copy(), fsum=fsum.copy())
            if with_docs:
                res["docs"] = b.fetch_topk_docs().copy()
            check(env, op, 10, pick, res, ("prepared", op, nq))
            runs.append(res)
        b.close()
        assert same_bits(runs[0], runs[1]), (op, nq)


PIPELINE_SIZES = [LARGE, 1, 513, 2047, 0, 2049, 64, LARGE, 1535, 2]


@pytest.mark.parametrize("first_op", [0, 4])
def test_pipeline_slots_shrink_and_grow(env, first_op):
    """depth 3, slots in turn: slot 0 holds LARGE, 2047, 64, 2; slot 1 (odd: the second stream set below 2048 queries) 1, 0, LARGE;
    slot 2 513, 2049, 1535. The operator rotates over all eight (from `and`, and from ranked_and), k alternates 10 / 65; a batch of few
    queries, empty ones among them, follows LARGE in the same slot, and its rows must be its own."""
    g = env.index("block_optpfor")
    p = d.Pipeline(g, depth=3)
    inflight = []

    def collect(item):
        op, k, nq, with_docs, t = item
        pick = bc.batch(nq)[0]
        if with_docs:
            count, topk, docs, tlen = p.wait_docs(t)
            res = dict(count=count, topk=topk, tlen=tlen, docs=docs)
        else:
            count, topk, tlen = p.wait(t)
            res = dict(count=count, topk=topk, tlen=tlen)
        check(env, op, k if op in bc.KS else 1, pick, res, ("pipeline", op, k, nq))

    for i, nq in enumerate(PIPELINE_SIZES):
        op, k = OPS[(first_op + i) % len(OPS)], (10, 65)[i & 1]
        with_docs = op == "ranked_and"
        inflight.append((op, k, nq, with_docs, p.submit(op, bc.batch(nq)[2], k=k, with_docs=with_docs)))
        if len(inflight) == 3:
            collect(inflight.pop(0))
    while inflight:
        collect(inflight.pop(0))
    p.close()


# ---------------------------------------------------------------- 5. other kinds
@pytest.mark.parametrize("ops", list(OP_SETS))
@pytest.mark.parametrize("codec", ["opt", "block_qmx"])
def test_other_kinds(env, codec, ops):
    """opt (transcoded at upload, the default) and block_qmx (class kernels: no side tables, no list streams)"""
    g = env.index(codec)
    for nq in (0, 1, 1023, 1025, LARGE):
        run_ops(env, g, OP_SETS[ops], nq, where=codec)


def test_block_qmx_large_is_one_unit_per_query_and_more(env):
    """block_qmx has no list streams: every query of LARGE has a work unit, more than 36 000 units in all (41 979 for `and`), the one-
    and two-term queries' in one launch (30 592). With DS2I_UNIT_CAP=4 (no unit of a ranked conjunction holds more than 4 blocks of its
    shortest list, 8 beyond two lists) that one launch holds more than 36 000 units, and the rows are the same."""
    pick, queries, _ = bc.batch(LARGE)
    for knobs, ops in (((), ("and", "ranked_and")), (("DS2I_UNIT_CAP=4",), ("ranked_and",))):
        g = env.index("block_qmx", knobs)
        assert not g.info()["has_side_tables"]
        for op in ops:
            b = d.Batch(g, op, queries)
            b.run()
            count, topk, tlen, fsum = b.fetch()
            groups = _groups(b)
            b.close()
            check(env, op, 10, pick, dict(count=count, topk=topk, tlen=tlen), ("block_qmx", knobs, op))
            print("block_qmx %s %s, %d queries: units per launch group %s" % (knobs, op, LARGE, [gr["units"] for gr in groups]))
            assert sum(gr["queries"] for gr in groups) == LARGE and sum(gr["units"] for gr in groups) > LARGE, (op, groups)
            short = int(np.count_nonzero((env.nterms[pick] >= 1) & (env.nterms[pick] <= 2)))
            assert max(gr["units"] for gr in groups) >= short > LARGE // 2, (op, short, groups)
            if knobs:
                assert max(gr["units"] for gr in groups) > LARGE, (op, groups)
