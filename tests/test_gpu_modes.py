"""Differential matrix of the batch modes (-m gpu). plan_batch / launch_batch route a batch by operator, codec, k (TopK up to 64,
TopKBig<4> to 256, TopKBig<16> to 1024), query length, stream launch group or class kernel and seed pass; the modes below must
all give the answers of a one-shot Batch:

  M0  a one-shot Batch                        M3  enable_block_profile(), before the first run and after a run
  M1  the same Batch run again                M4  a Pipeline of depth 3 with operators and k changing in the same slots
  M2  set_instrumented(False)                 M5  reference_order=True

Every cell is checked against the oracle (_check_against_oracle's contract: counts, freq sums, doc-id lists bit-exact, top-k
lengths exact, scores within 1e-5, -inf past the length), against properties that need no reference (rows sorted, length =
min(result size, k), the top-k at k a prefix of the top-k at a larger k, wand == maxscore == ranked_or bit for bit) and, at k =
1 / 65 / 257 / 1024, against a float64 BM25 of the raw lists (helpers.topk64). The modes that keep the kernel family (M1, M2,
M4) must equal M0 bit for bit, the others within the oracle's tolerance.

Two collections: a crafted one whose AND / OR sizes straddle every k boundary, with ties at the k-th place
(helpers.boundary_collection), and the 20 000-document synthetic one of test_gpu.py with edge-shaped queries. Each runs as two
batches: the queries of at most 16 terms (the stream kernels take them) and a small batch that adds the queries beyond 16 terms
(they send the whole batch to the one-document-per-step kernels at k > 64). The oracle reads the block_optpfor image: its
answers do not depend on the codec."""
import numpy as np
import pytest

import ds2i_amd as d
import oracle as o
from helpers import Collection, boundary_collection, boundary_queries, edge_queries, queries_for, small_params, topk64

pytestmark = pytest.mark.gpu
RTOL = 1e-5
NCLS = 5
COLLS = ["boundary", "synth"]
CODECS = ["block_optpfor", "block_mixed", "opt", "block_qmx"]   # block_mixed / opt: transcoded at upload (the default)
DEVICE_OPTPFOR = ("block_optpfor", "block_mixed", "opt")          # ... so these three run every stream path; block_qmx: M0 only
KS = [1, 10, 64, 65, 128, 129, 256, 257, 1000, 1024]
K64 = (1, 65, 257, 1024)
RANKED = ["ranked_and", "wand", "maxscore", "ranked_or"]
UNION = ["wand", "maxscore", "ranked_or"]
UNRANKED = ["and", "and_freq", "or", "or_freq"]
SEEDED = ("wand", "maxscore", "ranked_or")                         # a ranked_and seed pass runs first at k <= 64
ORACLE_THREADS = 8


class World:
    """one collection: its query sets, device indexes per codec, and the cached answers of the oracle, of float64 and of M0"""

    def __init__(self, coll, queries):
        self.coll = coll
        self.sets = {"short": [q for q in queries if len(set(q)) <= 16]}
        self.sets["mixed"] = [q for q in queries if len(set(q)) > 16] + self.sets["short"][::7]
        self.wand = coll.wand_image()
        self.images = {c: coll.index_image(c) for c in CODECS}
        self.oidx = o.Index("block_optpfor", self.images["block_optpfor"], self.wand)
        self._g, self._o, self._m0 = {}, {}, {}
        self.f64 = {}       # (set, conjunctive) -> (scores float64[nq, 1024] padded with -inf, result sizes)
        for name, qs in self.sets.items():
            for conj in (True, False):
                top = np.full((len(qs), max(KS)), -np.inf)
                n = np.zeros(len(qs), dtype=np.int64)
                for i, q in enumerate(qs):
                    s, n[i] = topk64(coll, q, max(KS), conj)
                    top[i, :len(s)] = s
                self.f64[name, conj] = (top, n)

    def gidx(self, codec):
        if codec not in self._g:
            self._g[codec] = d.Index(codec, self.images[codec], self.wand)
        return self._g[codec]

    def oracle(self, op, k, name):
        key = (op, k if op in RANKED else 1, name)
        if key not in self._o:
            self._o[key] = self.oidx.query_batch_mt(op, self.sets[name], k=key[1], threads=ORACLE_THREADS)[:4]
        return self._o[key]

    def m0(self, codec, op, k, name):
        """(count, topk, tlen, fsum) of a one-shot Batch, checked against the oracle and the structure once"""
        key = (codec, op, k if op in RANKED else 1, name)
        if key not in self._m0:
            b = _batch(self.gidx(codec), op, self.sets[name], key[2])
            b.run()
            got = b.fetch()
            if op in ("and", "and_freq"):
                _check_matches(self, b, got[0], name)
            b.close()
            _check_oracle(self, op, key[2], name, got)
            self._m0[key] = got
        return self._m0[key]


@pytest.fixture(scope="module")
def worlds(built_lib):
    out = {}

    def get(name):
        if name not in out:
            if name == "boundary":
                coll = boundary_collection()
                out[name] = World(coll, boundary_queries(coll))
            else:
                coll = Collection(small_params(num_docs=20000, num_terms=300))
                out[name] = World(coll, queries_for(coll, 120) + edge_queries(coll.p.num_terms))
        return out[name]
    yield get
    for w in out.values():
        for g in w._g.values():
            g.close()


def _batch(gidx, op, qs, k, reference_order=False):
    return d.Batch(gidx, op, qs, k=k, want_matches=op in ("and", "and_freq"), reference_order=reference_order)


def _check_oracle(w, op, k, name, got):
    count, topk, tlen, fsum = got
    oc, otopk, otlen, ofsum = w.oracle(op, k, name)
    assert np.array_equal(count, oc), (op, k, name, np.argwhere(count != oc)[:3])
    if op.endswith("_freq"):
        assert np.array_equal(fsum, ofsum), (op, name)
    if op in RANKED:
        assert np.array_equal(tlen, otlen), (op, k, name, np.argwhere(tlen != otlen)[:3])
        f = np.isfinite(otopk)
        assert np.array_equal(np.isfinite(topk), f) and np.all(np.isneginf(topk[~f])), (op, k, name)
        bad = ~np.isclose(topk[f], otopk[f], rtol=RTOL, atol=0)
        assert not bad.any(), (op, k, name, np.argwhere(f)[np.flatnonzero(bad)[:3]])


def _check_matches(w, b, count, name):
    got = b.fetch_matches(count)
    for i, q in enumerate(w.sets[name]):
        assert np.array_equal(got[i], w.oidx.query("and", q, want_matches=True)["matches"]), (name, q)


def _check_structure(w, op, k, name, got):
    """no reference needed: rows sorted descending, -inf past the length, length = min(result size, k)"""
    _, topk, tlen, _ = got
    _, n = w.f64[name, op == "ranked_and"]
    assert np.array_equal(tlen, np.minimum(n, k)), (op, k, name, np.argwhere(tlen != np.minimum(n, k))[:3])
    assert np.all(topk[:, 1:] <= topk[:, :-1]), (op, k, name)
    assert np.all(np.isfinite(topk) == (np.arange(k)[None, :] < tlen[:, None])), (op, k, name)


def _check_float64(w, op, k, name, got):
    _, topk, tlen, _ = got
    top, n = w.f64[name, op == "ranked_and"]
    assert np.array_equal(tlen, np.minimum(n, k))
    f = np.isfinite(top[:, :k])
    assert np.array_equal(np.isfinite(topk), f)
    bad = ~np.isclose(topk[f], top[:, :k][f], rtol=RTOL, atol=0)
    assert not bad.any(), (op, k, name, np.argwhere(f)[np.flatnonzero(bad)[:3]])


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a[:3], b[:3])):   # count, topk, tlen
        assert np.array_equal(x, y), (what, ("count", "topk", "tlen")[i], np.argwhere(x != y)[:3])


def _within(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), what
    f = np.isfinite(b[1])
    assert np.array_equal(np.isfinite(a[1]), f), what
    assert np.allclose(a[1][f], b[1][f], rtol=RTOL, atol=0), what


# ---------------------------------------------------------------- M0: a one-shot Batch
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("coll", COLLS)
def test_m0_unranked_ops(worlds, coll, codec):
    """and / and_freq / or / or_freq (they ignore k): counts, freq sums, doc-id lists = the oracle; counts = the float64
    reference's result sizes"""
    w = worlds(coll)
    for name in w.sets:
        for op in UNRANKED:
            count = w.m0(codec, op, 1, name)[0]
            assert np.array_equal(count, w.f64[name, op.startswith("and")][1]), (op, name)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("coll", COLLS)
def test_m0_ranked_ops(worlds, coll, codec, k):
    w = worlds(coll)
    for name, qs in w.sets.items():
        for op in RANKED:
            got = w.m0(codec, op, k, name)
            _check_structure(w, op, k, name, got)
            if k in K64:
                _check_float64(w, op, k, name, got)
        if codec in DEVICE_OPTPFOR and name == "short":
            # the block-synchronous union kernels sum a document's term scores in fixed point: the three operators agree bit for bit
            # (a >16-term query goes to the one-document-per-step traversal -- at k > 64 with the whole batch -- which keeps the
            # reference's float sums)
            ref = w.m0(codec, "wand", k, name)
            for op in ("maxscore", "ranked_or"):
                _same_bits(w.m0(codec, op, k, name), ref, (op, "== wand", k, name))
        if codec == "block_optpfor":
            # ranked_and on block_optpfor is bit-identical to the oracle (ranked_stream_probe.py: queries of up to 8 terms)
            _, topk, _, _ = w.m0(codec, "ranked_and", k, name)
            otopk = w.oracle("ranked_and", k, name)[1]
            rows = [i for i, q in enumerate(qs) if len(set(q)) <= 8]
            assert np.array_equal(topk[rows], otopk[rows]), (k, name)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("coll", COLLS)
def test_m0_topk_is_a_prefix_of_a_larger_k(worlds, coll, codec):
    w = worlds(coll)
    for name in w.sets:
        for op in RANKED:
            for k1, k2 in zip(KS, KS[1:]):
                a, b = w.m0(codec, op, k1, name)[1], w.m0(codec, op, k2, name)[1][:, :k1]
                f = np.isfinite(a)
                assert np.array_equal(np.isfinite(b), f), (op, k1, k2, name)
                assert np.allclose(a[f], b[f], rtol=RTOL, atol=0), (op, k1, k2, name)


@pytest.mark.parametrize("k", [10, 100, 1000])
@pytest.mark.parametrize("coll", COLLS)
def test_m0_runs_the_stream_kernels_and_m3_none(worlds, coll, k):
    """the path really ran: on block_optpfor a one-shot ranked_and and wand batch runs at least one pipelined stream launch group
    (k_ranked_stream / k_union_stream, TopKBig beyond 64); with the block profile on, none -- every decode is counted"""
    w = worlds(coll)
    gidx = w.gidx("block_optpfor")
    for op in ("ranked_and", "wand"):
        b = _batch(gidx, op, w.sets["short"], k)
        b.run()
        assert any(g["pipelined_stream"] for c in range(NCLS) for g in b.class_groups(c)), (op, k)
        b.enable_block_profile()
        b.run()
        got = b.fetch()
        assert not any(g["pipelined_stream"] for c in range(NCLS) for g in b.class_groups(c)), (op, k)
        b.close()
        _check_oracle(w, op, k, "short", got)


# ---------------------------------------------------------------- M1, M2, M3, M5 against M0
MODES = ["M1_rerun", "M2_uninstrumented", "M3_profile_before_run", "M3_profile_after_run", "M5_reference_order"]


def _profile_totals(w, b, op, k, st, name):
    """block_profile() column sums against the run's counters. finish_batch returns the counters of the batch's own kernels only
    (the seed pass's are dropped), while the profile counts every decode -- the seed pass's too (launch_batch hands it the same
    buffer). So: equal for the operators without a seed pass (and for wand / maxscore / ranked_or beyond 64, which have none);
    for a seeded batch the difference is the seed pass's, and it is 0 when the seed has no query to answer -- the union kernels
    leave it only the one-term queries -- which the batch of the multi-term queries checks exactly."""
    prof = b.block_profile()
    nd, nf = int(prof[:, 0].sum()), int(prof[:, 1].sum())
    assert st.docs_blocks_decoded > 0 or not any(len(q) for q in w.sets[name])
    if op not in SEEDED or k > 64:
        assert (nd, nf) == (st.docs_blocks_decoded, st.freqs_blocks_decoded), (op, k, name)
    else:
        assert nd >= st.docs_blocks_decoded and nf >= st.freqs_blocks_decoded, (op, k, name)


def _run_mode(w, codec, op, k, name, mode):
    qs = w.sets[name]
    b = _batch(w.gidx(codec), op, qs, k, reference_order=mode == "M5_reference_order")
    if mode == "M3_profile_before_run":
        b.enable_block_profile()
    st = b.run()
    first = b.fetch()
    if mode == "M1_rerun":
        st = b.run()
        second = b.fetch()
        _same_bits(second, first, (mode, op, k, name, "run 2 == run 1"))
    elif mode == "M2_uninstrumented":
        b.set_instrumented(False)
        b.run()
    elif mode == "M3_profile_after_run":
        b.enable_block_profile()
        st = b.run()
    got = b.fetch()
    if mode.startswith("M3"):
        _profile_totals(w, b, op, k, st, name)
        assert not any(g["pipelined_stream"] for c in range(NCLS) for g in b.class_groups(c)), (mode, op, k, name)
    if op in ("and", "and_freq"):
        _check_matches(w, b, got[0], name)
    b.close()
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("codec", DEVICE_OPTPFOR)
@pytest.mark.parametrize("coll", COLLS)
def test_modes_ranked(worlds, coll, codec, mode, k):
    w = worlds(coll)
    for name in w.sets:
        for op in RANKED:
            got = _run_mode(w, codec, op, k, name, mode)
            _check_oracle(w, op, k, name, got)
            _check_structure(w, op, k, name, got)
            if k in K64:
                _check_float64(w, op, k, name, got)
            if mode in ("M1_rerun", "M2_uninstrumented"):
                _same_bits(got, w.m0(codec, op, k, name), (mode, op, k, name, "== M0"))
            else:
                _within(got, w.m0(codec, op, k, name), (mode, op, k, name, "~ M0"))
    if mode.startswith("M3") and k <= 64:
        # the seeded operators on a batch whose seed pass has nothing to answer (no one-term query, none beyond 16 terms):
        # the profile and the counters are then the same decodes
        multi = [q for q in w.sets["short"] if len(set(q)) >= 2]
        for op in SEEDED:
            b = _batch(w.gidx(codec), op, multi, k)
            b.enable_block_profile()
            st = b.run()
            prof = b.block_profile()
            assert (int(prof[:, 0].sum()), int(prof[:, 1].sum())) == (st.docs_blocks_decoded, st.freqs_blocks_decoded), (op, k)
            got = b.fetch()
            b.close()
            rows = [i for i, q in enumerate(w.sets["short"]) if len(set(q)) >= 2]
            ref = w.m0(codec, op, k, "short")
            _within(got, tuple(x[rows] for x in ref), (mode, op, k, "multi-term batch ~ M0"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("codec", DEVICE_OPTPFOR)
@pytest.mark.parametrize("coll", COLLS)
def test_modes_unranked(worlds, coll, codec, mode):
    w = worlds(coll)
    for name in w.sets:
        for op in UNRANKED:
            got = _run_mode(w, codec, op, 1, name, mode)
            _check_oracle(w, op, 1, name, got)
            ref = w.m0(codec, op, 1, name)
            assert np.array_equal(got[0], ref[0]), (mode, op, name)
            if op.endswith("_freq"):
                assert np.array_equal(got[3], ref[3]), (mode, op, name)


# ---------------------------------------------------------------- M4: a pipeline with k and operators changing in its slots
PIPE_KS = [10, 1024, 65, 1, 257, 128, 1000, 64, 129, 256]


@pytest.mark.parametrize("codec", DEVICE_OPTPFOR)
@pytest.mark.parametrize("coll", COLLS)
def test_m4_pipeline_mixed_k(worlds, coll, codec):
    """depth 3, three batches in flight: k = 10 -> 1024 -> 65 -> ... and the operator change from one submission to the next in
    the same slots (every k of the matrix on every ranked operator, both query sets, `and` / `or_freq` between them); every answer
    is M0's, bit for bit"""
    w = worlds(coll)
    sched = []
    for j, op in enumerate(RANKED):
        for i, k in enumerate(PIPE_KS):
            sched.append((RANKED[(i + j) % 4], k, "short" if (i + j) % 3 else "mixed"))
        sched.append((("and", "or_freq")[j % 2], 1, "short"))
    pipe = d.Pipeline(w.gidx(codec), depth=3)
    tickets = []

    def collect():
        t, (op, k, name) = tickets.pop(0)
        got = pipe.wait(t)
        ref = w.m0(codec, op, k, name)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]), ("M4", op, k, name)
        if op in RANKED:
            assert np.array_equal(got[1], ref[1]), ("M4", op, k, name, np.argwhere(got[1] != ref[1])[:3])
    for op, k, name in sched:
        w.m0(codec, op, k, name)   # (the one-shot answer first: nothing else runs while the pipeline is in flight)
    for op, k, name in sched:
        if len(tickets) == 3:
            collect()
        tickets.append((pipe.submit(op, w.sets[name], k=k), (op, k, name)))
    while tickets:
        collect()
    pipe.close()
