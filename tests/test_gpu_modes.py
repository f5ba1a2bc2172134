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
answers do not depend on the codec. The World and the checks live in modes_matrix.py; test_gpu_upload_modes.py runs them over the
other uploads the planner tells apart."""
import numpy as np
import pytest

import ds2i_amd as d
from modes_matrix import (COLLS, KS, MODES, NCLS, RANKED, RTOL, SEEDED, UNION, UNRANKED, _batch, _check_float64, _check_oracle,  # noqa: F401
                          _check_structure, _run_mode, _same_bits, _within, close_devices, world)

pytestmark = pytest.mark.gpu
CODECS = ["block_optpfor", "block_mixed", "opt", "block_qmx"]   # block_mixed / opt: transcoded at upload (the default)
DEVICE_OPTPFOR = ("block_optpfor", "block_mixed", "opt")          # ... so these three run every stream path; block_qmx: M0 only
K64 = (1, 65, 257, 1024)


@pytest.fixture(scope="module")
def worlds(built_lib):
    """the World of a collection (modes_matrix.py: shared with test_gpu_upload_modes.py); this module's device indexes are closed after it"""
    yield world
    close_devices()


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


# ---------------------------------------------------------------- M1, M2, M3, M5 against M0 (MODES, _run_mode: modes_matrix.py)
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
