"""The k-class and batch-mode matrix on every kind of upload (-m gpu). test_gpu_modes.py crosses operator x k x mode at one point of
the index dimension (block_optpfor with every table; block_mixed and opt are transcoded to the same device image). plan_route picks a
batch's kernels from a dozen facts about the INDEX as well; upload_variants.py holds the uploads it tells apart -- no side slots, no
block weights, no range tables, coarse tables, no hints, no bitmaps, the class kernels behind DS2I_NO_RANKED_STREAM /
DS2I_NO_UNION_RSTREAM, DS2I_STREAM_NT_MAX 8 / 4, every query split, opt and block_mixed native, block_varint, block_interpolative --
and this module runs each of them through

  M0  a one-shot Batch            M3  enable_block_profile() before the first run
  M1  the same Batch run again    M4  a Pipeline of depth 3, k and operator changing in the same slots
  M2  set_instrumented(False)     M5  reference_order=True

at k = 10, 64, 65, 256, 257, 1024 (both sides of every TopK / TopKBig<4> / TopKBig<16> edge), the four ranked operators and both query
sets of the two collections of modes_matrix.py (AND / OR sizes on both sides of 64, 256, 1024; ties at the k-th place). One test id per
(variant, collection, mode, query set) loops over k and the ranked operators; one per (variant, collection) holds the unranked ones.

Every cell: the oracle's contract (_check_oracle: counts, freq sums, doc-id lists exact, lengths exact, scores within RTOL = 1e-5, -inf
past the length); _check_structure; at k = 65 / 257 / 1024 the float64 BM25 of the raw lists (_check_float64); M1, M2, M4 bit-equal to the
variant's own M0, M3 and M5 within RTOL of it; counts, freq sums and lengths equal to the M0 of the DEFAULT block_optpfor upload, scores
within RTOL of it; ranked_and bit-identical to the oracle on the queries of at most 8 distinct terms (every variant but the two native
ones); wand == maxscore == ranked_or bit for bit on the short set where all three run a block-synchronous union kernel
(upload_variants.union_bits; within RTOL where the batch goes to the one-document-per-step traversal: reference order, or a
counting run at k > 64). M0 must show the variant's expected paths (upload_variants.check_paths), M3 no stream group at all, and on
opt native the block profile is refused with DS2I_EINVAL. Every input is valid."""
import numpy as np
import pytest

import ds2i_amd as d
from modes_matrix import (COLLS, NCLS, RANKED, RTOL, UNION, UNRANKED, _batch, _check_float64, _check_matches, _check_oracle, _check_structure,  # noqa: F401
                          _run_mode, _same_bits, _within, close_devices, world)
from upload_variants import BY_NAME, DEFAULT, GROUP_OPS, NATIVE, NO_BLOCK_PROFILE, VARIANTS, check_paths, kclass, union_bits

pytestmark = pytest.mark.gpu
KE = [10, 64, 65, 256, 257, 1024]
K64 = (65, 257, 1024)
MODES = ["M0_oneshot", "M1_rerun", "M2_uninstrumented", "M3_profile_before_run", "M5_reference_order", "M4_pipeline"]
BIT_EQUAL_TO_M0 = ("M1_rerun", "M2_uninstrumented", "M4_pipeline")   # the modes that keep M0's kernels
NAMES = [v.name for v in VARIANTS]
DS2I_EINVAL = -1


@pytest.fixture(scope="module")
def worlds(built_lib):
    """the World of a collection (modes_matrix.py: its oracle and float64 answers are shared with test_gpu_modes.py)"""
    yield world
    close_devices()


def _upload(w, v):
    """the variant's device index, holding what Index.info() must report of it"""
    g = w.gidx(v)
    info = g.info()
    for field, want in v.info.items():
        assert info[field] == want, (v.name, field, info[field], want)
    return g


def _cell(w, v, op, k, name, got, mode):
    """what every cell asserts of an answer (count, topk, tlen, fsum or None)"""
    what = (v.name, mode, op, k, name)
    _check_oracle(w, op, k, name, got if got[3] is not None else got[:3] + (w.oracle(op, k, name)[3],))
    if op in RANKED:
        _check_structure(w, op, k, name, got)
        if k in K64:
            _check_float64(w, op, k, name, got)
    own, dflt = w.m0(v, op, k, name), w.m0(DEFAULT, op, k, name)
    if op in RANKED:
        (_same_bits if mode in BIT_EQUAL_TO_M0 else _within)(got, own, what + ("own M0",))
        _within(got, dflt, what + ("default upload's M0",))
    else:
        assert np.array_equal(got[0], own[0]) and np.array_equal(got[0], dflt[0]), what
    if op.endswith("_freq") and got[3] is not None:
        assert np.array_equal(got[3], own[3]) and np.array_equal(got[3], dflt[3]), what
    if op == "ranked_and" and v.name not in NATIVE:
        # block_optpfor images and the block codecs decoded at run time: the float32 sums of the reference's enumerator order, in every mode
        rows = [i for i, q in enumerate(w.sets[name]) if len(set(q)) <= 8]
        otopk = w.oracle("ranked_and", k, name)[1]
        assert np.array_equal(got[1][rows], otopk[rows]), what + (np.argwhere(got[1][rows] != otopk[rows])[:3],)


def _union_agreement(w, v, k, mode, got):
    """got: {op: answer} on the short set"""
    bits = union_bits(v, k) and mode != "M5_reference_order" and not (mode.startswith("M3") and k > 64)
    for op in ("maxscore", "ranked_or"):
        (_same_bits if bits else _within)(got[op], got["wand"], (v.name, mode, op, "== wand" if bits else "~ wand", k))


def _refused_profile(w, v, op, k, name):
    """opt native: no block profile (capi_batch.cpp:578) -- refused, and the batch still answers as M0 does"""
    b = _batch(w.gidx(v), op, w.sets[name], k)
    with pytest.raises(d.Ds2iError) as e:
        b.enable_block_profile()
    assert e.value.code == DS2I_EINVAL, (v.name, op, k, e.value)
    b.run()
    got = b.fetch()
    b.close()
    return got


def _expected_paths(w, v):
    """M0 on the short set: the launch groups the variant's table says, per operator group and k class; the extras of the table"""
    for group in ("ranked_and", "union"):
        for op in GROUP_OPS[group]:
            for k in KE:
                check_paths(v.paths[group, kclass(k)], w.m0_paths(v, op, k, "short"), (v.name, op, k))
    widest = lambda u: max(g[1] for g in w.m0_paths(u, "ranked_and", 10, "short") if g[3])
    if "ranked_and_stream_lists" in v.extra:
        assert widest(DEFAULT) == 16 and widest(v) == v.extra["ranked_and_stream_lists"], (v.name, widest(v))
    if v.extra.get("more_units"):
        for op in ("ranked_and", "wand"):
            units = lambda u: sum(g[2] for g in w.m0_paths(u, op, 10, "short"))
            assert units(v) > units(DEFAULT), (v.name, op, units(v), units(DEFAULT))


def _pipeline(w, v, qset):
    """depth 3, three batches in flight: k and the operator change from one submission to the next in the same slots (every k of KE on
    every ranked operator over the id's query set; `and` / `or_freq` over the OTHER set between them, so the slots change size too);
    every answer is the cell's, and M0's bit for bit"""
    pipe_ks = [10, 1024, 65, 257, 64, 256]
    other = "mixed" if qset == "short" else "short"
    sched = []
    for j in range(len(RANKED)):
        for i, k in enumerate(pipe_ks):
            sched.append((RANKED[(i + j) % 4], k, qset))
        sched.append((("and", "or_freq")[j % 2], 1, other))
    for op, k, name in sched:
        w.m0(v, op, k, name)   # (the one-shot answers first: nothing else runs while the pipeline is in flight)
        w.m0(DEFAULT, op, k, name)
    pipe = d.Pipeline(w.gidx(v), depth=3)
    tickets, answers = [], []
    for job in sched:
        if len(tickets) == 3:
            answers.append((tickets[0][1], pipe.wait(tickets.pop(0)[0])))
        tickets.append((pipe.submit(job[0], w.sets[job[2]], k=job[1]), job))
    while tickets:
        answers.append((tickets[0][1], pipe.wait(tickets.pop(0)[0])))
    pipe.close()
    for (op, k, name), got in answers:
        _cell(w, v, op, k, name, tuple(got) + (None,), "M4_pipeline")   # (a ticket returns no freq sums)


@pytest.mark.parametrize("qset", ["short", "mixed"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("variant", NAMES)
def test_upload_modes_ranked(worlds, variant, coll, mode, qset):
    """one id per (variant, collection, mode, query set): every k of KE, the four ranked operators"""
    w, v = worlds(coll), BY_NAME[variant]
    _upload(w, v)
    if mode == "M4_pipeline":
        return _pipeline(w, v, qset)
    for k in KE:
        got = {}
        for op in RANKED:
            if mode == "M0_oneshot":
                got[op] = w.m0(v, op, k, qset)
            elif mode.startswith("M3") and v.name in NO_BLOCK_PROFILE:
                got[op] = _refused_profile(w, v, op, k, qset)
            else:
                got[op] = _run_mode(w, v, op, k, qset, mode)   # (M3: the profile's totals, and no stream group)
            _cell(w, v, op, k, qset, got[op], mode)
        if qset == "short":
            _union_agreement(w, v, k, mode, got)
    if mode == "M0_oneshot" and qset == "short":
        _expected_paths(w, v)


@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("variant", NAMES)
def test_upload_modes_unranked(worlds, variant, coll):
    """and / and_freq / or / or_freq (they ignore k) in M0, M1, M2, M3 and M5 (M4: between the ranked batches of the pipeline above):
    counts, freq sums and the doc-id lists of `and` / `and_freq` = the oracle's, the variant's M0's and the default upload's; the
    `and` group's expected paths (the same entry in both k classes: k is ignored)"""
    w, v = worlds(coll), BY_NAME[variant]
    _upload(w, v)
    for mode in MODES[:-1]:
        for name in w.sets:
            for op in UNRANKED:
                if mode == "M0_oneshot":
                    got = w.m0(v, op, 1, name)
                    assert np.array_equal(got[0], w.f64[name, op.startswith("and")][1]), (v.name, op, name)
                elif mode.startswith("M3") and v.name in NO_BLOCK_PROFILE:
                    got = _refused_profile(w, v, op, 1, name)
                else:
                    got = _run_mode(w, v, op, 1, name, mode)
                _cell(w, v, op, 1, name, got, mode)
    assert v.paths["and", "k<=64"] == v.paths["and", "k>64"]
    for op in GROUP_OPS["and"]:
        for k in (10, 65):
            b = _batch(w.gidx(v), op, w.sets["short"], k)
            b.run()
            groups = [(c, g["lists"], g["units"], g["pipelined_stream"]) for c in range(NCLS) for g in b.class_groups(c)]
            got = b.fetch()
            b.close()
            check_paths(v.paths["and", kclass(k)], groups, (v.name, op, k))
            assert np.array_equal(got[0], w.m0(v, op, 1, "short")[0]), (v.name, op, k)
