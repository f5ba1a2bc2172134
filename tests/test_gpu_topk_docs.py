"""DS2I_OP_TOPK_DOCS on the GPU (-m gpu): the doc-id of every top-k score, for every ranked operator, codec and k class.

Contract (include/ds2i_hip.h): scores, lengths and counts are the bits of the same batch without ids; a row is ordered by score
descending, equal scores by doc-id ascending, and holds the k largest (score, -doc-id) pairs; entries past the length are
0xFFFFFFFF. ranked_and is bit-identical to the float32 brute force (tests/topk_docs_ref.py), so its ids are checked exactly; the
union operators sum in fixed point (kernels_disjunctive.inc), so theirs are checked against float64 scores and by the order rule,
and must agree between wand, maxscore and ranked_or bit for bit."""
import numpy as np
import pytest

import ds2i_amd as d
from helpers import Collection, boundary_collection, edge_queries, queries_for, small_params
from topk_docs_ref import brute_pairs, doc_scores64, member_any, scored_docs

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
RANKED = ["ranked_and", "wand", "maxscore", "ranked_or"]
UNION = ["wand", "maxscore", "ranked_or"]
KS = [1, 10, 64, 65, 257, 1024]
# (codec, knob set before the upload): the stream path, the class kernels, block_mixed / opt transcoded and queried natively
UPLOADS = [("block_optpfor", None), ("block_qmx", None), ("block_mixed", None), ("opt", None),
           ("block_mixed", "DS2I_MIXED_NATIVE"), ("opt", "DS2I_PEF_NATIVE")]


class Env:
    def __init__(self, coll):
        self.coll, self.wand, self.images, self.idx = coll, coll.wand_image(), {}, {}

    def index(self, codec, knobs=()):
        key = (codec,) + tuple(knobs)
        if key not in self.idx:
            if codec not in self.images:
                self.images[codec] = self.coll.index_image(codec)
            try:
                for kn in knobs:
                    name, _, val = kn.partition("=")
                    d.set_option(name, val or "1")
                self.idx[key] = d.Index(codec, self.images[codec], self.wand)
            finally:
                for kn in knobs:
                    d.set_option(kn.partition("=")[0], None)
        return self.idx[key]

    def close(self):
        for g in self.idx.values():
            g.close()


@pytest.fixture(scope="module")
def synth():
    e = Env(Collection(small_params(num_docs=20000, num_terms=300)))
    e.queries = [q for q in edge_queries(300) if len(q) <= 16] + queries_for(e.coll, 120)
    e.brute = {}
    yield e
    e.close()


@pytest.fixture(scope="module")
def boundary():
    e = Env(boundary_collection())
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _structure(docs, tlen, num_docs, k):
    for i in range(len(tlen)):
        n = int(tlen[i])
        assert n <= k
        assert np.all(docs[i, n:] == NONE), i
        assert np.all(docs[i, :n] < num_docs), i
        assert len(np.unique(docs[i, :n])) == n, i


def _order(topk, docs, tlen):
    """score descending; equal scores by doc-id ascending"""
    for i in range(len(tlen)):
        n = int(tlen[i])
        s, dd = topk[i, :n].astype(np.float64), docs[i, :n].astype(np.int64)
        assert np.all(np.diff(s) <= 0), i
        tie = np.diff(s) == 0
        assert np.all(np.diff(dd)[tie] > 0), i


def run_pair(g, op, qs, k, num_docs):
    """one-shot run with and without ids: the scores part must be the same bits"""
    c0, t0, l0, _ = g.query_batch(op, qs, k)
    c1, t1, docs, l1, st = g.query_batch_docs(op, qs, k)
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1) and np.array_equal(_bits(t0), _bits(t1)), (op, k)
    _structure(docs, l1, num_docs, k)
    _order(t1, docs, l1)
    assert st.docs_blocks_decoded == 0  # (the docs kernels carry no counters: kernel_ms only)
    return c1, t1, docs, l1


def _brute(env, q, conj):
    key = (tuple(q), conj)
    if key not in env.brute:
        env.brute[key] = brute_pairs(env.coll, q, 1024, conj, order="size" if conj else "term")
    return env.brute[key]


@pytest.mark.parametrize("codec,knob", UPLOADS)
def test_ranked_and_ids_exact(synth, codec, knob):
    g = synth.index(codec, [knob] if knob else [])
    for k in KS:
        _, topk, docs, tlen = run_pair(g, "ranked_and", synth.queries, k, synth.coll.num_docs)
        for i, q in enumerate(synth.queries):
            s, bd = _brute(synth, q, True)
            n = min(k, len(bd))
            assert int(tlen[i]) == n, (q, k)
            assert np.array_equal(docs[i, :n], bd[:n]), (codec, knob, k, q)
            # (numpy's float32 BM25 can differ from the kernels' in the last bit: the ids above are the exact check)
            np.testing.assert_allclose(topk[i, :n], s[:n], rtol=1e-6, err_msg=str((codec, knob, k, q)))


def _check_union(env, q, topk, docs, n, k):
    """float64 scores of the returned ids, everything clearly above the k-th score present, membership"""
    if n == 0:
        return
    ids = docs[:n]
    assert np.all(member_any(env.coll, q, ids)), q
    np.testing.assert_allclose(doc_scores64(env.coll, q, ids), topk[:n], rtol=1e-5, err_msg=str(q))
    if n == k:
        alld, _ = scored_docs(env.coll, q, False)
        all64 = doc_scores64(env.coll, q, alld)
        kth = float(doc_scores64(env.coll, q, ids[-1:])[0])
        assert set(alld[all64 > kth * (1 + 1e-5)].tolist()) <= set(ids.tolist()), q


@pytest.mark.parametrize("codec,knob", [UPLOADS[0], UPLOADS[1], UPLOADS[5]])
def test_union_operators_ids(synth, codec, knob):
    g = synth.index(codec, [knob] if knob else [])
    qs = synth.queries[:90]
    for k in (1, 10, 65, 1024):
        res = {op: run_pair(g, op, qs, k, synth.coll.num_docs) for op in UNION}
        for op in UNION[1:]:
            # the same ids wherever the operators' scores are the same bits: everywhere on the block-synchronous kernels (k <= 64, and
            # the stream kernels at any k on block_optpfor); the one-document-per-step kernels that answer k > 64 on the other codecs
            # sum a document's terms in each operator's own order, and a last-bit difference may decide a tie there
            same = np.array([np.array_equal(_bits(res[op][1][i]), _bits(res["wand"][1][i])) for i in range(len(qs))])
            if codec == "block_optpfor" or k <= 64:
                assert same.all(), (codec, op, k)
            assert np.count_nonzero(same & (res["wand"][3] > 0)) >= len(qs) // 4, (codec, op, k, int(same.sum()))
            assert np.array_equal(res[op][2][same], res["wand"][2][same]), (codec, op, k)
        for op in UNION:
            _, topk, docs, tlen = res[op]
            for i, q in enumerate(qs):
                _check_union(synth, q, topk[i], docs[i], int(tlen[i]), k)


def test_tie_group(boundary):
    coll = boundary.coll
    tie = len(coll.lists) - 1
    group = coll.lists[tie][0]
    qs = [[tie], [0, tie]]
    for codec in ("block_optpfor", "block_qmx"):
        g = boundary.index(codec)
        for k in (1, 64, 65, 299, 300, 301, 1024):
            for op in RANKED:
                _, topk, docs, tlen = run_pair(g, op, qs, k, coll.num_docs)
                for i, q in enumerate(qs):
                    m = min(k, 300)
                    assert np.array_equal(docs[i, :m], group[:m]), (codec, op, k, q)
                    assert np.all(_bits(topk[i, :m]) == _bits(topk[i, :1])), (codec, op, k, q)


def test_every_form_gives_the_same_ids(synth):
    g = synth.index("block_optpfor")
    qs = synth.queries[:100]
    ref = {(op, k): run_pair(g, op, qs, k, synth.coll.num_docs) for op in ("ranked_and", "wand") for k in (10, 65, 300)}
    for (op, k), r in ref.items():
        b = d.Batch(g, op, qs, k=k, with_docs=True)
        for _ in range(2):
            b.run()
            c, t, l, _ = b.fetch()
            assert np.array_equal(b.fetch_topk_docs(), r[2]) and np.array_equal(_bits(t), _bits(r[1])), (op, k)
        b.close()
    # depth 3, docs and scores-only tickets interleaved in the same slots, k changing from slot to slot
    p = d.Pipeline(g, depth=3)
    plan = [("ranked_and", 10, True), ("wand", 65, False), ("wand", 300, True), ("ranked_and", 65, True), ("ranked_and", 300, False),
            ("wand", 10, True), ("ranked_and", 300, True), ("wand", 65, True), ("ranked_and", 10, False)]
    inflight = []
    for op, k, docs in plan:
        inflight.append((op, k, docs, p.submit(op, qs, k=k, with_docs=docs)))
        if len(inflight) == 3:
            _collect(p, inflight.pop(0), ref)
    while inflight:
        _collect(p, inflight.pop(0), ref)
    p.close()


def _collect(p, item, ref):
    op, k, docs, t = item
    r = ref[(op, k)]
    if docs:
        c, topk, dd, tlen = p.wait_docs(t)
        assert np.array_equal(dd, r[2]), (op, k)
    else:
        c, topk, tlen = p.wait(t)
    assert np.array_equal(_bits(topk), _bits(r[1])) and np.array_equal(tlen, r[3]) and np.array_equal(c, r[0]), (op, k, docs)


def test_reference_order(synth):
    g = synth.index("block_optpfor")
    qs = synth.queries[:60]
    for k in (10, 65):
        _, t0, d0, l0 = run_pair(g, "ranked_and", qs, k, synth.coll.num_docs)
        b = d.Batch(g, "ranked_and", qs, k=k, reference_order=True, with_docs=True)
        b.run()
        c, t, l, _ = b.fetch()
        dd = b.fetch_topk_docs()
        b.close()
        assert np.array_equal(l, l0)
        same = np.array([np.array_equal(_bits(t[i]), _bits(t0[i])) for i in range(len(qs))])
        assert same.all()  # (ranked_and: bit-identical in every traversal)
        assert np.array_equal(dd[same], d0[same])
        for op in UNION:
            b = d.Batch(g, op, qs, k=k, reference_order=True, with_docs=True)
            b.run()
            c, t, l, _ = b.fetch()
            dd = b.fetch_topk_docs()
            b.close()
            _structure(dd, l, synth.coll.num_docs, k)
            _order(t, dd, l)
            for i, q in enumerate(qs):
                _check_union(synth, q, t[i], dd[i], int(l[i]), k)


def test_split_queries_and_long_queries(synth):
    """split units (k_merge / k_merge_big with ids: units > queries) and > 16 terms (k_daat_long, at k = 10 and 100)"""
    g = synth.index("block_optpfor", ["DS2I_UNIT_CAP=8", "DS2I_UT_BLOCKS=1"])
    short = synth.queries[:80]
    long_ = [list(range(0, 40, 2)), list(range(1, 60, 3))]
    # (a query beyond 16 terms sends a whole wand batch at k > 64 to k_daat_long, one unit per query: the split batches leave them out)
    for qs, ks, split in ((short, (10, 100, 300), True), (short + long_, (10, 100), False)):
        for k in ks:
            for op in ("ranked_and", "wand"):
                b = d.Batch(g, op, qs, k=k, with_docs=True)
                b.run()
                c, t, l, _ = b.fetch()
                dd = b.fetch_topk_docs()
                groups = [gr for cls in range(5) for gr in b.class_groups(cls)]
                b.close()
                if split:
                    assert sum(gr["units"] for gr in groups) > len(qs), (op, k)
                _structure(dd, l, synth.coll.num_docs, k)
                _order(t, dd, l)
                if op == "ranked_and":
                    for i, q in enumerate(qs):
                        s, bd = _brute(synth, q, True)
                        n = min(k, len(bd))
                        assert np.array_equal(dd[i, :n], bd[:n]), (k, q)
                else:
                    for i, q in enumerate(qs):
                        _check_union(synth, q, t[i], dd[i], int(l[i]), k)


def test_errors(synth):
    g = synth.index("block_optpfor")
    qs = synth.queries[:20]
    for op in ("and", "and_freq", "or", "or_freq"):
        with pytest.raises(d.Ds2iError) as e:
            g.query_batch(d.OPS[op] | d.TOPK_DOCS, qs, 10)
        assert e.value.code == -1
        import ctypes as C
        terms, offs = d.flatten_queries(qs)
        h = C.c_void_p()
        assert d.lib().ds2i_hip_batch_prepare(g._h, d.OPS[op] | d.TOPK_DOCS, 10, terms.ctypes.data, offs.ctypes.data, len(qs), 0, C.byref(h)) == -1
    with pytest.raises(d.Ds2iError) as e:  # ds2i_hip_query_batch has no place for the ids
        g.query_batch(d.OPS["wand"] | d.TOPK_DOCS, qs, 10)
    assert e.value.code == -1
    b = d.Batch(g, "ranked_and", qs, k=10)
    b.run()
    with pytest.raises(d.Ds2iError) as e:
        b.fetch_topk_docs()
    assert e.value.code == -1
    b.close()
    b = d.Batch(g, "ranked_and", qs, k=10, with_docs=True)
    with pytest.raises(d.Ds2iError) as e:
        b.enable_block_profile()
    assert e.value.code == -1
    b.close()
    p = d.Pipeline(g, depth=2)
    t = p.submit("wand", qs, k=10)
    with pytest.raises(d.Ds2iError) as e:
        p.wait_docs(t)
    assert e.value.code == -1
    c, topk, tlen = p.wait(t)  # (the refused wait left the ticket in flight)
    c2, topk2, tlen2, _ = g.query_batch("wand", qs, 10)
    assert np.array_equal(_bits(topk), _bits(topk2))
    t = p.submit("wand", qs, k=10, with_docs=True)
    c, topk, tlen = p.wait(t)  # plain wait on a docs ticket drops the ids
    assert np.array_equal(_bits(topk), _bits(topk2))
    p.close()


def test_queries_cli_dump_docs(synth, tmp_path):
    """tools/queries --dump-docs: the same file with one replica and with three (the replicated path, gpu_set_query_op, through
    per-replica pipelines), equal to the Python ids; --dump keeps its format"""
    import os
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ds2i_amd", "tools", "queries")
    if not os.path.exists(tool):
        subprocess.check_call(["make", "-C", os.path.dirname(tool), "-s"])
    idx_path, wand_path = tmp_path / "idx", tmp_path / "wand"
    synth.index("block_optpfor")
    idx_path.write_bytes(synth.images["block_optpfor"])
    wand_path.write_bytes(synth.wand)
    qs = [q for q in synth.queries if q]
    log = "\n".join(" ".join(str(t) for t in q) for q in qs) + "\n"
    ops = ["and", "ranked_and", "wand", "maxscore", "ranked_or"]
    files = []
    for gpus in (1, 3):
        dd, dump = tmp_path / ("docs%d" % gpus), tmp_path / ("dump%d" % gpus)
        r = subprocess.run([tool, "block_optpfor", ":".join(ops), str(idx_path), str(wand_path), "--gpus", str(gpus), "--dump", str(dump),
                            "--dump-docs", str(dd)], input=log, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        files.append(dd.read_text().splitlines())
        lines = dump.read_text().splitlines()
        assert len(lines) == len(ops) * len(qs) and all(":" not in l for l in lines)
    assert files[0] == files[1] and len(files[0]) == 4 * len(qs)  # (ranked operators only)
    g = synth.index("block_optpfor")
    for j, op in enumerate(ops[1:]):
        _, topk, docs, tlen, _ = g.query_batch_docs(op, qs, 10)
        for i in range(len(qs)):
            got = files[0][j * len(qs) + i].split()
            assert got[0] == op and int(got[1]) == int(tlen[i]), (op, i)
            pairs = [p.split(":") for p in got[2:]]
            assert [int(a) for a, _ in pairs] == docs[i, :tlen[i]].tolist(), (op, i)
            assert [int(b, 16) for _, b in pairs] == _bits(topk[i, :tlen[i]]).tolist(), (op, i)


def test_query_op_classes(synth):
    g = synth.index("block_optpfor")
    q = synth.queries[10]
    op = d.ranked_and_query(k=10, with_docs=True)
    op(g, q)
    s, bd = _brute(synth, q, True)
    assert np.array_equal(op.topk_docs(), bd[:len(op.topk())])
