"""The machinery of the batch-mode matrices (test_gpu_modes.py, test_gpu_upload_modes.py): a plain module, no test in it.

One World per collection holds its query sets, the device index of every upload asked for, and the cached answers of the oracle, of
float64 (helpers.topk64) and of every upload's one-shot Batch (M0). An upload is named by a codec ("block_optpfor": the default
upload of that codec) or by a variant of upload_variants.py (a codec plus knobs set around the upload); device indexes and M0
answers are keyed by the upload's name. The oracle reads the block_optpfor image and float64 the raw lists: neither depends on the
upload, so both are computed once per collection (world()) and shared by every test module of the process."""
import numpy as np

import ds2i_amd as d
import oracle as o
from helpers import Collection, boundary_collection, boundary_queries, edge_queries, queries_for, small_params, topk64

RTOL = 1e-5
NCLS = 5
COLLS = ["boundary", "synth"]
KS = [1, 10, 64, 65, 128, 129, 256, 257, 1000, 1024]
RANKED = ["ranked_and", "wand", "maxscore", "ranked_or"]
UNION = ["wand", "maxscore", "ranked_or"]
UNRANKED = ["and", "and_freq", "or", "or_freq"]
SEEDED = ("wand", "maxscore", "ranked_or")                         # a ranked_and seed pass runs first at k <= 64
ORACLE_THREADS = 8


def collection(name):
    """(collection, queries) of COLLS[..]: the crafted boundary collection, or the 20 000-document synthetic one with edge-shaped queries"""
    if name == "boundary":
        coll = boundary_collection()
        return coll, boundary_queries(coll)
    coll = Collection(small_params(num_docs=20000, num_terms=300))
    return coll, queries_for(coll, 120) + edge_queries(coll.p.num_terms)


def query_sets(queries):
    """short: the queries of at most 16 distinct terms (the stream kernels take them); mixed: the ones beyond 16 plus every 7th short one"""
    sets = {"short": [q for q in queries if len(set(q)) <= 16]}
    sets["mixed"] = [q for q in queries if len(set(q)) > 16] + sets["short"][::7]
    return sets


def _upload(v):
    """(name, codec, knobs) of an upload: a codec name, or a variant (upload_variants.Variant)"""
    return (v, v, ()) if isinstance(v, str) else (v.name, v.codec, tuple(v.knobs))


class World:
    """one collection: its query sets, device indexes per upload, and the cached answers of the oracle, of float64 and of M0"""

    def __init__(self, coll, queries):
        self.coll = coll
        self.sets = query_sets(queries)
        self.wand = coll.wand_image()
        self.images = {}
        self.oidx = o.Index("block_optpfor", self.image("block_optpfor"), self.wand)
        self._g, self._o, self._m0, self._matches = {}, {}, {}, {}
        self.paths = {}     # M0 key -> launch groups of that one-shot Batch [(class, lists, units, pipelined_stream)]
        self.f64 = {}       # (set, conjunctive) -> (scores float64[nq, 1024] padded with -inf, result sizes)
        for name, qs in self.sets.items():
            for conj in (True, False):
                top = np.full((len(qs), max(KS)), -np.inf)
                n = np.zeros(len(qs), dtype=np.int64)
                for i, q in enumerate(qs):
                    s, n[i] = topk64(coll, q, max(KS), conj)
                    top[i, :len(s)] = s
                self.f64[name, conj] = (top, n)

    def image(self, codec):
        if codec not in self.images:
            self.images[codec] = self.coll.index_image(codec)
        return self.images[codec]

    def gidx(self, v):
        """the device index of an upload; a variant's knobs hold for the index that read them, so they are set around the upload only"""
        name, codec, knobs = _upload(v)
        if name not in self._g:
            img = self.image(codec)
            try:
                for kn in knobs:
                    opt, _, val = kn.partition("=")
                    d.set_option(opt, val or "1")
                self._g[name] = d.Index(codec, img, self.wand)
            finally:
                for kn in knobs:
                    d.set_option(kn.partition("=")[0], None)
        return self._g[name]

    def oracle(self, op, k, name):
        key = (op, k if op in RANKED else 1, name)
        if key not in self._o:
            self._o[key] = self.oidx.query_batch_mt(op, self.sets[name], k=key[1], threads=ORACLE_THREADS)[:4]
        return self._o[key]

    def m0(self, v, op, k, name):
        """(count, topk, tlen, fsum) of a one-shot Batch, checked against the oracle and the structure once"""
        key = (_upload(v)[0], op, k if op in RANKED else 1, name)
        if key not in self._m0:
            b = _batch(self.gidx(v), op, self.sets[name], key[2])
            b.run()
            got = b.fetch()
            self.paths[key] = [(c, g["lists"], g["units"], g["pipelined_stream"]) for c in range(NCLS) for g in b.class_groups(c)]
            if op in ("and", "and_freq"):
                _check_matches(self, b, got[0], name)
            b.close()
            _check_oracle(self, op, key[2], name, got)
            self._m0[key] = got
        return self._m0[key]

    def m0_paths(self, v, op, k, name):
        self.m0(v, op, k, name)
        return self.paths[_upload(v)[0], op, k if op in RANKED else 1, name]

    def close_devices(self):
        """closes the device indexes; every cached answer stays (an upload asked for again is made again)"""
        for g in self._g.values():
            g.close()
        self._g = {}


_WORLDS = {}


def world(name):
    """the World of a collection, made once per process"""
    if name not in _WORLDS:
        _WORLDS[name] = World(*collection(name))
    return _WORLDS[name]


def close_devices():
    for w in _WORLDS.values():
        w.close_devices()


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
    if name not in w._matches:   # (the oracle's doc-id lists of a query set: asked for once)
        w._matches[name] = [w.oidx.query("and", q, want_matches=True)["matches"] for q in w.sets[name]]
    for i, q in enumerate(w.sets[name]):
        assert np.array_equal(got[i], w._matches[name][i]), (name, q)


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
