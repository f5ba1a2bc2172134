#!/usr/bin/env python
"""k_ranked_stream asks a dense list's exact bitmap instead of its membership hint (ranked_stream.hip; RmwLevels::has_bitmap,
bitmap_first): a crafted collection of 16 384 documents -- a list carries a bitmap from 256 postings on -- with lists at one
posting per 2, 4, 8, 16, 32 and 64 documents, one of 255 postings (just no bitmap) and sparse ones, doc-ids planted on the byte and
line edges of a bitmap, and a clustered list whose ranges hold several postings next to candidates that are not in it.

collection() / queries() build the case, reference() computes what every operator must return (the oracle and the numpy brute
force; no GPU), main() runs the case on the GPU against a stored reference. Run as a subprocess by tests/test_gpu_ranked_bitmaps.py,
because the library's knobs are read once per process:
`[DS2I_UNIT_CAP=8] [DS2I_NO_BITMAPS=1] [DS2I_RMW_G=2] [DS2I_STREAM_NT_MAX=4] python tests/ranked_bitmaps_probe.py reference.npz`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds2i_amd as d  # noqa: E402
from helpers import Collection, brute_and  # noqa: E402

NUM_DOCS = 16384
EDGES = (0, 7, 8, 1023, 1024, NUM_DOCS - 1)  # first / last bit of a bitmap byte, last / first doc-id of a 128-byte line, the padded end
KS = (10, 100)
NONE = 0xFFFFFFFF
# terms: 0..5 dense (1/2 .. 1/64: bitmaps), 6: 255 postings (no bitmap), 7: clustered (1/16), 8: candidates inside its ranges,
# 9..12 sparse
D2, D4, D8, D16, D32, D64, S255, CL, NEAR, SP130, SP100, SP40, SP17 = range(13)


def collection():
    rng = np.random.default_rng(0xB17A)
    n = NUM_DOCS
    edges = np.array(EDGES)
    rest = np.setdiff1d(np.arange(n), edges)

    def draw(m, planted):  # m postings in all, the edges among them if planted
        if planted:
            return np.sort(np.concatenate([edges, rng.choice(rest, m - len(edges), replace=False)]))
        return np.sort(rng.choice(rest, m, replace=False))
    docs = [draw(n // 2, True), draw(n // 4, False), draw(n // 8, True), draw(n // 16, False), draw(n // 32, True), draw(n // 64, True),
            draw(255, True)]
    assert len(docs[D64]) == 256 and len(docs[S255]) == 255
    # the clustered list: in every other 32-document window the offsets 1, 2, 5, 6 (two pairs, each inside one range of 2, 4 or 8
    # doc-ids) ...
    win = np.arange(1, n // 32 - 1, 2) * 32
    docs.append(np.sort(np.concatenate([win + o for o in (1, 2, 5, 6)])))
    assert len(docs[CL]) * 16 == n - 64
    # ... and candidates in the same ranges: offset 3 (between the pairs: not a member) in every window, offset 2 (a member) in every
    # third, offset 4 in every fifth
    docs.append(np.sort(np.concatenate([win + 3, win[::3] + 2, win[::5] + 4])))
    docs += [draw(130, True), draw(100, True), draw(40, False), draw(17, True)]
    lists = [(dd, rng.integers(1, 9, len(dd)).astype(np.uint32)) for dd in docs]
    sizes = rng.integers(20, 400, n).astype(np.uint32)
    return Collection.from_lists(n, lists, sizes)


def queries():
    rng = np.random.default_rng(0xB17B)
    dense = [D2, D4, D8, D16, D32, D64]
    qs = [[D2], [SP17], [D64, D64], [D8, D8, D2], [SP100, D4, SP100, D2]]                      # one term; a list repeated
    qs += [dense[i:i + m] for m in range(2, 7) for i in range(0, 7 - m)]                       # all dense, 2..6 lists
    qs += [[D2, D8, D64], [D4, D16, D64, D2], [D2, D4, D8], [D2, D4, D8, D16], [D2, D4], [D4, D8]]
    qs += [[s] + dense[:m] for s in (SP130, SP100, SP40, SP17) for m in range(1, 6)]           # sparse list 0, dense list 1..
    qs += [[SP130, D32, D64], [SP130, D16, D32, D64], [SP130, D64, D8]]
    qs += [[SP100, S255], [SP100, S255, D8], [SP40, S255, D8, D2], [SP17, SP130, S255, D64, D4, D2], [S255, D64], [S255, D2, D4]]  # no bitmap on list 1, bitmaps further on
    qs += [[NEAR, CL], [NEAR, CL, D2], [NEAR, CL, D4, D2], [D64, CL, D2], [SP130, CL, D8, D2, D4], [CL, D2], [CL, D4, D2], [NEAR, D2, CL, D8, D4, D16]]  # several postings per range
    qs += [sorted(set(int(t) for t in rng.integers(0, 13, m + 1)))[:m] for m in range(2, 7) for _ in range(10)]
    return [q for q in qs if q]


def reference(path):
    """what the oracle (scores, counts, freq sums) and the numpy brute force (doc-id lists) say; stored for the GPU runs"""
    import oracle as o
    from topk_docs_ref import brute_pairs
    coll, qs = collection(), queries()
    img, wand = coll.index_image("block_optpfor"), coll.wand_image()
    oidx = o.Index("block_optpfor", img, wand)
    out = {}
    for k in KS:
        oc, otopk, otlen, _, _ = oidx.query_batch("ranked_and", qs, k=k)
        ids = np.full((len(qs), k), NONE, dtype=np.uint32)
        for i, q in enumerate(qs):
            _, bd = brute_pairs(coll, q, k, True)
            ids[i, :len(bd)] = bd
        out.update({"count%d" % k: oc, "topk%d" % k: otopk, "tlen%d" % k: otlen, "ids%d" % k: ids})
    ac, _, _, _, _ = oidx.query_batch("and", qs)
    fc, _, _, ffs, _ = oidx.query_batch("and_freq", qs)
    m = [brute_and(coll, q) for q in qs]
    assert np.array_equal(ac, [len(x) for x in m]) and np.array_equal(fc, ac)
    out.update({"and_count": ac, "freq_sum": ffs, "matches": np.concatenate(m), "match_off": np.cumsum([0] + [len(x) for x in m])})
    # the case holds what it is meant to hold: thresholds that never form and thresholds that do, at both k
    nres = np.asarray(ac)
    multi = np.array([len(set(q)) >= 3 for q in qs])
    assert (nres[multi] < 10).sum() >= 10 and (nres[multi] >= 100).sum() >= 5 and ((nres[multi] >= 10) & (nres[multi] < 100)).sum() >= 3
    np.savez(path, **out)


def main(path):
    ref = np.load(path)
    coll, qs = collection(), queries()
    wand = coll.wand_image()
    g = d.Index("block_optpfor", coll.index_image("block_optpfor"), wand)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    streamed = False
    for k in KS:
        b = d.Batch(g, "ranked_and", qs, k=k)
        b.run()
        gc, gtopk, gtlen, _ = b.fetch()
        streamed |= any(grp["pipelined_stream"] for c in range(4) for grp in b.class_groups(c))
        b.close()
        assert np.array_equal(gc, ref["count%d" % k]) and np.array_equal(gtlen, ref["tlen%d" % k]), (k, np.argwhere(gc != ref["count%d" % k])[:3])
        assert np.array_equal(bits(gtopk), bits(ref["topk%d" % k])), (k, [qs[i] for i in np.argwhere(bits(gtopk) != bits(ref["topk%d" % k]))[:3, 0]])
        c1, t1, docs, l1, _ = g.query_batch_docs("ranked_and", qs, k)
        assert np.array_equal(c1, gc) and np.array_equal(l1, gtlen) and np.array_equal(bits(t1), bits(gtopk)), k
        assert np.array_equal(docs, ref["ids%d" % k]), (k, [qs[i] for i in np.argwhere(docs != ref["ids%d" % k])[:3, 0]])
    assert streamed
    stream_groups = lambda b: [grp for c in range(4) for grp in b.class_groups(c) if grp["pipelined_stream"]]
    for want in (False, True):
        b = d.Batch(g, "and", qs, want_matches=want)
        b.run()
        gc, _, _, _ = b.fetch()
        assert stream_groups(b), ("and", want)  # (the AND instantiations of k_ranked_stream took their share of the batch)
        assert np.array_equal(gc, ref["and_count"]), ("and", want, [qs[i] for i in np.argwhere(gc != ref["and_count"])[:3, 0]])
        if want:
            got, off = b.fetch_matches(gc), ref["match_off"]
            for i in range(len(qs)):
                assert np.array_equal(got[i], ref["matches"][off[i]:off[i + 1]]), qs[i]
        b.close()
    b = d.Batch(g, "and_freq", qs)
    b.run()
    gc, _, _, gfs = b.fetch()
    assert stream_groups(b), "and_freq"
    b.close()
    assert np.array_equal(gc, ref["and_count"]) and np.array_equal(gfs, ref["freq_sum"]), "and_freq"
    # The bitmap is what answers where there is one: for [NEAR, CL] with the doc-id lists wanted (k_ranked_stream<2, AND>; no list
    # streams) CL's bitmap settles every candidate, so only NEAR's own blocks are decoded. Without bitmaps the candidates between
    # CL's pairs sit in ranges of several postings (hint 255) and CL's blocks have to be searched and decoded.
    bitmaps = os.environ.get("DS2I_NO_BITMAPS") is None
    assert bool(g.info()["has_bitmaps"]) == bitmaps
    b = d.Batch(g, "and", [[NEAR, CL]], want_matches=True)
    decoded = b.run().as_dict()["docs_blocks_decoded"]
    assert stream_groups(b)
    b.close()
    own = (len(coll.lists[NEAR][0]) + 127) // 128
    assert (0 < decoded <= own) if bitmaps else decoded > own, (bitmaps, decoded, own)
    g.close()
    print("ranked_bitmaps_probe ok: %d queries" % len(qs))


if __name__ == "__main__":
    main(sys.argv[1])
