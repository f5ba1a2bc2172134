"""The table-edge collection (tests/table_edge_cases.py) without a GPU: it is what its docstring says, its census meets the floors the
GPU test (tests/test_gpu_table_edges.py) relies on, the union direction and the top 10 are what the alias cases need, and the oracle
answers every query like numpy -- so a mismatch on the GPU points at the GPU."""
import numpy as np
import pytest

import oracle as o
import table_edge_cases as tc
from helpers import brute_or, doc_term_weight, topk64
from table_edge_cases import A, ALIAS, ANCHORS, B, C, CATEGORIES, D, E, GS, NAMES, NUM_DOCS, PD, PROBE_OF, SPARSE

RTOL = 1e-5
FLOOR = 8  # candidates per census cell that can exist


@pytest.fixture(scope="module")
def coll():
    return tc.collection()


def test_collection_is_what_it_says(coll):
    assert coll.num_docs == NUM_DOCS == (1 << 20) + 37 and len(coll.lists) == 16
    assert 95 <= coll.sizes.mean() <= 115
    n = [len(dd) for dd, _ in coll.lists]
    assert max(n) < NUM_DOCS // 5                                   # no idf near 0
    shifts = {G: [tc.expected_shift(m, G) for m in n] for G in GS}
    assert [shifts[4][t] for t in ANCHORS] == [8, 7, 6, 3, 0]
    assert [shifts[2][t] for t in ANCHORS] == [9, 8, 7, 4, 1]
    assert [shifts[1][t] for t in ANCHORS] == [10, 9, 8, 5, 2]
    assert tc.has_bitmap(n[D]) and tc.has_bitmap(n[E]) and not any(tc.has_bitmap(n[t]) for t in (A, B, C))
    for anchor, probe, _ in SPARSE:
        assert n[probe] < n[anchor]                                 # the probe drives the conjunction
        dd, ff = coll.lists[anchor]
        assert dd[-1] == NUM_DOCS - 1 and dd[0] < 64 and np.count_nonzero(ff != 1) == 1
        cnt = np.bincount(dd >> 10, minlength=1025)
        lone = dd[(cnt[dd >> 10] == 1) & ((dd & 1023) < 2)]
        assert len(lone) >= 300                                     # several hundred windows with one posting at offset 0 or 1
        assert {253, 254, 255} <= set((dd[cnt[dd >> 10] == 1] & 255).tolist())
        assert np.count_nonzero(cnt == 0) >= 60 and np.count_nonzero(cnt > 1) >= 100
        pd = coll.lists[probe][0]
        for step in tc.ALIAS_STEPS:                                 # the probe holds the document `step` above some lone postings
            assert np.count_nonzero(np.isin(lone + step, pd)) >= 80 and not np.isin(lone + step, dd).any()
        assert np.count_nonzero(np.isin(lone, pd)) >= 50 and np.count_nonzero(np.isin(lone + 100, pd)) >= 50
        assert NUM_DOCS - 1 in pd
    dd = coll.lists[D][0]
    assert np.isin([0, 7, 8, 63, 64, NUM_DOCS - 1], dd).all() and not np.isin([1, 6, 9, 62, 65, NUM_DOCS - 2], dd).any()
    assert np.isin([0, 1, 6, 7, 8, 9, 62, 63, 64, 65, NUM_DOCS - 2, NUM_DOCS - 1], coll.lists[PD][0]).all()
    # the weight edge: a few hundred postings of C below 1/255 of its maximum, some ranges holding nothing else at every shift C takes
    dd, ff = coll.lists[C]
    w = doc_term_weight(ff, coll.norm_lens[dd])
    tiny = w < w.max() / np.float32(255.0)
    assert 200 <= np.count_nonzero(tiny) <= 400 and np.isin(dd[tiny], coll.lists[PROBE_OF[C]][0]).all()
    assert np.all(coll.sizes[dd[tiny]] >= 550 * coll.sizes.mean())
    core = coll.lists[0][0]
    for dd, _ in coll.lists[1:]:
        core = np.intersect1d(core, dd)
    assert len(core) >= 80


def test_queries_cover_the_shapes(coll):
    qs = tc.queries()
    assert 80 <= len(qs) <= 110 and qs == tc.queries()
    assert all([t] in qs for t in range(16)) and all([PROBE_OF[a], a] in qs for a in ANCHORS)
    assert {len(set(q)) for q in qs} >= {1, 2, 3, 4, 5, 6, 8, 16}
    assert sum(len(q) > 16 for q in qs) == 1 and len(qs[-1]) > 16
    assert any(len(q) > len(set(q)) for q in qs[:-1])
    for a in ANCHORS:  # the probe with its anchor and one, two, three and more further anchors
        assert {len(set(q) & set(ANCHORS)) for q in qs if q[0] == PROBE_OF[a] and a in q} >= {1, 2, 3, 4, 5}
    assert all(len(tc.reference()[i]["and"]) >= 1 for i in range(len(qs)))  # the shared core: no conjunction is empty


def test_census_meets_its_floors(coll, capsys):
    """every cell (category, anchor, G) that can exist at the anchor's shift holds at least FLOOR candidates, summed over the pairs that
    probe the anchor; alias candidates at shift exactly 8: at least 8 per G; at shift 9 and beyond: at least 32 per G that has such a list"""
    lines = []
    for G in GS:
        cells = tc.census(G)
        assert all(b != a for a, b in cells)
        at8 = beyond = 0
        for anchor in ANCHORS:
            s = tc.expected_shift(len(coll.lists[anchor][0]), G)
            mine = [cell for (_, probed), cell in cells.items() if probed == anchor]
            assert len(mine) >= 2, (G, NAMES[anchor])
            for name in CATEGORIES:
                total = sum(cell[name] for cell in mine)
                lines.append("G = %d  %-2s shift %2d  %-42s %6d%s" % (G, NAMES[anchor], s, name, total, "" if tc.possible(name, anchor, G) else "  (cannot exist)"))
                if tc.possible(name, anchor, G):
                    assert total >= FLOOR, (G, NAMES[anchor], s, name, total)
                elif name == ALIAS:
                    assert total == 0, (G, NAMES[anchor], s)
            at8 += sum(cell[ALIAS] for cell in mine) if s == 8 else 0
            beyond += sum(cell[ALIAS] for cell in mine) if s >= 9 else 0
        assert at8 >= 8, (G, at8)
        assert beyond >= 32 or G == 4, (G, beyond)  # (at G = 4 no anchor is beyond shift 8)
        # E's last range is one document wide at every shift it takes: the document is there, and its probe asks for it
        assert NUM_DOCS - 1 in coll.lists[E][0] and NUM_DOCS - 1 in coll.lists[PROBE_OF[E]][0]
    print("\n".join(lines))  # (every cell, shown when the test fails)
    with capsys.disabled():
        print("\n%-42s %s" % ("candidates, all pairs", "  ".join("G = %d" % G for G in GS)))
        for name, row in tc.census_table().items():
            print("%-42s %s" % (name, "  ".join("%6d" % v for v in row)))


def test_union_direction_and_top_ten(coll):
    """for every sparse anchor and its probe: the anchor's maximum score exceeds the probe's (in the union kernels the anchor is the
    exclusion list: its hints are read for the probe's candidates), and the float64 top 10 of their union are alias documents -- at
    least 8 of them the document 254 above a lone posting, an alias at every shift from 8 on"""
    for anchor, probe, _ in SPARSE:
        assert tc.max_score(coll, anchor) > 1.05 * tc.max_score(coll, probe), NAMES[anchor]
        docs = brute_or(coll, [probe, anchor]).astype(np.int64)
        from topk_docs_ref import doc_scores64
        s = doc_scores64(coll, [probe, anchor], docs)
        top = docs[np.argsort(-s, kind="stable")[:10]]
        alias254 = coll.marks[anchor]["alias"][254]
        assert np.count_nonzero(np.isin(top, alias254)) >= 8, (NAMES[anchor], top.tolist())
        for G in GS:
            sh = tc.expected_shift(len(coll.lists[anchor][0]), G)
            if sh >= 8:
                cat = tc.categories(coll, probe, anchor, G, top)
                assert np.count_nonzero(cat[ALIAS]) >= 8, (NAMES[anchor], G)
        assert s[np.argsort(-s)[9]] > s[np.argsort(-s)[200]] * (1 + 1e-3)  # (dropping the alias documents changes the 10 scores)


def test_oracle_equals_numpy(coll):
    qs, ref = tc.queries(), tc.reference()
    oidx = o.Index("block_optpfor", coll.index_image("block_optpfor"), coll.wand_image())
    for i, q in enumerate(qs):
        r = oidx.query("and", q, want_matches=True)
        assert r["count"] == len(ref[i]["and"]) and np.array_equal(r["matches"], ref[i]["and"]), q
        assert oidx.query("or", q)["count"] == ref[i]["or"], q
        rf = oidx.query("and_freq", q)
        assert rf["count"] == len(ref[i]["and"]) and rf["freq_sum"] == ref[i]["and_freq"], q
        rf = oidx.query("or_freq", q)
        assert rf["count"] == ref[i]["or"] and rf["freq_sum"] == ref[i]["or_freq"], q
    for k in (1, 10, 64, 65):
        _, topk, tlen, _, _ = oidx.query_batch("ranked_and", qs, k=k)
        for i, q in enumerate(qs):
            want = ref[i]["top_and"][:k]
            assert int(tlen[i]) == len(want), (q, k)
            np.testing.assert_allclose(topk[i, :len(want)], want, rtol=RTOL, err_msg=str(("ranked_and", q, k)))
    for k in (10, 64):
        for op in ("wand", "maxscore", "ranked_or"):
            _, topk, tlen, _, _ = oidx.query_batch(op, qs, k=k)
            for i, q in enumerate(qs):
                want = ref[i]["top_or"][:k]
                assert int(tlen[i]) == len(want), (op, q, k)
                np.testing.assert_allclose(topk[i, :len(want)], want, rtol=RTOL, err_msg=str((op, q, k)))
    oidx.close()
    assert topk64(coll, qs[0], 1, True)[1] == len(coll.lists[qs[0][0]][0])
