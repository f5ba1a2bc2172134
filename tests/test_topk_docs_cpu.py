"""DS2I_OP_TOPK_DOCS without a GPU: the brute-force (score, doc-id) reference, the header and wrappers, and the docs translation
units of the hand-issued-load kernels (the audit of test_abi_cpu.test_hand_issued_loads_have_no_register_destination, plus
register budgets of the docs instantiations)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
from helpers import Collection, boundary_collection, edge_queries, queries_for, small_params, topk64
from topk_docs_ref import brute_pairs, canonical_topk, doc_scores64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_canonical_order_breaks_ties_by_doc_id():
    docs = np.array([9, 3, 7, 1, 5], dtype=np.uint32)
    s = np.array([2.0, 1.0, 2.0, 1.0, 3.0], dtype=np.float32)
    ts, td = canonical_topk(docs, s, 4)
    assert td.tolist() == [5, 7, 9, 1] and ts.tolist() == [3.0, 2.0, 2.0, 1.0]


@pytest.fixture(scope="module")
def synth():
    return Collection(small_params(num_docs=20000, num_terms=300))


@pytest.mark.parametrize("conj", [True, False])
def test_brute_pairs_against_float64(synth, conj):
    """equal scores to 1e-5 and equal doc sets wherever the float64 scores are separated by more than 1e-5"""
    qs = [q for q in edge_queries(300) + queries_for(synth, 40) if len(q)]
    for q in qs:
        for k in (1, 10, 257):
            s32, docs = brute_pairs(synth, q, k, conj, order="size" if conj else "term")
            s64, n = topk64(synth, q, k, conj)
            assert len(s32) == len(s64) == min(k, n), q
            np.testing.assert_allclose(s32, s64, rtol=1e-5, err_msg=str(q))
            if not len(docs):
                continue
            own = doc_scores64(synth, q, docs)
            np.testing.assert_allclose(own, s32, rtol=1e-5, err_msg=str(q))
            kth = s64[-1]
            # every document clearly above the k-th score is returned
            from topk_docs_ref import scored_docs
            alld, _ = scored_docs(synth, q, conj)
            all64 = doc_scores64(synth, q, alld)
            must = set(alld[all64 > kth * (1 + 1e-5)].tolist())
            assert must <= set(docs.tolist()), q


def test_tie_group_returns_smallest_doc_ids():
    coll = boundary_collection()
    tie = len(coll.lists) - 1
    group = coll.lists[tie][0]
    for q in ([tie], [0, tie]):
        for k in (1, 64, 65, 299, 300, 301):
            s, docs = brute_pairs(coll, q, k, True)
            assert np.all(s == s[0])
            assert docs.tolist() == group[:min(k, 300)].tolist()


def test_header_declares_docs_interface():
    h = open(os.path.join(ROOT, "include", "ds2i_hip.h")).read()
    assert re.search(r"DS2I_OP_TOPK_DOCS\s*=\s*0x400", h)
    for sym in ("ds2i_hip_query_batch_docs", "ds2i_hip_batch_fetch_topk_docs", "ds2i_hip_pipeline_wait_docs"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, h), sym
    assert d.TOPK_DOCS == 0x400


@pytest.mark.parametrize("op", ["and", "and_freq", "or", "or_freq"])
def test_wrappers_refuse_docs_on_unranked_operators(op, monkeypatch):
    """refused in Python, before the library is asked (no library call, no GPU needed)"""
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(d.api, "lib", no_library)
    with pytest.raises(ValueError):
        d.Batch(None, op, [[1, 2]], k=10, with_docs=True)
    with pytest.raises(ValueError):
        d.Pipeline.submit(d.Pipeline.__new__(d.Pipeline), op, [[1, 2]], k=10, with_docs=True)
    with pytest.raises(ValueError):
        d.Index.query_batch_docs(None, op, [[1, 2]], k=10)
    cls = d.and_query if op.startswith("and") else d.or_query
    with pytest.raises(ValueError):
        cls(with_freqs=op.endswith("freq"), with_docs=True)


# ---- the docs units of the kernels that issue loads by hand, compiled once for the module with the build's flags and defines (ds2i_amd/build.py, DOCS_UNITS)


@pytest.fixture(scope="module")
def docs_listings(tmp_path_factory):
    from concurrent.futures import ThreadPoolExecutor
    from ds2i_amd import build as bld
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("docs_tus")
    units = {u.replace(".hip", ""): (src, defs) for src, u, defs in bld.DOCS_UNITS if not u.startswith("kernels")}
    assert units and all("-DDS2I_DOCS_TU" in defs for _, defs in units.values())

    def compile_one(item):
        name, (src, defs) = item
        out = str(tmp / (name + ".s"))
        subprocess.check_call([hipcc, "--offload-arch=gfx950"] + bld.COMMON + defs + ["-S", "--cuda-device-only", "-o", out,
                              os.path.join(ROOT, "ds2i_amd", "csrc", src)], stderr=subprocess.DEVNULL)
        return name, open(out).read()
    with ThreadPoolExecutor(max_workers=len(units)) as pool:
        return dict(pool.map(compile_one, units.items()))


def _meta(text):
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[nm] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in ("sgpr_spill_count", "vgpr_spill_count", "vgpr_count", "private_segment_fixed_size")}
    return out


def test_docs_units_hand_issued_loads_have_no_register_destination(docs_listings):
    import asm_audit
    for name, (kpat, nkern, min_dma) in {"ranked_stream_docs": (r"k_ranked_stream_docs", 5, 6), "ranked_stream_bigk_docs": (r"k_ranked_stream_docs", 10, 6),
                                         "ranked_stream_mixed_docs": (r"k_ranked_stream_mixed_docs", 3, 4), "union_stream_docs": (r"k_union_stream_docs", 5, 6),
                                         "union_stream_bigk_docs": (r"k_union_stream_docs", 10, 6)}.items():
        text = docs_listings[name]
        assert "s_swappc" not in text and "s_call_b64" not in text, name
        ks = {n: l for n, l in asm_audit.kernels(text).items() if re.search(kpat, n)}
        assert len(ks) == nkern, (name, sorted(ks))
        for kn, lines in ks.items():
            in_asm, dma = False, 0
            for l in lines:
                t = l.strip()
                if t.startswith(";;#ASMSTART"):
                    in_asm = True
                elif t.startswith(";;#ASMEND"):
                    in_asm = False
                elif in_asm and re.match(r"(global|buffer|flat)_load", t):
                    assert "_lds_" in t.split()[0], (kn, t)
                    dma += 1
            assert dma >= min_dma, (name, kn)
            assert asm_audit.audit(lines) == [], (name, kn)


# Register budgets of the docs instantiations (uninstrumented; list capacity, heap registers NK) -> (VGPRs, VGPR spills, scratch bytes,
# SGPR spills), recorded from the code-object metadata of this source. The doc-id beside each heap register costs one VGPR per NK:
# at the 80-VGPR budget of capacity 2 / 4 (6 waves per SIMD, the scores-only launch bounds kept) that is spilled -- capacity 2 goes
# from 0 to 14 spilled VGPRs, capacity 4 from 23 to 27; the others stay in registers.
RS_BUDGET = {(2, 1): (80, 14, 44, 61), (4, 1): (80, 27, 96, 107), (6, 1): (111, 0, 0, 144), (8, 1): (116, 0, 0, 176), (16, 1): (142, 0, 0, 333),
             (2, 4): (89, 0, 0, 94), (4, 4): (105, 0, 0, 129), (6, 4): (121, 0, 0, 150), (8, 4): (125, 0, 0, 184), (16, 4): (151, 0, 0, 343),
             (2, 16): (126, 0, 0, 157), (4, 16): (142, 0, 0, 225), (6, 16): (149, 0, 0, 268), (8, 16): (153, 0, 0, 313), (16, 16): (188, 0, 0, 419)}
US_BUDGET = {(2, 1): (80, 0, 0, 52), (4, 1): (96, 0, 0, 147), (6, 1): (121, 0, 0, 185), (8, 1): (131, 0, 0, 276), (16, 1): (179, 0, 0, 585),
             (2, 4): (94, 0, 0, 65), (4, 4): (115, 0, 0, 140), (6, 4): (128, 0, 0, 196), (8, 4): (140, 0, 0, 274), (16, 4): (188, 0, 0, 585),
             (2, 16): (130, 0, 0, 164), (4, 16): (148, 0, 0, 250), (6, 16): (164, 0, 0, 322), (8, 16): (168, 2, 12, 370), (16, 16): (225, 0, 0, 677)}
MIXED_BUDGET = {2: (80, 28, 136, 126), 3: (96, 34, 120, 229), 4: (96, 30, 128, 315)}


def _within(m, budget, slack=8):
    vg, vs, ps, ss = budget
    # (VGPRs are bounded by the launch bounds; spills and scratch may move a little with the compiler: a small slack, never a new spill class)
    return m["vgpr_count"] <= vg and m["vgpr_spill_count"] <= (vs + slack if vs else 0) and m["private_segment_fixed_size"] <= (ps + 4 * slack if ps else 0) \
        and m["sgpr_spill_count"] <= ss + 4 * slack


def test_docs_kernels_register_budgets(docs_listings):
    seen = 0
    for tu in ("ranked_stream_docs", "ranked_stream_bigk_docs"):
        for nm, m in _meta(docs_listings[tu]).items():
            mm = re.search(r"k_ranked_stream_docsILi(\d+)ELb0ELb0ELb0ELi(\d+)EE", nm)
            if mm:
                seen += 1
                assert _within(m, RS_BUDGET[(int(mm.group(1)), int(mm.group(2)))]), (nm, m)
    for tu in ("union_stream_docs", "union_stream_bigk_docs"):
        for nm, m in _meta(docs_listings[tu]).items():
            mm = re.search(r"k_union_stream_docsILi(\d+)ELb0ELi(\d+)EE", nm)
            if mm:
                seen += 1
                assert _within(m, US_BUDGET[(int(mm.group(1)), int(mm.group(2)))]), (nm, m)
    for nm, m in _meta(docs_listings["ranked_stream_mixed_docs"]).items():
        mm = re.search(r"k_ranked_stream_mixed_docsILi(\d+)E", nm)
        if mm:
            seen += 1
            assert _within(m, MIXED_BUDGET[int(mm.group(1))]), (nm, m)
    assert seen == 33
