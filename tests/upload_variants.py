"""The uploads the batch planner tells apart, as data (no test in here; test_gpu_upload_modes.py runs them, test_upload_variants_cpu.py
checks this module's own claims).

plan_route (ds2i_amd/csrc/batch_plan.cpp:140-202) picks the kernels of a batch from what the INDEX has -- side_tables, bound_tables,
rmw, has_bitmaps, skip_or_pef, kind and the knobs no_ranked_stream, no_union_rstream, stream_nt_max -- crossed with the operator, the k
class and the mode flags. A Variant is one point of the index dimension: a codec, the DS2I_* knobs set through set_option around the
upload (they hold for the index that read them, so every variant lives in one process), what Index.info() must report afterwards, and
the EXPECTED PATHS of a one-shot batch of the queries of at most 16 distinct terms, per operator group and k class:

  "S"    at least one pipelined_stream launch group (Batch.class_groups), none in the long class
  "S+L"  stream groups, and the queries above DS2I_STREAM_NT_MAX terms in the long class (k_daat_long)
  "C"    class kernels only: no stream group, nothing in the long class
  "L"    the whole batch in the long class (the one-document-per-step traversal with TopKBig heaps): no other group

A green run over a knob that was silently ignored would prove nothing; the paths are how a variant shows that it left the default.

How an entry follows (batch_plan.cpp lines; goes_long is batch_plan.hpp:78-83):
  stream_tables = side_tables && bound_tables                                                         :167
  bigk_ok       = k > 64 && stream_tables && !no_ranked_stream && stream_nt_max >= 4                  :169
  ranked_and    k <= 64: "S" iff rs_ok = !no_ranked_stream && (side_tables || native block_mixed with its skip table) && bound_tables
                (:198-199; the groups: form_groups :717-731), else "C". k > 64: bigk_stream = bigk_ok (:170) -- then the queries of
                1 .. stream_nt_max terms stream and the others go long (goes_long, hpp:80): "S" at 16, "S+L" below; without bigk_stream
                rs_ok falls (:198) and every query goes long (hpp:82): "L"
  union         k <= 64: union_stream = bound_tables && skip_or_pef (:177); its groups are k_union_stream iff us_ok = !no_union_rstream &&
                stream_tables (:178, form_groups :703-715): "S", else "C" (k_union_topk, or k_disjunctive without bound tables).
                k > 64: bigk_union = bigk_ok && !no_union_rstream (:171): "S"; else union_stream falls (:177) and every query goes long: "L"
  and           k is ignored (:157). "S" (k_ranked_stream<.., AND>) iff block_optpfor (rs_and, :190) and rs_ok, else "C"

The union operators agree bit for bit wherever all three run a block-synchronous union kernel -- k_disjunctive sums in fixed point
(kernels_daat.inc:272-291), k_union_topk and k_union_stream add in one fixed order (kernels_disjunctive.inc:555-556) -- that is every
code but "L", where k_daat_long keeps each operator's reference-order float sums (union_bits)."""
from collections import namedtuple

Variant = namedtuple("Variant", "name codec knobs info paths extra")

GROUPS = ("ranked_and", "union", "and")
KCLASSES = ("k<=64", "k>64")
CODES = ("S", "S+L", "C", "L")
GROUP_OPS = {"ranked_and": ("ranked_and",), "union": ("wand", "maxscore", "ranked_or"), "and": ("and", "and_freq")}

EVERY_TABLE = {"has_side_tables": 1, "has_block_weights": 1, "has_range_tables": 1, "has_bitmaps": 1, "has_membership_hints": 1,
               "range_table_entries_per_posting": 4, "transcoded_from": -1}


def _every_table_but(**changed):
    out = dict(EVERY_TABLE)
    out.update(changed)
    return out


def _paths(ranked_and, union, and_):
    """ranked_and, union: (code at k <= 64, code at k > 64); and_: one code (k is ignored)"""
    return {("ranked_and", "k<=64"): ranked_and[0], ("ranked_and", "k>64"): ranked_and[1],
            ("union", "k<=64"): union[0], ("union", "k>64"): union[1], ("and", "k<=64"): and_, ("and", "k>64"): and_}


# every table, default knobs: rs_ok, us_ok, bigk_stream and bigk_union all hold
DEFAULT_PATHS = _paths(("S", "S"), ("S", "S"), "S")
# no stream kernel anywhere: stream_tables is false (:167), so rs_ok (:198-199: no side tables), us_ok (:178) and bigk_ok (:169) are
NO_STREAM_PATHS = _paths(("C", "L"), ("C", "L"), "C")

VARIANTS = [
    # side_tables false (capi_internal.hpp:116: no d_xslots) -> stream_tables false
    Variant("bare", "block_optpfor", ("DS2I_NO_XSLOTS",), _every_table_but(has_side_tables=0), NO_STREAM_PATHS, {}),
    # no d_bmw, and the range tables are built from the block weights' pass (capi.cpp:738): bound_tables false -> stream_tables false (:167),
    # rs_ok false (:199), union_stream false (:177: k_disjunctive); capi_batch.cpp:213 then hands ranked_and no rmw either
    Variant("no_bmw", "block_optpfor", ("DS2I_NO_BMW",),
            {"has_side_tables": 1, "has_block_weights": 0, "has_range_tables": 0, "has_bitmaps": 0, "has_membership_hints": 0},
            NO_STREAM_PATHS, {}),
    # d_bmw without d_rmw: bound_tables false as above
    Variant("no_rmw", "block_optpfor", ("DS2I_NO_RMW",),
            {"has_side_tables": 1, "has_block_weights": 1, "has_range_tables": 0, "has_bitmaps": 0, "has_membership_hints": 0},
            NO_STREAM_PATHS, {}),
    # the planner reads neither the granularity nor the hints: the default route over coarser tables / without the hint bytes
    Variant("coarse", "block_optpfor", ("DS2I_RMW_G=1",), _every_table_but(range_table_entries_per_posting=1), DEFAULT_PATHS, {}),
    Variant("no_hints", "block_optpfor", ("DS2I_NO_RMH",), _every_table_but(has_membership_hints=0), DEFAULT_PATHS, {}),
    # has_bitmaps false: and_stream falls (:180: 2-4-term all-dense `and` queries keep their units), the kernels get rmw_bitmaps = 0
    # (capi_batch.cpp:214); the groups are the default's
    Variant("no_bitmaps", "block_optpfor", ("DS2I_NO_BITMAPS",), _every_table_but(has_bitmaps=0), DEFAULT_PATHS, {}),
    # no_ranked_stream: rs_ok false (:198) and bigk_ok false (:169) -- EVERY ranked operator of a k > 64 batch goes long, the union ones too;
    # at k <= 64 the union operators keep k_union_stream (us_ok, :178, does not read the knob)
    Variant("class_ranked", "block_optpfor", ("DS2I_NO_RANKED_STREAM",), EVERY_TABLE, _paths(("C", "L"), ("S", "L"), "C"), {}),
    # no_union_rstream: us_ok false (:178: k_union_topk) and bigk_union false (:171); ranked_and and `and` as by default
    Variant("class_union", "block_optpfor", ("DS2I_NO_UNION_RSTREAM",), EVERY_TABLE, _paths(("S", "S"), ("C", "L"), "S"), {}),
    # stream_nt_max 8 / 4 (>= 4: bigk_ok holds): ranked_and streams 2 .. 8 / 2 .. 4 lists (rs_nt :194, cap_of :724) and at k > 64 sends the
    # longer queries long while the rest of the batch stays on the TopKBig streams (goes_long, hpp:80); the union kernels do not read it
    # (cap_of :713, goes_long hpp:81). extra: the widest list capacity a ranked_and stream group may have at k <= 64
    Variant("nt8", "block_optpfor", ("DS2I_STREAM_NT_MAX=8",), EVERY_TABLE, _paths(("S", "S+L"), ("S", "S"), "S"), {"ranked_and_stream_lists": 8}),
    Variant("nt4", "block_optpfor", ("DS2I_STREAM_NT_MAX=4",), EVERY_TABLE, _paths(("S", "S+L"), ("S", "S"), "S"), {"ranked_and_stream_lists": 4}),
    # the default route with every query cut fine: ranked_and units of at most 8 (4 beyond 2 lists) blocks (cut_units :600-612), union
    # units of 8 blocks of the driving list (cut_union_query :487-492). extra: more units than the default upload plans
    Variant("split", "block_optpfor", ("DS2I_UNIT_CAP=8", "DS2I_UT_BLOCKS=8"), EVERY_TABLE, DEFAULT_PATHS, {"more_units": True}),
    # kind = opt, uploaded as it is: no side tables (:116 asks for block_optpfor), bound tables and the chunk directory (skip_or_pef)
    Variant("opt_native", "opt", ("DS2I_PEF_NATIVE",), {"has_side_tables": 0, "has_block_weights": 1, "has_range_tables": 1, "transcoded_from": -1},
            NO_STREAM_PATHS, {}),
    # kind = block_mixed with its skip table: rs_ok holds for ranked_and (:199; k_ranked_stream_mixed, 2 .. 4 lists: rs_nt :194) but not
    # for `and` (rs_and, :190, asks for block_optpfor); stream_tables false -> nothing else streams, k > 64 goes long
    Variant("mixed_native", "block_mixed", ("DS2I_MIXED_NATIVE",), {"has_side_tables": 0, "has_block_weights": 1, "has_range_tables": 1, "transcoded_from": -1},
            _paths(("S", "L"), ("C", "L"), "C"), {"ranked_and_stream_lists": 4}),
    # the runtime-codec kinds: block indexes with a skip table and bound tables, no side tables
    Variant("varint", "block_varint", (), {"has_side_tables": 0, "has_block_weights": 1, "has_range_tables": 1, "transcoded_from": -1}, NO_STREAM_PATHS, {}),
    Variant("interpolative", "block_interpolative", (), {"has_side_tables": 0, "has_block_weights": 1, "has_range_tables": 1, "transcoded_from": -1},
            NO_STREAM_PATHS, {}),
]
BY_NAME = {v.name: v for v in VARIANTS}
DEFAULT = "block_optpfor"                     # the default upload (modes_matrix names it by its codec): every table, default knobs
NATIVE = ("opt_native", "mixed_native")     # the device image is not block_optpfor, nor a block codec decoded at run time
NO_BLOCK_PROFILE = ("opt_native",)          # enable_block_profile: DS2I_EINVAL on a freq_index (capi_batch.cpp:578)


def kclass(k):
    return "k<=64" if k <= 64 else "k>64"


def union_bits(v, k):
    """wand == maxscore == ranked_or bit for bit on a batch without a query beyond 16 terms"""
    return v.paths["union", kclass(k)] != "L"


def check_paths(code, groups, what):
    """groups: the launch groups of a one-shot batch [(class, lists, units, pipelined_stream)] (World.m0_paths); class 4 is the long class"""
    stream = [g for g in groups if g[3]]
    long_ = [g for g in groups if g[0] == 4]
    rest = [g for g in groups if g[0] != 4 and not g[3]]
    assert groups, what
    assert not any(g[0] == 4 for g in stream), what
    if code == "S":
        assert stream and not long_, (what, code, groups)
    elif code == "S+L":
        assert stream and long_, (what, code, groups)
    elif code == "C":
        assert rest and not stream and not long_, (what, code, groups)
    else:
        assert code == "L" and long_ and not stream and not rest, (what, code, groups)


# ---------------------------------------------------------------- what the query sets must reach for the variants to differ
STREAM_CAPACITIES = ((2, 2), (3, 4), (5, 6), (7, 8), (9, 16))   # distinct terms per capacity of k_ranked_stream / k_union_stream


def distinct_terms(q):
    return len(set(q))


def set_claims(coll, sets):
    """The claims test_upload_variants_cpu.py holds for each collection's query sets; returns a dict of booleans / counts.
    short: a query of every stream capacity and a one-term query (nt8 / nt4 move the 9-16- / 5-16-term queries, the one-term ones ride
    in the capacity-4 launch at k > 64); mixed: a query beyond 16 terms (it sends a k > 64 union batch long); no_bitmaps: a queried list
    dense enough to carry a bitmap (RmwLevels::has_bitmap: 64 * n >= num_docs); split: a multi-term query whose SHORTEST list has more
    than 8 blocks (DS2I_UNIT_CAP bounds the units of the shortest list) and a list of more than 8 blocks in a union query."""
    nts = [distinct_terms(q) for q in sets["short"]]
    terms = sorted({t for qs in sets.values() for q in qs for t in q})
    n = lambda t: len(coll.lists[t][0])
    multi = [q for q in sets["short"] if distinct_terms(q) >= 2]
    return {
        "capacities": {cap: sum(lo <= x <= hi for x in nts) for lo, hi in STREAM_CAPACITIES for cap in [hi]},
        "one_term": sum(x == 1 for x in nts),
        "beyond_16": sum(distinct_terms(q) > 16 for q in sets["mixed"]),
        "short_beyond_16": sum(x > 16 for x in nts),
        "dense_lists": sum(64 * n(t) >= coll.num_docs for t in terms),
        "sparse_lists": sum(64 * n(t) < coll.num_docs for t in terms),
        "lists_over_8_blocks": sum(n(t) > 8 * 128 for t in terms),
        "queries_shortest_over_8_blocks": sum(min(n(t) for t in q) > 8 * 128 for q in multi),
    }
