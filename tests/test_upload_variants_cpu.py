"""tests/upload_variants.py's own claims, without a device: the variant table is well formed (unique names, knobs the library knows,
an expected-paths entry for every operator group and k class), and the query sets of the two collections of the mode matrices reach what
the variants differ on -- every stream capacity, a one-term query, a query beyond 16 terms, a list dense enough to carry a bitmap (else
DS2I_NO_BITMAPS changes nothing), lists and shortest lists of more than 8 blocks (else DS2I_UNIT_CAP=8 / DS2I_UT_BLOCKS=8 split nothing)."""
import os
import re

import pytest

import upload_variants as uv

HERE = os.path.dirname(os.path.abspath(__file__))


def _known_knobs():
    """kKnobs of capi.cpp: the names ds2i_hip_set_option accepts"""
    src = open(os.path.join(HERE, "..", "ds2i_amd", "csrc", "capi.cpp")).read()
    body = re.search(r"kKnobs\[\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    knobs = re.findall(r'"(DS2I_[A-Z0-9_]+)"', body)
    assert len(knobs) >= 15
    return set(knobs)


def test_variant_table_is_well_formed():
    names = [v.name for v in uv.VARIANTS]
    assert len(set(names)) == len(names)
    wanted = {"bare", "no_bmw", "no_rmw", "coarse", "no_hints", "no_bitmaps", "class_ranked", "class_union", "nt8", "nt4", "split", "opt_native",
              "mixed_native", "varint", "interpolative"}
    assert wanted <= set(names)
    known = _known_knobs()
    import ds2i_amd as d
    from ds2i_amd.api import IndexInfo
    for v in uv.VARIANTS:
        assert v.codec in d.CODECS, v.name
        for kn in v.knobs:
            assert kn.partition("=")[0] in known, (v.name, kn)
        assert v.info, v.name
        assert all(f in dict(IndexInfo._fields_) for f in v.info), v.name
        assert set(v.paths) == {(g, kc) for g in uv.GROUPS for kc in uv.KCLASSES}, v.name
        assert all(code in uv.CODES for code in v.paths.values()), v.name
        assert v.paths["and", "k<=64"] == v.paths["and", "k>64"] in ("S", "C"), v.name   # k is ignored, and nothing of `and` goes long
        assert all(v.paths[g, "k<=64"] in ("S", "C") for g in uv.GROUPS), v.name             # k <= 64: only a query beyond 16 terms goes long
    assert set(uv.NATIVE) | set(uv.NO_BLOCK_PROFILE) <= set(names)
    # a variant that sets a knob differs from the default upload in what info() reports, in its paths or in an extra: nothing else would
    # tell a silently ignored knob from one that was read
    for v in uv.VARIANTS:
        if v.codec == "block_optpfor":
            assert v.info != uv.EVERY_TABLE or v.paths != uv.DEFAULT_PATHS or v.extra, v.name


def test_check_paths_tells_the_codes_apart():
    groups = {"S": [(0, 2, 5, True), (0, 2, 1, False)], "S+L": [(1, 4, 5, True), (4, 16, 2, False)], "C": [(0, 2, 5, False)], "L": [(4, 17, 3, False)]}
    for code, g in groups.items():
        for want in uv.CODES:
            if want == code:
                uv.check_paths(want, g, code)
            else:
                with pytest.raises(AssertionError):
                    uv.check_paths(want, g, (code, want))
    for want in uv.CODES:
        with pytest.raises(AssertionError):
            uv.check_paths(want, [], want)


@pytest.fixture(scope="module", params=["boundary", "synth"])
def claims(request, built_lib):
    from modes_matrix import collection, query_sets
    coll, queries = collection(request.param)
    return uv.set_claims(coll, query_sets(queries))


def test_query_sets_reach_every_stream_capacity(claims):
    assert all(n > 0 for n in claims["capacities"].values()), claims["capacities"]
    assert sorted(claims["capacities"]) == [2, 4, 6, 8, 16]
    assert claims["one_term"] > 0
    assert claims["beyond_16"] > 0 and claims["short_beyond_16"] == 0


def test_no_bitmaps_precondition(claims):
    assert claims["dense_lists"] > 0 and claims["sparse_lists"] > 0, claims


def test_split_precondition(claims):
    assert claims["lists_over_8_blocks"] > 0 and claims["queries_shortest_over_8_blocks"] > 0, claims
