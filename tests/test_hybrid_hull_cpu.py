"""The hulls of the block_mixed optimiser, part by part (ds2i_hybrid_hull / HybridBuilder.hull). host_hybrid.hpp measures a
part (integers: sizes, exception counts, live interpolative nodes) and turns the record into its (space, time) hull in two
steps, so that the GPU analysis can supply the records; these properties of the hulls hold whichever side measured."""
import numpy as np
import pytest

import ds2i_amd as d
from helpers import Collection, small_params

MIXED_INTERP = 2


@pytest.fixture(scope="module")
def coll(built_lib):
    return Collection(small_params(num_docs=30000, num_terms=120))


@pytest.fixture(scope="module")
def analysed(coll):
    rng = np.random.default_rng(5)
    hb = d.HybridBuilder(coll.num_docs)
    for docs, freqs in coll.lists:
        hb.add_posting_list(docs, freqs, rng.integers(0, 1000, (len(docs) + 127) // 128 * 2).astype(np.uint32))
    lo, hi = hb.analyse()
    hulls = [[(hb.hull(t, b, 0), hb.hull(t, b, 1)) for b in range((len(docs) + 127) // 128)] for t, (docs, _) in enumerate(coll.lists)]
    return hb, lo, hi, hulls


def test_every_hull_is_a_lower_convex_chain(coll, analysed):
    _, _, _, hulls = analysed
    sizes = set()
    for per_list in hulls:
        for pair in per_list:
            for h in pair:
                assert h.dtype == d.HULL_POINT and len(h) >= 1
                sizes.add(len(h))
                assert np.all(np.diff(h["space"].astype(np.int64)) > 0)  # increasing space ...
                assert np.all(np.diff(h["time"]) < 0)                    # ... buys strictly less time
                assert np.all((h["type"] == 0) == (h["b"] >= 0)) and np.all(h["type"] <= 2)
    assert max(sizes) >= 3  # (the collection has parts with a real trade-off)


def test_hull_ends_sum_to_min_and_max_space(analysed):
    _, lo, hi, hulls = analysed
    assert sum(int(h["space"][0]) for per_list in hulls for pair in per_list for h in pair) == lo
    assert sum(int(h["space"][-1]) for per_list in hulls for pair in per_list for h in pair) == hi
    assert lo < hi


def test_partial_block_has_one_interpolative_point(coll, analysed):
    _, _, _, hulls = analysed
    seen = 0
    for (docs, _), per_list in zip(coll.lists, hulls):
        for b, pair in enumerate(per_list):
            full = (b + 1) * 128 <= len(docs)
            for h in pair:
                if not full:
                    assert len(h) == 1 and h["type"][0] == MIXED_INTERP and h["b"][0] == -1 and h["time"][0] == 0.0
                    seen += 1
                else:
                    assert np.all(h["time"] > 0)
    assert seen > 0


def test_hull_errors(coll, analysed):
    hb = analysed[0]
    for args in ((len(coll.lists), 0, 0), (0, 10 ** 6, 0), (0, 0, 2)):
        with pytest.raises(d.Ds2iError):
            hb.hull(*args)
    fresh = d.HybridBuilder(coll.num_docs)
    fresh.add_posting_list(*coll.lists[0])
    with pytest.raises(d.Ds2iError):  # not analysed yet
        fresh.hull(0, 0, 0)
