"""The build side of block_mixed on the GPU (-m gpu): ds2i_hip_encode_index for block_varint and block_interpolative, and the
optimiser's device half (ds2i_hip_hybrid_analyse / ds2i_hip_hybrid_freeze). The reference of every comparison is the HOST builder
or optimiser (build_index, HybridBuilder with device=None); everything is compared bit for bit -- images as bytes, hull points as
raw 8-byte records (the float as its u32), rate and model time as Python floats with ==."""
import numpy as np
import pytest

import ds2i_amd as d
from helpers import Collection, queries_for, small_params

pytestmark = pytest.mark.gpu

NEW_KINDS = ("block_varint", "block_interpolative")
FRACS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def coll(built_lib):
    return Collection(small_params(num_docs=20000, num_terms=300))


@pytest.fixture(scope="module")
def queries(coll):
    return queries_for(coll, 300) + [[], [5], [5, 5], [7, 3, 7, 3], [0, 1, 2], [0], [299, 298, 297, 296, 295, 294]]


def _from_gaps(gaps_m1, freqs_m1):
    """(docs, freqs) whose gaps - 1 and freqs - 1 are the given values"""
    docs = np.cumsum(np.asarray(gaps_m1, dtype=np.uint64) + 1) - 1
    assert int(docs[-1]) < (1 << 32) - 16
    return docs.astype(np.uint32), (np.asarray(freqs_m1, dtype=np.uint64) + 1).astype(np.uint32)


def _value_of_byte_length(rng, lens):
    lo = np.array([0, 0, 1 << 8, 1 << 16, 1 << 24], dtype=np.uint64)[lens]
    hi = np.array([0, 1 << 8, 1 << 16, 1 << 24, (1 << 24) + 4096], dtype=np.uint64)[lens]  # (4-byte values stay small: see below)
    return lo + (rng.integers(0, 1 << 62, len(lens)).astype(np.uint64) % (hi - lo))


@pytest.fixture(scope="module")
def edge_lists(built_lib):
    """Lengths around the block size; all-zero parts; values on the byte-length edges of VarInt-G8IU; a byte-length sequence in
    which groups fill to exactly 8 bytes and a 4-byte integer meets 5, 6 and 7 used bytes; gaps up to 2^19. Every 128-value part
    sums to less than 2^32 - 1 (the host's interpolative codes u32 prefix sums)."""
    rng = np.random.default_rng(0xED6E)
    lists = []
    for n in (1, 127, 128, 129, 128 * 3 + 5):
        lists.append(_from_gaps(rng.integers(0, 40, n), rng.integers(0, 6, n)))
    lists.append((np.arange(1000, 1000 + 256, dtype=np.uint32), np.ones(256, np.uint32)))  # zero interpolative bits, 16 full groups
    edges = np.array([255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24], dtype=np.uint64)
    lists.append(_from_gaps(edges[rng.integers(0, 6, 128)], edges[rng.integers(0, 6, 128)]))
    # 4 4 | 1 x 8 | 2 x 4 | 3 3 2 | 1 4 + pad 3 | 4 2 + pad 2 | 4 3 + pad 1 | 4 4
    pattern = [4, 4] + [1] * 8 + [2] * 4 + [3, 3, 2] + [1, 4] + [4, 2] + [4, 3] + [4, 4]
    lens = np.array((pattern * 11)[:256])
    lists.append(_from_gaps(_value_of_byte_length(rng, lens), _value_of_byte_length(rng, np.roll(lens, 7))))
    n = 128 * 3 + 5
    lists.append(_from_gaps(rng.integers(0, 1 << 19, n), rng.integers(0, 1 << 20, n)))
    for dd, ff in lists:  # the premise of the block_interpolative comparisons
        gaps = np.diff(np.concatenate([[-1], dd.astype(np.int64)])) - 1
        for k in range(0, len(dd), 128):
            assert int(gaps[k:k + 128].sum()) < (1 << 32) - 1 and int((ff[k:k + 128].astype(np.int64) - 1).sum()) < (1 << 32) - 1
    return lists


@pytest.fixture(scope="module")
def sweep_lists(built_lib):
    """the exception sweep (0 .. 110 exceptions per block, docs and freqs) and the big_f list of
    test_gpu.py::test_gpu_encode_is_byte_identical: big_f's full freq parts sum past 2^32 (no interpolative candidate) and hold 31-bit
    values (every b with max_b - b > 28 is skipped, b = 32 is a candidate)"""
    rng = np.random.default_rng(99)
    nblk = 111
    freqs = rng.integers(1, 5, 128 * nblk).astype(np.uint32)
    gaps = rng.integers(1, 5, 128 * nblk).astype(np.uint64)
    for k in range(nblk):
        pos = rng.choice(128, k, replace=False) + 128 * k
        freqs[pos] = 1 + (1 << 10) + rng.integers(0, 1 << 9, k).astype(np.uint32)
        pos = rng.choice(128, k, replace=False) + 128 * k
        gaps[pos] = 1 + (1 << 9) + rng.integers(0, 1 << 8, k)
    docs = (np.cumsum(gaps) - 1).astype(np.uint32)
    big_d = (np.cumsum(rng.integers(1, 1 << 19, 128 * 3 + 5).astype(np.uint64)) - 1).astype(np.uint32)
    big_f = rng.integers(1, (1 << 31) - 2, len(big_d)).astype(np.uint32)
    big_f[384:] = rng.integers(1, 1 << 20, len(big_d) - 384)
    assert int((big_f[:128].astype(np.int64) - 1).sum()) >= (1 << 32) and int(big_f[:128].max()) >= 1 << 30
    return [(docs, freqs), (big_d, big_f)]


def _num_docs(lists):
    return int(max(int(dd[-1]) for dd, _ in lists)) + 10


def _nblocks(docs):
    return (len(docs) + 127) // 128


def _model(name):
    """mi355x: the default decode-time model, under which OptPFor is the fastest decoder and interpolative the smallest -- the
    collection's blocks are interpolative or OptPFor, all OptPFor from about a third of the budget range on. cheap_varint: a
    CPU-like model whose VarInt-G8IU is the fastest decoder, so that the optimiser's images hold VarInt-G8IU blocks too (checked
    with the host path: about two thirds of the docs parts at half the range)."""
    if name == "mi355x":
        return None
    m = d.HybridModel.default()
    m.varint = 50.0
    return m


def _builder(num_docs, lists, access, model=None):
    """access: None or (blocks of all lists, 2) counters"""
    hb = d.HybridBuilder(num_docs, model)
    base = 0
    for docs, freqs in lists:
        nb = _nblocks(docs)
        hb.add_posting_list(docs, freqs, None if access is None else access[base:base + nb])
        base += nb
    return hb


def _all_hulls(hb, lists):
    return b"".join(hb.hull(t, b, side).tobytes() for t, (docs, _) in enumerate(lists) for b in range(_nblocks(docs)) for side in (0, 1))


# ---------------------------------------------------------------- the two new kinds of ds2i_hip_encode_index
@pytest.mark.parametrize("codec", NEW_KINDS)
def test_new_kinds_byte_identical_on_the_collection(coll, codec):
    img, ms = d.gpu_encode_index(coll.num_docs, coll.lists, codec=codec)
    assert img == d.build_index(codec, coll.num_docs, coll.lists) and ms > 0
    gidx = d.Index(codec, img)
    for t in (0, 171):
        dd, ff = gidx[t]
        assert np.array_equal(dd, coll.lists[t][0]) and np.array_equal(ff, coll.lists[t][1])


@pytest.mark.parametrize("codec", NEW_KINDS)
def test_new_kinds_byte_identical_on_the_edge_set(edge_lists, codec):
    N = _num_docs(edge_lists)
    img, _ = d.gpu_encode_index(N, edge_lists, codec=codec)
    assert img == d.build_index(codec, N, edge_lists)
    gidx = d.Index(codec, img)
    for t in (6, 7):  # the byte-length edges, the group-filling pattern
        dd, ff = gidx[t]
        assert np.array_equal(dd, edge_lists[t][0]) and np.array_equal(ff, edge_lists[t][1])


def test_optpfor_kind_unchanged_on_the_edge_set(edge_lists):
    N = _num_docs(edge_lists)
    assert d.gpu_encode_index(N, edge_lists)[0] == d.build_index("block_optpfor", N, edge_lists)


# ---------------------------------------------------------------- analyse: hulls
@pytest.fixture(scope="module")
def profile(coll, queries):
    """a real block-access profile: 64 ranked_and queries on the collection"""
    gidx = d.Index("block_optpfor", coll.index_image("block_optpfor"), coll.wand_image())
    b = d.Batch(gidx, "ranked_and", queries[:64], k=10)
    b.enable_block_profile()
    b.run()
    prof = b.block_profile().copy()
    b.close()
    assert prof.shape == (sum(_nblocks(dd) for dd, _ in coll.lists), 2) and int(prof.sum()) > 0
    return prof


@pytest.fixture(scope="module", params=["mi355x", "cheap_varint"])
def pair(request, coll, profile):
    """the collection in two builders with the profile's counters: one analysed on the host, one on the GPU"""
    m = _model(request.param)
    host, dev = _builder(coll.num_docs, coll.lists, profile, m), _builder(coll.num_docs, coll.lists, profile, m)
    return host, host.analyse(), dev, dev.analyse(device=0), request.param


def test_hulls_equal_on_the_collection(coll, pair):
    host, host_space, dev, dev_space, _ = pair
    assert dev_space == host_space and host_space[0] < host_space[1]
    assert dev.device_ms > 0
    assert _all_hulls(dev, coll.lists) == _all_hulls(host, coll.lists)


@pytest.mark.parametrize("counters", ["none", "random"])
def test_hulls_equal_on_edges_and_exception_sweep(edge_lists, sweep_lists, counters):
    lists = edge_lists + sweep_lists
    N = _num_docs(lists)
    access = None
    if counters == "random":
        access = np.random.default_rng(17).integers(0, 1000, (sum(_nblocks(dd) for dd, _ in lists), 2)).astype(np.uint32)
    host, dev = _builder(N, lists, access), _builder(N, lists, access)
    assert dev.analyse(device=0) == host.analyse()
    assert _all_hulls(dev, lists) == _all_hulls(host, lists)
    # what the big_f list is there for: no interpolative point, b = 32 on the hull or at least a candidate set without small b
    t = len(lists) - 1
    for h in (host.hull(t, 0, 1), dev.hull(t, 0, 1)):
        assert not np.any(h["type"] == 2) and np.all(h["b"][h["type"] == 0] >= 2)
    # ... and both freezes of this set agree too (interpolative, varint and raw 32-bit parts side by side)
    lo, hi = host.analyse()
    for budget in (lo, lo + (hi - lo) // 2, None):
        img, info = host.freeze(budget)
        gimg, ginfo = dev.freeze(budget, device=0)
        assert gimg == img and _same_info(ginfo, info)


# ---------------------------------------------------------------- freeze: images
def _same_info(ginfo, info):
    return all(ginfo[k] == info[k] for k in ("rate", "space", "model_time", "type_counts"))


def _budgets(lo, hi):
    return [lo, hi, None] + [int(lo + f * (hi - lo)) for f in FRACS]


@pytest.fixture(scope="module")
def host_frozen(pair):
    """the reference: host analysis, host freeze, at every budget"""
    host, (lo, hi), _, _, _ = pair
    return {budget: host.freeze(budget) for budget in _budgets(lo, hi)}


@pytest.mark.parametrize("analysed_on,frozen_on", [("gpu", "gpu"), ("gpu", "host"), ("host", "gpu")])
def test_images_equal(pair, host_frozen, analysed_on, frozen_on):
    host, _, dev, _, _ = pair
    hb = dev if analysed_on == "gpu" else host
    for budget, (img, info) in host_frozen.items():
        gimg, ginfo = hb.freeze(budget, device=0 if frozen_on == "gpu" else None)
        assert gimg == img, budget
        assert _same_info(ginfo, info), (budget, ginfo, info)
        if frozen_on == "gpu":
            assert ginfo["device_ms"] > 0


def test_freeze_analyses_on_the_device_first(coll, profile, pair, host_frozen):
    hb = _builder(coll.num_docs, coll.lists, profile, _model(pair[4]))
    lo, hi = pair[1]
    budget = int(lo + 0.5 * (hi - lo))
    img, info = hb.freeze(budget, device=0)
    assert img == host_frozen[budget][0] and _same_info(info, host_frozen[budget][1])
    assert hb.hull(3, 0, 0).tobytes() == pair[0].hull(3, 0, 0).tobytes()


def test_the_images_hold_several_block_types(pair, host_frozen):
    """The comparisons above are worth what the images hold. Under the MI355X model half the budget range already buys OptPFor
    for every block of this collection (host path, any counters: each part's hull is OptPFor from its second point on), so that
    model is held to two types at a tenth of the range (interpolative + OptPFor) and the cheap-varint model at half of it
    (OptPFor + VarInt-G8IU): together the three writers."""
    lo, hi = pair[1]
    f, types = (0.1, (0, 2)) if pair[4] == "mi355x" else (0.5, (0, 1))
    tc = host_frozen[int(lo + f * (hi - lo))][1]["type_counts"]
    for t in types:
        assert tc["docs"][t] + tc["freqs"][t] >= 20, (pair[4], f, tc)


@pytest.mark.parametrize("frac", [0.1, 0.5])
def test_gpu_frozen_image_answers_queries(coll, queries, pair, frac):
    _, (lo, hi), dev, _, _ = pair
    img, _ = dev.freeze(int(lo + frac * (hi - lo)), device=0)
    wand = coll.wand_image()
    mixed = d.Index("block_mixed", img, wand)
    ref = d.Index("block_optpfor", coll.index_image("block_optpfor"), wand)
    for t in (0, 299):
        dd, ff = mixed[t]
        assert np.array_equal(dd, coll.lists[t][0]) and np.array_equal(ff, coll.lists[t][1])
    assert np.array_equal(mixed.query_batch("and", queries)[0], ref.query_batch("and", queries)[0])
    _, topk, tlen, _ = mixed.query_batch("ranked_and", queries, k=10)
    _, rtopk, rtlen, _ = ref.query_batch("ranked_and", queries, k=10)
    assert np.array_equal(tlen, rtlen) and topk.tobytes() == rtopk.tobytes()


# ---------------------------------------------------------------- errors
def test_errors(coll):
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_encode_index(coll.num_docs, coll.lists[:3], codec="block_qmx")
    assert e.value.code == -1
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_encode_index(coll.num_docs, coll.lists[:3], codec="block_mixed")
    assert e.value.code == -1
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_encode_index(coll.num_docs, coll.lists[:3], device=99, codec="block_varint")
    assert e.value.code == -4
    hb = _builder(coll.num_docs, coll.lists[:3], None)
    with pytest.raises(d.Ds2iError) as e:
        hb.analyse(device=99)
    assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        hb.freeze(device=99)
    assert e.value.code == -4
    lo, _ = hb.analyse(device=0)
    with pytest.raises(d.Ds2iError) as e:  # as the host path: "budget below the smallest possible index"
        hb.freeze(lo - 1, device=0)
    assert e.value.code == -1


def test_empty_builder_behaves_as_on_the_host(coll):
    host, dev = d.HybridBuilder(coll.num_docs), d.HybridBuilder(coll.num_docs)
    assert dev.analyse(device=0) == host.analyse() == (0, 0)
    img, info = host.freeze()
    gimg, ginfo = dev.freeze(device=0)
    assert gimg == img and _same_info(ginfo, info)
