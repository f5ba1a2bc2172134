"""bench.py --dump-outputs without a GPU: the writer's file names, dtypes and its 64 MB cap (a fixed, seeded sample of the
queries above it, their batch positions in rows.npy)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _answer(nq, k, seed=1):
    rng = np.random.default_rng(seed)
    count = rng.integers(0, 1 << 40, nq, dtype=np.uint64)
    tlen = rng.integers(0, k + 1, nq).astype(np.uint32)
    topk = np.full((nq, k), -np.inf, dtype=np.float32)
    for i, t in enumerate(tlen):
        topk[i, :t] = np.sort(rng.random(t).astype(np.float32))[::-1]
    return count, topk, tlen


def _padded_with_zeros(topk, tlen):
    return np.where(np.arange(topk.shape[1])[None, :] < tlen[:, None], topk, 0).astype(np.float32)


def test_dump_whole_answer(tmp_path):
    count, topk, tlen = _answer(300, 10)
    assert (tlen < 10).any() and (tlen == 0).any()  # rows padded with -inf, whole rows of it included
    bench.dump_outputs(str(tmp_path / "d"), (count, topk, tlen), True, None, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["count.npy", "tlen.npy", "topk.npy"]
    c, t, n = (np.load(tmp_path / "d" / (x + ".npy")) for x in ("count", "topk", "tlen"))
    assert c.dtype == np.float64 and t.dtype == np.float32 and n.dtype == np.float64
    assert np.isfinite(c).all() and np.isfinite(t).all() and np.isfinite(n).all()
    assert np.array_equal(c.astype(np.uint64), count) and np.array_equal(n, tlen)
    valid = np.arange(10)[None, :] < tlen[:, None]
    assert np.array_equal(t[valid], topk[valid]) and not t[~valid].any()


def test_dump_counting_operator(tmp_path):
    """and / or return no top-k: count.npy alone."""
    count, topk, tlen = _answer(300, 10)
    topk[:] = -np.inf
    bench.dump_outputs(str(tmp_path / "d"), (count, topk, tlen), False, None, 0, 1)
    assert os.listdir(tmp_path / "d") == ["count.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "count.npy").astype(np.uint64), count)


def test_dump_samples_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 64 << 10)
    count, topk, tlen = _answer(5000, 16)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), (count, topk, tlen), True, None, 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["count.npy", "rows.npy", "tlen.npy", "topk.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in files) <= 64 << 10  # 128: the .npy header
    rows = np.load(tmp_path / "a" / "rows.npy")
    r = rows.astype(np.int64)
    assert rows.dtype == np.float64 and len(r) > 100 and np.all(np.diff(r) > 0) and r[-1] < 5000
    assert np.array_equal(np.load(tmp_path / "a" / "topk.npy"), _padded_with_zeros(topk, tlen)[r])
    assert np.array_equal(np.load(tmp_path / "a" / "count.npy").astype(np.uint64), count[r])
    for f in files:  # the same sample every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
