"""The partition planner of the opt layout on a CPU-only box: ds2i_opt_partition (the host DP over a CSR collection, the reference of
the device planner) returns well-formed end points that are the ones the host-built image holds, and ds2i_hip_opt_partition /
ds2i_hip_encode_index_with check their input on the host, before anything is staged or any device is touched."""
import ctypes as C

import numpy as np
import pytest

import ds2i_amd as d
import opt_partition_cases as cases


@pytest.mark.parametrize("name", ["window", "edge", "dense"])
def test_end_points_are_well_formed(built_lib, name):
    coll = cases.COLLECTIONS[name]()
    parts = cases.host_partitions(name)
    V = len(coll.lists)
    for side in (0, 1):
        ends, offs = parts[2 * side], parts[2 * side + 1]
        assert ends.dtype == np.uint32 and offs.dtype == np.uint64
        assert len(offs) == V + 1 and int(offs[0]) == 0 and int(offs[-1]) == len(ends)
        for t, (docs, _) in enumerate(coll.lists):
            e = cases.ends_of(parts, side, t).astype(np.int64)
            assert len(e) >= 1 and int(e[-1]) == len(docs), (side, t)
            assert int(e[0]) >= 1 and np.all(np.diff(e) > 0), (side, t)
            if len(docs) == 1:
                assert e.tolist() == [1], (side, t)


def test_the_window_lists_are_what_their_names_say(built_lib):
    coll, names = cases.window_collection()
    parts = cases.host_partitions("window")
    docs, freqs = coll.lists[names["long_run"]]
    assert len(docs) == 6000 and int(docs[-1] - docs[0]) + 1 == 6000 and int(freqs.max()) == 1
    for side in (0, 1):  # one partition, all ones, on both sides: the window never closes
        assert cases.ends_of(parts, side, names["long_run"]).tolist() == [6000]
    docs, _ = coll.lists[names["run_in_sparse"]]
    assert len(docs) == 4000 and np.all(np.diff(docs[500:3500].astype(np.int64)) == 1)
    assert len(coll.lists[names["long"]][0]) == 70000 > 1 << 16
    for m in cases.WINDOW_LENGTHS:
        assert len(coll.lists[names["len%d" % m]][0]) == m
    assert len(coll.lists[names["few_classes"]][0]) == 3
    docs, _ = coll.lists[names["clusters"]]
    assert len(docs) == 8000
    e = cases.ends_of(parts, 0, names["clusters"]).astype(np.int64)
    sizes = np.diff(np.concatenate([[0], e]))
    assert len(e) > 20 and len(set(sizes.tolist())) >= 5, (len(e), sorted(set(sizes.tolist())))


def test_end_points_are_chunk_boundaries_of_the_host_image(built_lib):
    """a chunk of the upload directory (opt_list_directory) never crosses a partition of either side: every end point the planner
    returns must be where a chunk of the HOST-built image ends"""
    coll = cases.small_collection()
    parts = cases.host_partitions("small")
    opt = coll.index_image("opt")
    seen = 0
    for t in range(0, len(coll.lists), 7):
        _, chunks, info = d.opt_list_directory(opt, t)
        assert info[0] == len(coll.lists[t][0])
        boundaries = set((chunks[:, 0].astype(np.int64) + (chunks[:, 1] & 0xFF)).tolist())
        for side in (0, 1):
            e = cases.ends_of(parts, side, t).tolist()
            assert set(e) <= boundaries, (t, side, sorted(set(e) - boundaries)[:5])
            seen += len(e)
    assert seen > 100


def test_host_side_checks_come_before_the_device(built_lib):
    L = built_lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    offs = np.array([0, 3], dtype=np.uint64)
    good_docs, good_freqs = np.array([1, 4, 9], dtype=np.uint32), np.array([1, 2, 1], dtype=np.uint32)
    bad = {b"doc id out of range": (offs, np.array([1, 4, 10], dtype=np.uint32), good_freqs),
           b"not strictly increasing": (offs, np.array([4, 4, 9], dtype=np.uint32), good_freqs),
           b"zero freq": (offs, good_docs, np.array([1, 0, 1], dtype=np.uint32)),
           b"List must be nonempty": (np.array([0, 0], dtype=np.uint64), good_docs, good_freqs)}
    hs = [C.c_void_p() for _ in range(4)]
    outs = [C.byref(h) for h in hs]
    h, ms = C.c_void_p(), C.c_double(-7.0)
    kind = d.CODECS["opt"]
    for device in (0, 99):  # the answer is the input's, whatever the device
        for text, (of, docs, freqs) in bad.items():
            assert L.ds2i_hip_opt_partition(device, 10, 1, p(of), p(docs), p(freqs), 0, *outs, C.byref(ms)) == -1, text
            assert text in L.ds2i_hip_last_error(), (text, L.ds2i_hip_last_error())
            for flags in (0, 1, 2):
                assert L.ds2i_hip_encode_index_with(device, kind, 10, 1, p(of), p(docs), p(freqs), flags, C.byref(h), C.byref(ms)) == -1, text
                assert text in L.ds2i_hip_last_error(), (text, L.ds2i_hip_last_error())
        # null arguments
        assert L.ds2i_hip_opt_partition(device, 10, 1, p(offs), p(good_docs), None, 0, *outs, C.byref(ms)) == -1
        assert b"null argument" in L.ds2i_hip_last_error()
        assert L.ds2i_hip_opt_partition(device, 10, 1, p(offs), p(good_docs), p(good_freqs), 0, outs[0], outs[1], outs[2], None,
                                        C.byref(ms)) == -1
        assert b"null argument" in L.ds2i_hip_last_error()
        assert L.ds2i_hip_encode_index_with(device, kind, 10, 1, p(offs), p(good_docs), p(good_freqs), 2, None, C.byref(ms)) == -1
        assert b"null argument" in L.ds2i_hip_last_error()
        # both planners at once, for a kind with a DP and for one without
        for k in (kind, d.CODECS["ef"], d.CODECS["block_optpfor"]):
            assert L.ds2i_hip_encode_index_with(device, k, 10, 1, p(offs), p(good_docs), p(good_freqs), 3, C.byref(h), C.byref(ms)) == -1
            assert b"both planners" in L.ds2i_hip_last_error()
    assert h.value is None and all(x.value is None for x in hs) and ms.value == -7.0


def test_the_host_entry_point_checks_its_input(built_lib):
    with pytest.raises(d.Ds2iError) as e:
        d.opt_partition(10, [(np.array([4, 4], np.uint32), np.array([1, 1], np.uint32))])
    assert e.value.code == -1 and "not strictly increasing" in str(e.value)
    with pytest.raises(d.Ds2iError) as e:
        d.opt_partition(10, [(np.array([4, 5], np.uint32), np.array([1, 0], np.uint32))])
    assert e.value.code == -1 and "zero freq" in str(e.value)
    de, do, fe, fo = d.opt_partition(10, [(np.array([7], np.uint32), np.array([3], np.uint32))])
    assert de.tolist() == [1] and fe.tolist() == [1] and do.tolist() == [0, 1] and fo.tolist() == [0, 1]
