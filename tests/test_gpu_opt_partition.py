"""The partition DP of the opt layout on the GPU (-m gpu): ds2i_hip_opt_partition against ds2i_opt_partition (the host DP), and
ds2i_hip_encode_index_with's two planners against the host builder. Everything is integers: every comparison is == (np.array_equal
on the end points, == on image bytes), there is no tolerance."""
import numpy as np
import pytest

import ds2i_amd as d
import opt_partition_cases as cases

pytestmark = pytest.mark.gpu

NAMES = ("docs_ends", "docs_offs", "freqs_ends", "freqs_offs")


def assert_same_partitions(got, want, coll):
    for side in (0, 1):
        for t in range(len(coll.lists)):
            g, w = cases.ends_of(got, side, t), cases.ends_of(want, side, t)
            if not np.array_equal(g, w):
                m = min(len(g), len(w))
                bad = np.flatnonzero(g[:m] != w[:m])
                at = int(bad[0]) if len(bad) else m
                print("first difference: list %d (%d postings), side %d, position %d: device %s (%d ends), host %s (%d ends)"
                      % (t, len(coll.lists[t][0]), side, at, g[at:at + 4].tolist(), len(g), w[at:at + 4].tolist(), len(w)))
                break
        else:
            continue
        break
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.parametrize("name", ["window", "edge", "dense", "small"])
def test_device_end_points_equal_the_hosts(built_lib, name):
    coll = cases.COLLECTIONS[name]()
    assert_same_partitions(d.gpu_opt_partition(coll.num_docs, coll.lists), cases.host_partitions(name), coll)


def groups_at(coll, scratch_bytes):
    """the planner's grouping rule: consecutive lists while 12 bytes x (n + 1) x 2 sides of each fit, at least one list"""
    groups, cur = 0, None
    for docs, _ in coll.lists:
        need = 24 * (len(docs) + 1)
        if cur is None or cur + need > scratch_bytes:
            groups, cur = groups + 1, need
        else:
            cur += need
    return groups


@pytest.mark.parametrize("scratch_bytes", [1 << 20, 1])
def test_forced_scratch_grouping(built_lib, scratch_bytes):
    """1 MiB: the window lists fall into several groups (the 70 000-posting list alone exceeds it); 1 byte: every list is a group"""
    coll = cases.COLLECTIONS["window"]()
    groups = groups_at(coll, scratch_bytes)
    assert groups == len(coll.lists) if scratch_bytes == 1 else 3 <= groups < len(coll.lists)
    assert_same_partitions(d.gpu_opt_partition(coll.num_docs, coll.lists, scratch_bytes=scratch_bytes), cases.host_partitions("window"), coll)


@pytest.mark.parametrize("name", ["window", "small"])
def test_both_planners_build_the_host_image(built_lib, name):
    coll = cases.COLLECTIONS[name]()
    host = coll.index_image("opt")
    by_device, ms = d.gpu_encode_index(coll.num_docs, coll.lists, codec="opt", plan="device")
    plan_ms = d.encode_plan_ms()
    assert by_device == host
    assert 0 < plan_ms <= ms
    by_host, _ = d.gpu_encode_index(coll.num_docs, coll.lists, codec="opt", plan="host")
    assert d.encode_plan_ms() == 0.0
    assert by_host == host
    by_default, _ = d.gpu_encode_index(coll.num_docs, coll.lists, codec="opt")
    assert by_default == host
    ef, _ = d.gpu_encode_index(coll.num_docs, coll.lists, codec="ef", plan="device")  # no DP: the flag is ignored
    assert d.encode_plan_ms() == 0.0
    assert ef == coll.index_image("ef")


def test_build_collection_and_convert_take_the_planner(built_lib):
    """whichever planner is the default, the one-call build and the conversion return the host builder's opt image"""
    coll = cases.COLLECTIONS["small"]()
    host = coll.index_image("opt")
    index, _, _ = d.gpu_build_collection(coll.num_docs, coll.sizes, coll.lists, codec="opt")
    assert index == host
    converted, _ = d.gpu_convert_index("block_optpfor", coll.index_image("block_optpfor"), "opt")
    assert converted == host


def test_errors(built_lib):
    coll = cases.COLLECTIONS["small"]()
    some = coll.lists[:3]
    zero = some + [(np.array([5, 9], np.uint32), np.array([1, 0], np.uint32))]
    unsorted = some + [(np.array([9, 5], np.uint32), np.array([1, 1], np.uint32))]
    for lists in (zero, unsorted):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_opt_partition(coll.num_docs, lists)
        assert e.value.code == -1
        for plan in ("host", "device"):
            with pytest.raises(d.Ds2iError) as e:
                d.gpu_encode_index(coll.num_docs, lists, codec="opt", plan=plan)
            assert e.value.code == -1
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_opt_partition(coll.num_docs, some, device=99)
    assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_encode_index(coll.num_docs, some, device=99, codec="opt", plan="device")
    assert e.value.code == -4
