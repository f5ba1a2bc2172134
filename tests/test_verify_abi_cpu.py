"""Index verification on a CPU-only box: the two symbols are exported and declared, the argument checks and the structure
comparison (number of documents, number of lists, list lengths) answer before any device is touched, and the tool's new flags
parse, refuse and report as documented."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
from ds2i_amd.api import VerifyReport, _csr
import verify_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "create_freq_index")
ARGS = {"ds2i_hip_index_verify": 8, "ds2i_hip_verify_collection": 11}
NO_DEVICE = 99


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_are_exported_and_declared(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds2i_hip.h")).read(), flags=re.S)
    for name, nargs in ARGS.items():
        assert hasattr(built_lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        assert len(getattr(built_lib, name).argtypes) == nargs
    assert "typedef struct ds2i_hip_verify_report" in src
    for i, name in enumerate(("OK", "NUM_DOCS", "LISTS", "LENGTH", "DOCID", "FREQ")):
        assert re.search(r"DS2I_VERIFY_%s\s*=\s*%d\b" % (name, i), src), name
    assert d.gpu_verify_collection and d.Index.verify


@pytest.fixture(scope="module")
def edge(built_lib):
    coll, names = cases.block_edge_collection()
    return coll, names


def _verify(L, kind, img, num_docs, lists, device=NO_DEVICE):
    n, offs, docs, freqs = _csr(lists)
    r, ms = VerifyReport(), C.c_double(-1.0)
    rc = L.ds2i_hip_verify_collection(device, d.CODECS[kind], img, len(img), num_docs, n, _p(offs), _p(docs), _p(freqs), C.byref(r), C.byref(ms))
    return rc, r, ms.value


def test_argument_checks(built_lib, edge):
    L = built_lib
    coll, _ = edge
    img = cases.image(coll, "block_optpfor")
    n, offs, docs, freqs = _csr(coll.lists)
    r = VerifyReport()
    call = lambda kind, image, o, dd, ff, rep: L.ds2i_hip_verify_collection(NO_DEVICE, kind, image, len(img), coll.num_docs, n, o, dd, ff, rep, None)
    assert call(0, None, _p(offs), _p(docs), _p(freqs), C.byref(r)) == -1
    assert call(0, img, None, _p(docs), _p(freqs), C.byref(r)) == -1
    assert call(0, img, _p(offs), None, _p(freqs), C.byref(r)) == -1
    assert call(0, img, _p(offs), _p(docs), None, C.byref(r)) == -1
    assert call(0, img, _p(offs), _p(docs), _p(freqs), None) == -1
    assert call(9, img, _p(offs), _p(docs), _p(freqs), C.byref(r)) == -1 and b"unknown index kind" in L.ds2i_hip_last_error()
    assert call(-1, img, _p(offs), _p(docs), _p(freqs), C.byref(r)) == -1
    down = offs.copy()
    down[3] = down[2] - 1
    assert call(0, img, _p(down), _p(docs), _p(freqs), C.byref(r)) == -1 and b"decrease" in L.ds2i_hip_last_error()
    late = offs.copy()
    late[0] = 1
    assert call(0, img, _p(late), _p(docs), _p(freqs), C.byref(r)) == -1
    # the handle form: a null handle (its null arrays need a handle: test_gpu_verify.py)
    assert L.ds2i_hip_index_verify(None, coll.num_docs, n, _p(offs), _p(docs), _p(freqs), C.byref(r), None) == -1


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_garbage_image_is_a_format_error(built_lib, kind):
    """-2 (DS2I_EFORMAT) is the code ds2i_hip_index_open gives ten garbage bytes; here the image is parsed on the host before a
    device is looked for, so the code comes back without one (test_gpu_verify.py holds the two calls against each other)"""
    coll, _ = cases.block_edge_collection()
    rc, _, _ = _verify(built_lib, kind, cases.GARBAGE, coll.num_docs, coll.lists)
    assert rc == -2


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_structure_reports_come_before_the_device(built_lib, edge, kind):
    L = built_lib
    coll, _ = edge
    img = cases.image(coll, kind)
    lists, N, V = coll.lists, coll.num_docs, len(coll.lists)
    lens = [len(dd) for dd, _ in lists]
    total = sum(lens)

    def report(num_docs, ls):
        rc, r, ms = _verify(L, kind, img, num_docs, ls)
        assert rc == 0 and ms == 0.0
        return (cases.WHAT[r.what], r.list, r.position, r.got, r.expected, r.postings_checked)

    assert report(N + 1, lists) == ("num_docs", 0, 0, N, N + 1, 0)
    assert report(N - 1, lists) == ("num_docs", 0, 0, N, N - 1, 0)
    assert report(N, lists[:-1]) == ("lists", 0, 0, V, V - 1, 0)
    assert report(N, lists + [lists[0]]) == ("lists", 0, 0, V, V + 1, 0)
    shorter = list(lists)
    shorter[3] = (lists[3][0][:-1], lists[3][1][:-1])
    assert report(N, shorter) == ("length", 3, 0, lens[3], lens[3] - 1, sum(lens[:3]))
    longer = list(lists)
    longer[-1] = (np.append(lists[-1][0][:-1], [N - 2, N - 1]), np.append(lists[-1][1], 1))
    assert report(N, longer) == ("length", V - 1, 0, lens[-1], lens[-1] + 1, total - lens[-1])
    # num_docs is looked at before the lists, the number of lists before their lengths
    assert report(N + 1, shorter[:-1])[0] == "num_docs" and report(N, shorter[:-1])[0] == "lists"
    # a pair that matches in structure goes on to the device, and there is none
    rc, r, _ = _verify(L, kind, img, N, lists)
    assert rc == -4 and b"no such HIP device" in L.ds2i_hip_last_error()
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_verify_collection(kind, img, N, lists, device=NO_DEVICE)
    assert e.value.code == -4
    assert d.gpu_verify_collection(kind, img, N, shorter, device=NO_DEVICE) == dict(
        ok=False, what="length", list=3, position=0, got=lens[3], expected=lens[3] - 1, postings_checked=sum(lens[:3]), device_ms=0.0)


@pytest.fixture(scope="module")
def tool_files(built_lib, tmp_path_factory):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])
    coll, _ = cases.block_edge_collection()
    base = str(tmp_path_factory.mktemp("verify") / "edge")
    cases.write_collection(base, coll.num_docs, coll.lists, coll.sizes)
    idx = base + ".block_optpfor"
    subprocess.check_call([TOOL, "block_optpfor", base, idx], stderr=subprocess.DEVNULL)
    assert open(idx, "rb").read() == cases.image(coll, "block_optpfor")
    return coll, base, idx


def _run(*args):
    p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    return p.returncode, p.stdout, p.stderr


def test_tool_check_only_without_a_device_is_an_error(tool_files):
    _, base, idx = tool_files
    rc, out, err = _run("block_optpfor", base, idx, "--check-only", "--device", str(NO_DEVICE))
    assert rc == 2 and out == "" and "no such HIP device" in err
    rc, out, err = _run("block_optpfor", "--device", str(NO_DEVICE), "--check-only", base, idx)  # flags in any place
    assert rc == 2 and "no such HIP device" in err


def test_tool_reports_a_length_mismatch_without_a_device(tool_files, tmp_path):
    coll, _, idx = tool_files
    lists = list(coll.lists)
    lists[2] = (lists[2][0][:-1], lists[2][1][:-1])
    base = str(tmp_path / "shorter")
    cases.write_collection(base, coll.num_docs, lists, coll.sizes)
    rc, out, _ = _run("block_optpfor", base, idx, "--check-only", "--device", str(NO_DEVICE))
    n = len(coll.lists[2][0])
    assert rc == 1 and out == "MISMATCH length list=2 got=%d expected=%d\n" % (n, n - 1)


def test_tool_refuses_gpu_for_kinds_without_an_encoder(tool_files, tmp_path):
    _, base, _ = tool_files
    for kind in ("block_qmx", "block_mixed"):
        out_path = str(tmp_path / kind)
        rc, out, err = _run(kind, base, out_path, "--gpu")
        assert rc == 2 and not os.path.exists(out_path)
        for name in cases.GPU_BUILT_KINDS:
            assert name in err
    rc, _, err = _run("block_optpfor", base, str(tmp_path / "x"), "--no-such-flag")
    assert rc == 2 and "usage" in err
    rc, _, err = _run("block_optpfor", base, str(tmp_path / "x"), "--check-only", "--device", "x")  # not a number: never device 0
    assert rc == 2 and "usage" in err
    # an unknown type with a check asked for is an error, not a success without a verification
    assert _run("no_such_type", base, str(tmp_path / "x"), "--check-only")[0] == 2
    assert _run("no_such_type", base, str(tmp_path / "x"), "--check")[0] == 2
