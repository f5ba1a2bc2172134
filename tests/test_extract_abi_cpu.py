"""Extraction and conversion on a CPU-only box: the three symbols are exported and declared, and every answer that needs no device
comes back without one -- the argument checks, the refusal of a target kind the GPU encoder does not write (before the image is
read), the host parse of the image (a garbage image gets ds2i_hip_index_open's code), and only then the missing device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import ds2i_amd as d
import verify_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "convert_index")
ARGS = {"ds2i_hip_index_extract": 9, "ds2i_hip_extract_collection": 10, "ds2i_hip_convert_index": 7}
NO_DEVICE = 99


def test_symbols_are_exported_and_declared(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds2i_hip.h")).read(), flags=re.S)
    for name, nargs in ARGS.items():
        assert hasattr(built_lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        assert len(getattr(built_lib, name).argtypes) == nargs
    assert d.gpu_extract_collection and d.gpu_convert_index and d.Index.extract


class Outputs:
    """the outputs of ds2i_hip_extract_collection, and whether any was written"""

    def __init__(self):
        self.num_docs, self.nlists, self.ms = C.c_uint64(0), C.c_uint64(0), C.c_double(-1.0)
        self.blobs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]

    def args(self, skip=None):
        a = [C.byref(self.num_docs), C.byref(self.nlists)] + [C.byref(b) for b in self.blobs]
        if skip is not None:
            a[skip] = None
        return a + [C.byref(self.ms)]

    def untouched(self):
        return not any(b.value for b in self.blobs) and self.num_docs.value == 0 and self.nlists.value == 0


def extract(L, kind, img, device=NO_DEVICE, skip=None, image_null=False):
    o = Outputs()
    rc = L.ds2i_hip_extract_collection(device, kind, None if image_null else img, len(img), *o.args(skip))
    assert o.untouched()
    return rc


def convert(L, from_kind, img, to_kind, device=NO_DEVICE, image_null=False, out_null=False):
    h = C.c_void_p()
    rc = L.ds2i_hip_convert_index(device, from_kind, None if image_null else img, len(img), to_kind, None if out_null else C.byref(h), None)
    assert not h.value
    return rc


@pytest.fixture(scope="module")
def image(built_lib):
    coll, _ = cases.block_edge_collection()
    return cases.image(coll, "block_optpfor")


def test_null_arguments(built_lib, image):
    L = built_lib
    assert extract(L, 0, image, image_null=True) == -1
    for skip in range(5):  # num_docs, nlists, the three blobs (device_ms may be null)
        assert extract(L, 0, image, skip=skip) == -1 and b"null argument" in L.ds2i_hip_last_error()
    assert convert(L, 0, image, 0, image_null=True) == -1
    assert convert(L, 0, image, 0, out_null=True) == -1
    # the handle form: a null handle (its other arguments need a handle: test_gpu_extract.py)
    offs, n = (C.c_uint64 * 4)(), C.c_uint64(7)
    assert L.ds2i_hip_index_extract(None, 0, 0, offs, None, None, 0, C.byref(n), None) == -1 and n.value == 7


def test_unknown_kinds(built_lib, image):
    L = built_lib
    for kind in (-1, 9, 99):
        assert extract(L, kind, image) == -1 and b"unknown index kind" in L.ds2i_hip_last_error()
        assert convert(L, kind, image, 0) == -1 and b"unknown index kind" in L.ds2i_hip_last_error()
        assert convert(L, 0, image, kind) == -1


@pytest.mark.parametrize("to_kind", ["block_qmx", "block_mixed"])
def test_targets_without_an_encoder_are_refused_before_the_image_is_read(built_lib, image, to_kind):
    L = built_lib
    for img in (image, cases.GARBAGE):  # (a garbage image would be -2 once parsed)
        assert convert(L, 0, img, d.CODECS[to_kind]) == -1
        for name in cases.GPU_BUILT_KINDS:
            assert name.encode() in L.ds2i_hip_last_error()


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_garbage_image_is_a_format_error(built_lib, kind):
    """-2 (DS2I_EFORMAT) is the code ds2i_hip_index_open gives ten garbage bytes (test_gpu_verify.py holds that call); here the
    image is parsed on the host before a device is looked for, so the code comes back without one"""
    assert extract(built_lib, d.CODECS[kind], cases.GARBAGE) == -2
    assert convert(built_lib, d.CODECS[kind], cases.GARBAGE, d.CODECS["block_optpfor"]) == -2
    assert convert(built_lib, d.CODECS[kind], cases.GARBAGE, d.CODECS["opt"]) == -2


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_a_good_image_goes_on_to_the_device_and_there_is_none(built_lib, kind):
    L = built_lib
    coll, _ = cases.block_edge_collection()
    img = cases.image(coll, kind)
    assert extract(L, d.CODECS[kind], img) == -4 and b"no such HIP device" in L.ds2i_hip_last_error()
    assert convert(L, d.CODECS[kind], img, d.CODECS["block_varint"]) == -4 and b"no such HIP device" in L.ds2i_hip_last_error()
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_extract_collection(kind, img, device=NO_DEVICE)
    assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_convert_index(kind, img, "opt", device=NO_DEVICE)
    assert e.value.code == -4
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_convert_index(kind, img, "block_mixed", device=NO_DEVICE)
    assert e.value.code == -1


def test_tool_usage_and_errors_without_a_device(built_lib, image, tmp_path):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])

    def run(*args):
        p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return p.returncode, p.stdout, p.stderr

    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    open(src, "wb").write(image)
    rc, _, err = run()
    assert rc == 2 and "usage" in err and ".sizes" in err
    assert run("no_such_type", src, "opt", out)[0] == 2
    assert run("block_optpfor", src, "no_such_type", out)[0] == 2
    assert run("no_such_type", src, "--dump", out)[0] == 2
    assert run("block_optpfor", src, "opt", out, "--no-such-flag")[0] == 2
    assert run("block_optpfor", src, "opt", out, "--device", "x")[0] == 2
    assert run("block_optpfor", src, "--dump", out, "--check")[0] == 2
    rc, _, err = run("block_optpfor", src, "block_qmx", out)
    assert rc == 2 and all(name in err for name in cases.GPU_BUILT_KINDS)
    rc, stdout, err = run("block_optpfor", src, "opt", out, "--device", str(NO_DEVICE))
    assert rc == 2 and stdout == "" and "no such HIP device" in err
    rc, _, err = run("block_optpfor", src, "--dump", out, "--device", str(NO_DEVICE))
    assert rc == 2 and "no such HIP device" in err
    assert not os.path.exists(out) and not os.path.exists(out + ".docs")
