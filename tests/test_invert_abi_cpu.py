"""Indexing documents on a CPU-only box: the host twins of the inversion and the transposition against the numpy references,
transpose(transpose(x)) == x, and every answer of the entry points that needs no device, in the order the headers state: null arguments
and the offsets, 2^32 documents or terms, a document of 2^32 tokens, then a token outside the terms (the twins) or the missing device
(the device forms)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ds2i_amd as d
import invert_cases as ic
import remap_cases as rc
import verify_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ds2i_amd", "tools", "index_documents")
NO_DEVICE = 99
HIP_ARGS = {"ds2i_hip_invert_postings": 10, "ds2i_hip_transpose_postings": 10, "ds2i_hip_invert_documents": 11, "ds2i_hip_forward_index": 10}
BUILD_ARGS = {"ds2i_invert_documents": 9, "ds2i_transpose_postings": 9}


def test_symbols_are_exported_and_declared(built_lib):
    for header, table in (("ds2i_hip.h", HIP_ARGS), ("ds2i_build.h", BUILD_ARGS)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name, nargs in table.items():
            assert hasattr(built_lib, name), name
            decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
            assert decl, name
            assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
            assert len(getattr(built_lib, name).argtypes) == nargs
    src = open(os.path.join(ROOT, "include", "ds2i_hip.h")).read()
    assert re.search(r"\bvoid\s+ds2i_hip_invert_ms\s*\(", src) and re.search(r"\buint32_t\s+ds2i_hip_invert_window\s*\(", src)
    assert hasattr(built_lib, "ds2i_hip_invert_ms") and hasattr(built_lib, "ds2i_hip_invert_window")
    assert d.invert_documents and d.transpose_postings and d.gpu_invert_postings and d.gpu_transpose_postings
    assert d.gpu_invert_documents and d.gpu_forward_index and d.Index.forward
    V = d.invert_window()
    assert V > 0 and V % 64 == 0


# ---------------------------------------------------------------- the host twins
def edge_inputs():
    """(name, (doc_offsets, tokens), nterms) of every edge input of invert_cases"""
    V, bounds = d.invert_window(), d.remap_class_bounds()
    yield "small", ic.small_edges(), ic.NTERMS_SMALL
    yield "lengths", ic.length_edge_documents(bounds)[1], 300
    for whole in (False, True):
        _, docs, nterms = ic.run_edge_documents(V, whole)
        yield "runs %s" % whole, docs, nterms
    for name, make in (("every", ic.every_document_case), ("past docs", ic.past_2_24_documents), ("past terms", ic.past_2_24_terms)):
        o, t, nterms = make()
        yield name, (o, t), nterms


def test_inversion_twin_equals_numpy_on_the_edge_inputs(built_lib):
    for name, (o, t), nterms in edge_inputs():
        want = ic.numpy_invert(o, t, nterms)
        ic.assert_csr_equal(d.invert_documents((o, t), nterms), want, name)
        ic.assert_csr_equal(d.invert_documents((o, t), nterms, threads=3), want, name)
        assert np.all(np.diff(want[0].astype(np.int64)) >= 0) and int(want[2].sum()) == len(t) == int(want[3].sum())


def test_the_small_edges_are_what_they_claim(built_lib):
    o, t = ic.small_edges()
    offs, docs, freqs, sizes = d.invert_documents([t[int(a):int(b)] for a, b in zip(o, o[1:])], ic.NTERMS_SMALL)  # (a list of arrays)
    assert sizes.tolist() == [0, 1, 4, 0, 5, 3, 0, 6, 0]
    lists = [(docs[int(a):int(b)].tolist(), freqs[int(a):int(b)].tolist()) for a, b in zip(offs, offs[1:])]
    assert lists[7] == ([2], [4]) and lists[4] == ([], []) and lists[9] == ([], [])
    assert lists[11] == ([4, 5], [2, 2])  # two neighbours that end and begin with the same term: both postings, each its own freq
    assert lists[0] == ([4], [2]) and lists[1] == ([7], [3])
    runs, (o, t), nterms = ic.run_edge_documents(d.invert_window(), False)
    offs, docs, freqs, _ = d.invert_documents((o, t), nterms)
    for doc, term, n in runs:  # every document of the run edges is one posting of its term, freq = its length
        at = int(offs[term]) + int(np.searchsorted(docs[int(offs[term]):int(offs[term + 1])], doc))
        assert docs[at] == doc and freqs[at] == n, (doc, term, n)
    assert int(offs[ic.RUN_TERM + 1] - offs[ic.RUN_TERM]) == 4


@pytest.mark.parametrize("which", ["small", "block_edge"])
def test_a_collection_written_as_documents_comes_back(built_lib, which):
    coll = rc.small_collection() if which == "small" else rc.block_edge_collection()
    o, t = ic.forward_of(coll)
    got = d.invert_documents((o, t), len(coll.lists))
    ic.assert_csr_equal(got, ic.numpy_invert(o, t, len(coll.lists)))
    ic.assert_csr_equal(got[:3], ic.csr_of(coll))
    assert np.array_equal(got[3], ic.with_token_sizes(coll).sizes)


@pytest.mark.parametrize("which", ["small", "block_edge"])
def test_transposition_twin_and_its_involution(built_lib, which):
    coll = rc.small_collection() if which == "small" else rc.block_edge_collection()
    V, n = len(coll.lists), coll.num_docs
    lists = ic.csr_of(coll)
    fwd = d.transpose_postings(V, n, *lists)
    ic.assert_csr_equal(fwd, ic.numpy_transpose(V, n, *lists))
    ic.assert_csr_equal(d.transpose_postings(V, n, *lists, threads=5), fwd)
    ic.assert_csr_equal(d.transpose_postings(n, V, *fwd), lists)  # transpose(transpose(x)) == x
    assert which == "small" or np.any(np.diff(fwd[0].astype(np.int64)) == 0)  # (documents without a posting: empty rows)
    # inversion = canonicalise, then transpose: the expanded forward index inverts to the lists
    ic.assert_csr_equal(d.invert_documents(ic.expand(*fwd), V)[:3], lists)


def test_transposition_of_empty_rows_and_columns(built_lib):
    offs, cols, vals = np.array([0, 0, 2, 2, 3, 3], dtype=np.uint64), np.array([1, 4, 4], dtype=np.uint32), np.array([7, 8, 9], dtype=np.uint32)
    got = d.transpose_postings(5, 6, offs, cols, vals)
    assert got[0].tolist() == [0, 0, 1, 1, 1, 3, 3] and got[1].tolist() == [1, 1, 3] and got[2].tolist() == [7, 8, 9]
    ic.assert_csr_equal(d.transpose_postings(6, 5, *got), (offs, cols, vals))
    none = d.transpose_postings(0, 0, [0], [], [])
    assert none[0].tolist() == [0] and len(none[1]) == 0
    assert d.transpose_postings(3, 0, [0, 0, 0, 0], [], [])[0].tolist() == [0]
    empty = d.invert_documents([[], [], []], 2)
    assert empty[0].tolist() == [0, 0, 0] and empty[3].tolist() == [0, 0, 0]


# ---------------------------------------------------------------- refusals, without a device
def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


U64 = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
U32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731


def call(L, name, num_docs, offs, tokens, nterms, null=None, vals=None, kind=0):
    """(code, message) of one of the five CSR entry points, with argument `null` (a position among the pointers, inputs first) null; no
    output handle and no time is written on an error"""
    device = name.startswith("ds2i_hip_")
    transposition = "transpose" in name
    ins = [ptr(offs), ptr(tokens)] + ([ptr(tokens if vals is None else vals)] if transposition else [])
    nouts = 3 if transposition else 4
    hs = [C.c_void_p() for _ in range(nouts)]
    outs = [C.byref(h) for h in hs]
    if null is not None:
        both = ins + outs
        both[null] = None
        ins, outs = both[:len(ins)], both[len(ins):]
    ms = C.c_double(-1.0)
    head = ([NO_DEVICE] if device else []) + ([kind] if name == "ds2i_hip_invert_documents" else [])
    shape = [num_docs, nterms] if transposition else [num_docs]
    mid = ins if transposition else ins + [nterms]
    tail = [C.byref(ms)] if device else []
    if not device:
        mid = mid + [1]
    code = getattr(L, name)(*head, *shape, *mid, *outs, *tail)
    assert code != 0 and not any(h.value for h in hs) and ms.value == -1.0, name
    return code, L.ds2i_hip_last_error().decode()


INVERTERS = ("ds2i_invert_documents", "ds2i_hip_invert_postings", "ds2i_hip_invert_documents")
TRANSPOSERS = ("ds2i_transpose_postings", "ds2i_hip_transpose_postings")


def test_null_arguments_and_offsets_come_first(built_lib):
    L = built_lib
    o, t = ic.small_edges()
    for name in INVERTERS + TRANSPOSERS:
        nptrs = (2 if name in INVERTERS else 3) + (3 if name in TRANSPOSERS else 4)
        for null in range(nptrs):
            if name == "ds2i_hip_invert_documents" and null == 3:
                continue  # (wand_image may be NULL: no wand data is built)
            code, msg = call(L, name, 1 << 40, o, t, 1 << 40, null=null)  # (before the sizes)
            assert code == -1 and "null argument" in msg, (name, null)
        bad = o.copy()
        bad[0] = 1
        code, msg = call(L, name, len(o) - 1, bad, t, 1 << 40)
        assert code == -1 and "must start at 0" in msg, name
        bad = o.copy()
        bad[[2, 3]] = bad[[3, 2]]
        code, msg = call(L, name, len(o) - 1, bad, t, 1 << 40)
        assert code == -1 and "decrease" in msg, name


def test_sizes_then_the_long_document(built_lib):
    L = built_lib
    huge = U64(0, 1 << 32, (1 << 32) + 1)  # (checked from the offsets alone: no token is read)
    for name in INVERTERS + TRANSPOSERS:
        code, msg = call(L, name, 2, huge, U32(0), 1 << 32)
        assert code == -1 and "2^32" in msg and "or more" in msg and "holds" not in msg, (name, msg)
        code, msg = call(L, name, 2, huge, U32(0), 5)
        assert code == -1 and "row 0" in msg and "holds 2^32 entries or more" in msg, (name, msg)


def test_the_kind_comes_before_everything_and_no_token_before_the_device(built_lib):
    L = built_lib
    o, t = ic.small_edges()
    for kind in ("block_qmx", "block_mixed"):
        for null in (None, 0, 1):
            code, msg = call(L, "ds2i_hip_invert_documents", len(o) - 1, o, t, 12, kind=d.CODECS[kind], null=null)
            assert code == -1 and all(k in msg for k in cases.GPU_BUILT_KINDS), msg
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_invert_documents(kind, (o, t), 12, device=NO_DEVICE)
        assert e.value.code == -1 and all(k in str(e.value) for k in cases.GPU_BUILT_KINDS)
    assert call(L, "ds2i_hip_invert_documents", len(o) - 1, o, t, 12, kind=99)[0] == -1
    code, msg = call(L, "ds2i_hip_invert_documents", 3, U64(0, 0, 0, 0), U32(0), 12)
    assert code == -1 and "List must be nonempty" in msg
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_invert_documents("opt", [[], []], 12, device=NO_DEVICE)
    assert e.value.code == -1 and "List must be nonempty" in str(e.value)


def test_then_the_device(built_lib):
    L = built_lib
    o, t = ic.small_edges()
    bad = t.copy()
    bad[3] = 12  # a token outside the terms is the device's to find: without one, the missing device is what is reported
    for name in ("ds2i_hip_invert_postings", "ds2i_hip_invert_documents", "ds2i_hip_transpose_postings"):
        code, msg = call(L, name, len(o) - 1, o, bad, 12)
        assert code == -4 and "no such HIP device" in msg, name
    image = cases.image(rc.block_edge_collection(), "opt")
    for make in (lambda: d.gpu_invert_postings((o, t), 12, device=NO_DEVICE), lambda: d.gpu_invert_documents("opt", (o, t), 12, device=NO_DEVICE),
                 lambda: d.gpu_transpose_postings(len(o) - 1, 12, o, t, t, device=NO_DEVICE), lambda: d.gpu_forward_index("opt", image, device=NO_DEVICE)):
        with pytest.raises(d.Ds2iError) as e:
            make()
        assert e.value.code == -4


def test_forward_index_checks_without_a_device(built_lib):
    L = built_lib
    image = cases.image(rc.block_edge_collection(), "block_optpfor")

    def forward(kind, img, null=None):
        n, v, ms = C.c_uint64(77), C.c_uint64(77), C.c_double(-1.0)
        hs = [C.c_void_p() for _ in range(3)]
        args = [None if null == 0 else img, len(img), None if null == 1 else C.byref(n), None if null == 2 else C.byref(v)]
        args += [None if null == 3 + k else C.byref(h) for k, h in enumerate(hs)]
        code = L.ds2i_hip_forward_index(NO_DEVICE, kind, *args, C.byref(ms))
        assert code != 0 and not any(h.value for h in hs) and n.value == 77 and v.value == 77 and ms.value == -1.0
        return code, L.ds2i_hip_last_error().decode()

    for null in range(6):
        code, msg = forward(99, cases.GARBAGE, null)  # (before the kind and the image)
        assert code == -1 and "null argument" in msg
    for kind in (-1, 9, 99):
        code, msg = forward(kind, cases.GARBAGE)  # (before the image)
        assert code == -1 and "unknown index kind" in msg
    for kind in ("block_optpfor", "opt"):
        assert forward(d.CODECS[kind], cases.GARBAGE)[0] == -2
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_forward_index(kind, cases.GARBAGE, device=NO_DEVICE)
        assert e.value.code == -2
    code, msg = forward(0, image)
    assert code == -4 and "no such HIP device" in msg


def test_the_twins_name_the_first_offender(built_lib):
    L = built_lib
    o, t = ic.small_edges()
    bad = t.copy()
    bad[[6, 9]] = [12, 4000]  # documents 4 and 4: the first is named
    code, msg = call(L, "ds2i_invert_documents", len(o) - 1, o, bad, 12)
    assert code == -2 and "document 4 holds token 12 at position 1, outside the 12 terms" in msg
    with pytest.raises(d.Ds2iError) as e:
        d.invert_documents((o, bad), 12)
    assert e.value.code == -2
    offs, cols, vals = U64(0, 2, 2, 5), U32(1, 3, 0, 2, 2), U32(1, 1, 1, 1, 1)
    code, msg = call(L, "ds2i_transpose_postings", 3, offs, cols, 4, vals=vals)
    assert code == -2 and "the columns of row 2 do not strictly increase at position 2" in msg
    code, msg = call(L, "ds2i_transpose_postings", 3, offs, U32(1, 3, 0, 2, 4), 4, vals=vals)
    assert code == -2 and "row 2 holds column 4 at position 2, outside the 4 columns" in msg
    code, msg = call(L, "ds2i_transpose_postings", 3, offs, U32(1, 4, 0, 2, 4), 4, vals=vals)
    assert code == -2 and "row 0 holds column 4 at position 1" in msg
    d.transpose_postings(3, 4, offs, U32(1, 3, 0, 2, 3), vals)  # (3 after a row end is no decrease)
    for fn, args in ((d.invert_documents, ((U64(0, 5), U32(1, 2)), 12)), (d.transpose_postings, (1, 4, U64(0, 5), U32(1, 2), U32(1, 2)))):
        with pytest.raises(ValueError):  # offsets past the arrays never reach the library
            fn(*args)


# ---------------------------------------------------------------- the host side under the sanitizers, as a program of its own
def test_twin_check_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """host_invert.hpp and tests/invert_twin_check.cpp (its own main) compiled with -fsanitize=address,undefined and run: nothing that is
    loaded into this interpreter runs under a sanitizer"""
    exe = str(tmp_path / "invert_twin_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread",  # (the runtimes inside the program: it asks nothing of its loader)
                           os.path.join(ROOT, "tests", "invert_twin_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and p.stdout == "OK\n" and p.stderr == "", (p.stdout, p.stderr)


# ---------------------------------------------------------------- the tool
def test_tool_usage_errors_without_a_device(built_lib, tmp_path):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.dirname(TOOL), "-s"])

    def run(*args):
        p = subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return p.returncode, p.stdout, p.stderr

    o, t = ic.small_edges()
    fwd, out, short = str(tmp_path / "fwd"), str(tmp_path / "out"), str(tmp_path / "short")
    ic.write_forward(fwd, o, t)
    open(short, "wb").write(open(fwd, "rb").read()[:-8])
    base = ("opt", fwd, "12", out)
    for args in ((), base[:3], base + ("wand", "extra"), base + ("--check", "--gpu-only"), base + ("--frobnicate",), base + ("--device",),
                 base + ("--device", "-1"), ("opt", fwd, "twelve", out), ("opt", fwd, "-12", out), ("opt", fwd, "12x", out),
                 ("opt", fwd, str(1 << 32 | 1), out)):
        rcode, stdout, err = run(*args)
        assert rcode == 2 and stdout == "" and "usage" in err, (args, err)
    for bad in (str(tmp_path / "missing"), short):
        rcode, stdout, err = run("opt", bad, "12", out, "--device", str(NO_DEVICE))
        assert rcode == 2 and stdout == "" and "usage" in err and "no such HIP device" not in err, (bad, err)
    rcode, _, err = run("nonsense", fwd, "12", out)
    assert rcode == 2 and "Unknown type" in err
    rcode, stdout, err = run("block_qmx", fwd, "12", out, "--device", str(NO_DEVICE))
    assert rcode == 2 and stdout == "" and all(k in err for k in cases.GPU_BUILT_KINDS)
    rcode, stdout, err = run("--check", "opt", "--device", str(NO_DEVICE), fwd, "12", out, str(tmp_path / "out.wand"))  # (flags in any place)
    assert rcode == 2 and stdout == "" and "no such HIP device" in err
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("out")]
