"""Extraction and conversion on the GPU (-m gpu): ds2i_hip_extract_collection, ds2i_hip_index_extract, ds2i_hip_convert_index and
the convert_index tool. Everything is integers: extracted postings are compared with np.array_equal, images and files with == on
bytes, against the lists the images were built from and the HOST builder's images (verify_cases.image)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ds2i_amd as d
import oracle as o
from ds2i_amd.api import _csr
import verify_cases as cases
from helpers import queries_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "ds2i_amd", "tools")
CONVERT, CREATE = os.path.join(TOOLS, "convert_index"), os.path.join(TOOLS, "create_freq_index")


def check_equal(got, lists):
    """(offsets, docs, freqs) is the CSR form of `lists`"""
    offs, docs, freqs = got
    _, eo, ed, ef = _csr(lists)
    assert offs.dtype == np.uint64 and docs.dtype == np.uint32 and freqs.dtype == np.uint32
    assert np.array_equal(offs, eo)
    total = int(eo[-1])
    assert len(docs) == total and len(freqs) == total
    assert np.array_equal(docs, ed[:total]) and np.array_equal(freqs, ef[:total])


@pytest.mark.parametrize("kind", cases.KINDS)
def test_host_built_images_give_their_collection_back(built_lib, kind):
    for coll in cases.clean_collections(kind):
        num_docs, offs, docs, freqs, info = d.gpu_extract_collection(kind, cases.image(coll, kind))
        assert num_docs == coll.num_docs and info["device_ms"] > 0
        check_equal((offs, docs, freqs), coll.lists)


@pytest.mark.parametrize("kind", ["block_optpfor", "opt"])
def test_many_lists_more_blocks_than_the_grid(built_lib, kind):
    """every wave wraps, and most lists are one posting long: a store past a list's end lands in its neighbour and shows"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    coll = cases.many_lists_collection(cus)
    assert sum((len(dd) + 127) // 128 for dd, _ in coll.lists) > 16 * cus
    img = cases.image(coll, kind)
    num_docs, offs, docs, freqs, _ = d.gpu_extract_collection(kind, img)
    assert num_docs == coll.num_docs
    check_equal((offs, docs, freqs), coll.lists)
    if kind == "block_optpfor":  # ... and through the side slots and the tail table of an opened index
        idx = d.Index(kind, img)
        try:
            check_equal(idx.extract()[:3], coll.lists)
        finally:
            idx.close()


HANDLES = [("block_optpfor", None, dict(has_side_tables=1)),
           ("block_optpfor", "DS2I_DECODE_GENERAL", dict(has_side_tables=1)),
           ("opt", None, dict(transcoded_from=d.CODECS["opt"])),
           ("opt", "DS2I_PEF_NATIVE", dict(transcoded_from=-1)),
           ("block_mixed", "DS2I_MIXED_NATIVE", dict(transcoded_from=-1))]


def open_with(kind, option, image, wand=None, value=1):
    """the knobs are read once by the upload and kept in the handle: the option is reset as soon as the index is open"""
    try:
        if option:
            d.set_option(option, value)
        return d.Index(kind, image, wand)
    finally:
        if option:
            d.set_option(option, None)


@pytest.mark.parametrize("kind,option,info", HANDLES, ids=["%s-%s" % (k, o) for k, o, _ in HANDLES])
def test_an_opened_index_extracts_as_queries_read_it(built_lib, kind, option, info):
    coll = cases.small_collection()
    idx = open_with(kind, option, cases.image(coll, kind), coll.wand_image())
    try:
        got = idx.info()
        assert {k: got[k] for k in info} == info
        offs, docs, freqs, st = idx.extract()
        assert st["device_ms"] > 0
        check_equal((offs, docs, freqs), coll.lists)
    finally:
        idx.close()


@pytest.mark.parametrize("kind,option", [("block_optpfor", None), ("block_varint", None), ("opt", "DS2I_PEF_NATIVE")])
def test_a_middle_range_of_lists(built_lib, kind, option):
    coll, names = cases.block_edge_collection()
    a, b, c = names["len127"], names["len128"], names["len129"]
    assert (a + 1, b + 1) == (b, c)
    idx = open_with(kind, option, cases.image(coll, kind))
    try:
        V = len(coll.lists)
        for begin, end in ((a, c + 1), (b, b + 1), (b, c + 1), (a, b), (c, V), (1, V - 1), (0, c), (b, b), (V, V)):
            offs, docs, freqs, _ = idx.extract(begin, end)
            assert offs[0] == 0 and len(offs) == end - begin + 1
            check_equal((offs, docs, freqs), coll.lists[begin:end])
    finally:
        idx.close()


def test_size_query_short_capacity_and_bad_ranges(built_lib):
    L = built_lib
    coll, _ = cases.block_edge_collection()
    V = len(coll.lists)
    lens = [len(dd) for dd, _ in coll.lists]
    idx = d.Index("block_optpfor", cases.image(coll, "block_optpfor"))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        offs, n, ms = np.full(V + 1, 77, dtype=np.uint64), C.c_uint64(), C.c_double(-1.0)
        assert L.ds2i_hip_index_extract(idx._h, 0, V, p(offs), None, None, 0, C.byref(n), C.byref(ms)) == 0
        assert n.value == sum(lens) and ms.value == 0.0 and np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)]))
        begin, end = 2, 6
        total = sum(lens[begin:end])
        offs = np.zeros(end - begin + 1, dtype=np.uint64)
        assert L.ds2i_hip_index_extract(idx._h, begin, end, p(offs), None, None, 0, C.byref(n), None) == 0
        assert n.value == total and int(offs[-1]) == total
        # a short capacity: nothing is written, the needed count is reported
        docs, freqs = np.full(total, 0xABCD, dtype=np.uint32), np.full(total, 0xABCD, dtype=np.uint32)
        n.value = 0
        assert L.ds2i_hip_index_extract(idx._h, begin, end, p(offs), p(docs), p(freqs), total - 1, C.byref(n), None) == -1
        assert n.value == total and b"capacity" in L.ds2i_hip_last_error()
        assert np.all(docs == 0xABCD) and np.all(freqs == 0xABCD)
        assert L.ds2i_hip_index_extract(idx._h, begin, end, p(offs), p(docs), p(freqs), total, C.byref(n), None) == 0
        check_equal((offs, docs, freqs), coll.lists[begin:end])
        # ranges outside the index, null arguments
        assert L.ds2i_hip_index_extract(idx._h, 3, 2, p(offs), None, None, 0, C.byref(n), None) == -1
        assert L.ds2i_hip_index_extract(idx._h, 0, V + 1, p(offs), None, None, 0, C.byref(n), None) == -1
        assert L.ds2i_hip_index_extract(idx._h, begin, end, None, p(docs), p(freqs), total, C.byref(n), None) == -1
        assert L.ds2i_hip_index_extract(idx._h, begin, end, p(offs), p(docs), p(freqs), total, None, None) == -1
        assert L.ds2i_hip_index_extract(idx._h, begin, end, p(offs), None, p(freqs), total, C.byref(n), None) == -1
        assert L.ds2i_hip_index_extract(idx._h, begin, end, p(offs), p(docs), None, total, C.byref(n), None) == -1
        with pytest.raises(d.Ds2iError) as e:
            idx.extract(3, 2)
        assert e.value.code == -1
    finally:
        idx.close()


# ---------------------------------------------------------------- conversions: == the host builder's image, on bytes
def block_collections():
    return [cases.small_collection(), cases.block_edge_collection()[0]]


def check_conversion(coll, from_kind, to_kind):
    img, info = d.gpu_convert_index(from_kind, cases.image(coll, from_kind), to_kind)
    assert info["device_ms"] > 0
    want = cases.image(coll, to_kind)
    if img != want:
        m = min(len(img), len(want))
        bad = np.flatnonzero(np.frombuffer(img[:m], dtype=np.uint8) != np.frombuffer(want[:m], dtype=np.uint8))
        print("lengths, first differing byte, differing bytes:", len(img), len(want), int(bad[0]) if len(bad) else None, len(bad))
    assert img == want


@pytest.mark.parametrize("from_kind", cases.KINDS)
def test_every_kind_converts_to_block_optpfor(built_lib, from_kind):
    for coll in block_collections():
        check_conversion(coll, from_kind, "block_optpfor")


@pytest.mark.parametrize("from_kind", cases.KINDS)
def test_every_kind_converts_to_opt(built_lib, from_kind):
    for coll in block_collections():
        check_conversion(coll, from_kind, "opt")


@pytest.mark.parametrize("to_kind", cases.GPU_BUILT_KINDS)
def test_block_optpfor_converts_to_every_gpu_built_kind(built_lib, to_kind):
    for coll in block_collections():
        check_conversion(coll, "block_optpfor", to_kind)


@pytest.mark.parametrize("from_kind", cases.FREQ_KINDS)
def test_freq_kinds_convert_among_themselves(built_lib, from_kind):
    """the freq edge and dense collections: prefix sums of the freqs pass 2^32, which the block codecs are not built for"""
    for coll in (cases.freq_edge_collection(), cases.freq_dense_collection()):
        for to_kind in cases.FREQ_KINDS:
            check_conversion(coll, from_kind, to_kind)


def test_conversion_errors(built_lib):
    coll, _ = cases.block_edge_collection()
    img = cases.image(coll, "opt")
    for to_kind in ("block_qmx", "block_mixed"):
        with pytest.raises(d.Ds2iError) as e:
            d.gpu_convert_index("opt", img, to_kind)
        assert e.value.code == -1 and all(name in str(e.value) for name in cases.GPU_BUILT_KINDS)
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_convert_index("opt", cases.GARBAGE, "block_optpfor")
    assert e.value.code == -2
    with pytest.raises(d.Ds2iError) as e:
        d.gpu_extract_collection("block_optpfor", cases.GARBAGE)
    assert e.value.code == -2


def test_a_converted_image_answers_queries(built_lib):
    coll = cases.small_collection()
    wand = coll.wand_image()
    img, _ = d.gpu_convert_index("opt", cases.image(coll, "opt"), "block_optpfor")
    queries = queries_for(coll, nq=48)
    converted, built = d.Index("block_optpfor", img, wand), d.Index("block_optpfor", cases.image(coll, "block_optpfor"), wand)
    try:
        count, topk, tlen, _ = converted.query_batch("ranked_and", queries, k=10)
        rcount, rtopk, rtlen, _ = built.query_batch("ranked_and", queries, k=10)
        assert np.array_equal(count, rcount) and np.array_equal(tlen, rtlen) and int(tlen.sum()) > 0
        assert topk.tobytes() == rtopk.tobytes()
    finally:
        converted.close()
        built.close()


# ---------------------------------------------------------------- the transcoding upload is the conversion
TRANSCODED_KINDS = ("opt", "ef", "single", "uniform", "block_mixed")


@pytest.mark.parametrize("kind", TRANSCODED_KINDS)
def test_transcoding_upload_is_the_conversion(built_lib, kind):
    """the default upload of an image that is transcoded, and a plain block_optpfor upload of the image gpu_convert_index makes of
    it, are the same index: the same info() but for transcoded_from, and both give the collection back"""
    coll = cases.small_collection()
    image, wand = cases.image(coll, kind), coll.wand_image()
    converted, _ = d.gpu_convert_index(kind, image, "block_optpfor")
    default, direct = d.Index(kind, image, wand), d.Index("block_optpfor", converted, wand)
    try:
        a, b = default.info(), direct.info()
        assert a.pop("transcoded_from") == d.CODECS[kind] and b.pop("transcoded_from") == -1
        assert a == b and a["has_side_tables"] and a["has_range_tables"]
        for idx in (default, direct):
            check_equal(idx.extract()[:3], coll.lists)
    finally:
        default.close()
        direct.close()


@pytest.mark.parametrize("kind", ["opt", "block_mixed"])
def test_budget_below_a_transcoded_index_keeps_the_image(built_lib, kind):
    """DS2I_TABLE_BUDGET = one byte per posting: a transcoded index needs more than two (its block_optpfor image alone), so the
    upload keeps the image as it is -- decided from the image on the host, before anything is uploaded -- and the native kernels
    answer: every list decodes to the raw list, ranked_and and `and` equal the oracle (counts exactly, scores within 1e-5
    relative: float32 sums in the same order)"""
    coll = cases.small_collection()
    image, wand = cases.image(coll, kind), coll.wand_image()
    queries = queries_for(coll, nq=48)
    idx = open_with(kind, "DS2I_TABLE_BUDGET", image, wand, value=cases.postings(coll))
    try:
        info = idx.info()
        assert info["transcoded_from"] == -1 and info["table_budget_bytes"] == cases.postings(coll)
        for t, (docs, freqs) in enumerate(coll.lists):
            dd, ff = idx[t]
            assert np.array_equal(dd, docs) and np.array_equal(ff, freqs), t
        oidx = o.Index(kind, image, wand)
        count, topk, tlen, _ = idx.query_batch("ranked_and", queries, k=10)
        ocount, otopk, otlen, _, _ = oidx.query_batch("ranked_and", queries, k=10)
        assert np.array_equal(count, ocount) and np.array_equal(tlen, otlen) and int(tlen.sum()) > 0
        for i in range(len(queries)):
            np.testing.assert_allclose(topk[i, :tlen[i]], otopk[i, :otlen[i]], rtol=1e-5, err_msg=str(queries[i]))
            assert np.all(np.isneginf(topk[i, tlen[i]:]))
        acount = idx.query_batch("and", queries)[0]
        assert np.array_equal(acount, oidx.query_batch("and", queries)[0]) and int(acount.sum()) > 0
    finally:
        idx.close()


# ---------------------------------------------------------------- the tool
@pytest.fixture(scope="module")
def files(built_lib, tmp_path_factory):
    if not (os.path.exists(CONVERT) and os.path.exists(CREATE)):
        subprocess.check_call(["make", "-C", TOOLS, "-s"])
    coll, _ = cases.block_edge_collection()
    base = str(tmp_path_factory.mktemp("extract_gpu") / "edge")
    cases.write_collection(base, coll.num_docs, coll.lists, coll.sizes)
    for kind in ("opt", "block_optpfor"):
        subprocess.check_call([CREATE, kind, base, base + "." + kind], stderr=subprocess.DEVNULL)
    return coll, base


def run(tool, *args):
    p = subprocess.run([tool] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_tool_converts_checks_and_writes_the_builders_file(files):
    coll, base = files
    out = base + ".converted"
    rc, stdout, err = run(CONVERT, "opt", base + ".opt", "block_optpfor", out, "--check")
    assert rc == 0, err
    assert stdout == "OK lists=%d postings=%d\n" % (len(coll.lists), cases.postings(coll))
    assert open(out, "rb").read() == open(base + ".block_optpfor", "rb").read()
    rc, stdout, err = run(CONVERT, "block_optpfor", "--device", "0", out, "opt", out + ".opt")  # flags in any place; no --check: no line
    assert rc == 0 and stdout == "", err
    assert open(out + ".opt", "rb").read() == open(base + ".opt", "rb").read()


def test_tool_dumps_the_collection(files):
    coll, base = files
    rc, stdout, err = run(CONVERT, "opt", base + ".opt", "--dump", base + ".dumped")
    assert rc == 0 and stdout == "", err
    for ext in (".docs", ".freqs"):
        assert open(base + ".dumped" + ext, "rb").read() == open(base + ext, "rb").read()
    assert not os.path.exists(base + ".dumped.sizes")


def test_tool_errors(files, tmp_path):
    _, base = files
    out = str(tmp_path / "x")
    assert run(CONVERT, "no_such_type", base + ".opt", "block_optpfor", out)[0] == 2
    assert run(CONVERT, "opt", base + ".opt", "no_such_type", out)[0] == 2
    rc, _, err = run(CONVERT, "opt", base + ".opt", "block_mixed", out)
    assert rc == 2 and "block_interpolative" in err
    assert run(CONVERT, "opt", str(tmp_path / "missing"), "block_optpfor", out)[0] == 2
    assert not os.path.exists(out)
