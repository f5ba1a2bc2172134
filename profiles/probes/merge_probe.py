"""Merging the shards of a collection into one index: the one device call against what a caller could do before it existed, on the
configs[1] collection (1 M docs, 65 536 terms, 52 M postings, seed 0xD5210002) cut into 4 contiguous doc ranges, each an opt image of its
own (documents renumbered from 0, terms without a posting in the range dropped and named by a term map).
    python profiles/probes/merge_probe.py [terms] [runs]
  * gpu_merge_indexes(4 x opt -> block_optpfor): one call, the postings never leave the device; default doc maps, so nothing is sorted;
  * by hand: ds2i_hip_extract_collection of every shard to the host, ds2i_merge_postings (the host twin) on 16 threads,
    ds2i_hip_encode_index of the result -- the C ABI directly, on CSR arrays, so that no Python list handling is timed.
Alternating runs in one process after a warm-up of each; median and range of `runs` (default 5). The device call's kernel time is
split into extraction, placement, sort and encoder (ds2i_hip_merge_ms). Both images are compared with the image of the whole collection.
Every GPU step runs under a time limit of its own: a step that passes it ends the process (exit 124)."""
import ctypes as C
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import ds2i_amd as d
from ds2i_amd.api import MergePostingsSource, _check, _ptr, _take_blob

terms = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SHARDS = 4
p = d.SynthParams(seed=0xD5210002, num_docs=1000000, num_terms=terms, zipf_exp=0.75, top_df_frac=0.5, min_len=128, clustered_every=4)
L = d.lib()
FROM, TO = d.CODECS["opt"], d.CODECS["block_optpfor"]


class limit:
    """ends the process when the step inside takes longer than `seconds` (a hung GPU call never returns to Python)"""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self.expired, (seconds, what))
        self.t.daemon = True

    @staticmethod
    def expired(seconds, what):
        print("TIME LIMIT: %s took more than %d s" % (what, seconds), flush=True)
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()


def encode(kind, num_docs, offs, docs, freqs):
    h, ms = C.c_void_p(), C.c_double()
    _check(L.ds2i_hip_encode_index(0, kind, num_docs, len(offs) - 1, _ptr(offs), _ptr(docs), _ptr(freqs), C.byref(h), C.byref(ms)))
    return _take_blob(h)


t0 = time.perf_counter()
whole = d.synth_build(p, "opt", 16)[0]
with limit(300, "extraction of the whole collection"):
    num_docs, offs, docs, freqs, _ = d.gpu_extract_collection("opt", whole)
with limit(300, "the image the merge must give"):
    want = encode(TO, num_docs, offs, docs, freqs)
sources = []
list_of = np.repeat(np.arange(terms), np.diff(offs).astype(np.int64))
for s in range(SHARDS):
    lo, hi = num_docs * s // SHARDS, num_docs * (s + 1) // SHARDS
    keep = (docs >= lo) & (docs < hi)
    counts = np.bincount(list_of[keep], minlength=terms)
    term_map = np.flatnonzero(counts).astype(np.uint32)
    soffs = np.concatenate([[0], np.cumsum(counts[term_map])]).astype(np.uint64)
    with limit(300, "encoding of shard %d" % s):
        sources.append(("opt", encode(FROM, hi - lo, soffs, (docs[keep] - np.uint32(lo)).astype(np.uint32), freqs[keep].copy()), None, term_map))
del docs, freqs, list_of, keep
print("%d lists, %d postings, %d opt shards of %s bytes (built in %.1f s)" %
      (terms, int(offs[-1]), SHARDS, [len(img) for _, img, _, _ in sources], time.perf_counter() - t0), flush=True)


def one_call():
    t0 = time.perf_counter()
    out, info = d.gpu_merge_indexes(sources, "block_optpfor", num_terms=terms)
    return time.perf_counter() - t0, info, out


def by_hand():
    t0 = time.perf_counter()
    arr, blobs = (MergePostingsSource * SHARDS)(), []
    for src, (_, img, _, term_map) in zip(arr, sources):
        n, v, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        ho, hd, hf = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(L.ds2i_hip_extract_collection(0, FROM, img, len(img), C.byref(n), C.byref(v), C.byref(ho), C.byref(hd), C.byref(hf), C.byref(ms)))
        blobs += [ho, hd, hf]
        src.num_docs, src.nlists = n.value, v.value
        src.list_offsets, src.docs, src.freqs = (L.ds2i_blob_data(h) for h in (ho, hd, hf))  # where the extraction left them: no copy
        src.term_map, src.terms_len = term_map.ctypes.data, len(term_map)
    t1 = time.perf_counter()
    n, v = C.c_uint64(), C.c_uint64()
    mo, md, mf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(L.ds2i_merge_postings(arr, SHARDS, terms, 16, C.byref(n), C.byref(v), C.byref(mo), C.byref(md), C.byref(mf)))
    t2 = time.perf_counter()
    h, ms = C.c_void_p(), C.c_double()
    _check(L.ds2i_hip_encode_index(0, TO, n.value, v.value, L.ds2i_blob_data(mo), L.ds2i_blob_data(md), L.ds2i_blob_data(mf), C.byref(h), C.byref(ms)))
    out = _take_blob(h)
    dt = time.perf_counter() - t0
    for b in blobs + [mo, md, mf]:
        L.ds2i_blob_free(b)
    return dt, (t1 - t0, t2 - t1, dt - (t2 - t0)), out


def spread(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


with limit(300, "warm-up of the device call"):
    same = one_call()[2] == want
with limit(400, "warm-up of the path by hand"):
    same = by_hand()[2] == want and same
calls, hands = [], []
for run in range(runs):
    with limit(400, "extract + host twin + encode"):
        hands.append(by_hand())
    with limit(300, "ds2i_hip_merge_indexes"):
        calls.append(one_call())
    print("  run %d: by hand %.3f s, one call %.3f s" % (run, hands[-1][0], calls[-1][0]), flush=True)
same = same and all(r[2] == want for r in calls + hands)
print("%d x opt -> block_optpfor, %d -> %d bytes, median (min .. max) of %d runs" % (SHARDS, sum(len(s[1]) for s in sources), len(want), runs))
print("  by hand  %s s = extract every shard to the host %s + host twin on 16 threads %s + stage and encode %s" %
      (spread([h[0] for h in hands]), spread([h[1][0] for h in hands]), spread([h[1][1] for h in hands]), spread([h[1][2] for h in hands])))
print("  one call %s s; kernels %s ms = extraction %s + placement %s + sort %s + encoder %s" %
      (spread([c[0] for c in calls]), spread([c[1]["device_ms"] for c in calls]), spread([c[1]["extract_ms"] for c in calls]),
       spread([c[1]["place_ms"] for c in calls]), spread([c[1]["sort_ms"] for c in calls]), spread([c[1]["encode_ms"] for c in calls])))
print("  the image of the whole collection every time: %s" % same, flush=True)
