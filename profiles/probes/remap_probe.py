"""Renumbering the documents of an index: the one device call against what a caller could do before it existed, on the configs[1]
collection (1 M docs, 65 536 terms, 52 M postings, seed 0xD5210002) with a seeded random doc-id map.
    python profiles/probes/remap_probe.py [terms] [runs]
  * gpu_remap_index(opt -> block_optpfor): one call, the postings never leave the device;
  * by hand: ds2i_hip_extract_collection to the host, ds2i_remap_postings (the host twin) on 16 threads, ds2i_hip_encode_index of
    the result -- the C ABI directly, on CSR arrays, so that no Python list handling is timed.
Alternating runs in one process after a warm-up of each; median and range of `runs` (default 5). The device call's kernel time is
split into extraction, map kernel, the three sort classes and the encoder (ds2i_hip_remap_ms). Both images are compared.
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
from ds2i_amd.api import _check, _ptr, _take_blob

terms = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
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


t0 = time.perf_counter()
img = d.synth_build(p, "opt", 16)[0]
doc_map = np.random.default_rng(0x52E3A9).permutation(p.num_docs).astype(np.uint32)
print("%d lists, opt image of %d bytes (built in %.1f s); classes W, L, T = %s" % (terms, len(img), time.perf_counter() - t0, d.remap_class_bounds()),
      flush=True)


def one_call():
    t0 = time.perf_counter()
    out, info = d.gpu_remap_index("opt", img, doc_map, "block_optpfor")
    return time.perf_counter() - t0, info, out


def by_hand():
    t0 = time.perf_counter()
    n, v, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    ho, hd, hf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(L.ds2i_hip_extract_collection(0, FROM, img, len(img), C.byref(n), C.byref(v), C.byref(ho), C.byref(hd), C.byref(hf), C.byref(ms)))
    t1 = time.perf_counter()
    data = [L.ds2i_blob_data(h) for h in (ho, hd, hf)]  # sorted where the extraction left them: no copy
    _check(L.ds2i_remap_postings(n.value, v.value, data[0], data[1], data[2], _ptr(doc_map), 16))
    t2 = time.perf_counter()
    h = C.c_void_p()
    _check(L.ds2i_hip_encode_index(0, TO, n.value, v.value, data[0], data[1], data[2], C.byref(h), C.byref(ms)))
    out = _take_blob(h)
    dt = time.perf_counter() - t0
    for b in (ho, hd, hf):
        L.ds2i_blob_free(b)
    return dt, (t1 - t0, t2 - t1, dt - (t2 - t0)), out


def spread(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


with limit(300, "warm-up of the device call"):
    want = one_call()[2]
with limit(400, "warm-up of the path by hand"):
    same = by_hand()[2] == want
calls, hands = [], []
for run in range(runs):
    with limit(400, "extract + host twin + encode"):
        hands.append(by_hand())
    with limit(300, "ds2i_hip_remap_index"):
        calls.append(one_call())
    print("  run %d: by hand %.3f s, one call %.3f s" % (run, hands[-1][0], calls[-1][0]), flush=True)
same = same and all(r[2] == want for r in calls + hands)
print("opt -> block_optpfor through a random map, %d -> %d bytes, median (min .. max) of %d runs" % (len(img), len(want), runs))
print("  by hand  %s s = extract to the host %s + host twin on 16 threads %s + stage and encode %s" %
      (spread([h[0] for h in hands]), spread([h[1][0] for h in hands]), spread([h[1][1] for h in hands]), spread([h[1][2] for h in hands])))
print("  one call %s s; kernels %s ms = extraction %s + map %s + class 1 %s + class 2 %s + class 3 %s + encoder %s" %
      (spread([c[0] for c in calls]), spread([c[1]["device_ms"] for c in calls]), spread([c[1]["extract_ms"] for c in calls]),
       spread([c[1]["map_ms"] for c in calls]), spread([c[1]["sort_ms"][0] for c in calls]), spread([c[1]["sort_ms"][1] for c in calls]),
       spread([c[1]["sort_ms"][2] for c in calls]), spread([c[1]["encode_ms"] for c in calls])))
print("  same image every time: %s" % same, flush=True)
