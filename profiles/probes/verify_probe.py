"""Verifying an index against its collection: ds2i_hip_verify_collection (one call, one launch over every block of every list)
against what a caller could do before it existed -- open the index, loop index[term] over all lists and compare with numpy on the
host -- per kind, on the configs[1] collection (1 M docs, 65 536 terms, 52 M postings, seed 0xD5210002).
    python profiles/probes/verify_probe.py [terms] [reps] [kinds, comma separated]
Best of `reps` alternating runs in one process. The one call's wall time is split into the host parse of the image + structure
comparison, the bare upload, the staging of the postings (ds2i_hip_verify_host_seconds) and the kernel (hipEvent); the rest is
the report and the close. Every GPU step runs under a time limit of its own: a step that passes it ends the process (exit 124)."""
import ctypes as C
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import ds2i_amd as d

terms = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
kinds = sys.argv[3].split(",") if len(sys.argv) > 3 else ["block_optpfor", "opt"]
p = d.SynthParams(seed=0xD5210002, num_docs=1000000, num_terms=terms, zipf_exp=0.75, top_df_frac=0.5, min_len=128, clustered_every=4)
L = d.lib()
ptr = lambda a: C.c_void_p(a.ctypes.data)


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
with ThreadPoolExecutor(16) as pool:
    lists = list(pool.map(lambda t: d.synth_list(p, t), range(terms)))
offs = np.zeros(terms + 1, dtype=np.uint64)
offs[1:] = np.cumsum([len(dd) for dd, _ in lists])
docs = np.concatenate([dd for dd, _ in lists])
freqs = np.concatenate([ff for _, ff in lists])
del lists
print("%d lists, %d postings (generated in %.1f s)" % (terms, len(docs), time.perf_counter() - t0), flush=True)


def one_call(kind, img):
    r, ms, host = d.api.VerifyReport(), C.c_double(), (C.c_double * 3)()
    t0 = time.perf_counter()
    rc = L.ds2i_hip_verify_collection(0, d.CODECS[kind], img, len(img), int(p.num_docs), terms, ptr(offs), ptr(docs), ptr(freqs),
                                      C.byref(r), C.byref(ms))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(L.ds2i_hip_last_error().decode())
    L.ds2i_hip_verify_host_seconds(host)
    return dt, ms.value, host[0], host[1], host[2], r.what == 0 and r.postings_checked == len(docs)


def the_loop(kind, img):
    t0 = time.perf_counter()
    idx = d.Index(kind, img)
    t_open = time.perf_counter() - t0
    o, ok = offs.tolist(), True
    for t in range(terms):
        dd, ff = idx[t]
        ok = ok and np.array_equal(dd, docs[o[t]:o[t + 1]]) and np.array_equal(ff, freqs[o[t]:o[t + 1]])
    dt = time.perf_counter() - t0
    idx.close()
    return dt, t_open, ok


for kind in kinds:
    img = d.synth_build(p, kind, 16)[0]
    with limit(120, "warm-up call"):
        one_call(kind, img)  # code objects, allocator
    calls, loops = [], []
    for rep in range(reps):
        with limit(400, "index[term] loop over %d lists" % terms):
            loops.append(the_loop(kind, img))
        print("  %s rep %d: loop %.3f s" % (kind, rep, loops[-1][0]), flush=True)
        with limit(120, "ds2i_hip_verify_collection"):
            calls.append(one_call(kind, img))
        print("  %s rep %d: one call %.3f s" % (kind, rep, calls[-1][0]), flush=True)
    c, lp = min(calls, key=lambda r: r[0]), min(loops, key=lambda r: r[0])
    print("%-14s image %d bytes | open + index[term] loop + numpy compare %.3f s (open %.3f s) | one call %.3f s = host parse %.3f s + bare "
          "upload %.3f s + staging %.3f s + kernel %.1f ms + report, close %.3f s | all clean: %s" %
          (kind, len(img), lp[0], lp[1], c[0], c[2], c[3], c[4], c[1], c[0] - c[2] - c[3] - c[4] - 1e-3 * c[1],
           all(r[5] for r in calls) and all(r[2] for r in loops)), flush=True)
