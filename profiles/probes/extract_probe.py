"""Getting a collection back out of an index, and converting an index to another kind: the one-launch entry points against what a
caller could do before they existed, on the configs[1] collection (1 M docs, 65 536 terms, 52 M postings, seed 0xD5210002).
    python profiles/probes/extract_probe.py [terms] [reps] [kinds, comma separated]
  * gpu_extract_collection(kind, image) against: open the index, loop index[term] over all lists, concatenate -- per kind;
  * gpu_convert_index(opt -> block_optpfor) against: gpu_extract_collection to the host, then gpu_encode_index of the lists.
Best of `reps` alternating runs in one process. The extraction's wall time is split into the host parse of the image, the bare
upload, the kernel (hipEvent) and the copy of the postings to the host (ds2i_hip_extract_host_seconds); the rest is allocation and
the close. Every GPU step runs under a time limit of its own: a step that passes it ends the process (exit 124)."""
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


def same(o, dd, ff):
    return bool(np.array_equal(o, offs) and np.array_equal(dd, docs) and np.array_equal(ff, freqs))


def one_call(kind, img):
    host = (C.c_double * 3)()
    t0 = time.perf_counter()
    _, o, dd, ff, info = d.gpu_extract_collection(kind, img)
    dt = time.perf_counter() - t0
    L.ds2i_hip_extract_host_seconds(host)
    return dt, info["device_ms"], host[0], host[1], host[2], same(o, dd, ff)


def the_loop(kind, img):
    t0 = time.perf_counter()
    idx = d.Index(kind, img)
    t_open = time.perf_counter() - t0
    got = [idx[t] for t in range(terms)]
    dd, ff = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    o = np.zeros(terms + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(g[0]) for g in got])
    dt = time.perf_counter() - t0
    idx.close()
    return dt, t_open, same(o, dd, ff)


def convert_call(img):
    t0 = time.perf_counter()
    out, info = d.gpu_convert_index("opt", img, "block_optpfor")
    return time.perf_counter() - t0, info["device_ms"], out


def convert_by_hand(img):
    t0 = time.perf_counter()
    n, o, dd, ff, _ = d.gpu_extract_collection("opt", img)
    t_extract = time.perf_counter() - t0
    ol = o.tolist()
    out, _ = d.gpu_encode_index(n, [(dd[ol[t]:ol[t + 1]], ff[ol[t]:ol[t + 1]]) for t in range(terms)], codec="block_optpfor")
    return time.perf_counter() - t0, t_extract, out


images = {}
for kind in kinds:
    img = images[kind] = d.synth_build(p, kind, 16)[0]
    with limit(120, "warm-up call"):
        one_call(kind, img)  # code objects, allocator
    calls, loops = [], []
    for rep in range(reps):
        with limit(400, "index[term] loop over %d lists" % terms):
            loops.append(the_loop(kind, img))
        print("  %s rep %d: loop %.3f s" % (kind, rep, loops[-1][0]), flush=True)
        with limit(120, "ds2i_hip_extract_collection"):
            calls.append(one_call(kind, img))
        print("  %s rep %d: one call %.3f s" % (kind, rep, calls[-1][0]), flush=True)
    c, lp = min(calls, key=lambda r: r[0]), min(loops, key=lambda r: r[0])
    print("%-14s image %d bytes | open + index[term] loop + concatenate %.3f s (open %.3f s) | one call %.3f s = host parse %.3f s + bare "
          "upload %.3f s + kernel %.1f ms + download %.3f s + allocation, close %.3f s | all equal: %s" %
          (kind, len(img), lp[0], lp[1], c[0], c[2], c[3], c[1], c[4], c[0] - c[2] - c[3] - c[4] - 1e-3 * c[1],
           all(r[5] for r in calls) and all(r[2] for r in loops)), flush=True)

if "opt" in images:
    img = images["opt"]
    with limit(300, "warm-up conversion"):
        want = convert_call(img)[2]
    calls, hands = [], []
    for rep in range(reps):
        with limit(400, "extract to the host + gpu_encode_index"):
            hands.append(convert_by_hand(img))
        print("  convert rep %d: by hand %.3f s" % (rep, hands[-1][0]), flush=True)
        with limit(300, "ds2i_hip_convert_index"):
            calls.append(convert_call(img))
        print("  convert rep %d: one call %.3f s" % (rep, calls[-1][0]), flush=True)
    c, h = min(calls, key=lambda r: r[0]), min(hands, key=lambda r: r[0])
    print("opt -> block_optpfor: %d -> %d bytes | extract to the host + gpu_encode_index %.3f s (extract %.3f s) | one call %.3f s, "
          "kernels %.1f ms | same image: %s" % (len(img), len(want), h[0], h[1], c[0], c[1], all(r[2] == want for r in calls + hands)), flush=True)
