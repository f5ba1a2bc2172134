"""wand_data build: host threads vs ds2i_hip_build_wand, and the one staging of ds2i_hip_build_collection against
ds2i_hip_encode_index + ds2i_hip_build_wand called one after the other, on the configs[1] collection (1 M docs, 65 536 terms,
52 M postings, seed 0xD5210002). All entry points are called on the same CSR arrays through ctypes, so the wall times hold what
the C ABI costs: checks, staging, upload, kernels, download, freeze.
    python profiles/probes/wand_gpu_probe.py [threads] [terms]
The host side has no threaded entry point for a caller's own lists: `threads` builders (ds2i_wand_*) take a contiguous run of
lists each, balanced by postings, and their max_term_weight arrays are concatenated -- the image is checked against the GPU's.
The host figure therefore includes one ctypes call per list (the threads share the interpreter lock between calls)."""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import ds2i_amd as d

threads = int(sys.argv[1]) if len(sys.argv) > 1 else 16
terms = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
p = d.SynthParams(seed=0xD5210002, num_docs=1000000, num_terms=terms, zipf_exp=0.75, top_df_frac=0.5, min_len=128, clustered_every=4)
L = d.lib()
ptr = lambda a, off=0: C.c_void_p(a.ctypes.data + off)

t0 = time.perf_counter()
with ThreadPoolExecutor(threads) as pool:
    lists = list(pool.map(lambda t: d.synth_list(p, t), range(terms)))
sizes = d.synth_doc_sizes(p)
offs = np.zeros(terms + 1, dtype=np.uint64)
offs[1:] = np.cumsum([len(dd) for dd, _ in lists])
docs = np.concatenate([dd for dd, _ in lists])
freqs = np.concatenate([ff for _, ff in lists])
del lists
print("%d lists, %d postings, %d blocks (generated in %.1f s)" % (terms, len(docs), int(((offs[1:] - offs[:-1] + 127) // 128).sum()), time.perf_counter() - t0), flush=True)


def check(rc):
    if rc:
        raise RuntimeError(L.ds2i_hip_last_error().decode())


def take(h):
    n = L.ds2i_blob_size(h)
    out = (C.c_char * n).from_address(L.ds2i_blob_data(h)).raw
    L.ds2i_blob_free(h)
    return out


def host_wand():
    cuts = np.searchsorted(offs, np.linspace(0, int(offs[-1]), threads + 1)[1:-1]).tolist()
    bounds = [0] + cuts + [terms]
    o, da, fa = offs.tolist(), docs.ctypes.data, freqs.ctypes.data  # plain integers: the loop below is 65 536 ctypes calls

    def part(i):
        w = C.c_void_p()
        check(L.ds2i_wand_create(ptr(sizes), len(sizes), C.byref(w)))
        add = L.ds2i_wand_add_list
        for t in range(bounds[i], bounds[i + 1]):
            if add(w, o[t + 1] - o[t], da + 4 * o[t], fa + 4 * o[t]):
                check(-1)
        h = C.c_void_p()
        check(L.ds2i_wand_freeze(w, C.byref(h)))
        L.ds2i_wand_free(w)
        return take(h)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        imgs = list(pool.map(part, range(threads)))
    dt = time.perf_counter() - t0
    head = 8 + 4 * len(sizes)
    image = imgs[0][:head] + np.uint64(terms).tobytes() + b"".join(im[head + 8:] for im in imgs)
    return image, dt


def gpu_wand():
    h, ms = C.c_void_p(), C.c_double()
    t0 = time.perf_counter()
    check(L.ds2i_hip_build_wand(0, ptr(sizes), len(sizes), terms, ptr(offs), ptr(docs), ptr(freqs), C.byref(h), C.byref(ms)))
    return take(h), time.perf_counter() - t0, ms.value


def gpu_index():
    h, ms = C.c_void_p(), C.c_double()
    t0 = time.perf_counter()
    check(L.ds2i_hip_encode_index(0, 0, len(sizes), terms, ptr(offs), ptr(docs), ptr(freqs), C.byref(h), C.byref(ms)))
    return take(h), time.perf_counter() - t0, ms.value


def gpu_collection():
    hi, hw, ms = C.c_void_p(), C.c_void_p(), C.c_double()
    t0 = time.perf_counter()
    check(L.ds2i_hip_build_collection(0, 0, ptr(sizes), len(sizes), terms, ptr(offs), ptr(docs), ptr(freqs), C.byref(hi), C.byref(hw), C.byref(ms)))
    dt = time.perf_counter() - t0
    return take(hi), take(hw), dt, ms.value


gpu_wand()  # warm-up: code objects, allocator
rows = []
for rep in range(3):  # alternating, same process
    himg, hs = host_wand()
    gimg, gs, gms = gpu_wand()
    iimg, is_, ims = gpu_index()
    ci, cw, cs, cms = gpu_collection()
    same = gimg == himg and cw == gimg and ci == iimg
    rows.append((hs, gs, gms, is_, cs, cms, same))
    print("rep %d: host wand (%d threads) %.3f s | gpu wand %.3f s (kernel %.2f ms) | encode_index %.3f s (kernels %.1f ms) | "
          "build_collection %.3f s (kernels %.1f ms) vs separately %.3f s | identical: %s" % (rep, threads, hs, gs, gms, is_, ims, cs, cms, is_ + gs, same), flush=True)
med = lambda i: sorted(r[i] for r in rows)[1]
print("median: host wand %.3f s | gpu wand %.3f s end to end, kernel %.2f ms | build_collection %.3f s vs encode_index + build_wand %.3f s (saves %.3f s)"
      % (med(0), med(1), med(2), med(4), med(3) + med(1), med(3) + med(1) - med(4)))
