"""Elias-Fano layouts (opt, ef, single, uniform): the host builder on `threads` threads against ds2i_hip_encode_index, per kind, on
the configs[1] collection (1 M docs, 65 536 terms, 52 M postings, seed 0xD5210002). Both sides are called on the same CSR arrays
through ctypes, so the wall times hold what the C ABI costs: checks, planning, staging, kernels, download, freeze.
    python profiles/probes/freq_encode_probe.py [threads] [terms] [reps]
The host side has no threaded entry point for a caller's own lists: `threads` builders (ds2i_builder_*) take a contiguous run of
lists each, balanced by postings, one ctypes call per list, and freeze their part -- that is the host's time for the same work.
The GPU image is compared with ds2i_synth_build's (the same lists, encoded list-parallel on the host) under ==.
For the GPU call the split is: planning on the host (headers and jobs; the partition DP of opt when the host plans it), kernels
(hipEvent; the partition kernels of opt among them when the device plans, which is the default), download +
headers + freeze (ds2i_hip_encode_host_seconds); the rest of the wall time is the input check, the staging and the upload.
Last, the two planners of opt (ds2i_hip_encode_index_with: the partition DP on the host threads against partition_kernels.hip),
alternating in this process, `plan_reps` (argv[4], default 5) calls each: whole call, the host's planning seconds, the partition
kernels (ds2i_hip_encode_plan_ms), all kernels, and what remains of the planning phase -- medians with min / max. With
DS2I_PROBE_BASELINE_LIB=<another build of the library, e.g. the parent commit's> that library's ds2i_hip_encode_index(opt) is
timed in the same loop, from a child process of its own (two builds of the library do not share a process)."""
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
plan_reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
p = d.SynthParams(seed=0xD5210002, num_docs=1000000, num_terms=terms, zipf_exp=0.75, top_df_frac=0.5, min_len=128, clustered_every=4)
L = d.lib()
ptr = lambda a, off=0: C.c_void_p(a.ctypes.data + off)

t0 = time.perf_counter()
with ThreadPoolExecutor(threads) as pool:
    lists = list(pool.map(lambda t: d.synth_list(p, t), range(terms)))
offs = np.zeros(terms + 1, dtype=np.uint64)
offs[1:] = np.cumsum([len(dd) for dd, _ in lists])
docs = np.concatenate([dd for dd, _ in lists])
freqs = np.concatenate([ff for _, ff in lists])
del lists
print("%d lists, %d postings (generated in %.1f s)" % (terms, len(docs), time.perf_counter() - t0), flush=True)


def check(rc):
    if rc:
        raise RuntimeError(L.ds2i_hip_last_error().decode())


def take(h):
    n = L.ds2i_blob_size(h)
    out = (C.c_char * n).from_address(L.ds2i_blob_data(h)).raw
    L.ds2i_blob_free(h)
    return out


def host_build(kind):
    cuts = np.searchsorted(offs, np.linspace(0, int(offs[-1]), threads + 1)[1:-1]).tolist()
    bounds = [0] + cuts + [terms]
    o, da, fa = offs.tolist(), docs.ctypes.data, freqs.ctypes.data

    def part(i):
        b = C.c_void_p()
        check(L.ds2i_builder_create(kind, int(p.num_docs), C.byref(b)))
        add = L.ds2i_builder_add_posting_list
        for t in range(bounds[i], bounds[i + 1]):
            if add(b, o[t + 1] - o[t], C.c_void_p(da + 4 * o[t]), C.c_void_p(fa + 4 * o[t])):
                check(-1)
        h = C.c_void_p()
        check(L.ds2i_builder_freeze(b, C.byref(h)))
        L.ds2i_builder_free(b)
        return len(take(h))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        sizes = list(pool.map(part, range(threads)))
    return sum(sizes), time.perf_counter() - t0


def gpu_build(kind):
    h, ms, host = C.c_void_p(), C.c_double(), (C.c_double * 2)()
    t0 = time.perf_counter()
    check(L.ds2i_hip_encode_index(0, kind, int(p.num_docs), terms, ptr(offs), ptr(docs), ptr(freqs), C.byref(h), C.byref(ms)))
    dt = time.perf_counter() - t0
    L.ds2i_hip_encode_host_seconds(host)
    return take(h), dt, ms.value, host[0], host[1]


gpu_build(d.CODECS["ef"])  # warm-up: code objects, allocator
for name in d.FREQ_INDEX_KINDS:
    kind = d.CODECS[name]
    ref = d.synth_build(p, name, threads)[0]
    rows = []
    for rep in range(reps):
        _, hs = host_build(kind)
        img, gs, kms, plan_s, finish_s = gpu_build(kind)
        rows.append((hs, gs, kms, plan_s, finish_s, img == ref))
    best = min(rows, key=lambda r: r[1])
    print("%-8s image %d bytes | host builder (%d threads) %.3f s | gpu call %.3f s = plan %.3f s + kernels %.1f ms + download, headers, "
          "freeze %.3f s + check, staging %.3f s | identical: %s" % (name, len(ref), threads, min(r[0] for r in rows), best[1], best[3], best[2],
                                                                    best[4], best[1] - best[3] - 1e-3 * best[2] - best[4], all(r[5] for r in rows)), flush=True)


# ---- the two planners of opt
def planned_build(flags):
    h, ms, host, pms = C.c_void_p(), C.c_double(), (C.c_double * 2)(), C.c_double()
    t0 = time.perf_counter()
    check(L.ds2i_hip_encode_index_with(0, d.CODECS["opt"], int(p.num_docs), terms, ptr(offs), ptr(docs), ptr(freqs), flags, C.byref(h),
                                       C.byref(ms)))
    dt = time.perf_counter() - t0
    L.ds2i_hip_encode_host_seconds(host)
    L.ds2i_hip_encode_plan_ms(C.byref(pms))
    return take(h), dt, host[0], pms.value, ms.value, host[1]


def spread(xs):
    xs = sorted(xs)
    return "%.3f [%.3f, %.3f]" % (xs[len(xs) // 2], xs[0], xs[-1])


ref = d.synth_build(p, "opt", threads)[0]
rows = {"host": [], "device": []}
for rep in range(plan_reps):
    for name in ("host", "device"):
        img, dt, plan_s, plan_ms, all_ms, finish_s = planned_build({"host": 1, "device": 2}[name])  # DS2I_ENCODE_PLAN_*
        rows[name].append((dt, plan_s, plan_ms, all_ms, finish_s, img == ref))
for name, rs in rows.items():
    print("opt plan=%-6s whole call %s s | host planning %s s | partition kernels %s ms | all kernels %s ms | download, headers, freeze "
          "%s s | identical: %s" % (name, spread([r[0] for r in rs]), spread([r[1] for r in rs]), spread([r[2] for r in rs]),
                                   spread([r[3] for r in rs]), spread([r[4] for r in rs]), all(r[5] for r in rs)), flush=True)
print("partition scratch: %d bytes (12 per posting + 1 and side)" % (24 * (len(docs) + terms)), flush=True)

baseline = os.environ.get("DS2I_PROBE_BASELINE_LIB")
if baseline:
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for name, a in (("offs", offs), ("docs", docs), ("freqs", freqs)):
            np.save(os.path.join(tmp, name + ".npy"), a)
        child = ("import ctypes as C, numpy as np, sys, time\n"
                 "L = C.CDLL(sys.argv[1]); tmp = sys.argv[2]; reps = int(sys.argv[3])\n"
                 "offs, docs, freqs = (np.load(tmp + '/' + n + '.npy') for n in ('offs', 'docs', 'freqs'))\n"
                 "vp = C.c_void_p\n"
                 "L.ds2i_hip_encode_index.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_double)]\n"
                 "L.ds2i_blob_free.argtypes = [vp]\n"
                 "ts = []\n"
                 "for r in range(reps + 1):\n"
                 "    h, ms = vp(), C.c_double()\n"
                 "    t0 = time.perf_counter()\n"
                 "    rc = L.ds2i_hip_encode_index(0, 5, %d, len(offs) - 1, offs.ctypes.data, docs.ctypes.data, freqs.ctypes.data, C.byref(h), C.byref(ms))\n"
                 "    ts.append(time.perf_counter() - t0)\n"
                 "    assert rc == 0\n"
                 "    L.ds2i_blob_free(h)\n"
                 "ts = sorted(ts[1:])\n"
                 "print('baseline library opt call %%.3f [%%.3f, %%.3f] s' %% (ts[len(ts) // 2], ts[0], ts[-1]))\n") % int(p.num_docs)
        subprocess.run([sys.executable, "-c", child, baseline, tmp, str(plan_reps)], check=True, timeout=600)
