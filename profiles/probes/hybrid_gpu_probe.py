"""block_mixed optimiser: host threads vs the GPU entry points on the 4096-term configs[1]-shaped collection (1 M docs, seed
0xD5210002). Wall time of analyse + freeze on each side (the GPU side includes staging, upload, download and
the host hull building), the kernels' hipEvent time, and whether the two images are the same bytes.
    python profiles/probes/hybrid_gpu_probe.py [threads] [--gpu-only]
--gpu-only: one GPU analyse + freeze and nothing else (the form to run under rocprofv3 --kernel-trace --stats)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import ds2i_amd as d

args = [a for a in sys.argv[1:] if not a.startswith("--")]
threads = int(args[0]) if args else 16
gpu_only = "--gpu-only" in sys.argv
p = d.SynthParams(seed=0xD5210002, num_docs=1000000, num_terms=4096, zipf_exp=0.75, top_df_frac=0.5, min_len=128, clustered_every=4)
lists = [d.synth_list(p, t) for t in range(p.num_terms)]
postings = sum(len(dd) for dd, _ in lists)
blocks = sum((len(dd) + 127) // 128 for dd, _ in lists)
access = np.random.default_rng(7).integers(0, 1000, (blocks, 2)).astype(np.uint32)


def builder():
    hb = d.HybridBuilder(p.num_docs)
    base = 0
    for dd, ff in lists:
        nb = (len(dd) + 127) // 128
        hb.add_posting_list(dd, ff, access[base:base + nb])
        base += nb
    return hb


def run(device):
    hb = builder()
    t0 = time.perf_counter()
    lo, hi = hb.analyse(threads=threads, device=device)
    t1 = time.perf_counter()
    img, info = hb.freeze(int(lo + 0.5 * (hi - lo)), threads=threads, device=device)
    t2 = time.perf_counter()
    ms = (hb.device_ms, info["device_ms"]) if device is not None else (0.0, 0.0)
    return img, info, t1 - t0, t2 - t1, ms


print("%d lists, %d postings, %d parts" % (len(lists), postings, 2 * blocks))
if gpu_only:
    _, info, ta, tf, ms = run(0)
    print("gpu analyse %.3f s (kernel %.1f ms) freeze %.3f s (kernel %.1f ms)" % (ta, ms[0], tf, ms[1]))
    sys.exit(0)
run(0)  # warm-up: code objects, allocator
rows = []
for rep in range(3):  # alternating, same process
    himg, hinfo, ha, hf, _ = run(None)
    gimg, ginfo, ga, gf, ms = run(0)
    same = gimg == himg and all(ginfo[k] == hinfo[k] for k in ("rate", "space", "model_time", "type_counts"))
    rows.append((ha, hf, ga, gf, ms[0], ms[1], same))
    print("rep %d: host(%d threads) analyse %.3f s freeze %.3f s | gpu analyse %.3f s (kernel %.1f ms) freeze %.3f s (kernel %.1f ms) | identical: %s"
          % (rep, threads, ha, hf, ga, gf, ms[0], ms[1], same))
print("type_counts", hinfo["type_counts"], "image %.1f MB" % (len(himg) / 1e6))
med = lambda i: sorted(r[i] for r in rows)[1]
print("median: host %.3f s, gpu %.3f s (kernels %.1f ms): %.1fx" % (med(0) + med(1), med(2) + med(3), med(4) + med(5), (med(0) + med(1)) / (med(2) + med(3))))
