"""Cost of the doc-ids (DS2I_OP_TOPK_DOCS): fresh 4096-query batches through a depth-3 Pipeline with and without with_docs,
on bench.py's GOV2-scale collection and query generator (imported), ranked_and and wand at k = 10 and k = 100.

`python profiles/probes/topk_docs_probe.py [--steps 20] [--warmup 5] [--out FILE]` prints one JSON line per (op, k, mode) and
the docs / scores-only rate ratio; --out also writes them as one JSON document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (WORKLOADS: the collection bench.py measures)
import ds2i_amd as d  # noqa: E402


def rate(idx, op, k, flat, steps, warmup, with_docs, depth=3):
    pipe = d.Pipeline(idx, depth=depth)
    inflight, t0 = [], None
    nq = len(flat[0][1]) - 1
    for i, fq in enumerate(flat[:warmup + steps]):
        if i == warmup:
            while inflight:
                (pipe.wait_docs if with_docs else pipe.wait)(inflight.pop(0))
            t0 = time.perf_counter()
        inflight.append(pipe.submit(op, fq, k=k, with_docs=with_docs))
        if len(inflight) == depth:
            (pipe.wait_docs if with_docs else pipe.wait)(inflight.pop(0))
    while inflight:
        (pipe.wait_docs if with_docs else pipe.wait)(inflight.pop(0))
    dt = time.perf_counter() - t0
    pipe.close()
    return steps * nq / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    # (the workloads whose queries bench.py draws with synth_queries: the topical one draws them otherwise)
    ap.add_argument("--workload", default="gov2", choices=sorted(w for w in bench.WORKLOADS if not bench.WORKLOADS[w].get("topics")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W = bench.WORKLOADS[args.workload]
    p = d.SynthParams(seed=W["seed"], num_docs=W["num_docs"], num_terms=W["num_terms"], zipf_exp=W["zipf_exp"], top_df_frac=W["top_df_frac"],
                      min_len=W["min_len"], clustered_every=W["clustered_every"], topics=W.get("topics", 0), topic_boost=W.get("topic_boost", 0))
    t0 = time.time()
    img, wand, postings = d.synth_build(p, "block_optpfor", min(16, os.cpu_count() or 8))
    idx = d.Index("block_optpfor", img, wand)
    del img
    print("built + uploaded %s: %d postings, %.0fs" % (args.workload, postings, time.time() - t0), file=sys.stderr)
    n = args.steps + args.warmup
    # bench.py's query stream (rank 0, weak scaling): batch i of 4096 queries from seed 0x51E21 + 7919 i
    flat = [d.flatten_queries(d.synth_queries(0x51E21 + 7919 * i, p.num_terms, 4096)) for i in range(n)]
    rows = []
    for op in ("ranked_and", "wand"):
        for k in (10, 100):
            r = {}
            for mode in ("scores", "docs", "scores", "docs"):  # (interleaved twice: the second pass is the one reported, the first warms)
                r[mode] = rate(idx, op, k, flat, args.steps, args.warmup, mode == "docs")
            row = {"op": op, "k": k, "scores_qps": round(r["scores"]), "docs_qps": round(r["docs"]), "ratio": round(r["docs"] / r["scores"], 3)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        json.dump({"workload": args.workload, "batch": 4096, "depth": 3, "steps": args.steps, "rows": rows}, open(args.out, "w"), indent=1)
    idx.close()


if __name__ == "__main__":
    main()
