"""Multi-GPU sharding of a query batch: one process per GPU, index replicated in every GPU's HBM,
queries partitioned into contiguous slices, results concatenated on rank 0. The path has no exchange
step, so there is no data-path collective; torch.distributed (RCCL on GPUs, gloo on CPU)
is only used for rendezvous, barriers, the max-over-ranks timing and the result gather.

Document shards, one per GPU and process, are the other way to use several GPUs: every rank answers the whole batch over its shard
(an index with the collection's statistics, Index.set_collection_stats) and merge_topk_over_ranks gathers and merges the rows."""
import os

import numpy as np


def init_distributed(backend=None):
    """-> (rank, local_rank, world_size, dist-or-None). Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return rank, local_rank, world, None
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        torch.cuda.set_device(local_rank)  # one process per GPU
    if not dist.is_initialized():
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, local_rank, world, dist


def query_slice(nq, rank, world):
    """Contiguous slice [begin, end) of a batch of nq queries owned by `rank` (sizes differ by at most 1)."""
    base, rem = divmod(nq, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


def _device(dist):
    import torch
    return "cuda" if dist.get_backend() == "nccl" else "cpu"


def share_bytes(dist, rank, blob, path):
    """Rank 0 holds `blob`; every rank returns it. Goes through a file (page cache / tmpfs), not a collective:
    a GOV2-scale index image is gigabytes."""
    if dist is None:
        return blob
    if rank == 0:
        with open(path, "wb") as f:
            f.write(blob)
    dist.barrier()
    if rank != 0:
        with open(path, "rb") as f:
            blob = f.read()
    dist.barrier()
    if rank == 0:
        os.remove(path)
    return blob


def max_over_ranks(dist, value):
    if dist is None:
        return float(value)
    import torch
    t = torch.tensor([float(value)], dtype=torch.float64, device=_device(dist))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def broadcast_int(dist, value, src=0):
    if dist is None:
        return int(value)
    import torch
    t = torch.tensor([int(value)], dtype=torch.int64, device=_device(dist))
    dist.broadcast(t, src)
    return int(t.item())


def gather_concat(dist, rank, world, local):
    """Concatenates per-rank result arrays (first axis) in rank order on every rank."""
    local = np.ascontiguousarray(local)
    if dist is None:
        return local
    import torch
    dev = _device(dist)
    n = torch.tensor([local.shape[0]], dtype=torch.int64, device=dev)
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(sizes, n)
    sizes = [int(s.item()) for s in sizes]
    m = max(sizes) if sizes else 0
    pad = np.zeros((m,) + local.shape[1:], dtype=local.dtype)
    pad[:local.shape[0]] = local
    raw = torch.from_numpy(pad.view(np.uint8).reshape(m, -1) if m else np.zeros((0, 1), np.uint8)).to(dev)
    outs = [torch.zeros_like(raw) for _ in range(world)]
    dist.all_gather(outs, raw)
    parts = []
    for r in range(world):
        a = outs[r].cpu().numpy().reshape(-1).view(local.dtype).reshape((m,) + local.shape[1:])
        parts.append(a[:sizes[r]])
    return np.concatenate(parts, axis=0)


def rows_in_collection_order(scores, docs, lens, doc_map=None):
    """The top-k rows of one shard (scores float32[nq, k], docs uint32[nq, k] LOCAL doc-ids, lens uint32[nq]) with their ids mapped
    to the collection's (doc_map: local -> collection doc-id; None: they are the collection's already) and every row put into the
    order of the merge: score descending, equal scores by COLLECTION doc-id ascending. A shard returns its equal-score runs in
    local-id order, which under a doc map that does not increase is another order; a merge that is handed collection ids without a
    map (ds2i_hip_merge_topk with doc_map == NULL) relies on rows in this order. Entries past a row's length become -inf /
    0xFFFFFFFF. Returns (scores, docs, lens)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    docs = np.ascontiguousarray(docs, dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    if scores.ndim != 2 or docs.shape != scores.shape or lens.shape != (scores.shape[0],):
        raise ValueError("rows of one rank: scores and docs [nq, k], lens [nq]")
    nq, k = scores.shape
    if int(lens.max(initial=0)) > k:
        raise ValueError("a row is longer than k")
    live = np.arange(k)[None, :] < lens[:, None]
    ids = docs
    if doc_map is not None:
        doc_map = np.asarray(doc_map, dtype=np.uint32)
        if live.any() and int(docs[live].max()) >= len(doc_map):
            raise ValueError("a local doc-id lies outside the doc map")
        ids = np.zeros_like(docs)
        ids[live] = doc_map[docs[live]]
    # the merge's key: ((0xFFFFFFFF - bits(score)) << 32) | collection doc-id; what lies past a row's length sorts last
    key = ((np.uint64(0xFFFFFFFF) - scores.view(np.uint32).astype(np.uint64)) << np.uint64(32)) | ids.astype(np.uint64)
    key = np.sort(np.where(live, key, np.uint64(0xFFFFFFFFFFFFFFFF)), axis=1)
    out_scores = (np.uint64(0xFFFFFFFF) - (key >> np.uint64(32))).astype(np.uint32).view(np.float32)
    out_scores = np.where(live, out_scores, np.float32(-np.inf)).astype(np.float32)
    out_docs = np.where(live, key & np.uint64(0xFFFFFFFF), 0xFFFFFFFF).astype(np.uint32)
    return out_scores, out_docs, lens


def merge_topk_over_ranks(dist, rank, world, scores, docs, lens, doc_map=None, device=None):
    """Document shards, one per GPU and process: every rank holds the top-k rows its shard answered for the SAME nq queries and k
    (scores float32[nq, k], docs uint32[nq, k] local doc-ids, lens uint32[nq]; doc_map: local -> collection doc-id, None: the ids are
    the collection's). On every rank the ids are mapped and the rows put into the merge's order (rows_in_collection_order: a doc map
    need not increase), every rank's rows are gathered, and every rank returns the merge (ds2i_amd.merge_topk's order: score
    descending, equal scores by collection doc-id ascending): (scores, docs, lens) of the whole collection. device: merge with the HIP
    kernel on that device (gpu_merge_topk); None: the host twin. The replica helpers above shard the queries; this one shards the
    documents."""
    from . import api
    scores, docs, lens = rows_in_collection_order(scores, docs, lens, doc_map)
    nq, k = scores.shape
    all_scores = gather_concat(dist, rank, world, scores)
    all_docs = gather_concat(dist, rank, world, docs)
    all_lens = gather_concat(dist, rank, world, lens)
    if len(all_lens) != nq * (world if dist is not None else 1):
        raise ValueError("the ranks hold different numbers of queries")
    rows = [(all_scores[r * nq:(r + 1) * nq], all_docs[r * nq:(r + 1) * nq], all_lens[r * nq:(r + 1) * nq])
            for r in range(len(all_lens) // nq if nq else 0)]
    if not rows:
        return scores, docs, lens
    if device is None:
        return api.merge_topk(rows, k)
    return api.gpu_merge_topk(rows, k, device=device)[:3]
