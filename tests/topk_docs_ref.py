"""Canonical (score, doc-id) top-k of a brute-force float32 BM25 (the reference for DS2I_OP_TOPK_DOCS / TOPK_DOCS).

The arithmetic and term order are those of helpers.brute_ranked (size order for ranked_and); the ranking is the contract's
total order: score descending, equal scores by doc-id ascending, so on a tie at the k-th place the smaller doc-ids are kept."""
import numpy as np

from helpers import _term_freqs, brute_and, brute_or, doc_term_weight, query_term_weight


def scored_docs(coll, terms, conjunctive, order="size"):
    """(doc-ids ascending, float32 scores) of the AND / OR result set of `terms`"""
    tf = _term_freqs(terms)
    if not tf:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)
    N = coll.num_docs
    ents = []
    for t, qtf in tf:
        docs, _ = coll.lists[t]
        ents.append((len(docs), t, query_term_weight(qtf, len(docs), N)))
    if order == "size":
        ents.sort(key=lambda e: e[0])
    docset = brute_and(coll, [t for t, _ in tf]) if conjunctive else brute_or(coll, [t for t, _ in tf])
    score = np.zeros(len(docset), dtype=np.float32)
    if len(docset) == 0:
        return docset, score
    nl = coll.norm_lens[docset]
    for _, t, qw in ents:
        docs, freqs = coll.lists[t]
        pos = np.minimum(np.searchsorted(docs, docset), len(docs) - 1)
        hit = docs[pos] == docset
        w = (qw * doc_term_weight(freqs[pos], nl)).astype(np.float32)
        score = np.where(hit, (score + w).astype(np.float32), score)
    return docset, score


def canonical_topk(docs, scores, k):
    """the k largest (score, -doc) pairs, in that order -> (scores float32, doc-ids uint32)"""
    o = np.lexsort((docs.astype(np.int64), -scores.astype(np.float64)))[:k]
    return scores[o].astype(np.float32), docs[o].astype(np.uint32)


def brute_pairs(coll, terms, k, conjunctive, order="size"):
    d, s = scored_docs(coll, terms, conjunctive, order)
    return canonical_topk(d, s, k)


def doc_scores64(coll, terms, docs):
    """float64 BM25 (helpers.topk64's arithmetic) of the given documents for `terms`"""
    k1, b = 1.2, 0.5
    qtf = {}
    for t in terms:
        qtf[int(t)] = qtf.get(int(t), 0) + 1
    n_docs = coll.num_docs
    sizes = coll.sizes.astype(np.float64)
    norm = sizes / (sizes.sum() / n_docs)
    out = np.zeros(len(docs))
    docs = np.asarray(docs, dtype=np.int64)
    for t, f in qtf.items():
        ld, lf = coll.lists[t]
        df = float(len(ld))
        idf = max(1e-6, np.log(float(np.float32((n_docs - df + 0.5) / (df + 0.5)))))
        pos = np.minimum(np.searchsorted(ld, docs), len(ld) - 1)
        hit = ld[pos] == docs
        tf = lf[pos].astype(np.float64)
        out += np.where(hit, f * idf * (1.0 + k1) * tf / (tf + k1 * (1.0 - b + b * norm[docs])), 0.0)
    return out


def member_any(coll, terms, docs):
    """for each doc: does it hold at least one of the terms"""
    m = np.zeros(len(docs), dtype=bool)
    for t in set(int(x) for x in terms):
        ld = coll.lists[t][0]
        pos = np.minimum(np.searchsorted(ld, docs), len(ld) - 1)
        m |= ld[pos] == docs
    return m
