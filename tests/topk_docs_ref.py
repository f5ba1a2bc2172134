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


def _norm64(coll):
    """float64 size / average size of every document (kept on the collection: 17 M documents are not divided once per query)"""
    if getattr(coll, "_norm64", None) is None:
        sizes = coll.sizes.astype(np.float64)
        coll._norm64 = sizes / (sizes.sum() / coll.num_docs)
    return coll._norm64


def doc_scores64(coll, terms, docs):
    """float64 BM25 (helpers.topk64's arithmetic) of the given documents for `terms`"""
    k1, b = 1.2, 0.5
    qtf = {}
    for t in terms:
        qtf[int(t)] = qtf.get(int(t), 0) + 1
    n_docs = coll.num_docs
    norm = _norm64(coll)
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


# ---------------------------------------------------------------- exact checks of the tie rule that need no model of a kernel's arithmetic
def signature_keys(coll, terms, docs):
    """The signature of a document for a query is (size, freq in term 1 or 0, ..., freq in term n or 0) over the query's distinct
    terms: two documents with the same signature get the same score bits from any deterministic arithmetic (the union kernels'
    fixed-point sum included: it does not depend on the order of the terms). Returned packed into one uint64 per document
    (comparable within this collection and query only)."""
    ts = sorted(set(int(t) for t in terms))
    docs = np.asarray(docs, dtype=np.uint32)
    if getattr(coll, "_usizes", None) is None:
        coll._usizes = np.unique(coll.sizes)
    key = np.searchsorted(coll._usizes, coll.sizes[docs]).astype(np.uint64)
    shift = max(1, int(len(coll._usizes) - 1).bit_length())
    for t in ts:
        ld, lf = coll.lists[t]
        bits = int(lf.max()).bit_length()
        assert shift + bits <= 64, "signature does not fit 64 bits"
        if len(docs) <= len(ld):  # look the documents up in the list, or the list's postings in the (ascending) documents
            pos = np.minimum(np.searchsorted(ld, docs), len(ld) - 1)
            key |= np.where(ld[pos] == docs, lf[pos], 0).astype(np.uint64) << np.uint64(shift)
        elif len(docs):
            pos = np.minimum(np.searchsorted(docs, ld), len(docs) - 1)
            hit = docs[pos] == ld
            key[pos[hit]] |= lf[hit].astype(np.uint64) << np.uint64(shift)
        shift += bits
    return key


class TieRef:
    """What the checks below need of one result set (AND or OR of `terms`: scored_docs' document set, without its float32 scores,
    which no check here reads), built once per query: of every signature the `keep` smallest doc-ids (no top-k of k < keep may hold another), without the signatures that score clearly below the
    keep-th document (float64, 1e-3 relative: a hundred times the tolerance of the checks). n is the size of the whole result set,
    top64 its `keep` largest float64 scores."""

    def __init__(self, coll, terms, conjunctive, keep=1025):
        docs = (brute_and if conjunctive else brute_or)(coll, terms)
        self.terms, self.n, self.keep = list(terms), len(docs), keep
        key = signature_keys(coll, terms, docs)
        o = np.argsort(key, kind="stable")                    # by signature, then doc-id (docs are ascending)
        ks = key[o]
        first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if self.n else np.zeros(0, dtype=np.int64)
        count = np.diff(np.concatenate([first, [self.n]]))
        g64 = doc_scores64(coll, terms, docs[o[first]])       # one float64 score per signature
        by = np.argsort(-g64, kind="stable")
        cum = np.cumsum(count[by])
        kth = g64[by[min(int(np.searchsorted(cum, keep)), len(by) - 1)]] if self.n else 0.0
        group = np.repeat(np.arange(len(first)), count)
        rank = np.arange(self.n) - np.repeat(first, count)
        sel = (rank < keep) & (g64[group] >= kth * (1 - 1e-3))
        idx = np.sort(o[sel])                                 # back to doc-id order
        inv = np.empty(self.n, dtype=np.int64)
        inv[o] = np.arange(self.n)
        self.docs, self.key = docs[idx], key[idx]
        self.rank, self.s64 = rank[inv[idx]], g64[group[inv[idx]]]
        self.by_score = np.lexsort((self.docs, -self.s64))    # float64 score descending, doc-id ascending
        self.top64 = self.s64[self.by_score[:keep]]

    def tied_at(self, k):
        """more than k results, and the k-th and the (k+1)-th score equal"""
        return self.n > k and self.top64[k - 1] == self.top64[k]

    def locate(self, ids):
        """positions of the returned ids among the kept documents (-1: not among them)"""
        ids = np.asarray(ids, dtype=np.uint32)
        if not len(self.docs):
            return np.full(len(ids), -1, dtype=np.int64)
        pos = np.minimum(np.searchsorted(self.docs, ids), len(self.docs) - 1)
        return np.where(self.docs[pos] == ids, pos, -1)


def _strangers(ref, ids, pos):
    if np.all(pos >= 0):
        return None
    i = int(np.flatnonzero(pos < 0)[0])
    return "rank %d: doc %d is not in the result set, or scores far below its %d-th document, or has %d smaller doc-ids of its signature" % (
        i, int(ids[i]), ref.keep, ref.keep)


def same_signature_same_bits(ref, ids, scores):
    """returned documents with equal signatures carry equal score bits -> None, or what is wrong"""
    pos = ref.locate(ids)
    bad = _strangers(ref, ids, pos)
    if bad:
        return bad
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    o = np.lexsort((bits, ref.key[pos]))
    k, b = ref.key[pos][o], bits[o]
    diff = np.flatnonzero((k[1:] == k[:-1]) & (b[1:] != b[:-1]))
    if len(diff):
        i, j = int(o[diff[0]]), int(o[diff[0] + 1])
        return "ranks %d and %d: docs %d and %d have one signature and score bits %08x and %08x" % (i, j, int(ids[i]), int(ids[j]), int(bits[i]), int(bits[j]))
    return None


def closed_within_signature(ref, ids):
    """if a returned document has signature s, every document of the result set with signature s and a smaller doc-id is returned
    too (the k-th-place rule, at every rank) -> None, or what is wrong"""
    pos = ref.locate(ids)
    bad = _strangers(ref, ids, pos)
    if bad:
        return bad
    key, rank = ref.key[pos], ref.rank[pos]
    o = np.lexsort((rank, key))
    k, r = key[o], rank[o]
    start = np.concatenate([[True], k[1:] != k[:-1]]) if len(k) else np.zeros(0, dtype=bool)
    want = np.arange(len(k)) - np.maximum.accumulate(np.where(start, np.arange(len(k)), 0))
    miss = np.flatnonzero(r != want)
    if len(miss):
        i = int(o[miss[0]])
        left = ref.docs[(ref.key == key[i]) & (ref.rank == want[miss[0]])]
        return "rank %d: doc %d was returned, doc %d with the same signature and a smaller doc-id was not" % (i, int(ids[i]), int(left[0]))
    return None


def nothing_better_left_out(ref, ids, k, rtol=1e-5):
    """no document that was not returned scores (float64) above the k-th returned score by more than rtol; fewer than k returned:
    the whole result set -> None, or what is wrong"""
    if len(ids) != min(k, ref.n):
        return "%d documents returned, the result set holds %d (k = %d)" % (len(ids), ref.n, k)
    if len(ids) < k or not len(ids):
        return None
    pos = ref.locate(ids)
    bad = _strangers(ref, ids, pos)
    if bad:
        return bad
    kth = float(ref.s64[pos[-1]])
    head = ref.by_score[:k + 1]                               # (one of the k + 1 best is not returned: the best such is the best left out)
    out = head[~np.isin(ref.docs[head], ids)]
    if len(out) and ref.s64[out[0]] > kth * (1 + rtol):
        return "rank %d: doc %d (%.9g) was returned, doc %d (%.9g) was not" % (len(ids) - 1, int(ids[-1]), kth, int(ref.docs[out[0]]), float(ref.s64[out[0]]))
    return None
