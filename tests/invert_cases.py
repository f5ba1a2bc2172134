"""The inputs of the inversion tests (test_invert_abi_cpu.py, test_gpu_invert.py) and the numpy references of the semantics of
ds2i_invert_documents and ds2i_transpose_postings. A forward collection is (doc_offsets uint64[num_docs + 1], tokens uint32): document d
is tokens[doc_offsets[d]:doc_offsets[d + 1]], term ids in any order, with repeats. Its inversion is, for every term, the documents that
hold it, strictly increasing, with the term's count in each; a CSR matrix is (offsets, ids, values). Everything is integers and every
answer is unique: all comparisons are exact."""
import numpy as np

from helpers import Collection

_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def numpy_invert(doc_offsets, tokens, nterms):
    """the reference: (list_offsets uint64[nterms + 1], docs, freqs, doc_sizes), via np.unique over (term, doc) pairs with counts"""
    offs = np.asarray(doc_offsets, dtype=np.int64)
    num_docs, n = len(offs) - 1, int(offs[-1])
    tokens = np.asarray(tokens[:n], dtype=np.int64)
    doc_of = np.repeat(np.arange(num_docs, dtype=np.int64), np.diff(offs))
    pairs, freqs = np.unique(tokens << 32 | doc_of, return_counts=True)
    list_offsets = np.zeros(nterms + 1, dtype=np.uint64)
    list_offsets[1:] = np.cumsum(np.bincount(pairs >> 32, minlength=nterms))
    return list_offsets, (pairs & 0xFFFFFFFF).astype(np.uint32), freqs.astype(np.uint32), np.diff(offs).astype(np.uint32)


def numpy_transpose(nrows, ncols, row_offsets, cols, vals):
    """the reference: (col_offsets uint64[ncols + 1], rows, vals); a stable sort by column keeps the rows of a column increasing"""
    offs = np.asarray(row_offsets, dtype=np.int64)
    n = int(offs[-1])
    cols, vals = np.asarray(cols[:n], dtype=np.int64), np.asarray(vals[:n], dtype=np.uint32)
    row_of = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(offs))
    order = np.argsort(cols, kind="stable")
    col_offsets = np.zeros(ncols + 1, dtype=np.uint64)
    col_offsets[1:] = np.cumsum(np.bincount(cols, minlength=ncols))
    return col_offsets, row_of[order].astype(np.uint32), vals[order]


def assert_csr_equal(got, want, what=""):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), "%s: array %d" % (what, k)


def from_documents(docs):
    """a list of token arrays as (doc_offsets, tokens)"""
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in docs])
    return offs, (np.concatenate(docs) if docs else np.zeros(0)).astype(np.uint32)


def forward_arrays(coll, seed):
    """a Collection written as documents: every term repeated freq times, the tokens of every document shuffled with a seeded generator"""
    rng = np.random.default_rng(seed)
    term = np.concatenate([np.full(len(dd), t, dtype=np.int64) for t, (dd, _) in enumerate(coll.lists)])
    doc = np.concatenate([dd.astype(np.int64) for dd, _ in coll.lists])
    freq = np.concatenate([ff.astype(np.int64) for _, ff in coll.lists])
    tok_term, tok_doc = np.repeat(term, freq), np.repeat(doc, freq)
    order = np.lexsort((rng.random(len(tok_doc)), tok_doc))  # by document, at random within it
    offs = np.zeros(coll.num_docs + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(tok_doc, minlength=coll.num_docs))
    return offs, tok_term[order].astype(np.uint32)


def forward_of(coll, seed=0xF0D):
    return _once(("forward", id(coll), seed), lambda: forward_arrays(coll, seed))


def with_token_sizes(coll):
    """coll': the collection with `sizes` replaced by the token counts, what an inversion of forward_of(coll) knows of the documents"""
    def make():
        sizes = np.zeros(coll.num_docs, dtype=np.int64)
        for dd, ff in coll.lists:
            sizes[dd] += ff
        return Collection.from_lists(coll.num_docs, coll.lists, sizes.astype(np.uint32))
    return _once(("token sizes", id(coll)), make)


def csr_of(coll):
    """the posting lists of a Collection as a CSR matrix, terms by documents"""
    offs = np.zeros(len(coll.lists) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(dd) for dd, _ in coll.lists])
    return offs, np.concatenate([dd for dd, _ in coll.lists]), np.concatenate([ff for _, ff in coll.lists])


def expand(doc_offsets, terms, freqs):
    """a forward index (documents by terms, with freqs) written out as tokens"""
    num_docs = len(doc_offsets) - 1
    doc_of = np.repeat(np.arange(num_docs), np.diff(doc_offsets.astype(np.int64)))
    offs = np.zeros(num_docs + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(doc_of, weights=freqs, minlength=num_docs).astype(np.int64))
    return offs, np.repeat(terms, freqs).astype(np.uint32)


def write_forward(path, doc_offsets, tokens):
    """one sequence [n][n x u32] per document, empty ones included, no leading singleton"""
    with open(path, "wb") as f:
        for a, b in zip(doc_offsets[:-1], doc_offsets[1:]):
            np.array([int(b) - int(a)], dtype=np.uint32).tofile(f)
            np.asarray(tokens[int(a):int(b)], dtype=np.uint32).tofile(f)


# ---------------------------------------------------------------- small edge inputs
NTERMS_SMALL = 12


def small_edges():
    """(doc_offsets, tokens): an empty document first, last and between two others; a document of one token, one of one term repeated,
    two neighbours that end and begin with the same term (11, the largest), and terms (4, 9) that never occur"""
    docs = [[], [3], [7, 7, 7, 7], [], [0, 11, 5, 0, 11], [11, 2, 11], [], [1, 10, 6, 8, 1, 1], []]
    return from_documents([np.array(x, dtype=np.uint32) for x in docs])


# ---------------------------------------------------------------- document-length edges of the segmented sort
def length_edge_documents(bounds, pool=300):
    """(lengths, (doc_offsets, tokens)): documents of 0, 1, 2, 63, 64, 65, L - 1, L, L + 1, T - 1, T, T + 1 and 2 T + 1 tokens with an
    empty document first, last and between two others; tokens drawn with replacement from `pool` terms, so freqs > 1 are common"""
    def make():
        W, L, T = bounds
        lengths = [0, 1, 2, 63, 0, 64, 65, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T + 1, 0]
        rng = np.random.default_rng(0x1E46)
        return lengths, from_documents([rng.integers(0, pool, n).astype(np.uint32) for n in lengths])
    return _once(("length_edges", tuple(bounds), pool), make)


# ---------------------------------------------------------------- run edges of the run-length step
RUN_TERM = 5


def run_edge_documents(V, whole_windows):
    """(runs, (doc_offsets, tokens), nterms): documents that are n copies of one term for n in V, 1, 63, 64, 65, V - 1, V + 1,
    2 V + 1, 3 V - 1 -- the run of V comes first, so the second document starts on a window boundary as the first does, the others in
    mid-window -- each a term of its own but for pairs of neighbours that share RUN_TERM: one pair whose boundary lies between lane 63
    and lane 0 of a step and one whose boundary is a window edge. whole_windows: a filler document ends the tokens on a window boundary.
    runs: the (document, term, freq) every document must yield."""
    def make():
        docs, runs = [], []

        def add(term, n):
            runs.append((len(docs), term, n))
            docs.append(np.full(n, term, dtype=np.uint32))

        for k, n in enumerate([V, 1, 63, 64, 65, V - 1, V + 1, 2 * V + 1, 3 * V - 1]):
            add(10 + k, n)
        at = sum(len(x) for x in docs)
        add(30, -at % 64 or 64)            # up to a step boundary
        add(RUN_TERM, 64)                  # ends with lane 63 ...
        add(RUN_TERM, 3)                   # ... and the same term begins in lane 0: two postings of RUN_TERM
        at = sum(len(x) for x in docs)
        add(31, (-at - 7) % V or V)        # up to 7 tokens before a window edge
        add(RUN_TERM, 7)                   # ends on the window edge ...
        assert sum(len(x) for x in docs) % V == 0
        add(RUN_TERM, V + 2)               # ... and the same term goes on for more than a window
        add(32, 5)
        if whole_windows:
            add(33, -sum(len(x) for x in docs) % V or V)
        total = sum(len(x) for x in docs)
        assert (total % V == 0) == whole_windows
        return runs, from_documents(docs), 40
    return _once(("run_edges", V, whole_windows), make)


# ---------------------------------------------------------------- a term in every document
def every_document_case(num_docs=20000):
    """(doc_offsets, tokens, nterms): documents of 3 to 40 tokens that all hold term 0 (once or more), terms 1 .. 199 at random, terms
    200 .. 399 exactly once in the whole collection each, and terms 400 .. 449 never"""
    def make():
        rng = np.random.default_rng(0xE7E4)
        lengths = rng.integers(3, 41, num_docs)
        docs = [rng.integers(0, 200, n).astype(np.uint32) for n in lengths]
        for x in docs:
            x[rng.integers(0, len(x))] = 0
        for t, dnum in zip(range(200, 400), rng.choice(num_docs, 200, replace=False)):
            docs[dnum] = np.concatenate([docs[dnum][:2], [t], docs[dnum][2:]]).astype(np.uint32)
        return from_documents(docs) + (450,)
    return _once(("every_document", num_docs), make)


# ---------------------------------------------------------------- ids past 2^24
PAST_2_24 = (1 << 24) + 5


def past_2_24_documents():
    """(doc_offsets, tokens, nterms): 2^24 + 5 documents, all empty but a few dozen on both sides of 2^24, over 50 terms"""
    def make():
        rng = np.random.default_rng(0x2A24)
        ids = np.unique(np.concatenate([rng.integers(0, 1 << 24, 40), np.arange((1 << 24) - 3, PAST_2_24), [0]]))
        sizes = np.zeros(PAST_2_24, dtype=np.int64)
        sizes[ids] = rng.integers(1, 30, len(ids))
        offs = np.zeros(PAST_2_24 + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(sizes)
        return offs, rng.integers(0, 50, int(offs[-1])).astype(np.uint32), 50
    return _once("past_docs", make)


def past_2_24_terms():
    """(doc_offsets, tokens, nterms): 40 documents whose tokens are term ids on both sides of 2^24 of 2^24 + 5 terms, with repeats"""
    def make():
        rng = np.random.default_rng(0x2A25)
        pool = np.concatenate([rng.integers(0, 1 << 24, 30), np.arange((1 << 24) - 3, PAST_2_24), [0]]).astype(np.uint32)
        return from_documents([rng.choice(pool, n) for n in rng.integers(0, 90, 40)]) + (PAST_2_24,)
    return _once("past_terms", make)
