"""Shared test helpers: tiny seeded collections and a codec-independent brute-force oracle (numpy)."""
import numpy as np

import ds2i_amd as d

K1, B = np.float32(1.2), np.float32(0.5)


def small_params(num_docs=20000, num_terms=300, seed=0xD5210001, min_len=1, top=0.5, clustered_every=4):
    return d.SynthParams(seed=seed, num_docs=num_docs, num_terms=num_terms, zipf_exp=0.75, top_df_frac=top,
                         min_len=min_len, clustered_every=clustered_every)


class Collection:
    """A materialised synthetic collection: lists, doc sizes, norm_lens (float32 like wand_data.hpp:24-36)."""

    def __init__(self, p):
        self.p = p
        self.num_docs = int(p.num_docs)
        self.lists = [d.synth_list(p, t) for t in range(p.num_terms)]
        self.sizes = d.synth_doc_sizes(p)
        self._norm_lens()

    @classmethod
    def from_lists(cls, num_docs, lists, sizes):
        """A collection of explicit posting lists [(docs, freqs)] and per-document sizes (no synthetic parameters: p is None)."""
        self = cls.__new__(cls)
        self.p = None
        self.num_docs = int(num_docs)
        self.lists = [(np.asarray(dd, dtype=np.uint32), np.asarray(ff, dtype=np.uint32)) for dd, ff in lists]
        self.sizes = np.asarray(sizes, dtype=np.uint32)
        assert len(self.sizes) == self.num_docs
        for dd, ff in self.lists:
            assert len(dd) == len(ff) and len(dd) > 0 and np.all(np.diff(dd.astype(np.int64)) > 0) and int(dd[-1]) < self.num_docs
            assert np.all(ff > 0)
        self._norm_lens()
        return self

    def _norm_lens(self):
        lens = self.sizes.astype(np.float32)
        avg = np.float32(lens.astype(np.float64).sum() / float(self.num_docs))
        self.norm_lens = (lens / avg).astype(np.float32)

    def index_image(self, codec):
        return d.build_index(codec, self.num_docs, self.lists)

    def wand_image(self):
        return d.build_wand(self.sizes, self.lists)


def doc_term_weight(freq, norm_len):
    f = freq.astype(np.float32)
    return (f / (f + K1 * ((np.float32(1.0) - B) + B * norm_len))).astype(np.float32)


def query_term_weight(qtf, df, num_docs):
    f, fdf = np.float32(qtf), np.float32(df)
    idf = np.float32(np.log(np.float32((np.float32(num_docs) - fdf + np.float32(0.5)) / (fdf + np.float32(0.5)))))
    return np.float32(f * max(np.float32(1.0e-6), idf) * (np.float32(1.0) + K1))


def brute_and(coll, terms):
    ts = sorted(set(terms))
    if not ts:
        return np.zeros(0, dtype=np.uint32)
    out = coll.lists[ts[0]][0]
    for t in ts[1:]:
        out = np.intersect1d(out, coll.lists[t][0], assume_unique=True)
    return out.astype(np.uint32)


def brute_or(coll, terms):
    ts = sorted(set(terms))
    if not ts:
        return np.zeros(0, dtype=np.uint32)
    return np.unique(np.concatenate([coll.lists[t][0] for t in ts])).astype(np.uint32)


def _term_freqs(terms):
    ts = sorted(terms)
    out = []
    for t in ts:
        if out and out[-1][0] == t:
            out[-1][1] += 1
        else:
            out.append([t, 1])
    return out


def brute_ranked(coll, terms, k, conjunctive, order="size"):
    """top-k BM25 scores (descending) of the AND / OR result set. Scores are float32 sums in the
    reference's enumerator order: size-sorted for ranked_and (queries.hpp:357-360), term order for ranked_or."""
    tf = _term_freqs(terms)
    if not tf:
        return np.zeros(0, dtype=np.float32)
    N = coll.num_docs
    ents = []
    for t, qtf in tf:
        docs, freqs = coll.lists[t]
        ents.append((len(docs), t, query_term_weight(qtf, len(docs), N)))
    if order == "size":
        ents.sort(key=lambda e: e[0])  # python sort is stable, like insertion sort on <=16 elements
    docset = brute_and(coll, [t for t, _ in tf]) if conjunctive else brute_or(coll, [t for t, _ in tf])
    if len(docset) == 0:
        return np.zeros(0, dtype=np.float32)
    nl = coll.norm_lens[docset]
    score = np.zeros(len(docset), dtype=np.float32)
    for _, t, qw in ents:
        docs, freqs = coll.lists[t]
        pos = np.searchsorted(docs, docset)
        pos_c = np.minimum(pos, len(docs) - 1)
        hit = docs[pos_c] == docset
        w = (qw * doc_term_weight(freqs[pos_c], nl)).astype(np.float32)
        score = np.where(hit, (score + w).astype(np.float32), score)
    top = np.sort(score)[::-1][:k]
    return top.astype(np.float32)


def queries_for(coll, nq=200, seed=0x51E21):
    return d.synth_queries(seed, coll.p.num_terms, nq)


def mixed_block_type_counts(image, oracle_mod, max_blocks=20000):
    """Full blocks of a block_mixed image by type byte (mixed_block.hpp:38-66: 0 = OptPFor, 1 = VarInt-G8IU,
    2 = interpolative), walked straight off the on-disk layout: 5 B params | u64 size |
    u64 num_docs | bit_vector m_endpoints | u64 bytes | m_lists. Returns {"docs": [..3], "freqs": [..3]}; at most
    `max_blocks` blocks are visited (spread over the lists). The docs part's length -- needed to find the freqs part's
    type byte -- comes from the oracle's block decoder."""
    img = np.frombuffer(image, dtype=np.uint8)
    u64 = lambda off: int(np.frombuffer(img[off:off + 8].tobytes(), dtype=np.uint64)[0])
    size = u64(5)
    words = u64(5 + 8 + 8 + 8)           # after m_endpoints' bit count: its word vector
    lists_at = 5 + 8 + 8 + 8 + 8 + 8 * words
    nbytes = u64(lists_at)
    lists = img[lists_at + 8:lists_at + 8 + nbytes]
    oidx = oracle_mod.Index("block_mixed", image)
    counts = {"docs": [0, 0, 0], "freqs": [0, 0, 0]}
    visited = 0
    # a uniform sample over the BLOCKS of the index (every step-th full block in index order), so that long lists weigh
    # what they weigh in the index
    nfull = [int(oidx.list_size(t)) // 128 for t in range(size)]
    step = max(1, sum(nfull) // max(max_blocks, 1))
    cum = 0
    for t in range(size):
        full = nfull[t]
        first = (-cum) % step
        cum += full
        if first >= full:
            continue
        off = int(oidx.list_offset(t))
        n, vl = oracle_mod.decode_vbyte(lists[off:off + 5].tobytes())
        nb = (n + 127) // 128
        maxs = np.frombuffer(lists[off + vl:off + vl + 4 * nb].tobytes(), dtype=np.uint32)
        eps = np.frombuffer(lists[off + vl + 4 * nb:off + vl + 4 * nb + 4 * (nb - 1)].tobytes(), dtype=np.uint32)
        data = off + vl + 4 * nb + 4 * (nb - 1)
        for b in range(first, full, step):
            start = data + (int(eps[b - 1]) if b else 0)
            base = int(maxs[b - 1]) + 1 if b else 0
            blk = lists[start:start + 2048].tobytes()
            _, consumed = oracle_mod.decode_block("block_mixed", blk, 128, int(maxs[b]) - base - 127)
            counts["docs"][blk[0]] += 1
            counts["freqs"][blk[consumed]] += 1
            visited += 1
    assert visited > 0
    return counts


def topk64(coll, terms, k, conjunctive):
    """float64 top-k BM25 of the AND (conjunctive) / OR result set of `terms`, from the raw lists and document sizes alone --
    nothing of oracle/ and none of the float32 helpers above: k1 = 1.2, b = 0.5, idf floored at 1e-6, a repeated term
    weighted by its query frequency, norm_len = size / average size. Returns (scores descending, float64[min(k, n)], n = the
    size of the result set)."""
    k1, b = 1.2, 0.5
    qtf = {}
    for t in terms:
        qtf[int(t)] = qtf.get(int(t), 0) + 1
    if not qtf:
        return np.zeros(0), 0
    n_docs = coll.num_docs
    sizes = coll.sizes.astype(np.float64)
    norm = sizes / (sizes.sum() / n_docs)
    score = np.zeros(n_docs)
    hits = np.zeros(n_docs, dtype=np.int64)
    for t, f in qtf.items():
        docs, freqs = coll.lists[t]
        docs = docs.astype(np.int64)
        df = float(len(docs))
        # (the one step where float32 and float64 part by more than 1e-5: a list of about half the documents has a ratio near 1,
        # whose float32 rounding alone moves the idf by up to 1e-5 relative -- the ratio is rounded as the scoring rounds it)
        idf = max(1e-6, np.log(float(np.float32((n_docs - df + 0.5) / (df + 0.5)))))
        tf = freqs.astype(np.float64)
        score[docs] += f * idf * (1.0 + k1) * tf / (tf + k1 * (1.0 - b + b * norm[docs]))
        hits[docs] += 1
    member = hits == len(qtf) if conjunctive else hits > 0
    s = np.sort(score[member])[::-1]
    return s[:k], len(s)


def check_pruning_tables(gidx, coll, terms, codec, G=4, hints=True, bitmaps=True, where=""):
    """The upload-time tables of the lists `terms` of the device index gidx (an upload of `coll` as `codec`) against numpy on the raw
    lists: bmw[b] is exactly the largest doc_term_weight of block b; every byte of the level-1 doc-id-range table is 0 iff its range
    holds no posting, else an upper bound (<= 1/255 of the list maximum above) of the largest weight in the range -- its last entry, the
    partial range, included; the list has G entries per posting at least (or one per doc-id); levels 2 and 3 are maxima of 64 entries of
    the level below; a list holding one document in 64 or more carries its exact bitmap (every byte of it, the last, partial one too);
    the hints are 0 for an empty range, 255 for several postings, else 1 + offset % 254. G / hints / bitmaps: what the upload was asked
    for (DS2I_RMW_G, DS2I_NO_RMH, DS2I_NO_BITMAPS)."""
    for t in terms:
        docs, freqs = coll.lists[t]
        w = doc_term_weight(freqs, coll.norm_lens[docs])
        bw = gidx.block_weights(t)
        if codec in d.BLOCK_CODECS:
            nb = (len(docs) + 127) // 128
            assert len(bw) == nb
            exp = np.array([w[b * 128:(b + 1) * 128].max() for b in range(nb)], dtype=np.float32)
            assert np.array_equal(bw, exp), (where, codec, t)
        else:  # chunks of <= 128 postings cut at partition boundaries: the maxima of consecutive runs, in order
            assert len(bw) >= (len(docs) + 127) // 128 and np.float32(bw.max()) == np.float32(w.max()), (where, codec, t)
        tab, sh, mx = gidx.range_table(t)
        assert len(tab) == (coll.num_docs >> sh) + 1 and np.float32(mx) == np.float32(w.max()), (where, codec, t)
        rmax = np.zeros(len(tab), dtype=np.float32)
        np.maximum.at(rmax, docs >> sh, w)
        occupied = np.zeros(len(tab), dtype=bool)
        occupied[docs >> sh] = True
        assert np.array_equal(tab != 0, occupied), (where, codec, t, np.flatnonzero((tab != 0) != occupied)[:4].tolist())
        bound = tab.astype(np.float32) * np.float32(mx / 255.0)
        assert np.all(bound[occupied] * np.float32(1 + 2 ** -17) >= rmax[occupied]), (where, codec, t)
        assert np.all(bound[occupied] <= rmax[occupied] + np.float32(mx) * np.float32(1.01 / 255.0)), (where, codec, t)
        assert G * len(docs) <= len(tab) or sh == 0, (where, codec, t)  # DS2I_RMW_G entries per posting at least (or one per doc-id)
        bm, _, _ = gidx.range_table(t, 0)  # dense lists (>= one document in 64) carry their exact bitmap
        if bitmaps and 64 * len(docs) >= coll.num_docs:
            assert len(bm) == (coll.num_docs + 7) // 8, (where, codec, t)
            bits = np.unpackbits(bm, bitorder="little")
            assert not bits[coll.num_docs:].any(), (where, codec, t)  # (the last byte's spare bits)
            assert np.array_equal(np.flatnonzero(bits[:coll.num_docs]).astype(np.uint32), docs), (where, codec, t)
        else:
            assert len(bm) == 0
        prev = tab
        for level in (2, 3):  # the coarser levels: maxima of 64 entries of the level below
            up, shl, _ = gidx.range_table(t, level)
            assert shl == sh + 6 * (level - 1) and len(up) == (len(prev) + 63) // 64
            padded = np.zeros(len(up) * 64, dtype=np.uint8)
            padded[:len(prev)] = prev
            assert np.array_equal(up, padded.reshape(-1, 64).max(axis=1)), (where, codec, t, level)
            prev = up
        hint, hsh, _ = gidx.range_table(t, 4)  # membership hints: 0 empty, 255 several postings, else 1 + offset % 254
        if hints:  # (every index kind carries them since the ranked / and / wand kernels of all kinds consult them)
            assert hsh == sh and len(hint) == len(tab)
            cnt = np.bincount(docs >> sh, minlength=len(tab))
            exp = np.zeros(len(tab), dtype=np.uint8)
            exp[cnt > 1] = 255
            single = cnt[docs >> sh] == 1
            exp[(docs >> sh)[single]] = (1 + (docs[single] & ((1 << sh) - 1)) % 254).astype(np.uint8)
            assert np.array_equal(hint, exp), (where, codec, t, np.flatnonzero(hint != exp)[:4].tolist())
        else:
            assert len(hint) == 0


# ---------------------------------------------------------------- a crafted collection whose result-set sizes are known exactly
BOUNDARY_SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 3000)


def boundary_collection(num_docs=5000, seed=0xB0DA):
    """Term 0 holds every document (freq 1); term 1 + i the first BOUNDARY_SIZES[i] documents of one fixed order that starts
    with doc 0 and doc num_docs - 1, so these lists are nested: an AND of several is the shortest, an OR the longest, and every
    size of BOUNDARY_SIZES (block edges 127 / 128 / 129 / 256 among them) is the result size of some query. Two strided lists
    have random freqs. The last term is a group of 300 documents of equal size, all with freq 3: its one-term query, and its
    AND with term 0, tie across every k-th place. (No list holds close to half the documents: an idf near 0 is
    ill-conditioned in float32.)"""
    rng = np.random.default_rng(seed)
    n = num_docs
    order = np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)]).astype(np.int64)
    tie = np.sort(rng.choice(n, 300, replace=False))
    sizes = rng.integers(20, 400, n).astype(np.uint32)
    sizes[tie] = 150
    lists = [(np.arange(n), np.ones(n, dtype=np.uint32))]
    for m in BOUNDARY_SIZES:
        lists.append((np.sort(order[:m]), rng.integers(1, 12, m).astype(np.uint32)))
    for stride in (3, 7):
        docs = np.arange(stride // 2, n, stride)
        lists.append((docs, rng.integers(1, 30, len(docs)).astype(np.uint32)))
    lists.append((tie, np.full(len(tie), 3, dtype=np.uint32)))
    return Collection.from_lists(n, lists, sizes)


def boundary_queries(coll):
    """Empty, every term alone, duplicated terms, [all, list of size m] (AND = m, OR = num_docs), neighbouring nested lists (AND =
    the smaller size, OR = the larger: every size is an OR size too), every length 2 .. 16 and two queries of more than 16 terms."""
    T = len(coll.lists)
    pre = list(range(1, 1 + len(BOUNDARY_SIZES)))
    tie = T - 1
    nested = [0] + pre[::-1] + [T - 3]                   # (16 lists: all, 3000, 1025, ..., 1, the stride-3 list)
    qs = [[]] + [[t] for t in range(T)] + [[5, 5], [tie, tie], [0, 0, pre[4]]]
    qs += [[0, t] for t in pre] + [[0, tie], [tie, pre[-1]], [tie, pre[-2], pre[-2]]]
    qs += [[pre[i], pre[i + 1]] for i in range(len(pre) - 1)] + [[pre[0], pre[-1]], [pre[-1], pre[3]]]
    qs += [nested[:L] for L in range(2, 17)]              # AND = the (L-1)-th largest size, OR = num_docs
    qs += [pre[i:i + L] for L in (3, 5, 9, 14) for i in (0, len(pre) - L)]
    qs += [list(range(T)), list(range(T)) + [tie, 2]]     # > 16 terms
    return qs


def edge_queries(num_terms):
    """the edge shapes for a synthetic collection: empty, one term, duplicates, every length 2 .. 16, one beyond 16 terms"""
    T = num_terms
    qs = [[], [5], [T - 1], [5, 5], [7, 3, 7, 3], [0, 0, 1]]
    qs += [[(11 * j + L) % T for j in range(L)] for L in range(2, 17)]
    qs.append(list(range(0, 40, 2)))
    return qs


# ---------------------------------------------------------------- a collection where equal scores are the norm, past doc-id 2^24
TIE_EDGE = 1 << 24            # the first doc-id a float32 (or a 24-bit field) cannot tell from its neighbour
TIE_NUM_DOCS = TIE_EDGE + (1 << 18)
TIE_WINDOW_LO = TIE_EDGE - 64  # the window lists live in [TIE_WINDOW_LO, TIE_NUM_DOCS): a few ids below 2^24, the rest above
TIE_SIZES = (60, 150, 150, 400)
TIE_FREQS = (1, 1, 1, 2, 3)
TIE_HALF = 16                 # lists per half: terms 0 .. 15 spread over the universe, 16 .. 31 in the window, term 32 dense
TIE_CORE = 1500               # documents common to every list of a half (an AND of any of them is not empty)
TIE_STRADDLE = (TIE_EDGE - 2, TIE_EDGE - 1, TIE_EDGE, TIE_EDGE + 1)  # in every window list, same size and freq: a tie across 2^24


def tie_ladder(lo, hi, n=TIE_HALF):
    """n list lengths, geometric from lo to hi"""
    return [int(round(lo * (hi / lo) ** (i / (n - 1)))) for i in range(n)]


def tie_collection(seed=0x71E5):
    """Documents of three distinct sizes and freqs from {1, 2, 3} (skewed to 1): a query sees a few dozen distinct scores, so
    almost every k-th place is tied, across blocks, units and lists. Terms 0 .. 15 are spread over all 2^24 + 2^18 documents,
    a geometric ladder of about 2 k .. 2 M postings (the longest are cut into several units by the default planner); terms
    16 .. 31 (2 k .. 128 k postings) sit in a window that starts 64 documents below 2^24 and ends with the last document, so
    their top-k ids are mostly above 2^24 and reach below it. Each half shares a core of TIE_CORE documents (present in all
    of its lists with one freq per document), which keeps every AND inside a half non-empty and tied at every length; the
    window core holds TIE_STRADDLE, four neighbours around 2^24 of equal size and freq. Term 32 is dense: every document of
    the first, the last and the 2^16 documents around 2^24, so it holds doc 0 and doc num_docs - 1."""
    rng = np.random.default_rng(seed)
    n = TIE_NUM_DOCS
    sizes = rng.choice(np.array(TIE_SIZES, dtype=np.uint32), n)
    sizes[list(TIE_STRADDLE)] = 150
    fr = np.array(TIE_FREQS, dtype=np.uint32)
    lists = []
    for lo, hi, lens in ((0, n, tie_ladder(2000, 2000000)), (TIE_WINDOW_LO, n, tie_ladder(2000, 128000))):
        core = np.unique(rng.integers(lo, hi, TIE_CORE))
        if lo:
            core = np.union1d(core, np.array(TIE_STRADDLE))
        core_freq = rng.choice(fr, len(core))
        if lo:
            core_freq[np.searchsorted(core, np.array(TIE_STRADDLE))] = 3
        for m in lens:
            own = np.setdiff1d(np.unique(rng.integers(lo, hi, max(m - len(core), 1))), core, assume_unique=True)
            docs = np.concatenate([core, own])
            freqs = np.concatenate([core_freq, rng.choice(fr, len(own))])
            o = np.argsort(docs, kind="stable")
            lists.append((docs[o], freqs[o]))
    run = 1 << 15
    dense = np.concatenate([np.arange(0, run), np.arange(TIE_EDGE - run, TIE_EDGE + run), np.arange(n - run, n)])
    lists.append((dense, rng.choice(fr, len(dense))))
    return Collection.from_lists(n, lists, sizes)


def tie_queries(coll, seed=0x71E6):
    """The empty query, one-term queries, duplicated terms, every length 2 .. 16 drawn within each half, random 2 .. 4-term queries
    within each half (more of them in the window, whose ids are the ones past 2^24), queries with the dense list, mixed-half
    queries (for the union operators: an AND across the halves is nearly empty) and, last, two queries of more than 16 terms."""
    assert len(coll.lists) == 2 * TIE_HALF + 1
    rng = np.random.default_rng(seed)
    spread, window, dense = np.arange(TIE_HALF), TIE_HALF + np.arange(TIE_HALF), 2 * TIE_HALF
    pick = lambda pool, m: [int(t) for t in rng.choice(pool, m, replace=False)]
    qs = [[]] + [[t] for t in (0, TIE_HALF - 1, TIE_HALF, 2 * TIE_HALF - 1, dense)]
    qs += [[5, 5], [20, 20, 25], [31, 31, 16], [12, 3, 12, 3]]
    for L in range(2, TIE_HALF + 1):
        qs += [pick(spread, L), pick(window, L)]
    qs += [pick(spread, int(rng.integers(2, 5))) for _ in range(30)]
    qs += [pick(window, int(rng.integers(2, 5))) for _ in range(50)]
    qs += [[dense] + pick(window, m) for m in (1, 2, 3)] + [[dense] + pick(spread[8:], m) for m in (1, 2)]
    qs += [pick(spread, a) + pick(window, b) for a, b in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 4), (4, 4), (2, 6))]
    qs += [[dense] + pick(spread, 2) + pick(window, 2)]
    qs += [[int(t) for t in window] + [dense, 15], [int(t) for t in range(0, 2 * TIE_HALF, 2)] + [17, 21, 25, dense]]
    return qs
