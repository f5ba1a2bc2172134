"""One crafted collection that puts a candidate on every edge of the upload-time membership structures (abi_structs.hpp:
BatchArgs::rmw / rmh, RmwLevels), its queries, and a census that counts, from the raw lists alone, how many candidates fall on each edge.

The structures: a list's doc-id-range table has one weight byte per range of 1 << shift doc-ids (0 iff the range is empty), a parallel
hint byte (0 empty, 255 several postings, else rmh_code = 1 + offset % 254 of the ONE posting) and, for a list holding one document in
64 or more, an exact bitmap. rmh_code is injective only over ranges of at most 254 doc-ids (shift <= 7): at shift 8 the offsets {0, 254}
and {1, 255} share a code, from shift 9 on every offset has an alias 254 away. k_ranked_stream<AND> and k_union_stream take a matching
code for proof up to shift 7 and for a filter beyond; a random collection puts a candidate on the alias of a lone posting about once in
30 000 candidates, this one does so hundreds of times.

NUM_DOCS = 2^20 + 37 is a multiple of neither 64 nor any range width: every list's last range and the last bitmap word are partial. The
documents are seen as 1024 windows of 1024 doc-ids and the 37 documents of the last, partial window. The lists (terms):

  A, B, C   sparse anchors of 800 / 1 500 / 3 000 postings: shift 8 / 7 / 6 at G = DS2I_RMW_G = 4, 9 / 8 / 7 at G = 2, 10 / 9 / 8 at G = 1.
            Per anchor the windows are of four kinds: ONE posting at window offset 0 or 1 (the lone posting of its range at every shift
            <= 10, and its code is one of the two aliased ones at shift 8); one posting at another offset (253, 254, 255 modulo every
            range width among them); several postings; empty. Window 0 is of the first kind (a posting in the first range), the last
            window holds NUM_DOCS - 1 alone. Every posting has freq 1 but one: freq 60 in a document of size 1, the list's maximum.
            C also holds 300 documents of 65 000 words (freq 1: a weight below 1/255 of the list maximum) in windows that hold nothing else.
  PA, PB, PC  their probes, shorter than the anchor (they drive the conjunction), built relative to it: for the lone postings the same
            document | the documents 254, 508 and 762 above it (same code at shift >= 8 / 9 / 10, other document) | a document 100 above it
            (another code, same range from shift 7 on) | nothing; documents in empty windows; a member and a non-member of every window
            with several postings; NUM_DOCS - 1 and seven more documents of the last window; C's heavy documents. The alias documents
            carry the probe's largest weights (freq 2, the smallest sizes) and every document the pair shares is large, so that the
            top 10 of the two-list union are alias documents: one dropped changes the answer. The anchor's maximum score exceeds the
            probe's, so in the union kernels the anchor is the exclusion list whose hints are read.
  D, PD     a dense anchor of about 20 000 postings (bitmap; shift 3 / 4 / 5: bitmap_first holds at G = 4 only) that holds documents 0, 7, 8,
            63, 64 and NUM_DOCS - 1 but not their neighbours, and the same pattern in 150 more 64-document words; PD holds both.
  E, PE     one doc-id per entry at G = 4 (140 000 postings, shift 0 / 1 / 2): without hints its weight byte alone is the answer. PE holds
            members and their right neighbours.
  F0 .. F5  fillers of 2 000 .. 100 000 random postings for the 3-, 4-, 5-, 8- and 16-list queries.
Every list holds the 80 core documents (in windows where every anchor has several postings), so every conjunction is non-empty. No list
comes near half the documents."""
import numpy as np

from helpers import Collection, doc_term_weight, query_term_weight

NUM_DOCS = (1 << 20) + 37
WIN = 1024
NWIN = 1 << 10               # full windows; [LAST_LO, NUM_DOCS) is the partial last one
LAST_LO = NWIN * WIN
GS = (4, 2, 1)
A, B, C, PA, PB, PC, D, PD, E, PE = range(10)
FILLERS = tuple(range(10, 16))
NAMES = ("A", "B", "C", "PA", "PB", "PC", "D", "PD", "E", "PE", "F0", "F1", "F2", "F3", "F4", "F5")
SPARSE = ((A, PA, 800), (B, PB, 1500), (C, PC, 3000))
ANCHORS = (A, B, C, D, E)
PROBE_OF = {A: PA, B: PB, C: PC, D: PD, E: PE}
HEAVY_ANCHOR = C
ALIAS_STEPS = (254, 508, 762)
OTHER_OFFSETS = (253, 254, 255, 509, 510, 511, 765, 766, 767, 1021, 1022, 1023, 2, 100, 127, 128, 300, 512, 513, 640, 1000)
DENSE_IN, DENSE_OUT = (0, 7, 8, 63, 64), (1, 6, 9, 62, 65)  # offsets from the start of a 64-document word: byte and word edges
LAST_PROBED = (0, 5, 17, 32, 33, 34, 35, 36)                # offsets into the last window that every probe holds (36 = NUM_DOCS - 1)
CATEGORIES = ("empty range", "lone + same document", "lone + other code", "lone + same code, other document", "several + member",
              "several + non-member", "bitmap member at a byte or word edge", "bitmap non-member at a byte or word edge", "last range",
              "tiny-weight-only range")
ALIAS = CATEGORIES[3]


def expected_shift(n, G, num_docs=NUM_DOCS):
    """the shift of a list of n postings (capi.cpp): the largest s with (num_docs >> s) >= G * n, else 0"""
    s = 0
    for c in range(1, 32):
        if (num_docs >> c) >= G * n:
            s = c
    return s


def has_bitmap(n, num_docs=NUM_DOCS):
    return 64 * n >= num_docs


def rmh_code(doc, shift):
    return 1 + (np.asarray(doc, dtype=np.int64) & ((1 << shift) - 1)) % 254


def _sparse_pair(rng, target, core_windows, core_docs, heavy):
    """one sparse anchor and its probe -> (anchor docs, anchor freqs, probe docs, probe freqs, marks); marks: document sets by role"""
    free = np.setdiff1d(np.arange(1, NWIN), core_windows)
    free = free[rng.permutation(len(free))]
    n_lone = 400 if target < 1000 else 300
    n_other, n_tiny_lone, n_tiny_multi = 100, (60 if heavy else 0), (80 if heavy else 0)
    n_multi = {800: 60, 1500: 110, 3000: 150}[target]
    cut = np.cumsum([n_lone - 1, n_other, n_tiny_lone, n_tiny_multi, n_multi, 60])
    w_lone, w_other, w_tl, w_tm, w_multi, w_empty = np.split(free[:cut[-1]], cut[:-1])
    w_lone = np.concatenate([[0], w_lone])  # window 0: a posting in the first range
    lone = w_lone * WIN + rng.integers(0, 2, len(w_lone))
    other = w_other * WIN + np.array([OTHER_OFFSETS[i % len(OTHER_OFFSETS)] for i in range(len(w_other))])
    heavy_docs = np.concatenate([w_tl * WIN + rng.integers(2, WIN, len(w_tl))] +
                                [w * WIN + rng.choice(WIN, 3, replace=False) for w in w_tm]).astype(np.int64)
    fixed = len(lone) + len(other) + len(heavy_docs) + 1 + 1  # (+ NUM_DOCS - 1, + the maximum's document)
    multi_windows = np.concatenate([core_windows, w_multi])
    per = np.full(len(multi_windows), (target - fixed - len(core_docs)) // len(multi_windows))
    per[:(target - fixed - len(core_docs)) - per.sum()] += 1
    assert per.min() >= 2
    multi, members, non_members, top_doc = [], [], [], None
    for i, w in enumerate(multi_windows):
        taken = core_docs[(core_docs >= w * WIN) & (core_docs < (w + 1) * WIN)] - w * WIN
        if i < len(core_windows):
            multi.append(w * WIN + rng.choice(np.setdiff1d(np.arange(WIN), taken), per[i], replace=False))
            continue
        # base and base + 2 (base a multiple of 4) are postings, base + 1 is not: one range with them from shift 2 on; the probe holds
        # base (a member of a range with several postings) and base + 1 (a non-member of it)
        base = 4 * int(rng.integers(0, WIN // 4))
        offs = rng.choice(np.setdiff1d(np.arange(WIN), np.arange(base, base + 4)), per[i] - 1, replace=False)
        multi.append(w * WIN + np.concatenate([[base, base + 2], offs[:per[i] - 2]]))
        members.append(w * WIN + base)
        non_members.append(w * WIN + base + 1)
        if top_doc is None:
            top_doc = int(w * WIN + offs[-1])  # the list's maximum: freq 60 in a document of size 1, not in the probe
    a_docs = np.concatenate([lone, other, heavy_docs, core_docs, np.concatenate(multi), [top_doc, NUM_DOCS - 1]]).astype(np.int64)
    assert len(np.unique(a_docs)) == len(a_docs) == target
    o = np.argsort(a_docs)
    a_docs, a_freqs = a_docs[o], np.ones(target, dtype=np.uint32)
    a_freqs[np.searchsorted(a_docs, top_doc)] = 60
    # the probe, relative to the anchor
    nm, na, no = (60, 90, 60) if target < 1000 else (50, 80, 50)
    order = rng.permutation(len(lone) - 1) + 1  # (window 0's lone posting: a member, below)
    same = np.concatenate([lone[:1], lone[order[:nm]]])
    aliased = lone[order[nm:nm + na]]
    alias = {step: aliased + step for step in ALIAS_STEPS}
    other_code = lone[order[nm + na:nm + na + no]] + 100
    po = rng.permutation(len(other))
    other_same = other[po[:30]]
    other_moved = other[po[30:60]] // WIN * WIN + (other[po[30:60]] % WIN + 77) % WIN
    in_empty = w_empty * WIN + rng.integers(0, WIN, len(w_empty))
    last = LAST_LO + np.array(LAST_PROBED)
    parts = [same] + list(alias.values()) + [other_code, other_same, other_moved, in_empty, np.array(members), np.array(non_members), core_docs,
                                             last, heavy_docs]
    p_docs = np.unique(np.concatenate(parts)).astype(np.int64)
    assert len(p_docs) == sum(len(x) for x in parts) < target
    p_freqs = np.ones(len(p_docs), dtype=np.uint32)
    for step in ALIAS_STEPS:
        p_freqs[np.searchsorted(p_docs, alias[step])] = 2
    return a_docs, a_freqs, p_docs, p_freqs, {"alias": alias, "shared": np.intersect1d(a_docs, p_docs), "heavy": heavy_docs, "top": top_doc}


def _with_core(rng, docs, core_docs, hi=9):
    docs = np.union1d(docs, core_docs).astype(np.int64)
    return docs, rng.integers(1, hi, len(docs)).astype(np.uint32)


_COLL = None


def collection():
    """the collection (built once per process: about a second)"""
    global _COLL
    if _COLL is not None:
        return _COLL
    rng = np.random.default_rng(0x7AB1E)
    core_windows = np.sort(rng.choice(np.arange(1, NWIN), 40, replace=False))
    core_docs = np.sort(np.concatenate([w * WIN + rng.choice(WIN, 2, replace=False) for w in core_windows])).astype(np.int64)
    lists, marks = [None] * 16, {}
    sizes = rng.integers(70, 111, NUM_DOCS).astype(np.uint32)
    for anchor, probe, target in SPARSE:
        ad, af, pd, pf, m = _sparse_pair(rng, target, core_windows, core_docs, anchor == HEAVY_ANCHOR)
        lists[anchor], lists[probe], marks[anchor] = (ad, af), (pd, pf), m
    # the dense anchor: random documents, then the edge pattern in word 0 and 150 more words; PD holds the pattern's members and neighbours
    words = np.concatenate([[0], np.sort(rng.choice(np.arange(1, NUM_DOCS // 64 - 1), 150, replace=False))])
    inn = (words[:, None] * 64 + np.array(DENSE_IN)[None, :]).ravel()
    out = (words[:, None] * 64 + np.array(DENSE_OUT)[None, :]).ravel()
    dd = np.setdiff1d(np.union1d(rng.choice(NUM_DOCS, 20000, replace=False), np.concatenate([inn, [LAST_LO + 32, NUM_DOCS - 1]])),
                      np.concatenate([out, [NUM_DOCS - 2]]))
    lists[D] = _with_core(rng, dd, core_docs)
    extra = rng.choice(NUM_DOCS, 400, replace=False)
    pdd = np.unique(np.concatenate([inn, out, extra, lists[D][0][rng.choice(len(lists[D][0]), 400, replace=False)], LAST_LO + np.array(LAST_PROBED)]))
    lists[PD] = _with_core(rng, pdd, core_docs, 4)
    # one doc-id per entry at G = 4
    ed = np.union1d(rng.choice(NUM_DOCS, 140000, replace=False), [NUM_DOCS - 1])
    lists[E] = _with_core(rng, ed, core_docs)
    em = lists[E][0][rng.choice(len(lists[E][0]), 1000, replace=False)]
    ped = np.unique(np.concatenate([em, np.minimum(em + 1, NUM_DOCS - 1), LAST_LO + np.array(LAST_PROBED)]))
    lists[PE] = _with_core(rng, ped, core_docs, 4)
    for t, n in zip(FILLERS, (2000, 5000, 12000, 30000, 60000, 100000)):
        lists[t] = _with_core(rng, rng.choice(NUM_DOCS, n, replace=False), core_docs)
    # sizes: the alias documents the smallest (254 above the lone posting smallest of all), then whatever an anchor and its probe share
    # large, the heavy documents, the maxima's documents
    for anchor, _, _ in SPARSE:
        for step, (lo, hi) in zip(ALIAS_STEPS, ((30, 41), (44, 53), (56, 65))):
            docs = marks[anchor]["alias"][step]
            sizes[docs] = rng.integers(lo, hi, len(docs))
    for anchor, _, _ in SPARSE:
        sizes[marks[anchor]["shared"]] = 400
    sizes[marks[HEAVY_ANCHOR]["heavy"]] = 65000
    for anchor, _, _ in SPARSE:
        sizes[marks[anchor]["top"]] = 1
    _COLL = Collection.from_lists(NUM_DOCS, lists, sizes)
    _COLL.marks = marks
    return _COLL


def queries():
    """every list alone; every probe with its anchor, then with two, three, four and all five anchors; anchor pairs; probes with foreign
    anchors; filler queries of 3, 4, 5, 8 and 16 lists; duplicated terms; last, one query of more than 16 terms"""
    qs = [[t] for t in range(16)]
    qs += [[PROBE_OF[a], a] for a in ANCHORS]
    for i, a in enumerate(ANCHORS):
        ring = [ANCHORS[(i + j) % 5] for j in range(5)]
        qs += [[PROBE_OF[a]] + ring[:m] for m in (2, 3, 4, 5)]
    qs += [[ANCHORS[i], ANCHORS[j]] for i in range(5) for j in range(i + 1, 5)]
    qs += [[PA, B], [PA, C], [PB, A], [PB, C], [PC, A], [PC, B], [PD, A], [PE, B], [PA, D], [PB, E], [PC, D], [PA, PB, C], [PC, PB, A, D]]
    qs += [[PA, A, 10], [PB, B, 11], [PC, C, 12], [PD, D, 13], [PE, E, 14], [PA, A, B, 10, 11], [PB, B, C, 12, 13, 14], [PC, C, D, E, 15],
           [A, B, C, 10], [A, B, C, D, E, 10, 11, 12], [PA, PB, PC, A, B, C, 10, 11], [PD, PE, A, B, C, D, E, 15], list(range(16)),
           [t for t in range(16) if t != E], [PC, C, 10, 11, 12, 13], [PD, D, A, 10, 15], [PE, E, C, B, 13, 14, 15]]
    qs += [[PA, A, PA], [A, A], [PD, D, D], [PB, B, C, B], [E, PE, PE, E]]
    qs.append(list(range(16)) + [A, PA, D])
    return qs


def pairs(qs):
    """the (driving list, probed list) pairs the queries form: a conjunction is driven by its shortest list and probes every other one (in
    a two-list union of a probe and its anchor the probe drives as well: the anchor has the higher maximum score)"""
    coll, out = collection(), set()
    for q in qs:
        ts = sorted(set(q), key=lambda t: (len(coll.lists[t][0]), t))
        out |= {(ts[0], t) for t in ts[1:]}
    return sorted(out)


def categories(coll, driver, probed, G, docs=None):
    """{category: boolean mask} over the candidates (the driving list's documents, or `docs`) against the probed list's structures at G"""
    c = (coll.lists[driver][0] if docs is None else np.asarray(docs)).astype(np.int64)
    pd, pf = coll.lists[probed]
    pd = pd.astype(np.int64)
    s = expected_shift(len(pd), G, coll.num_docs)
    nr = (coll.num_docs >> s) + 1
    cnt = np.bincount(pd >> s, minlength=nr)
    code = np.zeros(nr, dtype=np.int64)
    single = cnt[pd >> s] == 1
    code[(pd >> s)[single]] = rmh_code(pd[single], s)
    w = doc_term_weight(pf, coll.norm_lens[pd])
    rmax = np.zeros(nr, dtype=np.float32)
    np.maximum.at(rmax, pd >> s, w)
    r, member, k = c >> s, np.isin(c, pd), cnt[c >> s]
    same_code = rmh_code(c, s) == code[r]
    edge = np.isin(c & 7, (0, 7)) | np.isin(c & 63, (0, 63))
    bm = has_bitmap(len(pd), coll.num_docs)
    m = [k == 0, (k == 1) & member, (k == 1) & ~member & ~same_code, (k == 1) & ~member & same_code, (k > 1) & member, (k > 1) & ~member,
         edge & member & bm, edge & ~member & bm, r == (coll.num_docs >> s), (k > 0) & (rmax[r] < w.max() / np.float32(255.0))]
    return dict(zip(CATEGORIES, m))


def category_of(coll, driver, probed, G, doc):
    return " | ".join(name for name, m in categories(coll, driver, probed, G, [doc]).items() if m[0]) + \
        " (list %s, shift %d)" % (NAMES[probed], expected_shift(len(coll.lists[probed][0]), G, coll.num_docs))


def census(G, qs=None):
    """{(driving list, probed list): {category: candidates}} at G entries per posting"""
    coll = collection()
    return {(a, b): {name: int(m.sum()) for name, m in categories(coll, a, b, G).items()} for a, b in pairs(queries() if qs is None else qs)}


def possible(category, anchor, G):
    """can a candidate of this category exist for this anchor at its shift? (a range of one doc-id holds neither several postings nor a
    non-member; an alias needs a range wider than 254; the last range of E is at most one document wide)"""
    coll = collection()
    n = len(coll.lists[anchor][0])
    s = expected_shift(n, G)
    i = CATEGORIES.index(category)
    return [True, True, s >= 1, s >= 8, s >= 1, s >= 2, has_bitmap(n), has_bitmap(n), NUM_DOCS - (NUM_DOCS >> s << s) >= 5 and anchor != E,
            anchor == HEAVY_ANCHOR][i]


def census_table():
    """category x G -> candidates summed over every pair (CHANGELOG.md holds its print-out)"""
    return {name: [sum(cell[name] for cell in census(G).values()) for G in GS] for name in CATEGORIES}


def max_score(coll, t):
    dd, ff = coll.lists[t]
    return float(query_term_weight(1, len(dd), coll.num_docs)) * float(doc_term_weight(ff, coll.norm_lens[dd]).max())


_REF = None


def reference():
    """numpy's answers to queries(), computed once: per query the AND doc-id list, the OR count, the and_freq / or_freq sums (every
    distinct term's freq of every document of the result) and the float64 top 65 of the AND / top 64 of the OR (helpers.topk64)"""
    global _REF
    if _REF is None:
        from helpers import brute_and, brute_or, topk64
        coll, _REF = collection(), []
        for q in queries():
            both = brute_and(coll, q)
            ts = sorted(set(q))
            _REF.append({"and": both, "or": len(brute_or(coll, q)),
                         "and_freq": sum(int(coll.lists[t][1][np.searchsorted(coll.lists[t][0], both)].sum()) for t in ts) if len(both) else 0,
                         "or_freq": sum(int(coll.lists[t][1].sum(dtype=np.uint64)) for t in ts),
                         "top_and": topk64(coll, q, 65, True)[0], "top_or": topk64(coll, q, 64, False)[0]})
    return _REF


if __name__ == "__main__":
    print("%-42s %s" % ("category", "  ".join("G = %d" % G for G in GS)))
    for name, row in census_table().items():
        print("%-42s %s" % (name, "  ".join("%6d" % v for v in row)))
