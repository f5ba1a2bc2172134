// host_invert.hpp -- the host's side of indexing documents (no HIP): every check of a forward collection's and of a CSR matrix's
// arguments, and the host twins of the device inversion and transposition. The device entry points (capi_invert.cpp) make the same checks.
//
// A forward collection holds num_docs documents in CSR form: document d is tokens[doc_offsets[d] .. doc_offsets[d + 1]), every token a
// term id < nterms, in any order, with repeats; empty documents are allowed. Its CANONICAL form has every document's tokens sorted and
// equal neighbours turned into one (term, freq) entry: a CSR matrix, documents by terms, with the freqs as values. The inversion is the
// transposition of that matrix: for every term the documents that hold it, strictly increasing, each with the term's count in it. Every
// answer is unique. transpose(transpose(x)) == x.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_parallel.hpp"

namespace ds2i_host {

// a matrix in CSR form: row r is ids / vals [offs[r], offs[r + 1])
struct csr_matrix {
    std::vector<uint64_t> offs;
    std::vector<uint32_t> ids, vals;
};

// "" or what is wrong with the shape of a CSR input whose pointers are not null, in this order: the offsets (not starting at 0, or
// decreasing); 2^32 rows or columns, or more; a row of 2^32 entries or more. `rows` / `cols` / `offsets` name them in the message
// ("documents", "terms", "doc_offsets"). No entry is looked at.
inline std::string csr_shape_fault(const char* who_, uint64_t nrows, uint64_t ncols, const uint64_t* offs, const char* rows, const char* cols,
                                   const char* offsets) {
    const std::string who = std::string(who_) + ": ";
    if (offs[0] != 0) return who + offsets + " must start at 0";
    for (uint64_t r = 0; r < nrows; ++r)
        if (offs[r + 1] < offs[r]) return who + offsets + " decrease";
    if (nrows >= (1ull << 32) || ncols >= (1ull << 32)) return who + "2^32 " + rows + " or " + cols + ", or more";
    for (uint64_t r = 0; r < nrows; ++r)
        if (offs[r + 1] - offs[r] >= (1ull << 32)) return who + "row " + std::to_string(r) + " of the " + rows + " holds 2^32 entries or more";
    return "";
}
inline std::string invert_shape_fault(const char* who, uint64_t num_docs, uint64_t nterms, const uint64_t* doc_offsets) {
    return csr_shape_fault(who, num_docs, nterms, doc_offsets, "documents", "terms", "doc_offsets");
}
inline std::string transpose_shape_fault(const char* who, uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets) {
    return csr_shape_fault(who, nrows, ncols, row_offsets, "rows", "columns", "row_offsets");
}

// fn(first row, end row, chunk) over at most `threads` * 8 contiguous chunks of [0, nrows), on `threads` workers
template <class Fn>
void for_row_chunks(uint64_t nrows, unsigned threads, Fn&& fn) {
    const uint64_t chunks = std::min<uint64_t>(nrows, (uint64_t)(threads ? threads : 1) * 8);
    if (!chunks) return;
    parallel_for(chunks, threads, [&](uint64_t c, unsigned) { fn(nrows / chunks * c + std::min(c, nrows % chunks), nrows / chunks * (c + 1) + std::min(c + 1, nrows % chunks), c); });
}

// the position of the FIRST entry for which bad(row, position) holds, or `none`: the chunks look in parallel, the earliest wins
template <class Bad>
uint64_t first_offender(uint64_t nrows, const uint64_t* offs, unsigned threads, uint64_t none, Bad&& bad) {
    std::vector<uint64_t> found(std::min<uint64_t>(nrows, (uint64_t)(threads ? threads : 1) * 8), none);
    for_row_chunks(nrows, threads, [&](uint64_t r0, uint64_t r1, uint64_t c) {
        for (uint64_t r = r0; r < r1 && found[c] == none; ++r)
            for (uint64_t i = offs[r]; i < offs[r + 1]; ++i)
                if (bad(r, i)) {
                    found[c] = i;
                    break;
                }
    });
    for (uint64_t f : found)
        if (f != none) return f;
    return none;
}

// Throws std::runtime_error naming the first token >= nterms; else nothing.
inline void check_tokens(const char* who, uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms, unsigned threads) {
    const uint64_t none = ~0ull;
    const uint64_t i = first_offender(num_docs, doc_offsets, threads, none, [&](uint64_t, uint64_t k) { return tokens[k] >= nterms; });
    if (i == none) return;
    const uint64_t d = std::upper_bound(doc_offsets, doc_offsets + num_docs + 1, i) - doc_offsets - 1;
    throw std::runtime_error(std::string(who) + ": document " + std::to_string(d) + " holds token " + std::to_string(tokens[i]) + " at position " +
                             std::to_string(i - doc_offsets[d]) + ", outside the " + std::to_string(nterms) + " terms");
}

// Throws std::runtime_error naming the first entry whose column is >= ncols or does not exceed its left neighbour in the row.
inline void check_columns(const char* who, uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets, const uint32_t* cols, unsigned threads) {
    const uint64_t none = ~0ull;
    const uint64_t i = first_offender(nrows, row_offsets, threads, none, [&](uint64_t r, uint64_t k) {
        return cols[k] >= ncols || (k > row_offsets[r] && cols[k - 1] >= cols[k]);
    });
    if (i == none) return;
    const uint64_t r = std::upper_bound(row_offsets, row_offsets + nrows + 1, i) - row_offsets - 1;
    if (cols[i] >= ncols)
        throw std::runtime_error(std::string(who) + ": row " + std::to_string(r) + " holds column " + std::to_string(cols[i]) + " at position " +
                                 std::to_string(i - row_offsets[r]) + ", outside the " + std::to_string(ncols) + " columns");
    throw std::runtime_error(std::string(who) + ": the columns of row " + std::to_string(r) + " do not strictly increase at position " +
                             std::to_string(i - row_offsets[r]));
}

// The canonical form of checked documents (check_tokens): row-parallel, every document sorted in a worker's scratch, its runs counted,
// the counts scanned, the runs written.
inline void canonical_documents(uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, unsigned threads, csr_matrix& out) {
    out.offs.assign(num_docs + 1, 0);
    for_row_chunks(num_docs, threads, [&](uint64_t d0, uint64_t d1, uint64_t) {
        std::vector<uint32_t> s;
        for (uint64_t d = d0; d < d1; ++d) {
            s.assign(tokens + doc_offsets[d], tokens + doc_offsets[d + 1]);
            std::sort(s.begin(), s.end());
            out.offs[d + 1] = std::unique(s.begin(), s.end()) - s.begin();
        }
    });
    for (uint64_t d = 0; d < num_docs; ++d) out.offs[d + 1] += out.offs[d];
    out.ids.resize(out.offs[num_docs]);
    out.vals.resize(out.offs[num_docs]);
    for_row_chunks(num_docs, threads, [&](uint64_t d0, uint64_t d1, uint64_t) {
        std::vector<uint32_t> s;
        for (uint64_t d = d0; d < d1; ++d) {
            s.assign(tokens + doc_offsets[d], tokens + doc_offsets[d + 1]);
            std::sort(s.begin(), s.end());
            uint64_t to = out.offs[d];
            for (size_t i = 0; i < s.size();) {
                size_t j = i;
                while (j < s.size() && s[j] == s[i]) ++j;
                out.ids[to] = s[i];
                out.vals[to++] = (uint32_t)(j - i);
                i = j;
            }
        }
    });
}

// The transpose of a checked matrix (check_columns). The histogram of the columns and its scan are one pass; then every worker owns a
// range of columns and walks all rows in order, storing the entries of its columns: the rows of a column come out increasing.
inline void transpose_csr(uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets, const uint32_t* cols, const uint32_t* vals, unsigned threads,
                          csr_matrix& out) {
    const uint64_t n = row_offsets[nrows];
    out.offs.assign(ncols + 1, 0);
    for (uint64_t i = 0; i < n; ++i) ++out.offs[(uint64_t)cols[i] + 1];
    for (uint64_t c = 0; c < ncols; ++c) out.offs[c + 1] += out.offs[c];
    out.ids.resize(n);
    out.vals.resize(n);
    std::vector<uint64_t> cursor(out.offs.begin(), out.offs.end() - 1);
    if (!threads) threads = 1;
    if (n < (1u << 16)) threads = 1; // (a small matrix is not worth one pass over the rows per worker)
    parallel_for(threads, threads, [&](uint64_t w, unsigned) {
        const uint64_t c0 = ncols / threads * w + std::min<uint64_t>(w, ncols % threads);
        const uint64_t c1 = ncols / threads * (w + 1) + std::min<uint64_t>(w + 1, ncols % threads);
        for (uint64_t r = 0; r < nrows; ++r)
            for (uint64_t i = row_offsets[r]; i < row_offsets[r + 1]; ++i) {
                const uint64_t c = cols[i];
                if (c < c0 || c >= c1) continue;
                const uint64_t to = cursor[c]++;
                out.ids[to] = (uint32_t)r;
                out.vals[to] = vals[i];
            }
    });
}

// The inversion twin: lists for all nterms terms (terms that never occur have empty lists) and every document's token count.
inline void invert_documents(const char* who, uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms, unsigned threads,
                             csr_matrix& lists, std::vector<uint32_t>& doc_sizes) {
    check_tokens(who, num_docs, doc_offsets, tokens, nterms, threads);
    csr_matrix fwd;
    canonical_documents(num_docs, doc_offsets, tokens, threads, fwd);
    transpose_csr(num_docs, nterms, fwd.offs.data(), fwd.ids.data(), fwd.vals.data(), threads, lists);
    doc_sizes.resize(num_docs);
    for (uint64_t d = 0; d < num_docs; ++d) doc_sizes[d] = (uint32_t)(doc_offsets[d + 1] - doc_offsets[d]);
}

// the lists that hold a posting: term_map[list] = old term (strictly increasing), offs = their offsets, from 0
inline void nonempty_lists(uint64_t nterms, const uint64_t* list_offsets, std::vector<uint32_t>& term_map, std::vector<uint64_t>& offs) {
    term_map.clear();
    offs.assign(1, 0);
    for (uint64_t t = 0; t < nterms; ++t)
        if (list_offsets[t + 1] != list_offsets[t]) {
            term_map.push_back((uint32_t)t);
            offs.push_back(list_offsets[t + 1]);
        }
}

} // namespace ds2i_host
