// Host side of indexing documents on the device (include/ds2i_hip.h: ds2i_hip_invert_postings, ds2i_hip_transpose_postings,
// ds2i_hip_invert_documents, ds2i_hip_forward_index): the argument checks, all made on the host (host_invert.hpp) before a device is
// looked for, and the steps over tokens and entries that lie on the device. to_forward: the tokens copied up and staged, sorted within
// their documents by the segmented sort of the remap, and turned into the canonical forward index by the run-length kernels of
// invert_kernels.hip -- mark, count, the scan of the window counts on the host, scatter, offsets. transpose: the histogram of the
// columns, its scan on the host, the scatter through one cursor per column, and the segmented sort once more, over the columns. An
// inversion is the two in a row; the forward index of an image is its extraction, then the transposition.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_util.hpp"
#include "host_invert.hpp"
#include "launchers.hpp"

namespace {

using namespace ds2i_dev;

// {check, document sort, count, scatter + offsets, transpose count + scatter, column sort, extraction, encoder + wand}: hipEvent
// milliseconds of this thread's last inversion, transposition or forward index (ds2i_hip_invert_ms)
thread_local double invert_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};

struct Device {
    const char* who;
    int device, cus = 1;
    Device(const char* who_, int device_) : who(who_), device(device_) {}
    int open() {
        HIP_OK(hipSetDevice(device));
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        if (cus <= 0) cus = 1;
        return DS2I_OK;
    }
    int nomem(const char* what) const {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": " + what + " do not fit on the device").c_str());
    }
};

// two fresh buffers of n words each (one unused word when n == 0: hipMalloc of 0 bytes gives no pointer to free)
bool alloc_pair(DevPostings& p, uint64_t n) {
    return hipMalloc((void**)&p.docs, 4 * std::max<uint64_t>(n, 1)) == hipSuccess && hipMalloc((void**)&p.freqs, 4 * std::max<uint64_t>(n, 1)) == hipSuccess;
}

// Checked documents on the host -> their canonical forward index on the device: fwd = the (term, freq) entries, fwd_offs[d] = the
// entries before document d (num_docs + 1 values). A token >= nterms is DS2I_EFORMAT. Everything else is freed before this returns.
int to_forward(Device& dv, uint64_t num_docs, const uint64_t* doc_offs, const uint32_t* tokens, uint64_t nterms, DevPostings& fwd,
               std::vector<uint64_t>& fwd_offs) {
    const uint64_t n = doc_offs[num_docs];
    fwd_offs.assign(num_docs + 1, 0);
    if (!n) return alloc_pair(fwd, 0) ? DS2I_OK : dv.nomem("the tokens (8 bytes each)");
    const uint64_t windows = (n + INVERT_WINDOW - 1) / INVERT_WINDOW;
    hipStream_t stream = nullptr;
    DevPostings tok; // the tokens as keys and their payloads: gone before this returns
    InvertArgs a{};
    {
        DevTemps dev;
        if (!alloc_pair(tok, n) || dev.alloc(&a.flag, 4) != hipSuccess) return dv.nomem("the tokens (8 bytes each)");
        HIP_OK(hipMemcpy(tok.docs, tokens, 4 * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(a.flag, 0, 4));
        a.keys = tok.docs;
        a.vals = tok.freqs;
        a.n = n;
        a.nterms = nterms;
        const unsigned grid = (unsigned)std::min<uint64_t>((n + SPLIT_THREADS - 1) / SPLIT_THREADS, 8ull * dv.cus);
        HIP_OK(timed_span(stream, invert_ms[0], [&] { return ds2i_launch_invert_stage(a, grid, stream); }));
        uint32_t flag = 0;
        HIP_OK(hipMemcpy(&flag, a.flag, 4, hipMemcpyDeviceToHost));
        if (flag) return ds2i_set_error(DS2I_EFORMAT, (std::string(dv.who) + ": a token lies outside the " + std::to_string(nterms) + " terms").c_str());
    }
    // The segmented sort of the remap, as the merge calls it: the segments are the documents, the keys the tokens, the key bound nterms.
    // Its keys were distinct within a list until now; here they repeat. Nothing in its three classes needs them distinct: classes 1 and
    // 2 compare whole (key, payload) pairs in a bitonic network, equal (term, 1) pairs are interchangeable, and the padding pair is all
    // ones, which no (term < nterms <= 2^32 - 1, 1) equals; class 3 is a stable LSD radix sort over the key bits.
    double ms[4];
    int rc = ds2i_remap_device_postings(dv.who, dv.device, nterms, num_docs, doc_offs, tok, nullptr, ms);
    invert_ms[1] += ms[1] + ms[2] + ms[3];
    if (rc != DS2I_OK) return rc;
    a.keys = tok.docs; // (the sort may have exchanged the pair)
    a.vals = tok.freqs;
    DevTemps dev;
    uint64_t *d_doc_first = nullptr, *d_win_base = nullptr;
    if (dev.alloc(&d_doc_first, 8 * (num_docs + 1)) != hipSuccess || dev.alloc(&a.heads_before, 8 * (num_docs + 1)) != hipSuccess ||
        dev.alloc(&a.win_count, 4 * windows) != hipSuccess || dev.alloc(&d_win_base, 8 * (windows + 1)) != hipSuccess)
        return dv.nomem("the tables of the run-length step (16 bytes per document, 12 per window)");
    HIP_OK(hipMemcpy(d_doc_first, doc_offs, 8 * (num_docs + 1), hipMemcpyHostToDevice));
    a.doc_first = d_doc_first;
    a.ndocs = num_docs;
    a.win_base = d_win_base;
    const unsigned grid_docs = (unsigned)std::min<uint64_t>((num_docs + SPLIT_THREADS - 1) / SPLIT_THREADS, 8ull * dv.cus);
    HIP_OK(timed_span(stream, invert_ms[2], [&] {
        const hipError_t e = ds2i_launch_invert_mark(a, grid_docs, stream);
        return e != hipSuccess ? e : ds2i_launch_invert_count(a, split_grid(windows, dv.cus), stream);
    }));
    std::vector<uint32_t> win_count(windows);
    std::vector<uint64_t> win_base(windows + 1, 0);
    HIP_OK(hipMemcpy(win_count.data(), a.win_count, 4 * windows, hipMemcpyDeviceToHost));
    for (uint64_t w = 0; w < windows; ++w) win_base[w + 1] = win_base[w] + win_count[w]; // (u64: a collection holds more than 2^32 entries)
    HIP_OK(hipMemcpy(d_win_base, win_base.data(), 8 * (windows + 1), hipMemcpyHostToDevice));
    const uint64_t entries = win_base[windows];
    if (!alloc_pair(fwd, entries)) return dv.nomem("the forward entries (8 bytes each) beside the tokens");
    HIP_OK(hipMemset(fwd.freqs, 0, 4 * std::max<uint64_t>(entries, 1))); // (the scatter adds a run's two ends into its word)
    a.dst_terms = fwd.docs;
    a.dst_freqs = fwd.freqs;
    HIP_OK(timed_span(stream, invert_ms[3], [&] {
        const hipError_t e = ds2i_launch_invert_scatter(a, split_grid(windows, dv.cus), stream);
        return e != hipSuccess ? e : ds2i_launch_invert_offsets(a, split_grid(num_docs + 1, dv.cus), stream);
    }));
    HIP_OK(hipMemcpy(fwd_offs.data(), a.heads_before, 8 * (num_docs + 1), hipMemcpyDeviceToHost));
    if (fwd_offs[0] != 0 || fwd_offs[num_docs] != entries)
        return ds2i_set_error(DS2I_EDEVICE, (std::string(dv.who) + ": the offsets kernel and the count kernel disagree").c_str());
    return DS2I_OK;
}

// A matrix whose entries lie on the device in row order (dp.docs = columns, dp.freqs = values; row_offs on the host) -> its transpose:
// dp = (rows, values) column by column, every column in row order; col_offs = ncols + 1 offsets. A column >= ncols or a row that does
// not strictly increase is DS2I_EFORMAT. The input pair is freed as soon as the scatter has read it.
int transpose(Device& dv, uint64_t nrows, uint64_t ncols, const uint64_t* row_offs, DevPostings& dp, std::vector<uint64_t>& col_offs) {
    const uint64_t n = row_offs[nrows];
    col_offs.assign(ncols + 1, 0);
    if (!n) return DS2I_OK;
    const uint64_t windows = (n + INVERT_WINDOW - 1) / INVERT_WINDOW;
    hipStream_t stream = nullptr;
    {
        DevTemps dev;
        DevPostings out;
        TransposeArgs a{};
        uint64_t *d_row_first = nullptr, *d_col_first = nullptr;
        if (dev.alloc(&d_row_first, 8 * (nrows + 1)) != hipSuccess || dev.alloc(&a.count, 4 * ncols) != hipSuccess ||
            dev.alloc(&d_col_first, 8 * (ncols + 1)) != hipSuccess || dev.alloc(&a.flag, 4) != hipSuccess || !alloc_pair(out, n))
            return dv.nomem("the transposed entries (8 bytes each) and the tables (8 bytes per row, 12 per column)");
        HIP_OK(hipMemcpy(d_row_first, row_offs, 8 * (nrows + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(a.count, 0, 4 * std::max<uint64_t>(ncols, 1)));
        HIP_OK(hipMemset(a.flag, 0, 4));
        a.cols = dp.docs;
        a.vals = dp.freqs;
        a.n = n;
        a.row_first = d_row_first;
        a.nrows = (uint32_t)nrows;
        a.ncols = ncols;
        a.col_first = d_col_first;
        a.out_rows = out.docs;
        a.out_vals = out.freqs;
        const unsigned grid = split_grid(windows, dv.cus);
        HIP_OK(timed_span(stream, invert_ms[4], [&] { return ds2i_launch_transpose_count(a, grid, stream); }));
        uint32_t flag = 0;
        HIP_OK(hipMemcpy(&flag, a.flag, 4, hipMemcpyDeviceToHost));
        if (flag)
            return ds2i_set_error(DS2I_EFORMAT, (std::string(dv.who) + ": a column lies outside the " + std::to_string(ncols) +
                                                 " columns, or the columns of a row do not strictly increase").c_str());
        std::vector<uint32_t> count(ncols);
        if (ncols) HIP_OK(hipMemcpy(count.data(), a.count, 4 * ncols, hipMemcpyDeviceToHost));
        for (uint64_t c = 0; c < ncols; ++c) col_offs[c + 1] = col_offs[c] + count[c];
        if (col_offs[ncols] != n) return ds2i_set_error(DS2I_EDEVICE, (std::string(dv.who) + ": the histogram of the columns misses entries").c_str());
        HIP_OK(hipMemcpy(d_col_first, col_offs.data(), 8 * (ncols + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(a.count, 0, 4 * std::max<uint64_t>(ncols, 1))); // the histogram becomes the cursors
        HIP_OK(timed_span(stream, invert_ms[4], [&] { return ds2i_launch_transpose_scatter(a, grid, stream); }));
        std::swap(dp.docs, out.docs); // (`out` frees the input pair here, `dev` the tables, before the sort's second pair arrives)
        std::swap(dp.freqs, out.freqs);
    }
    // every column in row order: the segments are the columns, the keys the row ids (distinct within a column), the key bound nrows
    double ms[4];
    const int rc = ds2i_remap_device_postings(dv.who, dv.device, nrows, ncols, col_offs.data(), dp, nullptr, ms);
    invert_ms[5] += ms[1] + ms[2] + ms[3];
    return rc;
}

int shape_fault(const std::string& fault) { return fault.empty() ? DS2I_OK : ds2i_set_error(DS2I_EINVAL, fault.c_str()); }

// n words of a device buffer as a blob
int download(ds2i_blob& b, const uint32_t* d, uint64_t n) {
    b.data.resize(4 * n);
    if (n) HIP_OK(hipMemcpy(b.data.data(), d, 4 * n, hipMemcpyDeviceToHost));
    return DS2I_OK;
}

double sum_ms() {
    double s = 0.0;
    for (double x : invert_ms) s += x;
    return s;
}

std::vector<uint32_t> sizes_of(uint64_t num_docs, const uint64_t* doc_offs) {
    std::vector<uint32_t> sizes(num_docs);
    for (uint64_t d = 0; d < num_docs; ++d) sizes[d] = (uint32_t)(doc_offs[d + 1] - doc_offs[d]);
    return sizes;
}

} // namespace

extern "C" {

int ds2i_hip_invert_postings(int device, uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms, ds2i_blob** list_offsets,
                             ds2i_blob** docs, ds2i_blob** freqs, ds2i_blob** doc_sizes, double* device_ms) {
    static const char* const who = "ds2i_hip_invert_postings";
    if (!doc_offsets || !tokens || !list_offsets || !docs || !freqs || !doc_sizes) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_invert_postings: null argument");
    DS2I_TRY
    int rc = shape_fault(ds2i_host::invert_shape_fault(who, num_docs, nterms, doc_offsets));
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(invert_ms, invert_ms + 8, 0.0);
    Device dv(who, device);
    rc = dv.open();
    if (rc != DS2I_OK) return rc;
    DevPostings dp;
    std::vector<uint64_t> fwd_offs, list_offs;
    rc = to_forward(dv, num_docs, doc_offsets, tokens, nterms, dp, fwd_offs);
    if (rc != DS2I_OK) return rc;
    rc = transpose(dv, num_docs, nterms, fwd_offs.data(), dp, list_offs);
    if (rc != DS2I_OK) return rc;
    std::unique_ptr<ds2i_blob> bo(ds2i_blob_of(list_offs)), bd(new ds2i_blob), bf(new ds2i_blob), bs(ds2i_blob_of(sizes_of(num_docs, doc_offsets)));
    rc = download(*bd, dp.docs, list_offs[nterms]);
    if (rc == DS2I_OK) rc = download(*bf, dp.freqs, list_offs[nterms]);
    if (rc != DS2I_OK) return rc;
    *list_offsets = bo.release();
    *docs = bd.release();
    *freqs = bf.release();
    *doc_sizes = bs.release();
    if (device_ms) *device_ms = sum_ms(); // (like every output, written only when the call succeeds)
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_transpose_postings(int device, uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets, const uint32_t* cols, const uint32_t* vals,
                                ds2i_blob** col_offsets, ds2i_blob** rows, ds2i_blob** out_vals, double* device_ms) {
    static const char* const who = "ds2i_hip_transpose_postings";
    if (!row_offsets || !cols || !vals || !col_offsets || !rows || !out_vals) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_transpose_postings: null argument");
    DS2I_TRY
    int rc = shape_fault(ds2i_host::transpose_shape_fault(who, nrows, ncols, row_offsets));
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(invert_ms, invert_ms + 8, 0.0);
    Device dv(who, device);
    rc = dv.open();
    if (rc != DS2I_OK) return rc;
    const uint64_t n = row_offsets[nrows];
    DevPostings dp;
    if (!alloc_pair(dp, n)) return dv.nomem("the entries (8 bytes each)");
    if (n) {
        HIP_OK(hipMemcpy(dp.docs, cols, 4 * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dp.freqs, vals, 4 * n, hipMemcpyHostToDevice));
    }
    std::vector<uint64_t> col_offs;
    rc = transpose(dv, nrows, ncols, row_offsets, dp, col_offs);
    if (rc != DS2I_OK) return rc;
    std::unique_ptr<ds2i_blob> bo(ds2i_blob_of(col_offs)), br(new ds2i_blob), bv(new ds2i_blob);
    rc = download(*br, dp.docs, n);
    if (rc == DS2I_OK) rc = download(*bv, dp.freqs, n);
    if (rc != DS2I_OK) return rc;
    *col_offsets = bo.release();
    *rows = br.release();
    *out_vals = bv.release();
    if (device_ms) *device_ms = sum_ms(); // (like every output, written only when the call succeeds)
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_invert_documents(int device, int index_kind, uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms,
                              ds2i_blob** index_image, ds2i_blob** wand_image, ds2i_blob** term_map, ds2i_blob** doc_sizes, double* device_ms) {
    static const char* const who = "ds2i_hip_invert_documents";
    int rc = ds2i_check_encoder_kind(who, index_kind); // (before anything else is read)
    if (rc != DS2I_OK) return rc;
    if (!doc_offsets || !tokens || !index_image || !term_map || !doc_sizes) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_invert_documents: null argument");
    DS2I_TRY
    rc = shape_fault(ds2i_host::invert_shape_fault(who, num_docs, nterms, doc_offsets));
    if (rc != DS2I_OK) return rc;
    if (!doc_offsets[num_docs]) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_invert_documents: the documents hold no token: List must be nonempty");
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(invert_ms, invert_ms + 8, 0.0);
    Device dv(who, device);
    rc = dv.open();
    if (rc != DS2I_OK) return rc;
    DevPostings dp;
    std::vector<uint64_t> fwd_offs, all_offs, offs;
    rc = to_forward(dv, num_docs, doc_offsets, tokens, nterms, dp, fwd_offs);
    if (rc != DS2I_OK) return rc;
    rc = transpose(dv, num_docs, nterms, fwd_offs.data(), dp, all_offs);
    if (rc != DS2I_OK) return rc;
    std::vector<uint64_t>().swap(fwd_offs);
    // terms that never occur vanish: the postings stay where they lie, only the offsets lose their repeats
    std::vector<uint32_t> terms;
    ds2i_host::nonempty_lists(nterms, all_offs.data(), terms, offs);
    std::vector<uint64_t>().swap(all_offs);
    const std::vector<uint32_t> sizes = sizes_of(num_docs, doc_offsets);
    uint32_t *d_docs = dp.docs, *d_freqs = dp.freqs;
    dp.release(); // (the encoder's staging owns them from here on)
    ds2i_blob *img = nullptr, *wand = nullptr;
    rc = ds2i_build_device_postings(who, device, index_kind, num_docs, terms.size(), offs.data(), d_docs, d_freqs, sizes.data(), &img,
                                    wand_image ? &wand : nullptr, &invert_ms[7]);
    if (rc != DS2I_OK) return rc;
    std::unique_ptr<ds2i_blob> bi(img), bw(wand), bt(ds2i_blob_of(terms)), bs(ds2i_blob_of(sizes));
    *index_image = bi.release();
    if (wand_image) *wand_image = bw.release();
    *term_map = bt.release();
    *doc_sizes = bs.release();
    if (device_ms) *device_ms = sum_ms(); // (like every output, written only when the call succeeds)
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_forward_index(int device, int index_kind, const void* image, size_t bytes, uint64_t* num_docs, uint64_t* nterms, ds2i_blob** doc_offsets,
                           ds2i_blob** terms, ds2i_blob** freqs, double* device_ms) {
    static const char* const who = "ds2i_hip_forward_index";
    if (!image || !num_docs || !nterms || !doc_offsets || !terms || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_forward_index: null argument");
    if (index_kind < DS2I_BLOCK_OPTPFOR || index_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_forward_index: unknown index kind");
    DS2I_TRY
    uint64_t ndocs = 0, nlists = 0;
    std::vector<uint32_t> lengths;
    int rc = ds2i_parse_image(index_kind, image, bytes, ndocs, nlists, &lengths);
    if (rc != DS2I_OK) return rc;
    if (ndocs >= (1ull << 32) || nlists >= (1ull << 32)) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_forward_index: 2^32 documents or terms, or more");
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(invert_ms, invert_ms + 8, 0.0);
    std::vector<uint64_t> offs(nlists + 1, 0);
    for (uint64_t t = 0; t < nlists; ++t) offs[t + 1] = offs[t] + lengths[t];
    std::vector<uint32_t>().swap(lengths);
    DevPostings dp;
    {
        ds2i_hip_index* raw = nullptr;
        rc = ds2i_index_open_bare(device, index_kind, image, bytes, &raw);
        if (rc != DS2I_OK) return rc;
        IndexHandle idx(raw);
        rc = ds2i_extract_to_device(idx.get(), 0, nlists, offs.data(), dp, invert_ms[6]);
        if (rc != DS2I_OK) return rc;
    } // (the image leaves the device before the transposed entries arrive)
    Device dv(who, device);
    rc = dv.open();
    if (rc != DS2I_OK) return rc;
    std::vector<uint64_t> doc_offs;
    rc = transpose(dv, nlists, ndocs, offs.data(), dp, doc_offs);
    if (rc != DS2I_OK) return rc;
    std::unique_ptr<ds2i_blob> bo(ds2i_blob_of(doc_offs)), bt(new ds2i_blob), bf(new ds2i_blob);
    rc = download(*bt, dp.docs, doc_offs[ndocs]);
    if (rc == DS2I_OK) rc = download(*bf, dp.freqs, doc_offs[ndocs]);
    if (rc != DS2I_OK) return rc;
    *num_docs = ndocs;
    *nterms = nlists;
    *doc_offsets = bo.release();
    *terms = bt.release();
    *freqs = bf.release();
    if (device_ms) *device_ms = sum_ms(); // (like every output, written only when the call succeeds)
    return DS2I_OK;
    DS2I_CATCH
}

void ds2i_hip_invert_ms(double ms[8]) {
    if (ms) std::memcpy(ms, invert_ms, sizeof invert_ms);
}

} // extern "C"
