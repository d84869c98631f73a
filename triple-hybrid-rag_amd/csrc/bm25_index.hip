// BM25 index set-up: the pruning bounds and quantised impacts of the postings (thr_bm25_bounds) and
// the per-doc rows of the dense terms (thr_bm25_dense_rows).
#include "bm25_common.hpp"

namespace thr {

// Upper bounds for WAND-style pruning, computed once at index set-up (thr_bm25_bounds) with the
// scoring formula itself: term_ub[t] = max over the postings of term t of bm25_contrib, and
// block_ub[j] = the same maximum over postings [128 j, 128 j + 128) of the posting array (a block
// that straddles two short lists bounds both).  Kept as order-preserving uint64 keys while the
// atomicMax passes run, decoded in place by bm25_bounds_decode.
__global__ __launch_bounds__(256) void bm25_bounds_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ post_doc,
    const int32_t* __restrict__ post_tf, const float* __restrict__ doclen,
    const double* __restrict__ idf, double avgdl, double k1, double b, int64_t n_vocab, int64_t nnz,
    unsigned long long* __restrict__ term_key, unsigned long long* __restrict__ block_key,
    uint8_t* __restrict__ post_imp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnz) return;
    int64_t lo = 0, hi = n_vocab;  // last term with rowptr[t] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= i) lo = mid; else hi = mid;
    }
    const double tfv = (double)post_tf[i], dlv = (double)doclen[post_doc[i]];
    const double c = bm25_contrib(idf[lo], tfv, dlv, avgdl, k1, b);
    if (post_imp) {
        // the posting's IMPACT tf (k1+1) / (tf + nrm) -- its contribution is idf * impact, and the
        // impact does not depend on the query -- rounded UP to 8 bits of (k1 + 1) / 255 (one more
        // step than the ceiling, so no rounding of this arithmetic can leave it below the impact)
        const double nrm = __dmul_rn(k1, __dadd_rn(__dsub_rn(1.0, b), __dmul_rn(b, __ddiv_rn(dlv, avgdl))));
        const double imp = __ddiv_rn(__dmul_rn(tfv, __dadd_rn(k1, 1.0)), __dadd_rn(tfv, nrm));
        const int qv = (int)ceil(imp * (255.0 / (k1 + 1.0))) + 1;
        post_imp[i] = (uint8_t)(qv > 255 ? 255 : qv < 0 ? 0 : qv);
    }
    const unsigned long long key = dkey(c);
    atomicMax(&term_key[lo], key);
    atomicMax(&block_key[i / BM_BLOCK], key);
}
__global__ void bm25_bounds_decode(unsigned long long* __restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        // an untouched slot (term without postings) bounds nothing: 0
        const double v = keys[i] ? dkey_inv(keys[i]) : 0.0;
        reinterpret_cast<double*>(keys)[i] = v;
    }
}

// DENSE TERMS (stop words: a term held by at least an eighth of the docs, chosen by the caller at
// index set-up).  Besides its CSR postings such a term gets one byte and one 16-bit word PER DOC:
// its quantised impact (post_imp of the doc's posting, 0 where the doc does not hold the term)
// and its term frequency (0 likewise).  bm25_window_kernel then needs no posting of the term at
// all: the bound of doc d is a coalesced byte load at [row + d], the exact contribution comes
// from the frequency at [row + d] -- no staging, no LDS atomics, no position search.
__global__ __launch_bounds__(256) void bm25_dense_rows_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ post_doc,
    const int32_t* __restrict__ post_tf, const uint8_t* __restrict__ post_imp,
    const int32_t* __restrict__ terms, int64_t stride, uint8_t* __restrict__ dense_imp,
    uint16_t* __restrict__ dense_tf) {
    const int row = blockIdx.y;
    const int term = terms[row];
    const int64_t lo = rowptr[term], hi = rowptr[term + 1];
    for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t at = (int64_t)row * stride + post_doc[i];
        const int32_t tf = post_tf[i];
        dense_imp[at] = post_imp[i];
        dense_tf[at] = (uint16_t)(tf > 65535 ? 65535 : tf);   // (the caller keeps terms with tf > 65535 out)
    }
}

}  // namespace thr

using namespace thr;

extern "C" size_t thr_bm25_block_count(int64_t nnz) { return nnz > 0 ? (size_t)((nnz + BM_BLOCK - 1) / BM_BLOCK) : 0; }

extern "C" int thr_bm25_bounds(const int64_t* rowptr, const int32_t* post_doc, const int32_t* post_tf,
                               const float* doclen, const double* idf, double avgdl, double k1,
                               double b, int64_t n_vocab, int64_t nnz, double* term_ub,
                               double* block_ub, uint8_t* post_imp, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!rowptr || !post_doc || !post_tf || !doclen || !idf || !term_ub || !block_ub,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_vocab <= 0 || nnz <= 0 || !(avgdl > 0.0), THR_ERR_INVALID);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (int64_t)thr_bm25_block_count(nnz);
    hipError_t e = hipMemsetAsync(term_ub, 0, sizeof(double) * n_vocab, st);
    if (e == hipSuccess) e = hipMemsetAsync(block_ub, 0, sizeof(double) * nb, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(bm25_bounds_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, rowptr,
                       post_doc, post_tf, doclen, idf, avgdl, k1, b, n_vocab, nnz,
                       (unsigned long long*)term_ub, (unsigned long long*)block_ub, post_imp);
    hipLaunchKernelGGL(bm25_bounds_decode, dim3((unsigned)((n_vocab + 255) / 256)), dim3(256), 0, st,
                       (unsigned long long*)term_ub, n_vocab);
    hipLaunchKernelGGL(bm25_bounds_decode, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st,
                       (unsigned long long*)block_ub, nb);
    return launch_status();
}

extern "C" int64_t thr_bm25_dense_stride(int64_t n_docs) {
    return n_docs > 0 ? ((n_docs + 15) & ~(int64_t)15) + BW_PAD : 0;
}

extern "C" int thr_bm25_dense_rows(const int64_t* rowptr, const int32_t* post_doc, const int32_t* post_tf,
                                   const uint8_t* post_imp, const int32_t* terms, int n_terms,
                                   int64_t n_docs, int64_t max_df, uint8_t* dense_imp, uint16_t* dense_tf,
                                   thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!rowptr || !post_doc || !post_tf || !post_imp || !terms || !dense_imp || !dense_tf,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_terms <= 0 || n_docs <= 0 || max_df <= 0, THR_ERR_INVALID);
    hipStream_t st = (hipStream_t)stream;
    const int64_t stride = thr_bm25_dense_stride(n_docs);
    hipError_t e = hipMemsetAsync(dense_imp, 0, (size_t)n_terms * stride, st);
    if (e == hipSuccess) e = hipMemsetAsync(dense_tf, 0, sizeof(uint16_t) * (size_t)n_terms * stride, st);
    if (e != hipSuccess) return (int)e;
    int bx = (int)((max_df + 256 * 16 - 1) / (256 * 16));
    bx = bx < 1 ? 1 : bx > 4096 ? 4096 : bx;
    hipLaunchKernelGGL(bm25_dense_rows_kernel, dim3(bx, n_terms), dim3(256), 0, st, rowptr, post_doc, post_tf,
                       post_imp, terms, stride, dense_imp, dense_tf);
    return launch_status();
}
