// Incremental ingest on the device: segmented concatenation of two CSRs over one row space.
//
// Stands where the reference inserts rag_child_chunks rows one document at a time
// (src/voice_agent/rag2/ingest.py:361-470) and PostgreSQL keeps the `tsv` column + GIN index
// behind the insert (database/migrations/20260114_rag2_schema.sql:146-148, 171-172).  Here the
// index is append-in-place: chunks that arrive later get the largest doc ids, posting lists are
// doc-ascending within a term, so the list of term t after the append is
//
//     [ A's list of t ][ B's list of t ]        A = the index so far, B = the new rows' CSR
//
// for every row t -- a streaming copy, no sort over A.  The same holds for the entity -> chunk
// mention CSR (entity-major, chunk-ascending, a float payload).  B may have more rows than A
// (the vocabulary grew): rows >= rows_a are empty in A.
//
//     rowptr_out[t] = rowptr_a[min(t, rows_a)] + rowptr_b[t]                     t in [0, rows_b]
//     out[rowptr_out[t] + o] = o < len_a(t) ? A[rowptr_a[t] + o] : B[rowptr_b[t] + o - len_a(t)]
//
// Work is cut by OUTPUT POSITION, not by row: this corpus has a handful of stop-word rows with
// >= 1e5 postings next to a long tail of singletons, and a row-per-wave kernel runs as long as its
// longest row.  Each workgroup owns CA_SLICE consecutive output positions, finds the rows they
// span with two binary searches in rowptr_out (wave-uniform: scalar loads), keeps that stretch of
// rowptr_out / rowptr_b in LDS one window at a time, and every lane copies groups of four
// positions: inside a long row source and destination are both contiguous, so a group that does
// not cross a run edge and whose source is 16-byte aligned moves as one dwordx4, anything else
// element by element.  Payloads are opaque 4-byte elements (int32 doc / tf / chunk, float conf),
// one or two arrays sharing the row pointers.  Every source index is checked against nnz_a /
// nnz_b and every destination against nnz_a + nnz_b before it is used, so row pointers that do not
// match the counts the caller passed cannot make the kernel leave its buffers.
#include "thr_common.hpp"

namespace thr {

constexpr int CA_THREADS = 256;
constexpr int CA_SLICE = 8192;   // output positions per workgroup (32 KiB per payload)
constexpr int CA_ROWS = 1024;    // rows per LDS window

__global__ __launch_bounds__(256) void csr_append_rowptr(const int64_t* __restrict__ rowptr_a, int64_t rows_a,
                                                         int64_t nnz_a, const int64_t* __restrict__ rowptr_b,
                                                         int64_t rows_b, int64_t* __restrict__ rowptr_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > rows_b) return;
    const int64_t a = t < rows_a ? rowptr_a[t] : nnz_a;   // (rowptr_a[rows_a] == nnz_a)
    rowptr_out[t] = a + rowptr_b[t];
}

struct Vec4 {
    uint32_t x, y, z, w;
};

template <bool TWO>
__global__ __launch_bounds__(CA_THREADS) void csr_append_copy(
    const int64_t* __restrict__ rowptr_out, const int64_t* __restrict__ rowptr_b, int64_t rows_b,
    const uint32_t* __restrict__ a0, const uint32_t* __restrict__ a1, int64_t nnz_a,
    const uint32_t* __restrict__ b0, const uint32_t* __restrict__ b1, int64_t nnz_b,
    uint32_t* __restrict__ out0, uint32_t* __restrict__ out1, int vec_ok) {
    __shared__ int64_t s_out[CA_ROWS + 1];
    __shared__ int64_t s_b[CA_ROWS + 1];
    const int64_t nnz = nnz_a + nnz_b;
    const int64_t s0 = (int64_t)blockIdx.x * CA_SLICE;
    const int64_t s1 = s0 + CA_SLICE < nnz ? s0 + CA_SLICE : nnz;
    if (s0 >= s1) return;
    // rows the slice spans: t_first = the row holding s0 (last t with rowptr_out[t] <= s0),
    // t_end = first t with rowptr_out[t] >= s1; both wave-uniform, searched side by side
    int64_t lo1 = 0, hi1 = rows_b + 1, lo2 = 0, hi2 = rows_b + 1;
    while (lo1 < hi1 || lo2 < hi2) {
        if (lo1 < hi1) {
            const int64_t m = (lo1 + hi1) >> 1;
            if (rowptr_out[m] <= s0) lo1 = m + 1; else hi1 = m;
        }
        if (lo2 < hi2) {
            const int64_t m = (lo2 + hi2) >> 1;
            if (rowptr_out[m] < s1) lo2 = m + 1; else hi2 = m;
        }
    }
    int64_t t_first = lo1 - 1;
    if (t_first < 0) t_first = 0;
    int64_t t_end = lo2 < rows_b ? lo2 : rows_b;
    for (int64_t tw = t_first; tw < t_end; tw += CA_ROWS) {
        const int nrows = (int)(t_end - tw < CA_ROWS ? t_end - tw : CA_ROWS);
        __syncthreads();   // (the previous window has been read)
        for (int i = threadIdx.x; i <= nrows; i += CA_THREADS) {
            s_out[i] = rowptr_out[tw + i];
            s_b[i] = rowptr_b[tw + i];
        }
        __syncthreads();
        const int64_t w0 = s_out[0], w1 = s_out[nrows];
        const int64_t lo = w0 > s0 ? w0 : s0, hi = w1 < s1 ? w1 : s1;
        for (int64_t g = (lo >> 2) + threadIdx.x; (g << 2) < hi; g += CA_THREADS) {
            int64_t p = g << 2;
            const int64_t pe = p + 4 < hi ? p + 4 : hi;
            if (p < lo) p = lo;
            // row of p inside the window: last i with s_out[i] <= p
            int l = 0, h = nrows;
            while (l < h) {
                const int m = (l + h + 1) >> 1;
                if (s_out[m] <= p) l = m; else h = m - 1;
            }
            int i = l;
            int64_t r_end = s_out[i + 1];
            int64_t a_end = r_end - s_b[i + 1];      // rowptr_a'[t + 1]
            int64_t edge = a_end + s_b[i];           // first position of the row that comes from B
            if (pe - p == 4 && pe <= r_end && (pe <= edge || p >= edge) && vec_ok) {
                const bool from_a = pe <= edge;
                const int64_t src = p - (from_a ? s_b[i] : a_end);
                if ((src & 3) == 0 && src >= 0 && src + 4 <= (from_a ? nnz_a : nnz_b)) {
                    *reinterpret_cast<Vec4*>(out0 + p) = *reinterpret_cast<const Vec4*>((from_a ? a0 : b0) + src);
                    if (TWO)
                        *reinterpret_cast<Vec4*>(out1 + p) = *reinterpret_cast<const Vec4*>((from_a ? a1 : b1) + src);
                    continue;
                }
            }
            for (; p < pe; ++p) {
                while (p >= r_end && i + 1 < nrows) {   // (empty rows in between are stepped over)
                    ++i;
                    r_end = s_out[i + 1];
                    a_end = r_end - s_b[i + 1];
                    edge = a_end + s_b[i];
                }
                if (p >= r_end) break;
                const bool from_a = p < edge;
                const int64_t src = p - (from_a ? s_b[i] : a_end);
                if (src < 0 || src >= (from_a ? nnz_a : nnz_b)) continue;
                out0[p] = (from_a ? a0 : b0)[src];
                if (TWO) out1[p] = (from_a ? a1 : b1)[src];
            }
        }
    }
}

}  // namespace thr

using namespace thr;

extern "C" int thr_csr_append(const int64_t* rowptr_a, int64_t rows_a, int64_t nnz_a, const void* a0,
                              const void* a1, const int64_t* rowptr_b, int64_t rows_b, int64_t nnz_b,
                              const void* b0, const void* b1, int64_t* rowptr_out, void* out0, void* out1,
                              int64_t out_capacity, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!rowptr_b || !rowptr_out, THR_ERR_INVALID);
    THR_RETURN_IF(rows_a < 0 || rows_b <= 0 || rows_b < rows_a || nnz_a < 0 || nnz_b < 0, THR_ERR_INVALID);
    THR_RETURN_IF(rows_b > ((int64_t)1 << 31) - 2 || nnz_a > ((int64_t)1 << 60) || nnz_b > ((int64_t)1 << 60),
                  THR_ERR_INVALID);
    THR_RETURN_IF((rows_a > 0 || nnz_a > 0) && !rowptr_a, THR_ERR_INVALID);
    THR_RETURN_IF(rows_a == 0 && nnz_a != 0, THR_ERR_INVALID);
    const int64_t nnz = nnz_a + nnz_b;
    const bool two = out1 != nullptr;
    THR_RETURN_IF(out_capacity < nnz, THR_ERR_INVALID);
    THR_RETURN_IF(nnz > 0 && !out0, THR_ERR_INVALID);
    THR_RETURN_IF((nnz_a > 0 && !a0) || (nnz_b > 0 && !b0), THR_ERR_INVALID);
    THR_RETURN_IF(two ? ((nnz_a > 0 && !a1) || (nnz_b > 0 && !b1)) : (a1 != nullptr || b1 != nullptr), THR_ERR_INVALID);
    // out of place: the destination is a buffer of its own
    THR_RETURN_IF(out0 && (out0 == a0 || out0 == b0 || out0 == out1), THR_ERR_INVALID);
    THR_RETURN_IF(out1 && (out1 == a1 || out1 == b1), THR_ERR_INVALID);
    THR_RETURN_IF(rowptr_out == rowptr_a || rowptr_out == rowptr_b, THR_ERR_INVALID);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(csr_append_rowptr, dim3((unsigned)((rows_b + 1 + 255) / 256)), dim3(256), 0, st, rowptr_a,
                       rows_a, nnz_a, rowptr_b, rows_b, rowptr_out);
    int rc = launch_status();
    if (rc || nnz == 0) return rc;
    const int64_t blocks = (nnz + CA_SLICE - 1) / CA_SLICE;
    THR_RETURN_IF(blocks > 0x7fffffff, THR_ERR_UNSUPPORTED);
    auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const int vec_ok = al(a0) && al(a1) && al(b0) && al(b1) && al(out0) && al(out1);
    const uint32_t *pa0 = (const uint32_t*)a0, *pa1 = (const uint32_t*)a1, *pb0 = (const uint32_t*)b0,
                   *pb1 = (const uint32_t*)b1;
    if (two)
        hipLaunchKernelGGL(csr_append_copy<true>, dim3((unsigned)blocks), dim3(CA_THREADS), 0, st, rowptr_out,
                           rowptr_b, rows_b, pa0, pa1, nnz_a, pb0, pb1, nnz_b, (uint32_t*)out0, (uint32_t*)out1, vec_ok);
    else
        hipLaunchKernelGGL(csr_append_copy<false>, dim3((unsigned)blocks), dim3(CA_THREADS), 0, st, rowptr_out,
                           rowptr_b, rows_b, pa0, pa1, nnz_a, pb0, pb1, nnz_b, (uint32_t*)out0, (uint32_t*)out1, vec_ok);
    return launch_status();
}
