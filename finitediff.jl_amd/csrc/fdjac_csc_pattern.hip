// CREATE of the consumers on SparseMatrixCSC storage (fdjac_cscsolve.hip, fdjac_csclsq.hip; declared in fdjac_csc_common.h).  Indices only,
// so like colouring it stays with the Float64 build and serves both element types.
//
// colptr / rowval are converted to 0-based Int32 and validated; every entry finds its column by a binary search in colptr and joins its
// row (counts by integer atomics, an exclusive scan, a fill pass whose order depends on the atomics' arrival); every row's segment is
// then SORTED by slot -- storage order is column order, so the lists equal a host counting sort's whatever the arrival order was.  Rows
// of more than kCsLong entries go on a list of their own (an atomic cursor: any order).  A row order per tile of 256 rows (descending
// length, ties by row) deals lanes to rows of similar length.  CSC_WANT_DIAG: the diagonal's slots and the pattern's reach.
// CSC_WANT_COLUMNS: the same lane order for the columns on colptr itself, and the columns of more than kCsLong entries in ASCENDING
// order (flags, a scan, a scatter).
#include "fdjac_internal.h"
#include "fdjac_device.h"
#include "fdjac_csc_common.h"
#include <cstring>

namespace fdjac {

enum { CS_BAD_COLPTR = 1, CS_BAD_ROW = 2, CS_BAD_ORDER = 4 };

__global__ void __launch_bounds__(kBlock) k_cs_colptr(const void *__restrict__ colptr, int ib, int base, int64_t N, int64_t nnz,
                                               int *__restrict__ cptr, unsigned *err)
{
    bool bad = false;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j <= N; j += (int64_t)gridDim.x * kBlock) {
        const int64_t a = cs_load(colptr, ib, j) - base;
        if (j < N) bad = bad || a > cs_load(colptr, ib, j + 1) - base;
        bad = bad || a < 0 || a > nnz || (j == 0 && a != 0) || (j == N && a != nnz);
        cptr[j] = (int)(a < 0 ? 0 : (a > nnz ? nnz : a));
    }
    if (bad) atomicOr(err, (unsigned)CS_BAD_COLPTR);
}

// one lane per entry: its row (validated against M, 0-based), its column (binary search in the monotone cptr), rows strictly ascending
// within the column, the row's count; with diag / reach (a square pattern's): the diagonal's slot and the pattern's reach
__global__ void __launch_bounds__(kBlock) k_cs_entries(const void *__restrict__ rowval, int ib, int base, const int *__restrict__ cptr,
                                                       int64_t M, int64_t N, int64_t nnz, int *__restrict__ erow, int *__restrict__ ecol,
                                                       int *__restrict__ rcnt, int *__restrict__ diag, int *reach, unsigned *err)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kBlock) {
        const int64_t r = cs_load(rowval, ib, q) - base;
        const bool ok = r >= 0 && r < M;
        int64_t lo = 0, hi = N;      // cptr[lo] <= q < cptr[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (cptr[mid] <= q) lo = mid; else hi = mid;
        }
        erow[q] = ok ? (int)r : 0;
        ecol[q] = (int)lo;
        if (!ok) { atomicOr(err, (unsigned)CS_BAD_ROW); continue; }
        if (q > cptr[lo] && cs_load(rowval, ib, q - 1) - base >= r) atomicOr(err, (unsigned)CS_BAD_ORDER);
        atomicAdd(&rcnt[r], 1);
        if (diag && r == lo) diag[lo] = (int)q;
        const int d = (int)(r > lo ? r - lo : lo - r);
        if (reach && d > 0) atomicMax(reach, d);
    }
}

constexpr int kCsScanPer = 8, kCsScanTile = kBlock * kCsScanPer;
__device__ __forceinline__ int cs_block_exscan(int v, int *s_w, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; ++i) {
        if (i < w) before += s_w[i];
        total += s_w[i];
    }
    return before + inc - v;
}
__global__ void __launch_bounds__(kBlock) k_cs_scan_sums(const int *__restrict__ in, int64_t n, int *__restrict__ bsum)
{
    __shared__ int s_w[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kCsScanTile + (int64_t)threadIdx.x * kCsScanPer;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kCsScanPer; ++k) s += i0 + k < n ? in[i0 + k] : 0;
    int total;
    (void)cs_block_exscan(s, s_w, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kBlock) k_cs_scan_top(int *__restrict__ bsum, int64_t nb)      // in place; bsum[nb] = the total
{
    __shared__ int s_w[kBlock / 64];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kBlock) {
        const int64_t i = b0 + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int total;
        const int ex = cs_block_exscan(v, s_w, total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}
__global__ void __launch_bounds__(kBlock) k_cs_scan_apply(const int *__restrict__ in, int64_t n, const int *__restrict__ bsum, int64_t nb,
                                                   int *__restrict__ out)
{
    __shared__ int s_w[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kCsScanTile + (int64_t)threadIdx.x * kCsScanPer;
    int v[kCsScanPer], s = 0;
#pragma unroll
    for (int k = 0; k < kCsScanPer; ++k) {
        v[k] = i0 + k < n ? in[i0 + k] : 0;
        s += v[k];
    }
    int total;
    int run = bsum[blockIdx.x] + cs_block_exscan(s, s_w, total);
#pragma unroll
    for (int k = 0; k < kCsScanPer; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

// the fill pass: slot q joins its row at the position an atomic cursor hands out (any order: the segments are sorted next)
__global__ void __launch_bounds__(kBlock) k_cs_fill(const int *__restrict__ erow, int64_t nnz, const int *__restrict__ rptr,
                                             int *__restrict__ cursor, int *__restrict__ rslot)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kBlock) {
        const int r = erow[q];
        rslot[rptr[r] + atomicAdd(&cursor[r], 1)] = (int)q;
    }
}
// short rows: one lane ranks every slot of its row among the row's (slots are distinct; at most kCsLong^2 compares, no private array),
// parks the sorted slots in the row's segment of rcol, then writes slots and columns; long rows are counted
__global__ void __launch_bounds__(kBlock) k_cs_sort_short(const int *__restrict__ rptr, int64_t N, int *rslot, const int *__restrict__ ecol,
                                                   int *rcol, int *nlong)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= N) return;
    const int a = rptr[r], n = rptr[r + 1] - a;
    if (n > kCsLong) { atomicAdd(nlong, 1); return; }
    for (int k = 0; k < n; ++k) {
        const int v = rslot[a + k];
        int rank = 0;
        for (int i = 0; i < n; ++i) rank += rslot[a + i] < v ? 1 : 0;
        rcol[a + rank] = v;
    }
    for (int k = 0; k < n; ++k) {
        const int v = rcol[a + k];
        rslot[a + k] = v;
        rcol[a + k] = ecol[v];
    }
}
__global__ void __launch_bounds__(kBlock) k_cs_list_long(const int *__restrict__ rptr, int64_t N, int *__restrict__ list, int *cnt)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < N && rptr[r + 1] - rptr[r] > kCsLong) list[atomicAdd(cnt, 1)] = (int)r;
}
// long rows: one workgroup per row ranks every slot among the row's (slots are distinct) into tmp, then copies back
__global__ void __launch_bounds__(kBlock) k_cs_sort_long(const int *__restrict__ rptr, const int *__restrict__ list, int *__restrict__ rslot,
                                                  int *__restrict__ tmp, const int *__restrict__ ecol, int *__restrict__ rcol)
{
    const int r = list[blockIdx.x], a = rptr[r], n = rptr[r + 1] - a;
    for (int k = threadIdx.x; k < n; k += kBlock) {
        const int v = rslot[a + k];
        int rank = 0;
        for (int i = 0; i < n; ++i) rank += rslot[a + i] < v ? 1 : 0;
        tmp[a + rank] = v;
    }
    __threadfence_block();
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kBlock) {
        const int v = tmp[a + k];
        rslot[a + k] = v;
        rcol[a + k] = ecol[v];
    }
}
// the lanes' rows: within every tile of 256 rows, descending length (capped at kCsLong + 1), ties by ascending row
__global__ void __launch_bounds__(kBlock) k_cs_order(const int *__restrict__ rptr, int64_t N, int *__restrict__ order)
{
    __shared__ int s_len[kBlock];
    const int64_t r0 = (int64_t)blockIdx.x * kBlock, r = r0 + threadIdx.x;
    int len = -1;
    if (r < N) { len = rptr[r + 1] - rptr[r]; if (len > kCsLong) len = kCsLong + 1; }
    s_len[threadIdx.x] = len;
    __syncthreads();
    int rank = 0;
    for (int u = 0; u < kBlock; ++u) {
        const int lu = s_len[u];
        rank += (lu > len || (lu == len && u < (int)threadIdx.x)) ? 1 : 0;
    }
    order[r0 + rank] = r < N ? (int)r : -1;
}

// the long columns in ascending order: a flag per column, its exclusive scan, a scatter
__global__ void __launch_bounds__(kBlock) k_cl_flag_long(const int *__restrict__ ptr, int64_t n, int *__restrict__ flag)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) flag[j] = ptr[j + 1] - ptr[j] > kCsLong ? 1 : 0;
}
__global__ void __launch_bounds__(kBlock) k_cl_scatter_long(const int *__restrict__ ptr, int64_t n, const int *__restrict__ pos, int *__restrict__ list)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n && ptr[j + 1] - ptr[j] > kCsLong) list[pos[j]] = (int)j;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static unsigned csc_grid(int64_t n, int per) { const int64_t g = (n + per - 1) / per; return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g)); }
static unsigned csc_tiles(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

static int csc_exscan(hipStream_t st, const int *in, int64_t n, int *out, int *bsum)
{
    const int64_t nb = (n + kCsScanTile - 1) / kCsScanTile;
    hipLaunchKernelGGL(k_cs_scan_sums, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, bsum);
    hipLaunchKernelGGL(k_cs_scan_top, dim3(1), dim3(kBlock), 0, st, bsum, nb);
    hipLaunchKernelGGL(k_cs_scan_apply, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, (const int *)bsum, nb, out);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

struct CscTemps {                      // what a build needs beside the lists; released by csc_lists_build whatever csc_lists_fill returns
    void *raw_cp = nullptr, *raw_rv = nullptr;      // the caller's host indices, staged
    int *ecol = nullptr, *cnt = nullptr, *pos = nullptr, *bsum = nullptr, *tmp = nullptr, *misc = nullptr;
};

static int csc_lists_fill(hipStream_t st, const char *who, const void *colptr, const void *rowval, int idx_bytes, int idx_base, int idx_kind,
                          unsigned want, CscLists *L, CscTemps &T)
{
    const int64_t M = L->M, N = L->N, nnz = L->nnz;
    const int64_t big = M > N ? M : N, nz1 = nnz > 0 ? nnz : 1;
    const int64_t mpad = (M + kBlock - 1) / kBlock * kBlock, npad = (N + kBlock - 1) / kBlock * kBlock;
    const int64_t nscan = (big + kCsScanTile - 1) / kCsScanTile + 2;
    const bool columns = (want & CSC_WANT_COLUMNS) != 0;
    int host_misc[4] = {0, 0, 0, 0};      // err, reach, the long rows, their cursor
    int ncl = 0;
    CSC_TRY(who, hipMalloc((void **)&L->colptr, sizeof(int) * (size_t)(N + 1)));
    CSC_TRY(who, hipMalloc((void **)&L->rowval, sizeof(int) * (size_t)nz1));
    CSC_TRY(who, hipMalloc((void **)&L->row_ptr, sizeof(int) * (size_t)(M + 1)));
    CSC_TRY(who, hipMalloc((void **)&L->row_col, sizeof(int) * (size_t)nz1));
    CSC_TRY(who, hipMalloc((void **)&L->row_slot, sizeof(int) * (size_t)nz1));
    CSC_TRY(who, hipMalloc((void **)&L->row_order, sizeof(int) * (size_t)mpad));
    if (want & CSC_WANT_DIAG) CSC_TRY(who, hipMalloc((void **)&L->diag, sizeof(int) * (size_t)N));
    if (columns) CSC_TRY(who, hipMalloc((void **)&L->col_order, sizeof(int) * (size_t)npad));
    CSC_TRY(who, hipMalloc((void **)&T.ecol, sizeof(int) * (size_t)nz1));
    CSC_TRY(who, hipMalloc((void **)&T.cnt, sizeof(int) * (size_t)big));
    if (columns) CSC_TRY(who, hipMalloc((void **)&T.pos, sizeof(int) * (size_t)(N + 1)));
    CSC_TRY(who, hipMalloc((void **)&T.bsum, sizeof(int) * (size_t)nscan));
    CSC_TRY(who, hipMalloc((void **)&T.misc, sizeof(int) * 4));
    const void *cp = colptr, *rv = rowval;
    if (idx_kind == FD_HOST) {
        CSC_TRY(who, hipMalloc(&T.raw_cp, (size_t)idx_bytes * (size_t)(N + 1)));
        CSC_TRY(who, hipMemcpyAsync(T.raw_cp, colptr, (size_t)idx_bytes * (size_t)(N + 1), hipMemcpyHostToDevice, st));
        cp = T.raw_cp;
        if (nnz > 0) {
            CSC_TRY(who, hipMalloc(&T.raw_rv, (size_t)idx_bytes * (size_t)nnz));
            CSC_TRY(who, hipMemcpyAsync(T.raw_rv, rowval, (size_t)idx_bytes * (size_t)nnz, hipMemcpyHostToDevice, st));
            rv = T.raw_rv;
        }
    }
    CSC_TRY(who, hipMemsetAsync(T.misc, 0, sizeof(int) * 4, st));
    CSC_TRY(who, hipMemsetAsync(T.cnt, 0, sizeof(int) * (size_t)big, st));
    if (L->diag) CSC_TRY(who, hipMemsetAsync(L->diag, 0xFF, sizeof(int) * (size_t)N, st));
    hipLaunchKernelGGL(k_cs_colptr, dim3(csc_grid(N + 1, kBlock)), dim3(kBlock), 0, st, cp, idx_bytes, idx_base, N, nnz, L->colptr, (unsigned *)T.misc);
    CSC_TRY(who, hipGetLastError());
    CSC_TRY(who, hipMemcpyAsync(host_misc, T.misc, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    CSC_TRY(who, hipStreamSynchronize(st));
    FD_REQUIRE(!(host_misc[0] & CS_BAD_COLPTR), FD_ERR_SHAPE, "%s: colptr is not a monotone sequence from the index base to nnz + base", who);
    if (nnz > 0) {
        hipLaunchKernelGGL(k_cs_entries, dim3(csc_grid(nnz, kBlock)), dim3(kBlock), 0, st, rv, idx_bytes, idx_base, (const int *)L->colptr, M, N, nnz,
                           L->rowval, T.ecol, T.cnt, L->diag, L->diag ? T.misc + 1 : (int *)nullptr, (unsigned *)T.misc);
        CSC_TRY(who, hipGetLastError());
    }
    CSC_TRY(who, hipMemcpyAsync(host_misc, T.misc, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    CSC_TRY(who, hipStreamSynchronize(st));
    FD_REQUIRE(!(host_misc[0] & CS_BAD_ROW), FD_ERR_SHAPE, "%s: rowval holds a row outside the %lld x %lld matrix", who, (long long)M, (long long)N);
    FD_REQUIRE(!(host_misc[0] & CS_BAD_ORDER), FD_ERR_SHAPE, "%s: the rows of a column are not strictly ascending", who);
    L->reach = host_misc[1];
    // the pattern by rows
    int rc = csc_exscan(st, T.cnt, M, L->row_ptr, T.bsum);
    if (rc != FD_OK) return rc;
    CSC_TRY(who, hipMemsetAsync(T.cnt, 0, sizeof(int) * (size_t)big, st));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_cs_fill, dim3(csc_grid(nnz, kBlock)), dim3(kBlock), 0, st, (const int *)L->rowval, nnz, (const int *)L->row_ptr, T.cnt, L->row_slot);
        CSC_TRY(who, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cs_sort_short, dim3(csc_tiles(M)), dim3(kBlock), 0, st, (const int *)L->row_ptr, M, L->row_slot, (const int *)T.ecol, L->row_col,
                       T.misc + 2);
    hipLaunchKernelGGL(k_cs_order, dim3(csc_tiles(M)), dim3(kBlock), 0, st, (const int *)L->row_ptr, M, L->row_order);
    CSC_TRY(who, hipGetLastError());
    if (columns) {      // their lane order and the long ones in ascending order
        hipLaunchKernelGGL(k_cs_order, dim3(csc_tiles(N)), dim3(kBlock), 0, st, (const int *)L->colptr, N, L->col_order);
        hipLaunchKernelGGL(k_cl_flag_long, dim3(csc_tiles(N)), dim3(kBlock), 0, st, (const int *)L->colptr, N, T.cnt);
        CSC_TRY(who, hipGetLastError());
        rc = csc_exscan(st, T.cnt, N, T.pos, T.bsum);
        if (rc != FD_OK) return rc;
        CSC_TRY(who, hipMemcpyAsync(&ncl, T.pos + N, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    CSC_TRY(who, hipMemcpyAsync(host_misc, T.misc, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    CSC_TRY(who, hipStreamSynchronize(st));
    L->nlong_r = host_misc[2];
    L->nlong_c = ncl;
    if (L->nlong_r > 0) {
        CSC_TRY(who, hipMalloc((void **)&L->long_rows, sizeof(int) * (size_t)L->nlong_r));
        CSC_TRY(who, hipMalloc((void **)&T.tmp, sizeof(int) * (size_t)nz1));
        hipLaunchKernelGGL(k_cs_list_long, dim3(csc_tiles(M)), dim3(kBlock), 0, st, (const int *)L->row_ptr, M, L->long_rows, T.misc + 3);
        hipLaunchKernelGGL(k_cs_sort_long, dim3((unsigned)L->nlong_r), dim3(kBlock), 0, st, (const int *)L->row_ptr, (const int *)L->long_rows, L->row_slot, T.tmp,
                           (const int *)T.ecol, L->row_col);
        CSC_TRY(who, hipGetLastError());
    }
    if (L->nlong_c > 0) {
        CSC_TRY(who, hipMalloc((void **)&L->long_cols, sizeof(int) * (size_t)L->nlong_c));
        hipLaunchKernelGGL(k_cl_scatter_long, dim3(csc_tiles(N)), dim3(kBlock), 0, st, (const int *)L->colptr, N, (const int *)T.pos, L->long_cols);
        CSC_TRY(who, hipGetLastError());
    }
    return FD_OK;
}

void csc_lists_free(CscLists *L)
{
    void *ptrs[] = {L->colptr, L->rowval, L->row_ptr, L->row_col, L->row_slot, L->row_order, L->long_rows, L->diag, L->col_order, L->long_cols};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    *L = CscLists();
}

int csc_lists_build(fd_ctx *ctx, const char *who, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base,
                    int idx_kind, unsigned want, CscLists *out)
{
    if (!ctx) {      // (no context can exist without a device: say which of the two is the matter)
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); FD_REQUIRE(false, FD_ERR_NODEVICE, "no HIP device"); }
        FD_REQUIRE(false, FD_ERR_ARG, "ctx is NULL");
    }
    FD_REQUIRE(colptr != nullptr, FD_ERR_ARG, "colptr is NULL");
    FD_REQUIRE(N >= 1 && N < ((int64_t)1 << 31) - 4096, FD_ERR_ARG, "N = %lld", (long long)N);      // (first: a square caller's M is its N)
    FD_REQUIRE(M >= 1 && M < ((int64_t)1 << 31) - 4096, FD_ERR_ARG, "M = %lld", (long long)M);
    FD_REQUIRE(idx_bytes == 4 || idx_bytes == 8, FD_ERR_ARG, "idx_bytes = %d (4 or 8)", idx_bytes);
    FD_REQUIRE(idx_base == 0 || idx_base == 1, FD_ERR_ARG, "idx_base = %d (0 or 1)", idx_base);
    FD_REQUIRE(idx_kind == FD_HOST || idx_kind == FD_DEVICE, FD_ERR_ARG, "idx_kind = %d", idx_kind);
    FD_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // nnz from the two ends of colptr
    int64_t ends[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const char *src = (const char *)colptr + (size_t)(k ? N : 0) * idx_bytes;
        int64_t v64 = 0; int32_t v32 = 0;
        void *dst = idx_bytes == 8 ? (void *)&v64 : (void *)&v32;
        if (idx_kind == FD_DEVICE) { FD_HIP_CHECK(hipStreamSynchronize(st)); FD_HIP_CHECK(hipMemcpy(dst, src, idx_bytes, hipMemcpyDeviceToHost)); }
        else std::memcpy(dst, src, idx_bytes);
        ends[k] = idx_bytes == 8 ? v64 : (int64_t)v32;
    }
    const int64_t nnz = ends[1] - ends[0];
    FD_REQUIRE(ends[0] == idx_base, FD_ERR_SHAPE, "colptr[first] = %lld, expected the index base %d", (long long)ends[0], idx_base);
    FD_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31) - 4096, FD_ERR_SHAPE, "colptr[last] - colptr[first] = %lld entries (0 <= nnz < 2^31)", (long long)nnz);
    FD_REQUIRE(nnz == 0 || rowval != nullptr, FD_ERR_ARG, "rowval is NULL");

    *out = CscLists();
    out->M = M; out->N = N; out->nnz = nnz;
    CscTemps T;
    const int rc = csc_lists_fill(st, who, colptr, rowval, idx_bytes, idx_base, idx_kind, want, out, T);
    // the one release of the temporaries, and after a failure of the half-built lists: behind everything the stream still holds
    (void)hipStreamSynchronize(st);
    void *t[] = {T.raw_cp, T.raw_rv, T.ecol, T.cnt, T.pos, T.bsum, T.tmp, T.misc};
    for (void *p : t) if (p) (void)hipFree(p);
    if (rc != FD_OK) csc_lists_free(out);
    return rc;
}

}  // namespace fdjac
