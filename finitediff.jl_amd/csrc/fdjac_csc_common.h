// Device helpers and create kernels shared by the consumers on SparseMatrixCSC storage (fdjac_cscsolve.hip, fdjac_csclsq.hip): index
// loads, the integer scan, the fill / sort passes that turn a column pattern into lists by rows, the lane order of a tile, and the
// ordered sums (block_sum, the ticket that lets the last-arriving workgroup finish a dot).  Kernels are static: every translation
// unit that includes this header has its own copies.
#pragma once
#include "fdjac_internal.h"
#include "fdjac_device.h"

namespace fdjac {

constexpr int kCsLong = 32;            // rows of more entries than this are summed by a workgroup each
constexpr int kCsVecTile = 1024;       // elements per workgroup of the vector kernels
constexpr int kCsBatchDefault = 8;     // iterations enqueued per record read back
enum { CS_BAD_COLPTR = 1, CS_BAD_ROW = 2, CS_BAD_ORDER = 4 };
// words of a solve, in device memory (the first four are the record the host reads per batch)
enum { W_DONE = 0, W_EARLY, W_FLAGS, W_ITERS, W_TICKET, W_FINAL, W_NWORDS = 8 };

struct CsRecord { int done, early, flags, iters; };       // what the host reads per batch (the first four words)

__device__ __forceinline__ int64_t cs_load(const void *p, int bytes, int64_t i)
{
    return bytes == 8 ? ((const int64_t *)p)[i] : (int64_t)((const int32_t *)p)[i];
}
__device__ __forceinline__ bool cs_bad_pivot(double x) { return !(fabs(x) > 0.0 && fabs(x) < __builtin_huge_val()); }
__device__ __forceinline__ int cs_word(const int *w, int i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- create ------------------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(kBlock) k_cs_colptr(const void *__restrict__ colptr, int ib, int base, int64_t N, int64_t nnz,
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
static __global__ void __launch_bounds__(kBlock) k_cs_scan_sums(const int *__restrict__ in, int64_t n, int *__restrict__ bsum)
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
static __global__ void __launch_bounds__(kBlock) k_cs_scan_top(int *__restrict__ bsum, int64_t nb)      // in place; bsum[nb] = the total
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
static __global__ void __launch_bounds__(kBlock) k_cs_scan_apply(const int *__restrict__ in, int64_t n, const int *__restrict__ bsum, int64_t nb,
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
static __global__ void __launch_bounds__(kBlock) k_cs_fill(const int *__restrict__ erow, int64_t nnz, const int *__restrict__ rptr,
                                                    int *__restrict__ cursor, int *__restrict__ rslot)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kBlock) {
        const int r = erow[q];
        rslot[rptr[r] + atomicAdd(&cursor[r], 1)] = (int)q;
    }
}
// short rows: one lane ranks every slot of its row among the row's (slots are distinct; at most kCsLong^2 compares, no private array),
// parks the sorted slots in the row's segment of rcol, then writes slots and columns; long rows are counted
static __global__ void __launch_bounds__(kBlock) k_cs_sort_short(const int *__restrict__ rptr, int64_t N, int *rslot, const int *__restrict__ ecol,
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
static __global__ void __launch_bounds__(kBlock) k_cs_list_long(const int *__restrict__ rptr, int64_t N, int *__restrict__ list, int *cnt)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < N && rptr[r + 1] - rptr[r] > kCsLong) list[atomicAdd(cnt, 1)] = (int)r;
}
// long rows: one workgroup per row ranks every slot among the row's (slots are distinct) into tmp, then copies back
static __global__ void __launch_bounds__(kBlock) k_cs_sort_long(const int *__restrict__ rptr, const int *__restrict__ list, int *__restrict__ rslot,
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
static __global__ void __launch_bounds__(kBlock) k_cs_order(const int *__restrict__ rptr, int64_t N, int *__restrict__ order)
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

// ---- sums ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cs_block_sum(double x, double *s_w)      // the result is valid in thread 0
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_down(x, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
// ND dots of one kernel: this workgroup's sums go to part[d * nb + block]; the last workgroup to arrive (ticket) adds every dot's
// partial sums in order and returns true in all its threads with the totals in out[] (valid in thread 0)
template <int ND>
__device__ __forceinline__ bool cs_finish(const double (&mine)[ND], double *part, int *words, double (&out)[ND], double *s_w)
{
    __shared__ int s_last;
    const int nb = gridDim.x;
    for (int d = 0; d < ND; ++d) {
        const double t = cs_block_sum(mine[d], s_w);
        if (threadIdx.x == 0) part[(size_t)d * nb + blockIdx.x] = t;
    }
    if (threadIdx.x == 0) {
        __threadfence();
        const int old = __hip_atomic_fetch_add(words + W_TICKET, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == nb - 1;
        if (s_last) __hip_atomic_store(words + W_TICKET, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    for (int d = 0; d < ND; ++d) {
        double acc = 0.0;
        for (int k = threadIdx.x; k < nb; k += kBlock)
            acc += __hip_atomic_load(part + (size_t)d * nb + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[d] = cs_block_sum(acc, s_w);
    }
    return true;
}

}  // namespace fdjac

static inline unsigned csc_grid(int64_t n, int per) { const int64_t g = (n + per - 1) / per; return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g)); }

static inline int csc_exscan(hipStream_t st, const int *in, int64_t n, int *out, int *bsum)
{
    const int64_t nb = (n + fdjac::kCsScanTile - 1) / fdjac::kCsScanTile;
    hipLaunchKernelGGL(fdjac::k_cs_scan_sums, dim3((unsigned)nb), dim3(fdjac::kBlock), 0, st, in, n, bsum);
    hipLaunchKernelGGL(fdjac::k_cs_scan_top, dim3(1), dim3(fdjac::kBlock), 0, st, bsum, nb);
    hipLaunchKernelGGL(fdjac::k_cs_scan_apply, dim3((unsigned)nb), dim3(fdjac::kBlock), 0, st, in, n, (const int *)bsum, nb, out);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}
