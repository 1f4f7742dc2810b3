// Shared by the consumers on SparseMatrixCSC storage (fdjac_cscsolve.hip, fdjac_csclsq.hip, fdjac_csctr.hip).  CREATE lives in fdjac_csc_pattern.hip: it
// touches indices only, so it is compiled once, with the Float64 build, and both element builds call it through the declarations below
// (CscLists, csc_lists_build, csc_lists_free).  Here: the constants, the device helpers of the iteration kernels (index loads, the ordered
// sums block_sum and the ticket that lets the last-arriving workgroup finish a dot, the breakdown store) and CscSolveState, the host
// side of a solve that the consumers share: its device words and scalars, the batch loop and the status read-back.
#pragma once
#include "fdjac_internal.h"
#include "fdjac_device.h"

// ---- the pattern, built once (fdjac_csc_pattern.hip) ---------------------------------------------------------------------------------
// No real_t in any of it: these names stay in the Float64 build's namespace, whatever fdjac_internal.h renames for the Float32 one.
#pragma push_macro("fdjac")
#undef fdjac
namespace fdjac {
enum { CSC_WANT_DIAG = 1, CSC_WANT_COLUMNS = 2 };
struct CscLists {                      // device arrays, 0-based Int32
    int64_t M = 0, N = 0, nnz = 0;
    int nlong_r = 0, nlong_c = 0, reach = 0;     // rows / columns of more than kCsLong entries; max |row - column| (with diag)
    int *colptr = nullptr, *rowval = nullptr;    // the pattern by columns, validated
    int *row_ptr = nullptr, *row_col = nullptr, *row_slot = nullptr;      // ... by rows: every row's columns ascending, and their slots
    int *row_order = nullptr, *long_rows = nullptr;      // the lanes' rows per tile of 256; the long rows in the order an atomic cursor gave
    int *diag = nullptr;                                 // CSC_WANT_DIAG (M == N): the slot of (j, j), -1: not stored
    int *col_order = nullptr, *long_cols = nullptr;      // CSC_WANT_COLUMNS: the lanes' columns per tile; the long columns, ascending
};
// Checks the arguments (`who` opens every message), validates the pattern and builds the lists on ctx's stream; three host
// synchronisations.  After a failure nothing is left allocated.
int csc_lists_build(fd_ctx *ctx, const char *who, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base,
                    int idx_kind, unsigned want, CscLists *out);
void csc_lists_free(CscLists *L);      // (the caller has synchronised the stream; a half-built object is fine)
}
#ifdef FDJAC_F32
namespace fdjac32 { using fdjac::CSC_WANT_DIAG; using fdjac::CSC_WANT_COLUMNS; using fdjac::CscLists; using fdjac::csc_lists_build; using fdjac::csc_lists_free; }
#endif
#pragma pop_macro("fdjac")

namespace fdjac {

constexpr int kCsLong = 32;            // rows of more entries than this are summed by a workgroup each
constexpr int kCsVecTile = 1024;       // elements per workgroup of the vector kernels
constexpr int kCsBatchDefault = 8;     // iterations enqueued per record read back
// words of a solve, in device memory (the first four are the record the host reads per batch)
enum { W_DONE = 0, W_EARLY, W_FLAGS, W_ITERS, W_TICKET, W_FINAL, W_NWORDS = 8 };

struct CsRecord { int done, early, flags, iters; };       // what the host reads per batch (the first four words)

__device__ __forceinline__ int64_t cs_load(const void *p, int bytes, int64_t i)
{
    return bytes == 8 ? ((const int64_t *)p)[i] : (int64_t)((const int32_t *)p)[i];
}
__device__ __forceinline__ bool cs_bad_pivot(double x) { return !(fabs(x) > 0.0 && fabs(x) < __builtin_huge_val()); }
__device__ __forceinline__ int cs_word(const int *w, int i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cs_breakdown(int *words)      // flag bit 1, and the solve is over
{
    atomicOr(words + W_FLAGS, 2);
    __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// ---- the host side of a solve ------------------------------------------------------------------------------------------------------
// a HIP call of a consumer's create: the failure is reported under the consumer's name, out of memory as FD_ERR_NOMEM
inline int csc_hip_failed(const char *who, const char *what, hipError_t e)
{
    set_error("%s: %s failed: %s", who, what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? FD_ERR_NOMEM : FD_ERR_HIP;
}
#define CSC_TRY(who, expr)                                                    \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) return ::fdjac::csc_hip_failed(who, #expr, _e); \
    } while (0)

struct CscSolveState {
    double *d_part = nullptr;          // the tiles' sums of the dots
    double *d_scal = nullptr;          // the consumer's scalars
    int *d_words = nullptr;            // W_*
    CsRecord *h_rec = nullptr;         // pinned: one record per batch in flight (two)
    hipEvent_t ev[2] = {nullptr, nullptr};
    int nscal = 0, batch = kCsBatchDefault;
    double rtol = 1e-10;
    int max_iterations = 500, keep = 0;
    bool solved = false;

    int create(const char *who, hipStream_t st, int nscal_, int64_t npart)
    {
        nscal = nscal_;
        if (const char *v = test_switch("FDJAC_CSC_BATCH")) { const int b = atoi(v); if (b >= 1 && b <= 64) batch = b; }
        CSC_TRY(who, hipMalloc((void **)&d_part, sizeof(double) * (size_t)npart));
        CSC_TRY(who, hipMalloc((void **)&d_scal, sizeof(double) * (size_t)nscal));
        CSC_TRY(who, hipMalloc((void **)&d_words, sizeof(int) * W_NWORDS));
        CSC_TRY(who, hipHostMalloc((void **)&h_rec, sizeof(CsRecord) * 2, hipHostMallocDefault));
        CSC_TRY(who, hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
        CSC_TRY(who, hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
        CSC_TRY(who, hipMemsetAsync(d_scal, 0, sizeof(double) * (size_t)nscal, st));
        CSC_TRY(who, hipMemsetAsync(d_words, 0, sizeof(int) * W_NWORDS, st));
        CSC_TRY(who, hipStreamSynchronize(st));
        return FD_OK;
    }
    void free()      // (the caller has synchronised the stream; a half-built object is fine)
    {
        void *ptrs[] = {d_part, d_scal, d_words};
        for (void *p : ptrs) if (p) (void)hipFree(p);
        if (h_rec) (void)hipHostFree(h_rec);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    int set_options(double rtol_, int max_iterations_)
    {
        FD_REQUIRE(rtol_ >= 0.0 && rtol_ < 1.0, FD_ERR_ARG, "rtol = %g (0 <= rtol < 1)", rtol_);
        FD_REQUIRE(max_iterations_ >= 1, FD_ERR_ARG, "max_iterations = %d", max_iterations_);
        rtol = rtol_; max_iterations = max_iterations_;
        return FD_OK;
    }
    // The iterations, in batches: enqueue_iteration() launches one iteration's kernels on st.  The record of batch k is read while batch
    // k + 1 is already enqueued (its kernels leave at once when the solve is done), so the device never waits for the host.
    template <class F> int run(hipStream_t st, F enqueue_iteration)
    {
        int enq = 0, nb = 0;
        bool stop = false;
        while (!stop) {
            const int todo = max_iterations - enq < batch ? max_iterations - enq : batch;
            for (int it = 0; it < todo; ++it) enqueue_iteration();
            enq += todo;
            FD_HIP_CHECK(hipGetLastError());
            FD_HIP_CHECK(hipMemcpyAsync(&h_rec[nb & 1], d_words, sizeof(CsRecord), hipMemcpyDeviceToHost, st));
            FD_HIP_CHECK(hipEventRecord(ev[nb & 1], st));
            if (nb >= 1) {
                FD_HIP_CHECK(hipEventSynchronize(ev[(nb - 1) & 1]));
                stop = h_rec[(nb - 1) & 1].done != 0;
            }
            ++nb;
            if (enq >= max_iterations) stop = true;
        }
        return FD_OK;
    }
    // synchronises; w[W_FINAL] is replaced by 0 before the first solve
    int read_status(const fd_ctx *ctx, int (&w)[W_NWORDS], double *scalars)
    {
        FD_HIP_CHECK(hipSetDevice(ctx->device));
        FD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        FD_HIP_CHECK(hipMemcpy(w, d_words, sizeof w, hipMemcpyDeviceToHost));
        FD_HIP_CHECK(hipMemcpy(scalars, d_scal, sizeof(double) * (size_t)nscal, hipMemcpyDeviceToHost));
        if (!solved) w[W_FINAL] = 0;
        return FD_OK;
    }
};

}  // namespace fdjac
