// Shared by the consumers on SparseMatrixCSC storage (fdjac_cscsolve.hip, fdjac_csclsq.hip, fdjac_csctr.hip).  CREATE lives in fdjac_csc_pattern.hip: it
// touches indices only, so it is compiled once, with the Float64 build, and both element builds call it through the declarations below
// (CscLists, csc_lists_build, csc_lists_free).  Here: the constants, CsView (the pattern as the kernels see it), the device helpers of the
// iteration kernels (index loads, the ordered sums block_sum and the ticket that lets the last-arriving workgroup finish a dot, the
// breakdown store), THE PRODUCT SCAFFOLD that every consumer's product is made of (cs_gather_sum: a short line's sum, eight gathers ahead;
// cs_strided_sum and k_cs_long: a long line by one workgroup; cs_tile_lines: a tile of 256 lines across LDS into line order), and the host
// side that the consumers share: CscSolveState (a solve's device words and scalars, the batch loop, the status read-back) and CscHandle
// (what every consumer's handle holds, with its create / destroy sequence).
#pragma once
#include "fdjac_internal.h"
#include "fdjac_device.h"
#include <initializer_list>
#include <new>
#include <utility>

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

// W_FLAGS: bit 1 (2) is the breakdown the status reports; the bits above it are INTERNAL to the solve's kernels -- GMRES keeps 4 and 8
// (fdjac_cscgmres.hip), and kCsYZero says that the accumulator is not the result: a warm start found b = 0, the final kernel writes y = 0.
// The host's record carries the word as it is: test single bits of CsRecord::flags, never flags != 0.
constexpr int kCsYZero = 16;
struct CsRecord { int done, early, flags, iters; };       // what the host reads per batch (the first four words)

struct CsView {                        // the pattern as the kernels see it: CscLists by value (what a consumer did not ask for is NULL)
    int M, N, nnz, nlong_r, nlong_c, reach, window;      // window: k_cs_rows stages v in LDS (the sparse solver alone)
    const int *colptr, *rowval, *row_ptr, *row_col, *row_slot, *row_order, *long_rows, *diag, *col_order, *long_cols;
};
inline CsView cs_view(const CscLists &L, int window = 0)
{
    return CsView{(int)L.M, (int)L.N, (int)L.nnz, L.nlong_r, L.nlong_c, L.reach, window,
                  L.colptr, L.rowval, L.row_ptr, L.row_col, L.row_slot, L.row_order, L.long_rows, L.diag, L.col_order, L.long_cols};
}
inline unsigned cs_tiles(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ int64_t cs_load(const void *p, int bytes, int64_t i)
{
    return bytes == 8 ? ((const int64_t *)p)[i] : (int64_t)((const int32_t *)p)[i];
}
__device__ __forceinline__ bool cs_bad_pivot(double x) { return !(fabs(x) > 0.0 && fabs(x) < __builtin_huge_val()); }
__device__ __forceinline__ bool cs_not_finite(double x) { return !(fabs(x) < __builtin_huge_val()); }
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

// ---- the product scaffold --------------------------------------------------------------------------------------------------------------
// A LINE is a row read through the row lists (ascending column) or, COLS, a column as it is stored; its entries are the positions
// a .. a + n - 1 of those lists.  Entry p's matrix value, widened, and the index of the vector element it meets:
template <bool COLS, typename TA>
__device__ __forceinline__ double cs_entry(const CsView &P, const TA *nz, int p) { return (double)(COLS ? nz[p] : nz[P.row_slot[p]]); }
template <bool COLS>
__device__ __forceinline__ int cs_meets(const CsView &P, int p) { return COLS ? P.rowval[p] : P.row_col[p]; }

// One lane's sum of a short line: acc = 0; acc += a(k) * v(k), k = 0 .. n - 1 ascending, in groups of eight whose gathers are all
// requested before the first is used.  a(k), v(k): entry k's matrix and vector value as double.  SQ: *sq = sum a(k) * a(k), added entry
// by entry in the same loop.  (The zero slots of a partial group are not added: x + 0.0 is not x for x = -0.0.)
template <bool SQ = false, class FA, class FV>
__device__ __forceinline__ double cs_gather_sum(int n, FA a, FV v, double *sq = nullptr)
{
    double acc = 0.0, acc2 = 0.0;
    for (int k0 = 0; k0 < n; k0 += 8) {
        double pa[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k0 + k < n) {
                pa[k] = a(k0 + k);
                pv[k] = v(k0 + k);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k0 + k < n) {
                acc += pa[k] * pv[k];
                if (SQ) acc2 += pa[k] * pa[k];
            }
        }
    }
    if (SQ) *sq = acc2;
    return acc;
}
// A workgroup's sum of a long line: thread t adds entries t, t + 256, ... in that order from +0.0, then block_sum() (valid in thread 0)
template <bool SQ = false, class FA, class FV>
__device__ __forceinline__ double cs_strided_sum(int n, FA a, FV v, double *s_w, double *sq = nullptr)
{
    double acc = 0.0, acc2 = 0.0;
    for (int k = threadIdx.x; k < n; k += kBlock) {
        const double e = a(k);
        acc += e * v(k);
        if (SQ) acc2 += e * e;
    }
    const double t = cs_block_sum(acc, s_w);
    if (SQ) *sq = cs_block_sum(acc2, s_w);
    return t;
}

// The long lines of a product go first: workgroup i sums line long_rows[i] (COLS: long_cols[i]) and writes y there; the tile kernel that
// follows takes the value from y.  What is written: the sum t (CS_LONG_SUM); alpha v_i + beta t (CS_LONG_AXPBY: the sparse solver's rows);
// t, and g_i = sum a^2 into g (CS_LONG_SUM_G: the start of a least-squares solve).  words: NULL, or the solve whose `done` ends the kernel.
// TY: y's type when it is not v's (the warm start of a solve: v = y0 in the element type, y = A y0 kept in Float64).
enum { CS_LONG_SUM = 0, CS_LONG_AXPBY, CS_LONG_SUM_G };
template <bool COLS, int EPI, typename TV, typename TY = TV>
__global__ void __launch_bounds__(kBlock) k_cs_long(CsView P, double alpha, double beta, const real_t *__restrict__ nz, const TV *__restrict__ v,
                                                    TY *__restrict__ y, double *__restrict__ g, const int *words)
{
    __shared__ double s_w[kBlock / 64];
    if (words && cs_word(words, W_DONE)) return;
    const int i = (COLS ? P.long_cols : P.long_rows)[blockIdx.x];
    const int *ptr = COLS ? P.colptr : P.row_ptr;
    const int a = ptr[i], n = ptr[i + 1] - a;
    double tg = 0.0;
    const double t = cs_strided_sum<EPI == CS_LONG_SUM_G>(n, [&](int k) { return cs_entry<COLS>(P, nz, a + k); },
                                                          [&](int k) { return (double)v[cs_meets<COLS>(P, a + k)]; }, s_w, &tg);
    if (threadIdx.x == 0) {
        y[i] = (TY)(EPI == CS_LONG_AXPBY ? alpha * (double)v[i] + beta * t : t);
        if (EPI == CS_LONG_SUM_G) g[i] = tg;
    }
}

// ... enqueued for the pattern's long lines, if it has any.  alpha, beta: CS_LONG_AXPBY alone reads them; g: CS_LONG_SUM_G alone writes it
template <bool COLS, int EPI, typename TV, typename TY>
inline void cs_launch_long(hipStream_t st, const CsView &P, const real_t *nz, const TV *v, TY *y, const int *words, double alpha = 0.0,
                           double beta = 0.0, double *g = nullptr)
{
    const int n = COLS ? P.nlong_c : P.nlong_r;
    if (n > 0) hipLaunchKernelGGL((k_cs_long<COLS, EPI, TV, TY>), dim3((unsigned)n), dim3(kBlock), 0, st, P, alpha, beta, nz, v, y, g, words);
}

// A tile of 256 lines per workgroup: this lane's line is order[tile0 + lane] (negative: none).  A line of at most kCsLong entries is
// summed here, entry p meeting vec(index); a longer one takes what k_cs_long left in y (G: and in g).  The value -- out(line, sum) of a
// short line -- goes to s_out[line - tile0] (G: the sum of squares to s_g), then the barrier: behind it s_out[t] belongs to line tile0 + t.
template <bool COLS, bool G, typename TA, typename TY, class FV, class FO>
__device__ __forceinline__ void cs_tile_lines(const CsView &P, int tile0, const TA *nz, const TY *y, const double *g, double *s_out, double *s_g,
                                              FV vec, FO out)
{
    const int i = (COLS ? P.col_order : P.row_order)[tile0 + threadIdx.x];
    if (i >= 0) {
        const int *ptr = COLS ? P.colptr : P.row_ptr;
        const int a = ptr[i], n = ptr[i + 1] - a;
        if (n <= kCsLong) {
            double sq = 0.0;
            const double acc = cs_gather_sum<G>(n, [&](int k) { return cs_entry<COLS>(P, nz, a + k); },
                                                [&](int k) { return vec(cs_meets<COLS>(P, a + k)); }, &sq);
            s_out[i - tile0] = out(i, acc);
            if (G) s_g[i - tile0] = sq;
        } else {
            s_out[i - tile0] = (double)y[i];
            if (G) s_g[i - tile0] = g[i];
        }
    }
    __syncthreads();
}
// ... with v read from memory and the plain sum as the value
template <bool COLS, bool G, typename TA, typename TV>
__device__ __forceinline__ void cs_tile_lines(const CsView &P, int tile0, const TA *nz, const TV *v, const TV *y, const double *g, double *s_out,
                                              double *s_g)
{
    cs_tile_lines<COLS, G>(P, tile0, nz, y, g, s_out, s_g, [&](int i) { return (double)v[i]; }, [](int, double acc) { return acc; });
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
    int set_policy(int keep_unconverged)
    {
        keep = keep_unconverged ? 1 : 0;
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

// ---- the host handle of a consumer ---------------------------------------------------------------------------------------------------
// What every consumer's handle (fd_csc_solver, fd_csc_lsq, fd_csc_tr) derives from.  The destructors free (the stream has been
// synchronised; a half-built object is fine): a consumer with buffers of its own frees them in its own.
struct CscHandle {
    fd_ctx *ctx = nullptr;
    CscLists L;                        // (fdjac_csc_pattern.hip)
    CscSolveState S;
    double *d_vec = nullptr;           // the vectors of a solve
    CscHandle() = default;
    CscHandle(const CscHandle &) = delete;
    ~CscHandle()
    {
        csc_lists_free(&L);
        S.free();
        if (d_vec) (void)hipFree(d_vec);
    }
    // the lists, nvec doubles of vectors, the state of a solve with nscal scalars and npart partial sums
    int init(fd_ctx *ctx_, const char *who, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base, int idx_kind,
             unsigned want, size_t nvec, int nscal, int64_t npart)
    {
        const int rc = csc_lists_build(ctx_, who, M, N, colptr, rowval, idx_bytes, idx_base, idx_kind, want, &L);
        if (rc != FD_OK) return rc;
        ctx = ctx_;
        CSC_TRY(who, hipMalloc((void **)&d_vec, sizeof(double) * nvec));
        return S.create(who, ctx->stream, nscal, npart);
    }
    // d_vec in slices: *first takes `second` doubles, in the order given
    void slice(std::initializer_list<std::pair<double **, size_t>> parts) const
    {
        double *p = d_vec;
        for (const auto &part : parts) { *part.first = p; p += part.second; }
    }
    // synchronises; the words and the scalars of the last solve, its flags and its iteration count
    int status(int (&w)[W_NWORDS], double *scalars, int *flags_out, int64_t *iterations_out)
    {
        const int rc = S.read_status(ctx, w, scalars);
        if (rc != FD_OK) return rc;
        if (flags_out) *flags_out = w[W_FINAL];
        if (iterations_out) *iterations_out = w[W_ITERS];
        return FD_OK;
    }
};
// create: init(handle) builds it; after a failure nothing is left allocated.  H: a CscHandle, or the matrix-free consumers' MfHandle
// (fdjac_mf_common.h) -- anything with a ctx that is NULL until it may be used, and a destructor that takes a half-built object
template <class H, class F> int csc_handle_create(H **out, F init)
{
    FD_REQUIRE(out != nullptr, FD_ERR_ARG, "NULL argument");
    *out = nullptr;
    H *s = new (std::nothrow) H();
    FD_REQUIRE(s != nullptr, FD_ERR_NOMEM, "out of host memory");
    const int rc = init(s);
    if (rc != FD_OK) {
        if (s->ctx) (void)hipStreamSynchronize(s->ctx->stream);
        delete s;
        return rc;
    }
    *out = s;
    return FD_OK;
}
template <class H> int csc_handle_destroy(H *s)
{
    if (!s) return FD_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
    return FD_OK;
}

}  // namespace fdjac
