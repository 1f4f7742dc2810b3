// The LEAST-SQUARES consumer: for a rectangular J (M x N) in SparseMatrixCSC storage, on the nzval a CSC plan has just written,
//     y = J v,   y = J^T v,   and the damped Gauss-Newton step   (J^T J + mu W) y = J^T b,   W = I or diag(g), g_j = sum_i J_ij^2,
// by CGLS on the normal equations (J^T J is never formed) preconditioned by m_j = g_j + mu w_j.  DESIGN.md 4.10 has the contract;
// tests/csc_lsq_model.py restates every order below in numpy and the GPU tests compare bits.
//
// CREATE is the shared builder's (fdjac_csc_pattern.hip), with the columns' lane order and the long columns in ascending order.
//
// ORDERS.  (The product scaffold -- cs_gather_sum, k_cs_long, cs_tile_lines -- is fdjac_csc_common.h's, shared with the other consumers.)
// Row r of at most kCsLong entries: acc = 0; acc += nzval[slot_k] * v[col_k], k ascending (ascending column); a longer row by
// one workgroup: thread t adds entries t, t + 256, ... in that order, then block_sum().  Column j of at most kCsLong entries: one lane, storage
// order from +0.0 (g_j: acc += a * a; the product: acc += a * v[row]); a longer column by one workgroup in the same way as a long row.  No
// LDS window of v.  A tile's results cross LDS once, so that everything behind the sums (s, z, the dots) is formed in row / column order.
// Dots of the product kernels: tiles of 256 (element t), dots of the vector kernels: tiles of kCsVecTile (thread t adds t, t + 256, t + 512,
// t + 768), block_sum() per tile, the last-arriving workgroup (an integer ticket) adds the tiles' sums.  All arithmetic is Float64 for
// either element type, nothing is contracted into an FMA, no floating-point atomics, no grid-wide barrier.
//
// THE SOLVE.  r = b, y = 0.  k_cl_cols<1>: g, s = J^T r, m = g + mu w (zero or not finite: breakdown), z = s / m, p = z, gamma = s.z,
// ||s||^2 (-> tol^2 = rtol^2 ||s||^2; 0: done, no iteration), pi = sum (w p) p.  An iteration is four launches (+ 1 with long rows, + 1 with
// long columns):
//   k_cl_rows<1>   q = J p, q.q;  delta = q.q + mu pi (zero or not finite: breakdown);  alpha = gamma / delta
//   k_cl_update    r = r - alpha q,  y = y + alpha p
//   k_cl_cols<2>   s = J^T r - mu (w y), z = s / m, gamma' = s.z, ||s||^2;  the iteration is counted;  ||s||^2 <= tol^2: done;  gamma' not
//                  finite: breakdown;  otherwise beta = gamma' / gamma, gamma = gamma'
//   k_cl_p         p = z + beta p,  pi = sum (w p) p
// Every kernel of an iteration reads the `done` word first and leaves.
#include "fdjac_internal.h"
#include "fdjac_device.h"
#include "fdjac_csc_common.h"
#include <cmath>

namespace fdjac {

// scalars of a least-squares solve, in device memory
enum { LS_GAMMA = 0, LS_ALPHA, LS_BETA, LS_PI, LS_TOL2, LS_GN2, LS_G02, LS_NSCAL = 8 };

struct ClVecs { double *r, *q, *y, *p, *s, *z, *m, *g; };      // r, q: M doubles; the others: N

// ---- products --------------------------------------------------------------------------------------------------------------------------
// The long rows first (k_cs_long<false, CS_LONG_SUM>), then the rows: a tile of 256 rows per workgroup, lane i takes row
// row_order[tile * 256 + i]; v is read from memory; the results cross LDS once (cs_tile_lines) so that y is written -- and q.q is
// summed -- in row order.  MODE 0: y only.  1: q = J p of an iteration, q.q -> delta, alpha.
template <typename TV, int MODE>
__global__ void __launch_bounds__(kBlock) k_cl_rows(CsView P, const real_t *__restrict__ nz, const TV *__restrict__ v, TV *__restrict__ y,
                                                    double mu, double *scal, int *words, double *part)
{
    __shared__ double s_out[kBlock];
    __shared__ double s_w[kBlock / 64];
    if (MODE != 0 && cs_word(words, W_DONE)) return;
    const int r0 = (int)blockIdx.x * kBlock;
    cs_tile_lines<false, false>(P, r0, nz, v, y, nullptr, s_out, nullptr);
    const int row = r0 + threadIdx.x;
    double yr = 0.0;
    if (row < P.M) {
        yr = s_out[threadIdx.x];
        y[row] = (TV)yr;
    }
    if (MODE == 1) {
        double mine[1] = {row < P.M ? yr * yr : 0.0}, tot[1];
        if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
            const double delta = tot[0] + mu * scal[LS_PI];
            if (cs_bad_pivot(delta)) cs_breakdown(words);
            else scal[LS_ALPHA] = scal[LS_GAMMA] / delta;
        }
    }
}

// The long columns first (k_cs_long<true, ...>: y_j, and with CS_LONG_SUM_G g_j = sum a^2 into V.g), then the columns: a tile of 256
// columns per workgroup, lane i takes column col_order[tile * 256 + i] (storage order from +0.0, eight entries' gathers ahead); the
// results cross LDS once (cs_tile_lines) so that what follows is formed in column order.
// MODE 0: y = J^T v.   1: the start of a solve (v = r = b; y = V.s).   2: step 3 of an iteration (v = r; y = V.s).
template <typename TV, int MODE>
__global__ void __launch_bounds__(kBlock) k_cl_cols(CsView P, const real_t *__restrict__ nz, const TV *v, TV *y, ClVecs V,
                                                    double mu, int kind, double rtol, double *scal, int *words, double *part)
{
    __shared__ double s_out[kBlock];
    __shared__ double s_g[MODE == 1 ? kBlock : 1];
    __shared__ double s_w[kBlock / 64];
    if (MODE == 2 && cs_word(words, W_DONE)) return;
    const int j0 = (int)blockIdx.x * kBlock;
    cs_tile_lines<true, MODE == 1>(P, j0, nz, v, y, V.g, s_out, s_g);
    const int col = j0 + threadIdx.x;
    const bool in = col < P.N;
    if (MODE == 0) {
        if (in) y[col] = (TV)s_out[threadIdx.x];
    } else if (MODE == 1) {
        double mine[3] = {0.0, 0.0, 0.0}, tot[3];
        bool bad = false;
        if (in) {
            const double g = s_g[threadIdx.x], s = s_out[threadIdx.x];
            const double w = kind ? g : 1.0;
            const double m = g + mu * w;
            bad = cs_bad_pivot(m);
            const double z = s / m;
            V.g[col] = g; V.m[col] = m; V.s[col] = s; V.z[col] = z; V.p[col] = z; V.y[col] = 0.0;
            mine[0] = s * z; mine[1] = s * s; mine[2] = (w * z) * z;
        }
        if (bad) atomicOr(words + W_FLAGS, 2);
        if (cs_finish<3>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
            scal[LS_GAMMA] = tot[0]; scal[LS_PI] = tot[2]; scal[LS_ALPHA] = 0.0; scal[LS_BETA] = 0.0;
            scal[LS_GN2] = tot[1]; scal[LS_G02] = tot[1];
            scal[LS_TOL2] = (rtol * rtol) * tot[1];
            int done = 0;
            if (tot[1] == 0.0) done = 1;                                             // J^T b = 0: y = 0, no iteration
            else if (cs_word(words, W_FLAGS) & 2) done = 1;                          // an m_j that is zero or not finite
            else if (cs_not_finite(tot[0])) { atomicOr(words + W_FLAGS, 2); done = 1; }   // gamma
            if (done) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        double mine[2] = {0.0, 0.0}, tot[2];
        if (in) {
            const double w = kind ? V.g[col] : 1.0;
            const double s = s_out[threadIdx.x] - mu * (w * V.y[col]);
            const double z = s / V.m[col];
            V.s[col] = s; V.z[col] = z;
            mine[0] = s * z; mine[1] = s * s;
        }
        if (cs_finish<2>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
            scal[LS_GN2] = tot[1];
            words[W_ITERS] = words[W_ITERS] + 1;
            if (tot[1] <= scal[LS_TOL2]) {
                __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (cs_not_finite(tot[0])) {
                cs_breakdown(words);
            } else {
                scal[LS_BETA] = tot[0] / scal[LS_GAMMA];
                scal[LS_GAMMA] = tot[0];
            }
        }
    }
}

// ---- the vector kernels ----------------------------------------------------------------------------------------------------------------
// r = b (the element type widened)
__global__ void __launch_bounds__(kBlock) k_cl_start(int M, const real_t *__restrict__ b, double *__restrict__ r)
{
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i < M) r[i] = (double)b[i];
    }
}
// r = r - alpha q (M elements), y = y + alpha p (N elements)
__global__ void __launch_bounds__(kBlock) k_cl_update(int M, int N, ClVecs V, const double *scal, const int *words)
{
    if (cs_word(words, W_DONE)) return;
    const double al = scal[LS_ALPHA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i < M) V.r[i] = V.r[i] - al * V.q[i];
        if (i < N) V.y[i] = V.y[i] + al * V.p[i];
    }
}
// p = z + beta p, pi = sum (w p) p
__global__ void __launch_bounds__(kBlock) k_cl_p(int N, int kind, ClVecs V, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    if (cs_word(words, W_DONE)) return;
    const double bk = scal[LS_BETA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[1] = {0.0}, tot[1];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double p = V.z[i] + bk * V.p[i];
        const double w = kind ? V.g[i] : 1.0;
        V.p[i] = p;
        mine[0] += (w * p) * p;
    }
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) scal[LS_PI] = tot[0];
}
// the end: bit 0 when the iterations ran out; y and the residual, or NaN after a failure unless the caller keeps the last iterate
__global__ void __launch_bounds__(kBlock) k_cl_final(int M, int N, ClVecs V, real_t *__restrict__ y, real_t *__restrict__ r_out, int *words, int keep)
{
    const int flags = (cs_word(words, W_FLAGS) & 2) | (cs_word(words, W_DONE) ? 0 : 1);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) words[W_FINAL] = flags;
    const bool nan = flags && !keep;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    if (i < N) y[i] = (real_t)(nan ? qnan : V.y[i]);
    if (r_out && i < M) r_out[i] = (real_t)(nan ? qnan : V.r[i]);
}

}  // namespace fdjac

struct fd_csc_lsq : fdjac::CscHandle {};      // d_vec: r, q (M doubles each), then y, p, s, z, m, g (N each)

using namespace fdjac;

static ClVecs cl_vecs(const fd_csc_lsq *s)
{
    ClVecs V;
    const size_t M = (size_t)s->L.M, N = (size_t)s->L.N;
    s->slice({{&V.r, M}, {&V.q, M}, {&V.y, N}, {&V.p, N}, {&V.s, N}, {&V.z, N}, {&V.m, N}, {&V.g, N}});
    return V;
}

int fd_csc_lsq_create(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base, int idx_kind,
                      fd_csc_lsq **out)
{
    return csc_handle_create(out, [&](fd_csc_lsq *s) {
        return s->init(ctx, "csc least squares", M, N, colptr, rowval, idx_bytes, idx_base, idx_kind, CSC_WANT_COLUMNS, 2 * (size_t)M + 6 * (size_t)N,
                       LS_NSCAL, 3 * (int64_t)cs_tiles(M > N ? M : N, kBlock));
    });
}

int fd_csc_lsq_destroy(fd_csc_lsq *s) { return csc_handle_destroy(s); }

int fd_csc_lsq_set_options(fd_csc_lsq *s, double rtol, int max_iterations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "lsq is NULL");
    return s->S.set_options(rtol, max_iterations);
}

int fd_csc_lsq_set_policy(fd_csc_lsq *s, int keep_unconverged)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "lsq is NULL");
    return s->S.set_policy(keep_unconverged);
}

// the lists, for the tests and for callers that want the pattern by rows: device pointers that live as long as the consumer
int fd_csc_lsq_row_lists(fd_csc_lsq *s, const void **row_ptr, const void **row_col, const void **row_slot, int64_t *nnz_out, int64_t *long_rows_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "lsq is NULL");
    if (row_ptr) *row_ptr = s->L.row_ptr;
    if (row_col) *row_col = s->L.row_col;
    if (row_slot) *row_slot = s->L.row_slot;
    if (nnz_out) *nnz_out = s->L.nnz;
    if (long_rows_out) *long_rows_out = s->L.nlong_r;
    return FD_OK;
}

int fd_csc_lsq_long_columns(fd_csc_lsq *s, const void **long_cols, int64_t *count_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "lsq is NULL");
    if (long_cols) *long_cols = s->L.long_cols;
    if (count_out) *count_out = s->L.nlong_c;
    return FD_OK;
}

// q = J v on the stream: the long rows, then the tiles
template <typename TV, int MODE>
static void cl_product_rows(fd_csc_lsq *s, const real_t *nz, const TV *v, TV *y, double mu, bool guarded)
{
    hipStream_t st = s->ctx->stream;
    const CsView P = cs_view(s->L);
    cs_launch_long<false, CS_LONG_SUM>(st, P, nz, v, y, guarded ? s->S.d_words : nullptr);
    hipLaunchKernelGGL((k_cl_rows<TV, MODE>), dim3(cs_tiles(P.M, kBlock)), dim3(kBlock), 0, st, P, nz, v, y, mu, s->S.d_scal, s->S.d_words, s->S.d_part);
}
// y = J^T v on the stream: the long columns, then the tiles
template <typename TV, int MODE>
static void cl_product_cols(fd_csc_lsq *s, const real_t *nz, const TV *v, TV *y, double mu, int kind)
{
    hipStream_t st = s->ctx->stream;
    const CsView P = cs_view(s->L);
    const ClVecs V = cl_vecs(s);
    if constexpr (MODE == 1) cs_launch_long<true, CS_LONG_SUM_G>(st, P, nz, v, y, nullptr, 0.0, 0.0, V.g);
    else cs_launch_long<true, CS_LONG_SUM>(st, P, nz, v, y, MODE == 2 ? s->S.d_words : nullptr);
    hipLaunchKernelGGL((k_cl_cols<TV, MODE>), dim3(cs_tiles(P.N, kBlock)), dim3(kBlock), 0, st, P, nz, v, y, V, mu, kind, s->S.rtol, s->S.d_scal, s->S.d_words, s->S.d_part);
}

int fd_csc_lsq_matvec_async(fd_csc_lsq *s, const void *nzval, const void *v, void *y, int transpose)
{
    FD_REQUIRE(s && v && y && (nzval || s->L.nnz == 0), FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(v != y, FD_ERR_ARG, "y must not be v");
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    if (transpose) cl_product_cols<real_t, 0>(s, (const real_t *)nzval, (const real_t *)v, (real_t *)y, 0.0, 0);
    else cl_product_rows<real_t, 0>(s, (const real_t *)nzval, (const real_t *)v, (real_t *)y, 0.0, false);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

int fd_csc_lsq_solve_async(fd_csc_lsq *s, double mu, int damping_kind, const void *nzval, const void *b, void *y, void *r_out)
{
    FD_REQUIRE(s && b && y && (nzval || s->L.nnz == 0), FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(damping_kind == FD_CSC_LSQ_DAMP_IDENTITY || damping_kind == FD_CSC_LSQ_DAMP_COLNORM, FD_ERR_ARG,
               "damping_kind = %d (0: identity, 1: column norms)", damping_kind);
    FD_REQUIRE(mu >= 0.0, FD_ERR_ARG, "mu = %g (mu >= 0)", mu);      // (a NaN fails the comparison)
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    CscSolveState &S = s->S;
    const int M = (int)s->L.M, N = (int)s->L.N;
    const real_t *nz = (const real_t *)nzval;
    const ClVecs V = cl_vecs(s);
    const unsigned gv = cs_tiles(N, kCsVecTile), gu = cs_tiles(M > N ? M : N, kCsVecTile);
    FD_HIP_CHECK(hipMemsetAsync(S.d_words, 0, sizeof(int) * W_NWORDS, st));
    hipLaunchKernelGGL(k_cl_start, dim3(cs_tiles(M, kCsVecTile)), dim3(kBlock), 0, st, M, (const real_t *)b, V.r);
    cl_product_cols<double, 1>(s, nz, V.r, V.s, mu, damping_kind);
    const int rc = S.run(st, [&] {      // one iteration: 4 launches (+ 1 with long rows, + 1 with long columns)
        cl_product_rows<double, 1>(s, nz, V.p, V.q, mu, true);
        hipLaunchKernelGGL(k_cl_update, dim3(gu), dim3(kBlock), 0, st, M, N, V, (const double *)S.d_scal, (const int *)S.d_words);
        cl_product_cols<double, 2>(s, nz, V.r, V.s, mu, damping_kind);
        hipLaunchKernelGGL(k_cl_p, dim3(gv), dim3(kBlock), 0, st, N, damping_kind, V, S.d_scal, S.d_words, S.d_part);
    });
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(k_cl_final, dim3(cs_tiles(M > N ? M : N, kBlock)), dim3(kBlock), 0, st, M, N, V, (real_t *)y, (real_t *)r_out, S.d_words, S.keep);
    FD_HIP_CHECK(hipGetLastError());
    S.solved = true;
    return FD_OK;
}

int fd_csc_lsq_status(fd_csc_lsq *s, int *flags_out, int64_t *iterations_out, double *grad_norm_out, double *grad0_norm_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "lsq is NULL");
    int w[W_NWORDS];
    double sc[LS_NSCAL];
    const int rc = s->status(w, sc, flags_out, iterations_out);
    if (rc != FD_OK) return rc;
    if (grad_norm_out) *grad_norm_out = std::sqrt(sc[LS_GN2]);
    if (grad0_norm_out) *grad0_norm_out = std::sqrt(sc[LS_G02]);
    return FD_OK;
}
