// The TRUST-REGION consumer: for a symmetric H (N x N, both triangles stored) in SparseMatrixCSC storage, on the nzval a Hessian launch has
// just written,
//     y = (H + lambda I) v     and the trust-region step     min g.y + 1/2 y.(H + lambda I) y   subject to   ||y||_W <= Delta,
// W = I or diag(m), m_j = |H_jj| + lambda, by the Steihaug-Toint truncated conjugate-gradient method preconditioned by m.  DESIGN.md 4.11
// has the contract; tests/csc_tr_model.py restates every order below in numpy and the GPU tests compare bits.  Float64 only.
//
// CREATE is the shared builder's (fdjac_csc_pattern.hip), with the diagonal's slots.  Symmetry is the caller's contract: not checked.
//
// ORDERS.  (The product scaffold -- cs_gather_sum, k_cs_long, cs_tile_lines -- is fdjac_csc_common.h's, shared with the other consumers.)
// Row r of at most kCsLong entries: acc = 0; acc += nzval[slot_k] * v[col_k], k ascending (ascending column); a longer row by
// one workgroup: thread t adds entries t, t + 256, ... in that order, then block_sum().  Then q_r = acc + lambda * v_r.  No LDS window of
// v.  A tile's results cross LDS once, so that q is written -- and p.q summed -- in row order.  The dot of the row kernel: tiles of 256
// (element t); dots of the vector kernels: tiles of kCsVecTile (thread t adds t, t + 256, t + 512, t + 768); block_sum() per tile, the
// last-arriving workgroup (an integer ticket) adds the tiles' sums.  The weighted dots are sum (w a) b.  Nothing is contracted into an
// FMA, no floating-point atomics, no grid-wide barrier.
//
// THE SOLVE.  k_tr_start: m (kind 1: zero or not finite is a breakdown; kind 0: 1), w = m, y = 0, r = g, z = r / m, p = -z, gamma = r.z,
// rho0 = r.r (-> tol^2 = rtol^2 rho0; 0: done, no iteration), pi_pp = sum (w p) p, pi_yp = pi_yy = 0.  An iteration is three launches
// (+ 1 with long rows):
//   k_tr_rows<1>   q = (H + lambda I) p, kappa = p.q.  kappa not finite: breakdown.  kappa <= 0: Delta^2 = +Inf -> exit 3 and breakdown,
//                  otherwise exit 2, alpha = tau.  kappa > 0: alpha = gamma / kappa; pi_yy + 2 alpha pi_yp + alpha^2 pi_pp >= Delta^2:
//                  exit 1, alpha = tau.   tau = d / (pi_yp + sqrt(pi_yp^2 + pi_pp d)), d = Delta^2 - pi_yy.
//   k_tr_update    y = y + alpha p, r = r + alpha q, z = r / m, gamma' = r.z, rho = r.r; the iteration is counted; an exit chosen by
//                  k_tr_rows: done; rho <= tol^2: done; gamma' not finite: breakdown; otherwise beta = gamma' / gamma, gamma = gamma'
//   k_tr_p         p = -z + beta p;  pi_pp = sum (w p) p, pi_yp = sum (w y) p, pi_yy = sum (w y) y
// Every kernel of an iteration reads the `done` word first and leaves.  k_tr_final: y, r_out (NaN after a failure unless kept),
// ||y||_W^2 = sum (w y) y, pred = -1/2 sum y (g + r).
#include "fdjac_internal.h"
#include "fdjac_device.h"
#include "fdjac_csc_common.h"
#include <cmath>

namespace fdjac {

// scalars of a trust-region solve, in device memory
enum { TR_GAMMA = 0, TR_ALPHA, TR_BETA, TR_PPP, TR_PYP, TR_PYY, TR_TOL2, TR_RHO, TR_RHO0, TR_YW2, TR_PRED, TR_NSCAL = 12 };
constexpr int W_EXIT = W_FINAL + 1;    // the exit kind, in one of the free words
static_assert(W_EXIT < W_NWORDS, "no free word");

struct TrVecs { double *r, *q, *y, *p, *z, *m; };      // N doubles each

// The step length and the exit of an iteration from kappa = p.q: taken by the last-arriving thread of the kernel that closes the product,
// k_tr_rows<1> here and k_jt_close<true> of the matrix-free consumer (fdjac_jftr.hip).
__device__ __forceinline__ void tr_decide(double kappa, double delta2, double *scal, int *words)
{
    const double ppp = scal[TR_PPP], pyp = scal[TR_PYP], pyy = scal[TR_PYY];
    const double d = delta2 - pyy;
    const double tau = d / (pyp + __dsqrt_rn(pyp * pyp + ppp * d));      // the root without cancellation (pi_yp >= 0)
    if (cs_not_finite(kappa)) {
        cs_breakdown(words);
    } else if (kappa <= 0.0) {
        if (cs_not_finite(delta2)) {          // negative curvature and no boundary to follow it to
            words[W_EXIT] = 3;
            cs_breakdown(words);
        } else {
            words[W_EXIT] = 2;
            scal[TR_ALPHA] = tau;
        }
    } else {
        const double al = scal[TR_GAMMA] / kappa;
        if (pyy + 2.0 * al * pyp + al * al * ppp >= delta2) {
            words[W_EXIT] = 1;
            scal[TR_ALPHA] = tau;
        } else {
            scal[TR_ALPHA] = al;
        }
    }
}

// ---- the product -----------------------------------------------------------------------------------------------------------------------
// The long rows first (k_cs_long<false, CS_LONG_SUM>), then the rows: a tile of 256 rows per workgroup, lane i takes row
// row_order[tile * 256 + i]; v is read from memory; the sums cross LDS once (cs_tile_lines) so that y = sum + lambda v is written -- and
// v.y summed -- in row order.  MODE 0: y only.  1: q = (H + lambda I) p of an iteration, kappa = p.q, and the last-arriving workgroup
// decides the step length and the exit.
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_tr_rows(CsView P, const double *__restrict__ nz, const double *__restrict__ v, double *__restrict__ y,
                                                    double lambda, double delta2, double *scal, int *words, double *part)
{
    __shared__ double s_out[kBlock];
    __shared__ double s_w[kBlock / 64];
    if (MODE != 0 && cs_word(words, W_DONE)) return;
    const int r0 = (int)blockIdx.x * kBlock;
    cs_tile_lines<false, false>(P, r0, nz, v, y, nullptr, s_out, nullptr);
    const int row = r0 + threadIdx.x;
    double vr = 0.0, yr = 0.0;
    if (row < P.N) {
        vr = v[row];
        yr = s_out[threadIdx.x] + lambda * vr;
        y[row] = yr;
    }
    if (MODE == 1) {
        double mine[1] = {vr * yr}, tot[1];
        if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) tr_decide(tot[0], delta2, scal, words);
    }
}

// ---- the vector kernels ----------------------------------------------------------------------------------------------------------------
// The start of a solve, for this consumer and the matrix-free one (k_jt_start, fdjac_jftr.hip).  weight(i, bad) returns m_i and sets
// bad where that consumer's test on it fails.
template <class FW>
__device__ __forceinline__ void tr_start_body(int N, const double *__restrict__ g, const TrVecs &V, double rtol, double *scal, int *words, double *part,
                                              double *s_w, FW weight)
{
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[3] = {0.0, 0.0, 0.0}, tot[3];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double m = weight(i, bad);
        const double r = g[i];
        const double z = r / m;
        const double p = -z;
        V.m[i] = m; V.r[i] = r; V.z[i] = z; V.p[i] = p; V.y[i] = 0.0;
        mine[0] += r * z; mine[1] += r * r; mine[2] += (m * p) * p;
    }
    if (bad) atomicOr(words + W_FLAGS, 2);
    if (cs_finish<3>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[TR_GAMMA] = tot[0]; scal[TR_PPP] = tot[2]; scal[TR_PYP] = 0.0; scal[TR_PYY] = 0.0; scal[TR_ALPHA] = 0.0; scal[TR_BETA] = 0.0;
        scal[TR_RHO] = tot[1]; scal[TR_RHO0] = tot[1];
        scal[TR_TOL2] = (rtol * rtol) * tot[1];
        int done = 0;
        if (tot[1] == 0.0) done = 1;                                             // g = 0: y = 0, no iteration
        else if (cs_word(words, W_FLAGS) & 2) done = 1;                          // an m_j that failed the consumer's test
        else if (cs_not_finite(tot[0])) { atomicOr(words + W_FLAGS, 2); done = 1; }   // gamma
        if (done) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// ... with m_j = |H_jj| + lambda (kind 1: zero or not finite is a breakdown), or 1
__global__ void __launch_bounds__(kBlock) k_tr_start(CsView P, int kind, const double *__restrict__ nz, const double *__restrict__ g, TrVecs V,
                                                     double lambda, double rtol, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    tr_start_body(P.N, g, V, rtol, scal, words, part, s_w, [&](int i, bool &bad) {
        if (!kind) return 1.0;
        const int s = P.diag[i];
        const double m = fabs(s >= 0 ? nz[s] : 0.0) + lambda;
        bad = bad || cs_bad_pivot(m);
        return m;
    });
}
// y = y + alpha p, r = r + alpha q, z = r / m, gamma' = r.z, rho = r.r
__global__ void __launch_bounds__(kBlock) k_tr_update(int N, TrVecs V, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    if (cs_word(words, W_DONE)) return;
    const double al = scal[TR_ALPHA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[2] = {0.0, 0.0}, tot[2];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double p = V.p[i];
        V.y[i] = V.y[i] + al * p;
        const double r = V.r[i] + al * V.q[i];
        const double z = r / V.m[i];
        V.r[i] = r; V.z[i] = z;
        mine[0] += r * z; mine[1] += r * r;
    }
    if (cs_finish<2>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[TR_RHO] = tot[1];
        words[W_ITERS] = words[W_ITERS] + 1;
        if (words[W_EXIT] != 0 || tot[1] <= scal[TR_TOL2]) {      // the boundary was reached (k_tr_rows), or converged inside
            __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (cs_not_finite(tot[0])) {
            cs_breakdown(words);
        } else {
            scal[TR_BETA] = tot[0] / scal[TR_GAMMA];
            scal[TR_GAMMA] = tot[0];
        }
    }
}
// p = -z + beta p; pi_pp, pi_yp, pi_yy from the vectors
__global__ void __launch_bounds__(kBlock) k_tr_p(int N, TrVecs V, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    if (cs_word(words, W_DONE)) return;
    const double bk = scal[TR_BETA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[3] = {0.0, 0.0, 0.0}, tot[3];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double p = -V.z[i] + bk * V.p[i];
        const double w = V.m[i], y = V.y[i];
        V.p[i] = p;
        mine[0] += (w * p) * p; mine[1] += (w * y) * p; mine[2] += (w * y) * y;
    }
    if (cs_finish<3>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[TR_PPP] = tot[0]; scal[TR_PYP] = tot[1]; scal[TR_PYY] = tot[2];
    }
}
// the end: bit 0 when the iterations ran out; ||y||_W^2 and pred from the last iterate; y and the model gradient, or NaN after a
// failure unless the caller keeps the last iterate (y or r_out may be g: every element is read before it is written)
__global__ void __launch_bounds__(kBlock) k_tr_final(int N, TrVecs V, const double *g, double *y, double *r_out, double *scal, int *words,
                                                     double *part, int keep)
{
    __shared__ double s_w[kBlock / 64];
    const int flags = (cs_word(words, W_FLAGS) & 2) | (cs_word(words, W_DONE) ? 0 : 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) words[W_FINAL] = flags;
    const bool nan = flags && !keep;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[2] = {0.0, 0.0}, tot[2];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double yi = V.y[i], ri = V.r[i], gi = g[i];
        mine[0] += (V.m[i] * yi) * yi; mine[1] += yi * (gi + ri);
        y[i] = nan ? qnan : yi;
        if (r_out) r_out[i] = nan ? qnan : ri;
    }
    if (cs_finish<2>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[TR_YW2] = tot[0];
        scal[TR_PRED] = -0.5 * tot[1];
    }
}

}  // namespace fdjac

struct fd_csc_tr : fdjac::CscHandle {};      // d_vec: r, q, y, p, z, m (N doubles each)

using namespace fdjac;

static TrVecs tr_vecs(const fd_csc_tr *s)
{
    TrVecs V;
    const size_t N = (size_t)s->L.N;
    s->slice({{&V.r, N}, {&V.q, N}, {&V.y, N}, {&V.p, N}, {&V.z, N}, {&V.m, N}});
    return V;
}

int fd_csc_tr_create(fd_ctx *ctx, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base, int idx_kind, fd_csc_tr **out)
{
    return csc_handle_create(out, [&](fd_csc_tr *s) {
        return s->init(ctx, "fd_csc_tr_create", N, N, colptr, rowval, idx_bytes, idx_base, idx_kind, CSC_WANT_DIAG, 6 * (size_t)N, TR_NSCAL,
                       3 * (int64_t)cs_tiles(N, kBlock));
    });
}

int fd_csc_tr_destroy(fd_csc_tr *s) { return csc_handle_destroy(s); }

int fd_csc_tr_set_options(fd_csc_tr *s, double rtol, int max_iterations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    return s->S.set_options(rtol, max_iterations);
}

int fd_csc_tr_set_policy(fd_csc_tr *s, int keep_unconverged)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    return s->S.set_policy(keep_unconverged);
}

// q = (H + lambda I) v on the stream: the long rows, then the tiles
template <int MODE>
static void tr_product(fd_csc_tr *s, const double *nz, const double *v, double *y, double lambda, double delta2)
{
    hipStream_t st = s->ctx->stream;
    const CsView P = cs_view(s->L);
    cs_launch_long<false, CS_LONG_SUM>(st, P, nz, v, y, MODE ? s->S.d_words : nullptr);
    hipLaunchKernelGGL((k_tr_rows<MODE>), dim3(cs_tiles(P.N, kBlock)), dim3(kBlock), 0, st, P, nz, v, y, lambda, delta2, s->S.d_scal, s->S.d_words, s->S.d_part);
}

static bool tr_lambda_ok(double lambda) { return lambda >= 0.0 && lambda < HUGE_VAL; }      // (a NaN fails the comparison)

int fd_csc_tr_matvec_async(fd_csc_tr *s, double lambda, const void *nzval, const void *v, void *y)
{
    FD_REQUIRE(s && nzval && v && y, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(v != y, FD_ERR_ARG, "y must not be v");
    FD_REQUIRE(tr_lambda_ok(lambda), FD_ERR_ARG, "lambda = %g (0 <= lambda < Inf)", lambda);
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    tr_product<0>(s, (const double *)nzval, (const double *)v, (double *)y, lambda, 0.0);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

int fd_csc_tr_step_async(fd_csc_tr *s, double lambda, double radius, int norm_kind, const void *nzval, const void *g, void *y, void *r_out)
{
    FD_REQUIRE(s && nzval && g && y, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(norm_kind == FD_CSC_TR_NORM_IDENTITY || norm_kind == FD_CSC_TR_NORM_DIAG, FD_ERR_ARG, "norm_kind = %d (0: identity, 1: diagonal)", norm_kind);
    FD_REQUIRE(tr_lambda_ok(lambda), FD_ERR_ARG, "lambda = %g (0 <= lambda < Inf)", lambda);
    FD_REQUIRE(radius > 0.0, FD_ERR_ARG, "radius = %g (radius > 0, or +Inf)", radius);      // (a NaN fails the comparison)
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    CscSolveState &S = s->S;
    const int N = (int)s->L.N;
    const double *nz = (const double *)nzval;
    const TrVecs V = tr_vecs(s);
    const CsView P = cs_view(s->L);
    const unsigned gv = cs_tiles(N, kCsVecTile);
    const double delta2 = radius * radius;      // +Inf (radius >= 1.35e154): no boundary
    FD_HIP_CHECK(hipMemsetAsync(S.d_words, 0, sizeof(int) * W_NWORDS, st));
    hipLaunchKernelGGL(k_tr_start, dim3(gv), dim3(kBlock), 0, st, P, norm_kind, nz, (const double *)g, V, lambda, S.rtol, S.d_scal, S.d_words, S.d_part);
    const int rc = S.run(st, [&] {      // one iteration: 3 launches (+ 1 with long rows)
        tr_product<1>(s, nz, V.p, V.q, lambda, delta2);
        hipLaunchKernelGGL(k_tr_update, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
        hipLaunchKernelGGL(k_tr_p, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
    });
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(k_tr_final, dim3(gv), dim3(kBlock), 0, st, N, V, (const double *)g, (double *)y, (double *)r_out, S.d_scal, S.d_words, S.d_part, S.keep);
    FD_HIP_CHECK(hipGetLastError());
    S.solved = true;
    return FD_OK;
}

int fd_csc_tr_status(fd_csc_tr *s, int *flags_out, int *exit_out, int64_t *iterations_out, double *resid_out, double *g_norm_out,
                     double *step_norm_out, double *pred_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    int w[W_NWORDS];
    double sc[TR_NSCAL];
    const int rc = s->status(w, sc, flags_out, iterations_out);
    if (rc != FD_OK) return rc;
    if (exit_out) *exit_out = w[W_EXIT];
    if (resid_out) *resid_out = std::sqrt(sc[TR_RHO]);
    if (g_norm_out) *g_norm_out = std::sqrt(sc[TR_RHO0]);
    if (step_norm_out) *step_norm_out = std::sqrt(sc[TR_YW2]);
    if (pred_out) *pred_out = sc[TR_PRED];
    return FD_OK;
}

#include "fdjac_jftr.hip"      // the matrix-free trust-region consumer (fd_jftr_*): this file's recurrence on the finite-difference JVP
