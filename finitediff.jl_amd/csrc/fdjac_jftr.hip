// The MATRIX-FREE TRUST-REGION consumer (fd_jftr_*): the Steihaug-Toint step of
//     min g.y + 1/2 y.B y   subject to   ||y||_W <= Delta,     B = lambda I + beta J(x),
// J(x) v the finite-difference JVP of fdjac_jvp.hip for the caller's f! (the gradient) at x -- no pattern, no colouring, no stored H.
// W = I or diag(m) with the caller's m > 0, which also preconditions.  A piece of fdjac_csctr.hip (included at its end, Float64 only):
// CscSolveState, the words, the TR_* scalars, W_EXIT, tr_start_body, tr_decide, k_tr_update, k_tr_p and k_tr_final are that file's; the
// handle's scaffold and the way into jvp_enqueue (JvpHooks) are MfHandle's (fdjac_mf_common.h), shared with fdjac_jfnk.hip.
// tests/jftr_model.py composes the existing models of all of it and the GPU tests compare bits.
//
// THE OPERATOR.  q is what fd_jvp_async gives for (x, v) with the consumer's steps and fdtype, on whichever route jvp_enqueue takes;
// then w_e = lambda v_e + beta q_e, two multiplications and one addition.  k_jt_close stands where k_jvp_diff stood: the quotient as
// k_jvp_diff forms it, the combination, and -- inside a step -- kappa = p.q as a vector-kernel dot (tiles of kCsVecTile, thread t adds
// t, t + 256, t + 512, t + 768, cs_finish<1>), whose last-arriving workgroup takes k_tr_rows<1>'s decision (tr_decide).
// THE DIRECTION.  Above kSmallN k_jt_p<PAIRED> computes p = -z + beta_k p and, in the same traversal, leaves the partial sums of
// dot(x, p) on k_dot_partial's grid and in its order (fdjac_dotx.h: one traversal, one tail), so that the
// JVP that follows skips its dot launch and the operator stays bit-equal to fd_jvp_async on (x, p).  PAIRED is jvp_enqueue's rule on x
// (p is the consumer's own and always starts on a pair).  pi_pp, pi_yp, pi_yy = sum (w p) p, sum (w y) p, sum (w y) y are formed in
// THAT traversal too: per thread in its element order, per workgroup by the same tail, and the last-arriving workgroup
// (an integer ticket) adds the workgroups' sums IN ASCENDING WORKGROUP INDEX from +0.0.  THIS ORDER DIFFERS FROM k_tr_p's (tiles of
// kCsVecTile, cs_finish<3>), so the three scalars -- and what follows from them -- differ in the last bits between the two routes.
// Up to kSmallN (or with the small route off and the fusion switched off): k_tr_p, then the JVP's own dot (k_jvp_small / k_dot_partial).
// The first product of a step (p = -z from k_jt_start) uses the JVP's own dot.
// THE REST is fd_csc_tr_step_async's: W_DONE guards every kernel of an iteration, y and r_out are NaN after a failure unless the
// policy keeps the iterate, pred = -1/2 sum y (g + r).  After `done` the caller's f! is still launched by the steps already enqueued:
// what it writes is scratch that nothing reads.  Nothing is contracted into an FMA, no floating-point atomics, no grid-wide barrier.
#pragma once
#include "fdjac_mf_common.h"

struct fd_jftr : fdjac::MfHandle {             // d_vec: r | q | y | p | z | m | fx; d_diag: the caller's m, or NULL (W = I)
    unsigned long long *d_napp = nullptr;      // the products a step has used, counted by k_jt_close's deciding thread
    int64_t applies = 0;                       // fd_jftr_apply_async calls
    bool fuse_p = true;                        // k_jt_p above kSmallN (FDJAC_JFTR_FUSE=0: k_tr_p and the JVP's own dot)
    ~fd_jftr() { if (d_napp) (void)hipFree(d_napp); }
};

namespace fdjac {

// the start of a step: tr_start_body with the caller's m, or 1; an m_j <= 0 or not finite is a breakdown
__global__ void __launch_bounds__(kBlock) k_jt_start(int N, const double *__restrict__ d, const double *__restrict__ g, TrVecs V, double rtol,
                                                     double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    tr_start_body(N, g, V, rtol, scal, words, part, s_w, [&](int i, bool &bad) {
        if (!d) return 1.0;
        const double m = d[i];
        bad = bad || !(m > 0.0 && m < __builtin_huge_val());
        return m;
    });
}

// The close hook.  q_i = lambda p_i + beta ((a_i - b_i) / e), e = eps[0] or 2 eps[0] exactly as k_jvp_diff forms it; b == NULL: a holds
// the quotient already (a lazy launcher's; a may be q).  STEP: kappa = p.q, and the last-arriving workgroup decides the step length
// and the exit as k_tr_rows<1> does; otherwise (fd_jftr_apply_async) the combination alone, unguarded.
template <bool STEP>
__global__ void __launch_bounds__(kBlock) k_jt_close(const double *a, const double *b, const double *__restrict__ eps, int central, int N,
                                                     double lambda, double beta, const double *__restrict__ p, double *q, double delta2,
                                                     double *scal, int *words, double *part, unsigned long long *napp)
{
    __shared__ double s_w[kBlock / 64];
    if (STEP && cs_word(words, W_DONE)) return;
    const double e = central ? 2 * eps[0] : eps[0];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[1] = {0.0}, tot[1];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double quo = b ? (a[i] - b[i]) / e : a[i];
        const double pi = p[i];
        const double qi = lambda * pi + beta * quo;
        q[i] = qi;
        mine[0] += pi * qi;
    }
    if (!STEP) return;
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        *napp = *napp + 1;
        tr_decide(tot[0], delta2, scal, words);
    }
}

// p = -z + beta_k p on k_dot_partial<PAIRED>'s grid: this workgroup's sum of x_i p_i in that kernel's order (dotx_for_each, dotx_finish)
// goes to partial[] (what k_jvp_eps reads), and its sums of (w p) p, (w y) p, (w y) y -- the same traversal, the same tail -- to
// part[d * gridDim.x + block]; the last-arriving workgroup adds those in ascending workgroup index.  z, p, y and w are the consumer's own
// (on a pair).
template <bool PAIRED>
__global__ void __launch_bounds__(kBlock) k_jt_p(const double *__restrict__ x, int64_t n, TrVecs V, double *__restrict__ partial, double *scal,
                                                 int *words, double *part)
{
    __shared__ double red[4][kBlock / 64];
    __shared__ double s_st[3][kBlock];
    __shared__ int s_last;
    if (cs_word(words, W_DONE)) return;
    typedef double d2_t __attribute__((ext_vector_type(2)));
    const double bk = scal[TR_BETA];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};      // x.p, pi_pp, pi_yp, pi_yy
    const auto one = [&](double xi, double zi, double pi, double wi, double yi) {
        const double pn = -zi + bk * pi;
        acc[0] += xi * pn;
        acc[1] += (wi * pn) * pn; acc[2] += (wi * yi) * pn; acc[3] += (wi * yi) * yi;
        return pn;
    };
    dotx_for_each<PAIRED>(n,
        [&](int64_t i) {
            const d2_t xv = reinterpret_cast<const d2_t *>(x)[i];
            const d2_t zv = reinterpret_cast<const d2_t *>(V.z)[i], pv = reinterpret_cast<const d2_t *>(V.p)[i];
            const d2_t wv = reinterpret_cast<const d2_t *>(V.m)[i], yv = reinterpret_cast<const d2_t *>(V.y)[i];
            d2_t pn;
            pn.x = one(xv.x, zv.x, pv.x, wv.x, yv.x);
            pn.y = one(xv.y, zv.y, pv.y, wv.y, yv.y);
            reinterpret_cast<d2_t *>(V.p)[i] = pn;
        },
        [&](int64_t i) { V.p[i] = one(x[i], V.z[i], V.p[i], V.m[i], V.y[i]); });
    dotx_finish<4>(acc, red);
    const int nb = gridDim.x;
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = acc[0];
        for (int d = 1; d < 4; ++d) part[(size_t)(d - 1) * nb + blockIdx.x] = acc[d];
        __threadfence();
        const int old = __hip_atomic_fetch_add(words + W_TICKET, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == nb - 1;
        if (s_last) __hip_atomic_store(words + W_TICKET, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    double tot = 0.0;                          // thread d < 3: dot d, the workgroups' sums in ascending index
    for (int k0 = 0; k0 < nb; k0 += kBlock) {
        const int k = k0 + threadIdx.x;
        for (int d = 0; d < 3; ++d)
            s_st[d][threadIdx.x] = k < nb ? __hip_atomic_load(part + (size_t)d * nb + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        __syncthreads();
        if (threadIdx.x < 3) {      // (the slots past nb hold +0.0, and tot + 0.0 is tot: from +0.0 a sum is never -0.0)
            const double *row = s_st[threadIdx.x];
#pragma unroll 16
            for (int j = 0; j < kBlock; ++j) tot += row[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) scal[TR_PPP] = tot;
    else if (threadIdx.x == 1) scal[TR_PYP] = tot;
    else if (threadIdx.x == 2) scal[TR_PYY] = tot;
}

struct JtOp {      // one application of the operator: what the closing kernel needs
    fd_jftr *s;
    double lambda, beta, delta2;
    const double *p;
    double *q;
    bool step;
};
static int jt_close(void *user, const double *a, const double *b, const double *eps, int central)
{
    const JtOp *o = (const JtOp *)user;
    fd_jftr *s = o->s;
    const dim3 grid(cs_tiles(s->N, kCsVecTile)), block(kBlock);
    if (o->step)
        hipLaunchKernelGGL(k_jt_close<true>, grid, block, 0, s->ctx->stream, a, b, eps, central, (int)s->N, o->lambda, o->beta, o->p, o->q, o->delta2,
                           s->S.d_scal, s->S.d_words, s->S.d_part, s->d_napp);
    else
        hipLaunchKernelGGL(k_jt_close<false>, grid, block, 0, s->ctx->stream, a, b, eps, central, (int)s->N, o->lambda, o->beta, o->p, o->q, o->delta2,
                           (double *)nullptr, (int *)nullptr, (double *)nullptr, (unsigned long long *)nullptr);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}
// q = lambda p + beta J(x) p; fin: the subtrahend of the forward arm (NULL in the central arm); own_base: it is the consumer's own f(x)
static int jt_operator(fd_jftr *s, double lambda, double beta, double delta2, fd_f_launch f, void *fctx, const double *x, const double *fin,
                       bool own_base, const double *p, double *q, bool have_partials, bool step)
{
    JtOp op = {s, lambda, beta, delta2, p, q, step};
    return s->enqueue(f, fctx, x, p, fin, own_base, q, have_partials, &op, jt_close);
}
constexpr int kJtBaseSlot = 6;      // d_vec: r | q | y | p | z | m | fx
static TrVecs jt_vecs(const fd_jftr *s) { return TrVecs{s->vec(0), s->vec(1), s->vec(2), s->vec(3), s->vec(4), s->vec(5)}; }
static bool jt_beta_ok(double beta) { return beta != 0.0 && std::fabs(beta) < HUGE_VAL; }      // (a NaN fails the comparison)

}  // namespace fdjac

int fd_jftr_create(fd_ctx *ctx, int64_t N, int fdtype, fd_jftr **out)
{
    return csc_handle_create(out, [&](fd_jftr *s) -> int {
        const char *who = "fd_jftr_create";
        // (the partial sums: 3 dots on at most ceil(N / 256) workgroups -- k_jt_p's grid, the JVP plan's nparts, is no larger)
        const int rc = s->init(ctx, who, N, fdtype, kJtBaseSlot + 1, TR_NSCAL, 3 * (int64_t)cs_tiles(N, kBlock));
        if (rc != FD_OK) return rc;
        { const char *e = test_switch("FDJAC_JFTR_FUSE"); s->fuse_p = !(e && *e && atoi(e) == 0); }
        CSC_TRY(who, hipMalloc((void **)&s->d_napp, sizeof(unsigned long long)));
        CSC_TRY(who, hipMemsetAsync(s->d_napp, 0, sizeof(unsigned long long), ctx->stream));
        return FD_OK;
    });
}

int fd_jftr_destroy(fd_jftr *s) { return csc_handle_destroy(s); }

int fd_jftr_set_options(fd_jftr *s, double rtol, int max_iterations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    return s->S.set_options(rtol, max_iterations);
}

int fd_jftr_set_policy(fd_jftr *s, int keep_unconverged)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    return s->S.set_policy(keep_unconverged);
}

int fd_jftr_set_steps(fd_jftr *s, double relstep, double absstep, double dir)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    return s->set_steps(relstep, absstep, dir);
}

int fd_jftr_set_lazy_f(fd_jftr *s, fd_f_launch_lazy_jvp lazy, int caps)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    return s->set_lazy(lazy, caps);
}

int fd_jftr_set_diagonal(fd_jftr *s, const void *m_dev)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    s->d_diag = (const double *)m_dev;
    return FD_OK;
}

int fd_jftr_apply_async(fd_jftr *s, double lambda, double beta, fd_f_launch f, void *fctx, const void *x, const void *f_in, const void *v, void *w)
{
    FD_REQUIRE(s && f && x && v && w, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(w != v && w != x, FD_ERR_ARG, "w must not be v or x");
    FD_REQUIRE(tr_lambda_ok(lambda), FD_ERR_ARG, "lambda = %g (0 <= lambda < Inf)", lambda);
    FD_REQUIRE(jt_beta_ok(beta), FD_ERR_ARG, "beta = %g (finite, not 0)", beta);
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    const double *fin;
    bool own;
    int rc = s->base(f, fctx, (const double *)x, (const double *)f_in, kJtBaseSlot, &fin, &own);
    if (rc == FD_OK) {
        s->applies += 1;
        rc = jt_operator(s, lambda, beta, 0.0, f, fctx, (const double *)x, fin, own, (const double *)v, (double *)w, false, false);
    }
    if (rc != FD_OK) (void)hipStreamSynchronize(s->ctx->stream);
    return rc;
}

int fd_jftr_step_async(fd_jftr *s, double lambda, double beta, double radius, fd_f_launch f, void *fctx, const void *x, const void *f_in,
                       const void *g, void *y, void *r_out)
{
    FD_REQUIRE(s && f && x && g && y, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(y != x && r_out != x, FD_ERR_ARG, "y and r_out must not be x");
    FD_REQUIRE(tr_lambda_ok(lambda), FD_ERR_ARG, "lambda = %g (0 <= lambda < Inf)", lambda);
    FD_REQUIRE(jt_beta_ok(beta), FD_ERR_ARG, "beta = %g (finite, not 0)", beta);
    FD_REQUIRE(radius > 0.0, FD_ERR_ARG, "radius = %g (radius > 0, or +Inf)", radius);      // (a NaN fails the comparison)
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    CscSolveState &S = s->S;
    const int N = (int)s->N;
    const double *xd = (const double *)x;
    const TrVecs V = jt_vecs(s);
    const unsigned gv = cs_tiles(N, kCsVecTile);
    const double delta2 = radius * radius;      // +Inf (radius >= 1.35e154): no boundary
    const bool fused = s->fuse_p && !(s->jp->small_ok && s->N <= kSmallN);
    const bool paired = (((uintptr_t)xd) & kPairMask) == 0;
    const auto run = [&]() -> int {
        const double *fin;
        bool own;
        const int rb = s->base(f, fctx, xd, (const double *)f_in, kJtBaseSlot, &fin, &own);
        if (rb != FD_OK) return rb;
        FD_HIP_CHECK(hipMemsetAsync(S.d_words, 0, sizeof(int) * W_NWORDS, st));
        hipLaunchKernelGGL(k_jt_start, dim3(gv), dim3(kBlock), 0, st, N, s->d_diag, (const double *)g, V, S.rtol, S.d_scal, S.d_words, S.d_part);
        bool partials = false;
        int rc = FD_OK;
        const int rr = S.run(st, [&] {      // one iteration: the JVP's launches with k_jt_close at their end, k_tr_update, k_jt_p / k_tr_p
            if (rc != FD_OK) return;
            rc = jt_operator(s, lambda, beta, delta2, f, fctx, xd, fin, own, V.p, V.q, partials, true);
            if (rc != FD_OK) return;
            hipLaunchKernelGGL(k_tr_update, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
            if (fused) {
                fd_pick<false, true>(paired, [&](auto PAIRED) {
                    hipLaunchKernelGGL(k_jt_p<PAIRED()>, dim3(s->jp->nparts), dim3(kBlock), 0, st, xd, (int64_t)N, V, s->jp->d_partial, S.d_scal, S.d_words,
                                       S.d_part);
                });
                partials = true;
            } else {
                hipLaunchKernelGGL(k_tr_p, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
            }
        });
        return rc != FD_OK ? rc : rr;
    };
    const int rc = run();
    if (rc != FD_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    hipLaunchKernelGGL(k_tr_final, dim3(gv), dim3(kBlock), 0, st, N, V, (const double *)g, (double *)y, (double *)r_out, S.d_scal, S.d_words, S.d_part, S.keep);
    FD_HIP_CHECK(hipGetLastError());
    S.solved = true;
    return FD_OK;
}

int fd_jftr_status(fd_jftr *s, int *flags_out, int *exit_out, int64_t *iterations_out, double *resid_out, double *g_norm_out, double *step_norm_out,
                   double *pred_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    int w[W_NWORDS];
    double sc[TR_NSCAL];
    const int rc = s->S.read_status(s->ctx, w, sc);
    if (rc != FD_OK) return rc;
    if (flags_out) *flags_out = w[W_FINAL];
    if (iterations_out) *iterations_out = w[W_ITERS];
    if (exit_out) *exit_out = w[W_EXIT];
    if (resid_out) *resid_out = std::sqrt(sc[TR_RHO]);
    if (g_norm_out) *g_norm_out = std::sqrt(sc[TR_RHO0]);
    if (step_norm_out) *step_norm_out = std::sqrt(sc[TR_YW2]);
    if (pred_out) *pred_out = sc[TR_PRED];
    return FD_OK;
}

int fd_jftr_counts(fd_jftr *s, int64_t *applications, int64_t *base_evaluations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "tr is NULL");
    if (applications) {
        unsigned long long used = 0;
        FD_HIP_CHECK(hipSetDevice(s->ctx->device));
        FD_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
        FD_HIP_CHECK(hipMemcpy(&used, s->d_napp, sizeof used, hipMemcpyDeviceToHost));
        *applications = s->applies + (int64_t)used;
    }
    if (base_evaluations) *base_evaluations = s->base_evaluations;
    return FD_OK;
}
