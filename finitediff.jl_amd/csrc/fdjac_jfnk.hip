// The MATRIX-FREE consumer (fd_jfnk_*): (alpha I + beta J(x)) y = b by the restarted GMRES of fdjac_cscgmres.hip on the
// operator itself,  A(x) z = alpha z + beta q,  q = the finite-difference JVP of fdjac_jvp.hip for (x, z) -- no pattern, no colouring, no
// stored J.  A piece of fdjac_cscsolve.hip (included there, in the Float64 build only): the GMRES kernels, CscSolveState, the words and
// the scalars are that file's, the host loop is csc_gmres_iterate(); the handle's scaffold and the way into jvp_enqueue (JvpHooks) are
// MfHandle's (fdjac_mf_common.h), shared with fdjac_jftr.hip.  tests/jfnk_model.py restates every order in numpy and the GPU tests
// compare bits.
//
// THE OPERATOR.  q is what fd_jvp_async gives for (x, z) with the solver's steps and fdtype, on whichever route jvp_enqueue takes (small,
// materialised, lazy values, lazy quotient); then w_e = alpha z_e + beta q_e, two multiplications and one addition.  The closing kernel
// k_jf_close forms the quotient as k_jvp_diff does and the combination in the same pass: it stands where k_jvp_diff stood.
// THE STEP'S z.  With a diagonal d (right preconditioner M = diag(d)) and N above kSmallN, k_jf_open reads x, v_j and d once, stores
// z = v_j / d and leaves the partial sums of dot(x, z) on k_dot_partial's grid and in its order (fdjac_dotx.h: one traversal, one tail);
// k_jvp_eps takes them as they are.  The order is the paired one when x is aligned to a pair (z is the solver's own and always is):
// jvp_enqueue's rule on (x, z), wherever v_j = V + j N and d sit -- off a pair they are read element by element.  Up to kSmallN:
// k_gm_scale<true>, then k_jvp_small.  Without a diagonal z is v_j in place and the JVP's own dot reads it there: for an odd N its
// variant alternates with j.
// A LENT FACTORISATION (fd_jfnk_solver_set_csc_preconditioner): M is what a sparse consumer's fd_csc_solver_factor_async last built --
// lagged by design, checked for validity before anything is enqueued.  Its Jacobi kind IS the diagonal path on the factored diagonal;
// block ILU applies with the lender's k_cs_ilu_apply and leaves the dot to the JVP; block Jacobi above kSmallN runs k_jf_open_blocks,
// k_jf_open with k_cs_bapply's sum in place of the division (up to kSmallN: k_cs_bapply, then k_jvp_small).  The cycle's end is the
// sparse consumer's: k_gm_combine<0>, the apply, k_gm_yadd.  tests/jfnk_pc_model.py composes the existing models of all of it.
// THE REST is the sparse consumer's GMRES (csc_gmres_iterate): y0 = 0 (or the caller's: fd_jfnk_solve_from_async, k_jf_from below),
// CGS2, the rotations, the back substitution, the restart through the same operator (r = b - A(x) y), flags, NaN in y after a failure
// unless the policy keeps the iterate.
// After `cycle over` the kernels here do nothing (gm_idle), but the caller's f! is still launched by the steps already enqueued: what it
// writes is scratch that nothing reads.
#pragma once
#include "fdjac_mf_common.h"

struct fd_jfnk_solver : fdjac::MfHandle {      // d_vec: r | z | w | u | y | fx
    int m = 30;                        // the restart
    double *d_gm = nullptr;            // fdjac_cscgmres.hip: CsGm
    fd_csc_solver *pc = nullptr;       // a sparse consumer's handle lent as the right preconditioner, or NULL (never with d_diag)
    int64_t applications = 0;
    ~fd_jfnk_solver() { if (d_gm) (void)hipFree(d_gm); }
};

namespace fdjac {

// z = v / d, and this workgroup's sum of x_i z_i in k_dot_partial<PAIRED>'s order: dotx_for_each and dotx_finish, as there.
// PAIRED is jvp_enqueue's own rule on the operands of the dot (x and z on a pair), so q is what fd_jvp_async gives for (x, z) wherever
// v and d sit; VLOAD: v and d are on a pair too and are read 16 bytes at a time, otherwise element by element (the same values).
template <bool PAIRED, bool VLOAD>
__global__ void __launch_bounds__(kBlock) k_jf_open(const double *__restrict__ x, const double *__restrict__ v, const double *__restrict__ d,
                                                    int64_t n, double *__restrict__ z, double *__restrict__ partial, const int *words)
{
    if (gm_idle(words)) return;
    typedef double d2_t __attribute__((ext_vector_type(2)));
    double acc[1] = {0.0};
    dotx_for_each<PAIRED>(n,
        [&](int64_t i) {
            const d2_t a = reinterpret_cast<const d2_t *>(x)[i];
            d2_t b, c;
            if (VLOAD) {
                b = reinterpret_cast<const d2_t *>(v)[i];
                c = reinterpret_cast<const d2_t *>(d)[i];
            } else {
                b = d2_t{v[2 * i], v[2 * i + 1]};
                c = d2_t{d[2 * i], d[2 * i + 1]};
            }
            const d2_t q = {b.x / c.x, b.y / c.y};
            reinterpret_cast<d2_t *>(z)[i] = q;
            acc[0] += a.x * q.x;
            acc[0] += a.y * q.y;
        },
        [&](int64_t i) {
            const double q = v[i] / d[i];
            z[i] = q;
            acc[0] += x[i] * q;
        });
    __shared__ double red[1][kBlock / 64];
    dotx_finish<1>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// z = Minv v over the block-Jacobi planes of a lent fd_csc_solver (k_cs_bapply's sum: from +0.0, c ascending, one multiply and one add,
// short last block), and this workgroup's sum of x_i z_i in k_dot_partial<PAIRED>'s order, on its grid.  Trip k of workgroup b covers
// the consecutive elements that k_dot_partial gives the workgroup on that trip: 512 from 2 (b 256 + k stride) when PAIRED (a
// pair per thread, z stored 16 bytes at a time), 256 from b 256 + k stride otherwise (x off a pair).  v for that range, widened to
// whole blocks, goes through LDS element by element wherever it sits.  The trips must be the same in every thread (barriers), so the loop
// is this kernel's own; the odd-N tail is thread 0 of workgroup 0's and the sum's tail is dotx_finish, as in k_jf_open.
template <bool PAIRED>
__global__ void __launch_bounds__(kBlock) k_jf_open_blocks(const double *__restrict__ x, const double *__restrict__ v, const double *__restrict__ minv,
                                                           int bs, int64_t n, double *__restrict__ z, double *__restrict__ partial, const int *words)
{
    constexpr int PER = PAIRED ? 2 : 1;
    __shared__ double s_v[2 * kBlock + 2 * (kCsBsMax - 1)];
    if (gm_idle(words)) return;
    typedef double d2_t __attribute__((ext_vector_type(2)));
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t nloop = PAIRED ? (n >> 1) : n;                  // pairs, or elements
    // one element of z: its block's row of Minv times the block's v (from LDS: `sv` holds v from element w0 on)
    const auto row = [=](int64_t e, const double *sv, int64_t w0) {
        const int64_t b0 = e / bs * bs;
        const int nb = n - b0 < bs ? (int)(n - b0) : bs;
        const double *m = minv + e, *vb = sv + (b0 - w0);
        double t = 0.0;
#pragma unroll 8
        for (int c = 0; c < nb; ++c) t += m[(size_t)c * (size_t)n] * vb[c];
        return t;
    };
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < nloop; base += stride) {      // (the same trips in every thread: barriers)
        const int64_t e0 = base * PER, e1 = e0 + kBlock * PER < nloop * PER ? e0 + kBlock * PER : nloop * PER;
        const int64_t w0 = e0 / bs * bs;
        int64_t w1 = (e1 + bs - 1) / bs * bs;
        if (w1 > n) w1 = n;
        for (int64_t i = w0 + threadIdx.x; i < w1; i += kBlock) s_v[i - w0] = v[i];
        __syncthreads();
        const int64_t i = base + threadIdx.x;
        if (i < nloop) {
            if (PAIRED) {
                const d2_t a = reinterpret_cast<const d2_t *>(x)[i];
                const d2_t q = {row(2 * i, s_v, w0), row(2 * i + 1, s_v, w0)};
                reinterpret_cast<d2_t *>(z)[i] = q;
                acc[0] += a.x * q.x;
                acc[0] += a.y * q.y;
            } else {
                const double q = row(i, s_v, w0);
                z[i] = q;
                acc[0] += x[i] * q;
            }
        }
        __syncthreads();
    }
    if (PAIRED && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t e = n - 1, b0 = e / bs * bs;
        double q = 0.0;
        for (int c = 0; c < (int)(n - b0); ++c) q += minv[(size_t)c * (size_t)n + e] * v[b0 + c];
        z[e] = q;
        acc[0] += x[e] * q;
    }
    __shared__ double red[1][kBlock / 64];
    dotx_finish<1>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// w = alpha z + beta q with q = (a - b) / e, e = eps[0] or 2 eps[0] exactly as k_jvp_diff forms it; b == NULL: a holds q already (a lazy
// launcher's quotient; a may be w).  mode 3: nothing once the cycle is over; 4: nothing once the solve is; words == NULL: unguarded.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_jf_close(const double *a, const double *b, const double *__restrict__ eps, int central, int64_t n,
                                                     double alpha, double beta, const double *__restrict__ z, double *w, const int *words, int mode)
{
    if (words && (cs_word(words, W_DONE) || (mode == 3 && cs_word(words, W_EARLY)))) return;
    typedef double d2_t __attribute__((ext_vector_type(2)));
    const double e = central ? 2 * eps[0] : eps[0];
    if (VEC) {
        const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2;
        if (i + 1 < n) {
            d2_t q = *reinterpret_cast<const d2_t *>(a + i);
            if (b) {
                const d2_t bv = *reinterpret_cast<const d2_t *>(b + i);
                q = d2_t{(q.x - bv.x) / e, (q.y - bv.y) / e};
            }
            const d2_t zv = *reinterpret_cast<const d2_t *>(z + i);
            *reinterpret_cast<d2_t *>(w + i) = d2_t{alpha * zv.x + beta * q.x, alpha * zv.y + beta * q.y};
        } else if (i < n) {
            const double q = b ? (a[i] - b[i]) / e : a[i];
            w[i] = alpha * z[i] + beta * q;
        }
        return;
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double q = b ? (a[i] - b[i]) / e : a[i];
        w[i] = alpha * z[i] + beta * q;
    }
}

// the start of a solve: r = b, y = 0, ||b||^2, and the diagonal's check -- k_cs_init<0> with the caller's d in place of the pattern's;
// fwords: the words of a lent factorisation (NULL: none), whose flag bit 1 ends the solve here as a bad d_e does
__global__ void __launch_bounds__(kBlock) k_jf_init(int N, const double *__restrict__ d, const double *__restrict__ b, double *__restrict__ r,
                                                    double *__restrict__ y, double rtol, double *scal, int *words, double *part, const int *fwords)
{
    __shared__ double s_w[kBlock / 64];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[1] = {0.0}, tot[1];
    bool bad = false;
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double bi = b[i];
        if (d) bad = bad || cs_bad_pivot(d[i]);
        r[i] = bi; y[i] = 0.0;
        mine[0] += bi * bi;
    }
    if (fwords && threadIdx.x == 0 && (cs_word(fwords, W_FLAGS) & 2)) bad = true;
    if (bad) atomicOr(words + W_FLAGS, 2);
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[S_BNORM2] = tot[0];
        int done = 0;
        if (tot[0] == 0.0) done = 1;                                                 // b = 0: y = 0, no iteration
        else if (cs_word(words, W_FLAGS) & 2) done = 1;                              // a d_e that is zero or not finite
        else if (cs_bad_pivot(tot[0])) { atomicOr(words + W_FLAGS, 2); done = 1; }   // ||b||^2 not finite
        if (done) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the warm start behind w = A(x) y0 (one application of the operator, k_jf_init before it): r0 = b - w (one subtraction), the
// accumulator y = y0, ||r0||^2 in dot_vec's order; the last workgroup leaves gamma^2 = ||r0||^2 for k_gm_start<2> and ends the solve on
// ||r0||^2 not finite (breakdown: a NaN in y0) or ||r0||^2 <= rtol^2 ||b||^2 (y = y0, no iteration).  Nothing once k_jf_init has ended
// the solve (b = 0: y stays 0; a bad preconditioner; ||b||^2 not finite).
__global__ void __launch_bounds__(kBlock) k_jf_from(int N, const double *__restrict__ b, const double *__restrict__ w, const double *__restrict__ y0,
                                                    double *__restrict__ r, double *__restrict__ y, double rtol, double *scal, int *words, double *part,
                                                    int keep)
{
    __shared__ double s_w[kBlock / 64];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    if (cs_word(words, W_DONE)) {      // k_jf_init has ended the solve: w is not read (it may hold anything) and k_gm_start<2> reports ||b||
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_GAMMA2] = scal[S_BNORM2];
        // under the keep policy the iterate of a breakdown before the first step is y0 (not after b = 0)
        if (keep && (cs_word(words, W_FLAGS) & 2) && scal[S_BNORM2] != 0.0)
            for (int k = 0; k < kCsVecTile / kBlock; ++k)
                if (i0 + k * kBlock < N) y[i0 + k * kBlock] = y0[i0 + k * kBlock];
        return;
    }
    double mine[1] = {0.0}, tot[1];
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double ri = b[i] - w[i];
        r[i] = ri; y[i] = y0[i];
        mine[0] += ri * ri;
    }
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[S_GAMMA2] = tot[0];
        if (cs_not_finite(tot[0])) cs_breakdown(words);
        else if (tot[0] <= (rtol * rtol) * scal[S_BNORM2]) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int balanced_grid(int64_t tiles, int64_t cap);

struct JfOp {      // one application of the operator: what the closing kernel needs
    fd_jfnk_solver *s;
    double alpha, beta;
    const double *z;
    double *w;
    const int *words;
    int mode;
};
static int jf_close(void *user, const double *a, const double *b, const double *eps, int central)
{
    const JfOp *o = (const JfOp *)user;
    const int64_t N = o->s->N;
    hipStream_t st = o->s->ctx->stream;
    const uintptr_t al = ((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)o->z) | ((uintptr_t)o->w);
    if ((al & kPairMask) == 0)
        hipLaunchKernelGGL(k_jf_close<true>, dim3((unsigned)((N + 2 * kBlock - 1) / (2 * kBlock))), dim3(kBlock), 0, st, a, b, eps, central, N, o->alpha,
                           o->beta, o->z, o->w, o->words, o->mode);
    else
        hipLaunchKernelGGL(k_jf_close<false>, dim3(balanced_grid((N + kBlock - 1) / kBlock, (int64_t)o->s->ctx->num_cus * 8)), dim3(kBlock), 0, st, a, b,
                           eps, central, N, o->alpha, o->beta, o->z, o->w, o->words, o->mode);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}
// w = alpha z + beta J(x) z; fin: the subtrahend of the forward arm (NULL in the central arm); own_base: it is the solver's own f(x)
static int jf_operator(fd_jfnk_solver *s, double alpha, double beta, fd_f_launch f, void *fctx, const double *x, const double *fin, bool own_base,
                       const double *z, double *w, bool have_partials, const int *words, int mode)
{
    JfOp op = {s, alpha, beta, z, w, words, mode};
    s->applications += 1;
    return s->enqueue(f, fctx, x, z, fin, own_base, w, have_partials, &op, jf_close);
}
constexpr int kJfBaseSlot = 5;      // d_vec: r | z | w | u | y | fx

}  // namespace fdjac

extern "C" {

int fd_jfnk_solver_create(fd_ctx *ctx, int64_t N, int fdtype, int restart, fd_jfnk_solver **out)
{
    return csc_handle_create(out, [&](fd_jfnk_solver *s) -> int {
        const char *who = "jfnk solver";
        const int ra = mf_check_args(ctx, N, fdtype);      // (first, as init has them: the restart's check comes after N's and fdtype's)
        if (ra != FD_OK) return ra;
        FD_REQUIRE(restart >= 1 && restart <= kGmMax, FD_ERR_ARG, "restart = %d (1 .. %d)", restart, kGmMax);
        const int rc = s->init(ctx, who, N, fdtype, kJfBaseSlot + 1, S_NSCAL, 2 * (int64_t)cs_tiles(N, kBlock));
        if (rc != FD_OK) return rc;
        s->m = restart;
        CSC_TRY(who, hipMalloc((void **)&s->d_gm, sizeof(double) * gm_doubles((size_t)N, restart, cs_tiles(N, kCsVecTile))));
        return FD_OK;
    });
}

int fd_jfnk_solver_destroy(fd_jfnk_solver *s) { return csc_handle_destroy(s); }

int fd_jfnk_solver_set_options(fd_jfnk_solver *s, double rtol, int max_iterations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    return s->S.set_options(rtol, max_iterations);
}

int fd_jfnk_solver_set_policy(fd_jfnk_solver *s, int keep_unconverged)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    return s->S.set_policy(keep_unconverged);
}

int fd_jfnk_solver_set_steps(fd_jfnk_solver *s, double relstep, double absstep, double dir)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    return s->set_steps(relstep, absstep, dir);
}

int fd_jfnk_solver_set_lazy_f(fd_jfnk_solver *s, fd_f_launch_lazy_jvp lazy, int caps)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    return s->set_lazy(lazy, caps);
}

int fd_jfnk_solver_set_diagonal(fd_jfnk_solver *s, const void *d_dev)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(d_dev == nullptr || s->pc == nullptr, FD_ERR_ARG, "a csc preconditioner is set: clear it first (fd_jfnk_solver_set_csc_preconditioner(solver, NULL))");
    s->d_diag = (const double *)d_dev;
    return FD_OK;
}

// the right preconditioner M of a lent sparse consumer: whatever its last fd_csc_solver_factor_async built, reused by every solve
int fd_jfnk_solver_set_csc_preconditioner(fd_jfnk_solver *s, fd_csc_solver *pc)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    if (pc) {
        FD_REQUIRE(s->d_diag == nullptr, FD_ERR_ARG, "a diagonal is set: clear it first (fd_jfnk_solver_set_diagonal(solver, NULL))");
        FD_REQUIRE(pc->elem_bytes == (int)sizeof(double), FD_ERR_ARG, "the preconditioner must be a Float64 fd_csc_solver (this one holds %d-byte elements)",
                   pc->elem_bytes);
        FD_REQUIRE(pc->ctx == s->ctx, FD_ERR_ARG, "the preconditioner lives on another context");
        FD_REQUIRE(pc->L.N == s->N, FD_ERR_SHAPE, "the preconditioner has N = %lld, the solver N = %lld", (long long)pc->L.N, (long long)s->N);
    }
    s->pc = pc;
    return FD_OK;
}

int fd_jfnk_apply_async(fd_jfnk_solver *s, double alpha, double beta, fd_f_launch f, void *fctx, const void *x, const void *f_in, const void *z,
                        void *w)
{
    FD_REQUIRE(s && f && x && z && w, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(w != z && w != x, FD_ERR_ARG, "w must not be z or x");
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    const double *fin;
    bool own;
    int rc = s->base(f, fctx, (const double *)x, (const double *)f_in, kJfBaseSlot, &fin, &own);
    if (rc == FD_OK) rc = jf_operator(s, alpha, beta, f, fctx, (const double *)x, fin, own, (const double *)z, (double *)w, false, nullptr, 0);
    if (rc != FD_OK) (void)hipStreamSynchronize(s->ctx->stream);
    return rc;
}

int fd_jfnk_solve_async(fd_jfnk_solver *s, double alpha, double beta, fd_f_launch f, void *fctx, const void *x, const void *f_in, const void *b,
                        void *y)
{
    return fd_jfnk_solve_from_async(s, alpha, beta, f, fctx, x, f_in, b, nullptr, y);
}

// y0 == NULL: the cold start, launch for launch.  Otherwise, behind k_jf_init: one application of the operator on y0 (the JVP's own
// launches) and k_jf_from; the first cycle then opens on r0 (k_gm_start<2>).  With a preconditioner the host reads the record behind
// k_jf_init first (one synchronisation): a solve that k_jf_init has ended -- a bad pivot above all -- enqueues and counts no product.
int fd_jfnk_solve_from_async(fd_jfnk_solver *s, double alpha, double beta, fd_f_launch f, void *fctx, const void *x, const void *f_in, const void *b,
                             const void *y0, void *y)
{
    FD_REQUIRE(s && f && x && b && y, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(y != x, FD_ERR_ARG, "y must not be x");
    fd_csc_solver *pc = s->pc;
    if (pc) {      // (before anything is enqueued)
        const int rv = csc_factor_valid(pc);
        if (rv != FD_OK) return rv;
    }
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    CscSolveState &S = s->S;
    const int N = (int)s->N;
    const unsigned gv = cs_tiles(N, kCsVecTile);
    // a lent factorisation: the Jacobi kind IS the diagonal path on the factored diagonal; blocks / ILU go through the lender's applies
    const bool pc_blocks = pc && pc->fact_kind != FD_CSC_PRECOND_JACOBI, pc_bjac = pc && pc->fact_kind == FD_CSC_PRECOND_BLOCK_JACOBI;
    const double *xd = (const double *)x, *d = pc ? (pc_blocks ? nullptr : pc->d_fdiag) : s->d_diag;
    CsVecs V = {};
    V.r = s->vec(0); V.p = s->vec(1); V.v = s->vec(2); V.s = s->vec(3); V.y = s->vec(4); V.d = const_cast<double *>(d);
    const CsGm G = gm_view(s->d_gm, (size_t)N, s->m);
    const int *words = S.d_words;
    const auto run = [&]() -> int {
        const double *fin = nullptr;
        bool own = false;
        if (!y0) {
            const int rb = s->base(f, fctx, xd, (const double *)f_in, kJfBaseSlot, &fin, &own);
            if (rb != FD_OK) return rb;
        }
        FD_HIP_CHECK(hipMemsetAsync(S.d_words, 0, sizeof(int) * W_NWORDS, st));
        hipLaunchKernelGGL(k_jf_init, dim3(gv), dim3(kBlock), 0, st, N, d, (const double *)b, V.r, V.y, S.rtol, S.d_scal, S.d_words, S.d_part,
                           pc ? (const int *)pc->d_fwords : (const int *)nullptr);
        if (y0) {
            if (d || pc) {      // the preconditioner's verdict before anything of the operator is enqueued
                FD_HIP_CHECK(hipMemcpyAsync(&S.h_rec[0], S.d_words, sizeof(CsRecord), hipMemcpyDeviceToHost, st));
                FD_HIP_CHECK(hipStreamSynchronize(st));
                if (S.h_rec[0].done) {      // (no product: V.v holds whatever the last solve left, and k_jf_from does not read it once `done`)
                    hipLaunchKernelGGL(k_jf_from, dim3(gv), dim3(kBlock), 0, st, N, (const double *)b, (const double *)V.v, (const double *)y0, V.r, V.y,
                                       S.rtol, S.d_scal, S.d_words, S.d_part, S.keep);
                    hipLaunchKernelGGL(k_gm_start<2>, dim3(gv), dim3(kBlock), 0, st, N, (const double *)V.r, G, S.rtol, S.d_scal, words);
                    return FD_OK;
                }
            }
            const int rb = s->base(f, fctx, xd, (const double *)f_in, kJfBaseSlot, &fin, &own);
            if (rb != FD_OK) return rb;
            const int ro = jf_operator(s, alpha, beta, f, fctx, xd, fin, own, (const double *)y0, V.v, false, words, 4);
            if (ro != FD_OK) return ro;
            hipLaunchKernelGGL(k_jf_from, dim3(gv), dim3(kBlock), 0, st, N, (const double *)b, (const double *)V.v, (const double *)y0, V.r, V.y, S.rtol,
                               S.d_scal, S.d_words, S.d_part, S.keep);
        }
        const bool fused = (d != nullptr || pc_bjac) && !(s->jp->small_ok && s->N <= kSmallN);
        bool partials = false;
        return csc_gmres_iterate(st, S, N, G, (const double *)b, V, y0 != nullptr,
            [&](const double *vj, double *z, const double **zj) {      // z = v_j / d, or v_j itself
                partials = false;
                if (pc_blocks) {
                    *zj = z;
                    if (!pc_bjac || !fused) { csc_factor_apply(pc, 1, vj, z, words); return FD_OK; }
                    const bool paired = ((((uintptr_t)xd) | ((uintptr_t)z)) & kPairMask) == 0;
                    fd_pick<false, true>(paired, [&](auto PAIRED) {
                        hipLaunchKernelGGL(k_jf_open_blocks<PAIRED()>, dim3(s->jp->nparts), dim3(kBlock), 0, st, xd, vj, (const double *)pc->d_minv, pc->fact_bs,
                                           (int64_t)N, z, s->jp->d_partial, words);
                    });
                    partials = true;
                    return FD_OK;
                }
                if (!d) { *zj = vj; return FD_OK; }
                *zj = z;
                if (!fused) {
                    hipLaunchKernelGGL(k_gm_scale<true>, dim3(gv), dim3(kBlock), 0, st, N, vj, d, z, words);
                    return FD_OK;
                }
                // the dot's order is jvp_enqueue's rule on (x, z); 0: scalar, 1: paired with v_j or d off a pair, 2: paired, 16-byte loads
                const bool paired = ((((uintptr_t)xd) | ((uintptr_t)z)) & kPairMask) == 0;
                const bool vload = ((((uintptr_t)vj) | ((uintptr_t)d)) & kPairMask) == 0;
                fd_pick<0, 1, 2>(paired ? (vload ? 2 : 1) : 0, [&](auto HOW) {
                    hipLaunchKernelGGL((k_jf_open<(HOW() > 0), (HOW() == 2)>), dim3(s->jp->nparts), dim3(kBlock), 0, st, xd, vj, d, (int64_t)N, z,
                                       s->jp->d_partial, words);
                });
                partials = true;
                return FD_OK;
            },
            [&](int mode, const double *v, double *w) {
                const bool hp = mode == 3 && partials;
                partials = false;
                return jf_operator(s, alpha, beta, f, fctx, xd, fin, own, v, w, hp, words, mode);
            },
            [&](double *u, double *z) {      // y = y + u / d, or y = y + u; blocks / ILU: the sparse consumer's three launches
                if (pc_blocks) {
                    hipLaunchKernelGGL(k_gm_combine<0>, dim3(gv), dim3(kBlock), 0, st, N, G, d, u, words);
                    csc_factor_apply(pc, 0, u, z, words);
                    hipLaunchKernelGGL(k_gm_yadd, dim3(gv), dim3(kBlock), 0, st, N, V.y, (const double *)z, words);
                } else if (d) hipLaunchKernelGGL(k_gm_combine<1>, dim3(gv), dim3(kBlock), 0, st, N, G, d, V.y, words);
                else hipLaunchKernelGGL(k_gm_combine<2>, dim3(gv), dim3(kBlock), 0, st, N, G, d, V.y, words);
                return FD_OK;
            });
    };
    const int rc = run();
    if (rc != FD_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    hipLaunchKernelGGL(k_gm_final, dim3(cs_tiles(N, kBlock)), dim3(kBlock), 0, st, N, (const double *)V.y, (double *)y, S.d_words, G.klast, S.keep);
    FD_HIP_CHECK(hipGetLastError());
    S.solved = true;
    return FD_OK;
}

int fd_jfnk_solver_status(fd_jfnk_solver *s, int *flags, int64_t *iterations, double *resid, double *bnorm)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    int w[W_NWORDS];
    double sc[S_NSCAL];
    const int rc = s->S.read_status(s->ctx, w, sc);
    if (rc != FD_OK) return rc;
    if (flags) *flags = w[W_FINAL];
    if (iterations) *iterations = w[W_ITERS];
    if (resid) *resid = sc[S_GRES];
    if (bnorm) *bnorm = std::sqrt(sc[S_BNORM2]);
    return FD_OK;
}

int fd_jfnk_solver_counts(fd_jfnk_solver *s, int64_t *applications, int64_t *base_evaluations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    if (applications) *applications = s->applications;
    if (base_evaluations) *base_evaluations = s->base_evaluations;
    return FD_OK;
}

int fd_jfnk_solver_basis(fd_jfnk_solver *s, const void **V_dev, const void **H_dev, int *restart, int *last_cycle_len)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(s->S.solved, FD_ERR_UNSUPPORTED, "no solve has run on this solver");
    const CsGm G = gm_view(s->d_gm, (size_t)s->N, s->m);
    if (V_dev) *V_dev = G.V;
    if (H_dev) *H_dev = G.H;
    if (restart) *restart = s->m;
    if (last_cycle_len) {
        FD_HIP_CHECK(hipSetDevice(s->ctx->device));
        FD_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
        FD_HIP_CHECK(hipMemcpy(last_cycle_len, G.klast, sizeof(int), hipMemcpyDeviceToHost));
    }
    return FD_OK;
}

}  // extern "C"
