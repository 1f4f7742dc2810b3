// The SPARSE consumer ("sparse solve in the Newton/Rosenbrock step"): for a square J in SparseMatrixCSC storage,
// on the nzval a CSC plan has just written,
//     y = (alpha I + beta J) v,   y = (alpha I + beta J)^T v,   and   (alpha I + beta J) y = b   by Jacobi-preconditioned BiCGStab.
// DESIGN.md 4.9 has the contract; tests/csc_solve_model.py restates every summation order below in numpy and the GPU tests compare bits.
//
// CREATE is the shared builder's (fdjac_csc_pattern.hip), with the diagonal's slots and the pattern's reach.
//
// ORDERS.  (The product scaffold -- cs_gather_sum, k_cs_long, cs_tile_lines -- is fdjac_csc_common.h's, shared with the other consumers.)
// Row r of at most kCsLong entries: acc = 0; acc += nzval[slot_k] * v[col_k] for k ascending; y_r = alpha v_r + beta acc.
// A longer row is summed by ONE workgroup: thread t adds the entries k = t, t + 256, ... in that order, then block_sum().
// block_sum(): in every wavefront x += shfl_down(x, 32), 16, 8, 4, 2, 1; then ((w0 + w1) + w2) + w3.
// A dot over N elements: tiles of kCsVecTile (vector kernels: thread t adds elements t, t + 256, t + 512, t + 768 of its tile) or of 256
// (product kernels: element t), block_sum() per tile, and the LAST-ARRIVING workgroup (an integer ticket) adds the tiles' sums: thread t
// adds sums t, t + 256, ... in order, then block_sum().  No floating-point atomics; every order is a function of N alone.  All
// arithmetic is Float64 for either element type, and nothing is contracted into an FMA.
//
// BLOCK JACOBI (fd_csc_solver_set_preconditioner, kind 1).  M = diag(B_k), B_k = alpha I + beta J[rows of k, columns of k] over the
// uniform ranges [k bs, min((k + 1) bs, N)), bs in 2..32, applied on the right where p / d and s / d stand.  Once per solve
// k_cs_binv gathers every B_k from colptr / rowval / nzval into LDS beside an identity and inverts it by Gauss-Jordan with partial
// pivoting (one wavefront per block, lane l = column l of [B | I]).  Step j = 0 .. n - 1 of a block of n rows:
//   pivot row  best = j; for i = j + 1 .. n - 1: if |a_ij| > |a_best,j| then best = i   (strictly greater: the lowest row wins a tie;
//              a NaN never replaces and a NaN a_jj is never replaced);  piv = a_best,j; zero or not finite: breakdown (flag bit 1, done);
//   swap rows j and best;  every row i != j: f_i = a_ij / piv, a_il = a_il - f_i * a_jl (one multiply, one subtraction);  then row j:
//   a_jl = a_jl / piv.  (Two rows that are equal bit for bit therefore leave an exact zero row, and a zero pivot, behind.)
// Minv is kept as bs planes of N doubles: plane c holds column c of every block's inverse at its global row (a short last block
// leaves zeros in the planes it does not have).  k_cs_bapply: out_i = sum_c plane_c[i] * x[first row of i's block + c], c ascending
// from +0.0, one multiply and one add per term; the block's x values go through LDS.  The vector kernels then skip the division
// (their PC = 1 instances), so an iteration is 7 launches (+ 2 with long rows) instead of 5; kind 0 runs the PC = 0 instances, which
// are the code of before.  tests/csc_block_model.py restates all of it.
//
// BLOCK ILU(0) (fd_csc_solver_set_block_ilu).  The same uniform ranges with bs in 2..1024; M = diag(L_k U_k), the ILU(0) factors of
// B_k on its own stored pattern (the diagonal always part of it), applied on the right like the inverses above.  An in-block entry is
// a stored entry whose row and column lie in one block: a contiguous run of the row's sorted list.  The schedule (built on the host when
// the preconditioner is selected) holds per row the run's bounds and the diagonal's split, the levels lev_f (0 without an in-block lower
// entry, else 1 + the largest level of those entries' columns) and lev_b (likewise over the upper entries), and per block the rows by
// (level, row).  ONE workgroup owns one block; a barrier separates the levels; nothing waits on another workgroup.
//   factor (k_cs_ilu_factor, once per solve, behind k_cs_init<1>): row i, one lane, IKJ: w_j = beta nzval (off the diagonal), d = alpha +
//     beta nzval or alpha; for every in-block (i, k), k < i ascending: l = w_k / u_k, w_k = l; for every in-block (k, j) of row k, j > k
//     ascending, f its final value: j == i: d = d - l f; else if (i, j) is stored in-block: w_j = w_j - l f (one multiply, one
//     subtraction; anything else is dropped); u_i = d, zero or not finite: breakdown (flag bit 1, done), the arithmetic goes on.
//     lu (nnz doubles, indexed like the row lists): l at the lower positions, the final values at the upper ones, u_i at a stored
//     diagonal's, +0.0 outside the block; u (N doubles): the diagonal.  The order of the rows inside a level does not matter: a row
//     reads only rows of lower levels.
//   apply (k_cs_ilu_apply): the block's x in LDS; forward, levels ascending: t = x_i, t = t - l_ik z_k (k ascending), z_i = t; backward:
//     t = z_i, t = t - u_ij z_j (j ascending), z_i = t / u_i.
// An iteration is 7 launches (+ 2 with long rows) as with block Jacobi.  tests/csc_ilu_model.py restates all of it.
//
// GMRES (fd_csc_solver_set_method): restarted, right-preconditioned by any of the three above, beside BiCGStab on the same handle; its
// kernels and its orders are in fdjac_cscgmres.hip, included below; the host loop is csc_gmres_iterate() here.
#include "fdjac_internal.h"
#include "fdjac_device.h"
#include "fdjac_csc_common.h"
#include <cmath>
#include <vector>

namespace fdjac {

constexpr int kCsWinHalo = 1920;       // the LDS window of v (the tile's 256 rows + the reach on either side) is used up to this reach
constexpr int kCsBsMax = 32;           // the largest block of the block-Jacobi preconditioner
constexpr int kCsBinvWaves = 2;        // blocks (one wavefront each) per workgroup of k_cs_binv: 2 x (32 x 65 + 32) doubles = 33 KiB at bs = 32
constexpr int kCsIluBsMax = FD_CSC_ILU_BS_MAX;      // the largest block of block ILU(0): its x / z fill 8 KiB of LDS
constexpr int kCsPcIlu = 2;            // pc_kind of block ILU(0): the solver's own, fd_csc_solver_set_preconditioner does not take it
// scalars of a solve, in device memory: doubles ...
enum { S_RHO = 0, S_RHO_OLD, S_ALPHA, S_OMEGA, S_BNORM2, S_TOL2, S_RNORM2, S_SNORM2,      // (the words and the record: fdjac_csc_common.h)
       S_GAMMA2, S_GTOL, S_GRES, S_NSCAL };      // GMRES: ||r||^2 at a cycle's start, rtol ||b||, the last residual estimate
constexpr int W_GM_K = 6, W_GM_UPD = 7;          // GMRES: the cycle's completed columns; the columns its end adds to y (0: none)
static_assert(W_GM_UPD < W_NWORDS, "the words of a solve");

// ---- products --------------------------------------------------------------------------------------------------------------------------
// The long rows first (k_cs_long<false, CS_LONG_AXPBY>: y_r = alpha v_r + beta sum), then the rows.
// rows: a tile of 256 rows per workgroup, lane i takes row row_order[tile * 256 + i] (cs_tile_lines); when the pattern's reach is at most kCsWinHalo, v
// goes through an LDS window of the tile's rows and `reach` elements on either side (anything outside it is read from memory: the
// bits do not depend on the window); a wider pattern reads v from memory; the results cross LDS once so that y is
// written -- and the dots are summed -- in row order.  MODE 0: y only.  1: + dot(c, y) -> alpha (the first product of an
// iteration).  2: + dot(y, c), dot(y, y) -> omega (the second).  3, 4: y only, guarded like 2 and like 1 (GMRES: a step's product and
// the explicit residual's).
template <typename TV, int MODE>
__global__ void __launch_bounds__(kBlock) k_cs_rows(CsView P, double alpha, double beta, const real_t *__restrict__ nz, const TV *__restrict__ v,
                                                    TV *__restrict__ y, const double *__restrict__ c, double *scal, int *words, double *part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_out[kBlock];
    __shared__ double s_w[kBlock / 64];
    if (MODE != 0 && (cs_word(words, W_DONE) || ((MODE == 2 || MODE == 3) && cs_word(words, W_EARLY)))) return;
    TV *s_v = (TV *)s_raw;
    const int ntile = (P.N + kBlock - 1) / kBlock;
    const int tile = MODE == 0 ? (int)fd_xcd_block(blockIdx.x, ntile) : (int)blockIdx.x;
    if (tile >= ntile) return;
    const int r0 = tile * kBlock;
    int w0 = 0, w1 = 0;
    if (P.window) {
        const int h = P.reach;
        w0 = r0 - h > 0 ? r0 - h : 0;
        w1 = r0 + kBlock + h < P.N ? r0 + kBlock + h : P.N;
        for (int i = w0 + threadIdx.x; i < w1; i += kBlock) s_v[i - w0] = v[i];
        __syncthreads();
    }
    // (captures by value: that keeps the Float64 instances at 64 VGPRs)
    const auto vec = [=](int i) { return (i >= w0 && i < w1) ? (double)s_v[i - w0] : (double)v[i]; };
    cs_tile_lines<false, false>(P, r0, nz, y, nullptr, s_out, nullptr, vec, [=](int r, double acc) { return alpha * vec(r) + beta * acc; });
    const int row = r0 + threadIdx.x;
    double yr = 0.0;
    if (row < P.N) {
        yr = s_out[threadIdx.x];
        y[row] = (TV)yr;
    }
    if (MODE == 1) {
        double mine[1] = {row < P.N ? c[row] * yr : 0.0}, tot[1];
        if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
            if (cs_bad_pivot(tot[0])) cs_breakdown(words);
            else scal[S_ALPHA] = scal[S_RHO] / tot[0];
        }
    } else if (MODE == 2) {
        double mine[2] = {row < P.N ? yr * c[row] : 0.0, row < P.N ? yr * yr : 0.0}, tot[2];
        if (cs_finish<2>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
            if (cs_bad_pivot(tot[1])) cs_breakdown(words);
            else scal[S_OMEGA] = tot[0] / tot[1];
        }
    }
}

// the transposed product on the CSC arrays as they are: one lane per column, storage order
__global__ void __launch_bounds__(kBlock) k_cs_cols(CsView P, double alpha, double beta, const real_t *__restrict__ nz, const real_t *__restrict__ v,
                                                    real_t *__restrict__ y)
{
    const int nb = (P.N + kBlock - 1) / kBlock, b = (int)fd_xcd_block(blockIdx.x, nb);
    const int j = b * kBlock + threadIdx.x;
    if (b >= nb || j >= P.N) return;
    double acc = 0.0;
    for (int q = P.colptr[j]; q < P.colptr[j + 1]; ++q) acc += (double)nz[q] * (double)v[P.rowval[q]];
    y[j] = (real_t)(alpha * (double)v[j] + beta * acc);
}

// ---- BiCGStab ------------------------------------------------------------------------------------------------------------------------
struct CsVecs { double *r, *rhat, *p, *v, *s, *t, *ph, *sh, *y, *d; };

// the start: d = alpha + beta J_ii, r = rhat = b, p = v = y = 0, rho = ||b||^2  (PC = 1, block Jacobi: no d; k_cs_binv follows)
template <int PC>
__global__ void __launch_bounds__(kBlock) k_cs_init(CsView P, CsVecs V, double alpha, double beta, const real_t *__restrict__ nz,
                                                    const real_t *__restrict__ b, double rtol, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[1] = {0.0}, tot[1];
    bool bad = false;
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= P.N) continue;
        const double bi = (double)b[i];
        if (PC == 0) {
            const int q = P.diag[i];
            const double d = q >= 0 ? alpha + beta * (double)nz[q] : alpha;
            bad = bad || cs_bad_pivot(d);
            V.d[i] = d;
        }
        V.r[i] = bi; V.rhat[i] = bi; V.p[i] = 0.0; V.v[i] = 0.0; V.y[i] = 0.0;
        mine[0] += bi * bi;
    }
    if (bad) atomicOr(words + W_FLAGS, 2);
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[S_RHO] = tot[0]; scal[S_RHO_OLD] = 1.0; scal[S_ALPHA] = 1.0; scal[S_OMEGA] = 1.0;
        scal[S_BNORM2] = tot[0]; scal[S_RNORM2] = tot[0]; scal[S_SNORM2] = 0.0;
        scal[S_TOL2] = (rtol * rtol) * tot[0];
        int done = 0;
        if (tot[0] == 0.0) done = 1;                                              // b = 0: y = 0, no iteration
        else if (cs_word(words, W_FLAGS) & 2) done = 1;                           // a Jacobi diagonal that is zero or not finite
        else if (cs_bad_pivot(tot[0])) { atomicOr(words + W_FLAGS, 2); done = 1; }   // rho
        if (done) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// THE WARM START (fd_csc_solve_from_async with a y0): one launch in k_cs_init's place, on its grid.  A workgroup takes its tile of
// kCsVecTile elements as kCsVecTile / 256 sub-tiles of 256 rows: each sub-tile is a k_cs_rows tile (lane i takes row
// row_order[sub-tile + i], a row of at most kCsLong entries is summed there in ascending column, a longer one takes what k_cs_long left
// in wl; y0 is read from memory: the bits do not depend on a window), w = alpha y0 + beta acc stays Float64 and crosses LDS once into
// row order.  Thread t then holds elements t, t + 256, ... of the tile as in k_cs_init, so ||b||^2 and ||r0||^2 are dot_vec's sums:
// r0 = b - w (one subtraction), r = rhat = r0, p = v = 0, the accumulator y = (double)y0, d as in k_cs_init, and one cs_finish<2>.
// The last workgroup: S_BNORM2, S_TOL2 from ||b||^2; rho = ||r0||^2 (S_GAMMA2 too: k_gm_start<2> opens the first GMRES cycle on it).
// b = 0: done, and kCsYZero in the flags makes the final kernel write y = 0 whatever y0 holds.  Then a bad diagonal; ||b||^2 or
// ||r0||^2 not finite: breakdown (a NaN in y0 ends here); ||r0||^2 <= tol^2: done, 0 iterations, y = y0.
template <int PC>
__global__ void __launch_bounds__(kBlock) k_cs_init_from(CsView P, CsVecs V, double alpha, double beta, const real_t *__restrict__ nz,
                                                         const real_t *__restrict__ b, const real_t *__restrict__ y0, const double *wl,
                                                         double rtol, double *scal, int *words, double *part)
{
    __shared__ double s_out[kBlock];
    __shared__ double s_w[kBlock / 64];
    const int t0 = blockIdx.x * kCsVecTile;
    double mine[2] = {0.0, 0.0}, tot[2];
    bool bad = false;
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int r0 = t0 + k * kBlock;
        if (r0 >= P.N) break;                                                    // (the same in every thread: barriers below)
        cs_tile_lines<false, false>(P, r0, nz, wl, nullptr, s_out, nullptr, [=](int i) { return (double)y0[i]; },
                                    [=](int r, double acc) { return alpha * (double)y0[r] + beta * acc; });
        const int i = r0 + threadIdx.x;
        if (i < P.N) {
            const double bi = (double)b[i], ri = bi - s_out[threadIdx.x];
            if (PC == 0) {
                const int q = P.diag[i];
                const double d = q >= 0 ? alpha + beta * (double)nz[q] : alpha;
                bad = bad || cs_bad_pivot(d);
                V.d[i] = d;
            }
            V.r[i] = ri; V.rhat[i] = ri; V.p[i] = 0.0; V.v[i] = 0.0; V.y[i] = (double)y0[i];
            mine[0] += bi * bi;
            mine[1] += ri * ri;
        }
        __syncthreads();                                                         // s_out is the next sub-tile's
    }
    if (bad) atomicOr(words + W_FLAGS, 2);
    if (cs_finish<2>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        const bool zero = tot[0] == 0.0;                                          // b = 0: y = 0 and r = b
        const double rn2 = zero ? tot[0] : tot[1];
        scal[S_RHO] = rn2; scal[S_RHO_OLD] = 1.0; scal[S_ALPHA] = 1.0; scal[S_OMEGA] = 1.0;
        scal[S_BNORM2] = tot[0]; scal[S_RNORM2] = rn2; scal[S_SNORM2] = 0.0; scal[S_GAMMA2] = rn2;
        scal[S_TOL2] = (rtol * rtol) * tot[0];
        int done = 0;
        if (zero) { atomicOr(words + W_FLAGS, kCsYZero); done = 1; }
        else if (cs_word(words, W_FLAGS) & 2) done = 1;
        else if (cs_not_finite(tot[0]) || cs_not_finite(rn2)) { atomicOr(words + W_FLAGS, 2); done = 1; }
        else if (rn2 <= (rtol * rtol) * tot[0]) done = 1;                        // y0 is good enough: y = y0, no iteration
        if (done) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// fd_csc_solver_factor_async under the Jacobi preconditioner: d = alpha + beta J_ii as k_cs_init<0> forms it, into storage of the
// factorisation's own; a d_i that is zero or not finite: breakdown in the factorisation's words
__global__ void __launch_bounds__(kBlock) k_cs_fdiag(CsView P, double alpha, double beta, const real_t *__restrict__ nz, double *__restrict__ d,
                                                     int *words)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.N) return;
    const int q = P.diag[i];
    const double di = q >= 0 ? alpha + beta * (double)nz[q] : alpha;
    d[i] = di;
    if (cs_bad_pivot(di)) cs_breakdown(words);
}
// p = r + beta (p - omega v), ph = p / d  (PC = 1: ph is k_cs_bapply's)
template <int PC>
__global__ void __launch_bounds__(kBlock) k_cs_p(int N, CsVecs V, const double *scal, const int *words)
{
    if (cs_word(words, W_DONE)) return;
    const double bk = (scal[S_RHO] / scal[S_RHO_OLD]) * (scal[S_ALPHA] / scal[S_OMEGA]), om = scal[S_OMEGA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double p = V.r[i] + bk * (V.p[i] - om * V.v[i]);
        V.p[i] = p;
        if (PC == 0) V.ph[i] = p / V.d[i];
    }
}
// s = r - alpha v, sh = s / d, ||s||^2; ||s||^2 <= tol^2 ends the iteration early (W_EARLY)  (PC = 1: sh is k_cs_bapply's)
template <int PC>
__global__ void __launch_bounds__(kBlock) k_cs_s(int N, CsVecs V, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    if (cs_word(words, W_DONE)) return;
    const double al = scal[S_ALPHA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[1] = {0.0}, tot[1];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double s = V.r[i] - al * V.v[i];
        V.s[i] = s;
        if (PC == 0) V.sh[i] = s / V.d[i];
        mine[0] += s * s;
    }
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        scal[S_SNORM2] = tot[0];
        if (tot[0] <= scal[S_TOL2]) __hip_atomic_store(words + W_EARLY, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// y += alpha ph + omega sh, r = s - omega t, ||r||^2 and the next rho = rhat . r  (early: y += alpha ph, the residual is s)
__global__ void __launch_bounds__(kBlock) k_cs_update(int N, CsVecs V, double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    if (cs_word(words, W_DONE)) return;
    const int early = cs_word(words, W_EARLY);
    const double al = scal[S_ALPHA], om = scal[S_OMEGA];
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[2] = {0.0, 0.0}, tot[2];
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        if (early) {
            V.y[i] = V.y[i] + al * V.ph[i];
        } else {
            V.y[i] = (V.y[i] + al * V.ph[i]) + om * V.sh[i];
            const double r = V.s[i] - om * V.t[i];
            V.r[i] = r;
            mine[0] += r * r;
            mine[1] += V.rhat[i] * r;
        }
    }
    if (cs_finish<2>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        int done = 0;
        if (early) {
            scal[S_RNORM2] = scal[S_SNORM2];
            done = 1;
        } else {
            scal[S_RNORM2] = tot[0];
            if (tot[0] <= scal[S_TOL2]) done = 1;
            else {
                scal[S_RHO_OLD] = scal[S_RHO];
                scal[S_RHO] = tot[1];
                if (cs_bad_pivot(tot[1])) { atomicOr(words + W_FLAGS, 2); done = 1; }
            }
        }
        words[W_ITERS] = words[W_ITERS] + 1;
        if (done) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// ---- block Jacobi ----------------------------------------------------------------------------------------------------------------------
// gather and invert: wavefront w of the workgroup takes block blockIdx.x * kCsBinvWaves + w; its tile is bs rows of [B | I] with a row
// stride of 2 bs + 1 doubles (odd: a column read does not stay in one bank); lane l < bs owns column l of B, lane bs + c column c of
// the companion; lane i < n also forms row i's factor f_i of every step.  A lane writes only its own column and column j is dead from
// step j on (it is neither swapped nor updated: nothing reads it again), so a step needs two barriers: behind the factors and behind the
// update.  Every loop runs to bs and every barrier is met by all threads whatever the block's length n (0: a wavefront without a block).
__global__ void __launch_bounds__(kCsBinvWaves * 64) k_cs_binv(CsView P, int bs, double alpha, double beta, const real_t *__restrict__ nz,
                                                                double *__restrict__ minv, int *words)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int ld = 2 * bs + 1, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double *a = (double *)s_raw + (size_t)w * (bs * ld + bs), *f = a + bs * ld;
    const int nblk = (P.N + bs - 1) / bs, blk = blockIdx.x * kCsBinvWaves + w;
    const int b0 = blk < nblk ? blk * bs : 0;
    const int n = blk < nblk ? (P.N - b0 < bs ? P.N - b0 : bs) : 0;
    const bool col_b = lane < n, col_i = lane >= bs && lane - bs < n;       // this lane's column exists
    if (lane < 2 * bs)
        for (int i = 0; i < bs; ++i) a[i * ld + lane] = lane == bs + i ? 1.0 : 0.0;
    if (col_b) {
        const int col = b0 + lane;
        a[lane * ld + lane] = alpha;                                        // a diagonal that is not stored
        for (int q = P.colptr[col]; q < P.colptr[col + 1]; ++q) {
            const int r = P.rowval[q];
            if (r >= b0 + n) break;                                         // (rows ascend within a column)
            if (r >= b0) a[(r - b0) * ld + lane] = r == col ? alpha + beta * (double)nz[q] : beta * (double)nz[q];
        }
    }
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < bs; ++j) {
        const bool step = j < n;
        int best = j;
        double piv = 1.0;
        if (step) {
            double mag = fabs(a[j * ld + j]);
            for (int i = j + 1; i < n; ++i) {
                const double m = fabs(a[i * ld + j]);
                if (m > mag) { mag = m; best = i; }
            }
            piv = a[best * ld + j];
            bad = bad || cs_bad_pivot(piv);
            if (lane < n) f[lane] = a[(lane == j ? best : (lane == best ? j : lane)) * ld + j] / piv;      // row `lane` after the swap
        }
        __syncthreads();
        if (step && ((col_b && lane > j) || col_i)) {
            const double t = a[best * ld + lane];
            a[best * ld + lane] = a[j * ld + lane];
            for (int i = 0; i < n; ++i)
                if (i != j) a[i * ld + lane] = a[i * ld + lane] - f[i] * t;
            a[j * ld + lane] = t / piv;
        }
        __syncthreads();
    }
    if (bad && lane == 0) cs_breakdown(words);      // (every lane of the wavefront has seen the same pivots)
    if (col_b)      // lane i writes row i of the inverse, plane by plane: n consecutive doubles per plane
        for (int c = 0; c < bs; ++c) minv[(size_t)c * P.N + b0 + lane] = c < n ? a[lane * ld + bs + c] : 0.0;
}
// out = Minv x on a tile of kCsVecTile elements; the blocks that reach into the tile are staged whole in LDS
template <int WHICH>      // 0: ph from p; 1: sh from s (not needed once the half step has converged)
__global__ void __launch_bounds__(kBlock) k_cs_bapply(int N, int bs, const double *__restrict__ minv, const double *__restrict__ x,
                                                      double *__restrict__ out, const int *words)
{
    __shared__ double s_x[kCsVecTile + 2 * (kCsBsMax - 1)];
    if (cs_word(words, W_DONE) || (WHICH == 1 && cs_word(words, W_EARLY))) return;
    const int t0 = blockIdx.x * kCsVecTile, t1 = t0 + kCsVecTile < N ? t0 + kCsVecTile : N;
    const int w0 = t0 / bs * bs;
    int w1 = (t1 + bs - 1) / bs * bs;
    if (w1 > N) w1 = N;
    for (int i = w0 + threadIdx.x; i < w1; i += kBlock) s_x[i - w0] = x[i];
    __syncthreads();
    // the offset of element i in its block: ONE division per lane (of a number below kBlock + bs); the next element of the lane is
    // kBlock further on, so its offset follows from kBlock % bs (the same for every lane) by an addition and a compare
    const int step = kBlock % bs;
    int off = (t0 - w0 + (int)threadIdx.x) % bs;
#pragma unroll
    for (int k = 0; k < kCsVecTile / kBlock; ++k, off = off + step >= bs ? off + step - bs : off + step) {
        const int i = t0 + threadIdx.x + k * kBlock;
        if (i >= N) continue;
        const int b0 = i - off, n = N - b0 < bs ? N - b0 : bs;
        const double *m = minv + i, *xb = s_x + (b0 - w0);
        double acc = 0.0;
#pragma unroll 8
        for (int c = 0; c < n; ++c) acc += m[(size_t)c * N] * xb[c];
        out[i] = acc;
    }
}
// ---- block ILU(0) ------------------------------------------------------------------------------------------------------------------------
struct CsIlu {                         // the schedule as the kernels see it (device, Int32)
    int bs;
    const int4 *run;                   // per row, positions in the row lists: the first in-block entry, the first with column >= row,
                                       // the first with column > row, the end of the in-block run
    const int *ord_f, *ord_b;          // block k's rows by (level, row) at [k bs, k bs + n)
    const int *off_f, *off_b;          // block k at k (bs + 1): level L's rows are ord[k bs + off[L] .. k bs + off[L + 1])
    const int *nlev_f, *nlev_b;        // levels per block
};
// factor: one workgroup per block, level by level (the forward levels: row i reads the rows k of its in-block lower entries), thread t
// takes rows t, t + 256, ... of the level, one lane per row.  lu and u are written and read by the same workgroup across its barriers:
// plain pointers, so that every read is a vector load behind the barrier's fence.
__global__ void __launch_bounds__(kBlock) k_cs_ilu_factor(CsView P, CsIlu I, double alpha, double beta, const real_t *__restrict__ nz,
                                                          double *lu, double *u, int *words)
{
    const int b0 = blockIdx.x * I.bs, nlev = I.nlev_f[blockIdx.x];
    const int *off = I.off_f + (size_t)blockIdx.x * (I.bs + 1);
    bool bad = false;
    for (int L = 0; L < nlev; ++L) {
        for (int t = off[L] + threadIdx.x; t < off[L + 1]; t += kBlock) {
            const int i = I.ord_f[b0 + t];
            const int4 r = I.run[i];
            const bool stored = r.z > r.y;                                    // the diagonal has a slot
            double d = alpha;
            for (int p = r.x; p < r.w; ++p) {
                const double w = beta * (double)nz[P.row_slot[p]];
                if (stored && p == r.y) d = alpha + w;
                else lu[p] = w;
            }
            for (int p = r.x; p < r.y; ++p) {
                const int k = P.row_col[p];
                const double l = lu[p] / u[k];
                lu[p] = l;
                const int4 rk = I.run[k];
                int pi = p + 1;                                               // row i's entry that (k, j) may meet: both lists ascend
                for (int q = rk.z; q < rk.w; ++q) {
                    const int j = P.row_col[q];
                    const double f = lu[q];
                    if (j == i) { d = d - l * f; continue; }
                    while (pi < r.w && P.row_col[pi] < j) ++pi;
                    if (pi < r.w && P.row_col[pi] == j) lu[pi] = lu[pi] - l * f;
                }
            }
            u[i] = d;
            if (stored) lu[r.y] = d;
            bad = bad || cs_bad_pivot(d);
        }
        __syncthreads();
    }
    if (bad) cs_breakdown(words);
}
// z = (L U)^-1 x per block: x through LDS, the forward levels (level 0 has nothing to subtract), the backward levels, then out
template <int WHICH>      // 0: ph from p; 1: sh from s (not needed once the half step has converged)
__global__ void __launch_bounds__(kBlock) k_cs_ilu_apply(CsView P, CsIlu I, const double *__restrict__ lu, const double *__restrict__ u,
                                                         const double *__restrict__ x, double *__restrict__ out, const int *words)
{
    __shared__ double s_z[kCsIluBsMax];
    if (cs_word(words, W_DONE) || (WHICH == 1 && cs_word(words, W_EARLY))) return;
    const int b0 = blockIdx.x * I.bs, n = P.N - b0 < I.bs ? P.N - b0 : I.bs;
    for (int t = threadIdx.x; t < n; t += kBlock) s_z[t] = x[b0 + t];
    __syncthreads();
    const int *off = I.off_f + (size_t)blockIdx.x * (I.bs + 1);
    int nlev = I.nlev_f[blockIdx.x];
    for (int L = 1; L < nlev; ++L) {
        for (int t = off[L] + threadIdx.x; t < off[L + 1]; t += kBlock) {
            const int i = I.ord_f[b0 + t];
            const int4 r = I.run[i];
            double acc = s_z[i - b0];
            for (int p = r.x; p < r.y; ++p) acc = acc - lu[p] * s_z[P.row_col[p] - b0];
            s_z[i - b0] = acc;
        }
        __syncthreads();
    }
    off = I.off_b + (size_t)blockIdx.x * (I.bs + 1);
    nlev = I.nlev_b[blockIdx.x];
    for (int L = 0; L < nlev; ++L) {
        for (int t = off[L] + threadIdx.x; t < off[L + 1]; t += kBlock) {
            const int i = I.ord_b[b0 + t];
            const int4 r = I.run[i];
            double acc = s_z[i - b0];
            for (int p = r.z; p < r.w; ++p) acc = acc - lu[p] * s_z[P.row_col[p] - b0];
            s_z[i - b0] = acc / u[i];
        }
        __syncthreads();
    }
    for (int t = threadIdx.x; t < n; t += kBlock) out[b0 + t] = s_z[t];
}
// the end: bit 0 when the iterations ran out; y, or NaN after a failure unless the caller keeps the last iterate (kCsYZero: a warm start
// found b = 0, the iterate is 0 and not the accumulator).  THE ONLY KERNEL OF A SOLVE THAT WRITES y: y0 may be y, y0 and y may be b.
__global__ void __launch_bounds__(kBlock) k_cs_final(int N, const double *__restrict__ yacc, real_t *__restrict__ y, int *words, int keep)
{
    const int f = cs_word(words, W_FLAGS);
    const int flags = (f & 2) | (cs_word(words, W_DONE) ? 0 : 1);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) words[W_FINAL] = flags;
    if (i >= N) return;
    y[i] = (real_t)((flags && !keep) ? __longlong_as_double(0x7FF8000000000000ll) : ((f & kCsYZero) ? 0.0 : yacc[i]));
}

}  // namespace fdjac

#include "fdjac_cscgmres.hip"

struct fd_csc_solver : fdjac::CscHandle {      // d_vec: ten vectors of N doubles
    int window = 1;
    int pc_kind = FD_CSC_PRECOND_JACOBI, pc_bs = 0;      // what the next solve uses
    double *d_minv = nullptr;          // block Jacobi: minv_bs planes of N doubles (allocated by the first solve that needs them)
    size_t minv_cap = 0;               // doubles allocated
    int minv_bs = 0;                   // the block size of the last block-Jacobi solve, 0: none yet
    // block ILU(0): the schedule of block size ilu_bs (0: none built) and the factor lu (nnz doubles) | u (N doubles)
    int ilu_bs = 0, ilu_max_f = 0, ilu_max_b = 0;
    bool ilu_factored = false;         // a block-ILU solve has run on this schedule
    int *d_ilu_int = nullptr;          // run (4 N) | lev_f | lev_b | ord_f | ord_b (N each) | off_f | off_b (nblk (bs + 1) each) | nlev_f | nlev_b (nblk each)
    double *d_ilu = nullptr;
    // GMRES (fd_csc_solver_set_method): what the next solve uses, and the buffers of the last GMRES solve (fdjac_cscgmres.hip: CsGm)
    int method = FD_CSC_METHOD_BICGSTAB, gm_restart = 30;
    double *d_gm = nullptr;
    size_t gm_cap = 0;                 // doubles allocated
    int gm_m = 0;                      // the restart of the last GMRES solve, 0: none yet
    bool last_gmres = false;           // the last solve was a GMRES solve: its status reads the estimate
    // the factorisation as an operation of its own (fd_csc_solver_factor_async / _apply_async; the matrix-free consumer borrows it):
    // `gen` counts what invalidates one -- a solve, a preconditioner setter, another factor -- and fact_gen is its value at the last
    // factor (0: none), so the factorisation stands while the two are equal
    int elem_bytes = (int)sizeof(FDJAC_REAL);    // which element build made the handle (fd_jfnk_solver_set_csc_preconditioner asks)
    uint64_t gen = 0, fact_gen = 0;
    int fact_kind = FD_CSC_PRECOND_JACOBI, fact_bs = 0;      // what the last factor built
    double *d_fdiag = nullptr;         // Jacobi: the N diagonals of the last factor (V.d is a solve's)
    int *d_fwords = nullptr;           // 2 W_NWORDS: the factorisation's words (flags bit 1, done), then a block that stays zero
    ~fd_csc_solver()
    {
        if (d_fdiag) (void)hipFree(d_fdiag);
        if (d_fwords) (void)hipFree(d_fwords);
        if (d_gm) (void)hipFree(d_gm);
        if (d_minv) (void)hipFree(d_minv);
        if (d_ilu_int) (void)hipFree(d_ilu_int);
        if (d_ilu) (void)hipFree(d_ilu);
    }
};

using namespace fdjac;

static size_t csc_win_bytes(const fd_csc_solver *s, size_t elem)
{
    if (!s->window) return 0;
    return (size_t)(kBlock + 2 * s->L.reach) * elem;
}

int fd_csc_solver_create(fd_ctx *ctx, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base, int idx_kind,
                         fd_csc_solver **out)
{
    return csc_handle_create(out, [&](fd_csc_solver *s) -> int {
        const int rc = s->init(ctx, "csc solver", N, N, colptr, rowval, idx_bytes, idx_base, idx_kind, CSC_WANT_DIAG, 10 * (size_t)N, S_NSCAL,
                               2 * (int64_t)cs_tiles(N, kBlock));
        if (rc != FD_OK) return rc;
        if (const char *v = test_switch("FDJAC_CSC_WINDOW")) s->window = atoi(v) != 0;
        // the LDS window of v only when the measured reach allows it: every column a tile's rows can name then lies inside the window;
        // a wider pattern would stage 2 * kCsWinHalo elements per tile to serve the near-diagonal gathers alone
        if (s->L.reach > kCsWinHalo) s->window = 0;
        return FD_OK;
    });
}

int fd_csc_solver_destroy(fd_csc_solver *s) { return csc_handle_destroy(s); }

int fd_csc_solver_set_options(fd_csc_solver *s, double rtol, int max_iterations)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    return s->S.set_options(rtol, max_iterations);
}

int fd_csc_solver_set_policy(fd_csc_solver *s, int keep_unconverged)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    return s->S.set_policy(keep_unconverged);
}

int fd_csc_solver_set_preconditioner(fd_csc_solver *s, int kind, int block_size)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(kind == FD_CSC_PRECOND_JACOBI || kind == FD_CSC_PRECOND_BLOCK_JACOBI, FD_ERR_ARG, "kind = %d (0: Jacobi, 1: block Jacobi)", kind);
    if (kind == FD_CSC_PRECOND_BLOCK_JACOBI)
        FD_REQUIRE(block_size >= 2 && block_size <= kCsBsMax, FD_ERR_ARG, "block_size = %d (2 .. %d)", block_size, kCsBsMax);
    s->pc_kind = kind;
    s->pc_bs = kind == FD_CSC_PRECOND_BLOCK_JACOBI ? block_size : 0;
    s->gen += 1;
    return FD_OK;
}

int fd_csc_solver_set_method(fd_csc_solver *s, int method, int restart)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(method == FD_CSC_METHOD_BICGSTAB || method == FD_CSC_METHOD_GMRES, FD_ERR_ARG, "method = %d (0: BiCGStab, 1: GMRES)", method);
    if (method == FD_CSC_METHOD_GMRES) {
        FD_REQUIRE(restart >= 1 && restart <= kGmMax, FD_ERR_ARG, "restart = %d (1 .. %d)", restart, kGmMax);
        s->gm_restart = restart;
    }
    s->method = method;
    return FD_OK;
}

// the buffers of a GMRES solve with restart m in d_gm (CsGm's arrays in its order, then the partial sums and one slot for klast)
static size_t gm_doubles(size_t N, int m, size_t ntile)
{
    const size_t k = (size_t)m;
    return (k + 1) * N + 2 * k * (k + 1) + 2 * k + (k + 1) + k + 2 * (k + 1) + (k + 2) * ntile + 1;
}
static CsGm gm_view(double *p, size_t N, int m)
{
    const size_t k = (size_t)m, ntile = cs_tiles((int64_t)N, kCsVecTile);
    CsGm G;
    G.m = m; G.ntile = (int)ntile;
    G.V = p; p += (k + 1) * N;
    G.H = p; p += k * (k + 1);
    G.R = p; p += k * (k + 1);
    G.c = p; p += k;
    G.s = p; p += k;
    G.g = p; p += k + 1;
    G.t = p; p += k;
    G.h1 = p; p += k + 1;
    G.h2 = p; p += k + 1;
    G.part = p; p += (k + 2) * ntile;
    G.klast = (int *)p;
    return G;
}
static CsGm csc_gm(const fd_csc_solver *s, int m) { return gm_view(s->d_gm, (size_t)s->L.N, m); }

// the basis and the Hessenberg columns of the last cycle of the last GMRES solve, for the tests: owned by the solver; synchronises
int fd_csc_solver_gmres_basis(fd_csc_solver *s, const void **V_dev, const void **H_dev, int *restart, int *last_cycle_len)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(s->gm_m > 0, FD_ERR_UNSUPPORTED, "no GMRES solve has run on this solver");
    const CsGm G = csc_gm(s, s->gm_m);
    if (V_dev) *V_dev = G.V;
    if (H_dev) *H_dev = G.H;
    if (restart) *restart = s->gm_m;
    if (last_cycle_len) {
        FD_HIP_CHECK(hipSetDevice(s->ctx->device));
        FD_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
        FD_HIP_CHECK(hipMemcpy(last_cycle_len, G.klast, sizeof(int), hipMemcpyDeviceToHost));
    }
    return FD_OK;
}

// the inverses of the last block-Jacobi solve, for the tests: block_size planes of N doubles, owned by the solver
int fd_csc_solver_block_inverses(fd_csc_solver *s, const void **inv_dev, int64_t *nblocks, int *block_size)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(s->minv_bs > 0, FD_ERR_UNSUPPORTED, "no block-Jacobi solve has run on this solver");
    if (inv_dev) *inv_dev = s->d_minv;
    if (nblocks) *nblocks = (s->L.N + s->minv_bs - 1) / s->minv_bs;
    if (block_size) *block_size = s->minv_bs;
    return FD_OK;
}

// ---- block ILU(0): the schedule, on the host from the solver's row lists (not on the hot path) ------------------------------------
static size_t ilu_nblk(const fd_csc_solver *s, int bs) { return (size_t)((s->L.N + bs - 1) / bs); }
static size_t ilu_ints(const fd_csc_solver *s, int bs) { return 8 * (size_t)s->L.N + 2 * ilu_nblk(s, bs) * (size_t)(bs + 1) + 2 * ilu_nblk(s, bs); }
static CsIlu csc_ilu(const fd_csc_solver *s)
{
    const size_t N = (size_t)s->L.N, nblk = ilu_nblk(s, s->ilu_bs), no = nblk * (size_t)(s->ilu_bs + 1);
    const int *p = s->d_ilu_int;
    CsIlu I;
    I.bs = s->ilu_bs;
    I.run = (const int4 *)p;
    I.ord_f = p + 6 * N; I.ord_b = p + 7 * N;
    I.off_f = p + 8 * N; I.off_b = p + 8 * N + no;
    I.nlev_f = p + 8 * N + 2 * no; I.nlev_b = p + 8 * N + 2 * no + nblk;
    return I;
}
static int ilu_build(fd_csc_solver *s, int bs)
{
    const size_t N = (size_t)s->L.N, nnz = (size_t)s->L.nnz, nblk = ilu_nblk(s, bs), no = nblk * (size_t)(bs + 1);
    std::vector<int> row_ptr(N + 1), row_col(nnz), h(ilu_ints(s, bs), 0);
    FD_HIP_CHECK(hipMemcpy(row_ptr.data(), s->L.row_ptr, sizeof(int) * (N + 1), hipMemcpyDeviceToHost));
    if (nnz) FD_HIP_CHECK(hipMemcpy(row_col.data(), s->L.row_col, sizeof(int) * nnz, hipMemcpyDeviceToHost));
    int *run = h.data(), *lev_f = run + 4 * N, *lev_b = run + 5 * N, *ord_f = run + 6 * N, *ord_b = run + 7 * N;
    int *off_f = run + 8 * N, *off_b = off_f + no, *nlev_f = off_b + no, *nlev_b = nlev_f + nblk;
    for (size_t i = 0; i < N; ++i) {        // the run of row i and the diagonal's split
        const int b0 = (int)(i / bs) * bs, b1 = b0 + bs;
        int p = row_ptr[i];
        const int e = row_ptr[i + 1];
        while (p < e && row_col[p] < b0) ++p;
        run[4 * i] = p;
        while (p < e && row_col[p] < (int)i) ++p;
        run[4 * i + 1] = p;
        if (p < e && row_col[p] == (int)i) ++p;
        run[4 * i + 2] = p;
        while (p < e && row_col[p] < b1) ++p;
        run[4 * i + 3] = p;
    }
    int max_f = 0, max_b = 0;
    for (size_t i = 0; i < N; ++i) {
        int lev = 0;
        for (int p = run[4 * i]; p < run[4 * i + 1]; ++p) lev = lev > lev_f[row_col[p]] + 1 ? lev : lev_f[row_col[p]] + 1;
        lev_f[i] = lev;
        max_f = max_f > lev ? max_f : lev;
    }
    for (size_t i = N; i-- > 0;) {
        int lev = 0;
        for (int p = run[4 * i + 2]; p < run[4 * i + 3]; ++p) lev = lev > lev_b[row_col[p]] + 1 ? lev : lev_b[row_col[p]] + 1;
        lev_b[i] = lev;
        max_b = max_b > lev ? max_b : lev;
    }
    for (int dir = 0; dir < 2; ++dir) {     // per block a counting sort by level: the rows of a level stay ascending
        const int *lev = dir ? lev_b : lev_f;
        int *ord = dir ? ord_b : ord_f, *off = dir ? off_b : off_f, *nlev = dir ? nlev_b : nlev_f;
        for (size_t k = 0; k < nblk; ++k) {
            const size_t b0 = k * (size_t)bs, n = N - b0 < (size_t)bs ? N - b0 : (size_t)bs;
            int *o = off + k * (size_t)(bs + 1), nl = 0;
            for (size_t i = b0; i < b0 + n; ++i) { ++o[lev[i] + 1]; nl = nl > lev[i] + 1 ? nl : lev[i] + 1; }      // (a level is below n)
            for (int L = 0; L < nl; ++L) o[L + 1] += o[L];
            std::vector<int> cur(o, o + nl);
            for (size_t i = b0; i < b0 + n; ++i) ord[b0 + cur[lev[i]]++] = (int)i;
            nlev[k] = nl;
        }
    }
    if (s->d_ilu_int) (void)hipFree(s->d_ilu_int);
    if (s->d_ilu) (void)hipFree(s->d_ilu);
    s->d_ilu_int = nullptr; s->d_ilu = nullptr; s->ilu_bs = 0; s->ilu_factored = false;
    const char *who = "block ILU";
    CSC_TRY(who, hipMalloc((void **)&s->d_ilu_int, sizeof(int) * h.size()));
    CSC_TRY(who, hipMalloc((void **)&s->d_ilu, sizeof(double) * (nnz + N)));
    CSC_TRY(who, hipMemcpy(s->d_ilu_int, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
    CSC_TRY(who, hipMemset(s->d_ilu, 0, sizeof(double) * (nnz + N)));      // +0.0 at every position outside a block: no kernel writes there
    CSC_TRY(who, hipDeviceSynchronize());
    s->ilu_bs = bs; s->ilu_max_f = max_f; s->ilu_max_b = max_b;
    return FD_OK;
}

int fd_csc_solver_set_block_ilu(fd_csc_solver *s, int block_size)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(block_size >= 2 && block_size <= kCsIluBsMax, FD_ERR_ARG, "block_size = %d (2 .. %d)", block_size, kCsIluBsMax);
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    FD_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
    s->gen += 1;
    if (s->ilu_bs != block_size) {
        const int rc = ilu_build(s, block_size);
        if (rc != FD_OK) {               // the preconditioner of before stays selected; block ILU of another size has lost its schedule
            if (s->pc_kind == kCsPcIlu) { s->pc_kind = FD_CSC_PRECOND_JACOBI; s->pc_bs = 0; }
            return rc;
        }
    }
    s->pc_kind = kCsPcIlu;
    s->pc_bs = block_size;
    return FD_OK;
}

// the levels of the schedule, for the tests: N Int32 each, owned by the solver
int fd_csc_solver_ilu_levels(fd_csc_solver *s, const void **lev_fwd_dev, const void **lev_bwd_dev, int *max_fwd, int *max_bwd)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(s->ilu_bs > 0, FD_ERR_UNSUPPORTED, "block ILU is not set on this solver");
    if (lev_fwd_dev) *lev_fwd_dev = s->d_ilu_int + 4 * (size_t)s->L.N;
    if (lev_bwd_dev) *lev_bwd_dev = s->d_ilu_int + 5 * (size_t)s->L.N;
    if (max_fwd) *max_fwd = s->ilu_max_f;
    if (max_bwd) *max_bwd = s->ilu_max_b;
    return FD_OK;
}

// the factors of the last block-ILU solve, for the tests: lu (nnz doubles, indexed like the row lists) and u (N doubles)
int fd_csc_solver_ilu_factors(fd_csc_solver *s, const void **lu_dev, const void **u_dev, int64_t *nblocks, int *block_size)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(s->ilu_bs > 0 && s->ilu_factored, FD_ERR_UNSUPPORTED, "no block-ILU solve has run on this solver");
    if (lu_dev) *lu_dev = s->d_ilu;
    if (u_dev) *u_dev = s->d_ilu + (size_t)s->L.nnz;
    if (nblocks) *nblocks = (int64_t)ilu_nblk(s, s->ilu_bs);
    if (block_size) *block_size = s->ilu_bs;
    return FD_OK;
}

// the solver's lists, for the tests and for callers that want the pattern by rows: device pointers that live as long as the solver
int fd_csc_solver_row_lists(fd_csc_solver *s, const void **row_ptr, const void **row_col, const void **row_slot, const void **diag_slot,
                            int64_t *nnz_out, int64_t *long_rows_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    if (row_ptr) *row_ptr = s->L.row_ptr;
    if (row_col) *row_col = s->L.row_col;
    if (row_slot) *row_slot = s->L.row_slot;
    if (diag_slot) *diag_slot = s->L.diag;
    if (nnz_out) *nnz_out = s->L.nnz;
    if (long_rows_out) *long_rows_out = s->L.nlong_r;
    return FD_OK;
}

// bs planes of N doubles in d_minv: allocated by the first solve or factor that needs them, grown when a larger block size comes
static int csc_minv_reserve(fd_csc_solver *s, int bs)
{
    const size_t n = (size_t)s->L.N;
    if (s->minv_cap >= (size_t)bs * n) return FD_OK;
    FD_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
    if (s->d_minv) (void)hipFree(s->d_minv);
    s->d_minv = nullptr; s->minv_cap = 0; s->minv_bs = 0;
    const hipError_t e = hipMalloc((void **)&s->d_minv, sizeof(double) * (size_t)bs * n);
    if (e != hipSuccess) { (void)hipGetLastError(); FD_REQUIRE(false, FD_ERR_NOMEM, "block Jacobi: %d planes of %d doubles: %s", bs, (int)n, hipGetErrorString(e)); }
    s->minv_cap = (size_t)bs * n;
    return FD_OK;
}
static void csc_binv_launch(fd_csc_solver *s, int bs, double alpha, double beta, const real_t *nz, int *words)
{
    hipLaunchKernelGGL(k_cs_binv, dim3(cs_tiles(cs_tiles(s->L.N, bs), kCsBinvWaves)), dim3(kCsBinvWaves * 64),
                       sizeof(double) * (size_t)kCsBinvWaves * (size_t)(bs * (2 * bs + 1) + bs), s->ctx->stream, cs_view(s->L, s->window), bs, alpha, beta, nz,
                       s->d_minv, words);
    s->minv_bs = bs;
}
static void csc_ilu_factor_launch(fd_csc_solver *s, double alpha, double beta, const real_t *nz, int *words)
{
    hipLaunchKernelGGL(k_cs_ilu_factor, dim3((unsigned)ilu_nblk(s, s->ilu_bs)), dim3(kBlock), 0, s->ctx->stream, cs_view(s->L, s->window), csc_ilu(s), alpha, beta,
                       nz, s->d_ilu, s->d_ilu + (size_t)s->L.nnz, words);
    s->ilu_factored = true;
}

template <typename TV, int MODE>
static void csc_product(fd_csc_solver *s, double alpha, double beta, const real_t *nz, const TV *v, TV *y, const double *c, bool guarded)
{
    hipStream_t st = s->ctx->stream;
    const CsView P = cs_view(s->L, s->window);
    const unsigned ntile = cs_tiles(s->L.N, kBlock);
    cs_launch_long<false, CS_LONG_AXPBY>(st, P, nz, v, y, guarded ? s->S.d_words : nullptr, alpha, beta);
    hipLaunchKernelGGL((k_cs_rows<TV, MODE>), dim3(MODE == 0 ? fd_xcd_grid(ntile) : ntile), dim3(kBlock), csc_win_bytes(s, sizeof(TV)), st, P, alpha, beta,
                       nz, v, y, c, s->S.d_scal, s->S.d_words, s->S.d_part);
}

int fd_csc_matvec_async(fd_csc_solver *s, double alpha, double beta, const void *nzval, const void *v, void *y, int transpose)
{
    FD_REQUIRE(s && v && y && (nzval || s->L.nnz == 0), FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(v != y, FD_ERR_ARG, "y must not be v");
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    if (transpose) {
        hipLaunchKernelGGL(k_cs_cols, dim3(fd_xcd_grid(cs_tiles(s->L.N, kBlock))), dim3(kBlock), 0, s->ctx->stream, cs_view(s->L, s->window), alpha, beta,
                           (const real_t *)nzval, (const real_t *)v, (real_t *)y);
    } else {
        csc_product<real_t, 0>(s, alpha, beta, (const real_t *)nzval, (const real_t *)v, (real_t *)y, nullptr, false);
    }
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

// The GMRES iterations behind the start kernels (fdjac_cscgmres.hip has the algorithm), shared by the sparse consumer and the
// matrix-free one (fdjac_jfnk.hip).  Each callable enqueues on st and returns FD_OK or the code that ends the call:
//   precond(vj, z)      the step's z = M^-1 v_j; returns where z is (vj itself without a preconditioner); guarded by `cycle over`
//   product(mode, v, w) w = A v; mode 3: a step's product (nothing once the cycle is over), 4: the explicit residual's (once the solve is)
//   add(u, z)           the cycle's end behind k_gm_tri: y = y + M^-1 (V t) over the columns W_GM_UPD counts
template <class PC, class PR, class AD>
static int csc_gmres_iterate(hipStream_t st, CscSolveState &S, int N, const CsGm &G, const real_t *b, const CsVecs &V, bool warm, PC precond, PR product,
                             AD add)
{
    const int m = G.m;
    const size_t n = (size_t)N;
    const unsigned gv = cs_tiles(N, kCsVecTile);
    double *z = V.p, *w = V.v, *u = V.s, *npart = G.part + (size_t)(m + 1) * G.ntile;
    int *words = S.d_words;
    int rc = FD_OK;
    // the first cycle: on r = b, or (warm: a y0 was given) on the r0 = b - A y0 and the ||r0||^2 that the warm start left
    hipLaunchKernelGGL(warm ? k_gm_start<2> : k_gm_start<1>, dim3(gv), dim3(kBlock), 0, st, N, (const double *)V.r, G, S.rtol, S.d_scal, (const int *)words);
    const auto step = [&](int j) {      // the sparse consumer: 10 launches (+ 1 with long rows)
        const double *vj = G.V + (size_t)j * n, *zj = nullptr;
        if ((rc = precond(vj, z, &zj)) != FD_OK) return;
        if ((rc = product(3, zj, w)) != FD_OK) return;
        for (int pass = 0; pass < 2; ++pass) {
            double *h = pass ? G.h2 : G.h1;
            hipLaunchKernelGGL(k_cs_gs_dots, dim3(gv), dim3(kBlock), 0, st, N, j + 1, (const double *)w, (const double *)G.V, G.part, (const int *)words);
            hipLaunchKernelGGL(k_cs_gs_reduce, dim3(j + 1), dim3(kBlock), 0, st, G.ntile, (const double *)G.part, h, (const int *)words);
            fd_pick<false, true>(pass == 1, [&](auto NORM) {
                hipLaunchKernelGGL(k_cs_gs_update<NORM()>, dim3(gv), dim3(kBlock), 0, st, N, j + 1, w, (const double *)G.V, (const double *)h, npart, (const int *)words);
            });
        }
        hipLaunchKernelGGL(k_gm_hess, dim3(1), dim3(kBlock), 0, st, j, G, S.max_iterations, S.d_scal, words);
        hipLaunchKernelGGL(k_gm_scale<false>, dim3(gv), dim3(kBlock), 0, st, N, (const double *)w, (const double *)(G.H + (size_t)j * (m + 1) + j + 1),
                           G.V + (size_t)(j + 1) * n, (const int *)words);
    };
    const auto cycle_end = [&] {
        hipLaunchKernelGGL(k_gm_tri, dim3(1), dim3(64), 0, st, G, words);
        if ((rc = add(u, z)) != FD_OK) return;
        hipLaunchKernelGGL(k_gm_close, dim3(1), dim3(64), 0, st, words);
        if ((rc = product(4, (const double *)V.y, w)) != FD_OK) return;
        hipLaunchKernelGGL(k_gm_resid, dim3(gv), dim3(kBlock), 0, st, N, b, (const double *)w, V.r, S.d_scal, words, S.d_part);
        hipLaunchKernelGGL(k_gm_start<0>, dim3(gv), dim3(kBlock), 0, st, N, (const double *)V.r, G, S.rtol, S.d_scal, (const int *)words);
    };
    // batches as in CscSolveState::run, but a batch ends where its cycle does, and the cycle's end goes with it
    int enq = 0, j = 0, nb = 0;
    bool stop = false;
    while (!stop) {
        int todo = S.max_iterations - enq < S.batch ? S.max_iterations - enq : S.batch;
        if (m - j < todo) todo = m - j;
        for (int it = 0; it < todo && rc == FD_OK; ++it) step(j++);
        enq += todo;
        if (rc == FD_OK && (j == m || enq >= S.max_iterations)) { cycle_end(); j = 0; }
        if (rc != FD_OK) return rc;
        FD_HIP_CHECK(hipGetLastError());
        FD_HIP_CHECK(hipMemcpyAsync(&S.h_rec[nb & 1], S.d_words, sizeof(CsRecord), hipMemcpyDeviceToHost, st));
        FD_HIP_CHECK(hipEventRecord(S.ev[nb & 1], st));
        if (nb >= 1) {
            FD_HIP_CHECK(hipEventSynchronize(S.ev[(nb - 1) & 1]));
            const CsRecord &rec = S.h_rec[(nb - 1) & 1];
            if (rec.done) stop = true;
            else if (rec.early) { cycle_end(); stop = true; }      // the cycle ended in the middle of that batch: what it has goes into y
            if (rc != FD_OK) return rc;
        }
        ++nb;
        if (enq >= S.max_iterations) stop = true;
    }
    return FD_OK;
}

int fd_csc_solve_async(fd_csc_solver *s, double alpha, double beta, const void *nzval, const void *b, void *y)
{
    return fd_csc_solve_from_async(s, alpha, beta, nzval, b, nullptr, y);
}

// y0 == NULL: the cold start, launch for launch.  Otherwise k_cs_init_from stands where k_cs_init stood (behind k_cs_long on y0 when the
// pattern has long rows); everything behind the start is the same solve.  y is written by the final kernel alone.
int fd_csc_solve_from_async(fd_csc_solver *s, double alpha, double beta, const void *nzval, const void *b, const void *y0, void *y)
{
    FD_REQUIRE(s && b && y && (nzval || s->L.nnz == 0), FD_ERR_ARG, "NULL argument");
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    CscSolveState &S = s->S;
    const int N = (int)s->L.N;
    const size_t n = (size_t)N;
    const real_t *nz = (const real_t *)nzval;
    CsVecs V;
    s->slice({{&V.r, n}, {&V.rhat, n}, {&V.p, n}, {&V.v, n}, {&V.s, n}, {&V.t, n}, {&V.ph, n}, {&V.sh, n}, {&V.y, n}, {&V.d, n}});
    const CsView P = cs_view(s->L, s->window);
    const unsigned gv = cs_tiles(N, kCsVecTile);
    const int bs = s->pc_kind == FD_CSC_PRECOND_BLOCK_JACOBI ? s->pc_bs : 0;
    s->gen += 1;      // whatever fd_csc_solver_factor_async left is this solve's from here on
    if (bs > 0) {
        const int rm = csc_minv_reserve(s, bs);
        if (rm != FD_OK) return rm;
    }
    const bool gmres = s->method == FD_CSC_METHOD_GMRES;
    if (gmres && (s->gm_cap < gm_doubles(n, s->gm_restart, gv) || s->gm_m != s->gm_restart)) {
        FD_HIP_CHECK(hipStreamSynchronize(st));
        const size_t need = gm_doubles(n, s->gm_restart, gv);
        if (s->gm_cap < need) {
            if (s->d_gm) (void)hipFree(s->d_gm);
            s->d_gm = nullptr; s->gm_cap = 0; s->gm_m = 0;
            const hipError_t e = hipMalloc((void **)&s->d_gm, sizeof(double) * need);
            if (e != hipSuccess) { (void)hipGetLastError(); FD_REQUIRE(false, FD_ERR_NOMEM, "GMRES: %d + 1 vectors of %d doubles: %s", s->gm_restart, N, hipGetErrorString(e)); }
            s->gm_cap = need;
        }
        s->gm_m = s->gm_restart;
    }
    FD_HIP_CHECK(hipMemsetAsync(S.d_words, 0, sizeof(int) * W_NWORDS, st));
    const bool ilu = s->pc_kind == kCsPcIlu, blocks = ilu || bs > 0;      // blocks: the PC = 1 instances of the vector kernels
    const CsIlu I = ilu ? csc_ilu(s) : CsIlu();
    const unsigned gi = ilu ? (unsigned)ilu_nblk(s, s->ilu_bs) : 0u;
    const double *lu = s->d_ilu, *u = ilu ? s->d_ilu + (size_t)s->L.nnz : nullptr;
    const double *scal = S.d_scal;
    const int *words = S.d_words;
    // precondition `which` (0: p -> ph; 1: s -> sh): out = M^-1 x behind the vector kernel (the diagonal: that kernel has divided already)
    const auto apply = [&](int which, const double *x, double *out) {
        if (ilu) hipLaunchKernelGGL(which ? k_cs_ilu_apply<1> : k_cs_ilu_apply<0>, dim3(gi), dim3(kBlock), 0, st, P, I, lu, u, x, out, words);
        else if (bs > 0) hipLaunchKernelGGL(which ? k_cs_bapply<1> : k_cs_bapply<0>, dim3(gv), dim3(kBlock), 0, st, N, bs, (const double *)s->d_minv, x, out, words);
    };
    // the start: init, then factor or invert
    if (y0) {      // w = A y0 of the long rows into V.t (nothing reads t before the iteration's second product writes it), then the fused start
        cs_launch_long<false, CS_LONG_AXPBY>(st, P, nz, (const real_t *)y0, V.t, nullptr, alpha, beta);
        fd_pick<0, 1>(blocks ? 1 : 0, [&](auto PCK) {
            hipLaunchKernelGGL(k_cs_init_from<PCK()>, dim3(gv), dim3(kBlock), 0, st, P, V, alpha, beta, nz, (const real_t *)b, (const real_t *)y0,
                               (const double *)V.t, S.rtol, S.d_scal, S.d_words, S.d_part);
        });
    } else if (blocks) hipLaunchKernelGGL(k_cs_init<1>, dim3(gv), dim3(kBlock), 0, st, P, V, alpha, beta, nz, (const real_t *)b, S.rtol, S.d_scal, S.d_words, S.d_part);
    else hipLaunchKernelGGL(k_cs_init<0>, dim3(gv), dim3(kBlock), 0, st, P, V, alpha, beta, nz, (const real_t *)b, S.rtol, S.d_scal, S.d_words, S.d_part);
    if (ilu) csc_ilu_factor_launch(s, alpha, beta, nz, S.d_words);
    else if (bs > 0) csc_binv_launch(s, bs, alpha, beta, nz, S.d_words);
    s->last_gmres = gmres;
    if (gmres) {
        const CsGm G = csc_gm(s, s->gm_m);
        const int rc = csc_gmres_iterate(st, S, N, G, (const real_t *)b, V, y0 != nullptr,
            [&](const double *vj, double *z, const double **zj) {      // z = M^-1 v_j
                if (blocks) apply(1, vj, z);
                else hipLaunchKernelGGL(k_gm_scale<true>, dim3(gv), dim3(kBlock), 0, st, N, vj, (const double *)V.d, z, words);
                *zj = z;
                return FD_OK;
            },
            [&](int mode, const double *v, double *w) {
                if (mode == 3) csc_product<double, 3>(s, alpha, beta, nz, v, w, nullptr, true);
                else csc_product<double, 4>(s, alpha, beta, nz, v, w, nullptr, true);
                return FD_OK;
            },
            [&](double *u, double *z) {      // y = y + M^-1 (V t): the diagonal inside k_gm_combine, the blocks behind it
                if (!blocks) {
                    hipLaunchKernelGGL(k_gm_combine<1>, dim3(gv), dim3(kBlock), 0, st, N, G, (const double *)V.d, V.y, words);
                } else {
                    hipLaunchKernelGGL(k_gm_combine<0>, dim3(gv), dim3(kBlock), 0, st, N, G, (const double *)V.d, u, words);
                    apply(0, u, z);
                    hipLaunchKernelGGL(k_gm_yadd, dim3(gv), dim3(kBlock), 0, st, N, V.y, (const double *)z, words);
                }
                return FD_OK;
            });
        if (rc != FD_OK) return rc;
        hipLaunchKernelGGL(k_gm_final, dim3(cs_tiles(N, kBlock)), dim3(kBlock), 0, st, N, (const double *)V.y, (real_t *)y, S.d_words,
                           csc_gm(s, s->gm_m).klast, S.keep);
        FD_HIP_CHECK(hipGetLastError());
        S.solved = true;
        return FD_OK;
    }
    const int rc = S.run(st, [&] {      // one iteration: 5 launches (+ 2 with long rows, + 2 with block Jacobi or block ILU)
        if (blocks) hipLaunchKernelGGL(k_cs_p<1>, dim3(gv), dim3(kBlock), 0, st, N, V, scal, words);
        else hipLaunchKernelGGL(k_cs_p<0>, dim3(gv), dim3(kBlock), 0, st, N, V, scal, words);
        apply(0, V.p, V.ph);
        csc_product<double, 1>(s, alpha, beta, nz, V.ph, V.v, V.rhat, true);
        if (blocks) hipLaunchKernelGGL(k_cs_s<1>, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
        else hipLaunchKernelGGL(k_cs_s<0>, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
        apply(1, V.s, V.sh);
        csc_product<double, 2>(s, alpha, beta, nz, V.sh, V.t, V.s, true);
        hipLaunchKernelGGL(k_cs_update, dim3(gv), dim3(kBlock), 0, st, N, V, S.d_scal, S.d_words, S.d_part);
    });
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(k_cs_final, dim3(cs_tiles(N, kBlock)), dim3(kBlock), 0, st, N, (const double *)V.y, (real_t *)y, S.d_words, S.keep);
    FD_HIP_CHECK(hipGetLastError());
    S.solved = true;
    return FD_OK;
}

// ---- the factorisation and its application as operations of their own ----------------------------------------------------------------
// M for alpha I + beta J from whichever preconditioner is selected: the launches a solve runs behind its k_cs_init, on words of the
// factorisation's own (a solve clears S.d_words), so the bits are those a solve with the same (alpha, beta, nzval) leaves
int fd_csc_solver_factor_async(fd_csc_solver *s, double alpha, double beta, const void *nzval)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(nzval || s->L.nnz == 0, FD_ERR_ARG, "nzval is NULL");
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const int N = (int)s->L.N;
    const real_t *nz = (const real_t *)nzval;
    s->gen += 1;
    s->fact_gen = 0;
    const char *who = "csc solver factor";
    if (!s->d_fwords) {
        CSC_TRY(who, hipMalloc((void **)&s->d_fwords, sizeof(int) * 2 * W_NWORDS));
        CSC_TRY(who, hipMemsetAsync(s->d_fwords, 0, sizeof(int) * 2 * W_NWORDS, st));
    }
    const int kind = s->pc_kind, bs = s->pc_bs;
    if (kind == FD_CSC_PRECOND_JACOBI && !s->d_fdiag) CSC_TRY(who, hipMalloc((void **)&s->d_fdiag, sizeof(double) * (size_t)N));
    if (kind == FD_CSC_PRECOND_BLOCK_JACOBI) {
        const int rm = csc_minv_reserve(s, bs);
        if (rm != FD_OK) return rm;
    }
    FD_HIP_CHECK(hipMemsetAsync(s->d_fwords, 0, sizeof(int) * W_NWORDS, st));
    if (kind == kCsPcIlu) csc_ilu_factor_launch(s, alpha, beta, nz, s->d_fwords);
    else if (kind == FD_CSC_PRECOND_BLOCK_JACOBI) csc_binv_launch(s, bs, alpha, beta, nz, s->d_fwords);
    else hipLaunchKernelGGL(k_cs_fdiag, dim3(cs_tiles(N, kBlock)), dim3(kBlock), 0, st, cs_view(s->L, s->window), alpha, beta, nz, s->d_fdiag, s->d_fwords);
    FD_HIP_CHECK(hipGetLastError());
    s->fact_kind = kind; s->fact_bs = bs;
    s->fact_gen = s->gen;
    return FD_OK;
}

// is the factorisation of the last fd_csc_solver_factor_async still in the solver's buffers?  FD_OK, or the code with its message
static int csc_factor_valid(const fd_csc_solver *s)
{
    FD_REQUIRE(s->fact_gen != 0, FD_ERR_UNSUPPORTED, "fd_csc_solver_factor_async has not run on this solver");
    FD_REQUIRE(s->fact_gen == s->gen, FD_ERR_STALE,
               "the factorisation is stale: a solve or a preconditioner setter came after fd_csc_solver_factor_async and its buffers are no longer that factorisation's");
    return FD_OK;
}
// out = M^-1 x with the solver's own apply kernels: WHICH 0 on `words` (W_DONE ends it), 1 also on `cycle over`
static void csc_factor_apply(fd_csc_solver *s, int which, const double *x, double *out, const int *words)
{
    hipStream_t st = s->ctx->stream;
    const int N = (int)s->L.N;
    const unsigned gv = cs_tiles(N, kCsVecTile);
    if (s->fact_kind == kCsPcIlu) {
        hipLaunchKernelGGL(which ? k_cs_ilu_apply<1> : k_cs_ilu_apply<0>, dim3((unsigned)ilu_nblk(s, s->ilu_bs)), dim3(kBlock), 0, st, cs_view(s->L, s->window),
                           csc_ilu(s), (const double *)s->d_ilu, (const double *)(s->d_ilu + (size_t)s->L.nnz), x, out, words);
    } else if (s->fact_kind == FD_CSC_PRECOND_BLOCK_JACOBI) {
        hipLaunchKernelGGL(which ? k_cs_bapply<1> : k_cs_bapply<0>, dim3(gv), dim3(kBlock), 0, st, N, s->fact_bs, (const double *)s->d_minv, x, out, words);
    } else {
        hipLaunchKernelGGL(k_gm_scale<true>, dim3(gv), dim3(kBlock), 0, st, N, x, (const double *)s->d_fdiag, out, words);
    }
}

// out = M^-1 x, N doubles each in either element build, unguarded: the words it runs on stay zero
int fd_csc_solver_apply_async(fd_csc_solver *s, const void *x, void *out)
{
    FD_REQUIRE(s && x && out, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(out != x, FD_ERR_ARG, "out must not be x");
    const int rv = csc_factor_valid(s);
    if (rv != FD_OK) return rv;
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    csc_factor_apply(s, 0, (const double *)x, (double *)out, s->d_fwords + W_NWORDS);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

// synchronises; flags bit 1: a pivot of the last factorisation was zero or not finite
int fd_csc_solver_factor_status(fd_csc_solver *s, int *flags)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    FD_REQUIRE(s->d_fwords != nullptr, FD_ERR_UNSUPPORTED, "fd_csc_solver_factor_async has not run on this solver");
    FD_HIP_CHECK(hipSetDevice(s->ctx->device));
    FD_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
    int w[W_NWORDS];
    FD_HIP_CHECK(hipMemcpy(w, s->d_fwords, sizeof w, hipMemcpyDeviceToHost));
    if (flags) *flags = w[W_FLAGS] & 2;
    return FD_OK;
}

int fd_csc_solver_status(fd_csc_solver *s, int *flags_out, int64_t *iterations_out, double *resid_out, double *bnorm_out)
{
    FD_REQUIRE(s != nullptr, FD_ERR_ARG, "solver is NULL");
    int w[W_NWORDS];
    double sc[S_NSCAL];
    const int rc = s->S.read_status(s->ctx, w, sc);
    if (rc != FD_OK) return rc;
    if (flags_out) *flags_out = w[W_FINAL];
    if (iterations_out) *iterations_out = w[W_ITERS];
    if (resid_out) *resid_out = s->last_gmres ? sc[S_GRES] : std::sqrt(sc[S_RNORM2]);
    if (bnorm_out) *bnorm_out = std::sqrt(sc[S_BNORM2]);
    return FD_OK;
}

#ifndef FDJAC_F32
#include "fdjac_jfnk.hip"      // the matrix-free consumer: Float64 only
#endif
