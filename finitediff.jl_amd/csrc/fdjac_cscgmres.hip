// Right-preconditioned restarted GMRES(m) of the sparse consumer (fd_csc_solver_set_method; DESIGN.md 4.9, "GMRES").  A piece of
// fdjac_cscsolve.hip (included there, in both element builds): it uses that file's handle, its products, its start kernels and its
// preconditioner applies as they are.  tests/csc_gmres_model.py restates every order below in numpy and the GPU tests compare bits.
//
// THE CYCLE.  r = b (first cycle) or b - A y (k_cs_rows<double, 4>, then k_gm_resid); gamma = sqrt(dot_vec(r, r)); v_0 = r / gamma
// (k_gm_start); g = (gamma, 0, ...).  A later cycle with gamma <= rtol ||b|| is converged; gamma^2 not finite is a breakdown.
// STEP j (host and device agree on j: a batch never spans two cycles, and a step after `cycle over` or `done` does nothing):
//   z = M^-1 v_j        the diagonal: k_gm_scale; blocks: k_cs_bapply<1> / k_cs_ilu_apply<1> (their `early` guard is `cycle over` here)
//   w = A z             k_cs_long + k_cs_rows<double, 3>
//   CGS2                k_cs_gs_dots, k_cs_gs_reduce: h_i = dot_vec(w, v_i), i = 0 .. j, all from the same w;
//                       k_cs_gs_update: w_e = ((w_e - h_0 v_0e) - h_1 v_1e) - ... (one multiply, one subtraction per term);
//                       the same again: h'_i, then the update, which also leaves the tiles' sums of dot_vec(w, w)
//   k_gm_hess           one workgroup: H[i, j] = h_i + h'_i, H[j + 1, j] = sqrt(dot_vec(w, w)); any of them not finite: breakdown (the
//                       column does not count).  The column goes through the stored rotations i = 0 .. j - 1:
//                       (a, b) = (col_i, col_i+1) -> (c_i a + s_i b, c_i b - s_i a); then rho = sqrt(a a + b b) of (col_j, col_j+1),
//                       rho = 0: c = 1, s = 0; else c = a / rho, s = b / rho; rho, c or s not finite: breakdown; R[j, j] = rho;
//                       g_j+1 = -s g_j, g_j = c g_j; the estimate is |g_j+1|.  The column is complete: iterations + 1.  `cycle over`
//                       when the estimate <= rtol ||b|| (converged), H[j + 1, j] = 0, j + 1 = m, or the iterations have run out.
//   v_j+1 = w / H[j + 1, j]    k_gm_scale (a division per element); not after `cycle over`
// THE END OF A CYCLE (enqueued where the host knows a cycle ends -- m columns or the last permitted step -- and once more when a record
// shows `cycle over` in the middle of one; it does nothing unless the device says `cycle over` and not `done`):
//   k_gm_tri            one lane: t_i = (g_i - sum_{k > i} R[i, k] t_k) / R[i, i], i = K - 1 .. 0, the sum from +0.0 with k ascending; a
//                       pivot that is zero or not finite: breakdown, and y keeps what the earlier cycles gave it
//   k_gm_combine        u_e = sum_i t_i v_ie, i ascending from +0.0; the diagonal: y_e = y_e + u_e / d_e at once
//   blocks              z = M^-1 u (k_cs_bapply<0> / k_cs_ilu_apply<0>), y = y + z (k_gm_yadd)
//   k_gm_close          converged, broken down or out of iterations: `done`; otherwise the next cycle starts (above)
// Nothing but the record of a batch goes to the host.  Launches per step: 10 (+ 1 with long rows); per cycle end: 8 (diagonal) or 10.
#pragma once
#include "fdjac_dotx.h"

namespace fdjac {

constexpr int kGmMax = FD_CSC_GMRES_RESTART_MAX;
// the internal bits of W_FLAGS beside bit 1 (breakdown): k_gm_final turns them into the status word
constexpr int kGmRanOut = 4, kGmConverged = 8;

struct CsGm {                          // the buffers of a GMRES solve as the kernels see them (restart m)
    int m, ntile;
    double *V;                         // the basis, vector-major: v_i at V + i N, i = 0 .. m
    double *H;                         // m columns of m + 1: H[i, j] at H[j (m + 1) + i], as Arnoldi gave them
    double *R;                         // the same columns behind the rotations (the triangle the back substitution reads)
    double *c, *s, *g, *t;             // the rotations (m each), the rotated right-hand side (m + 1), the combination (m)
    double *h1, *h2;                   // the two CGS passes' coefficients (m + 1 each)
    double *part;                      // [m + 1][ntile] sums of the tiles per basis vector, then ntile sums of dot_vec(w, w)
    int *klast;                        // the columns of the last cycle (fd_csc_solver_gmres_basis)
};
__device__ __forceinline__ bool gm_idle(const int *words) { return cs_word(words, W_DONE) || cs_word(words, W_EARLY); }
__device__ __forceinline__ bool gm_ending(const int *words) { return cs_word(words, W_EARLY) && !cs_word(words, W_DONE); }
// what _final does in the model: thread t adds part[t], part[t + 256], ... in order, then block_sum()
__device__ __forceinline__ double gm_final_sum(const double *part, int n, double *s_w)
{
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += kBlock) acc += part[k];
    return cs_block_sum(acc, s_w);
}

// ---- the Gram-Schmidt kernels ------------------------------------------------------------------------------------------------------------
// One workgroup per tile of kCsVecTile elements whatever nv is.  dot_vec's order puts element t + 256 k of the tile on thread t, so a lane
// loads 8 bytes at a time and a wavefront's load covers 512 consecutive bytes of one vector; the four loads of a lane's elements of
// kGsAhead vectors are all requested before the first is used.  w's four elements stay in registers; nothing that is used once goes
// through LDS (the wavefronts' sums do: nv x 4 doubles).
constexpr int kGsAhead = 4;
constexpr int kGsPer = kCsVecTile / kBlock;
__global__ void __launch_bounds__(kBlock) k_cs_gs_dots(int N, int nv, const double *__restrict__ w, const double *__restrict__ V,
                                                       double *__restrict__ part, const int *words)
{
    __shared__ double s_ws[(kGmMax + 1) * (kBlock / 64)];
    if (gm_idle(words)) return;
    const int e0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double we[kGsPer];
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) we[k] = e0 + k * kBlock < N ? w[e0 + k * kBlock] : 0.0;
    for (int i0 = 0; i0 < nv; i0 += kGsAhead) {
        double ve[kGsAhead][kGsPer];
#pragma unroll
        for (int a = 0; a < kGsAhead; ++a) {
            const double *v = V + (size_t)(i0 + a < nv ? i0 + a : nv - 1) * N;
#pragma unroll
            for (int k = 0; k < kGsPer; ++k) ve[a][k] = e0 + k * kBlock < N ? v[e0 + k * kBlock] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < kGsAhead; ++a) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < kGsPer; ++k) acc += we[k] * ve[a][k];
            acc = wave_sum(acc);      // (fdjac_dotx.h)
            if ((threadIdx.x & 63) == 0 && i0 + a < nv) s_ws[(i0 + a) * (kBlock / 64) + (threadIdx.x >> 6)] = acc;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nv; i += kBlock) {
        const double *q = s_ws + i * (kBlock / 64);
        part[(size_t)i * gridDim.x + blockIdx.x] = ((q[0] + q[1]) + q[2]) + q[3];
    }
}
// h_i = the tiles' sums of vector i in order: one workgroup per vector
__global__ void __launch_bounds__(kBlock) k_cs_gs_reduce(int ntile, const double *__restrict__ part, double *__restrict__ h, const int *words)
{
    __shared__ double s_w[kBlock / 64];
    if (gm_idle(words)) return;
    const double t = gm_final_sum(part + (size_t)blockIdx.x * ntile, ntile, s_w);
    if (threadIdx.x == 0) h[blockIdx.x] = t;
}
// w = w - V h, term by term in ascending i; NORM (the second pass): the tile's sum of dot_vec(w, w) of the new w goes to npart
template <bool NORM>
__global__ void __launch_bounds__(kBlock) k_cs_gs_update(int N, int nv, double *__restrict__ w, const double *__restrict__ V,
                                                         const double *__restrict__ h, double *__restrict__ npart, const int *words)
{
    __shared__ double s_w[kBlock / 64];
    if (gm_idle(words)) return;
    const int e0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double we[kGsPer];
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) we[k] = e0 + k * kBlock < N ? w[e0 + k * kBlock] : 0.0;
    for (int i0 = 0; i0 < nv; i0 += kGsAhead) {
        double ve[kGsAhead][kGsPer];
#pragma unroll
        for (int a = 0; a < kGsAhead; ++a) {
            const double *v = V + (size_t)(i0 + a < nv ? i0 + a : nv - 1) * N;
#pragma unroll
            for (int k = 0; k < kGsPer; ++k) ve[a][k] = e0 + k * kBlock < N ? v[e0 + k * kBlock] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < kGsAhead; ++a) {
            if (i0 + a >= nv) break;
            const double hi = h[i0 + a];
#pragma unroll
            for (int k = 0; k < kGsPer; ++k) we[k] = we[k] - hi * ve[a][k];
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) {
        if (e0 + k * kBlock < N) w[e0 + k * kBlock] = we[k];
        if (NORM) acc += we[k] * we[k];
    }
    if (NORM) {
        const double t = cs_block_sum(acc, s_w);
        if (threadIdx.x == 0) npart[blockIdx.x] = t;
    }
}

// ---- the vector kernels of a cycle ---------------------------------------------------------------------------------------------------
// out = x / d (z = v_j / d under the diagonal preconditioner) or out = x / *scalar (v_j+1 = w / H[j + 1, j]): a division per element
template <bool BYVEC>
__global__ void __launch_bounds__(kBlock) k_gm_scale(int N, const double *__restrict__ x, const double *__restrict__ d, double *__restrict__ out,
                                                     const int *words)
{
    if (gm_idle(words)) return;
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    const double by = BYVEC ? 0.0 : d[0];
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) {
        const int i = i0 + k * kBlock;
        if (i < N) out[i] = x[i] / (BYVEC ? d[i] : by);
    }
}
// the start of a cycle: v_0 = r / gamma, g_0 = gamma.  FIRST 1: gamma^2 = ||b||^2 (k_cs_init's), and the tolerance and the first estimate
// are set whatever the start kernels found; 2 (a warm start): gamma^2 = ||r0||^2 as the warm start kernel left it in S_GAMMA2, the
// tolerance still from ||b||; later cycles (0) take what k_gm_resid left
template <int FIRST>
__global__ void __launch_bounds__(kBlock) k_gm_start(int N, const double *__restrict__ r, CsGm G, double rtol, double *scal, const int *words)
{
    const double gamma = sqrt(scal[FIRST == 1 ? S_BNORM2 : S_GAMMA2]);
    if (FIRST && blockIdx.x == 0 && threadIdx.x == 0) {
        scal[S_GTOL] = rtol * (FIRST == 1 ? gamma : sqrt(scal[S_BNORM2]));
        scal[S_GRES] = gamma;
    }
    if (cs_word(words, W_DONE)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) G.g[0] = gamma;
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) {
        const int i = i0 + k * kBlock;
        if (i < N) G.V[i] = r[i] / gamma;
    }
}
// a later cycle: r = b - w (w = A y), gamma^2 = dot_vec(r, r); the workgroup that finishes the dot opens the cycle or ends the solve
__global__ void __launch_bounds__(kBlock) k_gm_resid(int N, const real_t *__restrict__ b, const double *__restrict__ w, double *__restrict__ r,
                                                     double *scal, int *words, double *part)
{
    __shared__ double s_w[kBlock / 64];
    if (cs_word(words, W_DONE)) return;
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double mine[1] = {0.0}, tot[1];
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) {
        const int i = i0 + k * kBlock;
        if (i >= N) continue;
        const double ri = (double)b[i] - w[i];
        r[i] = ri;
        mine[0] += ri * ri;
    }
    if (cs_finish<1>(mine, part, words, tot, s_w) && threadIdx.x == 0) {
        const double gamma = sqrt(tot[0]);
        scal[S_GAMMA2] = tot[0];
        scal[S_GRES] = gamma;
        if (cs_not_finite(tot[0])) cs_breakdown(words);
        else if (gamma <= scal[S_GTOL]) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else {
            words[W_GM_K] = 0;
            __hip_atomic_store(words + W_EARLY, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// column j of the Hessenberg matrix, its rotations and the estimate (the file's head has the arithmetic): one workgroup, the sum of
// dot_vec(w, w) by all of it, the rest by thread 0
__global__ void __launch_bounds__(kBlock) k_gm_hess(int j, CsGm G, int max_iterations, double *scal, int *words)
{
    __shared__ double s_w[kBlock / 64];
    if (gm_idle(words)) return;
    const double nrm2 = gm_final_sum(G.part + (size_t)(G.m + 1) * G.ntile, G.ntile, s_w);
    if (threadIdx.x != 0) return;
    const int ld = G.m + 1;
    double *Hj = G.H + (size_t)j * ld, *Rj = G.R + (size_t)j * ld;
    const double hn = sqrt(nrm2);
    bool bad = cs_not_finite(hn);
    for (int i = 0; i <= j; ++i) {
        const double hij = G.h1[i] + G.h2[i];
        Hj[i] = hij;
        Rj[i] = hij;
        bad = bad || cs_not_finite(hij);
    }
    Hj[j + 1] = hn;
    Rj[j + 1] = hn;
    for (int i = j + 2; i < ld; ++i) { Hj[i] = 0.0; Rj[i] = 0.0; }
    double c = 1.0, s = 0.0, rho = 0.0;
    if (!bad) {
        for (int i = 0; i < j; ++i) {
            const double a = Rj[i], b = Rj[i + 1], ci = G.c[i], si = G.s[i];
            Rj[i] = ci * a + si * b;
            Rj[i + 1] = ci * b - si * a;
        }
        const double a = Rj[j], b = Rj[j + 1];
        rho = sqrt(a * a + b * b);
        if (rho != 0.0) { c = a / rho; s = b / rho; }
        bad = cs_not_finite(rho) || cs_not_finite(c) || cs_not_finite(s);
    }
    if (bad) {                        // the column does not count: the iterate of the columns before it is what policy 1 keeps
        atomicOr(words + W_FLAGS, 2);
        __hip_atomic_store(words + W_EARLY, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    Rj[j] = rho;
    Rj[j + 1] = 0.0;
    G.c[j] = c;
    G.s[j] = s;
    const double gj = G.g[j];
    G.g[j] = c * gj;
    G.g[j + 1] = -s * gj;
    const double est = fabs(G.g[j + 1]);
    scal[S_GRES] = est;
    words[W_GM_K] = j + 1;
    const int iters = words[W_ITERS] + 1;
    words[W_ITERS] = iters;
    const bool conv = est <= scal[S_GTOL];
    if (conv) atomicOr(words + W_FLAGS, kGmConverged);
    else if (iters >= max_iterations) atomicOr(words + W_FLAGS, kGmRanOut);
    if (conv || hn == 0.0 || j + 1 == G.m || iters >= max_iterations)
        __hip_atomic_store(words + W_EARLY, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the back substitution R t = g over the K columns of the cycle: W_GM_UPD = K, or 0 when there is nothing to add to y
__global__ void k_gm_tri(CsGm G, int *words)
{
    if (threadIdx.x != 0) return;
    words[W_GM_UPD] = 0;
    if (!gm_ending(words)) return;
    const int K = words[W_GM_K], ld = G.m + 1;
    bool bad = false;
    for (int i = K - 1; i >= 0; --i) {
        double sum = 0.0;
        for (int k = i + 1; k < K; ++k) sum += G.R[(size_t)k * ld + i] * G.t[k];
        const double piv = G.R[(size_t)i * ld + i];
        bad = bad || cs_bad_pivot(piv);
        G.t[i] = (G.g[i] - sum) / piv;
    }
    if (bad) atomicOr(words + W_FLAGS, 2);
    else words[W_GM_UPD] = K;
}
// u = V t over the columns k_gm_tri counted; HOW 1: y = y + u / d at once; 2: y = y + u (no preconditioner: the matrix-free consumer);
// 0: u is stored for the block apply
template <int HOW>
__global__ void __launch_bounds__(kBlock) k_gm_combine(int N, CsGm G, const double *__restrict__ d, double *__restrict__ out, const int *words)
{
    const int K = words[W_GM_UPD];
    if (K == 0) return;
    const int e0 = blockIdx.x * kCsVecTile + threadIdx.x;
    double acc[kGsPer];
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) acc[k] = 0.0;
    for (int i0 = 0; i0 < K; i0 += kGsAhead) {
        double ve[kGsAhead][kGsPer];
#pragma unroll
        for (int a = 0; a < kGsAhead; ++a) {
            const double *v = G.V + (size_t)(i0 + a < K ? i0 + a : K - 1) * N;
#pragma unroll
            for (int k = 0; k < kGsPer; ++k) ve[a][k] = e0 + k * kBlock < N ? v[e0 + k * kBlock] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < kGsAhead; ++a) {
            if (i0 + a >= K) break;
            const double ti = G.t[i0 + a];
#pragma unroll
            for (int k = 0; k < kGsPer; ++k) acc[k] += ti * ve[a][k];
        }
    }
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) {
        const int i = e0 + k * kBlock;
        if (i >= N) continue;
        if (HOW == 1) out[i] = out[i] + acc[k] / d[i];
        else if (HOW == 2) out[i] = out[i] + acc[k];
        else out[i] = acc[k];
    }
}
// y = y + z (z = M^-1 u of a block preconditioner)
__global__ void __launch_bounds__(kBlock) k_gm_yadd(int N, double *__restrict__ y, const double *__restrict__ z, const int *words)
{
    if (words[W_GM_UPD] == 0) return;
    const int i0 = blockIdx.x * kCsVecTile + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kGsPer; ++k) {
        const int i = i0 + k * kBlock;
        if (i < N) y[i] = y[i] + z[i];
    }
}
// the cycle is over: is the solve?
__global__ void k_gm_close(int *words)
{
    if (threadIdx.x != 0 || !gm_ending(words)) return;
    if (cs_word(words, W_FLAGS) & (2 | kGmRanOut | kGmConverged)) __hip_atomic_store(words + W_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the end: the status word (bit 1: breakdown; bit 0: the iterations ran out), the last cycle's length, and y, or NaN after a failure
// unless the caller keeps the iterate
__global__ void __launch_bounds__(kBlock) k_gm_final(int N, const double *__restrict__ yacc, real_t *__restrict__ y, int *words, int *klast, int keep)
{
    const int f = cs_word(words, W_FLAGS);
    const int flags = (f & 2) ? 2 : (((f & kGmRanOut) || !cs_word(words, W_DONE)) ? 1 : 0);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        words[W_FINAL] = flags;
        *klast = words[W_GM_K];
    }
    if (i >= N) return;
    y[i] = (real_t)((flags && !keep) ? __longlong_as_double(0x7FF8000000000000ll) : ((f & kCsYZero) ? 0.0 : yacc[i]));
}

}  // namespace fdjac
