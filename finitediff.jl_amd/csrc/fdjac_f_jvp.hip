// Included by fdjac_builtin_f.hip (namespace fdjac, after the family files: tridiag_row and stencil5_pair are theirs).
// ---- lazy-point launchers of a JVP (fd_f_launch_lazy_jvp): f at x + eps*v / x - eps*v, perturbed while loading ----
// Points are formed as x[j] + (eps*v[j]) and x[j] - (eps*v[j]) exactly as k_jvp_points writes them, rows are evaluated
// with the same helpers as the plain kernels => bit-identical to the materialised path.
template <bool NL>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_lazy_jvp(real_t *__restrict__ fx, int64_t fs, real_t *__restrict__ base_out, const real_t *__restrict__ x,
                     const real_t *__restrict__ v, const real_t *__restrict__ eps, int central, int64_t n,
                     real_t *__restrict__ qout)
{
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2;
    if (i >= n) return;
    const real_t e = eps[0];
    real_t xv[4], ev[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t j = i - 1 + k;
        const bool in = (j >= 0) & (j < n);
        xv[k] = in ? x[in ? j : 0] : 0.0;
        ev[k] = in ? e * v[in ? j : 0] : 0.0;
    }
    const bool two = i + 1 < n;
    if (qout) {   // fd_lazy_jvp_points.quotient_out: (f(x + eps v) - f(x)) / eps  or  (f(x + eps v) - f(x - eps v)) / (2 eps)
        real_t pp[4], pm[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { pp[k] = xv[k] + ev[k]; pm[k] = central ? xv[k] - ev[k] : xv[k]; }
        const real_t ed = central ? 2 * e : e;
        const real_t q0 = sub_exact(tridiag_row<real_t, NL>(pp[0], pp[1], pp[2]), tridiag_row<real_t, NL>(pm[0], pm[1], pm[2])) / ed;
        if (two) *reinterpret_cast<r2_t *>(qout + i) =
                     r2_t{q0, sub_exact(tridiag_row<real_t, NL>(pp[1], pp[2], pp[3]), tridiag_row<real_t, NL>(pm[1], pm[2], pm[3])) / ed};
        else qout[i] = q0;
        return;
    }
    if (base_out) {
        const real_t b0 = tridiag_row<real_t, NL>(xv[0], xv[1], xv[2]);
        if (two) *reinterpret_cast<r2_t *>(base_out + i) = r2_t{b0, tridiag_row<real_t, NL>(xv[1], xv[2], xv[3])};
        else base_out[i] = b0;
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m == 1 && !central) break;
        // forward: member 0 = x + eps v; central: member 0 = x - eps v, member 1 = x + eps v
        const bool minus = central && m == 0;
        real_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = minus ? xv[k] - ev[k] : xv[k] + ev[k];
        real_t *dst = fx + (int64_t)m * fs + i;
        const real_t v0 = tridiag_row<real_t, NL>(p[0], p[1], p[2]);
        if (two) *reinterpret_cast<r2_t *>(dst) = r2_t{v0, tridiag_row<real_t, NL>(p[1], p[2], p[3])};
        else dst[0] = v0;
    }
}

template <int SK>
__global__ void __launch_bounds__(kBlock)
k_f_stencil5_lazy_jvp(real_t *__restrict__ fx, int64_t fs, real_t *__restrict__ base_out, const real_t *__restrict__ x,
                      const real_t *__restrict__ v, const real_t *__restrict__ eps, int central, int64_t nx, int64_t ny,
                      real_t *__restrict__ qout)
{
    const int64_t n = nx * ny;
    const int64_t ntiles = (n + 2 * kBlock - 1) / (2 * kBlock);
    const int64_t tile = xcd_tile(blockIdx.x, ntiles);
    if (tile >= ntiles) return;
    const int64_t k = tile * (2 * kBlock) + threadIdx.x * 2;
    if (k >= n) return;
    const int64_t j = k / nx, i = k - j * nx;
    const bool hs = j > 0, hn = j + 1 < ny, hw = i > 0, he = i + 2 < nx;
    const int64_t idx[8] = {k, k + 1, k - nx, k - nx + 1, k + nx, k + nx + 1, k - 1, k + 2};
    const bool ok[8] = {true, true, hs, hs, hn, hn, hw, he};
    const real_t e = eps[0];
    real_t xv[8], ev[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int64_t at = ok[m] ? idx[m] : k;
        xv[m] = x[at];
        ev[m] = e * v[at];
    }
    if (qout) {   // fd_lazy_jvp_points.quotient_out
        real_t pp[8], pm[8], a0, a1, s0, s1;
#pragma unroll
        for (int q = 0; q < 8; ++q) { pp[q] = xv[q] + ev[q]; pm[q] = central ? xv[q] - ev[q] : xv[q]; }
        stencil5_pair<real_t, SK>(pp, hs, hn, hw, he, a0, a1);
        stencil5_pair<real_t, SK>(pm, hs, hn, hw, he, s0, s1);
        const real_t ed = central ? 2 * e : e;
        *reinterpret_cast<r2_t *>(qout + k) = r2_t{sub_exact(a0, s0) / ed, sub_exact(a1, s1) / ed};
        return;
    }
    if (base_out) {
        real_t b0, b1;
        stencil5_pair<real_t, SK>(xv, hs, hn, hw, he, b0, b1);
        *reinterpret_cast<r2_t *>(base_out + k) = r2_t{b0, b1};
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m == 1 && !central) break;
        const bool minus = central && m == 0;
        real_t p[8], o0, o1;
#pragma unroll
        for (int q = 0; q < 8; ++q) p[q] = minus ? xv[q] - ev[q] : xv[q] + ev[q];
        stencil5_pair<real_t, SK>(p, hs, hn, hw, he, o0, o1);
        *reinterpret_cast<r2_t *>(fx + (int64_t)m * fs + k) = r2_t{o0, o1};
    }
}

static bool has_lazy_jvp(const BuiltinF *b)
{
    if (b->family == FD_F_TRIDIAG || b->family == FD_F_TRIDIAG_NL) return true;
    return (b->family == FD_F_LAP5 || b->family == FD_F_CLAMP5 || b->family == FD_F_LAP5_NL) && (b->prm[0] % 2 == 0);  // pairs must not straddle grid rows
}

static int builtin_launch_lazy_jvp(void *fctx, void *fx, const fd_lazy_jvp_points *lp, int64_t fx_stride, void *stream)
{
    BuiltinF *b = (BuiltinF *)fctx;
    if (!b || b->magic != 0xFD0F00D5u || !lp) return 1;
    if (!has_lazy_jvp(b)) return FD_LAZY_DECLINED;
    if (((((uintptr_t)fx) | ((uintptr_t)lp->base_out) | ((uintptr_t)lp->quotient_out)) & kPairMask) != 0 || (fx_stride & 1)) return FD_LAZY_DECLINED;
    b->launches.fetch_add(1);
    b->points.fetch_add((lp->central ? 2 : 1) + ((lp->base_out || (lp->quotient_out && !lp->central)) ? 1 : 0));
    const hipStream_t s = (hipStream_t)stream;
    real_t *fxp = (real_t *)fx, *base = (real_t *)lp->base_out, *qout = (real_t *)lp->quotient_out;
    const real_t *x = (const real_t *)lp->x, *v = (const real_t *)lp->v, *eps = (const real_t *)lp->eps;
    if (b->family == FD_F_TRIDIAG || b->family == FD_F_TRIDIAG_NL) {
        const int64_t n = b->prm[0];
        const unsigned g = (unsigned)(((n + 1) / 2 + kBlock - 1) / kBlock);
        fd_pick<false, true>(b->family == FD_F_TRIDIAG_NL, [&](auto NL) {
            hipLaunchKernelGGL(k_f_tridiag_lazy_jvp<NL()>, dim3(g), dim3(kBlock), 0, s, fxp, fx_stride, base, x, v, eps, lp->central, n, qout);
        });
    } else {
        const int64_t n = b->prm[0] * b->prm[1];
        const unsigned g = (unsigned)(8 * xcd_chunks((n + 2 * kBlock - 1) / (2 * kBlock)));
        const int sk = b->family == FD_F_CLAMP5 ? 1 : b->family == FD_F_LAP5_NL ? 2 : 0;
        fd_pick<0, 1, 2>(sk, [&](auto SK) {
            hipLaunchKernelGGL(k_f_stencil5_lazy_jvp<SK()>, dim3(g), dim3(kBlock), 0, s, fxp, fx_stride, base, x, v, eps, lp->central,
                               b->prm[0], b->prm[1], qout);
        });
    }
    return launch_rc();
}
