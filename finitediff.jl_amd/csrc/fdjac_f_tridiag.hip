// The tridiagonal fixtures (FD_F_TRIDIAG, FD_F_TRIDIAG_NL) at lazily perturbed points: the kernels, then their launcher.
// Included by fdjac_builtin_f.hip (namespace fdjac, after launch_family).

template <typename T, bool NL> __device__ __forceinline__ T tridiag_row(T xm, T xi, T xp)
{
    T v = (xm - kTwo * xi) + xp;
    if (NL) v = v + (xi * xi) * xp;
    return v;
}

template <typename CT, int MODE, bool NL>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_lazy(real_t *__restrict__ fx, int64_t fs, real_t *__restrict__ base_out, const real_t *__restrict__ x,
                 const CT *__restrict__ color, const real_t *__restrict__ eps, int c_lo, int B, int64_t n, int64_t r0,
                 int64_t r1, int imag_only, int diff)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t i = r0 + ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; i < r1; i += stride) {
        // base values x[i-1..i+2] and their colours relative to the batch (-1: never perturbed)
        real_t xv[4];
        int cv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = i - 1 + k;
            const bool in = (j >= 0) & (j < n);
            xv[k] = in ? x[in ? j : 0] : 0.0;
            const int c = in ? (int)color[in ? j : 0] : -1;
            cv[k] = (c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;   // "none" is all-ones in CT
        }
        const bool two = i + 1 < n;
        real_t b0 = 0.0, b1 = 0.0;                    // f(x) at rows i, i+1 (written to base_out, or the subtrahend of diff)
        if (base_out || (diff && MODE == 0)) {
            b0 = tridiag_row<real_t, NL>(xv[0], xv[1], xv[2]);
            if (two) b1 = tridiag_row<real_t, NL>(xv[1], xv[2], xv[3]);
        }
        if (base_out) {
            if (two) *reinterpret_cast<r2_t *>(base_out + i) = r2_t{b0, b1};
            else base_out[i] = b0;
        }
        for (int b = 0; b < B; ++b) {
            const real_t e = eps[c_lo + b];
            real_t d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = (cv[k] == b) ? e : 0.0;
            if (MODE == 2) {
                cd p[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) p[k] = cd{xv[k], d[k]};
                const cd v0 = tridiag_row<cd, NL>(p[0], p[1], p[2]);
                if (imag_only) {   // imaginary parts as a real array (fd_lazy_points.imag_only)
                    real_t *dst = fx + (int64_t)b * fs + i;
                    if (two) {
                        const cd v1 = tridiag_row<cd, NL>(p[1], p[2], p[3]);
                        *reinterpret_cast<r2_t *>(dst) = r2_t{v0.im, v1.im};
                    } else {
                        dst[0] = v0.im;
                    }
                } else {
                    real_t *dst = fx + ((int64_t)b * fs + i) * 2;
                    *reinterpret_cast<r2_t *>(dst) = r2_t{v0.re, v0.im};
                    if (two) {
                        const cd v1 = tridiag_row<cd, NL>(p[1], p[2], p[3]);
                        *reinterpret_cast<r2_t *>(dst + 2) = r2_t{v1.re, v1.im};
                    }
                }
            } else if (diff) {
                // differences (fd_lazy_points.diff): f(x + d) - f(x), or f(x + d) - f(x - d), one array per colour
                real_t p[4], q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { p[k] = xv[k] + d[k]; q[k] = xv[k] - d[k]; }
                const real_t s0 = MODE == 1 ? tridiag_row<real_t, NL>(q[0], q[1], q[2]) : b0;
                const real_t v0 = sub_exact(tridiag_row<real_t, NL>(p[0], p[1], p[2]), s0);
                real_t v1 = 0.0;
                if (two) {
                    const real_t s1 = MODE == 1 ? tridiag_row<real_t, NL>(q[1], q[2], q[3]) : b1;
                    v1 = sub_exact(tridiag_row<real_t, NL>(p[1], p[2], p[3]), s1);
                }
                real_t *dst = fx + (int64_t)b * fs + i;
                if (two) *reinterpret_cast<r2_t *>(dst) = r2_t{v0, v1};
                else dst[0] = v0;
            } else {
#pragma unroll
                for (int sgn = 0; sgn < (MODE == 1 ? 2 : 1); ++sgn) {
                    real_t p[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) p[k] = sgn == 0 ? xv[k] + d[k] : xv[k] - d[k];
                    const real_t v0 = tridiag_row<real_t, NL>(p[0], p[1], p[2]);
                    real_t *dst = fx + (int64_t)(sgn * B + b) * fs + i;
                    if (two) {
                        const real_t v1 = tridiag_row<real_t, NL>(p[1], p[2], p[3]);
                        *reinterpret_cast<r2_t *>(dst) = r2_t{v0, v1};
                    } else {
                        dst[0] = v0;
                    }
                }
            }
        }
    }
}

// fd_lazy_points.store (include/fdjac_device.h): the tridiagonal fixture evaluated at the lazily perturbed points of a batch,
// difference quotients formed and stored into the banded Jacobian by this launch -- nothing follows it.  Operations per entry:
// those of the plain path (sub_exact, IEEE division), so the stored values have its bits.
//
// k_f_tridiag_store_wave (round 3; the default for an exactly tridiagonal band with all colours in one batch): COLUMN-centric --
// lane t of a wavefront owns the columns j = jw + 2t, j + 1, loads x[j-2 .. j+3] as three aligned 16-B pairs, evaluates the
// fixture on each column's three rows at x and at x +- eps_c e_j (the points differ from the colour's point x +- eps_c mask_c
// only in columns of colour c that do not touch these rows -- the plan verified C >= 3 cyclic colours on the exact band -- so
// every operand, including the "+ 0.0" of the unperturbed coordinates, and every operation is that of the coloured
// evaluation: same bits), and hands its six quotients to fd_band_emit_wave: staged in a wave-private LDS window in storage
// order, written as dense aligned non-temporal 16-B stores.  No workgroup barrier, no colour reads (cyclic colours are
// arithmetic), no position arithmetic per entry.  N = 10^7: 53-60 us for 320 MB (0.67-0.76 of the 8 TB/s peak; a pure
// 1:3 read:write stream of the same bytes takes 50 us) against 104-114 us for round 2's forms below, whose waves lived
// ~6 us each for one 8- or 16-B x load (scripts/ubench/fused_store_probe.hip, profiles/r03_a_fused_store_probe.txt).
//
// k_f_tridiag_lazy_store (round 2; kept for wider bands, colour chunks and colour ownership, CSC only): rows owned by
// workgroups, differences -> LDS [colour][row], the workgroup walks its storage positions.
__device__ __forceinline__ r2_t ld_pair_guarded(const real_t *__restrict__ x, int64_t a, int64_t n)
{
    if (a >= 0 && a + 1 < n) return *reinterpret_cast<const r2_t *>(x + a);
    r2_t v = {0, 0};
    if (a >= 0 && a < n) v.x = x[a];
    return v;
}

// the quotient of row j - 1 + k of column j (k = 0 .. 2): xv = x[j - 2 .. j + 2] (row j - 1 + k reads xv[k .. k + 2] only), the point
// x[j] +- e, every other coordinate x + 0.0 / x - 0.0.  The ONE place the storing wave kernels form a Float64 / pair-form quotient.
template <int MODE, bool NL>
__device__ __forceinline__ real_t tridiag_quotient(const real_t *xv, real_t e, int k)
{
    const real_t ed = MODE == 1 ? 2 * e : e;
    real_t p[3], m[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { const real_t dlt = k + i == 2 ? e : (real_t)0; p[i] = xv[k + i] + dlt; m[i] = xv[k + i] - dlt; }
    const real_t plus = tridiag_row<real_t, NL>(p[0], p[1], p[2]);
    const real_t sub = MODE == 1 ? tridiag_row<real_t, NL>(m[0], m[1], m[2]) : tridiag_row<real_t, NL>(xv[k], xv[k + 1], xv[k + 2]);
    return sub_exact(plus, sub) / ed;      // (the shared-reciprocal division measured 2 % slower here: bandwidth, not issue, bounds this kernel)
}

// the six quotients of a lane's two columns (rows j-1 .. j+1 of column j, then of column j + 1)
template <int MODE, bool NL>
__device__ __forceinline__ void tridiag_pair_quotients(const r2_t &L, const r2_t &Cc, const r2_t &R, real_t ea, real_t eb, real_t (&q)[6])
{
    const real_t xv[6] = {L.x, L.y, Cc.x, Cc.y, R.x, R.y};
#pragma unroll
    for (int o = 0; o < 2; ++o)                               // column j + o
#pragma unroll
        for (int k = 0; k < 3; ++k) q[3 * o + k] = tridiag_quotient<MODE, NL>(xv + o, o == 0 ? ea : eb, k);
}
// the line-aligned emit's seventh value (fd_band_emit_wave_lines' `qnext`): row j + 1 of column j + 2, the first stored value of the
// column after the lane's pair -- the quotient the next wavefront's lane 0 forms as its q[0], from the same operands
template <int MODE, bool NL>
__device__ __forceinline__ real_t tridiag_next_quotient(const r2_t &Cc, const r2_t &R, real_t en)
{
    const real_t xv[3] = {Cc.x, Cc.y, R.x};
    return tridiag_quotient<MODE, NL>(xv, en, 0);
}

// the colour of a wavefront's first column (the line-aligned placement may start a launch's first wavefront below column 0)
__device__ __forceinline__ int tridiag_wave_color(int64_t jw, const fd_band_store &bst)
{
    const int64_t m = (jw + bst.shift) % bst.C;
    return (int)(m < 0 ? m + bst.C : m);
}

template <int MODE, bool NL>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_store_wave(const real_t *__restrict__ x, const real_t *__restrict__ eps, int64_t n, fd_band_store bst, int64_t jstart, int lines)
{
    __shared__ __attribute__((aligned(16))) real_t s_win[kBlock / 64][FD_BAND_WAVE_LDS(3)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwaves = (bst.col_end - jstart + 127) / 128;
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (gw >= nwaves) return;
    const int64_t jw = jstart + gw * 128;                    // even: the x pairs are 16-B aligned
    const int64_t j = jw + 2 * lane;
    const r2_t Cc = ld_pair_guarded(x, j, n), L = ld_pair_guarded(x, j - 2, n), R = ld_pair_guarded(x, j + 2, n);
    // cyclic colours: column j has colour (j + shift) mod C, column j + 1 the next one
    const int c0w = tridiag_wave_color(jw, bst);             // (wave-uniform 64-bit modulo: scalar unit)
    const int c0 = (int)((uint32_t)(c0w + 2 * lane) % (uint32_t)bst.C);
    const int c1 = c0 + 1 == bst.C ? 0 : c0 + 1;
    const real_t ea = eps[c0], eb = eps[c1];
    const real_t en = lines ? eps[(uint32_t)(c0w + 128) % (uint32_t)bst.C] : (real_t)0;      // the step size of column jw + 128
    real_t q[6];
    tridiag_pair_quotients<MODE, NL>(L, Cc, R, ea, eb, q);
    if (lines) {
        // line-aligned spans (the launcher placed jstart for them): lane 63 adds the first value of the next wavefront's first column
        real_t qn = 0;
        if (lane == 63) qn = tridiag_next_quotient<MODE, NL>(Cc, R, en);
        fd_band_emit_wave_lines<real_t, true>(&bst, s_win[wave], jw, q, qn);
        return;
    }
    fd_band_emit_wave<real_t, 3, true>(&bst, s_win[wave], jw, q);      // (non-temporal: nothing re-reads nzval in this call)
}

// THE FUSED STEP (round 6): the whole Jacobian in ONE launch -- blockIdx 0 is the finisher of the step-size reduction, blockIdx
// 1 .. nblocks are its reduction workgroups (fdjac_eps_dev.h), everything after that stores: the wavefronts of k_f_tridiag_store_wave,
// which load their x, then wait for the step sizes of their colours to be published.  Same operations per value as the two-launch
// form: same bits.  N = 10^6: one launch instead of two, and a hand-off of two memory round trips instead of six.
template <int MODE, bool NL, int NC, bool PIPE>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_fused(const real_t *__restrict__ x, int64_t n, fd_band_store bst, int64_t jstart, int lines, FusedEps fz)
{
    // one LDS area, carved by role: storing workgroups (4 wave windows + the step sizes), reduction workgroups, finishers
    constexpr int kWinBytes = (kBlock / 64) * FD_BAND_WAVE_LDS(3) * (int)sizeof(real_t);
    constexpr int kLdsBytes = kWinBytes + 64 > (kFzMaxBlocks + 2 * kEpsGroups) * 8 ? kWinBytes + 64 : (kFzMaxBlocks + 2 * kEpsGroups) * 8;
    __shared__ __attribute__((aligned(16))) char s_lds[kLdsBytes];
    real_t (*s_win)[FD_BAND_WAVE_LDS(3)] = reinterpret_cast<real_t (*)[FD_BAND_WAVE_LDS(3)]>(s_lds);
    double *s_red = reinterpret_cast<double *>(s_lds);
    const int b = (int)blockIdx.x, nfin = fz.eg.C;
    if (b < nfin) { fused_finisher(fz, b, s_red, x, n); return; }
    if (b < nfin + fz.nblocks) { fused_eps_block<NC, PIPE>(x, n, fz, b - nfin, reinterpret_cast<double (*)[NC]>(s_red)); return; }
    // a storing workgroup: its wavefronts walk the 128-column tiles gw, gw + stride, ... (the launcher keeps the whole grid resident,
    // so nobody is dispatched after the step sizes are out); the first tile's x is in flight while the workgroup waits
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = b - nfin - fz.nblocks;
    const int64_t nwaves = (bst.col_end - jstart + 127) / 128;
    const int64_t gstride = (int64_t)((int)gridDim.x - nfin - fz.nblocks) * (kBlock / 64);
    int64_t gw = (int64_t)cb * (kBlock / 64) + wave;
    int64_t jw = jstart + gw * 128;
    r2_t Cc = {0, 0}, L = {0, 0}, R = {0, 0};
    // (a sharded x: the two lanes at the edges of the rank's columns take the neighbours' halo from the mailbox cells)
    auto load_x = [&](int64_t jt, r2_t &c_, r2_t &l_, r2_t &r_) {
        const int64_t j = jt + 2 * lane;
        c_ = ld_pair_guarded(x, j, n); l_ = ld_pair_guarded(x, j - 2, n); r_ = ld_pair_guarded(x, j + 2, n);
        if (fz.xw && fz.nranks > 1) {
            if (j == fz.own_begin && fz.rank > 0) { l_.x = fused_halo(fz, 0, 0); l_.y = fused_halo(fz, 0, 1); }
            if (j + 2 == fz.own_end && fz.rank + 1 < fz.nranks) { r_.x = fused_halo(fz, 1, 0); r_.y = fused_halo(fz, 1, 1); }
        }
    };
    if (gw < nwaves) load_x(jw, Cc, L, R);
    real_t *s_eps = reinterpret_cast<real_t *>(s_lds + kWinBytes);
    if (wave == 0) fused_wait_eps(fz, cb, s_eps);
    __syncthreads();
    for (; gw < nwaves; gw += gstride) {
        const int c0w = tridiag_wave_color(jw, bst);
        const int c0 = (int)((uint32_t)(c0w + 2 * lane) % (uint32_t)bst.C);
        const int c1 = c0 + 1 == bst.C ? 0 : c0 + 1;
        real_t q[6];
        tridiag_pair_quotients<MODE, NL>(L, Cc, R, s_eps[c0], s_eps[c1], q);
        if (lines) {
            real_t qn = 0;
            if (lane == 63) qn = tridiag_next_quotient<MODE, NL>(Cc, R, s_eps[(uint32_t)(c0w + 128) % (uint32_t)bst.C]);
            fd_band_emit_wave_lines<real_t, true>(&bst, s_win[wave], jw, q, qn);
        } else {
            fd_band_emit_wave<real_t, 3, true>(&bst, s_win[wave], jw, q);
        }
        // (the next tile's x requested BEFORE this tile is computed was measured: 12 more registers -- 6 instead of 8 wavefronts per
        //  SIMD -- for 0.3 us of a rank's 7.5-us storing phase, and 0.8 us lost at N = 10^6)
        jw = jstart + (gw + gstride) * 128;
        if (gw + gstride < nwaves) load_x(jw, Cc, L, R);
    }
    if (fz.trace && (blockIdx.x & 31) < 2) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); fz_mark_max(fz, 8); }
}

#ifdef FDJAC_F32
// Float32: the same kernel with FOUR columns per lane -- x as three aligned 16-B quads, twelve quotients, fd_band_emit_wave4's 16-B
// stores (a wavefront of the pair form moves 1.5 KB, half of the Float64 wavefront's bytes for the same instructions: N = 10^7
// 34.6 us for 160 MB).  Same operations per entry as the pair form: same bits.
typedef real_t r4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ r4_t ld_quad_guarded(const real_t *__restrict__ x, int64_t a, int64_t n)
{
    if (a >= 0 && a + 3 < n) return *reinterpret_cast<const r4_t *>(x + a);
    r4_t v = {0, 0, 0, 0};
    if (a >= 0 && a < n) v.x = x[a];
    if (a + 1 >= 0 && a + 1 < n) v.y = x[a + 1];
    if (a + 2 >= 0 && a + 2 < n) v.z = x[a + 2];
    if (a + 3 >= 0 && a + 3 < n) v.w = x[a + 3];
    return v;
}
template <int MODE, bool NL>
__device__ __forceinline__ void tridiag_quad_quotients(const r4_t &L, const r4_t &Cc, const r4_t &R, const real_t (&ev)[4], real_t (&q)[12])
{
    const real_t xv[8] = {L.z, L.w, Cc.x, Cc.y, Cc.z, Cc.w, R.x, R.y};      // x[j - 2 .. j + 5]
#pragma unroll
    for (int o = 0; o < 4; ++o) {                             // column j + o: x[j + o] +- e, every other coordinate x + 0.0 / x - 0.0
        const real_t e = ev[o];
        const real_t ed = MODE == 1 ? 2 * e : e;
        real_t p[5], m[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { const real_t dlt = k == 2 ? e : (real_t)0; p[k] = xv[o + k] + dlt; m[k] = xv[o + k] - dlt; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const real_t plus = tridiag_row<real_t, NL>(p[k], p[k + 1], p[k + 2]);
            const real_t sub = MODE == 1 ? tridiag_row<real_t, NL>(m[k], m[k + 1], m[k + 2])
                                         : tridiag_row<real_t, NL>(xv[o + k], xv[o + k + 1], xv[o + k + 2]);
            q[3 * o + k] = sub_exact(plus, sub) / ed;
        }
    }
}
template <int MODE, bool NL>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_store_wave4(const real_t *__restrict__ x, const real_t *__restrict__ eps, int64_t n, fd_band_store bst, int64_t jstart)
{
    __shared__ __attribute__((aligned(16))) real_t s_win[kBlock / 64][FD_BAND_WAVE4_LDS(3)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwaves = (bst.col_end - jstart + 255) / 256;
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (gw >= nwaves) return;
    const int64_t jw = jstart + gw * 256;                    // a multiple of 4: the x quads are 16-B aligned
    const int64_t j = jw + 4 * lane;
    const r4_t Cc = ld_quad_guarded(x, j, n), L = ld_quad_guarded(x, j - 4, n), R = ld_quad_guarded(x, j + 4, n);
    const int c0w = (int)((jw + bst.shift) % bst.C);
    int cc = (int)((uint32_t)(c0w + 4 * lane) % (uint32_t)bst.C);
    real_t ev[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) { ev[o] = eps[cc]; cc = cc + 1 == bst.C ? 0 : cc + 1; }
    real_t q[12];
    tridiag_quad_quotients<MODE, NL>(L, Cc, R, ev, q);
    fd_band_emit_wave4<real_t, 3, true>(&bst, s_win[wave], jw, q);
}
// the fused step (k_f_tridiag_fused), four columns per lane
template <int MODE, bool NL, int NC, bool PIPE>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_fused4(const real_t *__restrict__ x, int64_t n, fd_band_store bst, int64_t jstart, FusedEps fz)
{
    constexpr int kWinBytes = (kBlock / 64) * FD_BAND_WAVE4_LDS(3) * (int)sizeof(real_t);
    constexpr int kLdsBytes = kWinBytes + 64 > (kFzMaxBlocks + 2 * kEpsGroups) * 8 ? kWinBytes + 64 : (kFzMaxBlocks + 2 * kEpsGroups) * 8;
    __shared__ __attribute__((aligned(16))) char s_lds[kLdsBytes];
    real_t (*s_win)[FD_BAND_WAVE4_LDS(3)] = reinterpret_cast<real_t (*)[FD_BAND_WAVE4_LDS(3)]>(s_lds);
    double *s_red = reinterpret_cast<double *>(s_lds);
    const int b = (int)blockIdx.x, nfin = fz.eg.C;
    if (b < nfin) { fused_finisher(fz, b, s_red, x, n); return; }
    if (b < nfin + fz.nblocks) { fused_eps_block<NC, PIPE>(x, n, fz, b - nfin, reinterpret_cast<double (*)[NC]>(s_red)); return; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = b - nfin - fz.nblocks;
    const int64_t nwaves = (bst.col_end - jstart + 255) / 256;
    const int64_t gstride = (int64_t)((int)gridDim.x - nfin - fz.nblocks) * (kBlock / 64);
    int64_t gw = (int64_t)cb * (kBlock / 64) + wave;
    int64_t jw = jstart + gw * 256;
    r4_t Cc = {0, 0, 0, 0}, L = {0, 0, 0, 0}, R = {0, 0, 0, 0};
    auto load_x = [&](int64_t jt, r4_t &c_, r4_t &l_, r4_t &r_) {
        const int64_t j = jt + 4 * lane;
        c_ = ld_quad_guarded(x, j, n); l_ = ld_quad_guarded(x, j - 4, n); r_ = ld_quad_guarded(x, j + 4, n);
        if (fz.xw && fz.nranks > 1) {
            if (j == fz.own_begin && fz.rank > 0) { l_.z = fused_halo(fz, 0, 0); l_.w = fused_halo(fz, 0, 1); }
            if (j + 4 == fz.own_end && fz.rank + 1 < fz.nranks) { r_.x = fused_halo(fz, 1, 0); r_.y = fused_halo(fz, 1, 1); }
        }
    };
    if (gw < nwaves) load_x(jw, Cc, L, R);
    real_t *s_eps = reinterpret_cast<real_t *>(s_lds + kWinBytes);
    if (wave == 0) fused_wait_eps(fz, cb, s_eps);
    __syncthreads();
    for (; gw < nwaves; gw += gstride) {
        const int c0w = (int)((jw + bst.shift) % bst.C);
        int c = (int)((uint32_t)(c0w + 4 * lane) % (uint32_t)bst.C);
        real_t ev[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) { ev[o] = s_eps[c]; c = c + 1 == bst.C ? 0 : c + 1; }
        real_t q[12];
        tridiag_quad_quotients<MODE, NL>(L, Cc, R, ev, q);
        fd_band_emit_wave4<real_t, 3, true>(&bst, s_win[wave], jw, q);
        jw = jstart + (gw + gstride) * 256;
        if (gw + gstride < nwaves) load_x(jw, Cc, L, R);
    }
    if (fz.trace && (blockIdx.x & 31) < 2) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); fz_mark_max(fz, 8); }
}
#endif

// (32-bit index arithmetic: the launcher checked that every entry / row / column number is below 2^31)
__device__ __forceinline__ int band_colptr32(int j, int l, int u, int M)
{
    const int w = l + u + 1;
    const int nt = j < u ? j : u;
    const int top = nt * u - nt * (nt - 1) / 2;
    const int b0 = M - l, f0 = b0 > 0 ? b0 : 0;
    int bot = 0;
    if (j > f0) { const int nn = j - f0, a = f0 - b0 + 1; bot = nn * a + nn * (nn - 1) / 2; }
    return w * j - top - bot;
}
// Rows are owned by workgroups (2 * kBlock each: every thread evaluates its row pair at the base and at every point of the
// batch, differences -> LDS [colour][row], dense 16-B LDS stores); then the workgroup walks the storage positions its rows
// occupy -- one contiguous range of nzval -- and every position finds its (column, row) by the band's arithmetic (one
// multiply-shift in the interior, colptr's closed form in the corner workgroups), reads its difference, divides, and is
// written with its neighbour as a dense 16-B pair; positions of that range whose row belongs to the next workgroup are
// left to it.
template <typename CT, int MODE, bool NL, int BS>
__global__ void __launch_bounds__(BS)
k_f_tridiag_lazy_store(const real_t *__restrict__ x, const CT *__restrict__ color, const real_t *__restrict__ eps, int c_lo, int B,
                       int n, int r0, int r1, real_t *__restrict__ outp, int M, int N, int eb, int cb, int ce, int l, int u, int C,
                       int shift, int pitch, uint64_t mw, uint64_t mc)
{
    extern __shared__ real_t s_val[];                          // [B][pitch] differences of the workgroup's rows, then [B] divisors
    real_t *s_ed = s_val + (size_t)B * pitch;
    const int R0 = r0 + (int)blockIdx.x * (2 * BS);
    if (R0 >= r1) return;
    const int R1 = R0 + 2 * BS < r1 ? R0 + 2 * BS : r1;
    const int w = l + u + 1, top_full = u * (u + 1) / 2;
    if ((int)threadIdx.x < B) {
        const real_t e = eps[c_lo + threadIdx.x];
        s_ed[threadIdx.x] = MODE == 1 ? 2 * e : e;
    }
    // ---- phase A
    const int i = R0 + 2 * (int)threadIdx.x;
    if (i < R1) {
        real_t xv[4];
        int cv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = i - 1 + k;
            const bool in = (j >= 0) & (j < n);
            xv[k] = in ? x[in ? j : 0] : 0.0;
            const int c = in ? (int)color[in ? j : 0] : -1;
            cv[k] = (c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;
        }
        real_t b0 = 0.0, b1 = 0.0;
        if (MODE == 0) {
            b0 = tridiag_row<real_t, NL>(xv[0], xv[1], xv[2]);
            b1 = tridiag_row<real_t, NL>(xv[1], xv[2], xv[3]);
        }
        for (int b = 0; b < B; ++b) {
            const real_t e = eps[c_lo + b];
            real_t p[4], q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const real_t d = (cv[k] == b) ? e : 0.0; p[k] = xv[k] + d; q[k] = xv[k] - d; }
            const real_t s0 = MODE == 1 ? tridiag_row<real_t, NL>(q[0], q[1], q[2]) : b0;
            const real_t s1 = MODE == 1 ? tridiag_row<real_t, NL>(q[1], q[2], q[3]) : b1;
            *reinterpret_cast<r2_t *>(s_val + b * pitch + 2 * (int)threadIdx.x) =
                r2_t{sub_exact(tridiag_row<real_t, NL>(p[0], p[1], p[2]), s0), sub_exact(tridiag_row<real_t, NL>(p[1], p[2], p[3]), s1)};
        }
    }
    __syncthreads();
    // ---- phase B: the storage positions of rows [R0, R1) (local to the column range [cb, ce))
    const int jlo = R0 - l > cb ? R0 - l : cb, jhi = R1 - 1 + u < ce - 1 ? R1 - 1 + u : ce - 1;     // columns that touch those rows
    if (jhi < jlo) return;
    const int plo = (band_colptr32(jlo, l, u, M) - eb) & ~1, phi = band_colptr32(jhi + 1, l, u, M) - eb;   // [plo, phi)
    const bool interior = jlo >= u && jhi + l <= M - 1;        // no column cut off by the matrix edge
    const bool vec = ((((uintptr_t)outp) & kPairMask) == 0);
    auto column_of = [&](int g) -> int {
        int j = (int)fd_div31((uint32_t)(g + top_full), mw);
        if (j >= N) j = N - 1;
        while (j > 0 && band_colptr32(j, l, u, M) > g) --j;
        while (j + 1 < N && band_colptr32(j + 1, l, u, M) <= g) ++j;
        return j;
    };
    for (int pp = plo + 2 * (int)threadIdx.x; pp < phi; pp += 2 * BS) {
        real_t qv[2];
        bool wr[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int g = pp + h + eb;
            int j, row;
            if (interior) {
                const uint32_t Q = (uint32_t)(g + top_full);
                const uint32_t jq = fd_div31(Q, mw);
                j = (int)jq;
                row = j - u + (int)(Q - jq * (uint32_t)w);
            } else {
                const int gg = g < phi + eb ? g : phi + eb - 1;
                j = column_of(gg);
                row = (j - u > 0 ? j - u : 0) + (gg - band_colptr32(j, l, u, M));
            }
            const uint32_t cj = (uint32_t)(j + shift);
            const int b = (int)(cj - fd_div31(cj, mc) * (uint32_t)C) - c_lo;
            const bool live = pp + h >= 0 && pp + h < phi && row >= R0 && row < R1 && b >= 0 && b < B && j >= cb && j < ce;
            const int at = live ? b * pitch + (row - R0) : 0;
            qv[h] = s_val[at] / s_ed[live ? b : 0];
            wr[h] = live;
        }
        if (wr[0] & wr[1] & vec) *reinterpret_cast<r2_t *>(outp + pp) = r2_t{qv[0], qv[1]};
        else {
            if (wr[0]) outp[pp] = qv[0];
            if (wr[1]) outp[pp + 1] = qv[1];
        }
    }
}

// storing workgroups of a fused launch: as many as tiles, but never more than fit on the device next to the reduction's (what the
// kernel's registers and LDS allow per CU, asked of the runtime once per kernel): a workgroup dispatched only after others have left
// would start its life after the step sizes are out -- a second round of memory latency at the end of the launch
template <typename K>
static unsigned fused_grid(K kernel, unsigned tiles_wg, int prefix)
{
    static const int cus = [] { int dev = 0, n = 256; if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
    static std::mutex mu;
    static std::unordered_map<const void *, int> per_cu;
    int occ = 0;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = per_cu.find((const void *)kernel);
        if (it == per_cu.end()) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kBlock, 0) != hipSuccess || nb < 1) nb = 4;
            (void)hipGetLastError();
            it = per_cu.emplace((const void *)kernel, nb).first;
        }
        occ = it->second;
    }
    const int64_t room = (int64_t)cus * occ - prefix;
    const int64_t cap = room > cus ? room : cus;
    if ((int64_t)tiles_wg <= cap) return (unsigned)prefix + tiles_wg;
    const int64_t rounds = ((int64_t)tiles_wg + cap - 1) / cap;
    return (unsigned)prefix + (unsigned)(((int64_t)tiles_wg + rounds - 1) / rounds);
}

// The line-aligned emit (fd_band_emit_wave_lines; CSC nzval, Float64): the first wavefront's first column for it -- even (the x pairs
// stay 16-B aligned), at most 14 below the even column the launch would start at otherwise (possibly below 0: columns outside the
// local range are skipped anyway), and such that out + 8 (3 jstart - entry_begin) lies on a 128-B line:
// 3 jstart = entry_begin - out / 8 (mod 16), and 3 * 11 = 1 (mod 16).  False -- *jstart untouched, the launch keeps fd_band_emit_wave --
// when that solution is odd, out is not 8-B aligned, the storage is not CSC, or FDJAC_STORE_LINES=0 (test switch) says so.
static bool tridiag_lines_jstart(const fd_band_store &bst, int64_t *jstart)
{
    if (sizeof(real_t) != 8 || bst.layout != FD_BAND_CSC) return false;
    const char *sw = fdjac::test_switch("FDJAC_STORE_LINES");
    if (sw && *sw && atoi(sw) == 0) return false;
    const uintptr_t o = (uintptr_t)bst.out;
    if (o & 7) return false;
    const int64_t r = (int64_t)(((uint64_t)bst.entry_begin - (uint64_t)(o >> 3)) & 15);
    const int64_t want = (11 * r) & 15;
    if (want & 1) return false;
    *jstart -= (*jstart - want) & 15;
    return true;
}

template <typename CT>
static int lazy_tridiag_launch(BuiltinF *b, void *fx, const fd_lazy_points *lp, int64_t fs, int64_t r0, int64_t r1,
                               hipStream_t s)
{
    const int64_t r0e = r0 & ~(int64_t)1;
    // one pair of rows per thread, uncapped grid (measured faster than a capped grid-stride launch here)
    int64_t g = ((r1 - r0e + 1) / 2 + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    const bool nl = b->family == FD_F_TRIDIAG_NL;
    const int mode = lp->is_complex ? 2 : (lp->pts == 2 ? 1 : 0);
    // the storing kernels' <MODE, NL>: forward or central (the complex step is declined below)
    const auto pick_store = [&](auto &&launch) {
        fd_pick<0, 1>(mode == 0 ? 0 : 1, [&](auto M) { fd_pick<false, true>(nl, [&](auto NL) { launch(M, NL); }); });
    };
    if (lp->store) {
        // the launch stores the Jacobian itself (include/fdjac_device.h); one-shot launches
        if (lp->store_kind != FD_STORE_BAND) return FD_LAZY_DECLINED;
        const fd_band_store bst = *(const fd_band_store *)lp->store;
        if (bst.elem_bytes != (int)sizeof(real_t) || mode == 2) return FD_LAZY_DECLINED;
        if (bst.N != b->prm[0] || bst.M != b->prm[0]) return FD_LAZY_DECLINED;   // a plan of another problem size than this fixture's
        const int wband = bst.l + bst.u + 1;
        // an exactly tridiagonal band with every colour in this batch: the column-centric wave kernel, any layout; colour chunks,
        // colour ownership and wider bands take the row-owned kernel below
        const bool wave_ok = bst.l == 1 && bst.u == 1 && bst.M == bst.N && lp->c_lo == 0 &&
                             lp->ncolors == bst.C && bst.C >= 3 && (((uintptr_t)lp->x) & kPairMask) == 0 && bst.col_end > bst.col_begin;
#ifdef FDJAC_F32
        if (wave_ok && (((uintptr_t)lp->x) & 15) == 0) {      // Float32: four columns per lane
            const int64_t jstart = bst.col_begin & ~(int64_t)3;
            const int64_t nwaves = (bst.col_end - jstart + 255) / 256;
            const unsigned gw = (unsigned)((nwaves + kBlock / 64 - 1) / (kBlock / 64));
            if (lp->eps_job) {
                const FusedEps fz = *(const FusedEps *)lp->eps_job;
                pick_store([&](auto M, auto NL) {
                    fd_pick<4, kRegColors>(fz.eg.C <= 4 ? 4 : kRegColors, [&](auto NC) {
                        fd_pick<false, true>(fz.eg.tpb > 2, [&](auto PIPE) {
                            const auto k = k_f_tridiag_fused4<M(), NL(), NC(), PIPE()>;
                            hipLaunchKernelGGL(k, dim3(fused_grid(k, gw, fz.eg.C + fz.nblocks)), dim3(kBlock), 0, s, (const real_t *)lp->x,
                                               b->prm[0], bst, jstart, fz);
                        });
                    });
                });
                return launch_rc();
            }
            pick_store([&](auto M, auto NL) {
                hipLaunchKernelGGL((k_f_tridiag_store_wave4<M(), NL()>), dim3(gw), dim3(kBlock), 0, s, (const real_t *)lp->x,
                                   (const real_t *)lp->eps, b->prm[0], bst, jstart);
            });
            return launch_rc();
        }
#endif
        if (wave_ok) {
            int64_t jstart = bst.col_begin & ~(int64_t)1;
            const int lines = tridiag_lines_jstart(bst, &jstart) ? 1 : 0;
            const int64_t nwaves = (bst.col_end - jstart + 127) / 128;
            const unsigned gw = (unsigned)((nwaves + kBlock / 64 - 1) / (kBlock / 64));
            if (lp->eps_job) {
                // the fused step: this launch also runs the step-size reduction (finisher + reduction workgroups first, see k_f_tridiag_fused)
                const FusedEps fz = *(const FusedEps *)lp->eps_job;
                pick_store([&](auto M, auto NL) {
                    fd_pick<4, kRegColors>(fz.eg.C <= 4 ? 4 : kRegColors, [&](auto NC) {
                        fd_pick<false, true>(fz.eg.tpb > 2, [&](auto PIPE) {
                            const auto k = k_f_tridiag_fused<M(), NL(), NC(), PIPE()>;
                            hipLaunchKernelGGL(k, dim3(fused_grid(k, gw, fz.eg.C + fz.nblocks)), dim3(kBlock), 0, s, (const real_t *)lp->x,
                                               b->prm[0], bst, jstart, lines, fz);
                        });
                    });
                });
                return launch_rc();
            }
            pick_store([&](auto M, auto NL) {
                hipLaunchKernelGGL((k_f_tridiag_store_wave<M(), NL()>), dim3(gw), dim3(kBlock), 0, s, (const real_t *)lp->x,
                                   (const real_t *)lp->eps, b->prm[0], bst, jstart, lines);
            });
            return launch_rc();
        }
        if (lp->eps_job) return FD_LAZY_DECLINED;      // (the fused step exists for the wave kernels only: the library runs the reduction itself)
        if (bst.layout != FD_BAND_CSC) return FD_LAZY_DECLINED;
        const int bs = kBlock;      // (one-wave workgroups, BS = 64, measured slower: 111-119 vs 105 us at N = 10^7)
        const int pitch = 2 * bs + 2;
        const size_t shm = sizeof(real_t) * ((size_t)lp->ncolors * (size_t)pitch + (size_t)lp->ncolors + 2);
        const int64_t nnz_all = fd_band_colptr(&bst, bst.N);
        if (shm > (size_t)60 * 1024 || nnz_all + (int64_t)wband * wband + 64 >= ((int64_t)1 << 31) || bst.N + bst.C + 64 >= ((int64_t)1 << 31) ||
            bst.M + wband + 64 >= ((int64_t)1 << 31) || lp->ncolors > kBlock) return FD_LAZY_DECLINED;
        const unsigned gs = (unsigned)((r1 - r0e + 2 * bs - 1) / (2 * bs));
        pick_store([&](auto M, auto NL) {
            hipLaunchKernelGGL((k_f_tridiag_lazy_store<CT, M(), NL(), kBlock>), dim3(gs), dim3(kBlock), shm, s, (const real_t *)lp->x,
                               (const CT *)lp->color, (const real_t *)lp->eps, lp->c_lo, lp->ncolors, (int)b->prm[0], (int)r0e, (int)r1,
                               (real_t *)bst.out, (int)bst.M, (int)bst.N, (int)bst.entry_begin, (int)bst.col_begin, (int)bst.col_end,
                               bst.l, bst.u, bst.C, bst.shift, pitch, fd_magic31((uint32_t)wband), fd_magic31((uint32_t)bst.C));
        });
        return launch_rc();
    }
    fd_pick<0, 1, 2>(mode, [&](auto M) {
        fd_pick<false, true>(nl, [&](auto NL) {
            hipLaunchKernelGGL((k_f_tridiag_lazy<CT, M(), NL()>), dim3((unsigned)g), dim3(kBlock), 0, s, (real_t *)fx, fs,
                               (real_t *)lp->base_out, (const real_t *)lp->x, (const CT *)lp->color, (const real_t *)lp->eps, lp->c_lo,
                               lp->ncolors, b->prm[0], r0e, r1, lp->imag_only, mode != 2 ? lp->diff : 0);
        });
    });
    return launch_rc();
}
