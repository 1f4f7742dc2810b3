// The 5-point fixtures (FD_F_LAP5, FD_F_LAP5_NL, FD_F_CLAMP5) at lazily perturbed points: the kernels, then their launcher.
// Included by fdjac_builtin_f.hip (namespace fdjac, after fdjac_f_tridiag.hip).

// Lazy-point version of the 5-point stencils (see k_f_tridiag_lazy): the 8 base values a pair of rows
// depends on are loaded once, every point of the batch is evaluated from registers.
// v[8] = {c0, c1, s0, s1, n0, n1, w, e} = x at {k, k+1, k-nx, k-nx+1, k+nx, k+nx+1, k-1, k+2}.
template <typename T, int SK>
__device__ __forceinline__ void stencil5_pair(const T *v, bool hs, bool hn, bool hw, bool he, T &o0, T &o1)
{
    if (SK == 1) {
        const T w0 = hw ? v[6] : v[0], e1 = he ? v[7] : v[1];
        const T s0 = hs ? v[2] : v[0], s1 = hs ? v[3] : v[1], n0 = hn ? v[4] : v[0], n1 = hn ? v[5] : v[1];
        o0 = (((v[0] + w0) + v[1]) + s0) + n0;
        o1 = (((v[1] + v[0]) + e1) + s1) + n1;
    } else {
        const T z = zero_of<T>();
        const T w = hw ? v[6] : z, e = he ? v[7] : z;
        const T s0 = hs ? v[2] : z, s1 = hs ? v[3] : z, n0 = hn ? v[4] : z, n1 = hn ? v[5] : z;
        o0 = (((w + v[1]) + s0) + n0) - kFour * v[0];
        o1 = (((v[0] + e) + s1) + n1) - kFour * v[1];
        if (SK == 2) { o0 = o0 + (v[0] * v[0]) * v[1]; o1 = o1 + (v[1] * v[1]) * e; }
    }
}

template <typename CT, int MODE, int SK>
__global__ void __launch_bounds__(kBlock)
k_f_stencil5_lazy(real_t *__restrict__ fx, int64_t fs, real_t *__restrict__ base_out, const real_t *__restrict__ x,
                  const CT *__restrict__ color, const real_t *__restrict__ eps, int c_lo, int B, int64_t nx, int64_t ny,
                  int64_t r0, int64_t r1, int imag_only, int diff)
{
    const int64_t ntiles = (r1 - r0 + 2 * kBlock - 1) / (2 * kBlock);
    const int64_t tile = xcd_tile(blockIdx.x, ntiles);
    if (tile >= ntiles) return;
    const int64_t k = r0 + tile * (2 * kBlock) + threadIdx.x * 2;
    if (k >= r1) return;
    const int64_t j = k / nx, i = k - j * nx;
    const bool hs = j > 0, hn = j + 1 < ny, hw = i > 0, he = i + 2 < nx;
    const int64_t idx[8] = {k, k + 1, k - nx, k - nx + 1, k + nx, k + nx + 1, k - 1, k + 2};
    const bool ok[8] = {true, true, hs, hs, hn, hn, hw, he};
    real_t xv[8];
    int cv[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int64_t at = ok[m] ? idx[m] : k;
        xv[m] = x[at];
        const int c = (int)color[at];
        cv[m] = (!ok[m] || c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;
    }
    real_t b0 = 0.0, b1 = 0.0;                        // f(x) at rows k, k+1 (written to base_out, or the subtrahend of diff)
    if (base_out || (diff && MODE == 0)) stencil5_pair<real_t, SK>(xv, hs, hn, hw, he, b0, b1);
    if (base_out) *reinterpret_cast<r2_t *>(base_out + k) = r2_t{b0, b1};
    for (int b = 0; b < B; ++b) {
        const real_t e = eps[c_lo + b];
        real_t d[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) d[m] = (cv[m] == b) ? e : 0.0;
        if (MODE == 2) {
            cd p[8], o0, o1;
#pragma unroll
            for (int m = 0; m < 8; ++m) p[m] = cd{xv[m], d[m]};
            stencil5_pair<cd, SK>(p, hs, hn, hw, he, o0, o1);
            if (imag_only) {
                *reinterpret_cast<r2_t *>(fx + (int64_t)b * fs + k) = r2_t{o0.im, o1.im};
            } else {
                real_t *dst = fx + ((int64_t)b * fs + k) * 2;
                *reinterpret_cast<r2_t *>(dst) = r2_t{o0.re, o0.im};
                *reinterpret_cast<r2_t *>(dst + 2) = r2_t{o1.re, o1.im};
            }
        } else if (diff) {
            // differences (fd_lazy_points.diff): f(x + d) - f(x), or f(x + d) - f(x - d), one array per colour
            real_t p[8], q[8], o0, o1, s0 = b0, s1 = b1;
#pragma unroll
            for (int m = 0; m < 8; ++m) { p[m] = xv[m] + d[m]; q[m] = xv[m] - d[m]; }
            stencil5_pair<real_t, SK>(p, hs, hn, hw, he, o0, o1);
            if (MODE == 1) stencil5_pair<real_t, SK>(q, hs, hn, hw, he, s0, s1);
            *reinterpret_cast<r2_t *>(fx + (int64_t)b * fs + k) = r2_t{sub_exact(o0, s0), sub_exact(o1, s1)};
        } else {
#pragma unroll
            for (int sgn = 0; sgn < (MODE == 1 ? 2 : 1); ++sgn) {
                real_t p[8], o0, o1;
#pragma unroll
                for (int m = 0; m < 8; ++m) p[m] = sgn == 0 ? xv[m] + d[m] : xv[m] - d[m];
                stencil5_pair<real_t, SK>(p, hs, hn, hw, he, o0, o1);
                *reinterpret_cast<r2_t *>(fx + (int64_t)(sgn * B + b) * fs + k) = r2_t{o0, o1};
            }
        }
    }
}

// fd_lazy_points.store with a fd_stencil5_store (include/fdjac_device.h): the 5-point fixtures evaluated at the lazily perturbed
// points, difference quotients formed and stored into the CSC nzval of the stencil by this launch -- nothing follows it.
// COLUMN-centric like k_f_tridiag_store_wave: lane t of a wavefront owns the grid columns (i, j), (i + 1, j), i = i0 + 2t,
// loads the 6 x 5 window of x around them (11 aligned 16-B loads; the vertical re-reads come from L2: consecutive grid rows run
// on one XCD), and evaluates the five rows each column touches at x +- eps e_k.  Seen from one of those rows the colour's point
// x +- eps_c mask_c differs from x in column k only (the plan verified that colorvec is a valid colouring of the exact stencil),
// so every operand -- the "+ 0.0" of the unperturbed coordinates included -- and every operation (stencil5 row, sub_exact,
// IEEE division) is that of the colour-batched evaluation: same bits (scripts/ubench/stencil_store_probe.hip checks the form
// against the reference's loop order on the host).  The wavefront's 128 x 5 quotients leave through fd_stencil5_emit_wave.
template <typename T, int SK> __device__ __forceinline__ T stencil5_row(T c, T w, T e, T s, T n)
{
    T v = (((w + e) + s) + n) - kFour * c;
    if (SK == 2) v = v + (c * c) * e;
    return v;
}

// a / b for a divisor shared by several quotients, y = 1 / b computed once: one multiplication and two FMA correction steps give
// the CORRECTLY ROUNDED quotient (Markstein: q1 is a faithful rounding of a / b, so q2 = RN(a / b) when nothing over- or
// underflows; zero, tiny, huge and non-finite operands take the true division) -- the bits of IEEE a / b, about half its
// instructions (scripts/ubench/exact_div_probe.hip: 5e10 random and next-to-tie operand pairs, 0 mismatches).  Float64 only.
// `bok` = div_shared_ok(b), tested ONCE per divisor: with |b| in [2^-100, 2^100] and |a| in [2^-800, 2^800] the first quotient lies in
// [2^-900, 2^900] by itself -- two comparisons per quotient instead of four.  A/B on one box (scripts/ab_c5.sh, ab_c3.sh): the
// block-coupled kernel 49.9 -> 48.5 us (used there); the 5-point kernel 98 -> 100 us (not used there).
__device__ __forceinline__ bool div_shared_ok(real_t b) { const real_t mb = fabs(b); return mb >= (real_t)0x1p-100 && mb <= (real_t)0x1p100; }
// b = +-2^k with 2^k and 2^-k normal numbers: then a * (1 / b) IS a / b for every a -- one rounding of the same real number either way
// (scaling by a power of two is exact until the result leaves the normal range, and there both forms round the same value once).
// The complex step's divisor is eps(T) = 2^-52 / 2^-23 unless the caller chose another one.
__device__ __forceinline__ bool div_is_pow2(real_t b)
{
    if constexpr (sizeof(real_t) == 8) {
        const unsigned long long u = (unsigned long long)__double_as_longlong((double)b), ex = (u >> 52) & 0x7FFull;
        return (u & 0x000FFFFFFFFFFFFFull) == 0 && ex >= 2 && ex <= 2044;
    } else {
        const unsigned u = __float_as_uint((float)b), ex = (u >> 23) & 0xFFu;
        return (u & 0x007FFFFFu) == 0 && ex >= 2 && ex <= 252;
    }
}
template <bool FAST> __device__ __forceinline__ real_t div_shared(real_t a, real_t b, real_t y);
template <bool FAST> __device__ __forceinline__ real_t div_shared(real_t a, real_t b, real_t y, bool bok)
{
    if constexpr (FAST && sizeof(real_t) == 8) {
        const double ma = fabs(a);
        if (!(bok && ma >= 0x1p-800 && ma <= 0x1p800)) return a / b;
        const double q0 = a * y;
        const double r0 = __builtin_fma(-b, q0, a);
        const double q1 = __builtin_fma(r0, y, q0);
        const double r1 = __builtin_fma(-b, q1, a);
        return __builtin_fma(r1, y, q1);
    } else {
        return a / b;
    }
}
template <bool FAST> __device__ __forceinline__ real_t div_shared(real_t a, real_t b, real_t y)
{
    if constexpr (FAST && sizeof(real_t) == 8) {
        const double q0 = a * y;
        const double m = fabs(q0), ma = fabs(a);
        if (!(m >= 0x1p-900 && m <= 0x1p900 && ma >= 0x1p-900 && ma <= 0x1p900)) return a / b;
        const double r0 = __builtin_fma(-b, q0, a);
        const double q1 = __builtin_fma(r0, y, q0);
        const double r1 = __builtin_fma(-b, q1, a);
        return __builtin_fma(r1, y, q1);
    } else {
        return a / b;
    }
}

// the five quotients of column (ii, j) from the window W (rows j-2 .. j+2, columns i-2 .. i+3 of x, zero outside the grid), o =
// ii - i.  INTERIOR: every neighbour of every evaluated row exists (no guards).
// NUMER: q receives the five DIFFERENCES (the caller divides: k_f_stencil5_store_wave4).
// YGIVEN: the caller hands in yd = 1 / ed (one reciprocal per COLOUR, fetched from the colour's lane, instead of one per column).
template <int MODE, int SK, bool INTERIOR, bool FASTDIV, int WC, bool NUMER = false, bool YGIVEN = false>
__device__ __forceinline__ void stencil5_column_quotients(const real_t (&W)[5][WC], int o, int ii, int j, int nx, int ny, real_t e, real_t *q,
                                                          real_t yd_in = 0)
{
    const real_t ed = MODE == 1 ? 2 * e : e;
    const real_t yd = YGIVEN ? yd_in : (FASTDIV && sizeof(real_t) == 8) ? (real_t)1 / ed : (real_t)0;
    const real_t xc = W[2][2 + o], pc = xc + e, mc = xc - e;
    const bool hw = INTERIOR || ii > 0, he = INTERIOR || ii < nx - 1, hs = INTERIOR || j > 0, hn = INTERIOR || j < ny - 1;
    const real_t z = 0;
    // PV: what the plus point holds at an unperturbed coordinate (x + 0.0); MV: the minus point (x - 0.0 == x) -- and, for
    // forward differences, the base point x itself
#define PV(dj, di) (W[(dj) + 2][(di) + 2 + o] + z)
#define MV(dj, di) W[(dj) + 2][(di) + 2 + o]
    const real_t mcc = MODE == 1 ? mc : xc;
    {   // row (ii, j-1): its north neighbour is the perturbed coordinate
        const bool rhs = INTERIOR || j - 1 > 0;
        const real_t pl = stencil5_row<real_t, SK>(PV(-1, 0), hw ? PV(-1, -1) : z, he ? PV(-1, 1) : z, rhs ? PV(-2, 0) : z, pc);
        const real_t mi = stencil5_row<real_t, SK>(MV(-1, 0), hw ? MV(-1, -1) : z, he ? MV(-1, 1) : z, rhs ? MV(-2, 0) : z, mcc);
        q[0] = NUMER ? sub_exact(pl, mi) : div_shared<FASTDIV>(sub_exact(pl, mi), ed, yd);
    }
    {   // row (ii-1, j): east
        const bool rhw = INTERIOR || ii - 1 > 0;
        const real_t pl = stencil5_row<real_t, SK>(PV(0, -1), rhw ? PV(0, -2) : z, pc, hs ? PV(-1, -1) : z, hn ? PV(1, -1) : z);
        const real_t mi = stencil5_row<real_t, SK>(MV(0, -1), rhw ? MV(0, -2) : z, mcc, hs ? MV(-1, -1) : z, hn ? MV(1, -1) : z);
        q[1] = NUMER ? sub_exact(pl, mi) : div_shared<FASTDIV>(sub_exact(pl, mi), ed, yd);
    }
    {   // row (ii, j): centre
        const real_t pl = stencil5_row<real_t, SK>(pc, hw ? PV(0, -1) : z, he ? PV(0, 1) : z, hs ? PV(-1, 0) : z, hn ? PV(1, 0) : z);
        const real_t mi = stencil5_row<real_t, SK>(mcc, hw ? MV(0, -1) : z, he ? MV(0, 1) : z, hs ? MV(-1, 0) : z, hn ? MV(1, 0) : z);
        q[2] = NUMER ? sub_exact(pl, mi) : div_shared<FASTDIV>(sub_exact(pl, mi), ed, yd);
    }
    {   // row (ii+1, j): west
        const bool rhe = INTERIOR || ii + 1 < nx - 1;
        const real_t pl = stencil5_row<real_t, SK>(PV(0, 1), pc, rhe ? PV(0, 2) : z, hs ? PV(-1, 1) : z, hn ? PV(1, 1) : z);
        const real_t mi = stencil5_row<real_t, SK>(MV(0, 1), mcc, rhe ? MV(0, 2) : z, hs ? MV(-1, 1) : z, hn ? MV(1, 1) : z);
        q[3] = NUMER ? sub_exact(pl, mi) : div_shared<FASTDIV>(sub_exact(pl, mi), ed, yd);
    }
    {   // row (ii, j+1): south
        const bool rhn = INTERIOR || j + 1 < ny - 1;
        const real_t pl = stencil5_row<real_t, SK>(PV(1, 0), hw ? PV(1, -1) : z, he ? PV(1, 1) : z, pc, rhn ? PV(2, 0) : z);
        const real_t mi = stencil5_row<real_t, SK>(MV(1, 0), hw ? MV(1, -1) : z, he ? MV(1, 1) : z, mcc, rhn ? MV(2, 0) : z);
        q[4] = NUMER ? sub_exact(pl, mi) : div_shared<FASTDIV>(sub_exact(pl, mi), ed, yd);
    }
#undef PV
#undef MV
}

template <typename CT, int MODE, int SK>
__global__ void __launch_bounds__(kBlock, 6)       // a register budget for six waves per SIMD (78 VGPRs, no spills: 128 -> 121 us in round 3)
k_f_stencil5_store_wave(const real_t *__restrict__ x, const real_t *__restrict__ eps, fd_stencil5_store st, int64_t jrow0, int64_t jrow1)
{
    // two columns per lane: aligned 16-B loads of x, 128 columns per wavefront
    constexpr int TW = 128, WC = 6;
    constexpr bool FASTDIV = true;      // the shared-reciprocal exact division (the IEEE sequence spills under the register budget: 337 us)
    __shared__ __attribute__((aligned(16))) real_t s_win[kBlock / 64][FD_STENCIL5_WAVE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nx = (int)st.nx, ny = (int)st.ny;
    const int TPR = (nx + TW - 1) / TW;
    const int64_t ntiles = (jrow1 - jrow0) * TPR, ngroups = (ntiles + kBlock / 64 - 1) / (kBlock / 64);
    const int64_t grp = xcd_tile(blockIdx.x, ngroups);
    if (grp >= ngroups) return;
    const int64_t wt = grp * (kBlock / 64) + wave;
    if (wt >= ntiles) return;
    // (32-bit division: the launcher declines grids with 2^31 tiles or more; a 64-bit one is ~150 instructions per wavefront)
    const unsigned wrow = (unsigned)wt / (unsigned)TPR;
    const int j = (int)(jrow0 + wrow), i0 = (int)((unsigned)wt - wrow * (unsigned)TPR) * TW;
    // (scalar copies of j and i0 for the addresses alone -- readfirstlane -- measured no change: 100.6 / 103.0 us, scripts/ab_c3.sh)
    const int i = i0 + 2 * lane;
    const int64_t k = (int64_t)j * nx + i;
    const bool act = i < nx;
    // a tile whose whole neighbourhood lies inside the grid needs no guards (wave-uniform)
    const bool interior = j >= 2 && j + 2 < ny && i0 >= 2 && i0 + TW + 2 <= nx;
    // window rows j-2 .. j+2, columns i-2 .. i+3 (zero outside the grid; of rows j+-2 only the lane's own columns are used)
    real_t W[5][WC];
    // The first and the last tile of a grid row (2 of 32 at nx = 4000) with two rows above and three below: every address of the
    // window is inside the array, so the loads stay unconditional (an idle lane reads the tile's first column) and the coordinates
    // outside the grid are SELECTED to 0 -- loads inside per-lane conditionals are waited for one by one (the 7-point kernel's
    // lesson, profiles/r04_y_lap7_taken_apart.md).
    const bool edge_tile = !interior && j >= 2 && j + 3 < ny;
    if (edge_tile) {
        const int64_t kl = act ? k : (int64_t)j * nx + i0;
#pragma unroll
        for (int dj = -2; dj <= 2; ++dj) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                r2_t v = {0, 0};
                if (!((dj == -2 || dj == 2) && c != 1)) {
                    const int ic = i + 2 * (c - 1);
                    const r2_t w = *reinterpret_cast<const r2_t *>(x + (kl + (int64_t)dj * nx + 2 * (c - 1)));
                    v.x = (act && ic >= 0 && ic < nx) ? w.x : (real_t)0;
                    v.y = (act && ic + 1 >= 0 && ic + 1 < nx) ? w.y : (real_t)0;
                }
                W[dj + 2][2 * c] = v.x; W[dj + 2][2 * c + 1] = v.y;
            }
        }
    } else
#pragma unroll
    for (int dj = -2; dj <= 2; ++dj) {
        const bool rowok = interior || (act && j + dj >= 0 && j + dj < ny);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r2_t v = {0, 0};
            if (!((dj == -2 || dj == 2) && c != 1)) {
                const int ic = i + 2 * (c - 1);
                const int64_t kc = k + (int64_t)dj * nx + 2 * (c - 1);
                if (interior || (rowok && ic >= 0 && ic + 1 < nx)) v = *reinterpret_cast<const r2_t *>(x + kc);
                else if (rowok) { if (ic >= 0 && ic < nx) v.x = x[kc]; if (ic + 1 >= 0 && ic + 1 < nx) v.y = x[kc + 1]; }
            }
            W[dj + 2][2 * c] = v.x; W[dj + 2][2 * c + 1] = v.y;
        }
    }
    int cpair[2] = {0, 0};
    if (act) { cpair[0] = (int)((const CT *)st.color)[k]; cpair[1] = (int)((const CT *)st.color)[k + 1]; }
    real_t q[10];
    // (one reciprocal per COLOUR fetched from the colour's lane, as the Float32 kernel below does: 101 -> 105 us here, scripts/ab_c3.sh)
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        if (interior) stencil5_column_quotients<MODE, SK, true, FASTDIV, WC>(W, o, i + o, j, nx, ny, eps[cpair[o]], q + 5 * o);
        else stencil5_column_quotients<MODE, SK, false, FASTDIV, WC>(W, o, i + o, j, nx, ny, eps[cpair[o]], q + 5 * o);
    }
    fd_stencil5_emit_wave<real_t, true, 2>(&st, s_win[wave], j, i0, q);
}

#ifdef FDJAC_F32
// Float32 (round 6): FOUR columns per lane -- 16-byte loads of x and 16-byte stores of the values (a Float32 pair moves 512 B per
// instruction, half of what the memory pipeline takes), 256 columns per wavefront -- and the division through Float64:
//   (float)((double)a * (1.0 / (double)b))  has the bits of the Float32  a / b  whenever that quotient is a NORMAL number: the double
// product is within 2^-52 of a / b, and a quotient of two 24-bit significands that is not itself a Float32 lies at least 2^-49 (relative)
// from every rounding boundary (scripts/ubench/exact_div32_probe.hip: 5e10 pairs, 0 mismatches; denormal quotients can differ).  The
// reciprocal belongs to the COLOUR: lane c of every wavefront forms 1 / (double)(2 eps_c) once and the columns fetch theirs by
// ds_bpermute; a column whose five quotients are not all normal numbers (zero, denormal, infinite, NaN -- or a step outside
// [2^-100, 2^100], whose reciprocal is handed out as NaN) takes the true divisions.  Three conversions / products and a class test
// per quotient instead of the ten instructions of v_div_scale .. v_div_fixup.
__device__ __forceinline__ void div5_through_f64(const float (&a)[5], float b, double y, float *q)
{
    bool ok = true;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        const float v = (float)((double)a[m] * y);
        q[m] = v;
        ok = ok && __builtin_amdgcn_classf(v, 0x108);          // -normal | +normal
    }
    if (!ok) {
#pragma unroll
        for (int m = 0; m < 5; ++m) q[m] = a[m] / b;
    }
}
template <typename CT, int MODE, int SK>
__global__ void __launch_bounds__(kBlock, 4)
k_f_stencil5_store_wave4(const real_t *__restrict__ x, const real_t *__restrict__ eps, fd_stencil5_store st, int64_t jrow0, int64_t jrow1)
{
    constexpr int TW = 256, WC = 8;
    __shared__ __attribute__((aligned(16))) real_t s_win[kBlock / 64][FD_STENCIL5_WAVE4_LDS];
    const int lane = threadIdx.x & 63, wave = wave_index_scalar();
    const int nx = (int)st.nx, ny = (int)st.ny;                 // nx is a multiple of 4 (launcher): a lane's four columns share a grid row
    const int TPR = (nx + TW - 1) / TW;
    const int64_t ntiles = (jrow1 - jrow0) * TPR, ngroups = (ntiles + kBlock / 64 - 1) / (kBlock / 64);
    const int64_t grp = xcd_tile(blockIdx.x, ngroups);
    if (grp >= ngroups) return;
    const int64_t wt = grp * (kBlock / 64) + wave;
    if (wt >= ntiles) return;
    const unsigned wrow = (unsigned)wt / (unsigned)TPR;
    const int j = (int)(jrow0 + wrow), i0 = (int)((unsigned)wt - wrow * (unsigned)TPR) * TW;
    const int i = i0 + 4 * lane;
    const int64_t k = (int64_t)j * nx + i;
    const bool act = i < nx;
    // the colours' steps and reciprocals, one colour per lane (st.C <= 64: launcher)
    real_t e_l = 1;
    double y_l = 0;
    if (lane < st.C) {
        e_l = eps[lane];
        const real_t ed = MODE == 1 ? 2 * e_l : e_l, mb = fabsf(ed);
        y_l = (mb >= 0x1p-100f && mb <= 0x1p100f) ? 1.0 / (double)ed : __builtin_nan("");
    }
    const bool interior = j >= 2 && j + 2 < ny && i0 >= 4 && i0 + TW + 4 <= nx;
    // window rows j-2 .. j+2, columns i-2 .. i+5 (zero outside the grid; of rows j+-2 only the lane's own columns are used)
    real_t W[5][WC];
    const bool edge_tile = !interior && j >= 2 && j + 3 < ny;   // every address below is inside the array: unconditional loads + selects
    if (interior || edge_tile) {
        const int64_t kl = act ? k : (int64_t)j * nx + i0;
#pragma unroll
        for (int dj = -2; dj <= 2; ++dj) {
            const real_t *row = x + (kl + (int64_t)dj * nx);
            const r4_t B = *reinterpret_cast<const r4_t *>(row);
            r4_t A = {0, 0, 0, 0}, Cq = {0, 0, 0, 0};
            if (dj >= -1 && dj <= 1) { A = *reinterpret_cast<const r4_t *>(row - 4); Cq = *reinterpret_cast<const r4_t *>(row + 4); }
            const bool okA = interior || (act && i >= 4), okB = interior || act, okC = interior || (act && i + 4 < nx);
            W[dj + 2][0] = okA ? A.z : (real_t)0; W[dj + 2][1] = okA ? A.w : (real_t)0;
            W[dj + 2][2] = okB ? B.x : (real_t)0; W[dj + 2][3] = okB ? B.y : (real_t)0;
            W[dj + 2][4] = okB ? B.z : (real_t)0; W[dj + 2][5] = okB ? B.w : (real_t)0;
            W[dj + 2][6] = okC ? Cq.x : (real_t)0; W[dj + 2][7] = okC ? Cq.y : (real_t)0;
        }
    } else {
        // the two first and the three last grid rows: every coordinate guarded
#pragma unroll
        for (int dj = -2; dj <= 2; ++dj) {
            const bool rowok = act && j + dj >= 0 && j + dj < ny;
#pragma unroll
            for (int c = 0; c < WC; ++c) {
                const int ic = i + c - 2;
                real_t v = 0;
                if (rowok && ic >= 0 && ic < nx && !((dj == -2 || dj == 2) && (c < 2 || c > 5))) v = x[k + (int64_t)dj * nx + (c - 2)];
                W[dj + 2][c] = v;
            }
        }
    }
    int cq[4] = {0, 0, 0, 0};
    if (act) {
        if constexpr (sizeof(CT) == 1) {
            const unsigned cw = *reinterpret_cast<const unsigned *>((const unsigned char *)st.color + k);       // (k is a multiple of 4)
            cq[0] = (int)(cw & 255u); cq[1] = (int)((cw >> 8) & 255u); cq[2] = (int)((cw >> 16) & 255u); cq[3] = (int)(cw >> 24);
        } else {
#pragma unroll
            for (int o = 0; o < 4; ++o) cq[o] = (int)((const CT *)st.color)[k + o];
        }
    }
    real_t q[20];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const real_t e = __shfl(e_l, cq[o], 64);
        const double y = __shfl(y_l, cq[o], 64);
        real_t num[5];
        if (interior) stencil5_column_quotients<MODE, SK, true, false, WC, true>(W, o, i + o, j, nx, ny, e, num);
        else stencil5_column_quotients<MODE, SK, false, false, WC, true>(W, o, i + o, j, nx, ny, e, num);
        div5_through_f64(num, MODE == 1 ? 2 * e : e, y, q + 5 * o);
    }
    fd_stencil5_emit_wave4<real_t, true>(&st, s_win[wave], j, i0, q);
}
#endif

// fd_bbb_store (round 5): the 5-point families on an nx x ny grid storing into BandedBlockBandedMatrix data -- ny blocks of nx rows,
// block bandwidths (1, 1), sub-block bandwidths (1, 1): the reference's own fixture (test/coloring_tests.jl:99-115;
// ext/FiniteDiffBlockBandedMatricesExt.jl:16-42).  Thread k = (i, j) owns column k: it loads the 13 coordinates its five rows read, forms
// the five quotients exactly as the CSC storing kernel does (stencil5_column_quotients) and writes the NINE slots of its column -- block
// j-1: (0, q_S, 0), block j: (q_W, q_C, q_E), block j+1: (0, q_N, 0); slots of rows outside their block and whole columns without a colour
// are 0, as k_decompress_bbb writes them.  A slot whose row does not depend on the column holds the row's difference with itself over the
// step, as in the hand-over path (the plan verified that the colouring is valid for the nine-point BBB pattern: no perturbed column
// reaches such a row): +-0.0 for a finite row, NaN otherwise.
template <typename CT, int MODE, int SK>
__global__ void __launch_bounds__(kBlock) k_f_stencil5_store_bbb(const real_t *__restrict__ x, const real_t *__restrict__ eps, fd_bbb_store st, int nx, int ny)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= st.N) return;
    const int j = (int)(k / nx), i = (int)(k - (int64_t)j * nx);
    real_t W[5][5];
#pragma unroll
    for (int dj = -2; dj <= 2; ++dj)
#pragma unroll
        for (int di = -2; di <= 2; ++di) {
            W[dj + 2][di + 2] = 0;
            if ((dj < 0 ? -dj : dj) + (di < 0 ? -di : di) > 2) continue;      // (only the 13 points within L1 distance 2 are read)
            const int ii = i + di, jj = j + dj;
            const bool in = ii >= 0 && ii < nx && jj >= 0 && jj < ny;
            const real_t v = x[in ? (int64_t)jj * nx + ii : k];              // (unconditional load from a clamped index)
            W[dj + 2][di + 2] = in ? v : (real_t)0;
        }
    const int c = (int)((const CT *)st.color)[k];
    const bool none = c == (int)(CT)(-1);
    real_t q[5] = {0, 0, 0, 0, 0};
    const real_t e = none ? (real_t)1 : eps[c];
    if (!none) stencil5_column_quotients<MODE, SK, false, true, 5>(W, 0, i, j, nx, ny, e, q);
    // an in-block row that does not depend on the column (the four corner rows (i +- 1, j +- 1)): the hand-over path divides the difference
    // of the row's value with ITSELF by the step -- an exact +0.0 while that value is finite (the sign of the quotient follows the step's,
    // dir = -1), NaN where the row reads a NaN / Inf coordinate or overflows.  So the row is evaluated and fr - fr divided: a constant
    // zero here stored 0.0 where the reference and every other route store NaN (tests/test_gpu_exact_structured.py, nan_inf).
    // zc[a][b]: row (i + 2 b - 1, j + 2 a - 1); a row outside the grid gives a value that is never stored
    real_t zc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int dj = 2 * a - 1, di = 2 * b - 1;
            auto at = [&](int ddi, int ddj) -> real_t {                      // coordinate (i + ddi, j + ddj), 0 outside the grid
                const int ii = i + ddi, jj = j + ddj;
                const bool in = ii >= 0 && ii < nx && jj >= 0 && jj < ny;
                const real_t v = x[in ? (int64_t)jj * nx + ii : k];          // (unconditional load from a clamped index)
                return in ? v : (real_t)0;
            };
            const real_t fr = stencil5_row<real_t, SK>(at(di, dj), at(di - 1, dj), at(di + 1, dj), at(di, dj - 1), at(di, dj + 1));
            zc[a][b] = (fr - fr) / (MODE == 1 ? 2 * e : e);
        }
    // rows k - nx, k - 1, k, k + 1, k + nx; those that do not exist hold garbage in q: they are never stored
    real_t *out = (real_t *)st.out;
    const long long sJ = st.stride[j];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const long long st0 = st.start[d + 3 * (long long)j];
        if (st0 < 0) continue;
        const int K = j + d - 1;                                          // (bu = 1)
        const bool kin = K >= 0 && K < ny;
        real_t *o = out + st0 + (long long)i * sJ;                         // slots t = 0, 1, 2 <-> rows i - 1, i, i + 1 of block K (mu = 1)
        const real_t mid = d == 0 ? q[0] : d == 1 ? q[2] : q[4];
        const real_t lo = d == 1 ? q[1] : zc[d >> 1][0], hi = d == 1 ? q[3] : zc[d >> 1][1];
        o[0] = (kin && !none && i - 1 >= 0) ? lo : (real_t)0;
        o[1] = (kin && !none) ? mid : (real_t)0;
        o[2] = (kin && !none && i + 1 < nx) ? hi : (real_t)0;
    }
}

template <typename CT>
static int lazy_stencil5_launch(BuiltinF *b, void *fx, const fd_lazy_points *lp, int64_t fs, int64_t r0, int64_t r1,
                                hipStream_t s)
{
    const int64_t r0e = r0 & ~(int64_t)1;
    const int64_t ntiles = (r1 - r0e + 2 * kBlock - 1) / (2 * kBlock);
    const unsigned g = (unsigned)(8 * xcd_chunks(ntiles));
    const int sk = b->family == FD_F_CLAMP5 ? 1 : b->family == FD_F_LAP5_NL ? 2 : 0;
    const int mode = lp->is_complex ? 2 : (lp->pts == 2 ? 1 : 0);
    // the storing kernels' <MODE, SK>: forward or central, the Laplacian or its nonlinear variant (everything else is declined below)
    const auto pick_store = [&](auto &&launch) {
        fd_pick<0, 1>(mode == 0 ? 0 : 1, [&](auto M) { fd_pick<0, 2>(sk == 2 ? 2 : 0, [&](auto SK) { launch(M, SK); }); });
    };
    if (lp->store) {
        // the launch stores the stencil's CSC Jacobian itself (fd_stencil5_store): every colour in one batch, the Laplacian
        // fixtures (the clamped sum's boundary rows reach themselves twice: not this pattern's arithmetic)
        if (lp->store_kind == FD_STORE_BBB && mode != 2 && sk != 1) {
            // BandedBlockBandedMatrix data: ny blocks of nx rows, (1, 1) / (1, 1) bandwidths -- the structure of this family's Jacobian
            const fd_bbb_store bb = *(const fd_bbb_store *)lp->store;
            if (bb.elem_bytes != (int)sizeof(real_t) || bb.block_size != b->prm[0] || bb.nblk != b->prm[1] || bb.bl != 1 || bb.bu != 1 || bb.lam != 1 ||
                bb.mu != 1 || lp->c_lo != 0 || lp->ncolors != bb.C || bb.color_bytes != (int)sizeof(CT) || bb.N >= ((int64_t)1 << 31))
                return FD_LAZY_DECLINED;
            const unsigned gb = (unsigned)((bb.N + kBlock - 1) / kBlock);
            pick_store([&](auto M, auto SK) {
                hipLaunchKernelGGL((k_f_stencil5_store_bbb<CT, M(), SK()>), dim3(gb), dim3(kBlock), 0, s, (const real_t *)lp->x,
                                   (const real_t *)lp->eps, bb, (int)b->prm[0], (int)b->prm[1]);
            });
            return launch_rc();
        }
        if (lp->store_kind != FD_STORE_STENCIL5 || mode == 2 || sk == 1) return FD_LAZY_DECLINED;
        const fd_stencil5_store st = *(const fd_stencil5_store *)lp->store;
        if (st.elem_bytes != (int)sizeof(real_t) || st.nx != b->prm[0] || st.ny != b->prm[1] || lp->c_lo != 0 || lp->ncolors != st.C ||
            st.color_bytes != (int)sizeof(CT) || (((uintptr_t)lp->x) & kPairMask) != 0 || st.col_end <= st.col_begin)
            return FD_LAZY_DECLINED;
        const int64_t jrow0 = st.col_begin / st.nx, jrow1 = (st.col_end - 1) / st.nx + 1;      // grid rows with local columns
        const int64_t ntiles = (jrow1 - jrow0) * ((st.nx + 127) / 128), ngroups = (ntiles + kBlock / 64 - 1) / (kBlock / 64);
        const unsigned gs = (unsigned)(8 * xcd_chunks(ngroups));
        if (ntiles >= ((int64_t)1 << 31) || st.nx * st.ny >= ((int64_t)1 << 31)) return FD_LAZY_DECLINED;   // (32-bit tile / grid arithmetic in the kernel)
        // ONE form (round 3 measured the others, profiles/r03_h_stencil_store_ab.txt; the probes live in scripts/ubench/): two columns per
        // lane, non-temporal stores, the shared-reciprocal exact division, guard-free interior tiles, a register budget for six waves per SIMD
#ifdef FDJAC_F32
        {   // Float32: four columns per lane, the division through Float64 (k_f_stencil5_store_wave4)
            const char *sw = fdjac::test_switch("FDJAC_S5_WAVE4");
            const bool quad_ok = st.nx % 4 == 0 && st.C <= 64 && (((uintptr_t)lp->x) & 15) == 0 && (((uintptr_t)st.color) & 3) == 0 &&
                                 !(sw && *sw && atoi(sw) == 0);
            const int64_t nt4 = (jrow1 - jrow0) * ((st.nx + 255) / 256), ng4 = (nt4 + kBlock / 64 - 1) / (kBlock / 64);
            if (quad_ok) {
                const unsigned g4 = (unsigned)(8 * xcd_chunks(ng4));
                pick_store([&](auto M, auto SK) {
                    hipLaunchKernelGGL((k_f_stencil5_store_wave4<CT, M(), SK()>), dim3(g4), dim3(kBlock), 0, s, (const real_t *)lp->x,
                                       (const real_t *)lp->eps, st, jrow0, jrow1);
                });
                return launch_rc();
            }
        }
#endif
        pick_store([&](auto M, auto SK) {
            hipLaunchKernelGGL((k_f_stencil5_store_wave<CT, M(), SK()>), dim3(gs), dim3(kBlock), 0, s, (const real_t *)lp->x,
                               (const real_t *)lp->eps, st, jrow0, jrow1);
        });
        return launch_rc();
    }
    fd_pick<0, 1, 2>(mode, [&](auto M) {
        fd_pick<0, 1, 2>(sk, [&](auto SK) {
            hipLaunchKernelGGL((k_f_stencil5_lazy<CT, M(), SK()>), dim3(g), dim3(kBlock), 0, s, (real_t *)fx, fs,
                               (real_t *)lp->base_out, (const real_t *)lp->x, (const CT *)lp->color, (const real_t *)lp->eps, lp->c_lo,
                               lp->ncolors, b->prm[0], b->prm[1], r0e, r1, lp->imag_only, mode != 2 ? lp->diff : 0);
        });
    });
    return launch_rc();
}
