// The block-coupled fixture (FD_F_BLOCKCOUPLED) at lazily perturbed points: the kernels, then their launcher.
// Included by fdjac_builtin_f.hip (namespace fdjac, after fdjac_f_stencil5.hip).

// Lazy-point version of the block-coupled family.  One workgroup owns kBcG consecutive blocks: phase A forms
// sig_b of those blocks and their two neighbours for EVERY point of the batch (x~ built in registers, the same
// lane-order + shuffle-tree sum as k_f_block_sigma), phase B evaluates the rows.  x / colours are read once for all
// points, sin(x) / cos(x) once per row (a point differs from the base in at most the row's own coordinate), and the
// perturbed points are never written: the complex-step BlockBanded configuration drops from perturb 88 us + f! 596 us
// to one ~memory-bound launch.  Bit-identical to perturb + k_f_block_sigma + k_f_block_apply.
constexpr int kBcG = 6;
template <typename T> __device__ __forceinline__ T tree_sum64(T acc)
{
    for (int off = 32; off > 0; off >>= 1) {
        if constexpr (sizeof(T) == sizeof(real_t)) {
            real_t o = __shfl_down(*reinterpret_cast<real_t *>(&acc), off, 64);
            acc = acc + *reinterpret_cast<T *>(&o);
        } else {
            cd *a = reinterpret_cast<cd *>(&acc);
            cd o{__shfl_down(a->re, off, 64), __shfl_down(a->im, off, 64)};
            acc = acc + *reinterpret_cast<T *>(&o);
        }
    }
    return acc;
}
// lanes of ONE wave exchange data through LDS: LDS instructions of a wave execute in order, this keeps the compiler
// from reordering them across the hand-over
__device__ __forceinline__ void bc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <int MODE> struct BcT { typedef real_t type; };
template <> struct BcT<2> { typedef cd type; };
__device__ __forceinline__ real_t bc_make(real_t x, real_t d, int sgn, real_t) { return sgn == 0 ? x + d : x - d; }
__device__ __forceinline__ cd bc_make(real_t x, real_t d, int, cd) { return cd{x, d}; }

template <typename CT, int MODE>
__global__ void __launch_bounds__(kBlock)
k_f_blockcoupled_lazy(real_t *__restrict__ fx, int64_t fs, real_t *__restrict__ base_out, const real_t *__restrict__ x,
                      const CT *__restrict__ color, const real_t *__restrict__ eps, int c_lo, int B, int64_t nb, int bs,
                      int64_t blk0, int64_t blk1, int64_t r0, int64_t r1, int imag_only)
{
    typedef typename BcT<MODE>::type T;
    extern __shared__ real_t s_bc[];
    constexpr int pts = MODE == 1 ? 2 : 1;
    constexpr int NBLK = kBcG + 2;
    const int PB = B * pts + 1;                      // last slot: the unperturbed point (base_out, forward only)
    T *sig = reinterpret_cast<T *>(s_bc);            // [NBLK][PB]            sigma of every point
    T *tree = sig + (size_t)NBLK * PB;               // [NBLK][128]           the batch-base summation tree (levels 0..5)
    int *owner = reinterpret_cast<int *>(tree + (size_t)NBLK * 128);   // [waves][B]  duplicate-colour detection
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g0 = blk0 + (int64_t)blockIdx.x * kBcG;
    const real_t w = (real_t)(lane + 1) / (real_t)bs;
    const bool want_base = (MODE == 0) && (base_out != nullptr);
    int *own = owner + wave * B;

    // phase A: sig of blocks g0-1 .. g0+kBcG for every point.  A point differs from the batch's base values
    // (x_j + 0.0) in the lanes whose colour it is -- normally ONE lane per block (the columns of a dense block all
    // conflict), and then only the six partial sums on that leaf's path to the root of the fixed summation tree
    // change: keep the tree of the base values in LDS and let the lane re-add along its path.  (Blocks with a repeated
    // colour take the general path: one full tree per point.)  Same additions as k_f_block_sigma => same bits.
    for (int lb = wave; lb < NBLK; lb += kBlock / 64) {
        const int64_t bb = g0 - 1 + lb;
        const bool inb = (bb >= 0) & (bb < nb);
        const bool act = inb & (lane < bs);
        real_t xj = 0.0;
        int cj = -1;
        if (act) {
            xj = x[bb * bs + lane];
            const int c = (int)color[bb * bs + lane];
            cj = (c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;
            if (cj >= B) cj = -1;
        }
        T *tr = tree + (size_t)lb * 128;
        T *sg = sig + (size_t)lb * PB;
        // base tree of the batch: leaves 0.0 + w*(x + 0.0) (what an unperturbed lane of any point contributes)
        T acc = act ? zero_of<T>() + w * bc_make(xj, 0.0, 0, T{}) : zero_of<T>();
        tr[lane] = acc;
        int base_at = 64;
        for (int off = 32; off > 0; off >>= 1) {
            if constexpr (sizeof(T) == sizeof(real_t)) {
                real_t o = __shfl_down(*reinterpret_cast<real_t *>(&acc), off, 64);
                acc = acc + *reinterpret_cast<T *>(&o);
            } else {
                cd *a = reinterpret_cast<cd *>(&acc);
                cd o{__shfl_down(a->re, off, 64), __shfl_down(a->im, off, 64)};
                acc = acc + *reinterpret_cast<T *>(&o);
            }
            if (lane < off && off > 1) tr[base_at + lane] = acc;   // level partials: 32 @64, 16 @96, 8 @112, 4 @120, 2 @124
            base_at += off;
        }
        T root = acc;   // valid in lane 0
        if constexpr (sizeof(T) == sizeof(real_t)) {
            real_t r = __shfl(*reinterpret_cast<real_t *>(&root), 0, 64);
            root = *reinterpret_cast<T *>(&r);
        } else {
            cd *a = reinterpret_cast<cd *>(&root);
            cd r{__shfl(a->re, 0, 64), __shfl(a->im, 0, 64)};
            root = *reinterpret_cast<T *>(&r);
        }
        bc_wave_sync();   // the tree written by this wave's lanes is read by other lanes below
        // duplicate colours inside the block?
        for (int q = lane; q < B; q += 64) own[q] = -1;
        bc_wave_sync();
        if (cj >= 0) own[cj] = lane;
        bc_wave_sync();
        const bool dup = (cj >= 0) && (own[cj] != lane);
        const bool any_dup = __builtin_amdgcn_ballot_w64(dup) != 0;
        if (!any_dup) {
            for (int q = lane; q < PB - 1; q += 64) sg[q] = inb ? root : zero_of<T>();
            bc_wave_sync();
            if (cj >= 0) {
                const real_t e = eps[c_lo + cj];
#pragma unroll
                for (int sgn = 0; sgn < pts; ++sgn) {
                    T n = zero_of<T>() + w * bc_make(xj, e, sgn, T{});
                    int idx = lane;
                    n = n + tr[idx ^ 32]; idx &= 31;
                    n = n + tr[64 + (idx ^ 16)]; idx &= 15;
                    n = n + tr[96 + (idx ^ 8)]; idx &= 7;
                    n = n + tr[112 + (idx ^ 4)]; idx &= 3;
                    n = n + tr[120 + (idx ^ 2)]; idx &= 1;
                    n = n + tr[124 + (idx ^ 1)];
                    sg[sgn * B + cj] = n;
                }
            }
        } else {
            for (int q = 0; q < PB - 1; ++q) {
                T term = zero_of<T>();
                if (act) {
                    const int b = q < B ? q : q - B;
                    const real_t d = (cj == b) ? eps[c_lo + b] : 0.0;
                    term = zero_of<T>() + w * bc_make(xj, d, q < B ? 0 : 1, T{});
                }
                term = tree_sum64<T>(term);
                if (lane == 0) sg[q] = inb ? term : zero_of<T>();
            }
        }
        if (want_base) {   // the base evaluation f(x) uses x itself (not x + 0.0); MODE 0 only, T = real_t
            real_t tb = act ? 0.0 + w * xj : 0.0;
            tb = tree_sum64<real_t>(tb);
            if (lane == 0) reinterpret_cast<real_t *>(sg)[PB - 1] = inb ? tb : 0.0;
        }
    }
    __syncthreads();

    for (int lb = 1 + wave; lb <= kBcG; lb += kBlock / 64) {
        const int64_t bb = g0 - 1 + lb;
        if (bb >= blk1 || bb >= nb) continue;
        const int64_t k = bb * bs + lane;
        if (!(lane < bs && k >= r0 && k < r1)) continue;
        const real_t xk = x[k];
        const int c = (int)color[k];
        const int ck = (c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;
        const bool mine = (ck >= 0) & (ck < B);
        const real_t e = mine ? eps[c_lo + ck] : 0.0;
        // values every point shares, and the ones of the row's own colour
        const real_t x0 = xk + 0.0;                 // what an unperturbed point of the batch holds (x + 0.0)
        real_t s0, sP = 0.0, sM = 0.0, c0 = 0.0, ch = 1.0, sh = 0.0;
        const real_t ch0 = cosh(0.0 * xk), sh0 = sinh(0.0 * xk);   // cosh(0), sinh(0) through the same library calls
        if (MODE == 2) {
            s0 = sin(xk); c0 = cos(xk);
            if (mine) { ch = cosh(e); sh = sinh(e); }
        } else {
            s0 = sin(x0);
            if (mine) { sP = sin(xk + e); if (MODE == 1) sM = sin(xk - e); }
        }
        const T *sm = sig + (size_t)(lb - 1) * PB, *sc = sig + (size_t)lb * PB, *sp = sig + (size_t)(lb + 1) * PB;
        for (int q = 0; q < PB - 1; ++q) {
            const int b = q < B ? q : q - B;
            const bool hit = mine & (ck == b);
            const T S = (sm[q] + sc[q]) + sp[q];
            if constexpr (MODE == 2) {
                const cd xt{xk, hit ? e : (real_t)0};
                const cd sn{s0 * (hit ? ch : ch0), c0 * (hit ? sh : sh0)};
                const cd v = xt * S + sn;
                if (imag_only) fx[(int64_t)q * fs + k] = v.im;
                else *reinterpret_cast<r2_t *>(fx + ((int64_t)q * fs + k) * 2) = r2_t{v.re, v.im};
            } else {
                const real_t d = hit ? e : 0.0;
                const real_t xt = q < B ? xk + d : xk - d;
                const real_t sn = hit ? (q < B ? sP : sM) : s0;
                fx[(int64_t)q * fs + k] = xt * S + sn;
            }
        }
        if (want_base) {
            const real_t *sb = reinterpret_cast<const real_t *>(sig);
            const real_t S = (sb[(size_t)(lb - 1) * PB + PB - 1] + sb[(size_t)lb * PB + PB - 1]) + sb[(size_t)(lb + 1) * PB + PB - 1];
            base_out[k] = xk * S + sin(xk);
        }
    }
}

// fd_lazy_points.store with a fd_colrange_store (include/fdjac_device.h), complex step: the block-coupled fixture evaluated at
// the lazily perturbed points and imag(f) / eps stored into the BlockBandedMatrix data by this launch (config 5: 245 MB of stored
// values written once, instead of written as f! values, read back and written again -- 0.195 -> 0.06 ms per Jacobian).
// Phase A is k_f_blockcoupled_lazy's: sigma of every point of the batch for the blocks g0-2 .. g0+kBcS+1 (the tree of the base
// values in LDS, a perturbed lane re-adds along its leaf-to-root path).  Phase B is column-centric: for column (b, j) -- point q = its
// colour -- and a row k of block b' in b-1 .. b+1 the value is imag(x~_k * (sig_{b'-1} + sig_{b'} + sig_{b'+1}) + sin(x~_k)) at point
// q, the operations of k_f_blockcoupled_lazy's phase B on the same operands (the plan verified that no other column of colour q
// touches those rows), divided by eps_q: same bits as the hand-over path.
#ifndef FD_BCS
#define FD_BCS 4
#endif
#ifndef FD_BCT
#define FD_BCT 512
#endif
constexpr int kBcT = FD_BCT;      // threads per workgroup
constexpr int kBcS = FD_BCS;      // block-columns per workgroup (2 / 3 / 4 / 6 / 8 / 10 measured: 57 / 62 / 57 / 63 / 67 / 75 us on config 5)
// complex items of the LDS region phase A uses for its trees and owners and phase B for the S sums
__host__ __device__ constexpr size_t bcs_shared_items(int B)
{
    const size_t item = 2 * sizeof(real_t);
    const size_t a = (size_t)(kBcS + 2) * (size_t)B, b = (size_t)(kBcT / 64) * 128 + ((size_t)(kBcT / 64) * (size_t)B * 4 + item - 1) / item;
    return a > b ? a : b;
}
__device__ __forceinline__ int bc_lane_int(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
__device__ __forceinline__ long long bc_lane_i64(long long v, int i)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v & 0xffffffffu), i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), i);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
#ifndef FD_BC_RPL32
#define FD_BC_RPL32 2      // Float32: row pairs of four columns (29.2 us at config 5) or row quads of eight (29.9 us), same box
#endif
// RPL consecutive rows of one column: one 16-byte store (Float64 pair / Float32 quad; a Float32 destination that is only 8-byte aligned: two pairs)
template <int RPL> __device__ __forceinline__ void bc_store_rows(real_t *d, const real_t (&v)[RPL], bool al)
{
    if constexpr (RPL == 2) {
        __builtin_nontemporal_store(r2_t{v[0], v[1]}, reinterpret_cast<r2_t *>(d));
    } else {
        typedef real_t rq_t __attribute__((ext_vector_type(4)));
        if (al) __builtin_nontemporal_store(rq_t{v[0], v[1], v[2], v[3]}, reinterpret_cast<rq_t *>(d));
        else {
            __builtin_nontemporal_store(r2_t{v[0], v[1]}, reinterpret_cast<r2_t *>(d));
            __builtin_nontemporal_store(r2_t{v[2], v[3]}, reinterpret_cast<r2_t *>(d + 2));
        }
    }
}
// QUAD (round 5; blocks of exactly 32 rows, even destinations: fd_colrange_store.pairs): a lane of phase B is a ROW PAIR of one of
// FOUR adjacent columns -- every store is 16 bytes per lane, 256 contiguous bytes per 16 lanes, half the store instructions of the
// two-column form; the same operations per element, so the same bits.  Float32 (round 6): row pairs too (8-byte stores, 33.8 -> 29.2 us
// at config 5; FD_BC_RPL32 = 4 makes it a ROW QUAD of one of EIGHT adjacent columns, 16-byte stores: 29.9 us on the same box).
template <typename CT, bool TWO, bool QUAD = false>
__global__ void __launch_bounds__(kBcT)
k_f_blockcoupled_store(const real_t *__restrict__ x, const CT *__restrict__ color, const real_t *__restrict__ eps, int c_lo, int B,
                       int64_t nb, int bs, int64_t blk0, int64_t blk1, fd_colrange_store st)
{
    typedef cd T;
    extern __shared__ real_t s_bcs[];
    constexpr int NBLK = kBcS + 4, NW = kBcT / 64, NIT = (NBLK + NW - 1) / NW;
    const int PB = B + 1;
    constexpr int RS = TWO ? 32 : 64;                // rows of a block in the row arrays
    constexpr int NU = (2 * kBcS + NW - 1) / NW;     // units of phase B per wave
    T *sig = reinterpret_cast<T *>(s_bcs);            // [NBLK][PB]   sigma of every point
    T *ssum = sig + (size_t)NBLK * PB;               // [kBcS + 2][B] (sig[k-1] + sig[k]) + sig[k+1] of the row blocks g0-1 .. g0+kBcS;
    T *tree = ssum;                                  //   before that, phase A's [NW][128] batch-base summation trees
    int *owner = reinterpret_cast<int *>(tree + (size_t)NW * 128);      //   and [NW][B] owners
    real_t *rx = reinterpret_cast<real_t *>(ssum + bcs_shared_items(B));   // [(kBcS + 2) * RS] x of the rows of those blocks
    real_t *rc = rx + (kBcS + 2) * RS;               //   cos(x)
    real_t *rz = rc + (kBcS + 2) * RS;               //   cos(x) * sinh(0 * x): imag(sin(x~)) of a row the point does not perturb
    real_t *ce = rz + (kBcS + 2) * RS;               // [B] step size of every colour of the batch,
    real_t *cy = ce + B;                             //     its reciprocal (div_shared),
    real_t *cs = cy + B;                             //     sinh(eps): imag(sin(x + i eps)) = cos(x) sinh(eps)
    const int lane = threadIdx.x & 63, wave = wave_index_scalar();
    const int64_t g0 = blk0 + (int64_t)blockIdx.x * kBcS;
    const real_t w = (real_t)(lane + 1) / (real_t)bs;
    int *own = owner + wave * B;
    const int ucols = (bs + 1) / 2;                  // columns of a unit of phase B (half a block-column)

    // every global load of phase A up front (the blocks g0-2 .. g0+kBcS+1 this wave sums: x and the colour of their columns)
    real_t xa[NIT];
    int ca[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int lb = wave + it * NW;
        const int64_t bb = g0 - 2 + lb;
        const bool act = (lb < NBLK) & (bb >= 0) & (bb < nb) & (lane < bs);
        xa[it] = 0.0; ca[it] = -1;
        if (act) {
            xa[it] = x[bb * bs + lane];
            const int c = (int)color[bb * bs + lane];
            int cj = (c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;
            if (cj >= B) cj = -1;
            ca[it] = cj;
        }
    }
    // PACK (Float32, blocks of <= 32 rows): x, cos(x), cos(x) sinh(0 x) of the rows phase B evaluates -- blocks g0-1 .. g0+kBcS -- are formed
    // by FULL wavefronts, two blocks each (lanes 0-31 / 32-63), instead of by the half-empty wavefront that sums the block: half the wave
    // instructions of the library cosine; the same function of the same operand: same bits.  One box, events (scripts/ab_c5.sh): Float32
    // 29.0 -> 25.8 us at config 5 -- used; Float64 48.2 -> 50.8 us -- not used.
    constexpr bool PACK = TWO && sizeof(real_t) == 4;
    real_t xr = 0;
    bool actr = false;
    const int lbr = 1 + 2 * wave + (lane >> 5);
    if constexpr (PACK) {
        const int64_t bbr = g0 - 2 + lbr;
        actr = (lbr <= kBcS + 2) & (bbr >= 0) & (bbr < nb) & ((lane & 31) < bs);
        if (actr) xr = x[bbr * bs + (lane & 31)];
    }
    // ... and of phase B: lane i holds the colour and the destination of column i of each unit the wave will store
    int uq[NU];
    long long ud[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
        const int u = wave + k * NW;
        const int cstart = (u & 1) * ucols, ncol = min(bs, cstart + ucols) - cstart;
        const int64_t bcol = g0 + (u >> 1);
        uq[k] = -1; ud[k] = 0;
        if (u < 2 * kBcS && bcol < blk1 && bcol < nb && lane < ncol) {
            const int64_t j = bcol * bs + cstart + lane;
            if (j >= st.col_begin && j < st.col_end) {
                const int c = (int)color[j];
                const int q = (c == (int)(CT)(-1) || c < 0) ? -1 : c - c_lo;
                if (q >= 0 && q < B) { uq[k] = q; ud[k] = st.dest[j - st.col_begin]; }       // (else: another batch's colour)
            }
        }
    }
    int notp2 = 0;
    for (int q = threadIdx.x; q < B; q += kBcT) {
        const real_t e = eps[c_lo + q];
        ce[q] = e; cy[q] = (real_t)1 / e; cs[q] = sinh(e);
        notp2 |= div_is_pow2(e) ? 0 : 1;
    }
    // every step size of the batch a power of two (the complex step's default, eps(T)): imag * (1 / eps) is imag / eps, bit for bit --
    // no division at all.  Float32 only (whose quotients are true divisions: 39.3 -> 33.2 us at 10^4 blocks of 32 x 32, same box); for
    // Float64, where the quotient already is a product and two FMA corrections, dropping them measured no gain (52.2 against 51.5 us)
    const bool p2all = sizeof(real_t) == 4 && __syncthreads_or(notp2) == 0;
    if (sizeof(real_t) != 4) __syncthreads();

    if constexpr (PACK) {
        if (lbr <= kBcS + 2) {                         // (wave-uniform up to the two halves: the wavefronts 0 .. (kBcS + 1) / 2)
            const int at = (lbr - 1) * RS + (lane & 31);
            const real_t c0 = actr ? cos(xr) : (real_t)0;
            rx[at] = xr;
            rc[at] = c0;
            const real_t z = 0.0 * xr;                          // +-0 for a finite x: sinh(+-0) = +-0 (non-finite x: the library call)
            rz[at] = actr ? c0 * (z == (real_t)0 ? z : sinh(z)) : (real_t)0;
        }
    }
    // ---- phase A (as k_f_blockcoupled_lazy, MODE 2): sig of blocks g0-2 .. g0+kBcS+1 for every point of the batch
    real_t *tr = reinterpret_cast<real_t *>(tree) + (size_t)wave * 128;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int lb = wave + it * NW;
        if (lb >= NBLK) break;
        const int64_t bb = g0 - 2 + lb;
        const bool inb = (bb >= 0) & (bb < nb);
        const bool act = inb & (lane < bs);
        const real_t xj = xa[it];
        const int cj = ca[it];
        if (!PACK && lb >= 1 && lb <= kBcS + 2) {    // the rows phase B evaluates: x, cos once per row
            const int at = (lb - 1) * RS + lane;
            const real_t c0 = act ? cos(xj) : (real_t)0;
            if (lane < RS) {
            rx[at] = xj;
            rc[at] = c0;
            const real_t z = 0.0 * xj;                          // +-0 for a finite x: sinh(+-0) = +-0 (non-finite x: the library call)
            rz[at] = act ? c0 * (z == (real_t)0 ? z : sinh(z)) : (real_t)0;
            }
        }
        T *sg = sig + (size_t)lb * PB;
        // the base tree holds REAL parts only: the imaginary part of every base leaf is 0.0 + w * 0.0 = +0 and so is every partial
        // sum of them, and v + (+0) = v for the v = 0.0 + w * eps a perturbed lane starts from -- the bits of the complex tree
        real_t acc = act ? (real_t)0 + w * xj : (real_t)0;
        bc_wave_sync();                              // (the previous block's tree is no longer read)
        tr[lane] = acc;
        int base_at = 64;
        for (int off = 32; off > 0; off >>= 1) {
            acc = acc + __shfl_down(acc, off, 64);
            if (lane < off && off > 1) tr[base_at + lane] = acc;
            base_at += off;
        }
        const T root{__shfl(acc, 0, 64), (real_t)0};
        for (int q = lane; q < B; q += 64) own[q] = -1;
        bc_wave_sync();
        if (cj >= 0) own[cj] = lane;
        bc_wave_sync();
        const bool dup = (cj >= 0) && (own[cj] != lane);
        const bool any_dup = __builtin_amdgcn_ballot_w64(dup) != 0;
        if (!any_dup) {
            for (int q = lane; q < PB - 1; q += 64) sg[q] = inb ? root : zero_of<T>();
            bc_wave_sync();
            if (cj >= 0) {
                const real_t e = ce[cj];
                real_t n = (real_t)0 + w * xj;
                int idx = lane;
                n = n + tr[idx ^ 32]; idx &= 31;
                n = n + tr[64 + (idx ^ 16)]; idx &= 15;
                n = n + tr[96 + (idx ^ 8)]; idx &= 7;
                n = n + tr[112 + (idx ^ 4)]; idx &= 3;
                n = n + tr[120 + (idx ^ 2)]; idx &= 1;
                n = n + tr[124 + (idx ^ 1)];
                sg[cj] = T{n, (real_t)0 + w * e};
            }
        } else {
            for (int q = 0; q < PB - 1; ++q) {
                T term = zero_of<T>();
                if (act) {
                    const real_t d = (cj == q) ? ce[q] : 0.0;
                    term = zero_of<T>() + w * bc_make(xj, d, 0, T{});
                }
                term = tree_sum64<T>(term);
                if (lane == 0) sg[q] = inb ? term : zero_of<T>();
            }
        }
    }
    __syncthreads();

    // S of every (row block, point): (sig[k-1] + sig[k]) + sig[k+1], the sum k_f_blockcoupled_lazy's phase B forms, once per group
    for (int idx = threadIdx.x; idx < (kBcS + 2) * B; idx += kBcT) {
        const int lbk = 1 + idx / B, q = idx - (lbk - 1) * B;
        const T *sm = sig + (size_t)(lbk - 1) * PB + q;
        ssum[idx] = (sm[0] + sm[PB]) + sm[2 * PB];
    }
    __syncthreads();

    // ---- phase B, column-centric.  A wave takes a unit = half of the columns of one block-column; a lane is a ROW of the block (and,
    // TWO: blocks of <= 32 rows, one of two adjacent columns): it keeps x, cos(x) sinh(0 x) of its row in the three row blocks
    // b-1, b, b+1 in registers across the unit's columns and per column evaluates its three entries at the column's own point and
    // stores them (32 lanes = 256 contiguous bytes per row block; a column is one contiguous run).
    real_t *outp = (real_t *)st.out;
    if constexpr (QUAD) {
        // RPL rows per lane: a row pair of one of FOUR columns (Float64) or a row quad of one of EIGHT columns (Float32) -- 16 bytes per store
        constexpr int RPL = sizeof(real_t) == 4 ? FD_BC_RPL32 : 2, LPC = 32 / RPL, CPI = 64 / LPC;
        const int cq = lane / LPC, r2 = lane % LPC;                       // column of the iteration's CPI, rows RPL r2 .. RPL r2 + RPL - 1
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const int u = wave + k * NW;
            if (u >= 2 * kBcS) break;
            const int lb = 2 + (u >> 1), cstart = (u & 1) * ucols, ncol = min(bs, cstart + ucols) - cstart;
            const int64_t bcol = g0 - 2 + lb;
            if (bcol >= blk1 || bcol >= nb || ncol <= 0) continue;
            const int q_l = uq[k];
            const long long dest_l = ud[k];
            real_t xk[3][RPL], rzk[3][RPL], rcm[RPL];
            bool mv[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int64_t kb = bcol - 1 + m;
                mv[m] = (kb >= 0) & (kb < nb);
                const int at = (lb - 2 + m) * RS + RPL * r2;
#pragma unroll
                for (int h = 0; h < RPL; ++h) { xk[m][h] = rx[at + h]; rzk[m][h] = rz[at + h]; }
            }
#pragma unroll
            for (int h = 0; h < RPL; ++h) rcm[h] = rc[(lb - 1) * RS + RPL * r2 + h];
            const int first = bcol > 0 ? 0 : 1;
            const T *su = ssum + (size_t)(lb - 2) * B;
            for (int it = 0; CPI * it < ncol; ++it) {
                const int ci = CPI * it + cq;
                const int src = ci < ncol ? ci : 0;
                const int qs = __shfl(q_l, src, 64);
                const unsigned dlo = (unsigned)__shfl((int)(unsigned)((unsigned long long)dest_l & 0xffffffffu), src, 64);
                const unsigned dhi = (unsigned)__shfl((int)(unsigned)((unsigned long long)dest_l >> 32), src, 64);
                const bool cv = (ci < ncol) & (qs >= 0);
                const int q = cv ? qs : 0;
                real_t *dst = outp + (long long)(((unsigned long long)dhi << 32) | dlo) + RPL * r2;
                const real_t e = ce[q], ye = cy[q], sh = cs[q];
                const int jl = cstart + ci;
                real_t vim[3][RPL], qv[3][RPL];
                bool fast = p2all || (sizeof(real_t) == 8 && div_shared_ok(e));
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const T S = su[(size_t)m * B + q];
#pragma unroll
                    for (int h = 0; h < RPL; ++h) {
                        const bool hit = (m == 1) & (RPL * r2 + h == jl);
                        const real_t xim = hit ? e : (real_t)0;
                        const real_t snim = hit ? rcm[h] * sh : rzk[m][h];
                        vim[m][h] = (xk[m][h] * S.im + xim * S.re) + snim;
                        qv[m][h] = vim[m][h] * ye;
                        if (!p2all) {
                            const real_t ma = fabs(vim[m][h]);        // (the divisor's range is tested once per column: div_shared_ok)
                            fast = fast & (!mv[m] | ((ma >= (real_t)0x1p-800) & (ma <= (real_t)0x1p800)));
                        }
                    }
                }
                if (p2all) {
                    // (qv is the quotient already)
                } else if (fast) {
#pragma unroll
                    for (int m = 0; m < 3; ++m)
#pragma unroll
                        for (int h = 0; h < RPL; ++h) {
                            const real_t r0 = __builtin_fma(-e, qv[m][h], vim[m][h]);
                            const real_t q1 = __builtin_fma(r0, ye, qv[m][h]);
                            const real_t r1 = __builtin_fma(-e, q1, vim[m][h]);
                            qv[m][h] = __builtin_fma(r1, ye, q1);
                        }
                } else {
#pragma unroll
                    for (int m = 0; m < 3; ++m)
#pragma unroll
                        for (int h = 0; h < RPL; ++h) qv[m][h] = vim[m][h] / e;
                }
                // (Float32: a destination that is even but not a multiple of four -- pairs there)
                const bool al = RPL == 2 || (dlo & 3u) == 0;
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (cv & mv[m]) {
                        bc_store_rows<RPL>(dst + (m - first) * bs, qv[m], al);
                    }
            }
        }
        return;
    }
    const int half = TWO ? lane >> 5 : 0, r = TWO ? lane & 31 : lane;
    const bool ract = r < bs;
#pragma unroll
    for (int k = 0; k < NU; ++k) {
        const int u = wave + k * NW;
        if (u >= 2 * kBcS) break;
        const int lb = 2 + (u >> 1), cstart = (u & 1) * ucols, ncol = min(bs, cstart + ucols) - cstart;
        const int64_t bcol = g0 - 2 + lb;
        if (bcol >= blk1 || bcol >= nb || ncol <= 0) continue;
        const int q_l = uq[k];
        const long long dest_l = ud[k];
        // the lane's rows: block bcol - 1 + m, row r of it (block bandwidths (1, 1), equal blocks)
        real_t xk[3], rzk[3];
        bool mv[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int64_t kb = bcol - 1 + m;
            mv[m] = ract & (kb >= 0) & (kb < nb);
            const int at = (lb - 2 + m) * RS + r;
            xk[m] = rx[at]; rzk[m] = rz[at];
        }
        const real_t rcm = rc[(lb - 1) * RS + r];
        const int first = bcol > 0 ? 0 : 1;                               // the column's stored rows start at block max(bcol - 1, 0)
        const T *su = ssum + (size_t)(lb - 2) * B;
        for (int it = 0; it * (TWO ? 2 : 1) < ncol; ++it) {
            const int ci = TWO ? 2 * it + half : it;                      // column of the unit
            const int src = ci < ncol ? ci : 0;
            const int qs = __shfl(q_l, src, 64);
            const unsigned dlo = (unsigned)__shfl((int)(unsigned)((unsigned long long)dest_l & 0xffffffffu), src, 64);
            const unsigned dhi = (unsigned)__shfl((int)(unsigned)((unsigned long long)dest_l >> 32), src, 64);
            const bool cv = (ci < ncol) & (qs >= 0);
            const int q = cv ? qs : 0;
            real_t *dst = outp + (long long)(((unsigned long long)dhi << 32) | dlo) + r;
            const real_t e = ce[q], ye = cy[q], sh = cs[q];
            const int jl = cstart + ci;                                   // the column's own row is row jl of the middle block
            // the three entries of the lane as independent chains (nothing but the stores is predicated)
            real_t vim[3], qv[3];
            bool fast = p2all || (sizeof(real_t) == 8 && div_shared_ok(e));
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const T S = su[(size_t)m * B + q];
                const bool hit = (m == 1) & (r == jl);
                // imag(x~ * S + sin(x~)), x~ = (xk, hit ? e : 0):  (x~.re * S.im + x~.im * S.re) + cos(xk) * sinh(x~.im)
                const real_t xim = hit ? e : (real_t)0;
                const real_t snim = hit ? rcm * sh : rzk[m];
                vim[m] = (xk[m] * S.im + xim * S.re) + snim;
                qv[m] = vim[m] * ye;
                if (!p2all) {
                    const real_t ma = fabs(vim[m]);
                    fast = fast & (!mv[m] | ((ma >= (real_t)0x1p-800) & (ma <= (real_t)0x1p800)));
                }
            }
            // vim / e: div_shared's correctly rounded quotient (two FMA corrections of vim * (1 / e)); true division out of its range
            if (p2all) {
                // (a power-of-two step: qv is the quotient already)
            } else if (fast) {
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const real_t r0 = __builtin_fma(-e, qv[m], vim[m]);
                    const real_t q1 = __builtin_fma(r0, ye, qv[m]);
                    const real_t r1 = __builtin_fma(-e, q1, vim[m]);
                    qv[m] = __builtin_fma(r1, ye, q1);
                }
            } else {
#pragma unroll
                for (int m = 0; m < 3; ++m) qv[m] = vim[m] / e;
            }
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (cv & mv[m]) __builtin_nontemporal_store(qv[m], dst + (m - first) * bs);
        }
    }
}

static size_t bcs_lds_bytes(int ncolors, int bs)
{
    const size_t rs = bs <= 32 ? 32 : 64;
    return ((size_t)(kBcS + 4) * (size_t)(ncolors + 1) + bcs_shared_items(ncolors)) * 2 * sizeof(real_t) +
           (size_t)3 * (kBcS + 2) * rs * sizeof(real_t) + (size_t)(3 * ncolors + 2) * sizeof(real_t);
}

// LDS of k_f_blockcoupled_lazy: sigma of every point + the base summation tree, per block of the group, + owners
static size_t bc_lds_bytes(int ncolors, int pts, bool cplx)
{
    const size_t el = cplx ? 2 * sizeof(real_t) : sizeof(real_t);
    return (size_t)(kBcG + 2) * ((size_t)(ncolors * pts + 1) + 128) * el + (size_t)(kBlock / 64) * (size_t)ncolors * 4;
}

template <typename CT>
static int lazy_blockcoupled_launch(BuiltinF *b, void *fx, const fd_lazy_points *lp, int64_t fs, int64_t r0, int64_t r1,
                                    hipStream_t s)
{
    const int64_t nb = b->prm[0], bs = b->prm[1];
    const int mode = lp->is_complex ? 2 : (lp->pts == 2 ? 1 : 0);
    if (lp->store) {
        // the launch stores imag(f) / eps into the block-banded data itself (fd_colrange_store): complex step, the block structure of
        // this fixture (dense blocks of bs <= 64 rows, block bandwidths (1, 1))
        if (lp->store_kind != FD_STORE_COLRANGE || mode != 2) return FD_LAZY_DECLINED;
        const fd_colrange_store st = *(const fd_colrange_store *)lp->store;
        if (st.elem_bytes != (int)sizeof(real_t) || st.nblk != nb || st.block_size != bs || st.bl != 1 || st.bu != 1 || bs > 64 ||
            st.color_bytes != (int)sizeof(CT) || st.col_end <= st.col_begin || bcs_lds_bytes(lp->ncolors, (int)bs) > (size_t)64 * 1024)
            return FD_LAZY_DECLINED;
        const int64_t cb0 = st.col_begin / bs, cb1 = (st.col_end - 1) / bs + 1;      // blocks with local columns
        const int64_t gs = (cb1 - cb0 + kBcS - 1) / kBcS;
        // <TWO, QUAD>: 2 = row pairs (or Float32 row quads), 1 = two blocks per wave (bs <= 32), 0 = one
        const bool quad = bs == 32 && st.pairs && (((uintptr_t)st.out) & (sizeof(real_t) == 4 ? 4 * FD_BC_RPL32 - 1 : 15)) == 0;
        fd_pick<2, 1, 0>(quad ? 2 : bs <= 32 ? 1 : 0, [&](auto V) {
            hipLaunchKernelGGL((k_f_blockcoupled_store<CT, (V() >= 1), (V() == 2)>), dim3((unsigned)gs), dim3(kBcT),
                               bcs_lds_bytes(lp->ncolors, (int)bs), s, (const real_t *)lp->x, (const CT *)lp->color,
                               (const real_t *)lp->eps, lp->c_lo, lp->ncolors, nb, (int)bs, cb0, cb1, st);
        });
        return launch_rc();
    }
    const int64_t blk0 = r0 / bs, blk1 = (r1 - 1) / bs + 1;
    const int64_t g = (blk1 - blk0 + kBcG - 1) / kBcG;
    const size_t shm = bc_lds_bytes(lp->ncolors, lp->pts, mode == 2);
    fd_pick<0, 1, 2>(mode, [&](auto M) {
        hipLaunchKernelGGL((k_f_blockcoupled_lazy<CT, M()>), dim3((unsigned)g), dim3(kBlock), shm, s, (real_t *)fx, fs,
                           (real_t *)lp->base_out, (const real_t *)lp->x, (const CT *)lp->color, (const real_t *)lp->eps, lp->c_lo,
                           lp->ncolors, nb, (int)bs, blk0, blk1, r0, r1, lp->imag_only);
    });
    return launch_rc();
}
