// Built-in device f! families behind the fd_f_launch boundary: the reference's own test
// fixtures (test/coloring_tests.jl:5-13, 99-108, 124-133) and the benchmark configurations of
// BASELINE.json.  Each kernel evaluates `nbatch` independent points (grid.y = point index) and
// only the rows [row_begin,row_end) the plan will consume.  Real and complex (for the
// complex-step arm, src/jacobians.jl:623-648) instantiations share one template.
//
// Operation order follows the fixtures literally (e.g. (x[i-1] - 2x[i]) + x[i+1]) and the
// library is built with -ffp-contract=off, so a linear fixture reproduces the CPU values bit
// for bit.
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "fdjac_internal.h"
#include "fdjac_eps_dev.h"

namespace fdjac {

constexpr real_t kTwo = 2, kFour = 4;   // literals in the element type (Julia's 2x / 4x stay in eltype(x))
struct cd {
    real_t re, im;
};
__device__ __forceinline__ cd operator+(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cd operator-(cd a, cd b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cd operator*(cd a, cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cd operator*(real_t s, cd a) { return {s * a.re, s * a.im}; }
__device__ __forceinline__ cd operator+(cd a, real_t s) { return {a.re + s, a.im}; }
__device__ __forceinline__ cd operator-(cd a, real_t s) { return {a.re - s, a.im}; }

template <typename T> __device__ __forceinline__ T zero_of();
template <> __device__ __forceinline__ real_t zero_of<real_t>() { return 0.0; }
template <> __device__ __forceinline__ cd zero_of<cd>() { return {0.0, 0.0}; }

__device__ __forceinline__ real_t sin_of(real_t a) { return sin(a); }
__device__ __forceinline__ cd sin_of(cd a)
{
    // sin(a+ib) = sin a cosh b + i cos a sinh b
    return {sin(a.re) * cosh(a.im), cos(a.re) * sinh(a.im)};
}

// dx[i] = x[i-1] - 2x[i] + x[i+1]  (+ x[i]^2 * x[i+1] when NL), zero beyond the ends.
template <typename T, bool NL>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag(T *__restrict__ fx, const T *__restrict__ x, int64_t n, int64_t xs, int64_t fs, int64_t r0, int64_t r1)
{
    const T *xb = x + (int64_t)blockIdx.y * xs;
    T *fb = fx + (int64_t)blockIdx.y * fs;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = r0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < r1; i += stride) {
        const T xm = i > 0 ? xb[i - 1] : zero_of<T>();
        const T xp = i + 1 < n ? xb[i + 1] : zero_of<T>();
        const T xi = xb[i];
        T v = (xm - kTwo * xi) + xp;
        if (NL) v = v + (xi * xi) * xp;
        fb[i] = v;
    }
}

// Same fixture, two rows per thread: one aligned 16-B load of (x[i], x[i+1]) plus the two scalar
// neighbours (L1 hits), one 16-B store.  Needs even i and 16-B aligned batch bases.
template <bool NL>
__global__ void __launch_bounds__(kBlock)
k_f_tridiag_v2(real_t *__restrict__ fx, const real_t *__restrict__ x, int64_t n, int64_t xs, int64_t fs, int64_t r0,
               int64_t r1)
{
    const real_t *xb = x + (int64_t)blockIdx.y * xs;
    real_t *fb = fx + (int64_t)blockIdx.y * fs;
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t i = r0 + ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; i < r1; i += stride) {
        if (i + 1 < n) {
            const r2_t c = *reinterpret_cast<const r2_t *>(xb + i);
            const real_t xm = i > 0 ? xb[i - 1] : 0.0;
            const real_t xq = i + 2 < n ? xb[i + 2] : 0.0;
            real_t v0 = (xm - kTwo * c.x) + c.y;
            real_t v1 = (c.x - kTwo * c.y) + xq;
            if (NL) {
                v0 = v0 + (c.x * c.x) * c.y;
                v1 = v1 + (c.y * c.y) * xq;
            }
            *reinterpret_cast<r2_t *>(fb + i) = r2_t{v0, v1};
        } else {
            const real_t xm = i > 0 ? xb[i - 1] : 0.0;
            const real_t xi = xb[i];
            fb[i] = (xm - kTwo * xi) + 0.0;
        }
    }
}

// the wavefront's index in its workgroup, told to the compiler as the wave-uniform value it is: tile numbers, row starts, interior / edge
// verdicts and base addresses derived from it then live in scalar registers and are computed by the scalar unit.  One box, events
// (scripts/ab_all.sh): block-coupled store 49.6 -> 48.1 us (Float32 29.4 -> 28.9), Float32 5-point store 57.9 -> 57.2 -- used there;
// the Float64 5-point store 100 -> 127-132 us (its interior / edge / boundary window loads become real branches) and the tridiagonal
// stores unchanged -- not used there.
__device__ __forceinline__ int wave_index_scalar() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// the subtraction of fd_lazy_points.diff: an IEEE a - b of the two stored values, never contracted into a producer
__device__ __forceinline__ real_t sub_exact(real_t a, real_t b)
{
#pragma clang fp contract(off)
    return a - b;
}

// 5-point stencils on an nx (fast) x ny grid.  CLAMP = false: zero-Dirichlet Laplacian
// w + e + s + n - 4x ; CLAMP = true: the reference's clamped-edge sum x + x[i-1] + x[i+1] + x[j-1] + x[j+1].
// (SK: 0 = Laplacian, 1 = clamped sum, 2 = Laplacian + x[k]^2 * x[k+1]: a nonlinear variant whose J depends on x.)
template <typename T, int SK>
__global__ void __launch_bounds__(kBlock)
k_f_stencil5(T *__restrict__ fx, const T *__restrict__ x, int64_t nx, int64_t ny, int64_t xs, int64_t fs,
             int64_t r0, int64_t r1)
{
    const T *xb = x + (int64_t)blockIdx.y * xs;
    T *fb = fx + (int64_t)blockIdx.y * fs;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = r0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; k < r1; k += stride) {
        const int64_t j = k / nx, i = k - j * nx;
        if (SK == 1) {
            const int64_t im = i > 0 ? i - 1 : 0, ip = i + 1 < nx ? i + 1 : nx - 1;
            const int64_t jm = j > 0 ? j - 1 : 0, jp = j + 1 < ny ? j + 1 : ny - 1;
            fb[k] = (((xb[k] + xb[im + nx * j]) + xb[ip + nx * j]) + xb[i + nx * jm]) + xb[i + nx * jp];
        } else {
            const T w = i > 0 ? xb[k - 1] : zero_of<T>();
            const T e = i + 1 < nx ? xb[k + 1] : zero_of<T>();
            const T s = j > 0 ? xb[k - nx] : zero_of<T>();
            const T n = j + 1 < ny ? xb[k + nx] : zero_of<T>();
            T v = (((w + e) + s) + n) - kFour * xb[k];
            if (SK == 2) v = v + (xb[k] * xb[k]) * e;    // lap5_nl: + x[k]^2 * x[k+1] (J depends on x)
            fb[k] = v;
        }
    }
}

// Same stencils, two rows per thread (nx even): 16-B loads of the centre / south / north pairs, two
// scalar loads for the west / east neighbours, one 16-B store.  One-shot launch with the XCD-aware
// tile mapping: the rows k-nx, k, k+nx that share x lines are evaluated by the same XCD, so each
// line of x enters one L2 instead of three.
template <int SK>
__global__ void __launch_bounds__(kBlock)
k_f_stencil5_v2(real_t *__restrict__ fx, const real_t *__restrict__ x, int64_t nx, int64_t ny, int64_t xs, int64_t fs,
                int64_t r0, int64_t r1)
{
    const real_t *xb = x + (int64_t)blockIdx.y * xs;
    real_t *fb = fx + (int64_t)blockIdx.y * fs;
    const int64_t ntiles = (r1 - r0 + 2 * kBlock - 1) / (2 * kBlock);
    const int64_t tile = xcd_tile(blockIdx.x, ntiles);
    if (tile >= ntiles) return;
    const int64_t k = r0 + tile * (2 * kBlock) + threadIdx.x * 2;   // r0 even, nx even => k, k+1 share a grid row
    if (k >= r1) return;
    const int64_t j = k / nx, i = k - j * nx;
    const r2_t c = *reinterpret_cast<const r2_t *>(xb + k);
    const bool hs = j > 0, hn = j + 1 < ny, hw = i > 0, he = i + 2 < nx;
    r2_t s = r2_t{0.0, 0.0}, n = r2_t{0.0, 0.0};
    if (hs) s = *reinterpret_cast<const r2_t *>(xb + k - nx);
    if (hn) n = *reinterpret_cast<const r2_t *>(xb + k + nx);
    const real_t w = hw ? xb[k - 1] : 0.0;
    const real_t e = he ? xb[k + 2] : 0.0;
    real_t v0, v1;
    if (SK == 1) {
        const real_t w0 = hw ? w : c.x, e1 = he ? e : c.y;
        const real_t s0 = hs ? s.x : c.x, s1 = hs ? s.y : c.y, n0 = hn ? n.x : c.x, n1 = hn ? n.y : c.y;
        v0 = (((c.x + w0) + c.y) + s0) + n0;
        v1 = (((c.y + c.x) + e1) + s1) + n1;
    } else {
        v0 = (((w + c.y) + s.x) + n.x) - kFour * c.x;
        v1 = (((c.x + e) + s.y) + n.y) - kFour * c.y;
        if (SK == 2) { v0 = v0 + (c.x * c.x) * c.y; v1 = v1 + (c.y * c.y) * e; }
    }
    *reinterpret_cast<r2_t *>(fb + k) = r2_t{v0, v1};
}

// block-coupled: sig_b = sum_j w_j x_b[j], w_j = (j+1)/bs; one wave per block, fixed-order tree.
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_f_block_sigma(T *__restrict__ sig, const T *__restrict__ x, int64_t nb, int64_t bs, int64_t xs, int64_t b0, int64_t b1)
{
    const T *xb = x + (int64_t)blockIdx.y * xs;
    T *sb = sig + (int64_t)blockIdx.y * nb;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t b = b0 + wave; b < b1; b += nw) {
        T acc = zero_of<T>();
        for (int64_t j = lane; j < bs; j += 64) acc = acc + ((real_t)(j + 1) / (real_t)bs) * xb[b * bs + j];
        // serial-order-independent but fixed: tree over lanes
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
        if (lane == 0) sb[b] = acc;
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_f_block_apply(T *__restrict__ fx, const T *__restrict__ x, const T *__restrict__ sig, int64_t nb, int64_t bs,
                int64_t xs, int64_t fs, int64_t r0, int64_t r1)
{
    const T *xb = x + (int64_t)blockIdx.y * xs;
    const T *sb = sig + (int64_t)blockIdx.y * nb;
    T *fb = fx + (int64_t)blockIdx.y * fs;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = r0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; k < r1; k += stride) {
        const int64_t b = k / bs;
        const T sm = b > 0 ? sb[b - 1] : zero_of<T>();
        const T sp = b + 1 < nb ? sb[b + 1] : zero_of<T>();
        const T S = (sm + sb[b]) + sp;
        fb[k] = xb[k] * S + sin_of(xb[k]);
    }
}

// y[k] = (x1-3)^2 + x1*x2 + (x2+4)^2 - 3 with x1 = x[k], x2 = x[n+k]
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_f_nonsquare(T *__restrict__ fx, const T *__restrict__ x, int64_t n, int64_t xs, int64_t fs, int64_t r0, int64_t r1)
{
    const T *xb = x + (int64_t)blockIdx.y * xs;
    T *fb = fx + (int64_t)blockIdx.y * fs;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = r0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; k < r1; k += stride) {
        const T a = xb[k], b = xb[n + k];
        fb[k] = ((((a - 3.0) * (a - 3.0)) + a * b) + ((b + 4.0) * (b + 4.0))) - 3.0;
    }
}

struct BuiltinF {
    uint32_t magic = 0xFD0F00D5u;
    fd_ctx *ctx = nullptr;
    int family = 0;
    int64_t prm[3] = {0, 0, 0};
    int64_t M = 0, N = 0;
    int32_t *d_srow = nullptr, *d_scol = nullptr;   // FD_F_SPARSE: the pattern by rows (rowptr[M + 1], ascending columns), device
    int32_t *d_sdest = nullptr;                     //   per entry of that list: its slot in the CSC order it was built from (k_f_sparse_store_rows)
    std::vector<int32_t> h_colptr;                  //   that CSC pattern's column offsets (0-based), host
    struct RowsMemo {                               //   what the launcher knows about a plan (fd_csc_store.plan_serial): is its pattern mine?
        int verdict = 0;
        bool pending = false;
        hipEvent_t ev = nullptr;
        unsigned long long *h_note = nullptr;       //   pinned
    };
    std::atomic<int64_t> row_stores{0};
    std::unordered_map<unsigned long long, RowsMemo> rows_memo;
    std::mutex rows_mutex;
    std::atomic<int64_t> launches{0}, points{0};
    void *d_sig = nullptr;  // block-coupled sigma scratch
    int64_t sig_cap = 0;    // in (re,im)-capable elements
};

int balanced_grid(int64_t tiles, int64_t cap);

// grid.x covers `rows` work items of one point, grid.y = points; whole rounds (see balanced_grid)
static inline dim3 grid2(int64_t rows, int64_t nbatch, int num_cus)
{
    // one work item per thread, uncapped (N = 10^7 tridiagonal f!: 65 -> 59 us per launch against a capped grid, profiles/r04_b_*)
    (void)num_cus;
    const int64_t tiles = (rows + kBlock - 1) / kBlock;
    return dim3((unsigned)balanced_grid(tiles, (int64_t)1 << 30), (unsigned)nbatch, 1);
}

#include "fdjac_functor_f.hip"

template <typename T>
static int launch_family(BuiltinF *b, void *fx, const void *x, int64_t nbatch, int64_t xs, int64_t fs, int64_t r0,
                         int64_t r1, hipStream_t s)
{
    if (r1 <= r0) return 0;
    if (b->family == FD_F_LAP7 || b->family == FD_F_SPARSE) return functor_family_launch<T>(b, fx, x, nbatch, xs, fs, r0, r1, s);
    const int ncu = b->ctx->num_cus;
    T *fxp = (T *)fx;
    const T *xp = (const T *)x;
    const dim3 g = grid2(r1 - r0, nbatch, ncu);
    switch (b->family) {
    case FD_F_TRIDIAG:
    case FD_F_TRIDIAG_NL: {
        const bool nl = b->family == FD_F_TRIDIAG_NL;
        if constexpr (sizeof(T) == sizeof(real_t)) {
            const bool aligned = ((((uintptr_t)fx) | ((uintptr_t)x)) & kPairMask) == 0 && (xs % 2 == 0 || nbatch == 1) &&
                                 (fs % 2 == 0 || nbatch == 1);
            if (aligned) {
                const int64_t r0e = r0 & ~(int64_t)1;
                const dim3 g2 = grid2((r1 - r0e + 1) / 2, nbatch, ncu);
                fd_pick<false, true>(nl, [&](auto NL) {
                    hipLaunchKernelGGL((k_f_tridiag_v2<NL()>), g2, dim3(kBlock), 0, s, (real_t *)fx, (const real_t *)x, b->prm[0], xs, fs,
                                       r0e, r1);
                });
                break;
            }
        }
        fd_pick<false, true>(nl, [&](auto NL) {
            hipLaunchKernelGGL((k_f_tridiag<T, NL()>), g, dim3(kBlock), 0, s, fxp, xp, b->prm[0], xs, fs, r0, r1);
        });
        break;
    }
    case FD_F_LAP5:
    case FD_F_LAP5_NL:
    case FD_F_CLAMP5: {
        const int sk = b->family == FD_F_CLAMP5 ? 1 : b->family == FD_F_LAP5_NL ? 2 : 0;
        if constexpr (sizeof(T) == sizeof(real_t)) {
            const bool ok = ((((uintptr_t)fx) | ((uintptr_t)x)) & kPairMask) == 0 && (xs % 2 == 0 || nbatch == 1) &&
                            (fs % 2 == 0 || nbatch == 1) && (b->prm[0] % 2 == 0);
            if (ok) {
                const int64_t r0e = r0 & ~(int64_t)1;
                const int64_t ntiles = (r1 - r0e + 2 * kBlock - 1) / (2 * kBlock);
                const dim3 g2((unsigned)(8 * xcd_chunks(ntiles)), (unsigned)nbatch, 1);
                fd_pick<0, 1, 2>(sk, [&](auto SK) {
                    hipLaunchKernelGGL((k_f_stencil5_v2<SK()>), g2, dim3(kBlock), 0, s, (real_t *)fx, (const real_t *)x, b->prm[0], b->prm[1],
                                       xs, fs, r0e, r1);
                });
                break;
            }
        }
        fd_pick<0, 1, 2>(sk, [&](auto SK) {
            hipLaunchKernelGGL((k_f_stencil5<T, SK()>), g, dim3(kBlock), 0, s, fxp, xp, b->prm[0], b->prm[1], xs, fs, r0, r1);
        });
        break;
    }
    case FD_F_BLOCKCOUPLED: {
        const int64_t nb = b->prm[0], bs = b->prm[1];
        if (b->sig_cap < nbatch * nb) {
            if (b->d_sig) (void)hipFree(b->d_sig);
            b->d_sig = nullptr;
            if (hipMalloc(&b->d_sig, (size_t)(nbatch * nb) * 2 * sizeof(real_t)) != hipSuccess) return 2;
            b->sig_cap = nbatch * nb;
        }
        const int64_t b0 = std::max<int64_t>(r0 / bs - 1, 0), b1 = std::min<int64_t>((r1 + bs - 1) / bs + 1, nb);
        const dim3 gs = grid2((b1 - b0) * 64, nbatch, ncu);
        hipLaunchKernelGGL((k_f_block_sigma<T>), gs, dim3(kBlock), 0, s, (T *)b->d_sig, xp, nb, bs, xs, b0, b1);
        hipLaunchKernelGGL((k_f_block_apply<T>), g, dim3(kBlock), 0, s, fxp, xp, (const T *)b->d_sig, nb, bs, xs, fs, r0, r1);
        break;
    }
    case FD_F_NONSQUARE:
        hipLaunchKernelGGL((k_f_nonsquare<T>), g, dim3(kBlock), 0, s, fxp, xp, b->prm[0], xs, fs, r0, r1);
        break;
    default: return 3;
    }
    return launch_rc();
}

static int builtin_launch(void *fctx, void *fx, const void *x, int64_t nbatch, int64_t x_stride, int64_t fx_stride,
                          int64_t row_begin, int64_t row_end, int is_complex, void *stream)
{
    BuiltinF *b = (BuiltinF *)fctx;
    if (!b || b->magic != 0xFD0F00D5u) return 1;
    if (nbatch <= 0) return 0;
    if (nbatch > 65535) return 5;
    b->launches.fetch_add(1);
    b->points.fetch_add(nbatch);
    const int64_t r0 = std::max<int64_t>(row_begin, 0), r1 = std::min<int64_t>(row_end, b->M);
    if (is_complex)
        return launch_family<cd>(b, fx, x, nbatch, x_stride, fx_stride, r0, r1, (hipStream_t)stream);
    return launch_family<real_t>(b, fx, x, nbatch, x_stride, fx_stride, r0, r1, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Lazy-point evaluation (fd_f_launch_lazy): each thread loads the base x values and colours its
// rows depend on ONCE, then evaluates the fixture at every point of the batch by perturbing in
// registers -- x~ = x + eps_b*[color==b] (src/jacobians.jl:562 / 603-604 / 633) -- so the perturbed
// points never exist in memory and x is read once for all colours.  Values are bit-identical to
// evaluating the materialised points.  MODE 0 forward, 1 central (+ then -), 2 complex step.
// One file per family, each with its kernels directly above its launcher; the JVP's lazy points last.
// ---------------------------------------------------------------------------------------------
#include "fdjac_f_tridiag.hip"
#include "fdjac_f_stencil5.hip"
#include "fdjac_f_blockcoupled.hip"
#include "fdjac_f_jvp.hip"

static bool has_lazy(const BuiltinF *b)
{
    if (b->family == FD_F_TRIDIAG || b->family == FD_F_TRIDIAG_NL || b->family == FD_F_LAP7 || b->family == FD_F_SPARSE) return true;
    if (b->family == FD_F_BLOCKCOUPLED) return b->prm[1] <= 64;   // one wave per block
    return (b->family == FD_F_LAP5 || b->family == FD_F_CLAMP5 || b->family == FD_F_LAP5_NL) && (b->prm[0] % 2 == 0);  // pairs must not straddle grid rows
}

static int builtin_launch_lazy(void *fctx, void *fx, const fd_lazy_points *lp, int64_t fx_stride, int64_t row_begin,
                               int64_t row_end, void *stream)
{
    BuiltinF *b = (BuiltinF *)fctx;
    if (!b || b->magic != 0xFD0F00D5u || !lp) return 1;
    if (!has_lazy(b)) return 6;
    if (b->family == FD_F_LAP7 || b->family == FD_F_SPARSE) {      // functor families: the column-by-column store, or nothing
        const int rc = lp->color_bytes == 1 ? functor_family_lazy<uint8_t>(b, lp, (hipStream_t)stream) : functor_family_lazy<int32_t>(b, lp, (hipStream_t)stream);
        if (rc == 0) {
            b->launches.fetch_add(1);
            // (f(x) of a forward difference: one plain launch, counted there -- or, FD_LAZY_CAP_STORE_CSC_BASE without f_in, formed
            //  inside this launch: counted with the first colour chunk)
            const bool own_base = lp->pts == 1 && !lp->is_complex && lp->store && !((const fd_csc_store *)lp->store)->fx_base && lp->c_lo == 0;
            b->points.fetch_add((int64_t)lp->ncolors * lp->pts + (own_base ? 1 : 0));
        }
        return rc;
    }
    // 16-B vector accesses: bases are hipMalloc/torch allocations, fx_stride is a multiple of 32 elements
    if (((((uintptr_t)fx) | ((uintptr_t)lp->base_out)) & kPairMask) != 0 || (fx_stride & 1)) return 7;
    if (lp->diff && (b->family == FD_F_BLOCKCOUPLED || lp->is_complex || lp->base_out)) return 8;   // (not registered with FD_LAZY_CAP_DIFF)
    if (lp->store && !((lp->diff && (b->family == FD_F_TRIDIAG || b->family == FD_F_TRIDIAG_NL || b->family == FD_F_LAP5 || b->family == FD_F_LAP5_NL)) ||
                       (b->family == FD_F_BLOCKCOUPLED && lp->is_complex)))
        return 9;   // (FD_LAZY_CAP_STORE: the tridiagonal and Laplacian families; the block-coupled family in the complex step)
    const int64_t npts = (int64_t)lp->ncolors * lp->pts + ((lp->base_out || lp->diff == 2) ? 1 : 0);
    // the block-coupled kernel keeps one sigma per (block, point) in LDS: decline batches that would not fit
    if (b->family == FD_F_BLOCKCOUPLED && !lp->store && bc_lds_bytes(lp->ncolors, lp->pts, lp->is_complex != 0) > (size_t)56 * 1024)
        return FD_LAZY_DECLINED;
    const bool count_points = lp->nparts <= 1 || lp->part == 0;   // row strips: the parts together are ONE evaluation per point
    b->launches.fetch_add(1);
    if (count_points) b->points.fetch_add(npts);
    const int64_t r0 = std::max<int64_t>(row_begin, 0), r1 = std::min<int64_t>(row_end, b->M);
    if (r1 <= r0 || lp->ncolors <= 0) return 0;
    const hipStream_t s = (hipStream_t)stream;
    int rc;
    if (b->family == FD_F_BLOCKCOUPLED)
        rc = lp->color_bytes == 1 ? lazy_blockcoupled_launch<uint8_t>(b, fx, lp, fx_stride, r0, r1, s)
                                  : lazy_blockcoupled_launch<int32_t>(b, fx, lp, fx_stride, r0, r1, s);
    else if (b->family == FD_F_LAP5 || b->family == FD_F_CLAMP5 || b->family == FD_F_LAP5_NL)
        rc = lp->color_bytes == 1 ? lazy_stencil5_launch<uint8_t>(b, fx, lp, fx_stride, r0, r1, s)
                                  : lazy_stencil5_launch<int32_t>(b, fx, lp, fx_stride, r0, r1, s);
    else
        rc = lp->color_bytes == 1 ? lazy_tridiag_launch<uint8_t>(b, fx, lp, fx_stride, r0, r1, s)
                                  : lazy_tridiag_launch<int32_t>(b, fx, lp, fx_stride, r0, r1, s);
    if (rc == FD_LAZY_DECLINED) {   // nothing was enqueued: the library materialises / re-asks, and counts then
        b->launches.fetch_sub(1);
        if (count_points) b->points.fetch_sub(npts);
    }
    return rc;
}

}  // namespace fdjac

using namespace fdjac;

extern "C" {

int fd_builtin_f_create(fd_ctx *ctx, int family, const int64_t *params, int nparams, fd_f_launch *fn_out,
                        void **fctx_out)
{
    FD_REQUIRE(ctx && params && fn_out && fctx_out, FD_ERR_ARG, "NULL argument");
    BuiltinF *b = new (std::nothrow) BuiltinF();
    FD_REQUIRE(b != nullptr, FD_ERR_NOMEM, "out of host memory");
    b->ctx = ctx;
    b->family = family;
    int need = 1;
    switch (family) {
    case FD_F_TRIDIAG:
    case FD_F_TRIDIAG_NL: need = 1; break;
    case FD_F_LAP5:
    case FD_F_LAP5_NL:
    case FD_F_CLAMP5:
    case FD_F_BLOCKCOUPLED: need = 2; break;
    case FD_F_NONSQUARE: need = 1; break;
    case FD_F_LAP7: need = 3; break;
    default:
        delete b;
        set_error(family == FD_F_SPARSE ? "FD_F_SPARSE is created by fd_builtin_f_create_sparse" : "unknown built-in f family %d", family);
        return FD_ERR_ARG;
    }
    if (nparams < need) {
        delete b;
        set_error("family %d needs %d parameters", family, need);
        return FD_ERR_ARG;
    }
    for (int i = 0; i < need; ++i) b->prm[i] = params[i];
    for (int i = 0; i < need; ++i)
        if (b->prm[i] < 1) {
            delete b;
            set_error("parameters must be >= 1");
            return FD_ERR_ARG;
        }
    switch (family) {
    case FD_F_TRIDIAG:
    case FD_F_TRIDIAG_NL: b->M = b->N = b->prm[0]; break;
    case FD_F_NONSQUARE: b->M = b->prm[0]; b->N = 2 * b->prm[0]; break;
    case FD_F_LAP7:
        b->M = b->N = b->prm[0] * b->prm[1] * b->prm[2];
        if (b->prm[0] * b->prm[1] >= ((int64_t)1 << 31) || b->M >= ((int64_t)1 << 31)) {      // (32-bit grid arithmetic in the kernels)
            delete b;
            set_error("grid too large for the 7-point family");
            return FD_ERR_ARG;
        }
        break;
    default: b->M = b->N = b->prm[0] * b->prm[1]; break;
    }
    *fn_out = builtin_launch;
    *fctx_out = b;
    return FD_OK;
}

// FD_F_SPARSE: the pattern arrives as the CSC pattern of the Jacobian; the launcher keeps its transpose (rows, ascending columns)
int fd_builtin_f_create_sparse(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base,
                               fd_f_launch *fn_out, void **fctx_out)
{
    FD_REQUIRE(ctx && colptr && rowval && fn_out && fctx_out, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(idx_bytes == 4 || idx_bytes == 8, FD_ERR_ARG, "idx_bytes must be 4 or 8");
    FD_REQUIRE(idx_base == 0 || idx_base == 1, FD_ERR_ARG, "idx_base must be 0 or 1");
    FD_REQUIRE(M >= 1 && N >= 1 && M < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), FD_ERR_ARG, "bad shape");
    auto ld = [&](const void *p, int64_t i) { return idx_bytes == 8 ? ((const int64_t *)p)[i] : (int64_t)((const int32_t *)p)[i]; };
    const int64_t nnz = ld(colptr, N) - idx_base;
    FD_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31), FD_ERR_SHAPE, "colptr is not monotone / too many entries");
    std::vector<int32_t> srow((size_t)M + 1, 0), scol((size_t)std::max<int64_t>(nnz, 1)), sdest((size_t)std::max<int64_t>(nnz, 1)), hcp((size_t)N + 1);
    for (int64_t j = 0; j < N; ++j) {
        const int64_t a = ld(colptr, j) - idx_base, b2 = ld(colptr, j + 1) - idx_base;
        FD_REQUIRE(a >= 0 && a <= b2 && b2 <= nnz, FD_ERR_SHAPE, "colptr is not monotone at column %lld", (long long)j);
        hcp[(size_t)j] = (int32_t)a;
        hcp[(size_t)j + 1] = (int32_t)b2;
        for (int64_t q = a; q < b2; ++q) {
            const int64_t r = ld(rowval, q) - idx_base;
            FD_REQUIRE(r >= 0 && r < M, FD_ERR_SHAPE, "rowval[%lld] outside the matrix", (long long)q);
            ++srow[(size_t)r + 1];
        }
    }
    for (int64_t r = 0; r < M; ++r) srow[(size_t)r + 1] += srow[(size_t)r];
    {
        std::vector<int32_t> cur(srow.begin(), srow.end() - 1);
        for (int64_t j = 0; j < N; ++j)       // columns ascending: every row's entries end up in ascending column order
            for (int64_t q = ld(colptr, j) - idx_base; q < ld(colptr, j + 1) - idx_base; ++q) {
                const size_t at = (size_t)cur[(size_t)(ld(rowval, q) - idx_base)]++;
                scol[at] = (int32_t)j;
                sdest[at] = (int32_t)q;
            }
    }
    BuiltinF *b = new (std::nothrow) BuiltinF();
    FD_REQUIRE(b != nullptr, FD_ERR_NOMEM, "out of host memory");
    b->ctx = ctx;
    b->family = FD_F_SPARSE;
    b->M = M;
    b->N = N;
    b->prm[0] = M; b->prm[1] = N; b->prm[2] = nnz;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_srow, sizeof(int32_t) * srow.size());
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_scol, sizeof(int32_t) * scol.size());
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_sdest, sizeof(int32_t) * sdest.size());
    if (e == hipSuccess) e = hipMemcpy(b->d_sdest, sdest.data(), sizeof(int32_t) * sdest.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_srow, srow.data(), sizeof(int32_t) * srow.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_scol, scol.data(), sizeof(int32_t) * scol.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("uploading the pattern of the sparse family failed: %s", hipGetErrorString(e));
        if (b->d_srow) (void)hipFree(b->d_srow);
        if (b->d_scol) (void)hipFree(b->d_scol);
        if (b->d_sdest) (void)hipFree(b->d_sdest);
        delete b;
        return FD_ERR_HIP;
    }
    b->h_colptr.swap(hcp);
    *fn_out = builtin_launch;
    *fctx_out = b;
    return FD_OK;
}

int fd_builtin_f_destroy(void *fctx)
{
    BuiltinF *b = (BuiltinF *)fctx;
    if (!b) return FD_OK;
    FD_REQUIRE(b->magic == 0xFD0F00D5u, FD_ERR_ARG, "not a built-in f context");
    if (b->d_sig) (void)hipFree(b->d_sig);
    if (b->d_srow) (void)hipFree(b->d_srow);
    if (b->d_scol) (void)hipFree(b->d_scol);
    if (b->d_sdest) (void)hipFree(b->d_sdest);
    for (auto &kv : b->rows_memo) {
        if (kv.second.pending) (void)hipEventSynchronize(kv.second.ev);      // (a copy into the pinned word may still be in flight)
        if (kv.second.ev) (void)hipEventDestroy(kv.second.ev);
        if (kv.second.h_note) (void)hipHostFree(kv.second.h_note);
    }
    b->magic = 0;
    delete b;
    return FD_OK;
}

int fd_builtin_f_lazy(void *fctx, fd_f_launch_lazy *fn_out)
{
    BuiltinF *b = (BuiltinF *)fctx;
    FD_REQUIRE(b && b->magic == 0xFD0F00D5u && fn_out, FD_ERR_ARG, "not a built-in f context");
    if (!has_lazy(b)) {
        set_error("family %d has no lazy-point launcher (5-point stencils need an even nx)", b->family);
        return FD_ERR_UNSUPPORTED;
    }
    *fn_out = builtin_launch_lazy;
    return FD_OK;
}

int fd_builtin_f_lazy_jvp(void *fctx, fd_f_launch_lazy_jvp *fn_out)
{
    BuiltinF *b = (BuiltinF *)fctx;
    FD_REQUIRE(b && b->magic == 0xFD0F00D5u && fn_out, FD_ERR_ARG, "not a built-in f context");
    if (!has_lazy_jvp(b)) {
        set_error("family %d has no lazy JVP launcher (5-point stencils need an even nx)", b->family);
        return FD_ERR_UNSUPPORTED;
    }
    *fn_out = builtin_launch_lazy_jvp;
    return FD_OK;
}

int fd_builtin_f_lazy_jvp_caps(void *fctx, int *caps_out)
{
    BuiltinF *b = (BuiltinF *)fctx;
    FD_REQUIRE(b && b->magic == 0xFD0F00D5u && caps_out, FD_ERR_ARG, "bad argument");
    *caps_out = has_lazy_jvp(b) ? FD_LAZY_JVP_CAP_QUOTIENT : 0;
    return FD_OK;
}

int fd_builtin_f_lazy_caps(void *fctx, int *caps_out)
{
    BuiltinF *b = (BuiltinF *)fctx;
    FD_REQUIRE(b && b->magic == 0xFD0F00D5u && caps_out, FD_ERR_ARG, "not a built-in f context");
    // the tridiagonal and 5-point kernels write exactly the (pair-rounded) row window they are handed; the block-coupled
    // kernel writes whole blocks, so it does not claim FD_LAZY_CAP_ROW_WINDOW
    if (b->family == FD_F_LAP7 || b->family == FD_F_SPARSE) {      // functor families: the column-by-column store only
        // (a 7-point row costs less than the gather of its f(x), and the sparse family's row-wise store has f(x) of its rows anyway: both
        //  evaluate the unperturbed rows inside the storing launch)
        *caps_out = FD_LAZY_CAP_STORE_CSC | FD_LAZY_CAP_STORE_CSC_COMPLEX | FD_LAZY_CAP_STORE_CSC_BASE;
        return FD_OK;
    }
    *caps_out = has_lazy(b) ? (FD_LAZY_CAP_IMAG_ONLY | (b->family == FD_F_BLOCKCOUPLED ? 0 : (FD_LAZY_CAP_ROW_WINDOW | FD_LAZY_CAP_DIFF)) |
                               ((b->family == FD_F_TRIDIAG || b->family == FD_F_TRIDIAG_NL || b->family == FD_F_LAP5 || b->family == FD_F_LAP5_NL ||
                                 b->family == FD_F_BLOCKCOUPLED) ? FD_LAZY_CAP_STORE : 0) |
                               ((b->family == FD_F_TRIDIAG || b->family == FD_F_TRIDIAG_NL) ? FD_LAZY_CAP_FUSED_EPS : 0)) : 0;
    return FD_OK;
}

int fd_builtin_f_counts(void *fctx, int64_t *launches, int64_t *points)
{
    BuiltinF *b = (BuiltinF *)fctx;
    FD_REQUIRE(b && b->magic == 0xFD0F00D5u, FD_ERR_ARG, "not a built-in f context");
    if (launches) *launches = b->launches.load();
    if (points) *points = b->points.load();
    return FD_OK;
}

int fd_builtin_f_info(void *fctx, int key, int64_t *value)
{
    BuiltinF *b = (BuiltinF *)fctx;
    FD_REQUIRE(b && b->magic == 0xFD0F00D5u && value, FD_ERR_ARG, "not a built-in f context");
    FD_REQUIRE(key == FD_F_INFO_ROW_STORES, FD_ERR_ARG, "unknown key %d", key);
    *value = b->row_stores.load();
    return FD_OK;
}

}  // extern "C"
