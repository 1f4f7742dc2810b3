// Column colouring ON THE DEVICE (include/fdjac.h: fd_color_columns_device, fd_color_check_device) -- the step before
// fd_plan_create_csc_device for a caller whose pattern lives in HBM.  Element-type independent: built once, not in the Float32 pass.
//
// CONTRACT.  The column intersection graph (two columns conflict when they share a row) is coloured by Jones-Plassmann under the
// fixed priority color_prio(j) below, a bijection of the 64-bit integers (no ties): a column takes the smallest colour (1-based) that
// no conflicting column of HIGHER priority uses, as soon as all of those are coloured.  The result is therefore the sequential greedy
// colouring in order of descending priority -- a function of the pattern alone, whatever the grid, the number of rounds or the order
// in which neighbours finish.  A colour word goes 0 -> c exactly once (agent-scope atomic store, read by agent-scope atomic loads), so
// a stale or same-round read shows "not coloured yet" and costs a round, never a wrong colour.  tests/color_model.py restates the
// priority and the greedy order in numpy; tests/test_gpu_color.py compares element for element.
//
// Two facts keep the walk short.  A neighbour k that IS coloured while j is not has the higher priority (a lower one would still be
// waiting for j), so only an uncoloured neighbour's priority is ever computed.  And the colours a ready column reads are final.
//
// SCHEDULE.  (1) validate colptr / rowval and transpose the pattern (row counts by atomics, an exclusive scan, a fill pass: the order
// inside a row list depends on the atomics' arrival order -- the colouring only ever asks for the SET of colours in a row, so the
// result does not; nothing is sorted).  (2) rounds over a worklist of uncoloured columns, kColorBatch launches per read-back of the
// list lengths (a launch on an empty list exits at once); a column whose walk (sum of its rows' lengths) is short is handled by a
// lane with a 64-colour register mask, a long one by a wavefront with a 4096-colour bit map in LDS; a full window repeats the walk
// for the next one.  (3) once the list fits one workgroup (kColorTail columns) ONE launch finishes it: the workgroup loops over the
// levels with barriers, lists in LDS -- a row of d columns needs d levels under any greedy order, and d launches would be the cost
// otherwise.  Every loop is bounded: a level colours at least the highest-priority remaining column; one that colours nothing is
// reported (FD_ERR_HIP), not spun on.
#include <algorithm>
#include <climits>
#include <cstring>

#include "fdjac_internal.h"

namespace fdjac {

constexpr int kColorLaneWork = 256;     // a column whose rows hold at most this many entries in all is walked by one lane (tuning only)
constexpr int kColorWorkCap = 4096;     // ... a row adds at most this much to that sum (the sum is a 32-bit classification, not a count)
constexpr int kColorTail = 4096;        // the one-workgroup tail takes over at this many uncoloured columns
constexpr int kColorTailBlock = 1024;   // ... with this many threads
constexpr int kColorBatch = 8;          // rounds enqueued per read-back of the worklist lengths
constexpr int kColorWaveWin = 4096;     // colours per pass of a wavefront's LDS bit map (128 words)
constexpr int kCheckLaneLen = 16;       // fd_color_check_device: rows up to this length are compared pairwise by one lane

enum { COL_BAD_ROW = 1, COL_BAD_COLPTR = 2 };
struct ColStats {
    unsigned flags;                     // COL_*
    int nwork;                          // columns with entries (the first worklist's length)
    int max_color;
    int stuck;                          // a tail level coloured nothing
    int tail_levels;
    int pad;
    unsigned long long bad_rows;        // fd_color_check_device
};

// The priority: murmur3's 64-bit finaliser of j + 0x9E3779B97F4A7C15 (mod 2^64).  Every step is invertible, so distinct columns have
// distinct priorities.  Stated in include/fdjac.h, restated in tests/color_model.py, pinned by tests/test_color_cpu.py.
__host__ __device__ __forceinline__ uint64_t color_prio(uint64_t j)
{
    uint64_t x = j + 0x9E3779B97F4A7C15ull;
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ int64_t col_load(const void *p, int bytes, int64_t i)      // (fdjac_planbuild.hip: pb_load)
{
    return bytes == 8 ? ((const int64_t *)p)[i] : (int64_t)((const int32_t *)p)[i];
}
__device__ __forceinline__ int ld_color(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_color(int *p, int c) { __hip_atomic_store(p, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the lanes of a wavefront that `keep` append their item to list[*cnt...]: one atomic per wavefront.  Wave-uniform control flow only.
__device__ __forceinline__ void wave_append(bool keep, int item, int *list, int *cnt)
{
    const unsigned long long m = __ballot(keep);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(cnt, __popcll(m));
    base = __shfl(base, 0, 64);
    if (keep) list[base + __popcll(m & ((1ull << lane) - 1ull))] = item;
}

// ---- step 1: validation and the transposed pattern -------------------------------------------------------------------------------
// cptr[j] = colptr[j] - base - e0 (int32, clamped into [0, nnz] so that nothing downstream can leave its arrays)
__global__ void __launch_bounds__(kBlock) k_col_colptr(const void *__restrict__ colptr, int ib, int base, int64_t N, int64_t e0, int64_t e1,
                                                       int *__restrict__ cptr, ColStats *st)
{
    bool bad = false;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j <= N; j += (int64_t)gridDim.x * kBlock) {
        const int64_t a = col_load(colptr, ib, j) - base;
        if (j < N) bad = bad || a > col_load(colptr, ib, j + 1) - base;
        bad = bad || a < e0 || a > e1;
        cptr[j] = (int)(std::min<int64_t>(std::max<int64_t>(a, e0), e1) - e0);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&st->flags, (unsigned)COL_BAD_COLPTR);
}

__global__ void __launch_bounds__(kBlock) k_col_count(const void *__restrict__ rowval, int ib, int base, int64_t e0, int64_t nnz, int64_t M,
                                                      int *__restrict__ erow, int *__restrict__ rcnt, ColStats *st)
{
    bool bad = false;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kBlock) {
        const int64_t r = col_load(rowval, ib, e0 + q) - base;
        const bool ok = r >= 0 && r < M;
        bad = bad || !ok;
        erow[q] = ok ? (int)r : 0;
        if (ok) atomicAdd(&rcnt[r], 1);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&st->flags, (unsigned)COL_BAD_ROW);
}

// exclusive scan of in[0, n) into out[0, n], out[n] = the total: tile sums, one workgroup over the sums, tiles again
constexpr int kScanPer = 8, kScanTile = kBlock * kScanPer;
__device__ __forceinline__ int block_exscan(int v, int *s_w, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; ++i) {
        if (i < w) before += s_w[i];
        total += s_w[i];
    }
    return before + inc - v;
}
__global__ void __launch_bounds__(kBlock) k_col_scan_sums(const int *__restrict__ in, int64_t n, int *__restrict__ bsum)
{
    __shared__ int s_w[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) s += i0 + k < n ? in[i0 + k] : 0;
    int total;
    (void)block_exscan(s, s_w, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kBlock) k_col_scan_top(int *__restrict__ bsum, int64_t nb)      // in place; bsum[nb] = the total
{
    __shared__ int s_w[kBlock / 64];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kBlock) {
        const int64_t i = b0 + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int total;
        const int ex = block_exscan(v, s_w, total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}
__global__ void __launch_bounds__(kBlock) k_col_scan_apply(const int *__restrict__ in, int64_t n, const int *__restrict__ bsum, int64_t nb,
                                                           int *__restrict__ out)
{
    __shared__ int s_w[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    int v[kScanPer], s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        v[k] = i0 + k < n ? in[i0 + k] : 0;
        s += v[k];
    }
    int total;
    int run = bsum[blockIdx.x] + block_exscan(s, s_w, total);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

// every entry finds its column by a binary search in cptr (monotone: checked before this runs) and joins its row's list
__global__ void __launch_bounds__(kBlock) k_col_fill(const int *__restrict__ cptr, const int *__restrict__ erow, int64_t N, int64_t nnz,
                                                     const int *__restrict__ rptr, int *__restrict__ cursor, int *__restrict__ rcols,
                                                     int *__restrict__ work)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kBlock) {
        int64_t lo = 0, hi = N;      // cptr[lo] <= q < cptr[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (cptr[mid] <= q) lo = mid; else hi = mid;
        }
        const int r = erow[q];
        const int a = rptr[r], len = rptr[r + 1] - a;
        const int pos = atomicAdd(&cursor[r], 1);
        if (pos < len) rcols[a + pos] = (int)lo;
        if (work) atomicAdd(&work[lo], len < kColorWorkCap ? len : kColorWorkCap);
    }
}

// ---- step 2: the rounds ------------------------------------------------------------------------------------------------------------
// columns without entries get colour 1 (as the host greedy gives them); the others start at 0 and form the first worklist
__global__ void __launch_bounds__(kBlock) k_col_init(const int *__restrict__ cptr, int64_t N, int *__restrict__ color, int *__restrict__ list,
                                                     ColStats *st)
{
    for (int64_t b0 = (int64_t)blockIdx.x * kBlock; b0 < N; b0 += (int64_t)gridDim.x * kBlock) {
        const int64_t j = b0 + threadIdx.x;
        const bool has = j < N && cptr[j + 1] > cptr[j];
        if (j < N) color[j] = has ? 0 : 1;
        wave_append(has, (int)j, list, &st->nwork);
    }
}

struct ColGraph {
    const int *cptr, *erow, *rptr, *rcols, *work;
    int *color;
};

// one lane: the colour of column j, or 0 while a higher-priority neighbour is uncoloured
__device__ __forceinline__ int color_try_lane(const ColGraph &g, int j)
{
    const uint64_t pj = color_prio((uint64_t)j);
    const int qa = g.cptr[j], qb = g.cptr[j + 1];
    for (int wb = 0;; wb += 64) {
        unsigned long long forb = 0;
        for (int q = qa; q < qb; ++q) {
            const int r = g.erow[q];
            const int tb = g.rptr[r + 1];
            for (int t = g.rptr[r]; t < tb; ++t) {
                const int k = g.rcols[t];
                const int c = ld_color(g.color + k);
                if (c == 0) {
                    if (k != j && color_prio((uint64_t)k) > pj) return 0;
                } else {
                    const unsigned d = (unsigned)(c - 1 - wb);
                    if (d < 64u) forb |= 1ull << d;
                }
            }
        }
        if (~forb) return wb + __ffsll((unsigned long long)~forb);
    }
}

// one wavefront: lanes stride each row's columns; the forbidden colours of a window are OR-ed into the wavefront's LDS bit map
__device__ __forceinline__ int color_try_wave(const ColGraph &g, int j, unsigned *bm)
{
    const int lane = threadIdx.x & 63;
    const uint64_t pj = color_prio((uint64_t)j);
    const int qa = g.cptr[j], qb = g.cptr[j + 1];
    for (int wb = 0;; wb += kColorWaveWin) {
        bm[lane] = 0;
        bm[lane + 64] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int q = qa; q < qb; ++q) {
            const int r = g.erow[q];
            const int ta = g.rptr[r], tb = g.rptr[r + 1];
            for (int t0 = ta; t0 < tb; t0 += 64) {
                const int t = t0 + lane;
                bool wait = false;
                if (t < tb) {
                    const int k = g.rcols[t];
                    const int c = ld_color(g.color + k);
                    if (c == 0) {
                        wait = k != j && color_prio((uint64_t)k) > pj;
                    } else {
                        const unsigned d = (unsigned)(c - 1 - wb);
                        if (d < (unsigned)kColorWaveWin) atomicOr(&bm[d >> 5], 1u << (d & 31));
                    }
                }
                if (__ballot(wait)) return 0;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const unsigned f0 = ~bm[lane], f1 = ~bm[lane + 64];
        int cand = f0 ? lane * 32 + __ffs(f0) - 1 : (f1 ? (lane + 64) * 32 + __ffs(f1) - 1 : INT_MAX);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off, 64));
        __builtin_amdgcn_wave_barrier();
        if (cand != INT_MAX) return wb + cand + 1;
    }
}

// item i of list_in[0, n): colour it or keep it for the next round.  Called by whole wavefronts (i may lie outside the list).
__device__ __forceinline__ void color_step(const ColGraph &g, int i, int n, const int *list_in, int *list_out, int *cnt_out, unsigned *bm)
{
    const int lane = threadIdx.x & 63;
    const int j = i < n ? list_in[i] : -1;
    const bool is_long = j >= 0 && (g.work[j] > kColorLaneWork || g.cptr[j + 1] - g.cptr[j] > kColorLaneWork);
    bool pend = false;
    if (j >= 0 && !is_long) {
        const int c = color_try_lane(g, j);
        if (c) st_color(g.color + j, c); else pend = true;
    }
    unsigned long long m = __ballot(is_long);
    while (m) {
        const int src = __ffsll(m) - 1;
        m &= m - 1;
        const int jj = __shfl(j, src, 64);
        const int c = color_try_wave(g, jj, bm);
        if (lane == src) {
            if (c) st_color(g.color + j, c); else pend = true;
        }
    }
    wave_append(pend, j, list_out, cnt_out);
}

// one round: cnt[0] = the length of list_in, cnt[1] (zeroed by the host) receives the length of list_out
__global__ void __launch_bounds__(kBlock) k_col_round(ColGraph g, const int *__restrict__ list_in, int *__restrict__ list_out, int *cnt)
{
    __shared__ unsigned s_bm[kBlock / 64][128];
    const int n = cnt[0];
    if ((int64_t)blockIdx.x * kBlock >= n) return;
    color_step(g, (int)(blockIdx.x * kBlock + threadIdx.x), n, list_in, list_out, cnt + 1, s_bm[threadIdx.x >> 6]);
}

// ---- step 3: the tail -- ONE workgroup finishes a short list, a barrier per level ------------------------------------------------
// The workgroup is alone in its launch: there is no cross-workgroup progress assumption.  Colours still travel through global memory
// (agent-scope atomics, a fence and a barrier per level); the lists live in LDS.
__global__ void __launch_bounds__(kColorTailBlock) k_col_tail(ColGraph g, const int *__restrict__ list_in, int n0, ColStats *st)
{
    __shared__ int s_list[2][kColorTail];
    __shared__ unsigned s_bm[kColorTailBlock / 64][128];
    __shared__ int s_cnt[2];
    for (int i = threadIdx.x; i < n0; i += kColorTailBlock) s_list[0][i] = list_in[i];
    if (threadIdx.x == 0) s_cnt[0] = n0;
    int cur = 0, levels = 0;
    for (;;) {
        __syncthreads();
        const int n = s_cnt[cur];
        if (n == 0) break;
        if (threadIdx.x == 0) s_cnt[cur ^ 1] = 0;
        __syncthreads();
        for (int b0 = 0; b0 < n; b0 += kColorTailBlock)
            color_step(g, b0 + (int)threadIdx.x, n, s_list[cur], s_list[cur ^ 1], &s_cnt[cur ^ 1], s_bm[threadIdx.x >> 6]);
        __threadfence();
        __syncthreads();
        levels += 1;
        if (s_cnt[cur ^ 1] >= n) {       // nothing coloured: cannot happen (the highest remaining priority is always ready); never spin
            if (threadIdx.x == 0) st->stuck = 1;
            break;
        }
        cur ^= 1;
    }
    if (threadIdx.x == 0) st->tail_levels = levels;
}

// ---- step 5: the caller's colour width and the number of colours ------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_col_out(const int *__restrict__ color, int64_t N, void *__restrict__ out, int cb, ColStats *st)
{
    int m = 0;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += (int64_t)gridDim.x * kBlock) {
        const int c = color[j];
        if (cb == 8) ((int64_t *)out)[j] = c; else ((int32_t *)out)[j] = c;
        m = max(m, c);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&st->max_color, m);
}

// ---- the checker: rows in which two columns of the same non-zero colour meet ------------------------------------------------------
__device__ __forceinline__ bool check_row_wave(const int *__restrict__ rcols, int ta, int tb, const void *__restrict__ colorvec, int cb, unsigned *bm)
{
    const int lane = threadIdx.x & 63;
    long long lo = 1;      // the window [lo, lo + 4096) of colours; the next one starts at the smallest colour beyond it
    for (;;) {
        bm[lane] = 0;
        bm[lane + 64] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        long long nxt = LLONG_MAX;
        bool dup = false;
        for (int t0 = ta; t0 < tb; t0 += 64) {
            const int t = t0 + lane;
            if (t < tb) {
                const long long c = col_load(colorvec, cb, rcols[t]);
                if (c >= lo) {
                    if (c - lo < kColorWaveWin) {
                        const unsigned d = (unsigned)(c - lo), bit = 1u << (d & 31);
                        dup = dup || (atomicOr(&bm[d >> 5], bit) & bit);
                    } else {
                        nxt = c < nxt ? c : nxt;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (__ballot(dup)) return true;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const long long o = __shfl_xor(nxt, off, 64);
            nxt = o < nxt ? o : nxt;
        }
        if (nxt == LLONG_MAX) return false;
        lo = nxt;
    }
}

__global__ void __launch_bounds__(kBlock) k_col_check(const int *__restrict__ rptr, const int *__restrict__ rcols, int64_t M,
                                                      const void *__restrict__ colorvec, int cb, ColStats *st)
{
    __shared__ unsigned s_bm[kBlock / 64][128];
    const int lane = threadIdx.x & 63;
    for (int64_t b0 = (int64_t)blockIdx.x * kBlock; b0 < M; b0 += (int64_t)gridDim.x * kBlock) {
        const int64_t r = b0 + threadIdx.x;
        const int ta = r < M ? rptr[r] : 0, tb = r < M ? rptr[r + 1] : 0;
        const int len = tb - ta;
        bool bad = false;
        if (len >= 2 && len <= kCheckLaneLen) {
            for (int a = ta; a < tb && !bad; ++a) {
                const long long ca = col_load(colorvec, cb, rcols[a]);
                if (ca <= 0) continue;
                for (int b = a + 1; b < tb; ++b) bad = bad || col_load(colorvec, cb, rcols[b]) == ca;
            }
        }
        unsigned long long m = __ballot(len > kCheckLaneLen);
        while (m) {
            const int src = __ffsll(m) - 1;
            m &= m - 1;
            const bool b = check_row_wave(rcols, __shfl(ta, src, 64), __shfl(tb, src, 64), colorvec, cb, s_bm[threadIdx.x >> 6]);
            if (lane == src) bad = b;
        }
        const unsigned long long mb = __ballot(bad);
        if (lane == 0 && mb) atomicAdd(&st->bad_rows, (unsigned long long)__popcll(mb));
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
namespace {

struct ColorWs {        // the call's workspace: allocated inside the call, freed before it returns
    std::vector<void *> ptrs;
    ~ColorWs() { for (void *p : ptrs) (void)hipFree(p); }
    template <class T> bool alloc(T **out, int64_t n)
    {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(T) * (size_t)std::max<int64_t>(n, 1)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        ptrs.push_back(p);
        *out = (T *)p;
        return true;
    }
};

struct ColorPattern {
    int64_t nnz = 0;
    int *cptr = nullptr, *erow = nullptr, *rptr = nullptr, *rcols = nullptr, *work = nullptr, *cursor = nullptr, *bsum = nullptr;
    ColStats *st = nullptr;
};

inline unsigned col_grid(const fd_ctx *ctx, int64_t n, int per_block = kBlock)
{
    const int64_t want = (n + per_block - 1) / per_block;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * 16));
}

int color_args(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base, const void *colors,
               int color_bytes, const void *out)
{
    FD_REQUIRE(ctx && colptr && rowval && colors && out, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(idx_bytes == 4 || idx_bytes == 8, FD_ERR_ARG, "idx_bytes must be 4 or 8");
    FD_REQUIRE(color_bytes == 4 || color_bytes == 8, FD_ERR_ARG, "color_bytes must be 4 or 8");
    FD_REQUIRE(idx_base == 0 || idx_base == 1, FD_ERR_ARG, "idx_base must be 0 or 1");
    FD_REQUIRE(M >= 0 && N >= 1 && M < INT_MAX && N < INT_MAX, FD_ERR_SHAPE, "bad shape %lld x %lld", (long long)M, (long long)N);
    return FD_OK;
}

// step 1 on the context's stream; on FD_OK the stream is idle and the pattern is valid
int color_transpose(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr, const void *rowval, int ib, int base, bool want_work, ColorWs &ws,
                    ColorPattern &P)
{
    FD_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int64_t ends[2] = {0, 0};      // colptr[0], colptr[N]
    for (int k = 0; k < 2; ++k) {
        int64_t v64 = 0;
        int32_t v32 = 0;
        FD_HIP_CHECK(hipMemcpyAsync(ib == 8 ? (void *)&v64 : (void *)&v32, (const char *)colptr + (size_t)ib * (size_t)(k ? N : 0), (size_t)ib,
                                    hipMemcpyDeviceToHost, s));
        FD_HIP_CHECK(hipStreamSynchronize(s));
        ends[k] = (ib == 8 ? v64 : (int64_t)v32) - base;
    }
    const int64_t e0 = ends[0], e1 = ends[1];
    FD_REQUIRE(e0 >= 0 && e1 >= e0 && e1 - e0 < INT_MAX, FD_ERR_SHAPE, "colptr is not monotone (colptr[1] = %lld, colptr[N+1] = %lld)",
               (long long)(e0 + base), (long long)(e1 + base));
    const int64_t nnz = e1 - e0, nb = (M + kScanTile - 1) / kScanTile;
    P.nnz = nnz;
    const bool ok = ws.alloc(&P.st, 1) && ws.alloc(&P.cptr, N + 1) && ws.alloc(&P.erow, nnz) && ws.alloc(&P.rptr, M + 1) &&
                    ws.alloc(&P.rcols, nnz) && ws.alloc(&P.cursor, M) && ws.alloc(&P.bsum, nb + 1) && (!want_work || ws.alloc(&P.work, N));
    FD_REQUIRE(ok, FD_ERR_NOMEM, "hipMalloc of the colouring workspace failed (%lld entries)", (long long)nnz);
    FD_HIP_CHECK(hipMemsetAsync(P.st, 0, sizeof(ColStats), s));
    FD_HIP_CHECK(hipMemsetAsync(P.cursor, 0, sizeof(int) * (size_t)std::max<int64_t>(M, 1), s));
    if (want_work) FD_HIP_CHECK(hipMemsetAsync(P.work, 0, sizeof(int) * (size_t)N, s));
    k_col_colptr<<<col_grid(ctx, N + 1), kBlock, 0, s>>>(colptr, ib, base, N, e0, e1, P.cptr, P.st);
    if (nnz > 0) k_col_count<<<col_grid(ctx, nnz), kBlock, 0, s>>>(rowval, ib, base, e0, nnz, M, P.erow, P.cursor, P.st);
    ColStats h;
    FD_HIP_CHECK(hipMemcpyAsync(&h, P.st, sizeof(h), hipMemcpyDeviceToHost, s));
    FD_HIP_CHECK(hipStreamSynchronize(s));
    FD_REQUIRE(!(h.flags & COL_BAD_COLPTR), FD_ERR_SHAPE, "colptr is not monotone");
    FD_REQUIRE(!(h.flags & COL_BAD_ROW), FD_ERR_SHAPE, "rowval has an entry outside %d..%lld", base, (long long)(M - 1 + base));
    // row_ptr = exclusive scan of the row counts; the counts' array then serves as the fill pass's cursors
    k_col_scan_sums<<<(unsigned)std::max<int64_t>(nb, 1), kBlock, 0, s>>>(P.cursor, M, P.bsum);
    k_col_scan_top<<<1, kBlock, 0, s>>>(P.bsum, nb);
    k_col_scan_apply<<<(unsigned)std::max<int64_t>(nb, 1), kBlock, 0, s>>>(P.cursor, M, P.bsum, nb, P.rptr);
    FD_HIP_CHECK(hipMemsetAsync(P.cursor, 0, sizeof(int) * (size_t)std::max<int64_t>(M, 1), s));
    if (nnz > 0) k_col_fill<<<col_grid(ctx, nnz), kBlock, 0, s>>>(P.cptr, P.erow, N, nnz, P.rptr, P.cursor, P.rcols, P.work);
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

}  // namespace
}  // namespace fdjac

using namespace fdjac;

extern "C" {

int fd_color_columns_device(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr_dev, const void *rowval_dev, int idx_bytes, int idx_base,
                            void *colorvec_dev_out, int color_bytes, int64_t *ncolors_out)
{
    int rc = color_args(ctx, M, N, colptr_dev, rowval_dev, idx_bytes, idx_base, colorvec_dev_out, color_bytes, colorvec_dev_out);
    if (rc) return rc;
    // test switches (tests/test_gpu_color.py: the colours do not depend on the schedule)
    const char *sw_batch = test_switch("FDJAC_COLOR_BATCH"), *sw_tail = test_switch("FDJAC_COLOR_TAIL"), *sw_stats = test_switch("FDJAC_COLOR_STATS");
    const int batch = sw_batch && atoi(sw_batch) >= 1 ? std::min(atoi(sw_batch), kColorBatch) : kColorBatch;
    const bool use_tail = !(sw_tail && atoi(sw_tail) == 0);
    ColorWs ws;
    ColorPattern P;
    rc = color_transpose(ctx, M, N, colptr_dev, rowval_dev, idx_bytes, idx_base, true, ws, P);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    int *color = nullptr, *list[2] = {nullptr, nullptr}, *cnt = nullptr;
    FD_REQUIRE(ws.alloc(&color, N) && ws.alloc(&list[0], N) && ws.alloc(&list[1], N) && ws.alloc(&cnt, kColorBatch + 1), FD_ERR_NOMEM,
               "hipMalloc of the colouring workspace failed (%lld columns)", (long long)N);
    k_col_init<<<col_grid(ctx, N), kBlock, 0, s>>>(P.cptr, N, color, list[0], P.st);
    ColStats h;
    FD_HIP_CHECK(hipMemcpyAsync(&h, P.st, sizeof(h), hipMemcpyDeviceToHost, s));
    FD_HIP_CHECK(hipStreamSynchronize(s));
    const ColGraph g = {P.cptr, P.erow, P.rptr, P.rcols, P.work, color};
    int64_t n = h.nwork, rounds = 0, launches = 0, checks = 0;
    int in = 0;
    FD_HIP_CHECK(hipMemcpyAsync(cnt, &P.st->nwork, sizeof(int), hipMemcpyDeviceToDevice, s));
    while (n > 0) {
        if (use_tail && n <= kColorTail) {
            k_col_tail<<<1, kColorTailBlock, 0, s>>>(g, list[in], (int)n, P.st);
            launches += 1;
            FD_HIP_CHECK(hipMemcpyAsync(&h, P.st, sizeof(h), hipMemcpyDeviceToHost, s));
            FD_HIP_CHECK(hipStreamSynchronize(s));
            FD_REQUIRE(!h.stuck, FD_ERR_HIP, "device colouring made no progress in the tail (level %d, %lld columns left)", h.tail_levels, (long long)n);
            break;
        }
        // `batch` rounds, each on the list the one before left; blocks beyond a list's length exit at once
        FD_HIP_CHECK(hipMemsetAsync(cnt + 1, 0, sizeof(int) * (size_t)batch, s));
        const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
        for (int k = 0; k < batch; ++k) {
            k_col_round<<<grid, kBlock, 0, s>>>(g, list[in], list[in ^ 1], cnt + k);
            in ^= 1;
        }
        launches += batch;
        int hc[kColorBatch + 1];
        FD_HIP_CHECK(hipMemcpyAsync(hc, cnt, sizeof(int) * (size_t)(batch + 1), hipMemcpyDeviceToHost, s));
        FD_HIP_CHECK(hipStreamSynchronize(s));
        checks += 1;
        for (int k = 0; k < batch && hc[k] > 0; ++k) {
            rounds += 1;
            FD_REQUIRE(hc[k + 1] < hc[k], FD_ERR_HIP, "device colouring made no progress in round %lld (%d columns left)", (long long)rounds, hc[k]);
        }
        n = hc[batch];
        if (n > 0) FD_HIP_CHECK(hipMemcpyAsync(cnt, cnt + batch, sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    k_col_out<<<col_grid(ctx, N), kBlock, 0, s>>>(color, N, colorvec_dev_out, color_bytes, P.st);
    launches += 1;
    FD_HIP_CHECK(hipMemcpyAsync(&h, P.st, sizeof(h), hipMemcpyDeviceToHost, s));
    FD_HIP_CHECK(hipStreamSynchronize(s));
    FD_HIP_CHECK(hipGetLastError());
    if (ncolors_out) *ncolors_out = h.max_color;
    if (sw_stats && atoi(sw_stats) != 0)
        fprintf(stderr, "fd_color_columns_device: N=%lld nnz=%lld colors=%d rounds=%lld tail_levels=%d round_launches=%lld read_backs=%lld\n",
                (long long)N, (long long)P.nnz, h.max_color, (long long)rounds, h.tail_levels, (long long)launches, (long long)checks);
    return FD_OK;
}

int fd_color_check_device(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr_dev, const void *rowval_dev, int idx_bytes, int idx_base,
                          const void *colorvec_dev, int color_bytes, int64_t *bad_rows_out)
{
    int rc = color_args(ctx, M, N, colptr_dev, rowval_dev, idx_bytes, idx_base, colorvec_dev, color_bytes, bad_rows_out);
    if (rc) return rc;
    ColorWs ws;
    ColorPattern P;
    rc = color_transpose(ctx, M, N, colptr_dev, rowval_dev, idx_bytes, idx_base, false, ws, P);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (M > 0) k_col_check<<<col_grid(ctx, M), kBlock, 0, s>>>(P.rptr, P.rcols, M, colorvec_dev, color_bytes, P.st);
    ColStats h;
    FD_HIP_CHECK(hipMemcpyAsync(&h, P.st, sizeof(h), hipMemcpyDeviceToHost, s));
    FD_HIP_CHECK(hipStreamSynchronize(s));
    FD_HIP_CHECK(hipGetLastError());
    *bad_rows_out = (int64_t)h.bad_rows;
    return FD_OK;
}

}  // extern "C"
