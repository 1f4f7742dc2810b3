// K3r  the hand-over decompression ROW BY ROW (FD_PLAN_HANDOVER_ROWS, opt-in; FD_INFO_HANDOVER_ROWS): the same quotients as
//   k_decompress_list (fdjac_kernels.hip) -- `_colorediteration!`, ext/FiniteDiffSparseArraysExt.jl:38-47, for all colours of the
//   chunk at once -- walked through the plan's row lists (FD_PLAN_STORE_CSC_ROWS, fdjac_store_csc.hip) instead of in storage order.
//
//   thread = row, in the plan's lane order (tile of 256 rows by tile, a tile's rows by descending length): ONE 8-byte row_pack load
//   gives the row, its place in the tile's run of the lists and its length; the run's base comes from row_tile.  A wavefront then
//   gathers fx1[c][r] (and fx[r], once per thread) for 64 rows of ONE tile of 256 consecutive rows: at most C x 4 (Float32: x 2) 512-B
//   runs, hit again by the rows' next entries -- the entry-ordered gathers take one sector per entry in one of C arrays.  What it pays:
//   row_slot and the entry's colour are read with a stride of the row's length across the lanes, and the stores are scattered 8-byte
//   (Float32: 4-byte) stores, one slot each.
//   Rows whose row_pack fields are saturated (a run offset of 65535, a length of 32767) and rows longer than kRowsThreadMax entries are
//   served from row_ptr by the WAVEFRONT the thread sits in, lanes over entries, after the thread-per-row pass (a 3000-entry row costs
//   its wavefront 47 trips instead of holding 63 idle lanes for 3000).
//   Semantics of an entry with colour c, as k_decompress_list: c coloured and in [c_lo, c_hi) -> the quotient (IEEE division, the same
//   operand order); c "none" and c_lo == 0 -> 0; anything else -> the slot is left untouched.  Every slot is written by one thread.
//   MODE 0 / 1 / 2: forward / central / complex step (entry_value's expressions); LDS_EPS: the chunk's eps[] slice staged in LDS.
// Compiled in both element-type builds (fdjac_f32.hip includes it).
#include "fdjac_internal.h"

namespace fdjac {

constexpr int kRowsThreadMax = 64;   // a row longer than this is a wavefront's (one pass of 64 lanes covers what 64 trips of a thread would)
constexpr int kRowsUnroll = 4;       // entries of a row in flight per trip

template <typename CT> struct RowsColor;      // (the list kernel's conventions: "none" all ones, "pad" one below)
template <> struct RowsColor<uint8_t> { static constexpr int none = 0xFF; static constexpr int pad = 0xFE; };
template <> struct RowsColor<int32_t> { static constexpr int none = -1; static constexpr int pad = -2; };

template <typename CT, int MODE, bool LDS_EPS>
__global__ void __launch_bounds__(kBlock)
k_decompress_rows(const int32_t *__restrict__ row_pack, const int32_t *__restrict__ row_tile, const int32_t *__restrict__ row_ptr,
                  const int32_t *__restrict__ row_slot, const CT *__restrict__ row_color, const real_t *__restrict__ FXa,
                  const real_t *__restrict__ FXb, int64_t ld, const real_t *__restrict__ eps, int c_lo, int c_hi,
                  real_t *__restrict__ out, int64_t M)
{
    extern __shared__ real_t s_row_eps[];
    const int nB = c_hi - c_lo;
    if (LDS_EPS) {
        for (int c = threadIdx.x; c < nB; c += kBlock) s_row_eps[c] = eps[c_lo + c];
        __syncthreads();
    }
    constexpr int none = RowsColor<CT>::none, pad = RowsColor<CT>::pad;
    const int64_t ntiles = (M + kBlock - 1) / kBlock;
    const int64_t tile = xcd_tile(blockIdx.x, ntiles);      // XCD x walks its own contiguous range of row tiles
    if (tile >= ntiles) return;
    const int64_t pos = tile * kBlock + threadIdx.x;
    const bool in = pos < M;
    const int2 pk = *reinterpret_cast<const int2 *>(row_pack + 2 * (in ? pos : tile * kBlock));
    const int A0 = row_tile[tile];
    const int r = pk.x;
    const int b0 = pk.y & 0xFFFF, len = in ? (int)((unsigned)pk.y >> 16) : 0;
    const bool wide = in && (b0 == 65535 || len == 32767 || len > kRowsThreadMax);
    const int L = wide ? 0 : len;

    // one entry: list position q of row rr (subtrahend fxr, forward differences only)
    auto value = [&](int c, int rr, real_t fxr, bool &valid) -> real_t {
        const int cb = c - c_lo;
        valid = (c != none) & (c != pad) & ((unsigned)cb < (unsigned)nB);
        const int cs = valid ? cb : 0;
        const int64_t at = (int64_t)cs * ld + rr;
        const real_t e = LDS_EPS ? s_row_eps[cs] : eps[c_lo + cs];
        real_t q;
        if (MODE == 0) q = (FXa[at] - fxr) / e;
        else if (MODE == 1) q = (FXa[at] - FXb[at]) / (2 * e);
        else q = FXa[at * 2 + 1] / e;
        return valid ? q : (real_t)0.0;
    };

    if (L > 0) {
        const real_t fxr = MODE == 0 ? FXb[r] : (real_t)0.0;
        const int base = A0 + b0;
        for (int k0 = 0; k0 < L; k0 += kRowsUnroll) {
            int slot[kRowsUnroll], c[kRowsUnroll];
#pragma unroll
            for (int u = 0; u < kRowsUnroll; ++u) {          // (a trip past the row's end re-reads its last entry and stores nothing)
                const int q = base + (k0 + u < L ? k0 + u : L - 1);
                slot[u] = row_slot[q];
                c[u] = (int)row_color[q];
            }
            real_t v[kRowsUnroll];
            bool valid[kRowsUnroll];
#pragma unroll
            for (int u = 0; u < kRowsUnroll; ++u) v[u] = value(c[u], r, fxr, valid[u]);
#pragma unroll
            for (int u = 0; u < kRowsUnroll; ++u)
                if (k0 + u < L && (valid[u] | ((c[u] == none) & (c_lo == 0)))) out[slot[u]] = v[u];
        }
    }
    // the wavefront's wide rows, one after the other, lanes over entries (the mask is wave-uniform: no lane has left)
    unsigned long long m = __builtin_amdgcn_ballot_w64(wide);
    const int lane = (int)(threadIdx.x & 63);
    while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const int rr = __shfl(r, src, 64);
        const int q0 = row_ptr[rr], q1 = row_ptr[rr + 1];
        const real_t fxr = MODE == 0 ? FXb[rr] : (real_t)0.0;
        for (int q = q0 + lane; q < q1; q += 64) {
            const int c = (int)row_color[q];
            bool valid;
            const real_t v = value(c, rr, fxr, valid);
            if (valid | ((c == none) & (c_lo == 0))) out[row_slot[q]] = v;
        }
    }
}

int launch_decompress_rows(fd_plan *p, const real_t *FXa, const real_t *FXb, int c_lo, int c_hi, real_t *out, int mode)
{
    const int B = c_hi - c_lo;
    const int64_t ntiles = (p->M + kBlock - 1) / kBlock;
    if (ntiles <= 0) return FD_OK;
    const bool lds = B <= kEpsLdsMax;
    const size_t shm = lds ? sizeof(real_t) * (size_t)B : 0;
    const dim3 grid((unsigned)(8 * xcd_chunks(ntiles)));
    // <CT, MODE, LL>: the plan's colour width, the difference type, eps staged in LDS
    fd_pick<false, true>(p->color8, [&](auto C8) {
        using CT = std::conditional_t<C8(), uint8_t, int32_t>;
        fd_pick<0, 1, 2>(mode, [&](auto MD) {
            fd_pick<false, true>(lds, [&](auto LL) {
                hipLaunchKernelGGL((k_decompress_rows<CT, MD(), LL()>), grid, dim3(kBlock), shm, p->ctx->stream, p->d_sr_order, p->d_sr_tile,
                                   p->d_sr_ptr, p->d_sr_slot, (const CT *)p->d_sr_color, FXa, FXb, p->ldf, p->d_eps, c_lo, c_hi, out, p->M);
            });
        });
    });
    FD_HIP_CHECK(hipGetLastError());
    return FD_OK;
}

}  // namespace fdjac
