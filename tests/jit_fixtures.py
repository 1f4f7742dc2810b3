"""The source text of the runtime-compiled row functors that more than one GPU test module uses (fd.JitF, csrc/fdjac_jit.hip), each with
a numpy restatement in tests/exact_model.py in the functor's own operation order (band_f / band_fc, grid_f, blockrat_f / blockrat_fc).
Pure strings: importing this module needs neither the library nor a GPU.  Test infrastructure only."""
import struct

_BAND = """
// a residual whose Jacobian is the exact band (l, u): row i = sum over c = i - l .. i + u of w(i, c) (x_c + x_c^2 / 4)%(doc)s, left to right;
// generic in the point's value type (real_t for forward / central differences, fd_cplx<real_t> for the complex step)
struct %(name)s {
    long long n;
    int l, u;
    template <class P> __device__ typename P::value_type operator()(long long i, const P &X) const
    {
        typedef typename P::value_type V;
        V s = V();
        bool first = true;
        for (long long c = i - l; c <= i + u; ++c) {
            const bool in = c >= 0 && c < n;
            const V v = X(in ? c : i);
            const V t = ((real_t)1 + (real_t)0.125 * (real_t)(int)((i + 3 * c) & 7)) * (v + ((real_t)0.25 * v) * v)%(extra)s;
            if (in) { s = first ? t : s + t; first = false; }
        }
        return s;
    }
};
"""
BANDF = _BAND % dict(name="BandF", doc="", extra="")
# ... + copysign(1, x_c): the term sees the sign of a zero coordinate (forward / central differences only)
BAND_SIGN = _BAND % dict(name="BandSign", doc=" + copysign(1, x_c)", extra=" + (real_t)__builtin_copysign(1.0, (double)v)")


def band_params(N, l, u):
    return struct.pack("qii", N, l, u)


GRID_NL = """
// an nx x ny grid, row k = (i, j): neighbours within `reach` along the grid row and the points straight above / below, nonlinear in x_k
struct GridNL {
    long long nx, ny, reach;
    template <class P> __device__ typename P::value_type operator()(long long k, const P &X) const
    {
        typedef typename P::value_type V;
        const long long j = k / nx, i = k - j * nx;
        const V c = X(k);
        V s = c * c;
        for (long long d = 1; d <= reach; ++d) {
            const bool hw = i - d >= 0, he = i + d < nx;
            const V w = X(hw ? k - d : k), e = X(he ? k + d : k);
            s = s + (hw ? (real_t)(0.5 / d) * w : (real_t)0);
            s = s + (he ? (real_t)(0.25 * d) * e * c : (real_t)0);
        }
        const bool hs = j > 0, hn = j + 1 < ny;
        const V sv = X(hs ? k - nx : k), nv = X(hn ? k + nx : k);
        s = s + (hs ? sv : (real_t)0);
        s = s + (hn ? (real_t)2 * nv : (real_t)0);
        return s;
    }
};
"""


def grid_params(nx, ny, reach):
    return struct.pack("qqq", nx, ny, reach)


_BLOCK = """
// a RATIONAL block-coupled row (any block sizes): row k of block b = x_k (S_{b-bl} + ... + S_{b+bu}) + (x_k x_k) x_k, S_J = block J's
// coordinates%(doc)s added left to right, the sums added left to right (blocks outside the matrix: none); off = nb + 1 block offsets and
// blk = the block of every row, both in device memory
struct %(name)s {
    long long nb;
    const long long *off;
    const int *blk;
    int bl, bu;
    template <class P> __device__ typename P::value_type operator()(long long k, const P &X) const
    {
        typedef typename P::value_type V;
        const long long b = blk[k];
        V tot = V();
        bool first = true;
        for (long long bb = b - bl; bb <= b + bu; ++bb) {
            if (bb < 0 || bb >= nb) continue;
            V s = V();
            for (long long i = off[bb]; i < off[bb + 1]; ++i) { const V v = X(i)%(extra)s; s = i == off[bb] ? v : s + v; }
            tot = first ? s : tot + s;
            first = false;
        }
        const V xk = X(k);
        return xk * tot + (xk * xk) * xk;
    }
};
"""
BLOCK_RAT = _BLOCK % dict(name="BlockRat", doc="", extra="")
# S_J adds v + copysign(1, v): sees the sign of a zero coordinate (forward / central differences only)
BLOCK_SIGN = _BLOCK % dict(name="BlockSign", doc=" (each plus copysign(1, itself))", extra=" + (real_t)__builtin_copysign(1.0, (double)X(i))")


RAGGED_GRID = """
// GridNL with reach 2 on grid rows of DIFFERENT lengths (the blocks of a non-uniform BandedBlockBandedMatrix; the parameter block of
// BlockRat, bl and bu unused): row k of block K, local index i couples to i +- 1, i +- 2 inside the block and to local index i of the
// blocks K - 1 and K + 1 where they are long enough
struct RaggedGrid {
    long long nb;
    const long long *off;
    const int *blk;
    int bl, bu;
    template <class P> __device__ typename P::value_type operator()(long long k, const P &X) const
    {
        typedef typename P::value_type V;
        const long long K = blk[k], o = off[K], i = k - o, n = off[K + 1] - o;
        const V c = X(k);
        V s = c * c;
        for (long long d = 1; d <= 2; ++d) {
            const bool hw = i - d >= 0, he = i + d < n;
            const V w = X(hw ? k - d : k), e = X(he ? k + d : k);
            s = s + (hw ? (real_t)(0.5 / d) * w : (real_t)0);
            s = s + (he ? (real_t)(0.25 * d) * e * c : (real_t)0);
        }
        const bool hs = K > 0 && i < o - off[K > 0 ? K - 1 : 0], hn = K + 1 < nb && i < off[K + 1 < nb ? K + 2 : K + 1] - off[K + 1];
        const V sv = X(hs ? off[K - 1] + i : k), nv = X(hn ? off[K + 1] + i : k);
        s = s + (hs ? sv : (real_t)0);
        s = s + (hn ? (real_t)2 * nv : (real_t)0);
        return s;
    }
};
"""


def block_params(nb, off_ptr, blk_ptr, bl, bu):
    return struct.pack("qPPii", nb, off_ptr, blk_ptr, bl, bu)
