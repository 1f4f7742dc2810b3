"""The complex step of the BLOCK-COUPLED residual (FD_F_BLOCKCOUPLED; csrc/fdjac_builtin_f.hip: k_f_block_sigma, k_f_block_apply;
csrc/fdjac_f_blockcoupled.hip: k_f_blockcoupled_lazy, k_f_blockcoupled_store) against a high-precision value, entry by entry.
Pure numpy + mpmath; test infrastructure only.  tests/test_exact_complex_cpu.py holds the C oracle to the bound, tests/test_gpu_exact_complex.py the storing
launch and the hand-over path.

The residual.  nb blocks of bs coordinates; w_j = (j + 1) / bs for the j-th coordinate of a block; sig_b = sum_j w_j x_{b, j};
S_b = (sig_{b-1} + sig_b) + sig_{b+1} (0 outside); f_k = x_k S_{b(k)} + sin x_k.  Its Jacobian, for columns j in the blocks b(k) - 1 ..
b(k) + 1:  J_kj = x_k w_j + delta_kj (S_k + cos x_k).  `reference` evaluates that with mpmath at 200 bits on the element-type values of
x and returns it as a double-double (hi, lo), so that |got - J_kj| is known far below one ulp of either element type.  The complex
step's own truncation, cos x_k (sinh(eps) / eps - 1) = cos x_k eps^2 / 6 + ..., is not rounding error; `bound` adds eps^2 |cos x_k|
for it (2e-32, or 1e-14 in Float32, of the entry: nothing next to the rounding terms).

The allowed error of an entry.  u = eps(T) / 2 is the unit roundoff, g(n) = n u / (1 - n u) bounds the relative error of a quantity
that went through n roundings.  With a valid colouring, colour c's point perturbs ONE coordinate j of every three neighbouring
blocks, so the imaginary part of f_k is
    im_k = (x_k si + xi_k sr) + cos(x_k) sinh(xi_k),     si = im S = w_j eps,  sr = re S,  xi_k = eps if k == j else +0,
and the stored value is im_k / eps.  The path of every term, one rounding each:
    x_k w_j          the division (j + 1) / bs, the product w_j (x_j, eps), six levels of the wavefront's summation tree, the two block
                     additions of S, the product x_k si, the two additions that assemble im_k, the quotient by eps: 14 roundings.
                     (With one perturbed coordinate per three blocks the tree and block additions of the IMAGINARY parts add zeros
                     and w_j eps, im_k / eps scale by a power of two: those are exact.  They are counted all the same, so that the
                     bound does not lean on the colouring's zeros; the entry's own product and the division of w_j always round.)
    S_k              (the diagonal only) every term w_i x_i of the three blocks' sums: division, product, six tree levels, two block
                     additions, the product xi_k sr, the two additions, the quotient: 14 roundings, relative to the sum of the
                     MAGNITUDES sum_i |w_i x_i| of the terms the entry adds -- cancellation in S_k does not shrink the error.
    cos x_k          (the diagonal only) cos and sinh from the math library, their product, the last addition, the quotient.  The
                     libraries state their errors in ulps; the figures published for the HIP device library and for glibc (the
                     oracle's) lie between 1 and 3 ulp for cos and sinh in either element type (quoted from their accuracy tables,
                     which are not part of this repository).  The bound allows L = 4 ulp = 8 u for each of the two -- above those
                     figures -- so 3 + 16 = 19 roundings' worth.
    bound_kj = g(14) |x_k| w_j + delta_kj (g(14) sum_i |w_i x_i| + (g(19) + eps^2) |cos x_k|)
The C oracle sums sig_b sequentially (bs - 1 additions, not six levels), so for bs = 64 its worst case is not covered by g(14); it is
held to the same bound all the same, and its worst ratio is recorded (tests/test_exact_complex_cpu.py)."""
import functools

import numpy as np

from finitediff_jl_amd import patterns as P

SHAPES = [(1, 2), (3, 32), (5, 32), (9, 64), (7, 3), (70, 2)]
LIB_ULPS = 4          # allowed error of cos and of sinh, in ulps
N_PATH = 14           # roundings on the path of a product term (see above)
N_TRANS = 3 + 4 * LIB_ULPS


def layout(nb, bs):
    return P.BlockBandedLayout(np.full(nb, bs), 1, 1)


def operands(nb, bs, dtype):
    """Ordinary operands in the element type."""
    return (np.random.default_rng(77 + 1000 * nb + bs).random(nb * bs) - 0.3).astype(dtype)


def band_mask(nb, bs):
    b = np.arange(nb * bs) // bs
    return np.abs(b[:, None] - b[None, :]) <= 1


@functools.lru_cache(maxsize=None)
def _reference(nb, bs, dtype_name):
    import mpmath as mp
    dtype = np.dtype(dtype_name)
    x = operands(nb, bs, dtype)
    N = nb * bs
    with mp.workprec(200):
        xm = [mp.mpf(float(v)) for v in x]
        w = [mp.mpf(j + 1) / bs for j in range(bs)]
        sig = [mp.fsum(w[j] * xm[b * bs + j] for j in range(bs)) for b in range(nb)]
        S = [(sig[b - 1] if b > 0 else 0) + sig[b] + (sig[b + 1] if b + 1 < nb else 0) for b in range(nb)]
        hi = np.zeros((N, N))
        lo = np.zeros((N, N))
        for k in range(N):
            bk = k // bs
            for j in range(max(0, bk - 1) * bs, min(nb, bk + 2) * bs):
                v = xm[k] * w[j % bs]
                if j == k:
                    v = v + S[bk] + mp.cos(xm[k])
                h = float(v)
                hi[k, j] = h
                lo[k, j] = float(v - h)
    return hi, lo


def reference(nb, bs, dtype):
    """(hi, lo): the N x N Jacobian as a double-double, 0 outside the block band."""
    return _reference(nb, bs, np.dtype(dtype).name)


def bound(nb, bs, dtype):
    """The allowed absolute error of every entry (N x N, float64; 0 outside the block band)."""
    x = operands(nb, bs, dtype).astype(np.float64)
    e = float(np.finfo(dtype).eps)
    u = e / 2
    g = lambda n: n * u / (1 - n * u)
    w = (np.arange(bs) + 1.0) / bs
    wj = np.tile(w, nb)
    mag = np.abs(x.reshape(nb, bs) * w).sum(axis=1)                  # sum_j |w_j x_j| per block
    pad = np.concatenate([[0.0], mag, [0.0]])
    magS = np.repeat(pad[:-2] + pad[1:-1] + pad[2:], bs)             # ... of the three blocks of S_k
    B = g(N_PATH) * np.abs(x)[:, None] * wj[None, :]
    B[np.diag_indices(nb * bs)] += g(N_PATH) * magS + (g(N_TRANS) + e * e) * np.abs(np.cos(x))
    return B * band_mask(nb, bs)


def error(got_dense, nb, bs, dtype):
    """|got - reference| per entry (float64), exact to far below an ulp: got - hi is exact where the two are close."""
    hi, lo = reference(nb, bs, dtype)
    return np.abs((np.asarray(got_dense, np.float64) - hi) - lo)


def worst_ratio(got_dense, nb, bs, dtype):
    """max over the block band of error / bound, and where."""
    m = band_mask(nb, bs)
    got_dense = np.asarray(got_dense)
    assert np.isfinite(got_dense[m]).all()
    assert (got_dense[~m] == 0).all()
    r = np.zeros(m.shape)
    r[m] = error(got_dense, nb, bs, dtype)[m] / bound(nb, bs, dtype)[m]
    at = np.unravel_index(np.argmax(r), r.shape)
    return float(r[at]), (int(at[0]), int(at[1]))
