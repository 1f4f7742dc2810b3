"""Inputs, references and a fault-injecting host model for the three consumers of the Jacobian path: the tridiagonal partition solver
(csrc/fdjac_solve.hip), the banded block cyclic reduction (csrc/fdjac_bandsolve.hip) and the block-tridiagonal one
(csrc/fdjac_blocksolve.hip).  numpy and SciPy only; nothing here runs on the GPU.

Every generator returns a `System`: alpha, beta, the J storage a solver takes (in the solver's element type), the right-hand side, and
`A`, the matrix alpha I + beta J AS THE DEVICE SEES IT (Float64 arithmetic on the stored values; beta is always +-2^k, so beta * J is
exact and a fused and an unfused alpha + beta * J agree), as diagonals {offset: values indexed by row}.

Family E ("exact"): every row of A has diagonal D_i = +-1 and at most one off-diagonal entry O_i = +-1 at a column p(i) on ONE side of
the diagonal inside the solver's band: a signed unit-triangular forest, y_i = D_i (b_i - O_i y_p(i)).  With an integer right-hand side in
{-1, 0, 1} every quantity any pivot-free elimination order forms (a Schur complement of I - N, N nilpotent, is again of that form: all
principal minors are +-1) is an integer of magnitude <= N, exact in Float64: the device's y must EQUAL `System.y`, computed in int64.

Family S ("slow"): two-sided M-matrices whose Green's function decays over `lam` rows (block rows), scaled by random signs and random
powers of two per row: the coupling of unknowns 8^L (2^L) apart that level L of the elimination forms is O(1).  The reference is SciPy's
Float64 LU refined with residuals in extended precision (`refined_reference`).

Host models (`TriModel`, `tri_sharded_model`, `BcrModel`): the recursive partition (radix 8, a chunk's last unknown survives, identity
rows pad the last chunk) and radix-2 block cyclic reduction (odd block rows survive), restated from the header comments of the three
.hip files.  `fault=(L, mode)` zeroes ("zero") or negates ("flip") the coupling terms (a, c / A', C') of the level-L system, i.e. the ones
the reduction of level L - 1 forms; `tip_fault=(rank, mode)` does it to one rank's spike tips in the sharded solve.  They exist to prove
that the inputs discriminate (tests/test_solve_model_cpu.py)."""
import copy
from collections import namedtuple

import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

System = namedtuple("System", "kind N alpha beta J b A y meta")
#   kind "tri": J = (dl, d, du); "band": J = data (l+u+1, N), data[u + i - j, j] = J[i, j]; "block": J = BlockBandedMatrix data
#   A: {offset k: a_k}, a_k[i] = A[i, i + k] (0 where i + k is outside);  y: int64 exact solution (family E) or None

E_SHIFTS = [(0.0, 1.0), (2.0, -1.0), (-1.0, 2.0), (0.0, -1.0)]      # (2,-1): J's diagonal is 1; (-1,2): it is 0; beta < 0 flips signs
KCHUNK, KTOP = 8, 512                  # fdjac_solve.hip: rows per thread, rows the top level takes
BCR_TOP_ROWS = 1024                    # fdjac_bandsolve.hip: kBcrTopRows


# ------------------------------------------------------------------------------------------------------------ family E
def forest_solution(D, O, p, b):
    """y_i = D_i (b_i - O_i y_p(i)) in int64 by pointer doubling (O_i = 0 marks a root)."""
    D = np.asarray(D, np.int64); m = -(D * np.asarray(O, np.int64)); c = D * np.asarray(b, np.int64)
    p = np.where(m != 0, np.asarray(p, np.int64), np.arange(D.size))
    while np.any(m != 0):
        c = c + m * c[p]
        m = m * m[p]
        p = p[p]
    return c


def chain_solution(D, O, b, lower=True):
    """The same for p(i) = i - 1 (lower) / i + 1 everywhere: a segmented signed prefix sum, O(N)."""
    D = np.asarray(D, np.int64); O = np.asarray(O, np.int64); b = np.asarray(b, np.int64)
    if not lower:
        return chain_solution(D[::-1], O[::-1], b[::-1])[::-1]
    m, c = -(D * O), D * b                                    # y_i = c_i + m_i y_{i-1}
    n = D.size
    start = np.flatnonzero(m == 0)                            # m_0 = 0 by construction
    seg = np.cumsum(m == 0) - 1
    neg = np.cumsum(m < 0)
    P = 1 - 2 * ((neg - neg[start][seg]) & 1)                 # product of the m's since the segment's start (+-1)
    t = np.cumsum(c * P)
    base = np.where(start > 0, t[start - 1], 0) if n else t
    return P * (t - base[seg])


def _rng(seed):
    return np.random.default_rng(seed)


def _diag_for(shift, rng, N):
    alpha, beta = shift
    if alpha == 0.0:
        return rng.choice([-1.0, 1.0], N)
    return np.full(N, alpha + beta * (1.0 if beta == -1.0 else 0.0))      # the shifts that reach the diagonal: J_ii = 1 / 0


def _cast(x, dtype):
    return np.ascontiguousarray(np.asarray(x, np.float64).astype(dtype))


def _seen(alpha, beta, Jv):
    """alpha + beta * J in the device's Float64 arithmetic (beta = +-2^k: the product is exact)."""
    m, _e = np.frexp(abs(beta))
    assert m == 0.5, "beta must be a power of two"
    return alpha + beta * np.asarray(Jv, np.float64)


def _segments(N, rng, kind):
    """direction (+1: p = i - 1, -1: p = i + 1) per row and the mask of rows that have a coupling."""
    if kind == "lower":
        dirn = np.ones(N, np.int64); has = np.ones(N, bool)
    elif kind == "upper":
        dirn = -np.ones(N, np.int64); has = np.ones(N, bool)
    else:
        lens = []
        tot = 0
        while tot < N:
            L = int(np.exp(rng.uniform(0.0, np.log(1e5)))) if rng.random() < 0.8 else int(rng.integers(1, 20))
            lens.append(max(L, 1)); tot += lens[-1]
        ends = np.minimum(np.cumsum(lens), N)
        sid = np.searchsorted(ends, np.arange(N), side="right")
        dirn = np.where((sid + int(rng.integers(0, 2))) % 2 == 0, 1, -1).astype(np.int64)
        has = np.ones(N, bool)
        starts = np.concatenate([[0], ends[:-1]])
        first, last = starts[sid], ends[sid] - 1
        i = np.arange(N)
        has &= ~((dirn == 1) & (i == first)) & ~((dirn == -1) & (i == last))     # no coupling out of a segment: no 2-cycle
    i = np.arange(N)
    has &= ~((dirn == 1) & (i == 0)) & ~((dirn == -1) & (i == N - 1))
    return dirn, has


def e_tridiag(N, seed, kind="segmented", shift=(0.0, 1.0), dtype=np.float64):
    rng = _rng(seed)
    alpha, beta = shift
    D = _diag_for(shift, rng, N)
    dirn, has = _segments(N, rng, kind)
    O = np.where(has, rng.choice([-1.0, 1.0], N), 0.0)
    b = rng.integers(-1, 2, N).astype(np.float64)
    lo = np.where(dirn == 1, O, 0.0); up = np.where(dirn == -1, O, 0.0)
    J = (_cast(lo[1:] / beta, dtype), _cast((D - alpha) / beta, dtype), _cast(up[:-1] / beta, dtype))
    A = {-1: np.concatenate([[0.0], beta * J[0].astype(np.float64)]), 0: _seen(alpha, beta, J[1]),
         1: np.concatenate([beta * J[2].astype(np.float64), [0.0]])}
    assert np.array_equal(A[0], D) and np.array_equal(A[-1], lo) and np.array_equal(A[1], up)
    if kind == "segmented":
        yl = chain_solution(D, lo, b, True); yu = chain_solution(D, up, b, False)
        # a row belongs to a lower or an upper segment; roots appear in both and agree
        y = np.where(dirn == 1, yl, yu)
    else:
        y = chain_solution(D, O, b, kind == "lower")
    return System("tri", N, alpha, beta, J, _cast(b, dtype), A, y, dict(dirn=dirn, kind=kind))


def e_tridiag_crossing(N, cuts, seed, dtype=np.float64):
    """A segmented family-E system in which a chain crosses every rank cut (the first seed from `seed` on for which it does)."""
    for k in range(1000):
        s = e_tridiag(N, seed + 7919 * k, "segmented", E_SHIFTS[(seed + k) % 4], dtype)
        if all(s.A[-1][c] != 0 or s.A[1][c - 1] != 0 for c in cuts[1:-1]) and \
                all(r in through_ranks(s, cuts) for r in range(1, len(cuts) - 2) if cuts[r + 1] - cuts[r] <= KCHUNK):
            return s
    raise AssertionError("no seed gives a chain across every cut")


def through_ranks(s, cuts):
    """Ranks a family-E chain runs THROUGH (in at one cut, out at the other): the only ranks whose spike tips a forest uses -- a
    chain crosses a cut in one direction, the receiving rank's interface values depend on its tips, and only the NEXT rank reads them."""
    out = []
    for r in range(1, len(cuts) - 2):
        c0, c1 = cuts[r], cuts[r + 1]
        if np.all(s.A[-1][c0:c1 + 1] != 0) or np.all(s.A[1][c0 - 1:c1] != 0):
            out.append(r)
    return out


def sharded_lam(cuts):
    return float(max(8, 2 * int(np.max(np.diff(cuts)))))


def _forest_system(N, D, O, p):
    A = {0: D.copy()}
    k = np.where(O != 0, p - np.arange(N), 0)
    for off in np.unique(k[O != 0]):
        A[int(off)] = np.where((k == off) & (O != 0), O, 0.0)
    return A


def e_banded(N, l, u, seed, lower=True, shift=(0.0, 1.0), dtype=np.float64):
    """p(i) = i - k_i, k_i in 1..l (lower) or i + k_i, k_i in 1..u."""
    rng = _rng(seed)
    alpha, beta = shift
    w = l if lower else u
    assert w >= 1
    D = _diag_for(shift, rng, N)
    i = np.arange(N)
    k = rng.integers(1, w + 1, N)
    p = i - k if lower else i + k
    has = (p >= 0) & (p < N)              # (roots only at the ends: a chain broken at random would cut the upper levels' couplings)
    O = np.where(has, rng.choice([-1.0, 1.0], N), 0.0)
    p = np.where(has, p, i)
    b = rng.integers(-1, 2, N).astype(np.float64)
    A = _forest_system(N, D, O, p)
    data = np.zeros((l + u + 1, N))
    for off, v in A.items():                                     # A[i, i + off] -> data[u - off, i + off]
        rows = np.flatnonzero(v != 0) if off else i
        data[u - off, rows + off] = (v[rows] - (alpha if off == 0 else 0.0)) / beta
    data = _cast(data, dtype)
    assert np.array_equal(_seen(alpha, beta, data[u]), D)
    return System("band", N, alpha, beta, data, _cast(b, dtype), A, forest_solution(D, O, p, b), dict(l=l, u=u))


def block_data(A, nb, bs, alpha, beta, dtype):
    """BlockBandedMatrix data (uniform blocks, block bandwidths (1, 1): block column J's in-band blocks stacked into one column-major
    panel, panels one after the other) holding J = (A - alpha I) / beta."""
    N = nb * bs
    chunks = []
    Ad = {k: v for k, v in A.items()}
    dense = scipy.sparse.dia_matrix((np.array([np.roll(v, k) for k, v in Ad.items()]), list(Ad.keys())), shape=(N, N)).tocsc()
    dense = (dense - alpha * scipy.sparse.identity(N, format="csc")) / beta
    for Jb in range(nb):
        K0, K1 = max(0, Jb - 1), min(nb - 1, Jb + 1)
        panel = dense[K0 * bs:(K1 + 1) * bs, Jb * bs:(Jb + 1) * bs].toarray()
        chunks.append(panel.reshape(-1, order="F"))
    return _cast(np.concatenate(chunks), dtype)


def block_seen(data, nb, bs, alpha, beta):
    """The diagonals of alpha I + beta J from BlockBandedMatrix data, as the device computes them."""
    N = nb * bs
    data = np.asarray(data, np.float64)
    rows, cols, vals = [], [], []
    pos = 0
    for Jb in range(nb):
        K0, K1 = max(0, Jb - 1), min(nb - 1, Jb + 1)
        st = (K1 - K0 + 1) * bs
        rr, cc = np.meshgrid(K0 * bs + np.arange(st), Jb * bs + np.arange(bs), indexing="ij")
        rows.append(rr.ravel()); cols.append(cc.ravel()); vals.append(beta * data[pos:pos + st * bs].reshape((st, bs), order="F").ravel())
        pos += st * bs
    assert pos == data.size
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    A = {}
    for k in np.unique((cols - rows)[(vals != 0) | (cols == rows)]):
        m = cols - rows == k
        v = np.zeros(N); v[rows[m]] = vals[m]
        A[int(k)] = v
    A[0] = alpha + A[0]
    return A


def e_block(nb, bs, seed, lower=True, shift=(0.0, 1.0), dtype=np.float64):
    """p(i) anywhere in the previous block or earlier in the same block (mirrored: next block / later in the same block)."""
    rng = _rng(seed)
    alpha, beta = shift
    N = nb * bs
    D = _diag_for(shift, rng, N)
    i = np.arange(N)
    blk, lane = i // bs, i % bs
    lo = np.maximum(blk - 1, 0) * bs                         # candidates [lo, i) (lower)
    if lower:
        cnt = i - lo
        p = lo + (rng.random(N) * np.maximum(cnt, 1)).astype(np.int64)
    else:
        hi = np.minimum(blk + 2, nb) * bs                    # candidates (i, hi)
        cnt = hi - 1 - i
        p = i + 1 + (rng.random(N) * np.maximum(cnt, 1)).astype(np.int64)
    has = cnt > 0
    O = np.where(has, rng.choice([-1.0, 1.0], N), 0.0)
    p = np.where(has, p, i)
    b = rng.integers(-1, 2, N).astype(np.float64)
    A = _forest_system(N, D, O, p)
    data = block_data(A, nb, bs, alpha, beta, dtype)
    return System("block", N, alpha, beta, data, _cast(b, dtype), A, forest_solution(D, O, p, b), dict(nb=nb, bs=bs))


# ------------------------------------------------------------------------------------------------------------ family S
def _quant(x, bits=10):
    """x rounded to `bits` significant bits: r (2 + delta) and the shifted diagonals stay exactly representable."""
    m, e = np.frexp(x)
    return float(np.ldexp(np.round(m * 2 ** bits), e - bits))


def tri_levels(n):
    ns = [int(n)]
    while ns[-1] > KTOP:
        ns.append((ns[-1] + KCHUNK - 1) // KCHUNK)
    return ns


def bcr_levels(n):
    ns = [int(n)]
    while ns[-1] > 1:
        ns.append(ns[-1] // 2)
    return ns


def tri_default_lam(N):
    """A decay length that crosses the highest level a system of N rows has (its rows are 8^(levels - 1) apart)."""
    return float(max(4, KCHUNK ** (len(tri_levels(N)) - 1)))


def _scaled(T, N, rng, scale):
    """R S T S for T given as diagonals: random signs S and (scale) random powers of two R per row."""
    s = rng.choice([-1.0, 1.0], N)
    r = np.ldexp(1.0, rng.integers(-3, 4, N)) if scale else np.ones(N)
    out = {}
    for k, v in T.items():
        sk = np.zeros(N)
        if k >= 0: sk[:N - k] = s[k:]
        else: sk[-k:] = s[:N + k]
        out[k] = r * s * v * sk
    return out


def _shifted(A, alpha, beta, dtype):
    """J = (A - alpha I) / beta in the solver's type, and the matrix the device then sees (asserted equal to A in Float64 storage)."""
    J = {k: _cast((v - (alpha if k == 0 else 0.0)) / beta, dtype) for k, v in A.items()}
    seen = {k: (_seen(alpha, beta, v) if k == 0 else beta * v.astype(np.float64)) for k, v in J.items()}
    return J, seen


def s_tridiag(N, lam, seed, dtype=np.float64, shift=None):
    """T = tridiag(-1, 2 + delta, -1), delta = 1 / lam^2; A = R S T S.  Float64: J through (alpha, beta) = `shift` (default (1, -1/2)).
    Float32: 2 + delta is not a Float32 number, so R = I, J = S tridiag(-1, 2, -1) S and the shift carries delta: (delta, 1)."""
    rng = _rng(seed)
    delta = _quant(1.0 / lam ** 2)
    f32 = np.dtype(dtype) == np.float32
    i = np.arange(N)
    T = {-1: np.where(i > 0, -1.0, 0.0), 0: np.full(N, 2.0 if f32 else 2.0 + delta), 1: np.where(i < N - 1, -1.0, 0.0)}
    A = _scaled(T, N, rng, scale=not f32)
    alpha, beta = (0.0, 1.0) if f32 else (shift or (1.0, -0.5))
    J, seen = _shifted(A, alpha, beta, dtype)
    if f32:
        alpha = delta
        seen[0] = _seen(alpha, beta, J[0])
    else:
        assert all(np.array_equal(seen[k], A[k]) for k in A), "the shift is not exact"
    b = _cast(rng.standard_normal(N), dtype)
    return System("tri", N, alpha, beta, (J[-1][1:], J[0], J[1][:-1]), b, seen, None, dict(lam=lam, delta=delta))


def band_delta(l, u, lam):
    """delta of T = (l + u)(1 + delta) I - ones(band) for a decay length of lam rows: the symbol (l + u) delta + sum_k (1 - z^k) has a
    root z = 1 + eps with eps = (l + u) delta / |m1| when the first moment m1 = sum_{k<=u} k - sum_{k<=l} k is not 0 (a one-sided slow
    decay; the other side decays in O(1) rows), and eps^2 = 2 (l + u) delta / m2 (second moment, both sides) when it is."""
    m1 = sum(range(1, u + 1)) - sum(range(1, l + 1))
    m2 = sum(k * k for k in range(1, u + 1)) + sum(k * k for k in range(1, l + 1))
    return _quant(abs(m1) / ((l + u) * lam) if m1 else m2 / (2.0 * (l + u) * lam ** 2))


def s_banded(N, l, u, lam, seed, dtype=np.float64, shift=None):
    rng = _rng(seed)
    delta = band_delta(l, u, lam)
    f32 = np.dtype(dtype) == np.float32
    i = np.arange(N)
    T = {k: np.where((i + k >= 0) & (i + k < N), -1.0, 0.0) for k in range(-l, u + 1) if k}
    T[0] = np.full(N, float(l + u) if f32 else (l + u) * (1.0 + delta))
    A = _scaled(T, N, rng, scale=not f32)
    alpha, beta = (0.0, 1.0) if f32 else (shift or (1.0, -0.5))
    J, seen = _shifted(A, alpha, beta, dtype)
    if f32:
        alpha = (l + u) * delta
        seen[0] = _seen(alpha, beta, J[0])
    else:
        assert all(np.array_equal(seen[k], A[k]) for k in A), "the shift is not exact"
    data = np.zeros((l + u + 1, N), dtype)
    for k, v in J.items():                                    # J[i, i + k] -> data[u - k, i + k]
        rows = i[(i + k >= 0) & (i + k < N)]
        data[u - k, rows + k] = v[rows]
    b = _cast(rng.standard_normal(N), dtype)
    return System("band", N, alpha, beta, data, b, seen, None, dict(l=l, u=u, lam=lam, delta=delta))


def s_block_dominant(nb, bs, lam, seed, dtype=np.float64):
    """bs chains tridiag(-1, 2 + delta, -1) of nb unknowns each, chain c sitting in lane pi_K(c) of block K (pi_K random): diagonal
    blocks (2 + delta) I, off-diagonal blocks signed permutations; then R S . S as for the scalar systems.  Row dominant: status 0."""
    rng = _rng(seed)
    N = nb * bs
    delta = _quant(1.0 / lam ** 2)
    f32 = np.dtype(dtype) == np.float32
    pi = np.array([rng.permutation(bs) for _ in range(nb)])                 # pi[K, c]: lane of chain c in block K
    rows = (np.arange(nb)[:, None] * bs + pi)                               # global row of (K, c)
    s = rng.choice([-1.0, 1.0], N)
    r = np.ones(N) if f32 else np.ldexp(1.0, rng.integers(-3, 4, N))
    rr = [np.arange(N)]; cc = [np.arange(N)]; vv = [r * (2.0 if f32 else 2.0 + delta)]
    if nb > 1:
        a, c = rows[1:].ravel(), rows[:-1].ravel()                          # (K, c) <-> (K - 1, c)
        rr += [a, c]; cc += [c, a]; vv += [-r[a] * s[a] * s[c], -r[c] * s[c] * s[a]]
    M = scipy.sparse.coo_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(N, N)).todia()
    A = {int(k): np.roll(M.data[q], -int(k)) for q, k in enumerate(M.offsets)}
    alpha, beta = (0.0, 1.0) if f32 else (1.0, -0.5)
    data = block_data(A, nb, bs, alpha, beta, dtype)
    if f32:
        alpha = delta
    seen = block_seen(data, nb, bs, alpha, beta)
    if not f32:
        assert all(np.array_equal(seen[k], A[k]) for k in seen), "the shift is not exact"
    b = _cast(rng.standard_normal(N), dtype)
    return System("block", N, alpha, beta, data, b, seen, None, dict(nb=nb, bs=bs, lam=lam, delta=delta))


def spd_block(bs, rng):
    """G = Q diag(w) Q^T, Q the orthogonal factor of a Gaussian matrix, w uniform in [1, 3.9]: SPD with condition <= 3.9 (< 4 after
    rounding)."""
    Q, _ = np.linalg.qr(rng.standard_normal((bs, bs)))
    w = rng.uniform(1.0, 3.9, bs)
    w[0], w[-1] = 1.0, 3.9
    G = (Q * w) @ Q.T
    return 0.5 * (G + G.T)


def s_block_dense(nb, bs, lam, seed, dtype=np.float64):
    """A = T_delta (x) G with G dense SPD (spd_block): NOT row dominant for bs >= 2 -- the trust policy's case.  (alpha, beta) = (0, 1);
    Float32: delta = 2^-k >= 2^-20 so that (2 + delta) G keeps delta after rounding; the matrix is what the rounded data hold."""
    rng = _rng(seed)
    N = nb * bs
    delta = _quant(1.0 / lam ** 2)
    if np.dtype(dtype) == np.float32:
        delta = max(2.0 ** np.round(np.log2(delta)), 2.0 ** -20)
    G = spd_block(bs, rng)
    chunks = []
    for Jb in range(nb):
        K0, K1 = max(0, Jb - 1), min(nb - 1, Jb + 1)
        panel = np.concatenate([((2.0 + delta) if K == Jb else -1.0) * G for K in range(K0, K1 + 1)], axis=0)
        chunks.append(panel.reshape(-1, order="F"))
    data = _cast(np.concatenate(chunks), dtype)
    seen = block_seen(data, nb, bs, 0.0, 1.0)
    b = _cast(rng.standard_normal(N), dtype)
    return System("block", N, 0.0, 1.0, data, b, seen, None, dict(nb=nb, bs=bs, lam=lam, delta=delta, condG=float(np.linalg.cond(G))))


# ------------------------------------------------------------------------------------------------------------ references
def to_sparse(A, N):
    offs = sorted(A)
    return scipy.sparse.dia_matrix((np.array([np.roll(A[k], k) for k in offs]), offs), shape=(N, N))


def _matvec_ld(A, x):
    """A x in np.longdouble (64-bit significand here: products of two Float64 numbers are exact in it up to one rounding at 2^-64)."""
    N = x.size
    out = np.zeros(N, np.longdouble)
    for k, v in A.items():
        vl = v.astype(np.longdouble)
        if k >= 0:
            out[:N - k] += vl[:N - k] * x[k:]
        else:
            out[-k:] += vl[-k:] * x[:N + k]
    return out


def lapack_solver(A, N):
    """x = A^-1 r in Float64: LAPACK's banded LU for narrow bands, SuperLU otherwise."""
    lo, up = -min(A), max(A)
    if lo + up <= 16:
        ab = np.zeros((lo + up + 1, N))
        for k, v in A.items():
            ab[up - k] = np.roll(v, k)                         # ab[up + i - j, j] = A[i, j], j = i + k
        return lambda r: scipy.linalg.solve_banded((lo, up), ab, r)
    lu = scipy.sparse.linalg.splu(to_sparse(A, N).tocsc())
    return lu.solve


def refined_reference(sysm):
    """(y_ref as np.longdouble, E_lapack): Float64 LU, then iterative refinement with the residual in extended precision until the
    correction stops shrinking.  E_lapack = ||x_lapack - y_ref||_inf, the error of the plain Float64 solve of the same system."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not extended precision here"
    A, N = sysm.A, sysm.N
    b = sysm.b.astype(np.longdouble)
    solve = lapack_solver(A, N)
    x0 = solve(sysm.b.astype(np.float64))
    x = x0.astype(np.longdouble)
    prev = np.inf
    for _ in range(12):
        r = b - _matvec_ld(A, x)
        dx = solve(r.astype(np.float64))
        nrm = float(np.max(np.abs(dx)))
        if not nrm < 0.5 * prev:
            break
        x = x + dx.astype(np.longdouble)
        prev = nrm
    return x, float(np.max(np.abs(x0.astype(np.longdouble) - x)))


def s_tolerance(y_ref, e_lapack, dtype=np.float64, factor=16.0):
    """||y - y_ref||_inf <= factor * max(E_lapack, eps ||y_ref||) (+ the output rounding of a Float32 solver): a pivot-free partition /
    cyclic reduction of a row dominant matrix has LU's backward error form with growth <= 2 and a constant proportional to the
    elimination depth (<= 8 levels of radix 8; E_lapack is one sample of cond * eps)."""
    nrm = float(np.max(np.abs(y_ref)))
    tol = factor * max(e_lapack, np.finfo(np.float64).eps * nrm)
    if np.dtype(dtype) == np.float32:
        tol += 2.0 ** -24 * nrm
    return tol


# ------------------------------------------------------------------------------------------------------------ host models
def _fault(x, mode):
    return np.zeros_like(x) if mode == "zero" else -x


def _refault(model, L, mode):
    m = copy.copy(model)
    m.fault = None
    a, b, c, d = model.levels[L]
    m.levels = model.levels[:L] + [(_fault(a, mode), b, _fault(c, mode), d)]
    for k in range(L + 1, len(model.ns)):
        m.levels.append(m._reduce(*m.levels[-1], k))
    return m


class TriModel:
    """The recursive partition of fdjac_solve.hip for a x_{i-1} + b x_i + c x_{i+1} = d: chunks of 8 rows, a downward and an upward sweep
    per chunk leave one equation per chunk in the chunk's LAST unknown; levels until <= 512 rows; back-substitution of every level from
    the two boundary values of each chunk."""

    def __init__(self, a, b, c, d, fault=None):
        self.levels = [tuple(np.asarray(v, np.float64) for v in (a, b, c, d))]
        self.ns = tri_levels(len(self.levels[0][1]))
        self.fault = fault
        for L in range(1, len(self.ns)):
            self.levels.append(self._reduce(*self.levels[-1], L))

    @property
    def fault_levels(self):
        return list(range(1, len(self.ns)))

    def with_fault(self, L, mode):
        """This model with the couplings of level L corrupted (the levels below are shared, the ones above recomputed)."""
        return _refault(self, L, mode)

    @staticmethod
    def _pad(a, b, c, d):
        n = b.size
        nc = (n + KCHUNK - 1) // KCHUNK
        pad = nc * KCHUNK - n
        f = lambda v, fill: np.concatenate([v, np.full(pad, fill)]).reshape(nc, KCHUNK).copy()
        return f(a, 0.0), f(b, 1.0), f(c, 0.0), f(d, 0.0)

    @classmethod
    def _down(cls, a, b, c, d):
        f, b, c, d = cls._pad(a, b, c, d)
        for i in range(1, KCHUNK):
            mult = f[:, i] / b[:, i - 1]
            f[:, i] = -mult * f[:, i - 1]
            b[:, i] -= mult * c[:, i - 1]
            d[:, i] -= mult * d[:, i - 1]
        return f, b, c, d

    def _reduce(self, a, b, c, d, L):
        f, b, c, d = self._down(a, b, c, d)
        fe, be, ce, de = f[:, -1], b[:, -1], c[:, -1], d[:, -1]
        cf, cb, cg, cd = f[:, -2].copy(), b[:, -2].copy(), c[:, -2].copy(), d[:, -2].copy()
        for i in range(KCHUNK - 3, -1, -1):                   # the first row through the unknown before the chunk and the chunk's last
            mult = c[:, i] / cb
            cf = f[:, i] - mult * cf
            cg = -mult * cg
            cd = d[:, i] - mult * cd
            cb = b[:, i]
        t = np.zeros_like(ce)
        t[:-1] = ce[:-1] / cb[1:]
        na, nb, nc_, nd = fe.copy(), be.copy(), np.zeros_like(ce), de.copy()
        nb[:-1] -= t[:-1] * cf[1:]
        nc_[:-1] = -t[:-1] * cg[1:]
        nd[:-1] -= t[:-1] * cd[1:]
        if self.fault and self.fault[0] == L:
            na, nc_ = _fault(na, self.fault[1]), _fault(nc_, self.fault[1])
        return na, nb, nc_, nd

    @staticmethod
    def _thomas(a, b, c, d):
        n = b.size
        bb, dd = b.copy(), d.copy()
        for i in range(1, n):
            m = a[i] / bb[i - 1]
            bb[i] -= m * c[i - 1]
            dd[i] -= m * dd[i - 1]
        x = np.zeros(n)
        x[-1] = dd[-1] / bb[-1]
        for i in range(n - 2, -1, -1):
            x[i] = (dd[i] - c[i] * x[i + 1]) / bb[i]
        return x

    def solve(self, down_to=0):
        """The solution of level `down_to` (level L's unknowns are rows 8^L k + 8^L - 1 of level 0, where they exist)."""
        x = self._thomas(*self.levels[-1])
        for L in range(len(self.ns) - 2, down_to - 1, -1):
            f, b, c, d = self._down(*self.levels[L])
            nc = f.shape[0]
            z = np.zeros(nc); z[:x.size] = x
            prev = np.concatenate([[0.0], z[:-1]])
            X = np.empty_like(b)
            X[:, -1] = z
            for i in range(KCHUNK - 2, -1, -1):
                X[:, i] = (d[:, i] - f[:, i] * prev - c[:, i] * X[:, i + 1]) / b[:, i]
            x = X.reshape(-1)[:self.ns[L]]
            # (a padded last chunk's "last unknown" is a padding row's: the level above solved 0 for it)
        return x

    def level_rows(self, L):
        """Row of level 0 that each unknown of level L is; -1 for the padding unknown a short last chunk contributes."""
        idx = np.arange(self.ns[0])
        for _ in range(L):
            idx = np.concatenate([idx, np.full(-idx.size % KCHUNK, -1)])[KCHUNK - 1::KCHUNK]
        return idx


def tri_rows(sysm):
    A, N = sysm.A, sysm.N
    z = np.zeros(N)
    return A.get(-1, z), A[0], A.get(1, z), sysm.b.astype(np.float64)


def _gauss_jordan(B, R):
    """B^-1 R without pivoting, batched over the leading axis (the elimination of fdjac_blocksolve.hip / the K x K inverses of
    fdjac_bandsolve.hip; exact on family E, where every pivot is +-1)."""
    M = np.concatenate([B, R], axis=2).astype(np.float64)
    K = B.shape[1]
    for p in range(K):
        M[:, p, :] = M[:, p, :] / M[:, p, p][:, None]
        fcol = M[:, :, p].copy()
        fcol[:, p] = 0.0
        M -= fcol[:, :, None] * M[:, p, :][:, None, :]
    return M[:, :, K:]


def tri_sharded_model(a, b, c, d, cuts, tip_fault=None, fault=None):
    """SPIKE over the ranks' row ranges: T_r [g v w] = [d e_first e_last] per rank, the 2W x 2W interface system in the ranks' first and
    last unknowns, then T_r y = d - coupling * neighbour value.  tip_fault = (rank, mode) corrupts that rank's v and w tips."""
    W = len(cuts) - 1
    tips = []
    for r in range(W):
        c0, c1 = cuts[r], cuts[r + 1]
        n = c1 - c0
        al, cl = a[c0:c1].copy(), c[c0:c1].copy()
        lo, up = al[0], cl[-1]
        al[0] = 0.0; cl[-1] = 0.0
        e0 = np.zeros(n); e0[0] = 1.0
        e1 = np.zeros(n); e1[-1] = 1.0
        sol = [TriModel(al, b[c0:c1], cl, rhs, fault=fault).solve() for rhs in (d[c0:c1], e0, e1)]
        g, v, w = [(s[0], s[-1]) for s in sol]
        if tip_fault and tip_fault[0] == r:
            v, w = tuple(_fault(np.array(v), tip_fault[1])), tuple(_fault(np.array(w), tip_fault[1]))
        tips.append((g, v, w, lo if r > 0 else 0.0, up if r + 1 < W else 0.0))
    # unknowns: (first_r, last_r) at 2r, 2r + 1:  y_first = g_f - v_f lo last_{r-1} - w_f up first_{r+1}, the same for y_last
    M = np.eye(2 * W); rhs = np.zeros(2 * W)
    for r, (g, v, w, lo, up) in enumerate(tips):
        for q in (0, 1):
            rhs[2 * r + q] = g[q]
            if r > 0: M[2 * r + q, 2 * r - 1] += v[q] * lo
            if r + 1 < W: M[2 * r + q, 2 * r + 2] += w[q] * up
    z = _gauss_jordan(M[None], rhs[None, :, None])[0, :, 0]
    y = np.empty(b.size)
    for r, (g, v, w, lo, up) in enumerate(tips):
        c0, c1 = cuts[r], cuts[r + 1]
        al, cl, dl = a[c0:c1].copy(), c[c0:c1].copy(), d[c0:c1].copy()
        al[0] = 0.0; cl[-1] = 0.0
        if r > 0: dl[0] -= lo * z[2 * r - 1]
        if r + 1 < W: dl[-1] -= up * z[2 * r + 2]
        y[c0:c1] = TriModel(al, b[c0:c1], cl, dl, fault=fault).solve()
    return y


class BcrModel:
    """Radix-2 block cyclic reduction of a block-tridiagonal system with K x K blocks (block rows A_i x_{i-1} + B_i x_i + C_i x_{i+1} =
    d_i): a step keeps the odd block rows, A' = -A_i Bi_{i-1} A_{i-1}, B' = B_i - A_i Bi_{i-1} C_{i-1} - C_i Bi_{i+1} A_{i+1},
    C' = -C_i Bi_{i+1} C_{i+1} (Bi = B^-1), down to one block row; the even rows are then solved from their two known neighbours."""

    def __init__(self, A, B, C, d, fault=None):
        self.fault = fault
        self.levels = [(A, B, C, d)]
        self.ns = bcr_levels(B.shape[0])
        for L in range(1, len(self.ns)):
            self.levels.append(self._reduce(*self.levels[-1], L))

    @property
    def fault_levels(self):
        """Levels whose couplings are ever read: a level of one block row has no neighbour."""
        return [L for L in range(1, len(self.ns)) if self.ns[L] >= 2]

    def with_fault(self, L, mode):
        return _refault(self, L, mode)

    def _reduce(self, A, B, C, d, L):
        n, K = B.shape[0], B.shape[1]
        S = _gauss_jordan(B, np.concatenate([A, C, d[:, :, None]], axis=2))          # B^-1 [A | C | d] of every row
        SA, SC, Sd = S[:, :, :K], S[:, :, K:2 * K], S[:, :, 2 * K]
        odd = np.arange(1, n, 2)
        Ai, Ci = A[odd], C[odd]
        nA = -Ai @ SA[odd - 1]
        nB = B[odd] - Ai @ SC[odd - 1]
        nd = d[odd] - (Ai @ Sd[odd - 1][:, :, None])[:, :, 0]
        nC = np.zeros_like(nA)
        has = odd + 1 < n
        o2 = odd[has]
        nB[has] -= Ci[has] @ SA[o2 + 1]
        nC[has] = -Ci[has] @ SC[o2 + 1]
        nd[has] -= (Ci[has] @ Sd[o2 + 1][:, :, None])[:, :, 0]
        if self.fault and self.fault[0] == L:
            nA, nC = _fault(nA, self.fault[1]), _fault(nC, self.fault[1])
        return nA, nB, nC, nd

    def solve(self, down_to=0):
        A, B, C, d = self.levels[-1]
        x = _gauss_jordan(B, d[:, :, None])[:, :, 0]
        for L in range(len(self.ns) - 2, down_to - 1, -1):
            A, B, C, d = self.levels[L]
            n = B.shape[0]
            X = np.zeros((n, B.shape[1]))
            X[1:2 * x.shape[0]:2] = x
            ev = np.arange(0, n, 2)
            r = d[ev].copy()
            lo = ev > 0
            r[lo] -= (A[ev[lo]] @ X[ev[lo] - 1][:, :, None])[:, :, 0]
            hi = ev + 1 < n
            r[hi] -= (C[ev[hi]] @ X[ev[hi] + 1][:, :, None])[:, :, 0]
            X[ev] = _gauss_jordan(B[ev], r[:, :, None])[:, :, 0]
            x = X
        return x

    def level_rows(self, L):
        idx = np.arange(self.ns[0])
        for _ in range(L):
            idx = idx[1::2]
        return idx


def bcr_blocks(sysm, K):
    """The block rows (A, B, C, d) of a System for block size K (rows past N: identity, as level 0 of fdjac_bandsolve.hip pads)."""
    N = sysm.N
    n = (N + K - 1) // K
    Np = n * K
    A = np.zeros((n, K, K)); B = np.zeros((n, K, K)); C = np.zeros((n, K, K))
    d = np.zeros(Np); d[:N] = sysm.b.astype(np.float64)
    i = np.arange(N)
    I, a = i // K, i % K
    for k, v in sysm.A.items():
        ok = (i + k >= 0) & (i + k < N) & ((v != 0) | (k == 0))
        rows = i[ok]
        cb = a[ok] + k                                        # column relative to the block row's first column
        for blk, lo in ((A, -K), (B, 0), (C, K)):
            m = (cb >= lo) & (cb < lo + K)
            blk[I[ok][m], a[ok][m], cb[m] - lo] = v[rows[m]]
        assert np.all((cb >= -K) & (cb < 2 * K))
    pad = np.arange(N, Np)
    B[pad // K, pad % K, pad % K] = 1.0
    return A, B, C, d.reshape(n, K)


def band_K(l, u):
    return max(l, u)


# ------------------------------------------------------------------------------------------------------------ the cases of the GPU file
# (shared with tests/test_solve_model_cpu.py, which proves for every one of them that a fault at any level fails the GPU assertion)
TRI_N = [1, 2, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2113, 4095, 4096, 4097, 16385, 32769, 100003, 262143, 262144,
         262145, 10 ** 6, 3 * 10 ** 6 + 1]                     # the list of test_tridiagonal_solve_matches_scipy
TRI_E_N = TRI_N + [10 ** 7]
TRI_S_CASES = [(N, tri_default_lam(N)) for N in TRI_N] + [(3 * 10 ** 6 + 1, 3.0e5)]
TRI_SCHEDULE_N = [4095, 4096, 4097, 32769, 262143, 262144, 262145, 2 ** 21 + 65]       # around the 4096 / 262144 boundaries
TRI_F32 = 50021
TRI_CHAIN_N = [9, 513, 4097, 262145, 10 ** 6]          # one chain through the whole system, lower and upper
# sharded: (N, cuts); uneven, with a 1-row and an 8-row rank
TRI_SHARDED = [(40, [0, 1, 40]), (5003, [0, 8, 2500, 5003]), (100003, [0, 1, 9, 15000, 30000, 30001, 55000, 99995, 100003]),
               (70001, [0, 30000, 70001]), (9000, [0, 2048, 2049, 9000])]

BAND_SHAPES = [(1, 1, 1), (2, 2, 2), (7, 2, 2), (1000, 2, 2), (4097, 2, 1), (100003, 1, 2), (50001, 3, 3), (30000, 4, 4), (2049, 0, 2),
               (3000, 4, 0), (10 ** 6 + 1, 2, 2)]              # the list of test_banded_solve_matches_scipy
# N = K 2^m + {-1, 0, 1} where the level size crosses kBcrTopRows = 1024: ceil(N / K) = 1024 / 1025 (m = 10) and 2048 / 2049 (m = 11)
BAND_SHAPES += [(K * 2 ** m + e, l, u) for (K, l, u) in ((2, 2, 2), (3, 1, 3)) for m in (10, 11) for e in (-1, 0, 1)]
BLOCK_SHAPES = [(1, 32), (2, 32), (3, 31), (7, 32), (100, 32), (1000, 16), (1023, 5), (1024, 4), (1025, 4), (4097, 4), (100, 1), (1000, 1),
                (7, 5), (100, 16), (3, 4)]
BLOCK_DENSE_SHAPES = [(nb, bs) for nb, bs in BLOCK_SHAPES if bs >= 4]      # (bs = 1: T (x) g IS row dominant -- the dominant family)


def band_lam(N, l, u):
    """Decay length that crosses the highest level: a quarter of the system, at most 2^16 rows.  The cap only binds at N = 10^6 + 1,
    where a fault at the top level still misses the tolerance by a factor > 2000 (test_solve_model_cpu.py), while lam = N / 4 puts
    cond(A) near 10^11 and makes E_lapack -- ONE sample of cond * eps -- swing by two orders of magnitude between the Float64 and the
    Float32 twin of the case (profiles/solver_accuracy.md)."""
    return float(max(4, min(N // 4, 2 ** 16)))


def block_lam(nb):
    return float(max(2, nb // 4))


# seeds: a family-E case must differ from its faulted self at EVERY level (test_solve_model_cpu.py); where the first seed happens to put a
# zero of y under the one coupling a level has, the case takes the next seed that does not (found by that test's own criterion)
E_SEED_BUMP = {("band", 7, 2, 2, False): 1, ("band", 2048, 2, 2, False): 1, ("band", 6145, 1, 3, False): 1, ("block", 4097, 4, False): 1}


def gpu_band_systems(N, l, u, dtype, s_shift=None):
    q = BAND_SHAPES.index((N, l, u))
    sysS = s_banded(N, l, u, band_lam(N, l, u), 59 + q, dtype, shift=s_shift)
    sysE = [e_banded(N, l, u, 61 + q + 1000 * E_SEED_BUMP.get(("band", N, l, u, lower), 0), lower, E_SHIFTS[(q + lower) % 4], dtype)
            for lower in (True, False) if (l if lower else u) > 0]
    return sysS, sysE


def gpu_block_systems(nb, bs, dtype):
    q = BLOCK_SHAPES.index((nb, bs))
    sysS = s_block_dominant(nb, bs, block_lam(nb), 67 + q, dtype)
    sysE = [e_block(nb, bs, 71 + q + 1000 * E_SEED_BUMP.get(("block", nb, bs, lower), 0), lower, E_SHIFTS[(q + lower) % 4], dtype)
            for lower in (True, False)]
    return sysS, sysE
