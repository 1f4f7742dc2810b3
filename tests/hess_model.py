"""Exact host model of the objective Hessian / gradient contract (include/fdjac.h, fd_hessian / fd_gradient), and an independent
restatement of the reference's dense loops (src/hessians.jl:202-292, src/gradients.jl:407-446).

An objective is f(x) = sum_{r<M} phi_r(x).  Here phi is written ONCE for both sides as ``phi(r, get)``: ``r`` is an int64 array of
row numbers (one per lane), ``get(k)`` returns coordinate k of each lane's point (k an int64 array of the same shape).  Every
operation is numpy float64 ELEMENTWISE arithmetic -- exactly the IEEE operation of one scalar, lane by lane, never fused -- so a
vector of lanes is that many scalar evaluations in the contract's order (the device compiles with -ffp-contract=off).

The model (hessian / gradient) follows the contract: per-row differences, summed over the rows of each entry left to right in
ascending r, divided once.  The restatement (ref_hessian / ref_gradient) follows the reference's text: whole-f differences on
copies of x.  With M = 1 and dense support the two are the same operations; tests/test_hessian_cpu.py checks that bit for bit.
"""
import numpy as np

HESS_RELSTEP = 2.0 ** -13                        # eps(Float64)^(1/4)  (src/epsilons.jl:133-144, Val(:hcentral))
FWD_RELSTEP = float(np.sqrt(np.finfo(np.float64).eps))
CEN_RELSTEP = float(np.cbrt(np.finfo(np.float64).eps))


def step(x, relstep, absstep, fault=None):
    """max(relstep * |x|, absstep) with Julia's max: a NaN on either side is the result (src/epsilons.jl:74-77).
    (fault: a perturbed model of tests/test_hessian_cpu.py -- "fmax": C's fmax, which drops a NaN; "no_abs": relstep * x.)"""
    a = np.float64(relstep) * (np.asarray(x, np.float64) if fault == "no_abs" else np.abs(x))
    if fault == "fmax":
        return np.fmax(a, np.float64(absstep))
    return np.where((a > absstep) | (a != a), a, np.float64(absstep))


def _defaults(relstep, absstep, default):
    relstep = default if relstep is None or relstep <= 0 else float(relstep)
    absstep = relstep if absstep is None or absstep < 0 else float(absstep)
    return relstep, absstep


def support(M, N, colptr=None, rowval=None):
    """S as 0-based (colptr, rowval), rows ascending and unique per column; colptr None: dense support."""
    if colptr is None:
        return np.arange(N + 1, dtype=np.int64) * M, np.tile(np.arange(M, dtype=np.int64), N)
    colptr, rowval = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64)
    cp, rv = [0], []
    for j in range(N):
        rows = np.unique(rowval[colptr[j]:colptr[j + 1]])
        rv.extend(rows.tolist())
        cp.append(len(rv))
    return np.array(cp, np.int64), np.array(rv, np.int64)


def _point(x, ii, jj, vi, vj, fault=None):
    """the lanes' points: x with coordinate ii -> vi, then jj -> vj (jj overrides ii when equal), as fd_pair_point
    (fault "vi_over_vj": ii overrides jj)"""
    def get(k):
        k = np.asarray(k, np.int64)
        v = x[k]
        if fault == "vi_over_vj":
            v = np.where(k == jj, vj, v)
            return np.where(k == ii, vi, v)
        v = np.where(k == ii, vi, v)
        return np.where(k == jj, vj, v)
    return get


def _row_triples(M, N, cp, rv):
    """every (r, i, j), i <= j, with i and j both in row r's support, sorted by (j, i, r)"""
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(cp))
    order = np.lexsort((cols, rv))
    r_s, c_s = rv[order], cols[order]
    rp = np.zeros(M + 1, np.int64)
    np.add.at(rp, r_s + 1, 1)
    rp = np.cumsum(rp)
    per = np.diff(rp)[r_s]
    first = np.repeat(rp[r_s], per)
    k = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    r, i, j = np.repeat(r_s, per), np.repeat(c_s, per), c_s[first + k]
    keep = i <= j
    r, i, j = r[keep], i[keep], j[keep]
    o = np.lexsort((r, i, j))
    return r[o], i[o], j[o]


FAULTS = ("desc_rows", "four_last", "diag_assoc", "fmax", "no_abs", "dir_quot", "vi_over_vj", "diag_empty")


def hessian_entries(phi, x, M, N, colptr=None, rowval=None, relstep=None, absstep=None, fault=None):
    """The contract's upper entries of P: (i, j, H_ij), i <= j, sorted by (j, i).  fault: None, or one of FAULTS -- the model perturbed
    in one place, to count the cases that would notice (tests/test_hessian_cpu.py); "desc_rows": every sum in descending r;
    "four_last": 4 (e_i e_j); "diag_assoc": (phi+ + phi-) - 2 phi; "diag_empty": a diagonal entry (an empty sum) for a column no row
    reads; "fmax" / "no_abs": see step; "vi_over_vj": see _point; "dir_quot" is the gradient's."""
    relstep, absstep = _defaults(relstep, absstep, HESS_RELSTEP)
    x = np.asarray(x, np.float64)
    cp, rv = support(M, N, colptr, rowval)
    _pt = _point if fault != "vi_over_vj" else (lambda *a: _point(*a, fault=fault))
    if fault == "diag_empty":
        fi, fj, h = hessian_entries(phi, x, M, N, cp, rv, relstep, absstep)
        unread = np.flatnonzero(np.diff(cp) == 0)
        e = step(x[unread], relstep, absstep)
        with np.errstate(all="ignore"):
            fi, fj, h = np.concatenate([fi, unread]), np.concatenate([fj, unread]), np.concatenate([h, np.zeros(unread.size) / (e * e)])
        o = np.lexsort((fi, fj))
        return fi[o], fj[o], h[o]
    fx = phi(np.arange(M, dtype=np.int64), _pt(x, -1, -1, 0.0, 0.0))
    r, i, j = _row_triples(M, N, cp, rv)
    if r.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    new = np.ones(r.size, bool)
    new[1:] = (i[1:] != i[:-1]) | (j[1:] != j[:-1])
    ent = np.cumsum(new) - 1                     # entry of every triple
    pos = np.arange(r.size) - np.flatnonzero(new)[ent]      # its place in the entry's ascending row list
    if fault == "desc_rows":
        pos = (np.bincount(ent)[ent] - 1) - pos
    ei_all = step(x, relstep, absstep, fault)
    ei, ej = ei_all[i], ei_all[j]
    xi, xj = x[i], x[j]
    xip, xim, xjp, xjm = xi + ei, xi - ei, xj + ej, xj - ej
    diag = i == j
    t = np.empty(r.size)
    if diag.any():
        d = diag
        fp = phi(r[d], _pt(x, i[d], i[d], xip[d], xip[d]))
        fm = phi(r[d], _pt(x, i[d], i[d], xim[d], xim[d]))
        t[d] = (fp - 2.0 * fx[r[d]]) + fm if fault != "diag_assoc" else (fp + fm) - 2.0 * fx[r[d]]
    if (~diag).any():
        o = ~diag
        a, b = i[o], j[o]
        pp = phi(r[o], _pt(x, a, b, xip[o], xjp[o]))
        pm = phi(r[o], _pt(x, a, b, xip[o], xjm[o]))
        mp = phi(r[o], _pt(x, a, b, xim[o], xjp[o]))
        mm = phi(r[o], _pt(x, a, b, xim[o], xjm[o]))
        t[o] = ((pp - pm) - mp) + mm
    nent = int(ent[-1]) + 1
    s = np.zeros(nent)
    for p in range(int(pos.max()) + 1):          # left to right over each entry's rows
        sel = pos == p
        s[ent[sel]] = t[sel] if p == 0 else s[ent[sel]] + t[sel]
    fi, fj = i[new], j[new]
    e_i, e_j = ei_all[fi], ei_all[fj]
    with np.errstate(all="ignore"):
        h = np.where(fi == fj, s / (e_i * e_i), s / ((4.0 * e_i) * e_j if fault != "four_last" else 4.0 * (e_i * e_j)))
    return fi, fj, h


def hessian(phi, x, M, N, colptr=None, rowval=None, relstep=None, absstep=None):
    """The contract's H (dense N x N; +0.0 outside P) and P's mask."""
    fi, fj, h = hessian_entries(phi, x, M, N, colptr, rowval, relstep, absstep)
    H = np.zeros((N, N))
    mask = np.zeros((N, N), bool)
    H[fi, fj] = h
    H[fj, fi] = h
    mask[fi, fj] = mask[fj, fi] = True
    return H, mask


def gradient(phi, x, M, N, fdtype, colptr=None, rowval=None, relstep=None, absstep=None, dir=1.0, fault=None):
    """The contract's gradient: forward (step times dir) or central, per-row differences summed in ascending r (empty: +0.0).
    A column no row reads holds +0.0 / e: -0.0 forward with dir = -1, NaN where e is NaN or 0.  fault: as hessian_entries;
    "dir_quot": dir multiplies the forward quotient, not the step."""
    relstep, absstep = _defaults(relstep, absstep, FWD_RELSTEP if fdtype == "forward" else CEN_RELSTEP)
    x = np.asarray(x, np.float64)
    cp, rv = support(M, N, colptr, rowval)
    e = step(x, relstep, absstep, fault)
    if fdtype == "forward" and fault != "dir_quot":
        e = e * np.float64(dir)
    j = np.repeat(np.arange(N, dtype=np.int64), np.diff(cp))
    r = rv
    pos = np.arange(r.size) - cp[j]
    if fault == "desc_rows":
        pos = (np.diff(cp)[j] - 1) - pos
    xp, xm = x[j] + e[j], x[j] - e[j]
    fp = phi(r, _point(x, j, j, xp, xp))
    if fdtype == "forward":
        fx = phi(np.arange(M, dtype=np.int64), _point(x, -1, -1, 0.0, 0.0))
        t = fp - fx[r]
    else:
        t = fp - phi(r, _point(x, j, j, xm, xm))
    s = np.zeros(N)
    for p in range(int(pos.max()) + 1 if pos.size else 0):
        sel = pos == p
        s[j[sel]] = t[sel] if p == 0 else s[j[sel]] + t[sel]
    with np.errstate(all="ignore"):
        if fdtype == "forward" and fault == "dir_quot":
            return (s / e) * np.float64(dir)
        return s / e if fdtype == "forward" else s / (2.0 * e)


# ---- the reference's text, restated (M = 1: f(x) = phi_0(x)) --------------------------------------------------------------------
def _f_batch(phi, X):
    """f at every row of X (points x batch), phi_0 evaluated lane by lane"""
    out = np.empty(X.shape[0])
    for a in range(0, X.shape[0], 4096):
        B = X[a:a + 4096]
        lanes = np.arange(B.shape[0])
        out[a:a + 4096] = phi(np.zeros(B.shape[0], np.int64), lambda k: B[lanes, np.asarray(k, np.int64)])
    return out


def ref_hessian(phi, x, relstep=None, absstep=None):
    """src/hessians.jl:202-292 for f = phi_0: every f(x') of the double loop, then the stores and copytri!(H, 'U')."""
    relstep, absstep = _defaults(relstep, absstep, HESS_RELSTEP)
    x = np.asarray(x, np.float64)
    n = x.size
    fx = _f_batch(phi, x[None, :])[0]
    pts, plan = [], []
    for i in range(n):
        xi = x[i]
        epsilon = step(xi, relstep, absstep)            # compute_epsilon(Val(:hcentral), xi, relstep, absstep)
        xpp, xmm = x.copy(), x.copy()
        xpp[i], xmm[i] = xi + epsilon, xi - epsilon
        plan.append(("d", i, i, epsilon, epsilon, len(pts)))
        pts += [xpp, xmm]
        epsiloni = step(xi, relstep, absstep)           # compute_epsilon(Val(:central), ...): the same formula
        for j in range(i + 1, n):
            xj = x[j]
            epsilonj = step(xj, relstep, absstep)
            pp, pm, mp, mm = x.copy(), x.copy(), x.copy(), x.copy()
            pp[i], pm[i], mp[i], mm[i] = xi + epsiloni, xi + epsiloni, xi - epsiloni, xi - epsiloni
            pp[j], pm[j], mp[j], mm[j] = xj + epsilonj, xj - epsilonj, xj + epsilonj, xj - epsilonj
            plan.append(("o", i, j, epsiloni, epsilonj, len(pts)))
            pts += [pp, pm, mp, mm]
    F = _f_batch(phi, np.array(pts))
    H = np.zeros((n, n))
    for kind, i, j, ea, eb, k in plan:
        if kind == "d":
            H[i, i] = (F[k] - 2.0 * fx + F[k + 1]) / (ea * ea)     # epsilon^2 is epsilon * epsilon (Base.literal_pow)
        else:
            H[i, j] = (F[k] - F[k + 1] - F[k + 2] + F[k + 3]) / (4.0 * ea * eb)
    iu = np.triu_indices(n, 1)
    H[(iu[1], iu[0])] = H[iu]                                       # copytri!(H, 'U')
    return H


def ref_gradient(phi, x, fdtype, relstep=None, absstep=None, dir=1.0):
    """src/gradients.jl:407-446 (the StridedVector method) for f = phi_0, real x and df."""
    relstep, absstep = _defaults(relstep, absstep, FWD_RELSTEP if fdtype == "forward" else CEN_RELSTEP)
    x = np.asarray(x, np.float64)
    n = x.size
    pts = []
    for i in range(n):
        epsilon = step(x[i], relstep, absstep)
        if fdtype == "forward":
            epsilon = epsilon * np.float64(dir)
        c3 = x.copy()
        c3[i] += epsilon
        pts.append(c3)
        if fdtype == "central":
            c3 = x.copy()
            c3[i] = x[i] - epsilon
            pts.append(c3)
    F = _f_batch(phi, np.array(pts))
    df = np.empty(n)
    if fdtype == "forward":
        fx0 = _f_batch(phi, x[None, :])[0]
        for i in range(n):
            epsilon = step(x[i], relstep, absstep) * np.float64(dir)
            df[i] = (F[i] - fx0) / epsilon
    else:
        for i in range(n):
            epsilon = step(x[i], relstep, absstep)
            dfi = F[2 * i]
            dfi = dfi - F[2 * i + 1]
            df[i] = dfi / (2.0 * epsilon)
    return df


# ---- test objectives: the device source and the same arithmetic as phi(r, get) --------------------------------------------------
def _full(r, k):
    return np.full(np.shape(r), k, np.int64)


# M = 1, dense support: a polynomial with division over all n coordinates (the reference's setting)
POLYDIV_SRC = r"""
struct PolyDiv {
    long long n;
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        real_t s = 0;
        for (long long k = 0; k < n; ++k) {
            const real_t a = X(k), b = X(k + 1 < n ? k + 1 : 0);
            s = s + (a * a * b + 0.5 * a - 0.25) / (1.0 + b * b);
        }
        return s;
    }
};
"""


def phi_polydiv(n):
    def phi(r, get):
        s = np.zeros(np.shape(r))
        for k in range(n):
            a, b = get(_full(r, k)), get(_full(r, (k + 1) % n))
            s = s + (a * a * b + 0.5 * a - 0.25) / (1.0 + b * b)
        return s
    return phi


# M = N: row r reads x[r-1], x[r], x[r+1] (the loads unconditional, then selected); convex, H diagonally dominant, P pentadiagonal
CHAIN_SRC = r"""
struct Chain {
    long long n;
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        const real_t b = X(r), a0 = X(r > 0 ? r - 1 : r), c0 = X(r + 1 < n ? r + 1 : r);
        const real_t a = r > 0 ? a0 : 0.0, c = r + 1 < n ? c0 : 0.0;
        const real_t d = (a - 2 * b) + c;
        return (2 * b * b + b * b * b * b / 12) + 0.1 * d * d;
    }
};
"""


def phi_chain(n):
    def phi(r, get):
        b = get(r)
        a0, c0 = get(np.where(r > 0, r - 1, r)), get(np.where(r + 1 < n, r + 1, r))
        a, c = np.where(r > 0, a0, 0.0), np.where(r + 1 < n, c0, 0.0)
        d = (a - 2.0 * b) + c
        return (2.0 * b * b + b * b * b * b / 12.0) + 0.1 * d * d
    return phi


def chain_support(n):
    """S of the chain (column j: rows j-1, j, j+1), 0-based"""
    j = np.arange(n, dtype=np.int64)
    rows = np.stack([j - 1, j, j + 1], axis=1)
    has = (rows >= 0) & (rows < n)
    colptr = np.concatenate([[0], np.cumsum(has.sum(axis=1))]).astype(np.int64)
    return colptr, rows[has].astype(np.int64)


# M = N = nx * ny: node r = ix + nx * iy reads itself and its (up to) four neighbours
GRID5_SRC = r"""
struct Grid5 {
    long long nx, ny;
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        const long long ix = r % nx, iy = r / nx;
        const real_t b = X(r);
        const real_t w0 = X(ix > 0 ? r - 1 : r), e0 = X(ix + 1 < nx ? r + 1 : r), s0 = X(iy > 0 ? r - nx : r), n0 = X(iy + 1 < ny ? r + nx : r);
        const real_t w = ix > 0 ? w0 : 0.0, e = ix + 1 < nx ? e0 : 0.0, s = iy > 0 ? s0 : 0.0, nn = iy + 1 < ny ? n0 : 0.0;
        const real_t d = 4 * b - (((w + e) + s) + nn);
        return (b * b + 0.25 * b * b * b) + 0.05 * d * d;
    }
};
"""


def phi_grid5(nx, ny):
    def phi(r, get):
        ix, iy = r % nx, r // nx
        b = get(r)
        w0, e0 = get(np.where(ix > 0, r - 1, r)), get(np.where(ix + 1 < nx, r + 1, r))
        s0, n0 = get(np.where(iy > 0, r - nx, r)), get(np.where(iy + 1 < ny, r + nx, r))
        w, e = np.where(ix > 0, w0, 0.0), np.where(ix + 1 < nx, e0, 0.0)
        s, nn = np.where(iy > 0, s0, 0.0), np.where(iy + 1 < ny, n0, 0.0)
        d = 4.0 * b - (((w + e) + s) + nn)
        return (b * b + 0.25 * b * b * b) + 0.05 * d * d
    return phi


# M != N: row r reads 1..6 coordinates of a fixed hash among the first ncols (the last columns: never read)
RANDROWS_SRC = r"""
struct RandRows {
    long long ncols;
    __device__ long long col(long long r, long long t) const { return (r * 131 + t * 977 + (r % 7) * t * 31) % ncols; }
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        const long long L = 1 + (r * 5 + 3) % 6;
        real_t s = 0;
        for (long long t = 0; t < L; ++t) {
            const real_t a = X(col(r, t)), b = X(col(r, t + 1 < L ? t + 1 : 0));
            s = s + (a * b + 0.5 * a * a) / (2.0 + b * b);
        }
        return s;
    }
};
"""


def _rand_col(r, t, ncols):
    return (r * 131 + t * 977 + (r % 7) * t * 31) % ncols


def phi_randrows(ncols):
    def phi(r, get):
        r = np.asarray(r, np.int64)
        L = 1 + (r * 5 + 3) % 6
        s = np.zeros(r.shape)
        with np.errstate(all="ignore"):
            for t in range(6):
                on = t < L
                t1 = np.where(t + 1 < L, t + 1, 0)
                a, b = get(np.where(on, _rand_col(r, t, ncols), 0)), get(np.where(on, _rand_col(r, t1, ncols), 0))
                s = np.where(on, s + (a * b + 0.5 * a * a) / (2.0 + b * b), s)
        return s
    return phi


def randrows_support(M, N, ncols):
    """S of RandRows, 0-based CSC"""
    cols = [[] for _ in range(N)]
    for r in range(M):
        L = 1 + (r * 5 + 3) % 6
        for c in sorted({_rand_col(r, t, ncols) for t in range(L)}):
            cols[c].append(r)
    colptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    return colptr, np.array([r for c in cols for r in c], np.int64)


# any support, given as DATA: the functor holds S by rows (row_ptr int64, row_col int32 ascending per row, both on the device); row r
# with columns c_0 < ... < c_{L-1} is the left-to-right sum over t of (a b + 0.5 a a) / (2 + b b), a = X(c_t), b = X(c_{(t+1) mod L});
# L = 0: +0.0.  Only + - * /, so numpy restates it exactly.  params = the two pointers; one source, one compilation for every pattern.
LISTROWS_SRC = r"""
struct ListRows {
    const long long *rp;
    const int *rc;
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        const long long q0 = rp[r], L = rp[r + 1] - q0;
        real_t s = 0;
        for (long long t = 0; t < L; ++t) {
            const real_t a = X(rc[q0 + t]), b = X(rc[q0 + (t + 1 < L ? t + 1 : 0)]);
            s = s + (a * b + 0.5 * a * a) / (2.0 + b * b);
        }
        return s;
    }
};
"""


def rows_of(M, N, colptr, rowval):
    """S by rows, (row_ptr int64 [M + 1], row_col int32, columns ascending per row), from 0-based CSC with unique rows per column"""
    colptr, rowval = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64)
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    order = np.lexsort((cols, rowval))
    rp = np.zeros(M + 1, np.int64)
    np.add.at(rp, rowval + 1, 1)
    return np.cumsum(rp), cols[order].astype(np.int32)


def phi_listrows(row_ptr, row_col):
    rp, rc = np.asarray(row_ptr, np.int64), np.asarray(row_col, np.int64)

    def phi(r, get):
        r = np.asarray(r, np.int64)
        q0 = rp[r]
        L = rp[r + 1] - q0
        s = np.zeros(r.shape)
        with np.errstate(all="ignore"):
            for t in range(int(L.max()) if r.size else 0):
                on = t < L
                t1 = np.where(t + 1 < L, t + 1, 0)
                a, b = get(rc[np.where(on, q0 + t, 0)]), get(rc[np.where(on, q0 + t1, 0)])
                s = np.where(on, s + (a * b + 0.5 * a * a) / (2.0 + b * b), s)
        return s
    return phi


# the reference's own test objectives (tests/golden/hessian_known_answers.json): per = 0: M = 1, f itself; per = 1: M = n, one
# coordinate per row (diagonal S)
KNOWN_SRC = r"""
struct Known {
    long long kind, n, per;
    template <class P> __device__ real_t term(long long k, const P &X) const
    {
        const real_t v = X(k);
        if (kind == 0) return k == 0 ? sin(v) : cos(v);          // sin(x[1]) + cos(x[2])
        if (kind == 3) return k == 0 ? v * v : 2 * (v * v);      // x[1]^2 + 2 * x[2]^2
        return v * v;                                            // abs2 (kind 1: the sum halved)
    }
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        real_t s;
        if (per) s = term(r, X);
        else {
            s = term(0, X);
            for (long long k = 1; k < n; ++k) s = s + term(k, X);
        }
        return kind == 1 ? s / 2 : s;
    }
};
"""
KNOWN_KINDS = {"sin_cos": 0, "half_sum_abs2": 1, "sum_abs2": 2, "quadratic": 3}
