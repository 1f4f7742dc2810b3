"""Exact host model of the finite-difference JVP (csrc/fdjac_jvp.hip: fd_jvp, fd_jvp_async; the lazy JVP kernels of
csrc/fdjac_f_jvp.hip), restated in numpy independently of the library, one IEEE operation at a time.  Test infrastructure only.

  dot(x, v)    Float64 products of the elements cast to Float64, summed in one of THREE defined orders:
                 dot_small    k_jvp_small: 1024 threads of one workgroup, thread t takes t, t + 1024, ...; the 64-lane tree
                              v += shfl_down(v, off), off = 32 .. 1 (lane 0's value); the 16 waves left to right
                 dot_large    k_dot_partial<false> (scalar) / <true> (paired) on g = balanced_grid(ceil(N / 256), 8 num_cus) workgroups
                              of 256 threads -- the grid, and with it the order, depends on the device's CU count -- then k_jvp_eps:
                              256 threads stride over the g partials, tree, four waves
               every accumulator starts from +0.0 and takes its terms in ascending index order
  epsilon      T(t) FIRST, then sqrt(abs(.)) in the element type T, T(relstep) * abs(.), Julia's NaN-propagating max against T(absstep),
               * T(dir) in the forward rule only (src/epsilons.jl:26-29, 50-53; src/jvp.jl:253-254)
  jvp          ev = T(eps) * v (a product of its own, never fused into the sum); forward (f(x + ev) - base) / eps with base = f(x) or
               the caller's f_in as it is given; central (f(x + ev) - f(x - ev)) / (T(2) eps), f_in ignored (src/jvp.jl:255-269)

Every route of the library (fused small launch, materialised points paired / scalar, lazy values, lazy quotient, declined launcher,
host staging, async) promises these bits; only the summation order of the dot product differs between them."""
import numpy as np

import exact_model as X

F64 = np.float64
SMALL_N = 16384            # kSmallN: the fused single-workgroup launch up to this N
BLOCK, SMALL_BLOCK = 256, 1024
U = 2.0 ** -53


def balanced_grid(tiles, cap):
    """csrc/fdjac_kernels.hip, balanced_grid: at most `cap` workgroups, the tiles divided into whole rounds."""
    tiles, cap = max(int(tiles), 1), max(int(cap), 1)
    rounds = (tiles + cap - 1) // cap
    return (tiles + rounds - 1) // rounds


def grid(n, num_cus):
    return balanced_grid((n + BLOCK - 1) // BLOCK, 8 * int(num_cus))


def _products(x, v):
    x, v = np.asarray(x), np.asarray(v)
    assert x.dtype == v.dtype and x.ndim == 1 and x.shape == v.shape, (x.dtype, v.dtype, x.shape, v.shape)
    return x.astype(F64) * v.astype(F64)


def _strided(acc, terms):
    """acc[t] += terms[t], terms[t + T], ... in ascending order for the T = acc.size threads (a thread without a term keeps its sum)."""
    T, n = acc.size, terms.size
    for r in range((n + T - 1) // T):
        part = terms[r * T:(r + 1) * T]
        acc[:part.size] = acc[:part.size] + part
    return acc


def _tree_waves(acc):
    """(..., W * 64) thread sums -> (...): per wave v += shfl_down(v, off) for off = 32 .. 1 (lane 0's value), then the waves from a
    +0.0 left to right."""
    w = acc.reshape(acc.shape[:-1] + (acc.shape[-1] // 64, 64))
    for off in (32, 16, 8, 4, 2, 1):
        w = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    t = np.zeros(w.shape[:-1])
    for i in range(w.shape[-1]):
        t = t + w[..., i]
    return t


def dot_small(x, v):
    """k_jvp_small's dot(x, v) as a Float64."""
    with np.errstate(all="ignore"):
        acc = _strided(np.zeros(SMALL_BLOCK), _products(x, v))
        return F64(_tree_waves(acc))


def dot_large(x, v, paired, num_cus):
    """k_dot_partial<paired> on the balanced grid, then k_jvp_eps's sum of the partials, as a Float64."""
    with np.errstate(all="ignore"):
        p = _products(x, v)
        n = p.size
        g = grid(n, num_cus)
        acc = np.zeros(g * BLOCK)
        if paired:
            n2 = n >> 1
            T = acc.size
            for r in range((n2 + T - 1) // T):            # a thread's pair: element .x, then element .y
                lo, hi = r * T, min((r + 1) * T, n2)
                acc[:hi - lo] = (acc[:hi - lo] + p[2 * lo:2 * hi:2]) + p[2 * lo + 1:2 * hi:2]
            if n & 1:                                      # the tail: thread 0 of block 0, after its own pairs
                acc[0] = acc[0] + p[n - 1]
        else:
            acc = _strided(acc, p)
        partial = _tree_waves(acc.reshape(g, BLOCK))       # one partial per workgroup
        return F64(_tree_waves(_strided(np.zeros(BLOCK), partial)))


def dot(x, v, order, num_cus=256):
    """order: "small" | "scalar" | "paired"."""
    if order == "small":
        return dot_small(x, v)
    return dot_large(x, v, order == "paired", num_cus)


def chain_length(order, n, num_cus=256):
    """The longest chain of additions a term goes through in that order (the error bound of tests/test_jvp_model_cpu.py)."""
    if order == "small":
        return (n + SMALL_BLOCK - 1) // SMALL_BLOCK + 6 + SMALL_BLOCK // 64
    g = grid(n, num_cus)
    T = g * BLOCK
    own = 2 * (((n >> 1) + T - 1) // T) + (n & 1) if order == "paired" else (n + T - 1) // T
    return own + 6 + BLOCK // 64 + (g + BLOCK - 1) // BLOCK + 6 + BLOCK // 64


def steps(fdtype, relstep=None, absstep=None, dtype=F64):
    """(relstep, absstep) as jvp_enqueue applies its defaults: relstep not > 0 -> sqrt / cbrt of the element type's epsilon, computed
    in the element type; absstep < 0 -> relstep; absstep = 0 stays 0."""
    if relstep is None or not (relstep > 0):
        relstep = X.default_relstep(fdtype, dtype)
    if absstep is None or absstep < 0:
        absstep = relstep
    return float(relstep), float(absstep)


def epsilon(t, fdtype, relstep=None, absstep=None, dir=1.0, dtype=F64, max_=X.jl_max, dir_in_central=False):
    """The step size from the Float64 dot product t, in the element type.  (max_ / dir_in_central: the perturbed models of the CPU
    suite.)"""
    T = np.dtype(dtype).type
    relstep, absstep = steps(fdtype, relstep, absstep, dtype)
    with np.errstate(all="ignore"):
        tmp = np.sqrt(np.abs(T(t)))
        a = T(relstep) * np.abs(tmp)
        e = max_(a, T(absstep))
        if fdtype == "forward" or dir_in_central:
            e = e * T(dir)
    return T(e)


def jvp(f, x, v, eps, fdtype, f_in=None):
    """The M values of the product at the step size eps."""
    x, v = np.asarray(x), np.asarray(v)
    T = x.dtype.type
    assert v.dtype == x.dtype
    with np.errstate(all="ignore"):
        e = T(eps)
        ev = e * v
        if fdtype == "forward":
            base = f(x) if f_in is None else np.asarray(f_in, dtype=x.dtype)
            return (f(x + ev) - base) / e
        return (f(x + ev) - f(x - ev)) / (T(2) * e)
