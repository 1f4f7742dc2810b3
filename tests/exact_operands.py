"""The operand families of the exact-model tests (tests/test_gpu_exact_model.py, tests/exact_general.py): pure numpy, so that the CPU
suite can build every GPU case's inputs without the library or torch.  Test infrastructure only."""
import numpy as np


def operands(case, N, C, dtype, seed):
    """(x, relstep, absstep): the operand families of the matrix (colour k of column j is (j + shift) mod C, or the grid's)."""
    rng = np.random.default_rng(seed)
    x = rng.random(N) - 0.25
    rel, ab = None, None
    pick = lambda k: np.arange(N) % max(C, 1) == k % max(C, 1)
    if case == "signed_zeros":
        x[rng.random(N) < 0.5] = -0.0
        x[rng.random(N) < 0.3] = 0.0
    elif case == "cancel":                       # x + eps absorbed in a colour: zero numerators
        x[pick(1)] = 1e30 * (1 + rng.random(int(pick(1).sum())))
        rel, ab = 1e-30, 1e-30
    elif case == "eps_2p100_in":
        rel, ab = 1e-300, 2.0 ** 100
    elif case == "eps_2p100_out":
        rel, ab = 1e-300, 2.0 ** 100 * (1 + 2.0 ** -40)
    elif case == "eps_2m100_in":
        rel, ab = 1e-300, 2.0 ** -100
    elif case == "eps_2m100_out":
        rel, ab = 1e-300, 2.0 ** -100 * (1 - 2.0 ** -40)
    elif case == "num_2p800":
        x = x * 1e240                            # numerators ~2^800, and a sum of squares that overflows (scaled norm)
    elif case == "huge_range":
        k = np.nonzero(pick(0))[0]
        x[k] = 10.0 ** rng.uniform(154, 300, k.size) * np.where(rng.random(k.size) < 0.5, -1, 1)
    elif case == "tiny_1e-200":
        x = x * 1e-200
        ab = 0.0
    elif case == "subnormal":
        x = 5e-324 * rng.integers(-1000, 1000, N).astype(np.float64)
        ab = 0.0
    elif case == "nan_inf":
        if N >= 3 * C:
            x[C * (N // (3 * C)) + 0] = np.nan
            x[C * (N // (3 * C)) + 1 + C] = np.inf
            x[C * (2 * N // (3 * C)) + 2 + C] = -np.inf
    elif case == "f32_huge":
        x[pick(0)] = 3.0e38
        x[pick(2)] = -3.3e38
    elif case == "f32_subnormal":
        x = (1.4e-45 * rng.integers(-1000, 1000, N)).astype(np.float64)
        ab = 0.0
    return x.astype(dtype), rel, ab
