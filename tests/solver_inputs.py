"""The random, strongly diagonally dominant systems of test_gpu_solve.py, test_gpu_bandsolve.py and test_gpu_blocksolve.py, and their
SciPy references -- numpy and SciPy only, so that tests/test_solve_model_cpu.py can measure on the CPU how far these very inputs couple
(a change here is seen there)."""
import numpy as np
import scipy.linalg


def tridiag_system(N, seed, dominance=0.2):
    rng = np.random.default_rng(seed)
    dl, du = rng.random(max(N - 1, 0)) - 0.5, rng.random(max(N - 1, 0)) - 0.5
    d = rng.random(N) - 0.5
    # alpha*I + beta*J strictly diagonally dominant: |alpha + beta d_i| >= |beta|(|dl| + |du|) + dominance
    beta = -0.7
    alpha = 0.7 * (0.5 + 1.0) + dominance + 0.5
    b = rng.random(N) - 0.5
    return dl, d, du, b, alpha, beta


def tridiag_reference(dl, d, du, b, alpha, beta):
    N = d.size
    ab = np.zeros((3, N))
    ab[0, 1:] = beta * du
    ab[1, :] = alpha + beta * d
    ab[2, :-1] = beta * dl
    return scipy.linalg.solve_banded((1, 1), ab, b)


BAND_GAMMA = 0.05                                  # W = I - gamma J: diagonally dominant for |J| ~ 1


def band(N, l, u, rng, dominant=True):
    """BandedMatrix data (l+u+1) x N column-major: data[u + i - j, j] = A[i, j]; slots outside the matrix hold 0."""
    w = l + u + 1
    data = rng.standard_normal((w, N))
    for j in range(N):
        for k in range(w):
            i = j - u + k
            if i < 0 or i >= N:
                data[k, j] = 0.0
    return data


def band_scipy_solve(data, N, l, u, alpha, beta, b):
    ab = beta * data.copy()
    ab[u, :] += alpha          # row u of the (l+u+1) x N band holds the diagonal (scipy's layout is BandedMatrices' layout)
    return scipy.linalg.solve_banded((l, u), ab, b)


def block_system(nb, b, data_len, dtype=np.float64):
    """data, rhs, gamma of test_block_tridiagonal_solve_matches_scipy (data_len: BlockBandedLayout([b] * nb, 1, 1).data_len)."""
    rng = np.random.default_rng(nb + b)
    data = rng.standard_normal(data_len).astype(dtype)
    rhs = rng.standard_normal(nb * b).astype(dtype)
    gamma = 0.2 / (3 * b)                                  # I - gamma J: rows of ~3b entries of size ~1 stay diagonally dominant
    return data, rhs, gamma
