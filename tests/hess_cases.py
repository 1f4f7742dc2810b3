"""The cases of the objective Hessian / gradient edge tests (tests/test_gpu_hessian_edges.py on the device, tests/test_hessian_cpu.py on
the host): support patterns at the edges of the plan builder (csrc/fdjac_hessian.hip, build_pattern) and of the three kernels' index
spaces (256 lanes per workgroup, grids rounded up to 8 workgroups), and operand families at the edges of the step rule and the
quotients.  Pure numpy, so that the CPU suite evaluates the model on every case without the library or torch.  Every objective is
hess_model.phi_listrows on the pattern's rows.  Test infrastructure only."""
import functools

import numpy as np

import hess_model as hm

MIN_FINITE = 0.9                  # the least share of finite model values in any case (the cap of tests/exact_general.py)
_BUDGET = 0.08                    # the share of values a family's special columns may make non-finite, counted from the pattern alone


# ---- support patterns: (M, N, colptr, rowval), 0-based, rows ascending and unique per column -------------------------------------------
def _from_rows(M, N, rows):
    """CSC of the support whose row r reads the columns rows[r]"""
    r = np.repeat(np.arange(M, dtype=np.int64), [len(c) for c in rows])
    c = np.array([k for cs in rows for k in cs], np.int64)
    key = np.unique(c * M + r)
    c, r = key // M, key % M
    cp = np.zeros(N + 1, np.int64)
    np.add.at(cp, c + 1, 1)
    return M, N, np.cumsum(cp), r


def _chain_rows(n):
    return [[k for k in (r - 1, r, r + 1) if 0 <= k < n] for r in range(n)]


def _random_rows(M, N, lo, hi, seed, window=None, skip_cols=(), skip_rows=()):
    rng = np.random.default_rng(seed)
    ok = np.setdiff1d(np.arange(N), np.asarray(skip_cols, np.int64))
    rows = []
    for r in range(M):
        L = int(rng.integers(lo, hi + 1))
        if r in skip_rows or L == 0:
            rows.append([])
            continue
        cand = ok
        if window is not None:
            c0 = r * N // M
            cand = ok[(ok >= c0 - window) & (ok <= c0 + window)]
        rows.append(sorted(rng.choice(cand, size=min(L, cand.size), replace=False).tolist()))
    return rows


def _gaps():
    N = 257
    unread = sorted(set(range(0, N, 5)) | {N - 1})         # about every fifth column, the first and the last
    return _from_rows(N, N, _random_rows(N, N, 1, 4, 21, window=8, skip_cols=unread))


def _dense_row_trim(N):
    """one coordinate per row, and one row over the first 63 columns: N + 1953 upper entries"""
    return _from_rows(N + 1, N, [[r] for r in range(N)] + [list(range(63))])


def _dense_col():
    M, N = 513, 40
    rows = _random_rows(M, N, 1, 3, 22, skip_cols=[17])
    return _from_rows(M, N, [sorted(set(c) | {17}) for c in rows])


PATTERNS = {
    "tiny_1": lambda: _from_rows(1, 1, [[0]]),
    "tiny_2_dense": lambda: _from_rows(2, 2, [[0, 1], [1]]),
    "tiny_2_diag": lambda: _from_rows(2, 2, [[0], [1]]),
    "tiny_3_dense": lambda: _from_rows(2, 3, [[0, 1, 2], [2]]),
    "tiny_3_diag": lambda: _from_rows(3, 3, [[0], [1], [2]]),
    "empty": lambda: _from_rows(3, 5, [[], [], []]),
    "m1_sparse": lambda: _from_rows(1, 9, [[0, 2, 3, 6, 8]]),
    "gaps": _gaps,
    "empty_rows": lambda: _from_rows(300, 200, _random_rows(300, 200, 1, 5, 23, window=12, skip_rows=set(range(1, 300, 3)))),
    "dense_row": lambda: _from_rows(71, 70, _chain_rows(70) + [list(range(70))]),
    "dense_row_2047": lambda: _dense_row_trim(94),
    "dense_row_2048": lambda: _dense_row_trim(95),
    "dense_row_2049": lambda: _dense_row_trim(96),
    "dense_col": _dense_col,
    "ragged_wide": lambda: _from_rows(97, 300, _random_rows(97, 300, 0, 9, 24)),
    "ragged_tall": lambda: _from_rows(600, 130, _random_rows(600, 130, 0, 9, 25)),
    "diag": lambda: _from_rows(260, 260, [[r] for r in range(260)]),
}
CHAIN_SIZES = (255, 256, 257, 2047, 2048, 2049, 2305)
for _n in CHAIN_SIZES:
    PATTERNS["chain_%d" % _n] = functools.partial(lambda n: _from_rows(n, n, _chain_rows(n)), _n)
PATTERN_NAMES = tuple(PATTERNS)


@functools.lru_cache(maxsize=None)
def pattern(name):
    M, N, cp, rv = PATTERNS[name]()
    for a in (cp, rv):
        a.setflags(write=False)
    return M, N, cp, rv


def dup_unsorted(name="ragged_wide", seed=31):
    """the pattern with every column's rowval shuffled and some rows repeated: (colptr, rowval), 0-based -- the same support"""
    M, N, cp, rv = pattern(name)
    rng = np.random.default_rng(seed)
    out, ptr = [], [0]
    for j in range(N):
        rows = np.array(rv[cp[j]:cp[j + 1]])
        if rows.size:
            rows = np.concatenate([rows, rng.choice(rows, size=int(rng.integers(0, 3)))])
        out.extend(rng.permutation(rows).tolist())
        ptr.append(len(out))
    return np.array(ptr, np.int64), np.array(out, np.int64)


@functools.lru_cache(maxsize=None)
def triples(name):
    M, N, cp, rv = pattern(name)
    return hm._row_triples(M, N, cp, rv)


def plan_counts(name):
    """what the plan must report, counted from the model's triples: upper entries, nnz of P, length of the row lists, half-bandwidth"""
    r, i, j = triples(name)
    if r.size == 0:
        return dict(upper=0, nnz=0, list_len=0, bandwidth=0)
    ent = np.unique(j * pattern(name)[1] + i).size
    return dict(upper=ent, nnz=2 * ent - np.unique(i[i == j]).size, list_len=int(r.size), bandwidth=int((j - i).max()))


# ---- operand families ----------------------------------------------------------------------------------------------------------------
FAMILIES = ("ordinary", "signed_zeros", "tie", "neg_dir", "absstep0", "absorbed", "huge", "tiny", "subnormal", "inf_nan", "custom_steps")
# how a family's special columns can make values non-finite: not at all; only the entries / components OF a special column (a zero
# or overflowing step); or everything summed over a row that reads one (a NaN or Inf coordinate)
_REACH = {"absstep0": "local", "huge": "local", "tiny": "local", "subnormal": "local", "inf_nan": "rows"}
_WANT = {"signed_zeros": 0.3, "tie": 0.3, "absorbed": 0.1, "absstep0": 0.04, "huge": 0.04, "tiny": 0.04, "subnormal": 0.04, "inf_nan": 3}


def _candidates(name):
    """special columns in the order they are tried: the column of the longest list, a read column beside an unread one, an unread
    column, the first and the last column, then the rest spread evenly"""
    M, N, cp, rv = pattern(name)
    cnt = np.diff(cp)
    first = [int(np.argmax(cnt))]
    unread = np.flatnonzero(cnt == 0)
    beside = [j for j in range(N) if cnt[j] and ((j > 0 and cnt[j - 1] == 0) or (j + 1 < N and cnt[j + 1] == 0))]
    first += beside[len(beside) // 2:len(beside) // 2 + 1] + unread[unread.size // 2:unread.size // 2 + 1].tolist() + [0, N - 1]
    rest = np.random.default_rng(N).permutation(N).tolist()
    out = []
    for c in first + rest:
        if c not in out:
            out.append(c)
    return out


def _spoilt(name, cols, reach):
    """the share of Hessian entries and of gradient components that special columns `cols` can make non-finite"""
    M, N, cp, rv = pattern(name)
    r, i, j = triples(name)
    sel = np.zeros(N, bool)
    sel[list(cols)] = True
    if reach == "rows":
        bad_row = np.zeros(M, bool)
        bad_row[rv[np.repeat(sel, np.diff(cp))]] = True
        bad_t = bad_row[r] if r.size else np.zeros(0, bool)
        g_bad = sel.copy()
        g_bad[np.repeat(np.arange(N), np.diff(cp))[bad_row[rv]]] = True
    else:
        bad_t = sel[i] | sel[j] if r.size else np.zeros(0, bool)
        g_bad = sel
    key = j * N + i
    nent = max(np.unique(key).size, 1)
    return max(np.unique(key[bad_t]).size / nent, g_bad.mean())


@functools.lru_cache(maxsize=None)
def special_columns(name, family):
    """the family's special columns on this pattern, or None where the pattern cannot hold the family within the cap"""
    N = pattern(name)[1]
    want = _WANT.get(family)
    if want is None:
        return ()
    k = want if isinstance(want, int) else max(1, int(round(want * N)))
    reach = _REACH.get(family)
    got = []
    for c in _candidates(name):
        if len(got) == k:
            break
        if reach is None or _spoilt(name, got + [c], reach) <= _BUDGET:
            got.append(c)
    need = k if isinstance(want, int) else 1
    return tuple(got) if len(got) >= need else None


def operands(name, family, seed=0):
    """x and the keywords of the calls: dict(x, hess=(relstep, absstep), grad=(relstep, absstep), dirs of the forward gradient) -- None:
    the default.  neg_dir is negative x (with dir = -1 the forward point moves further out)."""
    M, N, cp, rv = pattern(name)
    rng = np.random.default_rng([seed, N, FAMILIES.index(family)])
    x = rng.standard_normal(N) * 1.5
    x[np.abs(x) < 1e-3] = 0.5
    cols = np.array(special_columns(name, family), np.int64)
    u = rng.random(cols.size)
    sgn = np.where(rng.random(cols.size) < 0.5, -1.0, 1.0)
    steps = (None, None)
    if family == "signed_zeros":
        x[cols] = np.where(np.arange(cols.size) % 2 == 0, -0.0, 0.0)
    elif family == "tie":                         # relstep |x| == absstep exactly, and one ulp to either side of it
        steps = (2.0 ** -10, 2.0 ** -12)
        x[cols] = sgn * np.array([0.25, np.nextafter(0.25, 1.0), np.nextafter(0.25, 0.0)])[np.arange(cols.size) % 3]
    elif family == "neg_dir":
        x = -np.abs(x)
    elif family == "absstep0":
        steps = (None, 0.0)
        x[cols] = np.where(np.arange(cols.size) % 2 == 0, 0.0, -0.0)
    elif family == "absorbed":                    # the step of a special column is 2^-10 (1 + u) beside |x| >= 2^60: x +- e == x
        steps = (2.0 ** -70, 2.0 ** -12)
        x[cols] = sgn * 2.0 ** 60 * (1 + u)
    elif family == "huge":                        # relstep 4: e_i e_i and (4 e_i) e_j overflow from 2^510 on, and so does phi there
        steps = (4.0, 2.0 ** -12)
        x[cols] = sgn * 2.0 ** np.where(np.arange(cols.size) % 2 == 0, 511 - (np.arange(cols.size) // 2) % 3, rng.integers(400, 510, cols.size))
    elif family == "tiny":                        # e_i e_i and (4 e_i) e_j subnormal, then zero
        steps = (None, 0.0)
        x[cols] = sgn * 2.0 ** -np.linspace(560, 511, cols.size).round()
    elif family == "subnormal":                   # x = k 2^-1074: the step is subnormal (k >= 2^13) or rounds to zero
        steps = (None, 0.0)
        x[cols] = sgn * 5e-324 * 2.0 ** rng.integers(0, 30, cols.size)
    elif family == "inf_nan":
        cnt = np.diff(cp)                         # the NaN on a column no row reads, where there is one: its step is NaN, its gradient 0 / NaN
        x[sorted(cols.tolist(), key=lambda c: cnt[c] != 0)] = [np.nan, np.inf, -np.inf]
    elif family == "custom_steps":
        steps = (1e-3, 1e-6)
    x.setflags(write=False)
    return dict(x=x, hess=steps, grad=steps, dirs=(1.0, -1.0))


def _cases():
    out = []
    for name in PATTERN_NAMES:
        for fam in FAMILIES:
            if name == "empty" and fam not in ("ordinary", "neg_dir", "inf_nan"):
                continue
            if name.startswith("chain_") and name not in ("chain_257", "chain_2049") and fam not in ("ordinary", "neg_dir"):
                continue                          # the chain sizes are about the grids: the families run at one small and one large size
            if name.startswith("dense_row_20") and fam not in ("ordinary", "absstep0"):
                continue
            if special_columns(name, fam) is not None:
                out.append((name, fam))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def model(name, family):
    """the model's values of one case: dict(ij=(i, j), H=upper values in (j, i) order, ("forward", dir) / "central": gradients)"""
    M, N, cp, rv = pattern(name)
    phi = hm.phi_listrows(*hm.rows_of(M, N, cp, rv))
    op = operands(name, family)
    with np.errstate(all="ignore"):               # (overflow, Inf - Inf and 0 / 0 are what some families are for)
        i, j, h = hm.hessian_entries(phi, op["x"], M, N, cp, rv, *op["hess"])
        out = dict(ij=(i, j), H=h)
        for d in op["dirs"]:
            out["forward", d] = hm.gradient(phi, op["x"], M, N, "forward", cp, rv, *op["grad"], dir=d)
        out["central"] = hm.gradient(phi, op["x"], M, N, "central", cp, rv, *op["grad"])
    return out


def second_x(name):
    """another x for the same plan (the plan's scratch is reused between calls)"""
    N = pattern(name)[1]
    return np.random.default_rng(N + 99).standard_normal(N) * 3
