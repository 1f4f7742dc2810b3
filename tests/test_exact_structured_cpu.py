"""The cases of tests/exact_structured_cases.py evaluated with the exact host model ALONE (no GPU, no library): the two new layouts against
the layout classes' own enumeration, the finite share of every case, the sides of fd_div_shared's fall-back rule the band cases populate,
the edges the operand families reach, and -- the point of a model -- that deliberately WRONG models are told apart by named cases."""
import collections

import numpy as np
import pytest

import exact_model as X
import exact_structured_cases as S
from finitediff_jl_amd import patterns as P

BY_ID = {c["id"]: c for c in S.CASES}


@pytest.fixture(scope="module")
def answers():
    """One model evaluation per distinct answer (the route does not enter it), shared and left unchanged."""
    out = {}
    for c in S.CASES:
        k = S.model_key(c)
        if k not in out:
            out[k] = S.model(c)
            out[k][0].setflags(write=False)
    return out


def _unique_D(C, M, dtype=np.float64):
    return (1.0 + np.arange(max(C, 1))[:, None] * 1000.0 + np.arange(M)[None, :]).astype(dtype)      # D[c][r] names (c, r)


@pytest.mark.parametrize("bs,bl,bu", [((3, 1, 4, 2), 1, 1), ((2, 2, 2), 1, 1), ((3, 2, 4, 1, 2), 2, 0), ((2, 3, 1), 0, 1), ((5,), 1, 1)])
def test_to_blockbanded_is_the_layouts_own_enumeration(bs, bl, bu):
    lay = P.BlockBandedLayout(np.array(bs), bl, bu)
    colors = lay.colors()
    colors[1 % lay.N] = 0                                    # a column without a colour
    c0, C = colors - 1, int(colors.max())
    D = _unique_D(C, lay.N)
    data = X.to_blockbanded(D, c0, lay)
    dense = lay.to_dense(data)
    off = np.concatenate([[0], np.cumsum(bs)])
    blk = np.repeat(np.arange(len(bs)), bs)
    seen = 0
    for r in range(lay.N):
        for j in range(lay.N):
            inband = blk[r] - blk[j] <= bl and blk[j] - blk[r] <= bu
            want = D[c0[j], r] if (inband and c0[j] >= 0) else 0.0
            assert dense[r, j] == want, (r, j)
            if inband:
                assert data[lay.index_of(np.array([r]), np.array([j]))[0]] == want
                seen += 1
    assert seen == lay.data_len and off[-1] == lay.N       # every element of data belongs to exactly one in-band entry


@pytest.mark.parametrize("bs,lam,mu", [((3, 3, 3), 1, 1), ((4, 2, 5, 1), 2, 2), ((2, 2), 3, 1), ((3,), 1, 1), ((3, 4), 0, 2)])
def test_to_bandedblockbanded_is_the_layouts_own_enumeration(bs, lam, mu):
    lay = P.BandedBlockBandedLayout(np.array(bs), 1, 1, lam, mu)
    colors = lay.colors()
    colors[lay.N // 2] = 0
    c0, C = colors - 1, int(colors.max())
    D = _unique_D(C, lay.N)
    data = X.to_bandedblockbanded(D, c0, lay)
    rows, cols, dest = lay.entries()
    assert np.unique(dest).size == dest.size
    want = np.where(c0[cols - 1] >= 0, D[np.maximum(c0[cols - 1], 0), rows - 1], 0.0)
    assert np.array_equal(data[dest], want)
    rest = np.ones(lay.data_len, bool)
    rest[dest] = False
    assert rest.any() and not data[rest].any() and not np.signbit(data[rest]).any()      # everything else: an exact +0.0
    # the mutation knobs: a slot outside its block left as it was (NaN) touches only slots no entry owns; one row off moves entries
    nan = X.to_bandedblockbanded(D, c0, lay, outside=np.nan)
    assert np.array_equal(nan[dest], want) and np.isnan(nan[rest]).any()
    assert not np.array_equal(X.to_bandedblockbanded(D, c0, lay, row_shift=1)[dest], want)


def test_every_case_keeps_most_values_finite(answers):
    kept, worst = collections.Counter(), {}
    for c in S.CASES:
        out = answers[S.model_key(c)][0]
        share = float(np.isfinite(out).mean()) if out.size else 1.0
        assert share >= S.MIN_FINITE, (c["id"], share)
        kept[c["layout"]] += 1
        worst[c["layout"]] = min(worst.get(c["layout"], 1.0), share)
    print("\nstructured cases kept per layout:", dict(kept), "worst finite share:", {k: round(v, 4) for k, v in worst.items()})
    print("families left out:", S.LEFT_OUT)
    assert set(kept) == {"band", "bandcsc", "blocks", "bbb"}


def test_band_cases_populate_both_sides_of_the_division_rule():
    """fd_band_store_cols divides with the three-argument fd_div_shared: the Markstein product iff |a y| and |a| lie in [2^-900, 2^900].
    Which side every band case of the mid-size shape populates; both sides must be reached, each by a named family."""
    sides = {}
    for c in S.CASES:
        if c["layout"] == "band" and c["route"] == "store" and c["dtype"] == "f64" and c["shape"] == S.MID["band"] and c["variant"] is None \
                and c["fdtype"] != "complex" and c["fixture"] == "band":
            sides[c["id"]] = (c["family"], S.div_sides(c))
    fam = collections.defaultdict(lambda: [0, 0])
    for _id, (f, d) in sides.items():
        fam[f][0] += d["rule3"][0]
        fam[f][1] += d["rule3"][1]
    print("\nband cases, (Markstein product, true division) per family:", dict(fam))
    assert fam["ordinary"][0] > 0 and fam["ordinary"][1] == 0
    assert fam["num_2m900"][1] > 0                       # numerators below 2^-900, non-zero
    assert fam["eps_2m100_in"][1] > 0 or fam["eps_2m100_out"][1] > 0 or fam["subnormal"][1] > 0
    assert fam["cancel"][1] > 0                          # zero numerators
    for f in S.DIV_FAMILIES:
        assert sum(fam[f]) > 0, f
    d = [v[1] for v in sides.values() if v[0] == "num_2p800"][0]
    assert d["a"][1] > 2.0 ** 800                        # numerators above 2^800 ...
    d = [v[1] for v in sides.values() if v[0] == "num_2m900"][0]
    assert 0 < d["a"][1] < 2.0 ** -900 or d["rule3"][1] > 0


def test_each_family_reaches_its_edge():
    for layout in ("band", "blocks", "bbb"):
        pick = lambda fam, **kw: next(c for c in S.CASES if c["layout"] == layout and c["family"] == fam and c["dtype"] == "f64"
                                      and all(c[k] == v for k, v in kw.items()))
        x = S.inputs(pick("signed_zeros"))["x"]
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        inp = S.inputs(pick("nan_inf"))
        x = inp["x"]
        assert np.isnan(x).sum() == 1 and (x == np.inf).sum() == 1 and (x == -np.inf).sum() == 1
        assert np.unique(inp["c0"][~np.isfinite(x)]).size == (3 if layout == "blocks" else 1)
        x = S.inputs(pick("subnormal"))["x"]
        assert (np.abs(x[x != 0]) < np.finfo(np.float64).tiny).all()
        for fam, want in (("eps_2p100_in", 2.0 ** 100), ("eps_2m100_in", 2.0 ** -100)):
            c = pick(fam, fdtype="central")
            inp = S.inputs(c)
            eps, _ = X.epsilons(inp["x"], inp["c0"], inp["C"], "central", relstep=inp["rel"], absstep=inp["ab"])
            assert (eps == want).all()
        for fam, cmp in (("eps_2p100_out", lambda e: e > 2.0 ** 100), ("eps_2m100_out", lambda e: e < 2.0 ** -100)):
            inp = S.inputs(pick(fam, fdtype="central"))
            eps, _ = X.epsilons(inp["x"], inp["c0"], inp["C"], "central", relstep=inp["rel"], absstep=inp["ab"])
            assert cmp(eps).all()
        inp = S.inputs(pick("cancel", fdtype="forward"))
        eps, _ = X.epsilons(inp["x"], inp["c0"], inp["C"], "forward", relstep=inp["rel"], absstep=inp["ab"])
        big = np.abs(inp["x"]) >= 1e30
        assert big.any() and (inp["x"][big] + eps[inp["c0"][big]] == inp["x"][big]).all()          # x + eps is absorbed
        c = pick("ordinary", variant="f_in")
        inp = S.inputs(c)
        assert inp["f_in"] is not None and 0 < (inp["f_in"] != inp["f"](inp["x"])).sum() < inp["N"]
        inp = S.inputs(pick("ordinary", variant="steps", fdtype="central"))
        assert inp["ab"] == 0.0 and inp["rel"] == 1e-3


# the mutations and the named cases that must see each (a mutation a layout cannot express is not listed for it)
SEEN_BY = {
    "plain_fx": ["band-2x2x1025-band-own-handover-forward-f64-ordinary-f_in", "blocks-9x32-blockrat-own-store-forward-f64-ordinary-f_in",
                 "bbb-23x17x3-grid-own-store-forward-f64-ordinary-f_in", "bbb-40x30x1-lap5_nl-own-store-forward-f64-ordinary-f_in"],
    "no_plus_zero": ["band-2x2x513-band_sign-own2-store-forward-f64-signed_zeros", "band-2x2x513-band_sign-own2-handover-central-f64-signed_zeros",
                     "blocks-5x7-block_sign-own-store-forward-f64-signed_zeros", "blocks-ragged-block_sign-own-handover-forwardm-f64-signed_zeros"],
    "unwritten_slot": ["band-2x2x513-band-own4-store-forward-f64-signed_zeros", "bbb-4x4x3-grid-own-store-forwardm-f64-signed_zeros",
                       "bbb-2x1x1-grid-own-handover-forwardm-f64-ordinary"],
    "dir_on_quotient": ["band-2x2x1025-band-own1-store-forwardm-f64-ordinary", "blocks-9x32-blockrat-own-store-forwardm-f64-ordinary",
                        "bbb-23x17x3-grid-own-handover-forwardm-f64-ordinary"],
    "neighbour_eps": ["band-2x2x1025-band-own1-store-forward-f64-ordinary", "blocks-9x32-blockrat-own-handover-central-f64-ordinary",
                      "bbb-23x17x3-grid-own-store-central-f64-ordinary"],
    "row_off": ["band-3x3x129-band-own1-handover-forwardm-f64-ordinary", "bbb-5x3x2-grid-own-store-central-f64-signed_zeros"],
}


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_a_named_case_sees_every_model_mutation(mutation):
    """plain_fx: f(x) instead of the caller's f_in; no_plus_zero: x_i instead of x_i + 0.0 on the plus side (seen only by a functor that
    sees the sign of a zero, at a -0.0 coordinate: the sign-sensitive fixtures -- BandF, BlockRat at these operands and GridNL never see
    it, tests/test_gpu_exact_structured.py says why); unwritten_slot: a slot outside the matrix / its block left as it was;
    dir_on_quotient: the step of dir = +1 with the quotient multiplied by dir; neighbour_eps: the step of the colour before;
    row_off: every slot takes the row below its own.  unwritten_slot and row_off are statements about a layout with implicit rows:
    BandedMatrix and BBB data (block-banded columns store whole block rows: there is no slot outside, and a row off is a wrong
    destination, which the unique-value layout test above pins)."""
    for cid in SEEN_BY[mutation]:
        assert cid in BY_ID, cid
        c = BY_ID[cid]
        inp = S.inputs(c)
        good, bad = S.model(c, inp=inp)[0], S.model(c, mutation, inp=inp)
        assert bad is not None, (mutation, cid)
        differs = ~X.same_bits(good, bad[0])
        assert differs.any(), (mutation, cid)


def test_the_two_forms_of_an_unperturbed_zero():
    """dir = -1: the model's x_i + copysign(0, eps) keeps a -0.0 coordinate, the library's x_i + (+0.0) does not.  The sign-sensitive
    fixtures tell the two apart (their dir = -1 cases are compared with the library's form); every other dir = -1 case at signed zeros
    gives the SAME stored bits under both, so those are compared with the model itself."""
    n_same = n_diff = 0
    for c in S.CASES:
        if not (c["family"] == "signed_zeros" and c["dir"] < 0 and c["fdtype"] == "forward" and c["route"] == "handover"):
            continue
        inp = S.inputs(c)
        eps, _ = X.epsilons(inp["x"], inp["c0"], inp["C"], "forward", relstep=inp["rel"], absstep=inp["ab"], dir=-1.0, dtype=inp["dtype"])
        lay = S.layout_fn(c, inp)
        a, b = (lay(X.colour_values(inp["f"], inp["x"], inp["c0"], inp["C"], eps, "forward", f_in=inp["f_in"], zero=z)) for z in ("model", "library"))
        if S.library_zero(c):
            assert not X.same_bits(a, b).all(), c["id"]
            n_diff += 1
        else:
            assert X.same_bits(a, b).all(), c["id"]
            n_same += 1
    assert n_same > 0 and n_diff > 0
