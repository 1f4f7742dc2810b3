"""The table of tests/handover_rows_cases.py and the constants of FD_PLAN_HANDOVER_ROWS, without a GPU: unique ids, a finite share of at
least exact_general.MIN_FINITE for every model key the table adds (the others are shown by tests/test_exact_model.py), and one value
for each new name in include/fdjac.h, finitediff.jl_amd/lib.py and the Julia shim."""
import os
import re

import numpy as np

import exact_general as G
import handover_rows_cases as H
from finitediff_jl_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_ids_are_unique_and_the_table_covers_what_it_names():
    ids = [c["id"] for c in H.CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    pats = {c["pattern"] for c in H.CASES}
    assert pats == {"random_band", "ragged", "wide", "tall", "lap5"} | {"tiny_%d" % n for n in G.TINY}
    assert sum(c["pattern"] == "ragged" and c["colouring"] in ("greedy", "none5") for c in H.CASES) == 1      # ~3000 launches of f: one case
    assert {c["family"] for c in H.CASES} == set(G.FAMILIES)
    for c in H.CASES:
        if c["family"] != "ordinary":
            assert (c["pattern"], c["colouring"], c["dtype"], c["variant"]) == ("random_band", "greedy", "f64", None), c["id"]
    assert {c["pattern"] for c in H.CASES if c["dtype"] == "f32"} == {"random_band", "lap5"}
    assert {c["variant"] for c in H.CASES if c["pattern"] == "random_band"} == {None, "chunked", "f_in"}
    # the long-row tail and the Int32 colour width are ragged's; more than kRegColors = 8 colours (eps from memory) random_band's
    M, N, colptr, rowval = G.pattern("ragged")
    assert np.bincount(rowval - 1, minlength=M).max() == 3000 and G.colouring("ragged", "greedy").max() > 253
    assert G.colouring("random_band", "greedy").max() > 8


def test_every_model_key_keeps_most_stored_values_finite():
    known = {G.model_key(c) for c in G.CASES}          # tests/test_exact_model.py::test_general_cases_keep_most_stored_values_finite
    added = {}
    for c in H.CASES:
        if G.model_key(c) not in known:
            added.setdefault(G.model_key(c), c)
    for c in H.CASES:
        if c["family"] != "ordinary":
            assert G.model_key(c) in known, c["id"]      # (no operand family on a key exact_general.CASES does not show)
    for key, c in added.items():
        want, _eps, _scaled = G.model(c)
        frac = float(np.isfinite(want).mean()) if want.size else 1.0
        print(c["id"], "finite share %.4f" % frac)
        assert want.size > 0 and frac >= G.MIN_FINITE, (c["id"], frac)


def _c_define(text, name):
    m = re.search(r"#define\s+%s\s+(\d+)\b" % name, text)
    assert m, name
    return int(m.group(1))


def test_header_lib_and_julia_shim_carry_the_same_values():
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flag = _c_define(hdr, "FD_PLAN_HANDOVER_ROWS")
    m = re.search(r"\bFD_INFO_HANDOVER_ROWS\s*=\s*(\d+)", hdr)
    assert m
    info = int(m.group(1))
    assert flag == 64 and flag == 2 * _c_define(hdr, "FD_PLAN_STORE_CSC_ROWS")                     # the next free bit
    others = [int(v) for v in re.findall(r"\bFD_INFO_[A-Z0-9_]+\s*=\s*(\d+)", hdr)]
    assert others.count(info) == 1 and info == max(others)                                          # the next free info number
    assert L.PLAN_HANDOVER_ROWS == flag and L.INFO_HANDOVER_ROWS == info
    jl = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    assert int(re.search(r"const FD_PLAN_HANDOVER_ROWS\s*=\s*Int32\((\d+)\)", jl).group(1)) == flag
    assert int(re.search(r"const FD_INFO_HANDOVER_ROWS\s*=\s*Cint\((\d+)\)", jl).group(1)) == info
    assert "handover_rows = false" in jl and "FD_PLAN_HANDOVER_ROWS : Int32(0)" in jl
    api = open(os.path.join(ROOT, "finitediff.jl_amd", "csrc", "fdjac_api.hip")).read()
    known = re.search(r"kPlanKnownFlags\s*=([^;]*);", api).group(1)
    assert "FD_PLAN_HANDOVER_ROWS" in known
