"""The cases of tests/test_gpu_handover_rows.py: the ROW-WISE hand-over decompression (FD_PLAN_HANDOVER_ROWS, k_decompress_rows in
csrc/fdjac_decompress_rows.hip) against the exact host model and against the route a plan without the flag takes.  Pure numpy:
patterns, colourings, operands, inputs, the destination's layout and the model's answer are those of tests/exact_general.py -- a case
here is a case of that table's shape, so G.inputs / G.layout / G.model / G.model_key take it as it is.  Test infrastructure only.

  patterns     random_band (19 greedy colours: per-colour eps from memory), ragged (empty rows, empty columns, ONE row of 3000
               entries: the wavefront-per-row tail; its greedy colouring has about 3000 colours: Int32 colours, and as many small
               launches of f -- one such case), wide, tall (rows of about 36 entries), lap5, tiny_N (N = 1, 2, 3, 65, 257: fewer
               rows than a wavefront, one more than a wavefront, one more than a tile of 256)
  colourings   greedy / none5 / invalid go round with forward / central / dir = -1 as in exact_general._build_cases
  Float32      random_band and lap5
  variants     chunked (two colours per chunk: `untouched` and `zero in the first chunk only`) and f_in on random_band
  operands     every family of G.FAMILIES on random_band x greedy x forward / central only: those model keys occur in
               exact_general.CASES, so tests/test_exact_model.py already shows with the model alone that at least 90 % of their stored
               values are finite (tests/test_handover_rows_cpu.py asserts the same for every key this table adds)"""
import exact_general as G
from exact_general import pattern, colouring, operands, inputs, layout, model      # noqa: F401  (the table's vocabulary, not restated)

ROUND = (("greedy", "forward", 1.0), ("none5", "central", 1.0), ("invalid", "forward", -1.0),
         ("greedy", "central", 1.0), ("none5", "forward", -1.0), ("invalid", "central", 1.0))
COMPLEX_PATTERNS = ("random_band", "tiny_65")      # the complex step (MODE 2) of test_complex_step_equals_the_list_route


def _case(pat, col, fdtype, dir=1.0, dtype="f64", family="ordinary", variant=None):
    cid = "-".join([pat, col, "rows", fdtype + ("m" if dir < 0 else ""), dtype, family] + ([variant] if variant else []))
    return dict(id=cid, pattern=pat, colouring=col, kernel="rows", fdtype=fdtype, dir=dir, dtype=dtype, family=family, variant=variant, tile=None)


def _build_cases():
    out = []
    for pat in ("random_band", "wide", "tall", "lap5", "tiny_65", "tiny_257"):
        out += [_case(pat, col, fdtype, dir) for col, fdtype, dir in ROUND]
    # (ragged: a valid colouring has one colour per column of the dense row -- about 3000 launches of f: ONE such case)
    out += [_case("ragged", "greedy", "forward"), _case("ragged", "invalid", "central"), _case("ragged", "invalid", "forward", dir=-1.0)]
    for n in (1, 2, 3):
        out += [_case("tiny_%d" % n, "greedy", "forward", dir=-1.0), _case("tiny_%d" % n, "greedy", "central")]
    for pat in ("random_band", "lap5"):
        out += [_case(pat, "greedy", "forward", dtype="f32"), _case(pat, "invalid", "central", dtype="f32")]
    out += [_case("random_band", "greedy", "central", variant="chunked"), _case("random_band", "none5", "forward", variant="chunked"),
            _case("random_band", "greedy", "forward", variant="f_in"), _case("random_band", "none5", "forward", variant="f_in")]
    for fam in G.FAMILIES:
        if fam == "ordinary":
            continue
        out += [_case("random_band", "greedy", fdtype, family=fam) for fdtype in ("forward", "central")]
    return out


CASES = _build_cases()
