"""The model behind tests/test_moe_kernels.py (tests/moe_kernel_model.py) is right and has teeth -- CPU only:

  * its stage references, chained, ARE oracle/ymt3_oracle.py::moe_ffn in float64 to 1e-9 (E = 8 and 12, bf16 and fp8, the oracle's recorded
    MOE_CHOSEN as the routing), and its quantisation is oracle.quant_rows_fp8 but for the two quotients, which torch rounds twice;
  * every random case of the GPU module keeps its caps under the reference ALONE (stable share >= MIN_STABLE, undecided rows <= MAX_LEFT_OUT), and
    the same model evaluated in fp32 -- a correct implementation with another summation order -- passes every check and every exact probe;
  * every mutant of moe_kernel_model.MUTANTS -- a wrong kernel written as a variant of the reference, in float64, so that nothing but the mutation
    differs -- FAILS a named check of a named GPU test on that test's own inputs;
  * the model.py wrapper refuses what needs no device to refuse.
"""
import types

import pytest
import torch

import moe_kernel_model as M
from oracle import ymt3_oracle as O
from yourmt3_amd.model import YourMT3

F64 = torch.float64
_CACHE = {}


def _router(E, R, row0):
    key = ("router", E, R, row0)
    if key not in _CACHE:
        c = M.router_case(E, R, row0)
        _CACHE[key] = (c, M.router_model(c))
    return _CACHE[key]


def _expert(name):
    if name not in _CACHE:
        _, st, fp8, E, R, row0 = next(x for x in M.EXPERT_RANDOM if x[0] == name)
        c = M.expert_case(st, fp8, E, R, row0)
        _CACHE[name] = (c, M.expert_model(c))
    return _CACHE[name]


def _edge(stage):
    key = ("edge", stage)
    if key not in _CACHE:
        c = M.fp8_edge_case(stage)
        _CACHE[key] = (c, M.expert_model(c))
    return _CACHE[key]


# ----------------------------------------------------------------------------- the references are the oracle
class _Q8AsDouble:
    """stands where the oracle expects the uint8 weights: .view(float8).float() gives their values in double, so its matmuls run in float64"""

    def __init__(self, q8):
        self.q8 = q8

    def view(self, *a):
        return self

    def float(self):
        return M.e4m3_values(self.q8).double()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("E", [8, 12])
def test_chained_stage_references_are_the_oracles_moe_ffn(E, fp8, monkeypatch):
    R = 6
    if fp8:      # the model's stages quantise with the oracle's own function here: its quotients are an ulp off the kernel's for some maxima
        monkeypatch.setattr(M, "QUANT", O.quant_rows_fp8)       # (test_quantisation_is_the_oracles_but_for_its_two_rounding_quotients)
    rc = M.router_case(E, R, 0, seed=3)
    r = M.router_model(rc)
    sel = r["sel"].reshape(-1)
    c1 = M.expert_case(1, fp8, E, R, 0, seed=1, sel=sel)
    c1["a"] = r["xn"].bfloat16()
    m1 = M.expert_model(c1)
    # (the hand-over rounds the DOUBLE straight to bf16, as the oracle run on doubles does; enc_kernel_model.rb goes through fp32, as a device
    # does from its fp32 value, and differs from it where the double lies within 2^-29 of a bf16 midpoint)
    hidden = O._r(m1["o"].clamp(min=0), True)
    c2 = M.expert_case(2, fp8, E, R, 0, seed=2, sel=sel)
    c2.update(a=hidden.bfloat16(), gate=r["gate"].reshape(-1))              # the float64 gates
    y = M.expert_model(c2)["o"]
    mine = y[0::2] + y[1::2]
    assert float(mine.abs().max()) > 1e-3
    p = "dec.0."
    W = {p + "router": rc["router"].double()}
    if fp8:
        W.update({p + "wi_q8": _Q8AsDouble(c1["w_q8"]), p + "wo2_q8": _Q8AsDouble(c2["w_q8"]), p + "wi_s": c1["w_s"], p + "wo2_s": c2["w_s"]})
        orig = O.quant_rows_fp8
        # the oracle's own quantisation on the (bf16-exact) values in fp32, its q handed on in double; the row scale stays fp32, so that
        # xs * wscale is the fp32 product it is in the oracle's fp32 run
        monkeypatch.setattr(O, "quant_rows_fp8", lambda x: (lambda q, s: (q.double(), s))(*orig(x.float())))
    else:
        W.update({p + "wi": c1["w"].double().reshape(E * M.D_FF, M.D_MODEL), p + "wo2": c2["w"].double().reshape(E * M.D_MODEL, M.D_FF)})
    cfg = types.SimpleNamespace(n_experts=E, moe_top_k=2, d_model=M.D_MODEL, d_ff=M.D_FF, moe_fp8=int(fp8))
    monkeypatch.setattr(O, "MOE_CHOSEN", [])
    ref = O.moe_ffn(r["xn"], W, p, cfg, True)
    assert torch.equal(O.MOE_CHOSEN[0], r["sel"])
    err = float((mine - ref).abs().max())
    assert err < 1e-9, err


def test_quantisation_is_the_oracles_but_for_its_two_rounding_quotients():
    """moe_kernel_model.quant_rows (the kernel's true divisions) against oracle.quant_rows_fp8 (torch's reciprocal-and-multiply for both
    quotients): inv and the row scale within one fp32 ulp, equal to the float64 quotient rounded once; q equal wherever x * inv is the same
    fp32 value, and one e4m3 step apart at the most elsewhere"""
    xs = [M.fp8_edge_case(1)["a"].float(), M.expert_case(2, True, 2, 40, 0)["a"].float()]
    for x in xs:
        q, s = M.quant_rows(x)
        oq, os_ = O.quant_rows_fp8(x)
        mx = x.abs().amax(-1, keepdim=True).clamp_min(1e-12)
        assert torch.equal(s, (mx.double() / 448).float())                         # the correctly rounded quotient (no double rounding: checked by the next line)
        assert bool(((mx.double() / 448) - s.double()).abs().max() <= (s.double() * 2.0 ** -24).max())
        ulp = torch.ldexp(torch.ones_like(s), torch.frexp(s)[1] - 24)
        assert bool(((s - os_).abs() <= ulp).all())
        inv, oinv = (448.0 / mx.double()).float(), (448.0 / mx).float()
        same = (x * inv) == (x * oinv)
        assert torch.equal(q[same], oq[same]) and float(same.float().mean()) > 0.5
        step = torch.ldexp(torch.ones_like(q), (torch.frexp(q.abs().clamp_min(2.0 ** -6))[1] - 1) - 3)
        assert bool(((q - oq).abs() <= step).all()) and float((q != oq).float().mean()) < 1e-3
    q, _ = M.quant_rows(xs[0])
    assert bool((q[1] == 0).all()) and float(q.abs().max()) == 448.0
    # trunc_e4m3 lands on the grid and never above the value in magnitude
    t = M.trunc_e4m3(xs[0] * 3.7)
    assert torch.equal(t.to(M.E4M3).float(), t) and bool((t.abs() <= (xs[0] * 3.7).abs()).all())


# ----------------------------------------------------------------------------- caps under the reference alone; the fp32 model passes
@pytest.mark.parametrize("E", M.ROUTER_E)
def test_router_cases_keep_their_caps_and_admit_the_fp32_model(E):
    for R in M.ROUTER_R:
        for row0 in M.ROUTER_ROW0:
            c, ref = _router(E, R, row0)
            own = M.check_router(c, M.router_simulate(c, F64), ref)
            assert own["ok"] and own["stable_share"] >= M.MIN_STABLE and own["undecided_share"] <= M.MAX_LEFT_OUT, (R, row0, own)
            rec = M.check_router(c, M.router_simulate(c), ref)
            assert rec["ok"], (R, row0, rec)


@pytest.mark.parametrize("name", [x[0] for x in M.EXPERT_RANDOM])
def test_expert_cases_keep_their_caps_and_admit_the_fp32_model(name):
    c, ref = _expert(name)
    own = M.check_expert(c, M.expert_simulate(c, F64), ref)
    assert own["ok"] and own.get("stable_share", 1.0) >= M.MIN_STABLE, own
    rec = M.check_expert(c, M.expert_simulate(c), ref)
    assert rec["ok"], rec


@pytest.mark.parametrize("stage", [1, 2])
def test_fp8_edge_case_keeps_its_caps_and_admits_the_fp32_model(stage):
    c, ref = _edge(stage)
    own = M.check_expert(c, M.expert_simulate(c, F64), ref)
    assert own["ok"] and own.get("stable_share", 1.0) >= M.MIN_STABLE, own
    assert M.check_expert(c, M.expert_simulate(c), ref)["ok"]
    q, _ = M.quant_rows(c["a"].float())
    assert bool(torch.isfinite(ref["o"]).all()) and bool((q[1 if stage == 1 else 2] == 0).all())


def test_alignment_probe_is_exact_in_fp32_and_the_measured_cut_meets_its_bound():
    """the probe's operands are on the e4m3 grid with every scale 1; plain fp32 arithmetic passes it; a device that cuts the small product of
    the big product's group to multiples of 2^3 (what the MI355X does) passes, one that cuts to 2^4 or cuts in ANOTHER group does not"""
    c = M.alignment_probe_case()
    ref = M.expert_model(c)
    q, xs = M.quant_rows(c["a"].float())
    assert torch.equal(q, c["a"].float()) and bool((xs == 1).all())
    assert M.check_expert(c, M.expert_simulate(c), ref)["ok"]
    exact = ref["o"]
    small = exact - 114688.0
    n = c["a"].shape[0] // 4

    def cut(unit, rows):
        out = exact.clone()
        out[rows] = 114688.0 + torch.floor(small[rows] / unit) * unit
        return out.float()
    assert M.check_alignment_probe(c, M.expert_simulate(c))["ok"] and M.check_alignment_probe(c, cut(8.0, slice(0, n)))["ok"]
    assert "cut within the window" in M.check_alignment_probe(c, cut(16.0, slice(0, n)))["failed"]
    assert "other groups whole" in M.check_alignment_probe(c, cut(8.0, slice(n, 2 * n)))["failed"]


def test_combine_cases_admit_the_fp32_model():
    for R in M.COMBINE_R:
        for row0 in M.COMBINE_ROW0:
            c = M.combine_case(R, row0)
            assert M.check_combine(c, M.combine_simulate(c))["ok"]
            assert M.check_combine(c, M.combine_simulate(c, F64))["ok"]


def test_probes_are_exact_under_the_fp32_model_and_cover_what_they_claim():
    seen = set()
    for E in M.ROUTER_E:
        for identical in (False, True):
            c, *want = M.router_probe(E, row0=5 if E == 9 else 0, identical=identical)
            rec = M.check_router_probe(c, want, M.router_simulate(c))
            assert rec["ok"], (E, identical, rec)
            l = M.router_model(c)["l"]
            top = l.sort(-1, descending=True).values
            assert bool(((top[:, 0] == top[:, 1]) | (top[:, 1] == top[:, 2] if E > 2 else True)).all())     # every row holds an exact tie
            if not identical:
                seen |= {tuple(s) for s in want[0].tolist()}
    assert {(0, 1), (3, 5), (7, 8), (8, 15), (15, 7), (0, 8), (6, 7), (13, 14)} <= seen, seen      # first slot, second slot, three-way
    for stage in (1, 2):
        for fp8 in (False, True):
            for name in ("count17", "invalid_sel", "row0_second_pass"):
                c, want = M.pattern_probe(stage, fp8, name)
                rec = M.check_pattern_probe(c, want, M.expert_simulate(c))
                assert rec["ok"], (stage, fp8, name, rec)
    # the patterns hold what their names say
    count = lambda name: int((M.pattern_sel(name)[2] == 1).sum())
    assert [count(f"count{n}") for n in (1, 16, 17, 32, 33)] == [1, 16, 17, 32, 33] and count("none") == 0 and count("six_passes") == 33
    at = (M.pattern_sel("six_passes")[2] == 1).nonzero().flatten()
    assert set((at // 512).tolist()) == set(range(6))
    assert (M.pattern_sel("only_second_pass")[2] == 1).nonzero().flatten().tolist() == [512, 513]
    assert (M.pattern_sel("pass_boundary")[2] == 1).nonzero().flatten().tolist() == [511, 512]


# ----------------------------------------------------------------------------- every mutant fails a named check of a named GPU test
ROUTER_MUTANTS = [  # (mutant, (E, R, row0) of test_router_random_cases_meet_the_criterion, the check that fails)
    ("swap_23", (8, 9, 5), "sel decided"), ("swap_23", (3, 7, 0), "sel decided"), ("ignore_8_15", (16, 9, 0), "sel decided"),
    ("ignore_8_15", (9, 9, 5), "sel decided"), ("gates_swapped", (8, 9, 0), "gate order / range / sum"), ("gates_swapped", (2, 1, 0), "gate bound"),
    ("softmax_all", (8, 9, 0), "gate bound"), ("softmax_all", (3, 8, 5), "gate bound"), ("unrounded_xn", (16, 9, 5), "gate bound"),
    ("eps_outside", (8, 9, 0), "xn"), ("eps_outside", (2, 7, 5), "xn"), ("row0_ignored", (8, 9, 5), "xn below row0 untouched"),
]


@pytest.mark.parametrize("mutant,shape,check", ROUTER_MUTANTS)
def test_router_mutants_fail_the_random_criterion(mutant, shape, check):
    c, ref = _router(*shape)
    rec = M.check_router(c, M.router_simulate(c, F64, mutant), ref)
    assert not rec["ok"] and check in rec["failed"], rec


@pytest.mark.parametrize("mutant,E", [("tie_higher", 2), ("tie_higher", 9), ("tie_higher", 16), ("ignore_8_15", 9), ("ignore_8_15", 16)])
def test_router_mutants_fail_the_tie_probe(mutant, E):
    """test_router_tie_probes_are_exact: the higher id at a tie, and a second pass that is not taken, name other experts"""
    c, *want = M.router_probe(E)
    rec = M.check_router_probe(c, want, M.router_simulate(c, F64, mutant))
    assert not rec["ok"] and "probe sel" in rec["failed"], rec
    if mutant == "tie_higher":
        c, *want = M.router_probe(E, identical=True)
        assert not M.check_router_probe(c, want, M.router_simulate(c, F64, mutant))["ok"]


EXPERT_MUTANTS = [  # (mutant, the case of test_expert_random_cases_meet_the_criterion, the check that fails)
    ("row_p", "s1_bf16_E3_R9_row3", "hidden"), ("row_p", "s1_fp8_E2_R40_row0", "hidden"), ("hidden_row0", "s2_bf16_E3_R9_row3", "y"),
    ("hidden_row0", "s2_fp8_E3_R40_row3", "y"), ("gate_other", "s2_bf16_E2_R40_row0", "y"), ("gate_other", "s2_fp8_E3_R9_row3", "y"),
    ("no_relu", "s1_bf16_E2_R1_row0", "hidden"), ("no_relu", "s1_fp8_E3_R9_row3", "hidden"), ("no_wscale", "s1_fp8_E3_R9_row3", "hidden"),
    ("no_wscale", "s2_fp8_E2_R40_row0", "y"), ("wscale_e0", "s1_fp8_E8_R9_row3", "hidden"), ("wscale_e0", "s2_fp8_E3_R40_row3", "y"),
    ("fp8_trunc", "s1_fp8_E2_R1_row0", "hidden"), ("fp8_trunc", "s2_fp8_E3_R9_row3", "y"), ("amax_slice", "s1_fp8_E3_R40_row3", "hidden"),
    ("amax_slice", "s2_fp8_E2_R1_row0", "y"), ("row0_ignored", "s1_bf16_E3_R9_row3", "pairs below row0 untouched"),
    ("row0_ignored", "s2_fp8_E3_R40_row3", "pairs below row0 untouched"), ("second_chunk_first", "s1_bf16_E2_R40_row0", "hidden"),
    ("second_chunk_first", "s2_fp8_E3_R40_row3", "y"),
]


@pytest.mark.parametrize("mutant,name,check", EXPERT_MUTANTS)
def test_expert_mutants_fail_the_random_criterion(mutant, name, check):
    c, ref = _expert(name)
    rec = M.check_expert(c, M.expert_simulate(c, F64, mutant), ref)
    assert not rec["ok"] and check in rec["failed"], rec


@pytest.mark.parametrize("mutant,stage", [("amax_slice", 1), ("amax_slice", 2), ("no_clamp", 1), ("no_clamp", 2)])
def test_fp8_mutants_fail_the_value_edges(mutant, stage):
    """test_fp8_value_edges: a maximum taken over one K / 8 slice misses the one in the last slice; without the clamp the zero row is NaN"""
    c, ref = _edge(stage)
    rec = M.check_expert(c, M.expert_simulate(c, F64, mutant), ref)
    assert not rec["ok"] and ("hidden" if stage == 1 else "y") in rec["failed"], rec


PATTERN_MUTANTS = [("ragged_written", "count17"), ("ragged_written", "count1"), ("second_chunk_first", "count17"), ("second_chunk_first", "count33"),
                   ("drop_beyond_512", "only_second_pass"), ("drop_beyond_512", "pass_boundary"), ("drop_beyond_512", "six_passes"),
                   ("row0_ignored", "row0_second_pass"), ("row_p", "count16"), ("hidden_row0", "row0_second_pass")]


@pytest.mark.parametrize("mutant,name", PATTERN_MUTANTS)
def test_walk_mutants_fail_the_routing_patterns(mutant, name):
    """test_expert_routing_patterns_are_exact, both stages where the mutant exists in both, bf16 and fp8"""
    for stage in ((1,) if mutant == "row_p" else (2,) if mutant == "hidden_row0" else (1, 2)):
        for fp8 in ((False, True) if name != "six_passes" else (False,)):
            c, want = M.pattern_probe(stage, fp8, name)
            rec = M.check_pattern_probe(c, want, M.expert_simulate(c, F64, mutant))
            assert not rec["ok"], (stage, fp8, rec)


@pytest.mark.parametrize("mutant,check", [("combine_rows", "h"), ("ssq_stale", "ssq tiles 1..31"), ("row0_ignored", "h")])
def test_combine_mutants_fail(mutant, check):
    c = M.combine_case(9, 5)
    rec = M.check_combine(c, M.combine_simulate(c, F64, mutant))
    assert not rec["ok"] and check in rec["failed"], rec


def test_every_listed_mutant_is_shown_failing():
    shown = {m for m, *_ in ROUTER_MUTANTS + EXPERT_MUTANTS + PATTERN_MUTANTS} | {"tie_higher", "no_clamp", "combine_rows", "ssq_stale"}
    assert shown == set(M.MUTANTS), shown ^ set(M.MUTANTS)


# ----------------------------------------------------------------------------- wrapper refusals that need no device
@pytest.fixture()
def w():
    obj = YourMT3.__new__(YourMT3)
    obj.device = torch.device("cpu")
    return obj


def _bf(*s):
    return torch.zeros(*s, dtype=torch.bfloat16)


def test_moe_stage_wrapper_refuses(w):
    R, E = 4, 3
    t = dict(h=torch.zeros(R, 512), gain=torch.ones(512), ssq=torch.zeros(32, R), router=_bf(E, 512), wi=_bf(E, 2048, 512), wo=_bf(E, 512, 2048),
             wi_q8=torch.zeros(E, 2048, 512, dtype=torch.uint8), wo_q8=torch.zeros(E, 512, 2048, dtype=torch.uint8), wi_s=torch.ones(E), wo_s=torch.ones(E),
             xn=_bf(R, 512), sel=torch.zeros(2 * R, dtype=torch.int32), gate=torch.zeros(2 * R), hidden=_bf(2 * R, 2048), y=torch.zeros(2 * R, 512))
    ok = dict(t, R=R, E=E)
    bad = [(4, ok), (-1, ok), (0, dict(ok, d_model=256)), (0, dict(ok, d_ff=1024)), (0, dict(ok, top_k=1)), (0, dict(ok, E=1)), (0, dict(ok, E=17)),
           (0, dict(ok, R=0)), (0, dict(ok, R=1537)), (0, dict(ok, row0=-1)), (0, dict(ok, row0=1)), (0, dict(ok, ssq_stride=R - 1)),
           (0, dict(ok, h=None)), (0, dict(ok, router=_bf(E - 1, 512))), (0, dict(ok, sel=t["sel"].long())), (0, dict(ok, gate=torch.zeros(2 * R - 1))),
           (0, dict(ok, ssq=torch.zeros(31, R))), (1, dict(ok, wi=None)), (1, dict(ok, fp8=True, wi_s=None)), (1, dict(ok, fp8=True, wi_q8=None)),
           (1, dict(ok, hidden=_bf(2 * R, 2047))), (1, dict(ok, wi=_bf(E, 2048, 511))), (2, dict(ok, fp8=True, wo_s=torch.ones(E - 1))),
           (2, dict(ok, fp8=True, wo_q8=None)), (2, dict(ok, gate=None)), (2, dict(ok, y=torch.zeros(2 * R, 511))), (3, dict(ok, y=None)),
           (3, dict(ok, h=torch.zeros(R, 512).double())), (3, dict(ok, ssq=None)), (2, dict(ok, hidden=_bf(2048, 2 * R).T))]
    for stage, kw in bad:
        with pytest.raises(ValueError):
            w.test_moe_stage(stage, **kw)
    for stage in range(4):             # (a valid call reaches the library, which this object does not have)
        with pytest.raises(AttributeError):
            w.test_moe_stage(stage, **ok)
        with pytest.raises(AttributeError):
            w.test_moe_stage(stage, **dict(ok, fp8=True))
