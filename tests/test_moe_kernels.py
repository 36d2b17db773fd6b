"""The mixture-of-experts decoder FFN's separate launches one by one (csrc/moe.hip: router, expert wi, expert wo, combine), through the test door
ymt3_test_moe_stage of include/ymt3.h, against float64 references of their contracts (tests/moe_kernel_model.py; tests/test_moe_kernels_cpu.py
shows that model right and sharp, and that every random case here keeps its caps under the reference alone):

  exact probes   one-hot router rows give exact logits in either summation order (ties to the lower id in both slots, across the two passes);
                 one-hot activation rows return a column of the expert's weights bit for bit under every routing the pair scan can meet
  criterion      tests/enc_kernel_model.py's: a stable element must equal the reference bit for bit, the others lie within beta + 1 bf16 ulp;
                 decided router rows must equal the reference's choice, gates lie within a derived bound
  guards         every output lies inside sentinels (Guarded): rows and pairs below row0, pairs of no expert, 64 elements either side must come
                 back untouched; inputs below row0 hold NaN
  state          a decode call after all the door calls gives the bits it gave before them (the last test of the module)
Every test records its figures under moe_kernel_* in the parity report.
"""
import ctypes

import pytest
import torch

import moe_kernel_model as M
from test_encoder_kernels import SENT, Guarded, m  # noqa: F401 (m: the encoder module's small handle, one per module)
from test_gpu_parity import _REPORT
from yourmt3_amd import _lib

pytestmark = pytest.mark.gpu
assert SENT == M.SENT
_BEFORE = {}
_DEV = {}


@pytest.fixture(scope="module", autouse=True)
def _decode_before_and_after(m):
    """the handle's own decode before any door call; test_decode_after_the_door_gives_the_same_bits compares"""
    g = torch.Generator().manual_seed(11)
    enc = torch.randn(2, m.cfg.n_frames, m.cfg.d_model, generator=g).bfloat16()
    _BEFORE["enc"] = enc
    _BEFORE["out"] = [t.cpu() for t in m.decode(enc, 24, return_logits=True)]
    yield
    _DEV.clear()


def _record(name, rec):
    rec = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}
    _REPORT["moe_kernel_" + name] = rec
    print(name, rec)
    return rec


def _span(n, lo, hi, *rest):
    w = torch.zeros((n,) + rest, dtype=torch.bool)
    w[lo:hi] = True
    return w


# ----------------------------------------------------------------------------- router
def _run_router(m, c):
    """one router launch -> the device's whole xn (rows, 512), sel (2 rows,), gate (2 rows,)"""
    dev = m.device
    row0, R = c["row0"], c["R"]
    rows = row0 + R
    xn, sel, gate = Guarded(m, rows * 512, torch.bfloat16), Guarded(m, 2 * rows, torch.int32), Guarded(m, 2 * rows, torch.float32)
    m.test_moe_stage(0, R=R, E=c["E"], row0=row0, eps=c["eps"], ssq_stride=c["stride"], h=c["h"].to(dev), gain=c["gain"].to(dev), ssq=c["ssq"].to(dev),
                     router=c["router"].to(dev), xn=xn.view, sel=sel.view, gate=gate.view)
    return dict(xn=xn.read(_span(rows, row0, rows, 512)).reshape(rows, 512), sel=sel.read(_span(2 * rows, 2 * row0, 2 * rows)),
                gate=gate.read(_span(2 * rows, 2 * row0, 2 * rows)))


@pytest.mark.parametrize("E", M.ROUTER_E)
def test_router_random_cases_meet_the_criterion(m, E):
    """xn on the norm-operand criterion; decided rows choose what the float64 logits of the device's own xn choose, order included; gates
    within their derived bound, ordered, in [0, 1], summing to 1 within 2^-23; R across the wave-per-row grid's edge at 8, row0 in {0, 5}"""
    for R in M.ROUTER_R:
        for row0 in M.ROUTER_ROW0:
            c = M.router_case(E, R, row0)
            rec = _record(f"router_E{E}_R{R}_row{row0}", M.check_router(c, _run_router(m, c)))
            assert rec["ok"] and rec["stable_share"] >= M.MIN_STABLE and rec["undecided_share"] <= M.MAX_LEFT_OUT, rec


@pytest.mark.parametrize("E", M.ROUTER_E)
def test_router_tie_probes_are_exact(m, E):
    """exact logits: a tie goes to the lower id in the first and in the second slot -- pairs (0, 1), (3, 5), (7, 8) across the two passes and
    (8, 15) inside the second -- a three-way tie, E identical router rows give (0, 1) with gates exactly 0.5, a gap of 200 gates exactly (1, 0)"""
    recs = []
    for row0, identical in ((0, False), (5, False), (0, True), (5, True)):
        c, *want = M.router_probe(E, row0, identical)
        recs.append(M.check_router_probe(c, want, _run_router(m, c)))
    rec = _record(f"router_tie_probe_E{E}", M.join(recs))
    assert rec["ok"], rec


def test_router_nan_and_inf_rows_stay_in_their_rows(m):
    """the door's only claim for a non-finite row is safety: sel inside [0, E), the guards intact (Guarded.read), and the finite rows of the same
    launch unaffected bit for bit; a repeat gives the same bits"""
    c = M.router_case(9, 9, 5)
    clean = _run_router(m, c)
    again = _run_router(m, c)
    assert all(torch.equal(clean[k].view(torch.int16 if k == "xn" else torch.int32), again[k].view(torch.int16 if k == "xn" else torch.int32)) for k in clean)
    h = c["h"].clone()
    h[5 + 3] = float("nan")
    h[5 + 6, 77] = float("inf")
    got = _run_router(m, dict(c, h=h))
    sel = got["sel"][10:]
    assert bool(((sel >= 0) & (sel < 9)).all()), sel
    keep = torch.ones(9, dtype=torch.bool)
    keep[[3, 6]] = False
    rows = 5 + keep.nonzero().flatten()
    pairs = torch.stack([2 * rows, 2 * rows + 1], 1).flatten()
    assert torch.equal(got["xn"][rows].view(torch.int16), clean["xn"][rows].view(torch.int16))
    assert torch.equal(got["sel"][pairs], clean["sel"][pairs]) and torch.equal(got["gate"][pairs].view(torch.int32), clean["gate"][pairs].view(torch.int32))
    _record("router_nan_inf_rows", dict(elements=int(rows.numel()), ok=True))


# ----------------------------------------------------------------------------- expert GEMMs
def _weights(m, c, key=None):
    """the case's expert weights on the device (`key`: kept for the module, the probes share theirs)"""
    names = ("w_q8", "w_s") if c["fp8"] else ("w",)
    if key is None:
        return {n: c[n].to(m.device) for n in names}
    if key not in _DEV:
        _DEV[key] = {n: c[n].to(m.device) for n in names}
    return _DEV[key]


def _run_expert(m, c, key=None):
    """one expert GEMM launch -> the device's whole output (2 rows, N): hidden bf16 (stage 1) or y f32 (stage 2)"""
    dev = m.device
    st, row0, R, E, fp8 = c["stage"], c["row0"], c["R"], c["E"], c["fp8"]
    rows = row0 + R
    N = M.D_FF if st == 1 else M.D_MODEL
    out = Guarded(m, 2 * rows * N, torch.bfloat16 if st == 1 else torch.float32)
    w = _weights(m, c, key)
    kw = dict(R=R, E=E, row0=row0, fp8=fp8, sel=c["sel"].to(dev))
    if st == 1:
        kw.update(xn=c["a"].to(dev), hidden=out.view, **({"wi_q8": w["w_q8"], "wi_s": w["w_s"]} if fp8 else {"wi": w["w"]}))
    else:
        kw.update(hidden=c["a"].to(dev), gate=c["gate"].to(dev), y=out.view, **({"wo_q8": w["w_q8"], "wo_s": w["w_s"]} if fp8 else {"wo": w["w"]}))
    m.test_moe_stage(st, **kw)
    written = torch.zeros(2 * rows, N, dtype=torch.bool)
    mine = c["sel"][2 * row0:]
    written[2 * row0:] = ((mine >= 0) & (mine < E))[:, None]
    return out.read(written).reshape(2 * rows, N)


@pytest.mark.parametrize("name", [x[0] for x in M.EXPERT_RANDOM])
def test_expert_random_cases_meet_the_criterion(m, name):
    """both stages, bf16 and fp8, on sign-coherent operands with random routing: hidden on the bf16 criterion (relu), y against its fp32 beta;
    R in {1, 9, 40}, row0 in {0, 3}, E in {2, 3}, 8 once per form and 16 once"""
    _, st, fp8, E, R, row0 = next(x for x in M.EXPERT_RANDOM if x[0] == name)
    c = M.expert_case(st, fp8, E, R, row0)
    rec = _record("expert_" + name, M.check_expert(c, _run_expert(m, c)))
    assert rec["ok"] and rec.get("stable_share", 1.0) >= M.MIN_STABLE, rec


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("stage", [1, 2])
def test_expert_routing_patterns_are_exact(m, stage, fp8):
    """one-hot activation rows (fp8: 448, power-of-two weight scales) return a column of the pair's expert bit for bit under every pattern of
    moe_kernel_model.PATTERNS: an expert with 0 / 1 / 16 / 17 / 32 / 33 pairs, all pairs on one expert, both slots on one expert, pairs only
    beyond the scan's first 512, on both sides of that boundary, six scan passes at R = 1536, row0 = 7 with a second pass, sel = -1 and sel = E"""
    recs = {}
    for name in M.PATTERNS:
        c, want = M.pattern_probe(stage, fp8, name)
        recs[name] = M.check_pattern_probe(c, want, _run_expert(m, c, key=("probe", stage, fp8)))
    rec = _record(f"expert_patterns_s{stage}_{'fp8' if fp8 else 'bf16'}", dict(M.join(list(recs.values())), patterns=len(recs),
                                                                            failed_patterns=[n for n, r in recs.items() if not r["ok"]]))
    assert rec["ok"], rec


@pytest.mark.parametrize("stage", [1, 2])
def test_fp8_value_edges(m, stage):
    """at kernel level: an all-zero row gives zeros, a maximum in the last K / 8 slice, a negative maximum, two rows of one chunk with maxima
    2^20 apart, and a 17-pair expert whose second chunk's row is 2^-20 of the first chunk's (row maxima are reset between chunks)"""
    c = M.fp8_edge_case(stage)
    got = _run_expert(m, c)
    rec = _record(f"expert_fp8_edges_s{stage}", M.check_expert(c, got))
    zero_pair = 2 * 1                                                   # row 1's slot-0 pair
    assert rec["ok"] and rec.get("stable_share", 1.0) >= M.MIN_STABLE and bool((got[zero_pair] == 0).all()), rec


def test_fp8_mfma_cut_inside_a_group_of_8_products_is_what_the_bound_allows(m):
    """moe_kernel_model.alignment_probe_case: a small product next to a 2^16 one.  In another group of 8, another MFMA or another wave it must
    arrive whole (the fp32 terms of fp8_beta alone); in the same group it may lose what mfma_fp8_alignment_loss states and no more"""
    c = M.alignment_probe_case()
    rec = _record("expert_fp8_mfma_alignment", M.check_alignment_probe(c, _run_expert(m, c)))
    assert rec["ok"], rec


def test_expert_value_regime_negative_operands(m):
    """stage 2 (fp32 out, gate 1) on value_regimes.gemm_operands('negative'): every product positive, the any-order bound at its tightest"""
    A, W = M.gemm_operands("negative", 12, 512, 2048)
    c = dict(stage=2, fp8=False, E=2, R=6, row0=0, a=A, sel=(torch.arange(12) % 2).int(), gate=torch.ones(12), w=torch.stack([W, -W]))
    rec = _record("expert_values_negative", M.check_expert(c, _run_expert(m, c)))
    assert rec["ok"], rec


# ----------------------------------------------------------------------------- combine
def _run_combine(m, c):
    dev = m.device
    row0, R, stride = c["row0"], c["R"], c["stride"]
    rows = row0 + R
    h = Guarded(m, rows * 512, torch.float32, c["h"].flatten())
    ssq = Guarded(m, 32 * stride, torch.float32)
    m.test_moe_stage(3, R=R, E=2, row0=row0, ssq_stride=stride, h=h.view, y=c["y"].to(dev), ssq=ssq.view)
    ws = torch.zeros(32, stride, dtype=torch.bool)
    ws[:, row0:rows] = True
    # (h's region is read whole: the rows below row0 hold the NaN they were given, which check_combine asserts)
    return dict(h=h.read(torch.ones(rows * 512, dtype=torch.bool)).reshape(rows, 512), ssq=ssq.read(ws).reshape(32, stride))


def test_combine_is_exact_and_leaves_the_next_norms_partials(m):
    """h + (y0 + y1) bit for bit, ssq tile 0 within its bound of sum(h_new^2), tiles 1..31 zero, the slack of ssq (stride > row0 + R) untouched"""
    recs = []
    for R in M.COMBINE_R:
        for row0 in M.COMBINE_ROW0:
            c = M.combine_case(R, row0)
            recs.append(M.check_combine(c, _run_combine(m, c)))
    rec = _record("combine", M.join(recs))
    assert rec["ok"], rec


def test_stages_chained_on_the_device_feed_each_other(m):
    """router -> wi -> wo -> combine on one set of buffers, each stage judged against the reference of what the stage before it LEFT"""
    E, R, row0 = 8, 9, 3
    rc = M.router_case(E, R, row0, seed=4)
    r = _run_router(m, rc)
    recs = [M.check_router(rc, r)]
    sel = torch.where(r["sel"] == int(SENT), torch.zeros_like(r["sel"]), r["sel"])                # pairs below row0: a valid id, as the cases have
    gate = torch.where(r["gate"] == SENT, torch.full_like(r["gate"], float("nan")), r["gate"])
    xn = torch.where(r["xn"] == SENT, torch.full_like(r["xn"], float("nan")), r["xn"])
    for fp8 in (False, True):
        c1 = dict(M.expert_case(1, fp8, E, R, row0, seed=6), a=xn, sel=sel, gate=gate)
        hid = _run_expert(m, c1)
        recs.append(M.check_expert(c1, hid))
        c2 = dict(M.expert_case(2, fp8, E, R, row0, seed=7), a=torch.where(hid == SENT, torch.full_like(hid, float("nan")), hid), sel=sel, gate=gate)
        y = _run_expert(m, c2)
        recs.append(M.check_expert(c2, y))
        cc = dict(R=R, row0=row0, stride=rc["stride"], h=rc["h"], y=torch.where(y == SENT, torch.full_like(y, float("nan")), y))
        recs.append(M.check_combine(cc, _run_combine(m, cc)))
    rec = _record("stages_chained", M.join(recs))
    assert rec["ok"], rec


# ----------------------------------------------------------------------------- refusals
def test_moe_stage_door_refuses(m):
    """the C side's own refusals (YMT3_ERR_ARG), past the wrapper: a raw argument struct per case; the door stays usable"""
    dev = m.device
    R, E = 4, 3
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    t = dict(h=z(R, 512), gain=z(512) + 1, ssq=z(32, R) + 1, router=z(E, 512, dt=torch.bfloat16), wi=z(E, 2048, 512, dt=torch.bfloat16),
             wo=z(E, 512, 2048, dt=torch.bfloat16), wi_q8=z(E, 2048, 512, dt=torch.uint8), wo_q8=z(E, 512, 2048, dt=torch.uint8), wi_s=z(16) + 1,
             wo_s=z(16) + 1, xn=z(R, 512, dt=torch.bfloat16), sel=z(2 * R, dt=torch.int32), gate=z(2 * R), hidden=z(2 * R, 2048, dt=torch.bfloat16),
             y=z(2 * R, 512))
    ptr = {k: v.data_ptr() for k, v in t.items()}

    def raw(stage, **f):
        base = dict(ptr, ssq_stride=R, fp8=0, row0=0, R=R, E=E, top_k=2, d_model=512, d_ff=2048, eps=1e-6)
        base.update(f)
        a = _lib.MoeArgs(**base)
        return m._lib.ymt3_test_moe_stage(m._handle, stage, ctypes.byref(a), m._stream())

    assert all(raw(s) == 0 for s in range(4)) and raw(1, fp8=1) == 0 and raw(2, fp8=1) == 0
    bad = [raw(4), raw(-1), raw(0, d_model=256), raw(0, d_ff=1024), raw(0, top_k=1), raw(0, E=1), raw(0, E=17), raw(0, R=0), raw(0, R=1537),
           raw(0, row0=-1), raw(0, ssq_stride=R - 1), raw(0, row0=1), raw(0, h=None), raw(0, gain=None), raw(0, ssq=None), raw(0, router=None),
           raw(0, xn=None), raw(0, sel=None), raw(0, gate=None), raw(0, sel=ptr["sel"] + 4), raw(0, xn=ptr["xn"] + 2), raw(1, xn=None), raw(1, sel=None),
           raw(1, hidden=None), raw(1, wi=None), raw(1, wi=ptr["wi"] + 2), raw(1, fp8=1, wi_q8=None), raw(1, fp8=1, wi_s=None), raw(1, fp8=1, wi_s=ptr["wi_s"] + 4),
           raw(2, hidden=None), raw(2, gate=None), raw(2, y=None), raw(2, wo=None), raw(2, fp8=1, wo_q8=None), raw(2, fp8=1, wo_s=None),
           raw(2, y=ptr["y"] + 8), raw(3, h=None), raw(3, y=None), raw(3, ssq=None), raw(3, ssq=ptr["ssq"] + 4)]
    assert all(rc != 0 for rc in bad), bad
    null = m._lib.ymt3_test_moe_stage(m._handle, 0, None, m._stream())
    assert null != 0
    assert all(raw(s) == 0 for s in range(4))
    # what a stage does not touch is not looked at
    assert raw(1, h=None, gain=None, ssq=None, router=None, gate=None, y=None, wo=None) == 0 and raw(3, sel=None, xn=None, wi=None) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the handle's own state (LAST test of the module)
def test_decode_after_the_door_gives_the_same_bits(m):
    after = [t.cpu() for t in m.decode(_BEFORE["enc"], 24, return_logits=True)]
    assert len(after) == len(_BEFORE["out"])
    for a, b in zip(after, _BEFORE["out"]):
        assert torch.equal(a, b)
