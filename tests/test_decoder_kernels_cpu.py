"""The model behind tests/test_decoder_kernels.py (tests/dec_kernel_model.py) is right and has teeth -- CPU only:

  * its references, chained, ARE oracle/ymt3_oracle.py::decoder_step: in float64 to 1e-9 at the first position and at a late one (the oracle run
    on double weights keeps the same rounding points), in fp32 within the noise of one flipped bf16 rounding; the attention reference alone is
    the oracle's attention(round_p=False);
  * every random case of the GPU module keeps its caps under the reference ALONE (stable share >= MIN_STABLE, left-out pairs <= MAX_LEFT_OUT),
    and the fp32 oracle arithmetic -- a correct implementation with another summation order -- passes every criterion and every exact probe;
  * every mutant -- a wrong kernel written as a variant of the reference, in float64, so that nothing but the mutation differs -- FAILS the
    check of a named GPU test on that test's own inputs;
  * the model.py wrappers refuse what needs no device to refuse.
"""
import pytest
import torch

import dec_kernel_model as D
from oracle import ymt3_oracle as O
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.model import YourMT3
from yourmt3_amd.weights import make_weights

_ATTN = D.attention_cases()
_FUSED = D.fused_cases()
_GEMM = D.gemm_cases()
_CACHE = {}


def _attn(name):
    if name not in _CACHE:
        c = _ATTN[name]()
        _CACHE[name] = (c,) + D.attention_reference(c)
    return _CACHE[name]


def _fused(name):
    if name not in _CACHE:
        c = _FUSED[name]()
        _CACHE[name] = (c, D.fused_reference(c))
    return _CACHE[name]


def _gemm(name):
    if name not in _CACHE:
        mode, make, la = _GEMM[name]
        c = make()
        _CACHE[name] = (mode, c, D.dec_gemm_reference(mode, c))
    return _CACHE[name]


# ----------------------------------------------------------------------------- the references are the oracle
@pytest.mark.parametrize("n", [1, 1000])
def test_attention_reference_in_fp32_is_the_oracles_attention(n):
    c = D.self_case("self8", [n] * 3, H=4, seed=n)
    parts, _ = D.attention_reference(c, dtype=torch.float32)
    k, v, bias, _ = D.gather_pairs(c)
    ref = O.attention(c["q"].float().reshape(12, 1, 64), k.float(), v.float(), bias[:, None, :], True, round_p=False)
    assert torch.allclose(D.rb(parts["o"]), ref[:, 0], atol=1e-6, rtol=1e-6)


def _chain(W, cfg, h, state, ckv, dtype):
    """one decoder layer and the lm_head as the chain of the kernels' references: QKV + append, self-attention, O-projection, cross query,
    cross-attention, O-projection, FFN-in, FFN-out, logits"""
    R, H, eps, t = h.shape[0], cfg.n_heads, cfg.ln_eps, state.pos
    L = t + 1
    w = lambda n: W[n]
    run = lambda mode, c: D.dec_gemm_model(mode, dict(c, eps=eps), dtype)
    keep = (lambda t: t.float()) if dtype == torch.float32 else (lambda t: t)      # the fp32 residual stream; in double the oracle keeps it in double
    tiles = lambda x: x.to(dtype).pow(2).reshape(R, 32, 16).sum(-1).T
    norm = lambda mode, x, gain, Wn: run(mode, dict(x=x, gain=w(gain), ssq=tiles(x), W=w(Wn)))["o"]
    qkv = D.rb(norm(D.DG_QKV, h, "dec.0.ln1", "dec.0.wqkv"))
    q, kc, vc = D.qkv_place(qkv, H, L, torch.full((R,), t), dtype)
    kc[:, :, :t], vc[:, :, :t] = state.k[0], state.v[0]
    bias = O.decoder_bias_by_distance(W["dec.relbias"], L, cfg)
    c = dict(form="self8", R=R, H=H, L=L, row0=0, rows_per_kv=1, n_keys=torch.full((R,), L), bias=bias, kc=kc, vc=vc)
    a = D.rb(D.attention_reference(c, q.reshape(-1, 64), dtype)[0]["o"]).reshape(R, -1)
    h = keep(run(D.DG_RESID, dict(a=a, W=w("dec.0.wo"), h=h))["o"])
    qc = D.rb(norm(D.DG_BF16, h, "dec.0.ln2", "dec.0.wq_c"))
    T = ckv[0][0].shape[2]
    c = dict(form="cross8", R=R, H=H, L=T, row0=0, rows_per_kv=1, n_keys=torch.full((R,), T), kc=ckv[0][0], vc=ckv[0][1])
    a = D.rb(D.attention_reference(c, qc.reshape(-1, 64), dtype)[0]["o"]).reshape(R, -1)
    h = keep(run(D.DG_RESID, dict(a=a, W=w("dec.0.wo_c"), h=h))["o"])
    ff = D.rb(norm(D.DG_RELU, h, "dec.0.ln3", "dec.0.wi").clamp(min=0))
    h = keep(run(D.DG_RESID, dict(a=ff, W=w("dec.0.wo2"), h=h))["o"])
    return norm(D.DG_LOGITS, h, "dec.ln_f", "dec.lm_head")


@pytest.mark.parametrize("pos", [0, 40])
def test_chained_references_are_the_oracles_decoder_step(pos):
    cfg = YMT3Config(segment_samples=8191, max_decode_len=64, n_enc_layers=1, n_dec_layers=1)
    W32 = make_weights(cfg, seed=1234)
    R = 3
    g = torch.Generator().manual_seed(pos)
    enc = torch.randn(R, 24, cfg.d_model, generator=g).bfloat16().float()
    toks = torch.randint(0, cfg.vocab, (pos + 1, R), generator=g)
    for dtype, W, tol in ((torch.float64, {k: v.double() for k, v in W32.items()}, 1e-9), (torch.float32, W32, None)):
        ckv = O.cross_kv(enc.to(dtype), W, cfg, True)
        state = O.DecoderState(R, cfg)
        state.k = [k.to(dtype) for k in state.k]
        state.v = [v.to(dtype) for v in state.v]
        for t in range(pos):
            O.decoder_step(toks[t], state, ckv, W, cfg, True)
        mine = _chain(W, cfg, W["dec.embed"][toks[pos]], state, ckv, dtype)
        ref = O.decoder_step(toks[pos], state, ckv, W, cfg, True)
        err = (mine.double() - ref.double()).abs()
        if tol is not None:
            assert float(err.max()) < tol, float(err.max())
        else:
            assert float(err.mean()) < 2e-3 and float(err.max()) < 0.06, (float(err.mean()), float(err.max()))


# ----------------------------------------------------------------------------- caps under the reference alone; the fp32 oracle passes
@pytest.mark.parametrize("name", list(_ATTN))
def test_attention_cases_keep_their_caps_and_admit_the_fp32_oracle(name):
    c, parts, beta = _attn(name)
    own = D.check_bf16(D.rb(parts["o"]), parts["o"], beta)
    assert own["ok"] and own["stable_share"] >= D.MIN_STABLE, own
    rec = D.check_attention(c, parts, beta, D.attention_simulate(c))
    assert rec["ok"], rec


@pytest.mark.parametrize("name", list(_FUSED))
def test_fused_cases_keep_their_caps_and_admit_the_fp32_oracle(name):
    c, fr = _fused(name)
    own = D.check_fused(fr, D.attention_simulate(c, torch.float64))
    assert own["ok"] and own["stable_share"] >= D.MIN_STABLE and own["left_out_share"] <= D.MAX_LEFT_OUT, own
    rec = D.check_fused(fr, D.attention_simulate(c))
    assert rec["ok"], rec
    if name.startswith("mc_"):                       # the same inputs under the one-term contract of dec_attn_kernel<false, true>
        c1 = dict(c, form="fused")
        assert D.check_fused(D.fused_reference(c1), D.attention_simulate(c1))["ok"]


@pytest.mark.parametrize("name", list(_GEMM))
def test_gemm_cases_keep_their_caps_and_admit_the_fp32_oracle(name):
    mode, c, ref = _gemm(name)
    own = D.check_dec_gemm(mode, c, ref, D.dec_gemm_simulate(mode, c, torch.float64))
    assert own["ok"] and own.get("stable_share", 1.0) >= D.MIN_STABLE, own
    rec = D.check_dec_gemm(mode, c, ref, D.dec_gemm_simulate(mode, c))
    assert rec["ok"], rec


def test_the_any_order_accumulation_term_would_break_the_cap_at_1024_keys():
    """why attention_beta takes the partition's depth for c: with c = n_keys the 1024-key rows fall below MIN_STABLE under the reference alone"""
    c, parts, beta = _attn("self8_step_n1024")
    k, v, bias, n = D.gather_pairs(c)
    q = c["q"].reshape(-1, 64)
    wide = D.attention_beta(q, parts, bias, n, 8, 6, depth_c=False)
    assert D.check_bf16(D.rb(parts["o"]), parts["o"], wide)["stable_share"] < D.MIN_STABLE
    assert D.check_bf16(D.rb(parts["o"]), parts["o"], beta)["stable_share"] >= D.MIN_STABLE


def test_probes_are_exact_under_the_fp32_oracle_and_cover_what_they_claim():
    for form in ("self8", "self2", "wo", "beam8", "beam2"):
        tails = D.TAILS_2WAVE if form.endswith("2") else D.TAILS_8WAVE
        for target in (None, "newest"):
            c = D.score_probe(form, tails, H=8 if form == "wo" else 2, target=target)
            rec = D.check_probe(c, D.attention_simulate(c))
            assert rec["ok"] and rec["exact_row_share"] == 1.0, (form, target, rec)
            parts, _ = D.attention_reference(c)
            assert bool((parts["e"].max(-1).values == 1).all()) and bool(((parts["e"] > 1e-100).sum(-1) == 1).all())      # every other key is exp(-256) or less: 0 in fp32
    # beam: every (position, holder) of a group of 4 occurs, both buffers are used, and a clamped entry is addressed
    c = D.score_probe("beam8", D.TAILS_8WAVE, target="newest")
    anc, n = c["anc"].long(), c["n_keys"]
    assert set(((n - 1) & 1).tolist()) == {0, 1}
    for p in (0, 2, 7):
        assert {int(anc[0, r, p]) for r in range(4)} == {0, 1, 2, 3}
    hit = [(r, int(n[r])) for r in range(c["R"]) if int(n[r]) == 2 and r % 2 == 1]
    assert hit and int(anc[(2 - 1) & 1, hit[0][0], 1]) >= c["W"]
    seen = set()
    for j in range(D.bias_probe_launches()):
        c = D.bias_probe("self8", j)
        seen |= set(c["peak"][c["target"][0] >= 0].tolist())
        if j in (0, 7, 15):
            assert D.check_bias_probe(c, D.attention_simulate(c))["ok"]
    assert seen == set(range(1024))
    for form, nc, row0 in (("fused", 1, 0), ("mc", 13, 13)):
        c = D.fused_probe(form, 256, 8, row0, nc)
        _, v, _, _ = D.gather_pairs(c)
        want = v[torch.arange(v.shape[0]), c["target"].reshape(-1)].reshape(c["R"], 8, 64)
        assert torch.equal(D.attention_simulate(c).float(), want.float())
        fq = D.fused_query(c)
        hot = (fq["q_pre"] != 0).sum(-1)
        assert bool((hot == 2).all()) and bool((fq["q_pre"] == D.rb(fq["q_pre"])).all())          # q is known exactly
        wq = c["wq"].float().reshape(8, 64, 512)
        assert bool((wq.sum(2) > 0).all()) and bool((wq.sum(1) == 2).all())       # every head row is hot for some k; two hot rows per column
    for mode in range(5):
        c, want = D.permutation_case(mode, 33, 512 if mode == D.DG_RESID else 384, 512)
        c.update(H=2, L=4, table=mode == D.DG_QKV)
        g = D.dec_gemm_simulate(mode, c)
        out = g.get("out", g.get("h", g.get("table")))
        w = want if mode in (D.DG_LOGITS, D.DG_RESID) else D.rb(want)
        assert torch.equal(out.float(), w.float()), mode


# ----------------------------------------------------------------------------- every mutant fails a named GPU test's check
ATTN_MUTANTS = [  # (mutant, the case of test_dec_attention_random_cases_meet_the_criterion it must fail)
    ("bias_by_key", "self8_tails"), ("bias_off_by_one", "self8_tails"), ("bias_next_head", "self8_tails"), ("skip_newest", "self8_tails"),
    ("stale_key", "self8_tails"), ("drop_wave", "self8_tails"), ("merge_no_rescale", "self8_tails"), ("scale", "self8_tails"),
    ("round_p", "self8_tails"), ("trunc_out", "self8_tails"), ("drop_wave", "self2_tails"), ("merge_no_rescale", "cross2_n250_rpk1_row3"),
    ("scale", "cross8_n512_rpk1_row0"), ("rows_per_kv_ignored", "cross8_n17_rpk3_row3"), ("rows_per_kv_ignored", "cross2_n128_rpk3_row0"),
    ("other_parity", "beam8_tails"), ("other_parity", "beam2_tails"), ("skip_newest", "self8_step_n385"), ("stale_key", "self2_step_n65"),
]


@pytest.mark.parametrize("mutant,name", ATTN_MUTANTS)
def test_attention_mutants_fail_the_random_criterion(mutant, name):
    c, parts, beta = _attn(name)
    rec = D.check_attention(c, parts, beta, D.attention_simulate(c, torch.float64, mutant))
    assert not rec["ok"], rec


@pytest.mark.parametrize("mutant", ["skip_newest", "bias_by_key", "other_parity"])
def test_attention_mutants_fail_the_exact_probes(mutant):
    """test_self_attention_score_probe_is_exact_at_every_tail_length[...-newest] / _bias_probe_...: the newest key left out returns another row
    of V; a bias read at `key` moves the peak; the other parity's table names another holder"""
    form = "beam8" if mutant == "other_parity" else "self8"
    c = D.score_probe(form, D.TAILS_8WAVE, target="newest")
    if mutant == "bias_by_key":
        c = D.bias_probe("self8", 3)
        assert not D.check_bias_probe(c, D.attention_simulate(c, torch.float64, mutant))["ok"]
    else:
        assert not D.check_probe(c, D.attention_simulate(c, torch.float64, mutant))["ok"]


FUSED_MUTANTS = [  # (mutant, the case of test_fused_query_attention_random_cases_meet_the_candidate_rule it must fail)
    ("round_p", "mc_T256_c13_seg3_row0"), ("round_p", "mc_T512_c16_seg1_row0"), ("ssq_31", "fused_T256_rpk1_row6"), ("ssq_31", "mc_T128_c2_seg3_row2"),
    ("eps_outside", "fused_T128_rpk3_row3"), ("gain_next", "fused_T512_rpk3_row3"), ("unrounded_operand", "fused_T256_rpk1_row6"),
    ("part_7", "fused_ipart_T256_rpk3_row6"), ("rows_per_kv_ignored", "fused_T128_rpk3_row3"), ("rows_per_kv_ignored", "mc_T256_c3_seg1_row3"),
    ("scale", "fused_ipart_T128_rpk1_row3"), ("trunc_out", "mc_T128_c3_seg1_row0"),
]


@pytest.mark.parametrize("mutant,name", FUSED_MUTANTS)
def test_fused_mutants_fail_the_candidate_rule(mutant, name):
    """(round_p on a multi-channel case IS the two-term split losing its low term)"""
    c, fr = _fused(name)
    rec = D.check_fused(fr, D.attention_simulate(c, torch.float64, mutant))
    assert not rec["ok"], rec


GEMM_MUTANTS = [  # (mutant, the case of test_dec_gemm_random_cases_meet_the_criterion it must fail)
    ("ssq_31", "bf16_R17_row5"), ("ssq_31", "mid_logits_R33"), ("eps_outside", "bf16_R17_row5"), ("eps_outside", "qkv_R33_row0"),
    ("gain_next", "relu_R17_row5"), ("gain_next", "mid_qkv_R65"), ("unrounded_operand", "bf16_nt2_R33"), ("unrounded_operand", "logits_nt2_R33"),
    ("no_relu", "relu_R17_row5"), ("no_relu", "mid_relu_R100"), ("resid_overwrites", "resid_K512"), ("resid_overwrites", "mid_resid_K2048_R33"),
    ("part_7", "resid_K512_part"), ("part_7", "resid_K2048_part"), ("ssq_from_s", "resid_K1024"), ("ssq_from_s", "mid_resid_K512_R31"),
    ("append_plus_one", "qkv_R17_row5"), ("append_plus_one", "qkv_lockstep_last"), ("swap_kv", "qkv_R17_row5"), ("swap_kv", "mid_qkv_R32"),
    ("pend_rows", "qkv_pend"), ("pend_rows", "logits_pend"), ("h_out_no_pend", "qkv_pend"), ("h_out_no_pend", "qkv_pend_nt2"),
]


@pytest.mark.parametrize("mutant,name", GEMM_MUTANTS)
def test_gemm_mutants_fail_the_random_criterion(mutant, name):
    mode, c, ref = _gemm(name)
    rec = D.check_dec_gemm(mode, c, ref, D.dec_gemm_simulate(mode, c, torch.float64, mutant))
    assert not rec["ok"], rec


def test_a_wrong_partial_fails_the_norm_that_reads_it():
    """test_dec_gemm_resid_accumulates_and_its_partials_feed_the_next_norm: partials of s^2 instead of h_new^2 move the next norm's scale"""
    mode, c, ref = _gemm("resid_K512")
    good, bad = D.dec_gemm_simulate(mode, c, torch.float64), D.dec_gemm_simulate(mode, c, torch.float64, "ssq_from_s")
    n = D.gemm_case(D.DG_BF16, 17, 128, 512, seed=3)
    n.update(x=good["h"], ssq=D.ssq_partials(good["h"]))
    refn = D.dec_gemm_reference(D.DG_BF16, n)
    assert D.check_dec_gemm(D.DG_BF16, n, refn, D.dec_gemm_simulate(D.DG_BF16, dict(n, ssq=good["ssq"]), torch.float64))["ok"]
    assert not D.check_dec_gemm(D.DG_BF16, n, refn, D.dec_gemm_simulate(D.DG_BF16, dict(n, ssq=bad["ssq"]), torch.float64))["ok"]


# ----------------------------------------------------------------------------- wrapper refusals that need no device
@pytest.fixture()
def w():
    """a YourMT3 that owns no handle: every refusal below is raised before the library would be touched"""
    obj = YourMT3.__new__(YourMT3)
    obj.device = torch.device("cpu")
    return obj


def _bf(*s):
    return torch.zeros(*s, dtype=torch.bfloat16)


def test_dec_gemm_wrapper_refuses(w):
    x, gain, ssq, W = torch.zeros(8, 512), torch.ones(512), torch.zeros(32, 8), _bf(512, 512)
    ok = dict(W=W, R=8, N=512, K=512, x=x, gain=gain, ssq=ssq, ssq_stride=8, out_bf16=_bf(8, 512))
    bad = [dict(ok, ssq_stride=7), dict(ok, row0=1), dict(ok, K=1024), dict(ok, N=520), dict(ok, W=_bf(511, 512)), dict(ok, x=torch.zeros(7, 512)),
           dict(ok, out_bf16=_bf(8, 511)), dict(ok, gain=torch.ones(511)), dict(ok, ssq=torch.zeros(31, 8)), dict(ok, x=x.double()),
           dict(ok, pend_y=torch.zeros(16, 512)), dict(ok, part=torch.zeros(8, 8, 512)), dict(ok, N=48, W=_bf(48, 512), mid_rows=1),
           dict(ok, R=0), dict(ok, out_bf16=None), dict(ok, W=W.T)]
    for kw in bad:
        with pytest.raises(ValueError):
            w.test_dec_gemm(1, **kw)
    qkv = dict(W=_bf(1536, 512), R=8, N=1536, K=512, x=x, gain=gain, ssq=ssq, ssq_stride=8, H=8, L=4, out_bf16=_bf(8, 512), kcache=_bf(8, 8, 4, 64),
               vcache=_bf(8, 8, 4, 64))
    pos = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3], dtype=torch.int32)
    bad = [dict(qkv, step=4), dict(qkv, step=-1), dict(qkv, N=1024, W=_bf(1024, 512)), dict(qkv, kcache=_bf(8, 8, 3, 64)), dict(qkv, row_pos=pos[:7]),
           dict(qkv, row_pos=pos + 1), dict(qkv, row_pos=pos - 1), dict(qkv, row_pos=pos.long()), dict(qkv, table=_bf(8, 1536), mid_rows=1),
           dict(qkv, pend_y=torch.zeros(16, 512), ssq=None), dict(qkv, pend_y=torch.zeros(16, 512), ssq=None, h_out=x),
           dict(qkv, pend_y=torch.zeros(15, 512), ssq=None, h_out=torch.zeros(8, 512))]
    for kw in bad:
        with pytest.raises(ValueError):
            w.test_dec_gemm(0, **kw)
    res = dict(W=W, R=8, N=512, K=512, a=_bf(8, 512), out_f32=torch.zeros(8, 512), ssq=ssq, ssq_stride=8)
    bad = [dict(res, N=256, W=_bf(256, 512)), dict(res, K=768, W=_bf(512, 768), a=_bf(8, 768)), dict(res, K=1024, W=_bf(512, 1024), a=_bf(8, 1024), mid_rows=1),
           dict(res, part=torch.zeros(8, 7, 512)), dict(res, part=torch.zeros(8, 8, 512), mid_rows=8), dict(res, out_f32=torch.zeros(7, 512)),
           dict(res, ssq=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            w.test_dec_gemm(4, **kw)
    # (a valid call reaches the library, which this object does not have: every check above came before it)
    with pytest.raises(AttributeError):
        w.test_dec_gemm(1, **ok)


def test_dec_attention_wrapper_refuses(w):
    H, L, R = 8, 16, 4
    q, kv, bias, out = _bf(R, H, 64), _bf(R, H, L, 64), torch.zeros(H, L), _bf(R, H, 64)
    ok = dict(self_attn=True, k=kv, v=kv, R=R, H=H, slab_keys=L, q=q, bias=bias, out=out)
    pos = torch.tensor([0, 5, 15, 3], dtype=torch.int32)
    bad = [dict(ok, step=L), dict(ok, step=-1), dict(ok, row_pos=pos + 1), dict(ok, row_pos=pos[:3]), dict(ok, k=_bf(R, H, L - 1, 64)), dict(ok, bias=bias[:, :15]),
           dict(ok, row0=1), dict(ok, H=0), dict(ok, rows_per_kv=0), dict(ok, n_keys_const=3), dict(ok, wq=_bf(512, 512)), dict(ok, out=None),
           dict(ok, wo=_bf(512, 512), opart=torch.zeros(R, 8, 512)), dict(ok, out=None, wo=_bf(512, 512), opart=torch.zeros(R, 7, 512)),
           dict(ok, out=None, wo=_bf(512, 512), opart=torch.zeros(R, 8, 512), force_many=True),
           dict(ok, anc=torch.zeros(2, R, 32, dtype=torch.uint8), anc_rows=R, anc_pitch=32, W=3),
           dict(ok, anc=torch.zeros(2, R, 32, dtype=torch.uint8), anc_rows=R, anc_pitch=16, W=4),
           dict(ok, anc=torch.zeros(2, R, 24, dtype=torch.uint8), anc_rows=R, anc_pitch=24, W=4),
           dict(ok, anc=torch.zeros(2, R - 1, 32, dtype=torch.uint8), anc_rows=R - 1, anc_pitch=32, W=4),
           dict(ok, anc=torch.zeros(1, R, 32, dtype=torch.uint8), anc_rows=R, anc_pitch=32, W=4)]
    for kw in bad:
        with pytest.raises(ValueError):
            w.test_dec_attention(**kw)
    cross = dict(self_attn=False, k=kv, v=kv, R=R, H=H, slab_keys=L, q=q, out=out, n_keys_const=L)
    x, gain, ssq, wq = torch.zeros(R, 512), torch.ones(512), torch.zeros(32, R), _bf(H * 64, 512)
    fused = dict(cross, q=None, wq=wq, x=x, gain=gain, ssq=ssq, ssq_stride=R)
    bad = [dict(cross, n_keys_const=0), dict(cross, n_keys_const=L + 1), dict(cross, bias=bias), dict(cross, row_pos=pos), dict(cross, rows_per_kv=2, k=_bf(1, H, L, 64)),
           dict(cross, slab_keys=5000, n_keys_const=4096, k=_bf(R, H, 5000, 64), v=_bf(R, H, 5000, 64)),
           dict(fused, ssq_stride=R - 1), dict(fused, x=torch.zeros(R, 256), gain=torch.ones(256)), dict(fused, force_many=True),
           dict(fused, ssq=None, ipart=torch.zeros(R, 8, 512), H=4, k=_bf(R, 4, L, 64), v=_bf(R, 4, L, 64), wq=_bf(256, 512), out=_bf(R, 4, 64)),
           dict(fused, ssq=None, ipart=torch.zeros(R, 7, 512)), dict(fused, ssq=None), dict(fused, wq=_bf(H * 64, 511))]
    for kw in bad:
        with pytest.raises(ValueError):
            w.test_dec_attention(**kw)
    for kw in (ok, cross, fused):
        with pytest.raises(AttributeError):
            w.test_dec_attention(**kw)


def test_mc_cross_attention_wrapper_refuses(w):
    H, T, nc = 8, 128, 3
    ok = dict(x=torch.zeros(nc, 512), gain=torch.ones(512), ssq=torch.zeros(32, nc), ssq_stride=nc, wq=_bf(H * 64, 512), k=_bf(1, H, T, 64),
              v=_bf(1, H, T, 64), out=_bf(nc, H, 64), n_seg=1, n_channels=nc, H=H, T=T)
    bad = [dict(ok, n_channels=1), dict(ok, n_channels=17), dict(ok, T=64), dict(ok, T=192), dict(ok, T=1024), dict(ok, ssq_stride=nc - 1), dict(ok, n_seg=2),
           dict(ok, row0=1), dict(ok, gain=torch.ones(256)), dict(ok, n_seg=0), dict(ok, out=_bf(nc, H, 63)), dict(ok, k=_bf(1, H, T - 1, 64))]
    for kw in bad:
        with pytest.raises(ValueError):
            w.test_mc_cross_attention(**kw)
    with pytest.raises(AttributeError):
        w.test_mc_cross_attention(**ok)
