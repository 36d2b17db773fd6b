"""Parity along the VALUE axis: the rest of the GPU suite runs one draw of weights (seed 1234, T5 init scales) and one kind of audio, so
hidden states of unit RMS, scores a few units wide, no two equal logits and nothing non-finite.  Here the same kernels meet the oracle
at other magnitudes, at exact ties and at non-finite inputs (tests/value_regimes.py builds the weights and the bounds).

Bounds.  Every logits error and TAU are divided by the std of the oracle's logits, encoder errors by the oracle output's RMS, and the
project's bounds for its standard model (logits max 0.06 / mean 6e-3, TAU 0.03, encoder max 0.0625 / mean 4e-3, MIN_SAFE 0.8) are
multiplied by max(1, intrinsic_regime / intrinsic_standard), where `intrinsic` is the oracle in fp32 against the oracle with every sum
in double, measured in the test.  The MoE, multi-channel, Perceiver-TF and many-row cases take the factor of the same regime's dense
4-segment model: the regime edits lie outside what those variants change, so the regime's share of the noise is the dense model's.

Which case reaches which site (rsqrtf(ss / K + eps) sites; `tiny` puts the variance far below eps at each, test_ln_eps moves eps):
  decode.hip dec_gemm_kernel (norm fused into the decode GEMMs, two sites)   every regime x "separate"; many80 / chains200
  decode.hip dec_gemm_mid_kernel                                             every regime x "mid"
  decode.hip folded O-projection + norm (the attention kernels' tail, two)   every regime x "merged" / "separate" (fold is on to 96 rows)
  dec_chain_body.h (GEMM chain)                                              every regime x "merged" / "stream"
  dec_step.hip                                                               every regime x "step"
  enc_attn.hip spec_embed_kernel, norm.hip rmsnorm_d128_kernel               ptf x {tiny, big, bias40, crossq8}
  norm.hip rmsnorm_kernel (encoder norms)                                    every regime x "merged" (front check)
  mc_cross_attn.hip                                                          mc3 / mc13 x {tiny, big, bias40, crossq8}
  moe.hip router norm                                                        moe x "five" x {bf16, fp8}
  moe_chain.hip (router norm, next-GEMM norm)                                moe x "chain" x {bf16, fp8}
Argmax branches (argmax_embed_kernel): lock-step plain -- every teacher-forced / free decode, the duplicated and all-zero heads;
lock-step constrained -- test_constraint_with_ties, the all-zero head under a constraint; slot plain -- "stream" cases, the all-zero
head through inference_stream; slot constrained -- the all-zero head and the non-finite batch through inference_stream(constraint=).

Non-finite inputs (include/ymt3.h, non-finite values) are tested last, by one test; the kernels were made safe for them by reading
(no index derived from a logit reaches memory unclamped) before that test first ran.
"""
import numpy as np
import pytest
import torch

import value_regimes as VR
from constraint_oracle import constrained_greedy_decode
from oracle import ymt3_oracle as O
from score_oracle import scores_from_logits
from test_config_space import ENVS, SEPARATE, _create, _prove_regime
from test_constraints import _random_automaton, _walk_states
from test_gpu_parity import MIN_SAFE, TAU, _REPORT, _check_ids, _check_stream_prefix, _model, _moe_case
from yourmt3_amd.config import ENC_PERCEIVER_TF, FFN_MOE
from yourmt3_amd.constraint import TokenAutomaton

pytestmark = pytest.mark.gpu
CFG = VR.CFG
L = CFG.max_decode_len
NOEOS = CFG.with_(eos_id=-1)


def _standard():
    return VR.oracle_case("std")


def _ids_and_logits(name, case, b, got_t, got_l, ref_t=None, ref_l=None, **kw):
    """_check_ids in units of the oracle logits' std, with the regime's bounds; the record gains the figures the bounds came from"""
    ref_t = case["ids"] if ref_t is None else ref_t
    ref_l = case["logits"] if ref_l is None else ref_l
    s = b["std"]
    rec = _check_ids(name, got_t, ref_t, ref_l / s, got_l.cpu() / s, tau=b["tau_std"], tol_max=b["tol_max"], tol_mean=b["tol_mean"],
                     min_safe=MIN_SAFE, **kw)
    rec.update(logits_std=s, oracle_fp32_vs_fp64_max=b["intrinsic_max"], oracle_fp32_vs_fp64_mean=b["intrinsic_mean"],
               standard_fp32_vs_fp64_max=b["intrinsic_standard_max"], standard_fp32_vs_fp64_mean=b["intrinsic_standard_mean"],
               bound_max=b["tol_max"], bound_mean=b["tol_mean"])
    return rec


def _stream_prefix(free, case, b):
    """_check_stream_prefix at the regime's TAU (it compares the margin with TAU: the margin is rescaled so that it does)"""
    _check_stream_prefix(free.cpu(), case["free_ids"], VR.margin(case["free_logits"]) / b["std"] * (TAU / b["tau_std"]))


def _front(case, b, m, rec):
    """log-mel and encoder output against the oracle, encoder errors in units of the oracle output's RMS"""
    cfg = case["cfg"]
    mel = m.logmel(case["audio"].cuda())
    d_mel = float((mel.cpu() - case["mel"]).abs().max())
    d = (m.encode(mel).float().cpu() - case["enc"]).abs() / case["enc_rms"]
    rec.update(logmel_max_abs=d_mel, enc_max=float(d.max()), enc_mean=float(d.mean()), enc_rms=case["enc_rms"],
               enc_bound_max=b["enc_max"], enc_bound_mean=b["enc_mean"])
    assert d_mel < 1e-3, rec
    if cfg.encoder_type == ENC_PERCEIVER_TF:          # its own intrinsic bound, as test_perceiver_tf_encoder_matches_oracle
        assert rec["enc_max"] <= b["enc_max"] and rec["enc_mean"] <= 1.25 * case["enc_intrinsic_mean"] + 1e-4, rec
    else:
        assert rec["enc_max"] <= b["enc_max"] and rec["enc_mean"] <= b["enc_mean"], rec


_SEP = {}


def _separate_bits(key, case, monkeypatch, cfg=CFG):
    if key not in _SEP:
        m = _create(cfg, SEPARATE, monkeypatch, weights=case["W"])
        e = case["enc"].bfloat16().cuda()
        t, lg = m.decode(e, L, forced=case["feed"].cuda(), return_logits=True)
        _SEP[key] = (t.cpu(), lg.cpu(), m.decode(e, L).cpu())
        m.close()
    return _SEP[key]


def _run_regime(name, case, b, regime, monkeypatch, key):
    """one weight set in one decode regime: launch counts, teacher-forced logits / ids, free stream, promised bit-identities"""
    cfg = case["cfg"]
    m = _create(cfg, ENVS[regime], monkeypatch, weights=case["W"])
    e = case["enc"].bfloat16().cuda()
    taken = _prove_regime(m, e, cfg, regime)
    if regime == "stream":
        a = case["audio"].cuda()
        lock = m.inference(a)
        assert torch.equal(lock, m.decode(m.encode(m.logmel(a))))
        for slots, interval in ((1, 4), (3, 3)):
            assert torch.equal(m.inference_stream(a, slots=slots, interval=interval), lock), (slots, interval)
        assert int(lock.min()) >= 0 and int(lock.max()) < cfg.vocab
        _REPORT[name] = {"regime": taken}
        m.close()
        return
    got_t, got_l = m.decode(e, L, forced=case["feed"].cuda(), return_logits=True)
    rec = _ids_and_logits(name, case, b, got_t, got_l)
    rec["regime"] = taken
    assert bool(torch.isfinite(got_l).all())
    free = m.decode(e, L).cpu()
    _stream_prefix(free, case, b)
    assert torch.equal(m.decode(e[1:2], L).cpu(), free[1:2])
    if regime == "merged":
        _front(case, b, m, rec)
    t, lg = got_t.cpu(), got_l.cpu()
    if regime == "separate":
        _SEP.setdefault(key, (t, lg, free))
    sep_t, sep_l, sep_free = _separate_bits(key, case, monkeypatch, cfg)
    if regime in ("merged", "step"):                 # the merged kernels promise the separate launches' bits, at any values
        assert torch.equal(t, sep_t) and torch.equal(lg, sep_l) and torch.equal(free, sep_free)
    if regime == "mid":                              # other tiles, other summation order: proves the mid-tile kernels ran
        assert not torch.equal(lg, sep_l)
    m.close()


# ----------------------------------------------------------------------------- 1. weight regimes
@pytest.mark.parametrize("regime", list(ENVS))
@pytest.mark.parametrize("name", VR.REGIMES)
def test_weight_regimes_in_every_decode_regime(name, regime, monkeypatch):
    case = VR.oracle_case(name)
    b = VR.bounds(case, _standard())
    assert case["finite"] and VR.safe_fraction(case, b) >= MIN_SAFE
    _run_regime(f"value_{name}_{regime}", case, b, regime, monkeypatch, name)


@pytest.mark.parametrize("eps", [1e-6, 1e-5, 1e-3])
@pytest.mark.parametrize("name", ["std", "tiny"])
def test_ln_eps(name, eps, monkeypatch):
    """the config's ln_eps reaches every norm site: the standard weights and `tiny` (where eps decides every norm) against the oracle at
    the same eps, through the merged, separate and per-step kernels and the encoder.  test_value_space_cpu.py shows that under `tiny`
    an oracle at eps 1e-5 in place of 1e-6 misses this bound by a factor of 50."""
    cfg = CFG.with_(ln_eps=eps)
    case = VR.oracle_case(name, cfg)
    std = VR.oracle_case("std", cfg)
    b = VR.bounds(case, std)
    for regime in ("merged", "separate", "step", "mid"):
        _run_regime(f"value_{name}_eps{eps:g}_{regime}", case, b, regime, monkeypatch, (name, eps))


VARIANTS = {
    "mc3": (dict(n_channels=3), 4), "mc13": (dict(n_channels=13), 4),
    "ptf": (dict(encoder_type=ENC_PERCEIVER_TF, n_enc_layers=0), 4),
    "many80": (dict(max_decode_len=32, eos_id=-1), 80),        # 65-96 rows: separate launches, fold, the argmax's two-level ticket
    "chains200": (dict(max_decode_len=32, eos_id=-1), 200),    # 168-256 rows: two concurrent chains
}


@pytest.mark.parametrize("name", ["tiny", "big", "bias40", "crossq8"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_regimes_through_the_other_decoders_and_row_counts(variant, name, monkeypatch):
    kw, B = VARIANTS[variant]
    cfg = CFG.with_(**kw)
    n = cfg.max_decode_len
    b0 = VR.bounds(VR.oracle_case(name), _standard())                       # the regime's factor (module docstring)
    W = VR.regime_weights(cfg, name)
    m = _create(cfg, {}, monkeypatch, max_batch=B, weights=W)
    rec = {}
    if B == 4:
        a = VR.audio(cfg, B)
        mel, enc = VR.oracle_encode(a, W, cfg)
        if variant == "ptf":
            _, enc64 = VR.oracle_encode(a, W, cfg, double=True)
            rms = float(enc.pow(2).mean().sqrt())
            case = dict(cfg=cfg, audio=a, mel=mel, enc=enc, enc_rms=rms, enc_intrinsic_mean=float((enc64.float() - enc).abs().mean()) / rms)
            _front(case, b0, m, rec)
    else:                                            # the decoder is under test: both sides decode the GPU's encoder output
        a = O.synthetic_audio(B, cfg, seed=19)
        enc = m.encode(m.logmel(a.cuda())).float().cpu()
    free_t, free_l = O.greedy_decode(enc, W, cfg, n, True, return_logits=True)
    feed = VR.tiny_feed(free_t.shape, cfg) if name == "tiny" else free_t
    ref_t, ref_l = (free_t, free_l) if feed is free_t else O.greedy_decode(enc, W, cfg, n, True, forced=feed, return_logits=True)
    b = dict(b0, std=float(ref_l.std()))
    e = enc.bfloat16().cuda()
    got_t, got_l = m.decode(e, n, forced=feed.cuda(), return_logits=True)
    rec.update(_ids_and_logits(f"value_{name}_{variant}", dict(ids=ref_t, logits=ref_l), b, got_t, got_l))
    _REPORT[f"value_{name}_{variant}"] = rec
    rec["chains"] = m.last_decode_chains
    assert rec["chains"] == (2 if variant == "chains200" else 1)
    p = {k: v["launches"] for k, v in m.profile_decode(e, 8, stride=4).items() if v["launches"]}
    rec["regime"] = p
    if variant.startswith("mc"):
        assert p.get("cross_attn", 0) > 0 and p.get("attn_pair", 0) == 0, p          # the shared-KV kernel is the multi-channel cross-attention
    if B > 64:
        assert p.get("attn_pair", 0) == 0 and p.get("gemm_chain", 0) == 0, p
    free = m.decode(e, n).cpu()
    _check_stream_prefix(free, free_t, VR.margin(free_l) / b["std"] * (TAU / b["tau_std"]))
    assert int(free.min()) >= 0 and int(free.max()) < cfg.vocab
    m.close()


@pytest.mark.parametrize("name", ["tiny", "big", "bias40", "crossq8"])
@pytest.mark.parametrize("launches", ["chain", "five"])
@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_regimes_through_the_moe_decoder(fp8, launches, name, monkeypatch):
    """routing teacher-forced as _moe_case does; its bf16 / fp8 bounds in std units times the regime's factor"""
    cfg = CFG.with_(dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
    b = VR.bounds(VR.oracle_case(name), _standard())
    f = b["tol_max"] / VR.TOL_MAX
    W = VR.regime_weights(cfg, name)
    if fp8:                                          # (value_regimes.mixed_norm_head: what keeps the fp8 id check's coverage above its cap)
        W = VR.mixed_norm_head(cfg, W)
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    if launches == "five":
        monkeypatch.setenv("YMT3_NO_MOE_CHAIN", "1")
    m = _model(cfg, max_batch=4, weights=W)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    monkeypatch.delenv("YMT3_NO_MOE_CHAIN", raising=False)
    _, enc = VR.oracle_encode(VR.audio(cfg), W, cfg)
    free_t, free_l = O.greedy_decode(enc, W, cfg, L, True, return_logits=True)
    feed = VR.tiny_feed(free_t.shape, cfg) if name == "tiny" else free_t
    s = float(free_l.std())
    key = f"value_{name}_moe_{'fp8' if fp8 else 'bf16'}_{launches}"
    # (the router's logits keep their scale in every regime -- the normed row times the router -- so max_deficit stays absolute)
    if fp8:
        _moe_case(cfg, L, 0.08 * f * s, 8e-3 * b["tol_mean"] / VR.TOL_MEAN * s, 0.08 * f * s, 0.04, monkeypatch, enc=enc, m=m, feed=feed, name=key)
    else:
        _moe_case(cfg, L, b["tol_max"] * s, b["tol_mean"] * s, b["tau_std"] * s, 0.01, monkeypatch, min_safe=MIN_SAFE, enc=enc, m=m,
                  feed=feed, name=key)
    p = {k: v["launches"] for k, v in m.profile_decode(enc.bfloat16().cuda(), 8, stride=4).items() if v["launches"]}
    assert (p.get("ffn_wi_gemm", 0) == 0) == (launches == "chain"), p
    _REPORT[key].update(logits_std=s, regime=p, bound_factor=f, units="raw logits: divide tau and the errors by logits_std")
    m.close()


# ----------------------------------------------------------------------------- 2. exact ties
def _np_first_argmax(logits, mask=None):
    x = logits.cpu().numpy().astype(np.float32)
    if mask is not None:
        x = np.where(mask, x, -np.inf)
    return torch.from_numpy(np.argmax(x, axis=-1))                     # numpy's argmax is the first index of the maximum


def _dup_case():
    W, grp = VR.dup_head(NOEOS, VR.regime_weights(NOEOS, "std"))
    return VR.oracle_case("dup_head", NOEOS, W=W, key="dup_head"), grp


@pytest.mark.parametrize("regime", ["merged", "separate", "step", "mid"])
def test_duplicated_head_rows_tie_to_the_first_index(regime, monkeypatch):
    """an lm_head of 48 distinct rows, each 30 or 36 times (value_regimes.dup_head): the maximum is always tied.  The emitted id is the first
    index of the maximum of the call's own logits, copies of a row give bit-equal logits in every tile of every decode GEMM, and the
    winning ROW is the oracle's wherever the oracle's margin between distinct rows is at least TAU."""
    case, grp = _dup_case()
    b = VR.bounds(case, _standard())
    m = _create(NOEOS, ENVS[regime], monkeypatch, weights=case["W"])
    e = case["enc"].bfloat16().cuda()
    _prove_regime(m, e, NOEOS, regime)
    got_t, got_l, got_s = m.decode(e, L, forced=case["feed"].cuda(), return_logits=True, return_scores=True)
    got_l = got_l.cpu()
    first = torch.stack([(grp == g).nonzero()[0, 0] for g in range(48)])
    assert torch.equal(got_l, got_l[..., first][..., grp]), "copies of one lm_head row gave different logits"
    assert torch.equal(got_t.cpu().long(), _np_first_argmax(got_l))
    win = _np_first_argmax(got_l)
    assert torch.equal(win, first[grp[win]])                           # ... which is its row's first copy
    ref_g, got_g = case["logits"][..., first], got_l[..., first]       # one logit per distinct row
    rec = _ids_and_logits(f"value_dup_head_{regime}", case, b, got_g.argmax(-1), got_g, ref_t=ref_g.argmax(-1), ref_l=ref_g)
    rel = set()
    for w in win.flatten().tolist():
        cols = (grp == grp[w]).nonzero().flatten().tolist()
        for j in cols[1:]:
            rel |= VR.tie_relations(cols[0], j)
    rec["tie_relations"] = sorted(rel)
    assert rel >= {"stride", "lanes", "dpp_rows", "waves", "tiles", "first_tile", "last_tile"}, rel
    ref_s = scores_from_logits(got_l, got_t.cpu(), NOEOS, case["feed"])
    d = (got_s.cpu().double() - ref_s).abs()
    assert bool((d <= 1e-4 + 1e-5 * ref_s.abs()).all()), float(d.max())
    free = m.decode(e, L).cpu().long()
    assert torch.equal(free, first[grp[free]])                         # free-running: only first copies are ever emitted
    m.close()


def test_all_zero_head_emits_the_lowest_allowed_id(monkeypatch):
    """every logit exactly 0: id 0 at every step in lock-step and slot mode; under a constraint the lowest id its state allows"""
    W = VR.regime_weights(NOEOS, "std")
    W["dec.lm_head"] = torch.zeros_like(W["dec.lm_head"])
    m = _model(NOEOS, max_batch=4, weights=W)
    a = VR.audio(NOEOS).cuda()
    t, lg, sc = m.decode(m.encode(m.logmel(a)), L, return_logits=True, return_scores=True)
    assert int(lg.abs().max()) == 0 and int(t.abs().max()) == 0
    assert float((sc.cpu().double() + np.log(NOEOS.vocab)).abs().max()) < 1e-4
    assert int(m.inference(a).abs().max()) == 0
    assert int(m.inference_stream(a, slots=2, interval=3).abs().max()) == 0
    aut = _random_automaton(NOEOS.vocab, seed=4, p=0.2)
    allowed = aut.allowed.copy()
    allowed[:, :7] = False                           # no state allows id 0
    aut = TokenAutomaton(allowed, aut.next)
    lowest = torch.from_numpy(np.argmax(aut.allowed, axis=1))
    c = m.compile_constraint(aut)
    starts = torch.tensor([[0], [1], [2], [1]])
    for got in (m.inference(a, constraint=c, start_states=starts), m.inference_stream(a, slots=2, interval=3, constraint=c, start_states=starts)):
        got = got.cpu().long()
        st = starts[:, 0].clone()
        for i in range(L):
            assert torch.equal(got[:, 0, i], lowest[st]), i
            st = torch.from_numpy(aut.next).long()[st, got[:, 0, i]]
    c.close()
    m.close()


@pytest.mark.parametrize("regime", ["merged", "separate"])
def test_constraint_with_ties(regime, monkeypatch):
    """the duplicated head under a random automaton: the lowest allowed index among the maxima, the state following it, the score the
    masked log_softmax; the distinct row chosen is the constrained oracle's wherever its masked margin between rows is at least TAU"""
    case, grp = _dup_case()
    V = NOEOS.vocab
    aut = _random_automaton(V, seed=12, p=0.3)
    starts = torch.tensor([[0], [1], [2], [0]])
    m = _create(NOEOS, ENVS[regime], monkeypatch, weights=case["W"])
    c = m.compile_constraint(aut)
    e = case["enc"].bfloat16().cuda()
    allowed = torch.from_numpy(aut.allowed)
    for forced in (case["feed"], None):
        got_t, got_l, got_s = m.decode(e, L, forced=None if forced is None else forced.cuda(), return_logits=True, return_scores=True,
                                       constraint=c, start_states=starts)
        got_t, got_l = got_t.cpu(), got_l.cpu()
        fed = got_t if forced is None else forced
        mask = allowed[_walk_states(aut, fed, starts)]                 # the host walk of the fed ids: the state of every position
        assert torch.equal(got_t.long(), _np_first_argmax(got_l, mask.numpy()))
        masked = got_l.masked_fill(~mask, float("-inf"))
        ref_s = torch.log_softmax(masked.double(), -1).gather(-1, fed.long()[..., None])[..., 0]
        fin = torch.isfinite(ref_s)
        assert torch.equal(torch.isfinite(got_s.cpu()), fin)
        d = (got_s.cpu().double()[fin] - ref_s[fin]).abs()
        assert bool((d <= 1e-4 + 1e-5 * ref_s[fin].abs()).all()), float(d.max())
    # against the constrained oracle, teacher-forced with its own stream
    feed, _, _ = constrained_greedy_decode(case["enc"], case["W"], NOEOS, L, True, aut, start_states=starts)
    ref_t, _, ref_l = constrained_greedy_decode(case["enc"], case["W"], NOEOS, L, True, aut, start_states=starts, forced=feed)
    got_t = m.decode(e, L, forced=feed.cuda(), constraint=c, start_states=starts).cpu()
    mask = allowed[_walk_states(aut, feed, starts)]
    ref_m = ref_l.masked_fill(~mask, float("-inf"))
    # margin between DISTINCT rows: the best allowed logit of every row group, top two
    gl = torch.stack([ref_m[..., grp == g].amax(-1) for g in range(48)], -1)
    top = gl.topk(2, -1).values
    safe = (top[..., 0] - top[..., 1]) >= TAU * case["std"]
    assert float(safe.float().mean()) >= MIN_SAFE
    assert torch.equal(got_t[safe], ref_t[safe])                       # the same row AND its lowest allowed copy
    c.close()
    m.close()


@pytest.mark.parametrize("name", ["bias40", "tiny"])
def test_scores_at_extremes(name, monkeypatch):
    """*_scored against the log_softmax in double of the call's own logits; under `tiny` every score is close to -log V"""
    case = VR.oracle_case(name)
    m = _model(CFG, max_batch=4, weights=case["W"])
    e = case["enc"].bfloat16().cuda()
    for forced in (case["feed"], None):
        t, lg, sc = m.decode(e, L, forced=None if forced is None else forced.cuda(), return_logits=True, return_scores=True)
        ref = scores_from_logits(lg.cpu(), t.cpu(), CFG, forced)
        d = (sc.cpu().double() - ref).abs()
        assert bool((d <= 1e-4 + 1e-5 * ref.abs()).all()), float(d.max())
        if name == "tiny":
            live = ref != 0
            assert float((ref[live] + np.log(CFG.vocab)).abs().max()) < 0.1
    m.close()


@pytest.mark.parametrize("launches", ["chain", "five"])
@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_router_ties_go_to_the_lower_expert(fp8, launches, monkeypatch):
    """router rows 2 and 5 identical in every layer: their logits are equal, so wherever the pair takes first or second place the
    trace shows expert 2 before expert 5, and never 5 without 2.  Parity with the oracle (which breaks ties the same way) on top."""
    cfg = CFG.with_(dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
    W = VR.regime_weights(cfg, "std")
    for l in range(cfg.n_dec_layers):
        W[f"dec.{l}.router"][5] = W[f"dec.{l}.router"][2]
    if fp8:
        W = VR.mixed_norm_head(cfg, W)
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    if launches == "five":
        monkeypatch.setenv("YMT3_NO_MOE_CHAIN", "1")
    m = _model(cfg, max_batch=4, weights=W)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    monkeypatch.delenv("YMT3_NO_MOE_CHAIN", raising=False)
    _, enc = VR.oracle_encode(VR.audio(cfg), W, cfg)
    out = {}
    key = f"value_router_tie_{'fp8' if fp8 else 'bf16'}_{launches}"
    feed, free_l = O.greedy_decode(enc, W, cfg, L, True, return_logits=True)
    s = float(free_l.std())                          # the MoE bounds in units of the logits' std (4.6 with the mixed-norm head)
    if fp8:
        _moe_case(cfg, L, 0.08 * s, 8e-3 * s, 0.08 * s, 0.04, monkeypatch, enc=enc, m=m, feed=feed, name=key, out=out)
    else:
        _moe_case(cfg, L, 0.06 * s, 6e-3 * s, TAU * s, 0.01, monkeypatch, min_safe=MIN_SAFE, enc=enc, m=m, feed=feed, name=key, out=out)
    _REPORT[key].update(logits_std=s, units="raw logits: divide tau and the errors by logits_std")
    sel = out["trace"].reshape(-1, 2)
    has2, has5 = (sel == 2).any(-1), (sel == 5).any(-1)
    assert int(has5.sum()) > 0 and not bool((has5 & ~has2).any())      # 5 only ever together with 2 ...
    both = sel[has5]
    assert bool((both[:, 0] == 2).all() and (both[:, 1] == 5).all())   # ... and behind it: tied for first
    _REPORT[key]["choices_with_the_tied_pair"] = int(has2.sum())
    m.close()


def test_fp8_expert_edges(monkeypatch):
    """expert 1's matrices hold one weight 65536 times their largest other one (the others are scaled down by 2^-16, so the expert's
    scale is set by the outlier and everything else quantises to e4m3 subnormals or 0); expert 3 is all zero (scale from
    clamp_min(1e-12), q = 0).  At the fp8 MoE bounds, with the mixed-norm head of the other fp8 cases."""
    from yourmt3_amd.weights import make_weights, quantize_fp8_per_expert
    cfg = CFG.with_(dec_ffn=FFN_MOE, moe_fp8=1, eos_id=-1)
    Wb = make_weights(cfg.with_(moe_fp8=0), seed=1234)                  # the same draw, bf16 experts: edit, then quantise
    W = make_weights(cfg, seed=1234)
    E = cfg.n_experts
    for l in range(cfg.n_dec_layers):
        for k in ("wi", "wo2"):
            w = Wb[f"dec.{l}.{k}"].clone()
            we = w.view(E, -1, w.shape[-1])
            top = we[1].abs().max().clone()
            we[1] *= 2.0 ** -16
            we[1, 3, 5] = top
            we[3] = 0.0
            W[f"dec.{l}.{k}_q8"], W[f"dec.{l}.{k}_s"] = quantize_fp8_per_expert(w, E)
    W = VR.mixed_norm_head(cfg, W)
    q = W["dec.0.wi_q8"].view(torch.float8_e4m3fn).float().view(E, -1, cfg.d_model)
    assert float(q[1].abs().max()) == 448.0 and float(q[1].abs().flatten().sort().values[-2]) < 2.0 ** -6 and int(q[3].abs().max()) == 0
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    m = _model(cfg, max_batch=4, weights=W)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    _, enc = VR.oracle_encode(VR.audio(cfg), W, cfg)
    out = {}
    feed, free_l = O.greedy_decode(enc, W, cfg, L, True, return_logits=True)
    s = float(free_l.std())                          # the fp8 MoE bounds in units of the logits' std
    _moe_case(cfg, L, 0.08 * s, 8e-3 * s, 0.08 * s, 0.04, monkeypatch, enc=enc, m=m, feed=feed, name="value_fp8_expert_edges", out=out)
    _REPORT["value_fp8_expert_edges"].update(logits_std=s, units="raw logits: divide tau and the errors by logits_std")
    used = out["trace"].flatten().bincount(minlength=E)
    assert int(used[1]) > 0 and int(used[3]) > 0, used
    m.close()


# ----------------------------------------------------------------------------- 4. audio values
def _signals(S):
    n = torch.arange(S, dtype=torch.float64)
    g = torch.Generator().manual_seed(9)
    return {
        "square440": torch.sign(torch.sin(2 * np.pi * 440.0 * n / 16000 + 0.1)).float(),
        "square1000": torch.sign(torch.sin(2 * np.pi * 1000.0 * n / 16000 + 0.1)).float(),
        "dc": torch.ones(S),
        "nyquist": (1 - 2 * (torch.arange(S) % 2)).float(),
        "amp1e4": 1e4 * O.synthetic_audio(1, CFG, seed=2)[0],
        "amp1e-20": 1e-20 * torch.randn(S, generator=g),
    }


def test_logmel_at_extreme_audio_values():
    m = _model(CFG, max_batch=8)
    sig = _signals(CFG.segment_samples)
    a = torch.stack(list(sig.values()))
    ref = O.logmel(a, CFG)
    got = m.logmel(a.cuda()).cpu()
    for i, k in enumerate(sig):
        d = float((got[i] - ref[i]).abs().max())
        _REPORT[f"value_logmel_{k}"] = {"logmel_max_abs": d}
        assert d < 1e-3, (k, d)
    floor = torch.log(torch.tensor(CFG.log_floor, dtype=torch.float32))
    assert torch.equal(got[5], torch.full_like(got[5], floor.item())) and torch.equal(ref[5], got[5])
    m.close()


@pytest.mark.parametrize("sr", [16000, 44100])
@pytest.mark.parametrize("kind", ["int16_extremes_mono", "int16_extremes_stereo", "float_1e4", "float_1e-20", "float_square"])
def test_ingest_then_logmel_at_extreme_audio_values(kind, sr):
    """ingest (mix, resample or the 16 kHz copy, slice) and the log-mel of its segments against their oracles"""
    from oracle import ingest_oracle as IO
    m = _model(CFG, max_batch=8)
    n = 30000
    k = np.arange(n)
    sq = np.sign(np.sin(2 * np.pi * 330.0 * k / sr + 0.1))
    if kind.startswith("int16"):
        x = np.where(sq > 0, 32767, -32768).astype(np.int16)[:, None]
        pcm = x if kind.endswith("mono") else np.concatenate([x, x[::-1]], 1)
        amp = 1.0
    else:
        amp = {"float_1e4": 1e4, "float_1e-20": 1e-20, "float_square": 1.0}[kind]
        pcm = (amp * (sq if kind == "float_square" else np.random.default_rng(3).standard_normal(n))).astype(np.float32)[:, None]
    ref = IO.ingest(pcm, sr, CFG.sample_rate, CFG.segment_samples)
    got = m.ingest(torch.from_numpy(pcm), sr)
    g = got.cpu().numpy()[:, 0]
    assert g.shape == ref.shape
    d_seg = float(np.abs(g - ref).max())
    assert d_seg < 5e-6 * amp if amp >= 1 else d_seg < 5e-6 * amp * 4, d_seg          # the ingest bound, relative to the scale
    # Each stage against its oracle on the SAME input: the log-mel of the segments the device ingest produced.  Two ingest results
    # inside the ingest bound need not have log-mels within 1e-3: for the stereo int16 case the oracle in double moves by 0.14 in
    # its quietest bins when the segment is perturbed by 5e-7 (a tenth of the ingest bound), while its fp32-vs-double error on one
    # input is 2e-4.
    mel_ref = O.logmel(got.cpu()[:, 0], CFG)
    mel = m.logmel(got).cpu()
    d = float((mel - mel_ref).abs().max())
    _REPORT[f"value_ingest_{kind}_{sr}"] = {"ingest_max_abs": d_seg, "logmel_max_abs": d}
    assert d < 1e-3, d
    if kind == "float_1e-20":
        assert float(mel.max()) == float(np.log(np.float32(CFG.log_floor)))
    m.close()


# ----------------------------------------------------------------------------- 5. non-finite values
def test_non_finite_audio_stays_in_its_rows():
    """A batch of 4 in which segment 1 holds a sample of 1e20 (infinite power) and segment 2 a NaN (include/ymt3.h, non-finite values):
    every call returns, the clean rows are bit-identical to the same rows of a clean batch, the bad rows' logits are all NaN, their
    ids are in range and follow the rule -- id 0, or the lowest id the row's state allows -- their scores are NaN, and the next call
    on the same handle gives the clean bits.  Through inference, *_scored, *_constrained and the constrained stream (slot path)."""
    cfg = NOEOS
    m = _model(cfg, max_batch=4)
    clean = VR.audio(cfg)
    bad = clean.clone()
    bad[1, 4000] = 1e20
    bad[2, 1234] = float("nan")
    good, ill = [0, 3], [1, 2]
    # the front end: the documented rule, against the oracle
    mel, ref = m.logmel(bad.cuda()).cpu(), O.logmel(bad, cfg)
    assert torch.equal(torch.isnan(mel[2]), torch.isnan(ref[2])) and bool(torch.isnan(mel[2]).any())     # NaN in exactly the oracle's frames
    assert float((mel[2][~torch.isnan(ref[2])] - ref[2][~torch.isnan(ref[2])]).abs().max()) < 1e-3
    p64 = O.frame_audio(bad[1:2].double(), cfg.n_fft, cfg.hop) * O.hann_window(cfg.n_fft).double()
    sp = torch.fft.rfft(p64, dim=-1)
    fb = O.mel_filterbank_htk(cfg.n_mels, cfg.n_fft, cfg.sample_rate, cfg.f_min, cfg.f_max).double()
    over = ((sp.real ** 2 + sp.imag ** 2) @ fb.T)[0] > 1e39          # a power beyond fp32: non-finite, never a finite number
    assert bool(over.any()) and not bool(torch.isfinite(mel[1][over]).any()) and not bool(torch.isfinite(ref[1][over]).any())
    assert torch.equal(mel[good], m.logmel(clean.cuda()).cpu()[good])

    aut = _random_automaton(cfg.vocab, seed=4, p=0.2)
    allowed = aut.allowed.copy()
    allowed[:, :7] = False
    aut = TokenAutomaton(allowed, aut.next)
    lowest = torch.from_numpy(np.argmax(aut.allowed, axis=1))
    nxt = torch.from_numpy(aut.next).long()
    c = m.compile_constraint(aut)
    starts = torch.tensor([[0], [1], [2], [1]])

    def constrained_rule(t):
        """an all-NaN row under a constraint: the lowest id its state allows, the state following it"""
        for r in ill:
            st = int(starts[r, 0])
            for tok in t[r, 0].tolist():
                assert tok == int(lowest[st]), (r, tok, st)
                st = int(nxt[st, tok])

    calls = {
        "inference": lambda a: (m.inference(a), None),
        "scored": lambda a: m.inference(a, return_scores=True),
        "constrained": lambda a: m.inference(a, return_scores=True, constraint=c, start_states=starts),
        "stream_constrained": lambda a: m.inference_stream(a, slots=3, interval=4, return_scores=True, constraint=c, start_states=starts),
        "stream": lambda a: (m.inference_stream(a, slots=2, interval=4), None),
    }
    for name, call in calls.items():
        ref_t, ref_s = call(clean.cuda())
        t, s = call(bad.cuda())                      # returns: YMT3_OK (anything else raises)
        t = t.cpu()
        assert torch.equal(t[good], ref_t.cpu()[good]), name
        assert int(t.min()) >= 0 and int(t.max()) < cfg.vocab, name
        if "constrained" in name:
            constrained_rule(t)
        else:
            assert int(t[ill].abs().max()) == 0, name
        if s is not None:
            assert torch.equal(s.cpu()[good], ref_s.cpu()[good]), name
            assert bool(torch.isnan(s.cpu()[ill]).all()), name
        again_t, again_s = call(clean.cuda())        # nothing sticks to the handle
        assert torch.equal(again_t, ref_t) and (s is None or torch.equal(again_s, ref_s)), name
    e = m.encode(m.logmel(bad.cuda()))
    assert bool(torch.isnan(e[ill].float()).all()) and bool(torch.isfinite(e[good].float()).all())
    t, lg = m.decode(e, 16, return_logits=True)
    assert bool(torch.isnan(lg[ill]).all()) and bool(torch.isfinite(lg[good]).all()) and int(t[ill].abs().max()) == 0
    c.close()
    m.close()
