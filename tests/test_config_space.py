"""Parity across the model shapes ymt3_create accepts, not only the one shape the rest of the suite runs.

Every other GPU test runs vocab 1536, d_ff 2048, 6 + 6 layers, n_fft 2048, 128 mels, hop 128, 8 experts, ptf_d 128, 32/128
relative-position buckets and pad 0 / EOS 1.  Each config here changes one of those (plus whatever a second field needs to stay
valid) from BASE and is checked against the CPU oracle at the tolerances of the test_gpu_parity.py docstring:
  log-mel abs 1e-3, an empty filter exactly log(log_floor); encoder max 0.0625 / mean 4e-3 (Perceiver-TF: its own intrinsic bound);
  teacher-forced logits and ids (_check_ids, TAU = 0.03) over all max_decode_len positions; a free-running stream through
  _check_stream_prefix.
The decoder-side configs (vocab, d_ff, layers, attention tables, ids, MoE) run in every decode regime, each handle created under its
environment; a regime is proved taken by the launch counts of profile_decode, and for the merged kernels also by merged_fallbacks == 0
(asserted at close() by test_gpu_parity._model, which creates every handle here).  The mid-tile kernels have no launch counter of their
own (they count as the GEMM they replace): that regime is proved by its logits differing from the separate launches' at the same rows,
which only another summation order can do.  The regimes that promise the separate launches' bits are compared with them bit for bit.
Oracle results are cached per config, so the regimes share them.  Every check records its errors, safe fraction and regime in the
parity report.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from test_constraints import _masked_oracle_logits, _random_automaton
from constraint_oracle import constrained_greedy_decode
from test_gpu_parity import MIN_SAFE, TAU, _REPORT, _check_ids, _check_stream_prefix, _margin, _model, _moe_case
from yourmt3_amd.config import ENC_PERCEIVER_TF, FFN_MOE, YMT3Config
from yourmt3_amd.constraint import TokenAutomaton
from yourmt3_amd.weights import make_weights

pytestmark = pytest.mark.gpu

BASE = YMT3Config(segment_samples=8191, max_decode_len=48)
PTF = dict(encoder_type=ENC_PERCEIVER_TF, n_enc_layers=0)

# decoder-side configs: (id, changes from BASE)
DENSE = [
    ("vocab1024", dict(vocab=1024)),                 # GEMM chain on: 32 stage-3 column tiles
    ("vocab1056", dict(vocab=1056)),                 # 33 tiles (odd)
    ("vocab2048", dict(vocab=2048)),                 # 64 tiles
    ("vocab1040", dict(vocab=1040)),                 # chain off: not a multiple of 32 (16-column logits tail, partial mask word)
    ("vocab2080", dict(vocab=2080)),                 # chain off: 65 tiles
    ("vocab512", dict(vocab=512)),                   # chain off: 16 tiles
    ("dff512", dict(d_ff=512)),
    ("dff1024", dict(d_ff=1024)),                    # the decoder's FFN-out at K = 1024
    ("dec1", dict(n_dec_layers=1)),                  # layer 0's chain goes straight to the lm_head
    ("dec2", dict(n_dec_layers=2)),
    ("dec8", dict(n_dec_layers=8)),                  # the step kernel's limit
    ("dec9", dict(n_dec_layers=9)),                  # beyond it: the per-layer launches
    ("enc0", dict(n_enc_layers=0)),
    ("enc1", dict(n_enc_layers=1)),
    ("rel16", dict(rel_buckets=16, rel_max_distance=64)),
    ("len37", dict(max_decode_len=37)),              # KV cache slab / bias table pitch not a multiple of 16
    ("pad3_eos5", dict(pad_id=3, eos_id=5)),
    ("pad3_eos75", dict(pad_id=3, eos_id=75)),       # an EOS the streams do emit (steps 7 and 12): PAD fill, pad_tail, slots retiring
]
# (144 teacher-forced positions, as test_moe_fp8_expert_gemms_match_oracle: its bounds include the share of steps covered at TAU = 0.08,
# which 48 positions of 4 segments estimate too coarsely -- 0.69 for 16 experts, against 0.76 over 144)
MOE = [(f"moe_e{e}_{'fp8' if q else 'bf16'}", dict(dec_ffn=FFN_MOE, n_experts=e, moe_fp8=q, max_decode_len=160))
       for e in (2, 3, 9, 16) for q in (0, 1)]
# front-end / encoder / multi-channel configs: default regime only
FRONT = [
    ("nfft512_mels64", dict(n_fft=512, n_mels=64)),
    ("nfft512_mels128", dict(n_fft=512)),            # one empty filter (mel_len == 0)
    ("mels64", dict(n_mels=64)),                     # the input projection at K = 64
    ("mels256", dict(n_mels=256)),
    ("hop64", dict(hop=64, segment_samples=4095)),
    ("hop256", dict(hop=256, segment_samples=16383)),
    ("hop100", dict(hop=100, segment_samples=6300)),  # a hop that is not a power of two
    ("ptf_d256", dict(PTF, ptf_d=256)),
    ("ptf_mels64", dict(PTF, n_mels=64)),             # spectral cross-attention at Tk = n_mels
    ("ptf_mels256", dict(PTF, n_mels=256)),
    ("ptf_t128", dict(PTF, segment_samples=16383)),
    ("mc3_t256", dict(n_channels=3, segment_samples=32767)),
    ("mc13_t256", dict(n_channels=13, segment_samples=32767)),
    ("mc3_t512", dict(n_channels=3, segment_samples=65535)),
    ("mc13_t512", dict(n_channels=13, segment_samples=65535)),
]
ALL = DENSE + MOE + FRONT

SEPARATE = {"YMT3_NO_ATTN_PAIR": "1", "YMT3_NO_GEMM_CHAIN": "1"}
ENVS = {"merged": {}, "separate": SEPARATE, "step": {"YMT3_STEP_KERNEL": "1"},
        "mid": dict(SEPARATE, YMT3_DEC_GEMM_MID_ROWS="1"), "stream": {}}


def _cfg(kw):
    return BASE.with_(**kw)


def _chain_ok(cfg):
    """runtime.hip: the GEMM chain's shape (dense FFN of 2048, 32..64 lm_head column tiles of 32)"""
    return cfg.dec_ffn == 0 and cfg.d_ff == 2048 and cfg.vocab % 32 == 0 and 32 <= cfg.vocab // 32 <= 64


def _step_ok(cfg):
    return _chain_ok(cfg) and cfg.n_dec_layers <= 8


def _regimes(cfg):
    return [r for r in ENVS if r != "step" or _step_ok(cfg)]


def _create(cfg, env, monkeypatch, max_batch=4, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return _model(cfg, max_batch=max_batch, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


_ORACLE = {}


def _oracle(name, cfg):
    """audio, weights, oracle log-mel, oracle encoder output (bf16 arithmetic) and its free-running ids + logits, once per config"""
    if name not in _ORACLE:
        W = make_weights(cfg, seed=1234)
        a = O.synthetic_audio(2, cfg, seed=5)
        mel, enc = O.encode(a, W, cfg, True)
        t, lg = O.greedy_decode(enc, W, cfg, cfg.max_decode_len, True, return_logits=True)
        _ORACLE[name] = (a, W, mel, enc, t, lg)
    return _ORACLE[name]


_SEP = {}


def _separate(name, cfg, monkeypatch):
    """the separate launches' teacher-forced logits / ids and free-running ids: what the merged kernels must equal bit for bit"""
    if name not in _SEP:
        _, _, _, enc, ref_t, _ = _oracle(name, cfg)
        m = _create(cfg, SEPARATE, monkeypatch)
        e = enc.bfloat16().cuda()
        t, lg = m.decode(e, cfg.max_decode_len, forced=ref_t.cuda(), return_logits=True)
        _SEP[name] = (t.cpu(), lg.cpu(), m.decode(e, cfg.max_decode_len).cpu())
        m.close()
    return _SEP[name]


def _prove_regime(m, e, cfg, regime):
    """the launch counts of a short profiled decode show which kernels the handle runs"""
    p = {k: v["launches"] for k, v in m.profile_decode(e, 8, stride=4).items()}
    merged = cfg.n_channels == 1
    if regime in ("merged", "stream") and merged:
        assert p["attn_pair"] > 0 and p["self_attn"] == 0, p
        assert (p["gemm_chain"] > 0) == _chain_ok(cfg), p
        assert p["step_layers"] == 0, p
    elif regime == "step":
        assert p["step_layers"] > 0, p
    elif regime in ("separate", "mid"):
        assert p["attn_pair"] == 0 and p["gemm_chain"] == 0 and p["step_layers"] == 0 and p["self_attn"] > 0, p
    return {k: v for k, v in p.items() if v}


def _check_front(name, cfg, m):
    """log-mel and encoder output against the oracle"""
    a, W, mel_ref, enc_ref, _, _ = _oracle(name, cfg)
    mel = m.logmel(a.cuda()).cpu()
    assert mel.shape == (2, cfg.n_frames, cfg.n_mels)
    d_mel = (mel - mel_ref).abs().max().item()
    fb = O.mel_filterbank_htk(cfg.n_mels, cfg.n_fft, cfg.sample_rate, cfg.f_min, cfg.f_max)
    empty = ((fb > 0).sum(1) == 0).nonzero().flatten()
    for i in empty.tolist():                     # no bin feeds it: the floor, exactly
        floor = torch.log(torch.tensor(cfg.log_floor, dtype=torch.float32))
        assert torch.equal(mel_ref[..., i], torch.full_like(mel_ref[..., i], floor.item())), i
        assert torch.equal(mel[..., i], mel_ref[..., i]), i
    enc = m.encode(mel.cuda()).float().cpu()
    d = (enc - enc_ref).abs()
    rec = {"logmel_max_abs": d_mel, "empty_filters": len(empty), "enc_max_abs": float(d.max()), "enc_mean_abs": float(d.mean())}
    assert d_mel < 1e-3, rec
    if cfg.encoder_type == ENC_PERCEIVER_TF:
        # as test_perceiver_tf_encoder_matches_oracle: the oracle's own fp32-vs-double spread at this shape, times 1.25
        from oracle.perceiver_oracle import encoder_perceiver_tf, in_double
        intrinsic = (encoder_perceiver_tf(mel_ref.double(), in_double(W), cfg, True).float() - enc_ref).abs()
        rec["oracle_fp32_vs_fp64_mean_abs"] = float(intrinsic.mean())
        assert d.max().item() <= 0.0625 and d.mean().item() <= 1.25 * intrinsic.mean().item() + 1e-4, rec
    else:
        assert d.max().item() <= 0.0625 and d.mean().item() <= 4e-3, rec
    return rec


def _check_decoder(name, cfg, m, regime):
    """teacher-forced logits / ids, a free-running stream, one segment alone == inside the batch"""
    _, _, _, enc, ref_t, ref_l = _oracle(name, cfg)
    L = cfg.max_decode_len
    e = enc.bfloat16().cuda()
    got_t, got_l = m.decode(e, L, forced=ref_t.cuda(), return_logits=True)
    rec = _check_ids(f"config_{name}_{regime}", got_t, ref_t, ref_l, got_l)
    free = m.decode(e, L).cpu()
    _check_stream_prefix(free, ref_t, _margin(ref_l))
    assert torch.equal(m.decode(e[1:2], L).cpu(), free[1:2])
    assert int(free.min()) >= 0 and int(free.max()) < cfg.vocab
    return rec, got_t.cpu(), got_l.cpu(), free


def _stream(m, cfg):
    """continuous batching against the lock-step call, and the end-to-end call against its stages"""
    a = O.synthetic_audio(3, cfg, seed=21).cuda()
    lock = m.inference(a)
    assert torch.equal(lock, m.decode(m.encode(m.logmel(a))))
    for slots, interval in ((1, 4), (2, 3)):
        assert torch.equal(m.inference_stream(a, slots=slots, interval=interval), lock), (slots, interval)


@pytest.mark.parametrize("name,kw,regime", [(n, kw, r) for n, kw in DENSE for r in _regimes(_cfg(kw))],
                         ids=[f"{n}-{r}" for n, kw in DENSE for r in _regimes(_cfg(kw))])
def test_dense_decoder_configs_in_every_regime(name, kw, regime, monkeypatch):
    cfg = _cfg(kw)
    _, _, _, enc, _, _ = _oracle(name, cfg)
    m = _create(cfg, ENVS[regime], monkeypatch)
    e = enc.bfloat16().cuda()
    taken = _prove_regime(m, e, cfg, regime)
    if regime == "stream":
        _stream(m, cfg)
        _REPORT[f"config_{name}_stream"] = {"regime": taken}
    else:
        rec, t, lg, free = _check_decoder(name, cfg, m, regime)
        rec["regime"] = taken
        if regime == "merged":
            rec.update(_check_front(name, cfg, m))
        if regime == "separate":
            _SEP.setdefault(name, (t, lg, free))
        sep_t, sep_l, sep_free = _separate(name, cfg, monkeypatch)
        if regime in ("merged", "step"):                 # the merged kernels promise the separate launches' bits
            assert torch.equal(t, sep_t) and torch.equal(lg, sep_l) and torch.equal(free, sep_free)
        if regime == "mid":                              # other tiles, other summation order: proves the mid-tile kernels ran
            assert not torch.equal(lg, sep_l)
    m.close()


@pytest.mark.parametrize("name,kw,regime", [(n, kw, r) for n, kw in MOE for r in ("merged", "separate", "mid", "stream")],
                         ids=[f"{n}-{r}" for n, kw in MOE for r in ("merged", "separate", "mid", "stream")])
def test_moe_decoder_configs_in_every_regime(name, kw, regime, monkeypatch):
    """E != 8 takes the five separate MoE launches (the MoE chain is E = 8 only) and the router's second pass over experts 8..15
    where E > 8.  Parity through _moe_case (the router's recorded choices fed to the oracle), fp8 at the bounds of
    test_moe_fp8_expert_gemms_match_oracle; the attention pair against the separate launches bit for bit."""
    cfg = _cfg(kw)
    n = 144
    if regime == "stream":
        m = _create(cfg, {}, monkeypatch)
        _prove_regime(m, m.encode(m.logmel(O.synthetic_audio(2, cfg).cuda())), cfg, regime)
        _stream(m, cfg)
        m.close()
        return
    for k, v in ENVS[regime].items():
        monkeypatch.setenv(k, v)
    try:
        if cfg.moe_fp8:
            m = _moe_case(cfg, n, 0.08, 8e-3, 0.08, 0.04, monkeypatch)
        else:
            m = _moe_case(cfg, n, 0.06, 6e-3, TAU, 0.01, monkeypatch, min_safe=MIN_SAFE)
    finally:
        for k in ENVS[regime]:
            monkeypatch.delenv(k)
    _REPORT[f"moe_fp8{cfg.moe_fp8}_{n}_steps_routing_teacher_forced"]["config"] = name
    _REPORT[f"config_{name}_{regime}"] = _REPORT.pop(f"moe_fp8{cfg.moe_fp8}_{n}_steps_routing_teacher_forced")
    a = O.synthetic_audio(4, cfg, seed=31).cuda()
    e = m.encode(m.logmel(a))
    _REPORT[f"config_{name}_{regime}"]["regime"] = _prove_regime(m, e, cfg, regime)
    t, lg = m.decode(e, 48, return_logits=True)
    assert torch.equal(m.decode(e[2:3], 48), t[2:3])
    if regime in ("merged", "mid"):
        sep = _create(cfg, SEPARATE, monkeypatch)
        s_t, s_l = sep.decode(e, 48, return_logits=True)
        if regime == "merged":                           # the attention pair promises the separate launches' bits
            assert torch.equal(t, s_t) and torch.equal(lg, s_l)
        else:                                            # other tiles, other summation order: the mid-tile kernels ran
            assert not torch.equal(lg, s_l)
        sep.close()
    m.close()


@pytest.mark.parametrize("name,kw", FRONT, ids=[f[0] for f in FRONT])
def test_front_end_encoder_and_channel_configs(name, kw, monkeypatch):
    cfg = _cfg(kw)
    m = _create(cfg, {}, monkeypatch)
    rec = _check_front(name, cfg, m)
    r2, _, _, _ = _check_decoder(name, cfg, m, "default")
    r2.update(rec)
    _, _, _, enc, _, _ = _oracle(name, cfg)
    r2["regime"] = _prove_regime(m, enc.bfloat16().cuda(), cfg, "merged")
    if cfg.n_channels == 1:
        _stream(m, cfg)
    m.close()


def test_constrained_decode_with_a_partial_mask_word():
    """vocab 1040: the constraint's last mask word holds 16 tokens; state 0 allows only three ids, 1039 among them"""
    cfg = _cfg(dict(vocab=1040, eos_id=-1))
    V = cfg.vocab
    base = _random_automaton(V, seed=8, p=0.4)
    allowed = base.allowed.copy()
    allowed[:, V - 1] = True
    allowed[0] = False
    allowed[0, [17, 1030, V - 1]] = True
    aut = TokenAutomaton(allowed, base.next)
    m = _model(cfg, max_batch=2)
    a = O.synthetic_audio(2, cfg, seed=3)
    _, enc = O.encode(a, m.weights, cfg, True)
    starts = torch.tensor([[0], [1]])
    n = cfg.max_decode_len
    feed, _, _ = constrained_greedy_decode(enc, m.weights, cfg, n, True, aut, start_states=starts)
    ref_t, _, ref_l = constrained_greedy_decode(enc, m.weights, cfg, n, True, aut, start_states=starts, forced=feed)
    assert int((ref_t == V - 1).sum()) > 0                    # the partial word's last bit is exercised
    c = m.compile_constraint(aut)
    got_t = m.decode(enc.bfloat16().cuda(), n, forced=feed.cuda(), constraint=c, start_states=starts)
    _check_ids("config_vocab1040_constrained_teacher_forced", got_t, ref_t, _masked_oracle_logits(aut, ref_l, feed, starts))
    free = m.decode(enc.bfloat16().cuda(), n, constraint=c, start_states=starts).cpu()
    for b in range(2):
        st = int(starts[b, 0])
        for tok in free[b, 0].tolist():
            assert aut.allows(st, tok), (b, tok, st)
            st = int(aut.next[st, tok])
    c.close()
    m.close()


def _create_rc(cfg):
    from yourmt3_amd import _lib
    from yourmt3_amd.config import to_c
    from yourmt3_amd.tables import derived_tables
    from yourmt3_amd.weights import pack_blob
    lib = _lib.load()
    W = make_weights(cfg)
    blob = pack_blob({**W, **derived_tables(W, cfg)})
    h = ctypes.c_void_p()
    cc = to_c(cfg, 2)
    rc = lib.ymt3_create(ctypes.byref(cc), ctypes.create_string_buffer(blob, len(blob)), len(blob), 0, ctypes.byref(h))
    if rc == 0:
        lib.ymt3_destroy(h)
    return rc, lib.ymt3_last_error().decode()


@pytest.mark.parametrize("kw,field", [
    (dict(segment_samples=24575), "n_frames"),                     # 192 frames: no encoder attention kernel
    (dict(segment_samples=16383 + 8192 * 4), "n_frames"),          # 384 frames
    (dict(PTF, segment_samples=24575), "n_frames"),                # 192 frames: no Perceiver-TF temporal attention kernel
    (dict(PTF, segment_samples=65535), "n_frames"),                # 512 frames (refused before too, now by the same early check)
    (dict(hop=512, segment_samples=32767), "hop"),                 # 64 frames of 512 samples
    (dict(hop=125, segment_samples=7875), "hop"),                  # odd: frames would start at odd sample offsets
    (dict(d_ff=1536), "d_ff"),                                     # no decoder FFN-out kernel at K = 1536
    (dict(d_ff=256), "d_ff"),
    (dict(n_fft=1024), "n_fft"),                                   # (refused before too, now before the blob is parsed)
], ids=["t192", "t384", "ptf_t192", "ptf_t512", "hop512", "hop125", "dff1536", "dff256", "nfft1024"])
def test_unrunnable_shapes_are_rejected_at_create(kw, field):
    rc, msg = _create_rc(_cfg(kw))
    assert rc == 4 and field in msg, (rc, msg)


def test_every_config_creates_and_runs_end_to_end():
    """every config of the tables above: create, then log-mel -> encode -> decode without an error"""
    for name, kw in ALL:
        cfg = _cfg(kw)
        m = _model(cfg, max_batch=1)
        a = O.synthetic_audio(1, cfg, seed=2).cuda()
        t = m.decode(m.encode(m.logmel(a)), 8)
        assert t.shape == (1, cfg.n_channels, 8) and int(t.min()) >= 0 and int(t.max()) < cfg.vocab, name
        m.close()
