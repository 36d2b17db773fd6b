"""Weight and value regimes for tests/test_value_space.py and tests/test_value_space_cpu.py.  TEST INFRASTRUCTURE ONLY.

Every regime is an edit of make_weights output that keeps each tensor bf16-exact where the blob stores bf16 (factors are powers of
two; rows are copied, negated or zeroed).  The reference quantities the bounds are built from come from the oracle alone:

  std        the std of the oracle's teacher-forced logits (fp32 accumulation): every logits error and TAU are in units of it
  intrinsic  the oracle's fp32 evaluation against the same oracle with every sum in double (same bf16 rounding points, same fed ids):
             what two correct implementations of the model may differ by, in std units, max and mean
  bound      the project's contract for its standard model (logits max 0.06, mean 6e-3, TAU 0.03; encoder max 0.0625, mean 4e-3) times
             max(1, intrinsic_regime / intrinsic_standard), max with max and mean with mean: the margin granted to the standard
             model, never more, and never a bound below the reference's own noise in a regime that is intrinsically noisier.
"""
from __future__ import annotations

import re

import torch

from oracle import ymt3_oracle as O
from oracle.perceiver_oracle import encoder_perceiver_tf, in_double
from yourmt3_amd.config import ENC_PERCEIVER_TF, YMT3Config
from yourmt3_amd.weights import make_weights

CFG = YMT3Config(segment_samples=8191, max_decode_len=64)
SEGMENTS = 4
AUDIO_SEED = 5
TOL_MAX, TOL_MEAN, TAU = 0.06, 6e-3, 0.03            # logits, in units of their std (tests/test_gpu_parity.py)
ENC_MAX, ENC_MEAN = 0.0625, 4e-3                     # encoder output, in units of its RMS
MIN_SAFE = 0.8
REGIMES = ["std", "seed7", "seed99", "big", "tiny", "neg_gain", "bias40", "crossq8", "selfqk2", "dead_relu"]
DEAD_LAYER, DEAD_CHANNEL, DEAD_LEVEL = 3, 77, 64.0

_OUT = re.compile(r"\.(wo|wo_c|wo2)$")
# what feeds the residual streams: scaled together with the output projections in `big` / `tiny`
_SOURCES = ("dec.embed", "dec.chan_embed", "in_proj.w", "ptf.spec_w", "ptf.spec_pos", "ptf.latents", "ptf.out_w")


def _is_gain(name):
    return name.rsplit(".", 1)[-1].startswith("ln")


def _scale_streams(W, f, bias):
    for k in list(W):
        if k in _SOURCES or _OUT.search(k) or (bias and k == "in_proj.b"):
            W[k] = W[k] * f
        elif k.endswith(".wo2_s"):                    # fp8 experts: the output projection's per-expert scale carries the factor
            W[k] = W[k] * f


def regime_weights(cfg, name, seed=1234):
    """the weights of regime `name` for `cfg` (any config make_weights accepts)"""
    if name.startswith("seed"):
        return make_weights(cfg, seed=int(name[4:]))
    W = {k: v.clone() for k, v in make_weights(cfg, seed=seed).items()}
    if name == "std":
        pass
    elif name == "big":
        _scale_streams(W, 256.0, bias=False)
    elif name == "tiny":
        _scale_streams(W, 2.0 ** -20, bias=True)
    elif name == "neg_gain":
        for k in W:
            if _is_gain(k):
                W[k] = -W[k]
        g = W["dec.1.ln2"]
        g[5:40:7] = 0.0
        g[300:340:5] = -0.0
    elif name == "bias40":
        for k in W:
            if k.endswith("relbias"):
                W[k] = W[k] * 40.0
    elif name == "crossq8":
        for k in W:
            if k.endswith(".wq_c"):
                W[k] = W[k] * 8.0
    elif name == "selfqk2":
        for k in W:
            if k.endswith(".wqkv"):
                W[k][: W[k].shape[0] // 3] *= 2.0
    elif name == "dead_relu":
        # Channel DEAD_CHANNEL of the decoder's residual stream is made a constant: every token embeds DEAD_LEVEL there and no
        # output projection writes to it.  Layer DEAD_LAYER's ln3 gain is positive there and its wi weighs that channel by -32 in
        # every row: every pre-activation is about -300 against a spread of a few units, so the ReLU output is exactly 0.
        j, p = DEAD_CHANNEL, f"dec.{DEAD_LAYER}."
        W["dec.embed"][:, j] = DEAD_LEVEL
        if "dec.chan_embed" in W:
            W["dec.chan_embed"][:, j] = 0.0
        for k in W:
            if k.startswith("dec.") and _OUT.search(k):
                W[k].view(-1, cfg.d_model, W[k].shape[-1])[:, j] = 0.0
        W[p + "ln3"][j] = 1.0
        W[p + "wi"][:, j] = -32.0
    else:
        raise KeyError(name)
    return W


def dup_head(cfg, W, distinct=48):
    """An lm_head whose rows are 48 distinct rows, each copied 30 or 36 times.  With the argmax kernel's layout (thread tid scans the
    columns tid + 256 k; 16 lanes to a DPP row, 4 rows to a wave, 4 waves) and the GEMM chain's 32-column tiles, group
        (i >> 1 & 7) + 8 * (3 * (k & 1) + (row + wave) % 3),   k = i / 256, row = i >> 4 & 3, wave = i >> 6 & 3
    puts copies of one row at i and i + 1 (two lanes of a DPP row), i and i + 512 (one thread's stride), at other DPP rows of one
    wave, at other waves, and in other column tiles; the groups of the first tile (columns 0..31) and of the last (1504..1535)
    win at some steps too (asserted on the CPU).  Returns (weights with the new head, group of every column)."""
    V = cfg.vocab
    i = torch.arange(V)
    grp = ((i >> 1) & 7) + 8 * (3 * ((i // 256) & 1) + (((i >> 4) & 3) + ((i >> 6) & 3)) % 3)
    assert int(grp.max()) == distinct - 1
    W = dict(W)
    W["dec.lm_head"] = W["dec.lm_head"][:distinct][grp].contiguous()
    return W, grp


def tie_relations(i, j):
    """how two tied columns i < j relate in the argmax kernel / GEMM chain"""
    rel = set()
    if i % 256 == j % 256:
        rel.add("stride")
    if i // 16 == j // 16:
        rel.add("lanes")
    if i // 256 == j // 256 and i // 64 == j // 64 and i // 16 != j // 16:
        rel.add("dpp_rows")
    if i // 256 == j // 256 and i // 64 != j // 64:
        rel.add("waves")
    if i // 32 != j // 32:
        rel.add("tiles")
    if i < 32:
        rel.add("first_tile")
    if j >= 1504:
        rel.add("last_tile")
    return rel


def audio(cfg=CFG, n=SEGMENTS):
    return O.synthetic_audio(n, cfg, seed=AUDIO_SEED)


def oracle_encode(a, W, cfg, double=False):
    """(log-mel, encoder output); double: every encoder sum in double from the fp32 log-mel, same rounding points"""
    mel = O.logmel(a, cfg)
    if not double:
        return mel, O.encode(a, W, cfg, True)[1]
    Wd = in_double(W)
    if cfg.encoder_type == ENC_PERCEIVER_TF:
        return mel, encoder_perceiver_tf(mel.double(), Wd, cfg, True)
    return mel, O.encoder_t5(O.input_projection(mel.double(), Wd, True), Wd, cfg, True)


def tiny_feed(shape, cfg, seed=3):
    """what `tiny` is teacher-forced with (oracle_case): uniform random ids"""
    return torch.randint(0, cfg.vocab, tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


_CASES = {}


def oracle_case(name, cfg=CFG, W=None, n_steps=None, segments=SEGMENTS, key=None):
    """Everything the oracle alone says about one regime, cached: audio, weights, log-mel, encoder output, the free-running ids
    and their logits, the fed ids with the teacher-forced ids and logits (fp32 sums), the logits' std, and the fp32-vs-double
    figures of encoder and logits (in RMS / std units).  The fed ids are the regime's own free-running stream, except under `tiny`:
    there a step's logits depend on little but the token fed (everything behind the embedding is 2^-20 of it), the free stream
    falls into a short cycle of ids whose margins are whatever that cycle holds (0.77 of the steps above TAU), so `tiny` is fed
    seeded random ids (tiny_feed) instead; its own free stream is still run and compared as a stream."""
    key = key or (name, cfg, n_steps, segments)
    if key in _CASES:
        return _CASES[key]
    W = regime_weights(cfg, name) if W is None else W
    n = n_steps or cfg.max_decode_len
    a = audio(cfg, segments)
    mel, enc = oracle_encode(a, W, cfg)
    free_t, free_l = O.greedy_decode(enc, W, cfg, n, True, return_logits=True)
    if name == "tiny":
        feed = tiny_feed(free_t.shape, cfg)
        t, lg = O.greedy_decode(enc, W, cfg, n, True, forced=feed, return_logits=True)
    else:
        feed, t, lg = free_t, free_t, free_l
    std = float(lg.std())
    _, enc64 = oracle_encode(a, W, cfg, double=True)
    _, lg64 = O.greedy_decode(enc.double(), in_double(W), cfg, n, True, forced=feed, return_logits=True)
    d = (lg64.float() - lg).abs() / std
    rms = float(enc.pow(2).mean().sqrt())
    de = (enc64.float() - enc).abs() / rms
    c = dict(name=name, cfg=cfg, W=W, audio=a, mel=mel, enc=enc, feed=feed, ids=t, logits=lg, free_ids=free_t, free_logits=free_l,
             std=std, enc_rms=rms, intrinsic_max=float(d.max()), intrinsic_mean=float(d.mean()),
             enc_intrinsic_max=float(de.max()), enc_intrinsic_mean=float(de.mean()),
             finite=bool(torch.isfinite(lg).all() and torch.isfinite(enc).all()))
    _CASES[key] = c
    return c


def bounds(case, standard):
    """the bounds of `case` from the standard model's contract and the two intrinsic figures (module docstring); tau in logit units"""
    f_max = max(1.0, case["intrinsic_max"] / standard["intrinsic_max"])
    f_mean = max(1.0, case["intrinsic_mean"] / standard["intrinsic_mean"])
    e_max = max(1.0, case["enc_intrinsic_max"] / standard["enc_intrinsic_max"])
    e_mean = max(1.0, case["enc_intrinsic_mean"] / standard["enc_intrinsic_mean"])
    return dict(tol_max=TOL_MAX * f_max, tol_mean=TOL_MEAN * f_mean, tau_std=TAU * f_max, tau=TAU * f_max * case["std"],
                enc_max=ENC_MAX * e_max, enc_mean=ENC_MEAN * e_mean, std=case["std"],
                intrinsic_max=case["intrinsic_max"], intrinsic_mean=case["intrinsic_mean"],
                intrinsic_standard_max=standard["intrinsic_max"], intrinsic_standard_mean=standard["intrinsic_mean"])


def margin(logits):
    t = logits.topk(2, -1).values
    return t[..., 0] - t[..., 1]


def safe_fraction(case, b):
    return float((margin(case["logits"]) >= b["tau"]).float().mean())


def logits_error(got, ref, std):
    """(max, mean) abs error in units of the oracle logits' std"""
    d = (got.float() - ref).abs() / std
    return float(d.max()), float(d.mean())


# ----------------------------------------------------------------------------- GEMM operands that are not randn
GEMM_KINDS = ["cancel", "negative", "scale_up", "scale_down", "scale_mixed", "signed_zeros", "subnormal"]


def gemm_operands(kind, M, N, K, seed=0):
    """bf16 operands A (M, K), W (N, K) for ymt3_test_gemm (out = A W^T, fp32 accumulation):
      cancel        columns in pairs (+a, -a) of about 1e4 against equal weights, and 16 columns of a small remainder that is the result
      negative      every element of both operands negative
      scale_up / scale_down / scale_mixed   operands times 2^60 / 2^-60 / one of each (products near 2^-120: partial products reach
                    the fp32 subnormals)
      signed_zeros  a third of the elements +0, a third -0
      subnormal     A holds bf16 subnormals (below 2^-126), W is about 2^100: nothing may be flushed on either side"""
    g = torch.Generator().manual_seed(seed + M + N + K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    if kind == "cancel":
        a = (1e4 * (1 + torch.rand(M, (K - 16) // 2, generator=g))).bfloat16().float()
        A[:, 0:K - 16:2], A[:, 1:K - 16:2] = a, -a
        W[:, 1:K - 16:2] = W[:, 0:K - 16:2]
        A[:, K - 16:] *= 1e-2
    elif kind == "negative":
        A, W = -A.abs() - 0.01, -W.abs() - 0.01
    elif kind == "scale_up":
        A = A * 2.0 ** 60
    elif kind == "scale_down":
        A, W = A * 2.0 ** -60, W * 2.0 ** -60
    elif kind == "scale_mixed":
        A, W = A * 2.0 ** 60, W * 2.0 ** -60
    elif kind == "signed_zeros":
        for X in (A, W):
            u = torch.rand(X.shape, generator=g)
            X[u < 1 / 3] = 0.0
            X[u > 2 / 3] = -0.0
    elif kind == "subnormal":
        A, W = A * 2.0 ** -130, W * 2.0 ** 100
    else:
        raise KeyError(kind)
    return A.bfloat16(), W.bfloat16()


def gemm_reference_and_bound(A, W):
    """The fp64 product of the bf16 values, and the bound an fp32-accumulated dot product of length K meets in ANY summation order:
    the products of two bf16 values are exact in fp32 (16 significant bits), each of at most K - 1 additions rounds its partial sum by
    at most 2^-24 relative, and no partial sum exceeds sum |a_k| |w_k|, so |error| <= K 2^-24 sum |a_k| |w_k|; where products or sums
    fall below 2^-126 a rounding is at most the subnormal spacing 2^-149 instead, K of them at the most."""
    K = A.shape[1]
    A64, W64 = A.double(), W.double()
    return A64 @ W64.T, K * 2.0 ** -24 * (A64.abs() @ W64.abs().T) + K * 2.0 ** -149


def mixed_norm_head(cfg, W):
    """The lm_head with row i times 2^(i % 4).  At the fp8 MoE's TAU of 0.08 std the plain head leaves the id check about 0.72 of the
    steps whatever the stream (1536 near-Gaussian logits: the top-2 gap is below 0.08 std at a fixed rate; the oracle alone gives
    0.64-0.77 over regimes and audio seeds), which no draw holds above the 0.7 cap reliably.  With rows of four norms the maximum
    comes from the 384 largest rows while the std is set by all: 0.86-0.90 of the steps are covered, from the oracle alone."""
    W = dict(W)
    W["dec.lm_head"] = W["dec.lm_head"] * (2.0 ** (torch.arange(cfg.vocab) % 4))[:, None]
    return W
