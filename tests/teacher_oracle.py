"""The teacher-forced decoder as ONE full-sequence pass on the CPU oracle (include/ymt3.h, sequence scoring), built only from
oracle.ymt3_oracle's pieces.

With the ids given nothing is sequential: position 0 consumes pad_id, positions 1 .. P the prompt, position P + j + 1 tokens[j], and
all positions of a row go through the layers at once.  Self-attention is causal -- the mask is -inf folded into the by-distance
bias -- and, like the cross-attention, rounds its softmax numerators to bf16 (`attention(round_p=True)`, the MFMA kernels'
contract).  The step oracle (O.decoder_step) keeps them in f32: the two are different correct evaluation orders of one model, and
tests/test_score_pass_cpu.py pins this restatement to it within the project's parity tolerances.

`attention(round_p=True)` rounds exp(s - GLOBAL max).  dec_seq_attn_kernel streams the keys in tiles of 64 and rounds exp(s - the running
max after the current tile), then rescales both accumulators in fp32: the kernel's contract is that tile schedule
(tests/seq_kernel_model.py::attention_tiles).  The two are the same arithmetic only up to 64 keys; beyond, this
oracle is another correct evaluation order, compared within tolerances, never bit for bit.
"""
from typing import Optional

import torch

from oracle import ymt3_oracle as O


def teacher_forward(enc_out: torch.Tensor, W, cfg, tokens: torch.Tensor, prompt: Optional[torch.Tensor] = None, bf16: bool = True) -> torch.Tensor:
    """tokens (B, K, n) [+ prompt (B, K, P)] -> logits (B, K, n, V) of the emitted positions P .. P + n - 1."""
    B, K, H, V = enc_out.shape[0], cfg.n_channels, cfg.n_heads, cfg.vocab
    R = B * K
    tok = tokens.reshape(R, -1).long().clamp(0, V - 1)                  # clamped where they are fed, as the forced path does
    n = tok.shape[1]
    pr = (prompt.reshape(R, -1).long().clamp(0, V - 1) if prompt is not None else torch.zeros(R, 0, dtype=torch.long))
    P = pr.shape[1]
    L = P + n
    fed = torch.cat([torch.full((R, 1), cfg.pad_id, dtype=torch.long), pr, tok[:, :-1]], 1)       # (R, L)
    h = W["dec.embed"][fed]
    if K > 1:
        h = h + W["dec.chan_embed"][torch.arange(R) % K][:, None, :]
    h = h if h.dtype == torch.float64 else h.float()                    # (double weights: a float64 run with the same rounding points)
    dist = torch.arange(L)[:, None] - torch.arange(L)[None, :]          # query - key
    bias = O.decoder_bias_by_distance(W["dec.relbias"], L, cfg)[:, dist.clamp(min=0)]             # (H, L, L)
    bias = bias.masked_fill(dist < 0, float("-inf"))[None]
    ckv = O.cross_kv(enc_out, W, cfg, bf16)
    for l in range(cfg.n_dec_layers):
        p = f"dec.{l}."
        xn = O._r(O.rmsnorm(h, W[p + "ln1"], cfg.ln_eps), bf16)
        qkv = O._r(xn @ W[p + "wqkv"].T, bf16)
        q, k, v = (O.split_heads(x, H) for x in qkv.split(cfg.inner, dim=-1))
        a = O.merge_heads(O.attention(q, k, v, bias, bf16, round_p=True))
        h = h + a @ W[p + "wo"].T
        xn = O._r(O.rmsnorm(h, W[p + "ln2"], cfg.ln_eps), bf16)
        q = O.split_heads(O._r(xn @ W[p + "wq_c"].T, bf16), H)
        kc, vc = ckv[l]
        if K > 1:
            kc = kc.repeat_interleave(K, dim=0)
            vc = vc.repeat_interleave(K, dim=0)
        a = O.merge_heads(O.attention(q, kc, vc, None, bf16, round_p=True))
        h = h + a @ W[p + "wo_c"].T
        xn = O._r(O.rmsnorm(h, W[p + "ln3"], cfg.ln_eps), bf16)
        h = h + O.dense_ffn(xn, W, p, bf16)
    xn = O._r(O.rmsnorm(h, W["dec.ln_f"], cfg.ln_eps), bf16)
    return (xn @ W["dec.lm_head"].T)[:, P:].reshape(B, K, n, V)


def teacher_scores(logits: torch.Tensor, tokens: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, K, n, V) logits + (B, K, n) ids [+ (B, K) lengths] -> (B, K, n) float64: log_softmax(logits)[id clamped into [0, V)],
    exactly 0.0 in the columns at or past a row's length (clamped into [0, n])."""
    n = tokens.shape[-1]
    s = torch.log_softmax(logits.double(), -1).gather(-1, tokens.long().clamp(0, logits.shape[-1] - 1)[..., None])[..., 0]
    if lengths is not None:
        s = s.masked_fill(torch.arange(n) >= lengths.long().clamp(0, n)[..., None], 0.0)
    return s


def teacher_score(enc_out: torch.Tensor, W, cfg, tokens: torch.Tensor, prompt: Optional[torch.Tensor] = None,
                  lengths: Optional[torch.Tensor] = None, bf16: bool = True):
    """-> (scores (B, K, n) float64, logits (B, K, n, V))."""
    logits = teacher_forward(enc_out, W, cfg, tokens, prompt, bf16)
    return teacher_scores(logits, tokens, lengths), logits
