"""The prompted greedy loop on the CPU oracle (task prompts, include/ymt3.h), built from oracle.ymt3_oracle's own pieces.

Step 0 consumes the decoder start id (pad_id); steps 0 .. P-1 feed prompt[r][t] instead of their argmax and emit nothing; the
argmax of step P + j is emitted token j -- the alignment of HF `generate(decoder_input_ids=[[pad, *prompt]])`.
"""
from typing import Optional

import torch

from oracle import ymt3_oracle as O


def prompted_greedy_decode(enc_out: torch.Tensor, W, cfg, prompt: torch.Tensor, n_steps: int, bf16: bool,
                           forced: Optional[torch.Tensor] = None, return_logits: bool = False):
    """prompt (B, K, P) ids -> tokens (B, K, n_steps) int32 [, logits (B, K, n_steps, V)]: the emitted steps only.  `forced`
    (B, K, n_steps) teacher-forces the ids fed back after the emitted steps, as in O.greedy_decode."""
    B, K = enc_out.shape[0], cfg.n_channels
    R, P = B * K, int(prompt.shape[-1])
    pr = prompt.reshape(R, P).long()
    ckv = O.cross_kv(enc_out, W, cfg, bf16)
    state = O.DecoderState(R, cfg)
    cur = torch.full((R,), cfg.pad_id, dtype=torch.long)
    for t in range(P):
        O.decoder_step(cur, state, ckv, W, cfg, bf16)            # a prompt position: its logits are not emitted
        cur = pr[:, t]
    finished = torch.zeros(R, dtype=torch.bool)
    out = torch.zeros(R, n_steps, dtype=torch.int32)
    all_logits = []
    for t in range(n_steps):
        logits = O.decoder_step(cur, state, ckv, W, cfg, bf16)
        nxt = torch.argmax(logits.float(), dim=-1)
        if cfg.eos_id >= 0:
            nxt = torch.where(finished, torch.full_like(nxt, cfg.pad_id), nxt)
            finished = finished | (nxt == cfg.eos_id)
        out[:, t] = nxt.to(torch.int32)
        if return_logits:
            all_logits.append(logits.clone())
        cur = forced.reshape(R, -1)[:, t].long() if forced is not None else nxt
    toks = out.view(B, K, n_steps)
    if return_logits:
        return toks, torch.stack(all_logits, 1).view(B, K, n_steps, -1)
    return toks
