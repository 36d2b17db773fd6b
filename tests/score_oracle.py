"""Token scores on the CPU oracle (include/ymt3.h, token scores), built on the prompted oracle loop.

score[r][col] = log_softmax(logits of that step)[id], with id the id fed to the next step: the emitted token when nothing is
forced, forced[r][col] (clamped into [0, vocab)) when it is.  An unforced row that has already emitted EOS (eos_id >= 0)
scores its PAD columns 0.0.  The log-softmax runs in float64 over the oracle's logits.
"""
from typing import Optional

import torch

from prompt_oracle import prompted_greedy_decode


def scores_from_logits(logits: torch.Tensor, tokens: torch.Tensor, cfg, forced: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, K, n, V) logits + the (B, K, n) emitted tokens [+ forced ids] -> (B, K, n) float64 scores by the rules above."""
    lp = torch.log_softmax(logits.double(), -1)
    fed = (forced if forced is not None else tokens).long().clamp(0, logits.shape[-1] - 1)
    s = lp.gather(-1, fed[..., None])[..., 0]
    if forced is None and cfg.eos_id >= 0:
        eos = (tokens == cfg.eos_id).int()
        s = s.masked_fill((eos.cumsum(-1) - eos) > 0, 0.0)          # columns after the row's first EOS
    return s


def scored_greedy_decode(enc_out: torch.Tensor, W, cfg, n_steps: int, bf16: bool, prompt: Optional[torch.Tensor] = None,
                         forced: Optional[torch.Tensor] = None):
    """-> tokens (B, K, n_steps) int32, scores (B, K, n_steps) float64, logits (B, K, n_steps, V) of the (prompted) oracle loop."""
    if prompt is None:
        prompt = torch.zeros(enc_out.shape[0], cfg.n_channels, 0, dtype=torch.int32)
    toks, logits = prompted_greedy_decode(enc_out, W, cfg, prompt, n_steps, bf16, forced=forced, return_logits=True)
    return toks, scores_from_logits(logits, toks, cfg, forced), logits
