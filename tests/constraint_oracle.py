"""The constrained greedy loop on the CPU oracle (include/ymt3.h, constraints), built from oracle.ymt3_oracle's own pieces in the
way prompt_oracle.py builds the prompted loop.

At every emitted position a live row in state s emits the first maximum of its logits over the tokens allowed[s]; with f the
fed id (the emitted token, or forced[...] clamped into [0, V)) its state becomes next[s][f].  Prompt positions neither mask
nor advance the state.  With eos_id >= 0 a row that has emitted EOS emits PAD and its state stays frozen.  A score is the
log_softmax of the masked row (disallowed tokens -inf) at f, in float64; an unforced row after its EOS scores 0.0.
"""
from typing import Optional

import torch

from oracle import ymt3_oracle as O


def constrained_greedy_decode(enc_out: torch.Tensor, W, cfg, n_steps: int, bf16: bool, automaton, start_states=None,
                              prompt: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None):
    """-> tokens (B, K, n_steps) int32, scores (B, K, n_steps) float64, raw logits (B, K, n_steps, V).  `start_states`: None
    (state 0), (K,) or (B, K); `prompt` (B, K, P); `forced` (B, K, n_steps)."""
    B, K = enc_out.shape[0], cfg.n_channels
    R = B * K
    allowed = torch.from_numpy(automaton.allowed)
    nxt = torch.from_numpy(automaton.next).long()
    if start_states is None:
        state = torch.zeros(R, dtype=torch.long)
    else:
        state = torch.as_tensor(start_states).long().expand(B, K).reshape(R).clone()
    P = 0 if prompt is None else int(prompt.shape[-1])
    pr = None if prompt is None else prompt.reshape(R, P).long()
    ckv = O.cross_kv(enc_out, W, cfg, bf16)
    dstate = O.DecoderState(R, cfg)
    cur = torch.full((R,), cfg.pad_id, dtype=torch.long)
    for t in range(P):
        O.decoder_step(cur, dstate, ckv, W, cfg, bf16)           # a prompt position: nothing emitted, the automaton waits
        cur = pr[:, t]
    finished = torch.zeros(R, dtype=torch.bool)
    out = torch.zeros(R, n_steps, dtype=torch.int32)
    scores = torch.zeros(R, n_steps, dtype=torch.float64)
    all_logits = []
    V = cfg.vocab
    rows = torch.arange(R)
    for t in range(n_steps):
        logits = O.decoder_step(cur, dstate, ckv, W, cfg, bf16).float()
        mask = allowed[state]
        masked = logits.masked_fill(~mask, float("-inf"))
        nxt_tok = torch.argmax(masked, dim=-1)                   # the first maximum among the allowed tokens
        was_finished = finished.clone()
        if cfg.eos_id >= 0:
            nxt_tok = torch.where(finished, torch.full_like(nxt_tok, cfg.pad_id), nxt_tok)
            finished = finished | (nxt_tok == cfg.eos_id)
        out[:, t] = nxt_tok.to(torch.int32)
        all_logits.append(logits.clone())
        fed = forced.reshape(R, -1)[:, t].long().clamp(0, V - 1) if forced is not None else nxt_tok
        s = torch.log_softmax(masked.double(), -1)[rows, fed]
        if forced is None and cfg.eos_id >= 0:
            s = torch.where(was_finished, torch.zeros_like(s), s)
        scores[:, t] = s
        live = ~was_finished if cfg.eos_id >= 0 else torch.ones(R, dtype=torch.bool)
        state = torch.where(live, nxt[state, fed], state)
        cur = fed
    return (out.view(B, K, n_steps), scores.view(B, K, n_steps), torch.stack(all_logits, 1).view(B, K, n_steps, V))
