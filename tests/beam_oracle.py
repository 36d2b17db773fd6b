"""Beam search on the CPU oracle (include/ymt3.h, beam search), built from oracle.ymt3_oracle's own pieces in the way
constraint_oracle.py builds the constrained loop: HF `GenerationMixin._beam_search` (transformers 5.x) with do_sample=False,
early_stopping=True, one EOS id, restated per group g = (segment, channel).

Rows are r = g * W + w.  `DecoderState.k / v` are per-row tensors, so a step's new beams take their history by indexing the cache with
their parents' rows (HF reorder_cache).  The oracle's decoder_step maps row r to channel r % n_channels and to segment r // n_channels;
with beams a segment has K * W rows, so the step runs under a view of the config with n_channels = K * W and a channel-embedding table
repeated W times per channel (a table of zeros for the one-channel decoder: x + 0.0 is x).

All search arithmetic is float64: lp = log_softmax(logits.double()) (masked by the beam's automaton state), run[w] cumulative.

`forced_trace` (n_steps, G, W, 2) int = (parent, token): the new running beams of every step are these instead of the oracle's own
choice, and their run values are the oracle's own scores of them -- so a device's discrete choices can be fed to the oracle and every
step compared (the way the MoE router's choices are).  Finished slots are then still the oracle's own (from its own candidates).
"""
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from oracle import ymt3_oracle as O

NEG = -1.0e9


class _CfgView:
    """cfg with n_channels replaced (the oracle's decoder_step reads rows-per-segment and the channel index from it)."""

    def __init__(self, cfg, n_channels):
        self._cfg, self.n_channels = cfg, n_channels

    def __getattr__(self, name):
        return getattr(self._cfg, name)


def host_select(acc: np.ndarray, W: int, eos_id: int, at_limit: bool, fin: list, length: int, alpha: float, forced=None):
    """Steps 2-7 of the semantics for one group on the host, float64.  acc: (W, V), NaN / -inf entries allowed (-inf = no candidate,
    NaN ranks at NEG).  fin: the group's finished slots, a list of dicts (score, len, parent, token, acc), best first, at most W.
    -> dict(cand=[(flat, acc)] the 2W candidates in order, beams=[(parent, token, run)] the next running beams (forced: the given ones
    with the host's scores), entered=[candidate indices that entered], fin=new slots, done=bool, kmod=hit-penalised scores of cand)."""
    V = acc.shape[1]
    key = np.where(np.isnan(acc), NEG, acc).reshape(-1)
    order = np.lexsort((np.arange(key.size), -key))[:2 * W]          # descending value, ties towards the lower flat index
    order = [int(f) for f in order if key[f] > -np.inf]
    cand = [(f, float(acc.reshape(-1)[f])) for f in order]
    while len(cand) < 2 * W:
        cand.append((0, float("-inf")))
    hit = [at_limit or (eos_id >= 0 and f % V == eos_id) for f, _ in cand]
    ck = [NEG if np.isnan(a) else a for _, a in cand]
    kmod = [k + NEG if h else k for k, h in zip(ck, hit)]
    if forced is None:
        pick = sorted(range(2 * W), key=lambda c: (-kmod[c], c))[:W]
        beams = [(cand[c][0] // V, cand[c][0] % V, cand[c][1] + NEG if hit[c] else cand[c][1]) for c in pick]
    else:
        beams = []
        for p, t in forced:
            p, t = int(p), int(t)
            h = at_limit or (eos_id >= 0 and t == eos_id)
            beams.append((p, t, float(acc[p, t]) + NEG if h else float(acc[p, t])))
    was_full = len(fin) >= W
    items = [dict(s) for s in fin]
    if not was_full:
        for c in range(W):
            if hit[c]:
                f, a = cand[c]
                items.append({"score": a / float(length) ** alpha, "len": length, "parent": f // V, "token": f % V, "acc": a, "new": c})
    skey = [NEG if np.isnan(s["score"]) else s["score"] for s in items]
    keep = sorted(range(len(items)), key=lambda i: (-skey[i], i))[:W]
    new_fin = [items[i] for i in keep]
    entered = [s["new"] for s in new_fin if "new" in s]
    return {"cand": cand, "hit": hit, "kmod": kmod, "beams": beams, "entered": entered, "fin": new_fin, "done": len(new_fin) >= W}


def beam_search(enc_out: torch.Tensor, W_, cfg, n_steps: int, bf16: bool, num_beams: int, num_return: Optional[int] = None,
                length_penalty: float = 1.0, prompt: Optional[torch.Tensor] = None, automaton=None, start_states=None,
                forced_trace=None, return_logits: bool = False):
    """-> SimpleNamespace(tokens (B, K, N, n_steps) int32, seq_scores (B, K, N) f64, token_scores (B, K, N, n_steps) f64,
    trace (n_steps, G, W, 2) int64 of the running beams actually followed, run (n_steps, G, W) f64, own (n_steps, G) list of
    host_select results of the oracle's OWN choice at every step (None for a done group), logits (n_steps, G, W, V) or None,
    done_step (G,) first step after which the group was done (n_steps - 1 at the latest), events: counters used by the tests)."""
    W = int(num_beams)
    N = int(num_return or W)
    B, K, V = enc_out.shape[0], cfg.n_channels, cfg.vocab
    G, R = B * K, B * K * W
    cfg_v = _CfgView(cfg, K * W)
    Wv = dict(W_)
    Wv["dec.chan_embed"] = (W_["dec.chan_embed"].repeat_interleave(W, 0) if K > 1 else
                            torch.zeros(W, cfg.d_model, dtype=W_["dec.embed"].dtype))
    allowed = nxt = None
    state = torch.zeros(R, dtype=torch.long)
    if automaton is not None:
        allowed = torch.from_numpy(automaton.allowed)
        nxt = torch.from_numpy(automaton.next).long()
        if start_states is not None:
            state = torch.as_tensor(start_states).long().expand(B, K).reshape(G).repeat_interleave(W).clone()
    P = 0 if prompt is None else int(prompt.shape[-1])
    ckv = O.cross_kv(enc_out, W_, cfg, bf16)
    ds = O.DecoderState(R, cfg)
    cur = torch.full((R,), cfg.pad_id, dtype=torch.long)
    for t in range(P):
        O.decoder_step(cur, ds, ckv, Wv, cfg_v, bf16)
        cur = prompt.reshape(G, P)[:, t].long().repeat_interleave(W)
    run = np.full((G, W), NEG)
    run[:, 0] = 0.0
    fins = [[] for _ in range(G)]
    hist_tok = np.zeros((G, W, n_steps), np.int64)            # tokens / lps of every running beam so far (gathered by parent, as HF does)
    hist_lp = np.zeros((G, W, n_steps))
    trace = np.zeros((n_steps, G, W, 2), np.int64)
    runs = np.zeros((n_steps, G, W))
    own = [[None] * G for _ in range(n_steps)]
    all_logits = []
    done_step = np.full(G, n_steps - 1)
    events = {"filled_early": 0, "ran_to_limit": 0, "displaced": 0, "eos_beyond_w_not_taken": 0}
    steps_run = 0
    for j in range(n_steps):
        logits = O.decoder_step(cur, ds, ckv, Wv, cfg_v, bf16)
        steps_run = j + 1
        if return_logits:
            all_logits.append(logits.float().view(G, W, V).clone())
        lg = logits.double()
        if allowed is not None:
            lg = lg.masked_fill(~allowed[state], float("-inf"))
        lp = torch.log_softmax(lg, -1).view(G, W, V).numpy()
        parent_rows = torch.arange(R)
        new_cur = torch.full((R,), cfg.pad_id, dtype=torch.long)
        new_state = state.clone()
        for g in range(G):
            if len(fins[g]) >= W:                             # done: frozen, its rows idle on PAD
                trace[j, g, :, 0] = np.arange(W)
                trace[j, g, :, 1] = cfg.pad_id
                runs[j, g] = run[g]
                continue
            acc = run[g][:, None] + lp[g]
            if allowed is not None:                           # disallowed tokens are no candidates
                acc = np.where(allowed[state[g * W:(g + 1) * W]].numpy(), acc, -np.inf)
            at_limit = j + 1 >= n_steps
            sel = host_select(acc, W, cfg.eos_id, at_limit, fins[g], j + 1, length_penalty)
            own[j][g] = sel
            use = sel
            if forced_trace is not None:
                use = host_select(acc, W, cfg.eos_id, at_limit, fins[g], j + 1, length_penalty, forced=np.asarray(forced_trace[j][g]))
            # bookkeeping of the four situations test 1 wants to have seen
            old_scores = [s["score"] for s in fins[g]]
            kept_old = [s["score"] for s in use["fin"] if "new" not in s]
            if len(kept_old) < len(old_scores):
                events["displaced"] += 1
            for c in range(W, 2 * W):
                if cfg.eos_id >= 0 and use["cand"][c][0] % V == cfg.eos_id and not at_limit:
                    events["eos_beyond_w_not_taken"] += 1
            # hypotheses that entered: their token strings (parent's history + the finishing token)
            for s in use["fin"]:
                if "new" in s:
                    s["tokens"] = list(hist_tok[g, s["parent"], :j]) + [s["token"]]
                    s["lps"] = list(hist_lp[g, s["parent"], :j]) + [float(lp[g, s["parent"], s["token"]])]
                    del s["new"]
            fins[g] = use["fin"]
            if use["done"]:
                done_step[g] = j
                events["ran_to_limit" if at_limit else "filled_early"] += 1
            ht, hl = hist_tok[g].copy(), hist_lp[g].copy()
            for i, (p, t, r) in enumerate(use["beams"]):
                trace[j, g, i] = (p, t)
                run[g, i] = r
                hist_tok[g, i] = ht[p]
                hist_lp[g, i] = hl[p]
                hist_tok[g, i, j] = t
                hist_lp[g, i, j] = lp[g, p, t]
                parent_rows[g * W + i] = g * W + p
                new_cur[g * W + i] = t
                if nxt is not None:
                    new_state[g * W + i] = nxt[state[g * W + p], t]
            runs[j, g] = run[g]
        for l in range(cfg.n_dec_layers):
            ds.k[l] = ds.k[l][parent_rows]
            ds.v[l] = ds.v[l][parent_rows]
        cur, state = new_cur, new_state
        if all(len(f) >= W for f in fins):
            break
    tokens = np.full((G, N, n_steps), cfg.pad_id, np.int32)
    seq = np.full((G, N), NEG)
    tsc = np.zeros((G, N, n_steps))
    for g in range(G):
        for n, s in enumerate(fins[g][:N]):
            tokens[g, n, :s["len"]] = s["tokens"]
            tsc[g, n, :s["len"]] = s["lps"]
            seq[g, n] = s["score"]
    return SimpleNamespace(tokens=torch.from_numpy(tokens).view(B, K, N, n_steps), seq_scores=torch.from_numpy(seq).view(B, K, N),
                           token_scores=torch.from_numpy(tsc).view(B, K, N, n_steps), trace=trace[:steps_run], run=runs[:steps_run],
                           own=own[:steps_run], logits=torch.stack(all_logits) if return_logits else None, done_step=done_step,
                           events=events, steps_run=steps_run, fins=fins)
