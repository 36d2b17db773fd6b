"""Token automata for constrained decoding (include/ymt3.h, constraints).

A `TokenAutomaton` has S states, `allowed` (S, V) bool and `next` (S, V) int32.  At every emitted position a row in state s
emits the first maximum of its logits over the tokens allowed[s], and the id it feeds (the emitted token, or the forced one)
moves it to next[s][id].  This is HF `generate(prefix_allowed_tokens_fn=...)` with the prefix summarised by a state.  The decode
kernels run the automaton on the device; `walk` is the same rule on the host.

Builders: `suppress` / `allow_only` (one state each) and `stack`, which puts automata side by side (block-diagonal) so that the
rows of one call can run different ones (e.g. the 13 channels of the multi-channel decoder), each from its own start state.
"""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

import numpy as np

MAX_STATES = 1024             # the C ABI's bound (ymt3_constraint_create)


class TokenAutomaton:
    def __init__(self, allowed, next):
        a = np.asarray(allowed)
        n = np.asarray(next)
        if a.dtype != np.bool_:
            raise ValueError(f"allowed must be bool, got {a.dtype}")
        if a.ndim != 2 or n.shape != a.shape:
            raise ValueError(f"allowed and next must both be (S, V), got {a.shape} and {n.shape}")
        if not np.issubdtype(n.dtype, np.integer):
            raise ValueError(f"next must be integer states, got {n.dtype}")
        S, V = a.shape
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f"{S} states outside [1, {MAX_STATES}]")
        if V < 1:
            raise ValueError("an automaton needs a vocabulary")
        if n.size and (int(n.min()) < 0 or int(n.max()) >= S):
            raise ValueError(f"next states must lie in [0, {S})")
        empty = np.flatnonzero(~a.any(1))
        if empty.size:
            raise ValueError(f"state {int(empty[0])} allows no token")
        self.allowed = np.ascontiguousarray(a)
        self.next = np.ascontiguousarray(n, dtype=np.int32)

    @property
    def n_states(self) -> int:
        return self.allowed.shape[0]

    @property
    def vocab(self) -> int:
        return self.allowed.shape[1]

    def bits(self) -> np.ndarray:
        """(S, ceil(V / 32)) uint32: bit i % 32 of word i // 32 is allowed[s][i] (the C ABI's allowed_bits)."""
        words = (self.vocab + 31) // 32
        pad = np.zeros((self.n_states, words * 32), bool)
        pad[:, :self.vocab] = self.allowed
        return np.packbits(pad, axis=1, bitorder="little").view("<u4").astype(np.uint32)

    def walk(self, tokens: Iterable[int], state: int = 0) -> np.ndarray:
        """The states a row passes through when it is fed `tokens` from `state`: (n + 1,) int32, states[i] is the state in
        which token i is chosen.  Ids are clamped into [0, V) as the device clamps fed ids."""
        if not 0 <= int(state) < self.n_states:
            raise ValueError(f"state {state} outside [0, {self.n_states})")
        out = [int(state)]
        for t in tokens:
            t = min(max(int(t), 0), self.vocab - 1)
            out.append(int(self.next[out[-1], t]))
        return np.array(out, np.int32)

    def allows(self, state: int, token: int) -> bool:
        return bool(self.allowed[int(state), int(token)])


def _one_state(vocab: int, ids: Sequence[int], allow: bool) -> TokenAutomaton:
    ids = np.asarray(list(ids), np.int64)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
        raise ValueError(f"token ids must lie in [0, {vocab})")
    a = np.full((1, vocab), not allow)
    a[0, ids] = allow
    return TokenAutomaton(a, np.zeros((1, vocab), np.int32))


def suppress(vocab: int, ids: Sequence[int]) -> TokenAutomaton:
    """One state that allows every token but `ids` (HF `suppress_tokens`)."""
    return _one_state(vocab, ids, allow=False)


def allow_only(vocab: int, ids: Sequence[int]) -> TokenAutomaton:
    """One state that allows `ids` only."""
    return _one_state(vocab, ids, allow=True)


def stack(parts: Sequence[TokenAutomaton]) -> Tuple[TokenAutomaton, List[int]]:
    """Block-diagonal union of `parts` -> (automaton, start offset of every part).  A row started at part k's offset (+ one of
    its states) stays inside part k."""
    if not parts:
        raise ValueError("stack needs at least one automaton")
    V = parts[0].vocab
    if any(p.vocab != V for p in parts):
        raise ValueError("stacked automata must share one vocabulary")
    offsets, off = [], 0
    for p in parts:
        offsets.append(off)
        off += p.n_states
    allowed = np.concatenate([p.allowed for p in parts], 0)
    nxt = np.concatenate([p.next + o for p, o in zip(parts, offsets)], 0)
    return TokenAutomaton(allowed, nxt), offsets
