"""Call sequences for the handle-state tests (tests/test_handle_state.py): which calls a handle is put through, and in which order.

A `Kind` is one call with fixed inputs of its own: a name, `make(ctx)` -> the inputs (a dict; tensors are staging copies that the runner
clones before every call), and `run(model, inputs)` -> the tuple of output tensors.  A catalogue is the list of kinds one handle
configuration is put through.  `euler_sequence(kinds)` orders a catalogue so that every ordered pair of kinds, (a, a) included, is met
as two consecutive calls exactly once: an Eulerian circuit of the complete directed graph with self-loops, built by Hierholzer's
algorithm with the neighbours taken in list order, so the sequence is a function of the list alone.

Nothing here needs a GPU to import: the closures touch the model only when called.  `ctx` (test_handle_state._Ctx) supplies
`audio(seed, off, B)`, `mel(...)`, `enc(...)` (rows [off, off + B) of one seeded synthetic batch: the rows differ in pitch, the seeds in
noise), `ids(seed, shape, lo, hi)`, `cfg` and `max_batch`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Sequence

import numpy as np
import torch

from yourmt3_amd import _lib
from yourmt3_amd.constraint import TokenAutomaton


def euler_sequence(kinds: Sequence) -> list:
    """A circuit over `kinds` of length n * n + 1 in which every ordered pair (a, b), a == b included, appears as consecutive elements
    exactly once, and which ends where it starts.  Hierholzer: walk unused edges (each vertex's neighbours in list order) until stuck,
    which can only happen at a vertex all of whose edges are used; back out, emitting vertices; the emitted order reversed is the circuit."""
    kinds = list(kinds)
    n = len(kinds)
    if n == 0:
        return []
    unused = [0] * n                      # vertex v has used its edges to neighbours [0, unused[v])
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if unused[v] < n:
            stack.append(unused[v])
            unused[v] += 1
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return [kinds[i] for i in circuit]


def pair_counts(seq: Sequence) -> Dict[tuple, int]:
    out: Dict[tuple, int] = {}
    for a, b in zip(seq[:-1], seq[1:]):
        out[(a, b)] = out.get((a, b), 0) + 1
    return out


@dataclass(frozen=True)
class Kind:
    name: str
    run: Callable = field(compare=False, repr=False)            # (model, inputs) -> tuple of tensors
    make: Callable = field(compare=False, repr=False)           # (ctx) -> dict of inputs
    tags: frozenset = frozenset()
    meta: tuple = ()                                            # (key, value) pairs, e.g. ("rows", 200)

    def get(self, key, default=None):
        return dict(self.meta).get(key, default)


# tags
FREE = "free"             # free-running ids of plain audio / enc: what the EOS id is picked from (output 0 = the ids)
MIX = "mix"               # its reference must hold finished and unfinished rows
LOCKSTEP = "lockstep"     # issued back to back without a readback (the asynchronous tests)
SILENT = "silent"         # returns nothing (a setting, or a refused call)
TRACED = "traced"         # MoE: a lock-step decode call, whose router choices the debug trace records


def random_automaton(vocab: int, seed: int, n_states: int, p: float = 0.35) -> TokenAutomaton:
    g = np.random.default_rng(seed)
    allowed = g.random((n_states, vocab)) < p
    return TokenAutomaton(allowed, g.integers(0, n_states, (n_states, vocab)).astype(np.int32))


def pick_eos(streams: Dict[str, torch.Tensor], must: Sequence[str], pad_id: int) -> int:
    """The EOS id for a catalogue, from its free-running streams ({kind: (rows, L) ids} decoded with eos_id = -1): among the ids that
    some rows of every kind in `must` emit and some never do, the one that splits the most kinds that way, then one that rows first
    emit at two different steps at least (slots then retire at different rounds), then the one most rows emit, then the smallest."""
    streams = {k: v.reshape(-1, v.shape[-1]).cpu() for k, v in streams.items()}
    best = None
    for cand in sorted(set(torch.cat([v.flatten() for v in streams.values()]).tolist())):
        if cand == pad_id:
            continue
        mixed, firsts, finished = [], set(), 0
        for k, s in streams.items():
            hit = (s == cand).any(1)
            if bool(hit.any()) and not bool(hit.all()):
                mixed.append(k)
            firsts.update(int((r == cand).nonzero()[0]) for r in s[hit])
            finished += int(hit.sum())
        if all(k in mixed for k in must):
            score = (len(mixed), min(len(firsts), 2), finished, -cand)
            if best is None or score > best[0]:
                best = (score, cand)
    assert best is not None, "no id that some rows of every required kind emit and some never do"
    return best[1]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _tup(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def constraint_of(model, inputs, key="automaton"):
    """the handle's compiled constraint for the kind's automaton: compiled at the kind's first call on this handle and kept"""
    cache = model.__dict__.setdefault("_kept_constraints", {})
    aut = inputs[key]
    if id(aut) not in cache:
        cache[id(aut)] = (aut, model.compile_constraint(aut))
    return cache[id(aut)][1]


def refused(call, *exc):
    """the call must raise; it returns nothing"""
    try:
        call()
    except exc or (_lib.YMT3Error,):
        return ()
    raise AssertionError("a call that must be refused was accepted")


def notes_tensors(notes, n_invalid):
    """sorted Note list -> ((n, 6) f64: onset, offset, is_drum, program, pitch, confidence (-1: none); (1,) the invalid count)"""
    rows = [[n.onset, n.offset, float(n.is_drum), float(n.program), float(n.pitch), -1.0 if n.confidence is None else n.confidence] for n in notes]
    return torch.tensor(rows, dtype=torch.float64).reshape(-1, 6), torch.tensor([int(n_invalid)], dtype=torch.int64)


# ----------------------------------------------------------------------------- kind constructors
# Every constructor takes the kind's own seed and row offset: no two kinds decode the same rows.
def k_logmel(name, seed, off, B):
    return Kind(name, lambda m, x: (m.logmel(x["audio"]),), lambda c: {"audio": c.audio(seed, off, B)})


def k_encode(name, seed, off, B):
    return Kind(name, lambda m, x: (m.encode(x["mel"]),), lambda c: {"mel": c.mel(seed, off, B)})


def k_inference(name, seed, off, B, L, *tags):
    return Kind(name, lambda m, x: (m.inference(x["audio"], max_token_length=L),), lambda c: {"audio": c.audio(seed, off, B)},
                frozenset((FREE, LOCKSTEP) + tags))


def k_decode(name, seed, off, B, n, *tags, meta=()):
    return Kind(name, lambda m, x: (m.decode(x["enc"], n),), lambda c: {"enc": c.enc(seed, off, B)}, frozenset((FREE, LOCKSTEP) + tags), meta)


def k_forced(name, seed, off, B, n, *tags):
    def make(c):
        return {"enc": c.enc(seed, off, B), "forced": c.ids(seed, (B, c.cfg.n_channels, n))}
    return Kind(name, lambda m, x: _tup(m.decode(x["enc"], n, forced=x["forced"], return_logits=True)), make, frozenset((LOCKSTEP,) + tags))


def k_prompted(name, seed, off, B, P, n):
    def make(c):
        return {"enc": c.enc(seed, off, B), "prompt": c.ids(seed, (B, c.cfg.n_channels, P))}
    return Kind(name, lambda m, x: (m.decode(x["enc"], n, prompt=x["prompt"]),), make, frozenset((LOCKSTEP,)))


def k_scored(name, seed, off, B, n, *tags):
    return Kind(name, lambda m, x: _tup(m.decode(x["enc"], n, return_scores=True)), lambda c: {"enc": c.enc(seed, off, B)},
                frozenset((FREE, LOCKSTEP) + tags))


def _constrained_inputs(c, seed, off, B, n_states, aseed, what="enc"):
    src = c.enc(seed, off, B) if what == "enc" else c.audio(seed, off, B)
    K = c.cfg.n_channels
    starts = (torch.arange(B * K, dtype=torch.int32) % (n_states - 1) + 1).reshape(B, K)          # per (segment, channel), never state 0
    return {what: src, "automaton": random_automaton(c.cfg.vocab, aseed, n_states), "starts": c.put(starts)}


def k_constrained(name, seed, off, B, n, n_states, aseed, *tags):
    def run(m, x):
        return _tup(m.decode(x["enc"], n, return_scores=True, constraint=constraint_of(m, x), start_states=x["starts"]))
    return Kind(name, run, lambda c: _constrained_inputs(c, seed, off, B, n_states, aseed), frozenset((LOCKSTEP,) + tags))


def k_constraint_churn(name, seed, off, B, n, n_states, aseed):
    """a constraint that lives for one call: created, used, destroyed"""
    def run(m, x):
        tmp = m.compile_constraint(x["automaton"])
        try:
            return _tup(m.decode(x["enc"], n, return_scores=True, constraint=tmp, start_states=x["starts"]))
        finally:
            tmp.close()
    return Kind(name, run, lambda c: _constrained_inputs(c, seed, off, B, n_states, aseed))


def k_beam(name, seed, off, B, n, W, N, alpha=1.0, n_states=0, aseed=0, meta=()):
    def make(c):
        return _constrained_inputs(c, seed, off, B, n_states, aseed) if n_states else {"enc": c.enc(seed, off, B)}

    def run(m, x):
        kw = dict(constraint=constraint_of(m, x), start_states=x["starts"]) if n_states else {}
        return _tup(m.decode(x["enc"], n, num_beams=W, num_return_sequences=N, length_penalty=alpha, return_scores=True, **kw))
    return Kind(name, run, make, frozenset((LOCKSTEP,)), meta)


def k_stream(name, seed, off, N, L, slots, interval, *tags):
    return Kind(name, lambda m, x: (m.inference_stream(x["audio"], max_token_length=L, slots=slots, interval=interval),),
                lambda c: {"audio": c.audio(seed, off, N)}, frozenset((FREE,) + tags))


def k_stream_scored_prompted(name, seed, off, N, L, P, slots, interval):
    def make(c):
        return {"audio": c.audio(seed, off, N), "prompt": c.ids(seed, (N, c.cfg.n_channels, P))}

    def run(m, x):
        return _tup(m.inference_stream(x["audio"], max_token_length=L, slots=slots, interval=interval, task_tokens=x["prompt"], return_scores=True))
    return Kind(name, run, make)


def k_stream_constrained(name, seed, off, N, L, slots, interval, n_states, aseed):
    def run(m, x):
        return _tup(m.inference_stream(x["audio"], max_token_length=L, slots=slots, interval=interval, return_scores=True,
                                       constraint=constraint_of(m, x), start_states=x["starts"]))
    return Kind(name, run, lambda c: _constrained_inputs(c, seed, off, N, n_states, aseed, what="audio"))


def k_stream_beam(name, seed, off, N, L, W, slots, interval):
    def run(m, x):
        return _tup(m.inference_stream(x["audio"], max_token_length=L, slots=slots, interval=interval, num_beams=W, num_return_sequences=W,
                                       return_scores=True))
    return Kind(name, run, lambda c: {"audio": c.audio(seed, off, N)})


def k_decode_score(name, seed, off, B, L):
    """teacher-forced scores in one pass, with per-row lengths: the full length, a part of it, and nothing"""
    def make(c):
        K = c.cfg.n_channels
        lengths = torch.tensor([[L, max(L // 3, 1), 0][(b + k) % 3] for b in range(B) for k in range(K)], dtype=torch.int32).reshape(B, K)
        return {"enc": c.enc(seed, off, B), "tokens": c.ids(seed, (B, K, L)), "lengths": c.put(lengths)}
    return Kind(name, lambda m, x: (m.decode_score(x["enc"], x["tokens"], lengths=x["lengths"]),), make, frozenset((LOCKSTEP,)))


def k_score(name, seed, off, B, L):
    def make(c):
        return {"audio": c.audio(seed, off, B), "tokens": c.ids(seed, (B, c.cfg.n_channels, L))}
    return Kind(name, lambda m, x: _tup(m.score(x["audio"], x["tokens"], lengths="eos")), make, frozenset((LOCKSTEP,)))


def k_detok(name, seed, n, L):
    """device detokenisation of fixed ids (the dense family of tests/detok_cases.py), a detokeniser of its own per call"""
    def make(c):
        import detok_cases as C
        tm = C.task_manager(C.TASK_OF_K[c.cfg.n_channels])
        rng = np.random.default_rng(seed)
        tokens = C._dense(rng, tm, n, c.cfg.n_channels, L)
        scores = (-np.abs(rng.standard_normal(tokens.shape)) * 2).astype(np.float32)
        return {"tokens": c.put(torch.from_numpy(tokens)), "scores": c.put(torch.from_numpy(scores)), "task_manager": tm,
                "starts": [i * 8192 / 16000 for i in range(n)], "end_sec": n * 8192 / 16000 + 1.0}

    def run(m, x):
        notes, bad = x["task_manager"].tokens_to_notes_device(m, x["tokens"], x["starts"], x["end_sec"], scores=x["scores"])
        return notes_tensors(notes, bad)
    return Kind(name, run, make, frozenset((LOCKSTEP,)))


def k_ingest(name, seed, sr, n_frames, n_ch, dtype):
    def make(c):
        g = torch.Generator().manual_seed(seed)
        pcm = torch.rand(n_frames, n_ch, generator=g) * 1.6 - 0.8
        if dtype == torch.int16:
            pcm = (pcm * 32767).round().to(torch.int16)
        return {"pcm": c.put(pcm if n_ch > 1 else pcm[:, 0])}
    return Kind(name, lambda m, x: (m.ingest(x["pcm"], sr),), make)


def k_profile(name, seed, off, B, n, stride):
    """the eager path (ymt3_profile_decode); the wrapper keeps the ids to itself, so the C call is made here"""
    def run(m, x):
        tokens = torch.empty(B, m.cfg.n_channels, n, device=m.device, dtype=torch.int32)
        ms, cnt = (ctypes.c_float * 16)(), (ctypes.c_int32 * 16)()
        _lib.check(m._lib.ymt3_profile_decode(m._handle, _ptr(x["enc"]), B, n, stride, _ptr(tokens), ms, cnt, m._stream()))
        return (tokens,)
    return Kind(name, run, lambda c: {"enc": c.enc(seed, off, B)})


def k_gemm(name, seed, M, N, K):
    def make(c):
        g = torch.Generator().manual_seed(seed)
        return {"a": c.put(torch.randn(M, K, generator=g).bfloat16()), "w": c.put(torch.randn(N, K, generator=g).bfloat16())}
    return Kind(name, lambda m, x: (m.test_gemm(x["a"], x["w"]),), make)


def k_early_stop(name, interval):
    return Kind(name, lambda m, x: m.set_early_stop(interval) or (), lambda c: {}, frozenset((SILENT,)))


def k_refused_steps(name, seed, off, B):
    """n_steps > max_decode_len"""
    return Kind(name, lambda m, x: refused(lambda: m.decode(x["enc"], m.cfg.max_decode_len + 1)), lambda c: {"enc": c.enc(seed, off, B)},
                frozenset((SILENT,)))


def k_refused_batch(name, seed, off):
    """B > max_batch"""
    return Kind(name, lambda m, x: refused(lambda: m.decode(x["enc"], 4)), lambda c: {"enc": c.enc(seed, off, c.max_batch + 1)},
                frozenset((SILENT,)))


def k_refused_beam(name, seed, off, B, W):
    """B * W > max_batch: the wrapper refuses it, and so does the C call, each on its own"""
    def run(m, x):
        refused(lambda: m.decode(x["enc"], 4, num_beams=W), ValueError)
        bp = _lib.BeamParams(W, 1, 1.0)
        tokens = torch.empty(B, m.cfg.n_channels, 1, 4, device=m.device, dtype=torch.int32)
        rc = m._lib.ymt3_decode_beam(m._handle, _ptr(x["enc"]), B, 4, None, 0, ctypes.byref(bp), _ptr(tokens), None, None, None, None, m._stream())
        assert rc == 1, rc                # YMT3_ERR_ARG
        return ()
    return Kind(name, run, lambda c: {"enc": c.enc(seed, off, B)}, frozenset((SILENT,)))


def k_refused_score(name, seed, off, B, L):
    """MoE: ymt3_score_tokens is YMT3_ERR_UNSUPPORTED"""
    def make(c):
        return {"enc": c.enc(seed, off, B), "tokens": c.ids(seed, (B, c.cfg.n_channels, L))}

    def run(m, x):
        try:
            m.decode_score(x["enc"], x["tokens"])
        except _lib.YMT3Error as e:
            assert "ymt3 error 4" in str(e), e
            return ()
        raise AssertionError("ymt3_score_tokens accepted an MoE decoder")
    return Kind(name, run, make, frozenset((SILENT,)))


def k_moe_trace(name, on, n_steps):
    """debug hook (YMT3_DEBUG_HOOKS=1): the router trace on / off; either way the handle drops its cached step graphs"""
    def run(m, x):
        if on:
            m.moe_trace(n_steps)
        else:
            _lib.check(m._lib.ymt3_debug_moe_trace(m._handle, None, 0, 0))
        m.trace_on = bool(on)
        return ()
    return Kind(name, run, lambda c: {}, frozenset((SILENT,)))


# ----------------------------------------------------------------------------- the catalogues
# A: dense, one channel, 64 frames, max_decode_len 32, max_batch 8
A_CONFIG = dict(segment_samples=8191, max_decode_len=32)
A_MAX_BATCH = 8


def catalogue_a() -> List[Kind]:
    return [
        k_logmel("logmel", 1, 0, 3),
        k_encode("encode", 2, 2, 2),
        k_inference("inference_b4", 3, 5, 4, 24, MIX),
        k_inference("inference_b1_full", 4, 9, 1, 32),
        k_forced("forced_logits_9", 5, 11, 3, 9),
        k_prompted("prompted", 6, 13, 2, 3, 20),
        k_scored("scored", 7, 14, 4, 18),
        k_constrained("constrained_3_states", 8, 17, 3, 22, 3, 41),
        k_constrained("constrained_5_states", 9, 19, 2, 21, 5, 42),
        k_constraint_churn("constraint_churn", 10, 21, 3, 16, 2, 43),
        k_beam("beam_w2", 11, 23, 4, 14, 2, 2),
        k_beam("beam_w4_length_penalty", 12, 26, 2, 12, 4, 3, alpha=0.6),
        k_beam("beam_constrained", 13, 27, 3, 13, 2, 2, n_states=3, aseed=44),
        k_stream("stream", 14, 6, 7, 24, 3, 4, MIX),
        k_stream_scored_prompted("stream_scored_prompted", 15, 12, 5, 20, 2, 2, 4),
        k_stream_constrained("stream_constrained", 16, 16, 4, 18, 3, 4, 4, 45),
        k_stream_beam("stream_beam", 17, 20, 3, 12, 2, 2, 4),
        k_decode_score("decode_score", 18, 22, 3, 20),
        k_score("score", 19, 24, 2, 16),
        k_detok("detokenize", 20, 3, 32),
        k_ingest("ingest_44k_stereo_i16", 21, 44100, 30000, 2, torch.int16),
        k_ingest("ingest_48k_mono_f32", 22, 48000, 20001, 1, torch.float32),
        k_profile("profile_decode", 23, 1, 2, 8, 4),
        k_gemm("test_gemm", 24, 200, 256, 512),
        k_early_stop("early_stop_4", 4),
        k_early_stop("early_stop_0", 0),
        k_refused_steps("refused_steps", 25, 3, 2),
        k_refused_batch("refused_batch", 26, 4),
        k_refused_beam("refused_beam", 27, 7, 3, 4),
    ]


# B: three channels, 128 frames, max_decode_len 24, max_batch 4 (no layer-0 table; channel embeddings; shared-K/V cross-attention)
B_CONFIG = dict(segment_samples=16383, n_channels=3, max_decode_len=24)
B_MAX_BATCH = 4


def catalogue_b() -> List[Kind]:
    return [
        k_decode("decode", 31, 0, 3, 20, MIX),
        k_forced("forced_logits_9", 32, 3, 2, 9),
        k_prompted("prompted", 33, 5, 2, 3, 17),
        k_scored("scored", 34, 7, 4, 16),
        k_constrained("constrained", 35, 11, 3, 18, 4, 46),
        k_beam("beam_w2", 36, 14, 2, 10, 2, 2),
        k_stream("stream", 37, 16, 5, 20, 2, 4, MIX),
        k_stream_beam("stream_beam", 38, 21, 3, 10, 2, 2, 4),
        k_decode_score("decode_score", 39, 24, 2, 15),
        k_refused_steps("refused_steps", 40, 1, 2),
        k_refused_batch("refused_batch", 41, 2),
        k_refused_beam("refused_beam", 42, 4, 3, 2),
    ]


# C: MoE decoder FFN on fp8 experts, max_decode_len 32, max_batch 6, created under YMT3_DEBUG_HOOKS=1
C_CONFIG = dict(segment_samples=8191, max_decode_len=32, dec_ffn=1, moe_fp8=1)
C_MAX_BATCH = 6


def catalogue_c() -> List[Kind]:
    return [
        k_decode("decode", 51, 0, 4, 24, MIX, TRACED),
        k_forced("forced_logits_9", 52, 4, 3, 9, TRACED),
        k_scored("scored", 53, 7, 2, 18, TRACED),
        k_constrained("constrained", 54, 9, 3, 20, 3, 47, TRACED),
        k_stream("stream", 55, 12, 5, 20, 2, 4, MIX),
        k_moe_trace("moe_trace_on", True, 32),
        k_moe_trace("moe_trace_off", False, 0),
        k_profile("profile_decode", 56, 17, 2, 8, 4),
        k_refused_score("refused_score_tokens", 57, 19, 2, 8),
    ]


# D: the row-count regimes on one handle: dense, one channel, max_decode_len 16, max_batch 200; every decode takes rows [0, B) of ONE
# encoded batch, so a smaller call's rows are a larger call's first rows
D_CONFIG = dict(segment_samples=8191, max_decode_len=16)
D_MAX_BATCH = 200
D_SEED, D_STEPS = 61, 12
D_ROWS = [200, 100, 65, 64, 8, 1]


def k_decode_early_stop(name, seed, B, n, interval):
    """early stop on for this call alone: at 168-256 rows one chain where the plain call runs two, under a graph key of its own"""
    def run(m, x):
        m.set_early_stop(interval)
        try:
            return (m.decode(x["enc"], n),)
        finally:
            m.set_early_stop(0)
    return Kind(name, run, lambda c: {"enc": c.enc(seed, 0, B)}, frozenset((FREE,)), (("rows", B), ("chains", 1), ("same_as", f"decode_{B}")))


def catalogue_d() -> List[Kind]:
    kinds = [k_decode(f"decode_{B}", D_SEED, 0, B, D_STEPS, *((MIX,) if B == 200 else ()), meta=(("rows", B),)) for B in D_ROWS]
    return kinds + [
        k_decode_early_stop("decode_200_early_stop", D_SEED, 200, D_STEPS, 4),
        k_stream("stream_70_through_40", D_SEED, 0, 70, D_STEPS, 40, 4, MIX),
        k_beam("beam_w2_b100", D_SEED, 0, 100, 8, 2, 2, meta=(("chains", 1),)),
    ]


CATALOGUES = {"A": catalogue_a, "B": catalogue_b, "C": catalogue_c, "D": catalogue_d}
