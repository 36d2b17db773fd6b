"""Decoder parity along the axis of the handle's HISTORY: a handle that has been through any other call gives the bits of a fresh handle.

A ymt3_handle carries state from call to call: the cache of captured step graphs (kernel arguments frozen at capture, filed under a key
derived from the call's step shape), the host settings that outlive a call (early stop, abort recovery, the debug traces; the per-call
modes -- slot mode, beam width, the layer-0 table switch -- travel in the step shape and are no longer kept on the handle, which this file
keeps holding to account), the device loop state (DecodeShared, finished / row_state / row_pos, the beam buffers), counters that are right only if the previous call left them at zero (ticket, chain_sync, pair_rows, step_sync),
buffers no call clears (the K/V cache, the MoE buffers, ckv, the logits) and objects the caller creates and destroys mid-life
(constraints, detokenisers, resampler filters).  The other axis files meet a handle fresh, or in whatever order a module's tests happen
to run.  Here the order is the subject.

The argument.  For every kind of call (tests/call_sequences.py: a call with fixed inputs of its own) the reference is what a handle
created for that kind alone returns from its FIRST call -- the case the rest of the suite compares with the CPU oracle.  One handle then
runs an Eulerian circuit over its catalogue, so every ordered pair of kinds, (a, a) included, is executed as two consecutive calls
exactly once (tests/test_call_sequences_cpu.py), and after every call every output tensor is compared with the kind's reference BIT FOR
BIT: there is no tolerance for a subtle error to hide under.  So that equal bits cannot be equally wrong, each run ends by holding the
history-laden handle itself against the oracle: teacher-forced ids and logits over all max_decode_len positions at the bounds of
test_gpu_parity.py (_check_ids: TAU 0.03, logits max 0.06 / mean 6e-3, MIN_SAFE; the MoE run through _moe_case at its fp8 bounds).  With
an EOS id a row's PAD fill hangs on its emitted ids, so a position counts only while no earlier step of its row was a sub-TAU choice
between the EOS id and another id (`stable`); no bound is new.

The kinds differ in audio seed, rows, batch, step count, prompt, automaton and start states, and references of equal shape are asserted
to differ: a leak from one kind into another cannot reproduce the right answer.  The EOS id is picked from a free run (as
test_eos_then_pad_fill does) so that some rows finish early and some never: the sequence goes through PAD fill, early stop, pad_tail and
slots retiring at different rounds.

The same references hold the asynchronous promises of INTEGRATION.md ("Threading, streams, errors"): every kind on a caller's stream other
than the default one, with the host running ahead of the device; calls issued back to back with nothing read back in between and their
inputs overwritten right after the call; two handles taking turns on one device; and a handle after a merged kernel gave up.
"""
import math
import os
import time

import numpy as np
import pytest
import torch

import call_sequences as S
from call_sequences import FREE, LOCKSTEP, MIX, SILENT, TRACED, constraint_of, euler_sequence, notes_tensors, pair_counts, pick_eos
from oracle import ymt3_oracle as O
from test_gpu_parity import TAU, _REPORT, _check_ids, _margin, _model, _moe_case
from test_row_space import MOE_BOUNDS, _regime
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.model import NOTE_RECORD, YourMT3
from yourmt3_amd.task_manager import Note
from yourmt3_amd.weights import make_weights

pytestmark = pytest.mark.gpu

ORACLE_ROWS = {"A": 4, "B": 2, "C": 4, "D": 8}        # segments of the closing oracle check
ORACLE_SEED = 71


def _create(cfg, env, max_batch, weights):
    """a handle created under `env` (the knobs are read at create); the environment is restored"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _model(cfg, max_batch=max_batch, weights=weights)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class _Ctx:
    """what a kind's make() draws its inputs from: rows [off, off + B) of a seeded synthetic batch (the rows differ in pitch, the seeds in
    noise), as audio, log-mel or encoder output of the base handle, and seeded ids"""

    def __init__(self, base, max_batch, batch):
        self.base, self.cfg, self.max_batch, self.batch = base, base.cfg, max_batch, batch
        self._audio, self._enc = {}, {}

    @staticmethod
    def put(t):
        return t.cuda()

    def audio(self, seed, off, B):
        if seed not in self._audio:
            self._audio[seed] = O.synthetic_audio(self.batch, self.cfg, seed=seed).cuda()
        assert off + B <= self.batch
        return self._audio[seed][off:off + B].clone()

    def mel(self, seed, off, B):
        return self.base.logmel(self.audio(seed, off, B))

    def enc(self, seed, off, B):
        if seed not in self._enc:
            self.audio(seed, 0, 1)
            self._enc[seed] = self.base.encode(self.base.logmel(self._audio[seed]))
        assert off + B <= self.batch
        return self._enc[seed][off:off + B].clone()

    def ids(self, seed, shape, lo=3, hi=None):
        g = torch.Generator().manual_seed(1000 + seed)
        return torch.randint(lo, hi or self.cfg.vocab, shape, generator=g, dtype=torch.int32).cuda()


def _fresh(inputs):
    """the call's own copies of the kind's inputs"""
    return {k: v.clone() if torch.is_tensor(v) else v for k, v in inputs.items()}


def _bits(t):
    if not t.is_floating_point():
        return t
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _first_diff(got, ref):
    """None if the tensors hold the same bits (NaNs and signed zeros included), else the first differing index"""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return ("shape", tuple(got.shape), got.dtype, tuple(ref.shape), ref.dtype)
    g, r = _bits(got), _bits(ref.to(got.device))
    if torch.equal(g, r):
        return None
    return tuple(int(v) for v in np.unravel_index(int((g != r).flatten().nonzero()[0]), tuple(g.shape)))


def _compare(label, prev, kind, out, refs):
    if SILENT in kind.tags:
        assert out == (), (label, kind.name)
        return
    ref = refs[kind.name]
    assert len(out) == len(ref), (label, kind.name, len(out), len(ref))
    for j, (g, r) in enumerate(zip(out, ref)):
        d = _first_diff(g, r)
        assert d is None, f"{label}: after {prev!r}, {kind.name!r}: output tensor {j} differs from the fresh handle's, first at {d}"


class _Rig:
    """One catalogue: its config (the EOS id picked from a free run), every kind's inputs, and every kind's reference -- the outputs of a
    handle created for that kind alone, whose first call it is."""

    def __init__(self, label, config, max_batch, env=None):
        t0 = time.perf_counter()
        self.label, self.max_batch, self.env = label, max_batch, dict(env or {})
        self.kinds = S.CATALOGUES[label]()
        self.by_name = {k.name: k for k in self.kinds}
        cfg0 = YMT3Config(**config, eos_id=-1)
        self.weights = make_weights(cfg0, seed=1234)
        batch = max(32, max_batch)
        base = _create(cfg0, {}, batch, self.weights)
        try:
            ctx = _Ctx(base, max_batch, batch)
            self.inputs = {k.name: k.make(ctx) for k in self.kinds}
            free = {k.name: k.run(base, _fresh(self.inputs[k.name]))[0] for k in self.kinds if FREE in k.tags}
            self.eos = pick_eos(free, [k.name for k in self.kinds if MIX in k.tags], cfg0.pad_id)
            self.oracle_enc = ctx.enc(ORACLE_SEED, 0, ORACLE_ROWS[label])
        finally:
            base.close()
        self.cfg = cfg0.with_(eos_id=self.eos)
        self._oracle = None
        self.refs, self.trace_refs, self.ref_chains, handles = {}, {}, {}, 1
        for k in self.kinds:
            if SILENT in k.tags:
                continue
            for traced in ((False, True) if TRACED in k.tags else (False,)):
                m = self.create()
                handles += 1
                try:
                    if traced:
                        m.moe_trace(self.cfg.max_decode_len).fill_(-1)
                    out = tuple(o.clone() for o in k.run(m, _fresh(self.inputs[k.name])))
                    if traced:
                        assert _first_diff(out[0], self.refs[k.name][0]) is None, k.name      # (the trace changes no bit)
                        self.trace_refs[k.name] = m._moe_trace.clone()
                    else:
                        self.refs[k.name] = out
                        self.ref_chains[k.name] = m.last_decode_chains
                finally:
                    m.close()
        self._check_references()
        self.seconds = time.perf_counter() - t0
        _REPORT[f"handle_state_references_{label}"] = {"kinds": len(self.kinds), "handles_created": handles, "eos_id": self.eos,
                                                       "seconds": round(self.seconds, 2), "finished_rows": self.finished_rows}
        print(f"references {label}: {handles} handles, {self.seconds:.1f} s, eos {self.eos}, finished rows {self.finished_rows}")

    def create(self, env=None):
        return _create(self.cfg, {**self.env, **(env or {})}, self.max_batch, self.weights)

    def _check_references(self):
        # rows that finish and rows that never do, in every kind that must have both
        self.finished_rows = {}
        for k in self.kinds:
            if FREE in k.tags:
                t = self.refs[k.name][0].cpu()
                fin = (t.reshape(-1, t.shape[-1]) == self.eos).any(1)
                self.finished_rows[k.name] = [int(fin.sum()), int(fin.numel())]
                if MIX in k.tags:
                    assert bool(fin.any()) and not bool(fin.all()), (k.name, self.finished_rows[k.name])
                pad = t.reshape(-1, t.shape[-1])[fin]
                first = (pad == self.eos).int().argmax(1)
                for row, f in zip(pad, first):
                    assert bool((row[int(f) + 1:] == self.cfg.pad_id).all())            # PAD after the EOS id
        # no two kinds of equal output shapes have equal references (but for a kind that declares whose outputs it must repeat)
        def sig(n):
            return [(tuple(o.shape), o.dtype) for o in self.refs[n]]
        names = list(self.refs)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                if sig(a) != sig(b):
                    continue
                same = all(_first_diff(x, y) is None for x, y in zip(self.refs[a], self.refs[b]))
                if self.by_name[b].get("same_as") == a:
                    assert same, (a, b)
                else:
                    assert not same, f"kinds {a!r} and {b!r} have equal references: a leak between them would go unseen"

    def oracle(self):
        """the CPU oracle's free-running ids and logits over all max_decode_len positions of ORACLE_ROWS segments of their own, once"""
        if self._oracle is None:
            L = self.cfg.max_decode_len
            ref_t, ref_l = O.greedy_decode(self.oracle_enc.float().cpu(), self.weights, self.cfg, L, True, return_logits=True)
            self._oracle = (ref_t, ref_l)
        return self._oracle


def _oracle_check(name, rig, m):
    """the closing check of a run: the history-laden handle against the CPU oracle, teacher-forced, at the bounds of _check_ids"""
    m.set_early_stop(0)
    ref_t, ref_l = rig.oracle()
    t, lg = m.decode(rig.oracle_enc, rig.cfg.max_decode_len, forced=ref_t.cuda(), return_logits=True)
    near = (_margin(ref_l) < TAU) & (ref_l.topk(2, -1).indices == rig.eos).any(-1)
    stable = (near.long().cumsum(-1) - near.long()) == 0          # no earlier sub-TAU choice for or against the EOS id in this row
    return _check_ids(name, t, ref_t, ref_l, lg, stable=stable)


def _euler_run(rig, m, after=None):
    """the Eulerian circuit over the rig's kinds on `m`, every output compared with its reference after every call"""
    names = [k.name for k in rig.kinds]
    seq = euler_sequence(names)
    t0 = time.perf_counter()
    prev = None
    for name in seq:
        kind = rig.by_name[name]
        tracing = TRACED in kind.tags and getattr(m, "trace_on", False)
        if tracing:
            m._moe_trace.fill_(-1)
        out = kind.run(m, _fresh(rig.inputs[name]))
        _compare(rig.label, prev, kind, out, rig.refs)
        if tracing:
            d = _first_diff(m._moe_trace, rig.trace_refs[name])
            assert d is None, f"{rig.label}: after {prev!r}, {name!r}: the recorded router choices differ from the fresh handle's, first at {d}"
        if after is not None:
            after(kind, m)
        prev = name
    torch.cuda.synchronize()
    pairs = pair_counts(seq)
    assert len(pairs) == len(names) ** 2 and set(pairs.values()) == {1}
    return {"kinds": len(names), "calls": len(seq), "pairs": len(pairs), "seconds": round(time.perf_counter() - t0, 2)}


def _finish(rig, m, rec, name):
    rec["oracle"] = _oracle_check(f"{name}_oracle", rig, m)
    assert m.merged_fallbacks == 0
    _REPORT[name] = rec
    print(name, {k: v for k, v in rec.items() if k != "oracle"})


@pytest.fixture(scope="module")
def rig_a():
    return _Rig("A", S.A_CONFIG, S.A_MAX_BATCH)


@pytest.fixture(scope="module")
def rig_b():
    return _Rig("B", S.B_CONFIG, S.B_MAX_BATCH)


@pytest.fixture(scope="module")
def rig_c():
    return _Rig("C", S.C_CONFIG, S.C_MAX_BATCH, env={"YMT3_DEBUG_HOOKS": "1"})


@pytest.fixture(scope="module")
def rig_d():
    return _Rig("D", S.D_CONFIG, S.D_MAX_BATCH)


# ----------------------------------------------------------------------------- the four runs
def test_a_dense_one_channel_handle_gives_the_fresh_bits_after_any_call(rig_a):
    """The merged regime with the layer-0 table on and graph_steps 16: every stage, every decode path (greedy, forced, prompted, scored,
    constrained with two automata and one that lives for a single call, beams, continuous batching in all its forms, scoring in one
    pass, detokenisation, ingest at two rates, the eager profile path, the GEMM hook), early stop switched on and off, and three refused
    calls: 29 kinds, 842 calls."""
    m = rig_a.create()
    try:
        rec = _euler_run(rig_a, m)
        _finish(rig_a, m, rec, "handle_state_A")
        assert m.qkv0_table_active and m.last_decode_chains == 1
    finally:
        m.close()


def test_b_three_channel_handle_gives_the_fresh_bits_after_any_call(rig_b):
    """128 frames, 3 channels: channel embeddings, the shared-K/V cross-attention, start states per (segment, channel); no layer-0 table."""
    m = rig_b.create()
    try:
        rec = _euler_run(rig_b, m)
        _finish(rig_b, m, rec, "handle_state_B")
        assert not m.qkv0_table_active
    finally:
        m.close()


def test_c_moe_fp8_handle_gives_the_fresh_bits_after_any_call(rig_c):
    """The MoE chain on fp8 experts: slot mode alternates the expert buffers, the router trace goes on and off (either drops the cached
    step graphs), the profile path runs eagerly, ymt3_score_tokens is refused.  While the trace is on, the recorded router choices of
    every lock-step decode call equal a fresh traced handle's."""
    m = rig_c.create()
    try:
        rec = _euler_run(rig_c, m)
        assert set(rig_c.trace_refs) == {k.name for k in rig_c.kinds if TRACED in k.tags}
        e = rig_c.oracle_enc
        out = {}
        _moe_case(rig_c.cfg, rig_c.cfg.max_decode_len, monkeypatch=None, enc=e.float().cpu(), m=m, feed=m.decode(e, rig_c.cfg.max_decode_len).cpu(),
                  name="handle_state_C_oracle", out=out, **MOE_BOUNDS[1])
        m.trace_on = False
        rec["oracle"] = out["rec"]
        assert m.merged_fallbacks == 0
        _REPORT["handle_state_C"] = rec
    finally:
        m.close()


def test_d_row_count_regimes_switch_on_one_handle(rig_d):
    """One handle of 200 rows through two chains on its own streams (200 rows), no fold and the two-level ticket (100), the fold and the
    ticket (65), the merged kernels (64, 8, 1), one chain at 200 rows under early stop, 70 segments through 40 slots and 200 beam rows:
    every regime after every other.  All decodes take rows [0, B) of one encoded batch, so by the row-independence contract
    (tests/test_row_space.py) a smaller call's reference is the first rows of a larger one's."""
    refs = rig_d.refs
    for B in S.D_ROWS[1:]:
        assert torch.equal(refs["decode_200"][0][:B], refs[f"decode_{B}"][0]), B
    for k in rig_d.kinds:
        if k.get("rows"):
            assert rig_d.ref_chains[k.name] == (k.get("chains") or _regime(k.get("rows"))["chains"]), k.name

    def after(kind, m):
        if kind.get("rows") or kind.get("chains"):
            want = kind.get("chains") or _regime(kind.get("rows"))["chains"]
            assert m.last_decode_chains == want, (kind.name, m.last_decode_chains, want)

    m = rig_d.create()
    try:
        rec = _euler_run(rig_d, m, after)
        _finish(rig_d, m, rec, "handle_state_D")
    finally:
        m.close()


# ----------------------------------------------------------------------------- streams and asynchrony
def _no_host_checks(monkeypatch):
    """The wrapper's range checks of a prompt and of start states read the tensor back (int(t.min())), which waits for the stream.  The
    asynchronous tests pass what those checks return -- (B, K, P) / (B, K) int32 device tensors, the very ones the lock-step runs have
    validated -- and take the checks out, so that the host reaches the C call with the inputs' copies still queued."""
    monkeypatch.setattr(YourMT3, "_prompt", lambda self, t, B, n: t)
    monkeypatch.setattr(YourMT3, "_start_states", lambda self, c, st, B: st)


_BUSY = {}


def _queue_unrelated_work():
    """Three fp32 products of 8192 x 8192 matrices on the current stream: 3.3 TFLOP, some tens of milliseconds of device time, where the
    host needs well under a millisecond to reach a call's first launch.  Whatever the call launches or clears on another stream than the
    caller's therefore runs long before the call's inputs exist and before the work queued ahead of it has finished."""
    if not _BUSY:
        g = torch.Generator(device="cuda").manual_seed(5)
        _BUSY["a"] = torch.randn(8192, 8192, device="cuda", generator=g)
        _BUSY["b"] = torch.randn(8192, 8192, device="cuda", generator=g)
        _BUSY["c"] = torch.empty(8192, 8192, device="cuda")
        torch.mm(_BUSY["a"], _BUSY["b"], out=_BUSY["c"])           # (the BLAS library's own start-up, outside the measured part)
        torch.cuda.synchronize()
    for _ in range(3):
        torch.mm(_BUSY["a"], _BUSY["b"], out=_BUSY["c"])


def _poison_(t):
    """never the right input: ids, states and lengths 0 (the kinds' own are above 0 somewhere), real values 0.25"""
    return t.zero_() if not t.is_floating_point() else t.fill_(0.25)


def _inputs_on_stream(inputs):
    """The call's inputs made on the current stream immediately before the call: clones of the staging tensors, queued behind unrelated
    work.  The memory the clones land in held poison before (blocks of the same size, just returned to this stream's pool)."""
    for v in inputs.values():
        if torch.is_tensor(v):
            _poison_(torch.empty_like(v))
    _queue_unrelated_work()
    return _fresh(inputs)


def _run_on_stream(rig, m, names, stream):
    outs = []
    with torch.cuda.stream(stream):
        for name in names:
            outs.append((name, rig.by_name[name].run(m, _inputs_on_stream(rig.inputs[name]))))
    return outs


def _compare_all(label, rig, outs):
    prev = None
    for name, out in outs:
        _compare(label, prev, rig.by_name[name], out, rig.refs)
        prev = name


S2_KINDS = {"A": ["inference_b4", "beam_w2", "stream"], "D": ["decode_200", "beam_w2_b100", "stream_70_through_40"]}


def test_every_call_runs_on_the_callers_stream(rig_a, rig_d, monkeypatch):
    """calls are asynchronous on the caller's stream.  Every kind of A once on a stream s1 that is not the default one,
    the inputs cloned on s1 right before each call behind queued work, one synchronisation at the end; then a greedy, a beam and a
    stream kind on s2 after s2.wait_stream(s1).  The same for D at 200 rows: the fork and join of the handle's chain streams hang on the
    caller's stream, here twice in a row with nothing in between.  A launch or a memset on the null stream would run ahead of all that."""
    _no_host_checks(monkeypatch)
    d_names = ["decode_200", "decode_200", "decode_200_early_stop", "beam_w2_b100", "decode_200", "stream_70_through_40", "decode_200"]
    for rig, names in ((rig_a, [k.name for k in rig_a.kinds]), (rig_d, d_names)):
        m = rig.create()
        try:
            for k in rig.kinds:                                 # (creating a constraint is a synchronous call: done beforehand)
                if "automaton" in rig.inputs[k.name] and k.name != "constraint_churn":
                    constraint_of(m, rig.inputs[k.name])
            torch.cuda.synchronize()
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            outs = _run_on_stream(rig, m, names, s1)
            if rig is rig_d:
                assert m.last_decode_chains == 2
            s1.synchronize()
            _compare_all(f"{rig.label} on s1", rig, outs)
            s2.wait_stream(s1)
            outs = _run_on_stream(rig, m, S2_KINDS[rig.label], s2)
            s2.synchronize()
            _compare_all(f"{rig.label} on s2", rig, outs)
            torch.cuda.synchronize()
            _oracle_check(f"handle_state_{rig.label}_streams_oracle", rig, m)
            assert m.merged_fallbacks == 0
        finally:
            torch.cuda.synchronize()
            m.close()


def _detok_async(m, det, x, keep):
    """ymt3_detokenize without the wrapper's copy back: (note records, counters) on the device, read after the synchronisation"""
    tokens, scores = x["tokens"], x["scores"]
    n, K, L = (int(v) for v in tokens.shape)
    starts = torch.tensor(x["starts"], dtype=torch.float64).cuda()
    notes = torch.empty(det.capacity * NOTE_RECORD.itemsize, device=m.device, dtype=torch.uint8)
    counts = torch.zeros(2, device=m.device, dtype=torch.int32)
    keep.append(starts)
    _lib.check(m._lib.ymt3_detokenize(m._handle, det.ptr, S._ptr(tokens), S._ptr(scores), n, L, tokens.stride(0), tokens.stride(1), S._ptr(starts),
                                      float(x["end_sec"]), S._ptr(notes), det.capacity, S._ptr(counts), m._stream()))
    return notes, counts


def _detok_result(notes, counts):
    """the records as TaskManager.tokens_to_notes_device turns them into notes"""
    n_notes, n_invalid = (int(v) for v in counts.cpu().tolist())
    rec = notes[:n_notes * NOTE_RECORD.itemsize].cpu().numpy().view(NOTE_RECORD)
    got = [Note(on, off, bool(dr), pg, pt, confidence=math.exp(sc))
           for on, off, pg, pt, dr, sc in zip(rec["onset"].tolist(), rec["offset"].tolist(), rec["program"].tolist(), rec["pitch"].tolist(),
                                              rec["is_drum"].tolist(), rec["score"].astype(np.float64).tolist())]
    return notes_tensors(sorted(got), n_invalid)


def test_back_to_back_calls_with_nothing_read_back(rig_a, rig_d, monkeypatch):
    """ymt3_set_abort_recovery(h, 0) takes the merged regime's end-of-call wait away: the lock-step kinds of A are issued one after
    another into output tensors of their own, forwards and then backwards, nothing is read back in between, and every call's input
    tensors (audio or enc, forced ids, prompt, start states, lengths) are overwritten on the same stream as soon as the call has returned
    -- legal for an asynchronous API.  One synchronisation, then every output against its reference.  The same for D's 100- and 200-row
    calls, which run the separate launches (no end-of-call wait to begin with)."""
    _no_host_checks(monkeypatch)
    a_names = [k.name for k in rig_a.kinds if LOCKSTEP in k.tags]
    assert len(a_names) >= 12 and "detokenize" in a_names
    d_names = ["decode_100", "decode_200", "decode_200", "decode_100", "decode_100", "beam_w2_b100", "decode_200", "beam_w2_b100", "decode_100"]
    for rig, names in ((rig_a, a_names + a_names[::-1]), (rig_d, d_names)):
        m = rig.create()
        det = None
        try:
            m.set_abort_recovery(0)
            for name in names:
                if "automaton" in rig.inputs[name]:
                    constraint_of(m, rig.inputs[name])
            if "detokenize" in names:
                x = rig.inputs["detokenize"]
                det = m.compile_detokenizer(x["task_manager"], x["tokens"].shape[0], x["tokens"].shape[2])
            torch.cuda.synchronize()
            outs, keep = [], []
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for name in names:
                    x = _fresh(rig.inputs[name])
                    out = _detok_async(m, det, x, keep) if name == "detokenize" else rig.by_name[name].run(m, x)
                    for v in x.values():
                        if torch.is_tensor(v):
                            _poison_(v)
                    outs.append((name, out))
            s.synchronize()
            outs = [(name, _detok_result(*out) if name == "detokenize" else out) for name, out in outs]
            _compare_all(f"{rig.label} back to back", rig, outs)
            m.set_abort_recovery(1)
            _oracle_check(f"handle_state_{rig.label}_back_to_back_oracle", rig, m)
            assert m.merged_fallbacks == 0
        finally:
            torch.cuda.synchronize()
            if det is not None:
                det.close()
            m.close()


def test_two_handles_take_turns_on_one_device(rig_a, rig_b):
    """A handle of A and a handle of B on the same device, their kinds alternating call by call on one stream (never concurrently: the
    merged kernels want the whole chip): what lives in one handle is not touched by the other's calls."""
    ma, mb = rig_a.create(), rig_b.create()
    try:
        na, nb = [k.name for k in rig_a.kinds], [k.name for k in rig_b.kinds]
        prev = None
        for i in range(max(len(na), len(nb))):
            for rig, m, name in ((rig_a, ma, na[i % len(na)]), (rig_b, mb, nb[i % len(nb)])):
                kind = rig.by_name[name]
                _compare(f"two handles, {rig.label}", prev, kind, kind.run(m, _fresh(rig.inputs[name])), rig.refs)
                prev = f"{rig.label}:{name}"
        _oracle_check("handle_state_two_handles_A_oracle", rig_a, ma)
        _oracle_check("handle_state_two_handles_B_oracle", rig_b, mb)
        assert ma.merged_fallbacks == 0 and mb.merged_fallbacks == 0
    finally:
        ma.close()
        mb.close()


def test_after_a_give_up_every_call_gives_the_fresh_bits(rig_a):
    """The software give-up word raised through the gated debug hook, as test_a_stage_abort_is_recovered_through_the_separate_launches
    does (nothing faults): the call is re-run through the separate launches, the handle drops its cached graphs and stays on those
    launches -- and every kind of A still returns the bits of a fresh handle on the merged kernels."""
    m = rig_a.create(env={"YMT3_DEBUG_HOOKS": "1"})
    m.fallback_expected = True
    try:
        first = rig_a.by_name["inference_b4"]
        _compare("A before the give-up", None, first, first.run(m, _fresh(rig_a.inputs[first.name])), rig_a.refs)
        assert m.merged_fallbacks == 0
        _lib.check(m._lib.ymt3_debug_force_stage_abort(m._handle))
        _compare("A, the call that gave up", first.name, first, first.run(m, _fresh(rig_a.inputs[first.name])), rig_a.refs)
        assert m.merged_fallbacks == 1
        prev = first.name
        for kind in rig_a.kinds:
            _compare("A after the give-up", prev, kind, kind.run(m, _fresh(rig_a.inputs[kind.name])), rig_a.refs)
            prev = kind.name
        assert m._lib.ymt3_debug_force_stage_abort(m._handle) == 4            # nothing merged left to give up
        _oracle_check("handle_state_A_after_give_up_oracle", rig_a, m)
        assert m.merged_fallbacks == 1
    finally:
        m.close()
