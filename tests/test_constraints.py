"""Constrained decoding on the GPU (include/ymt3.h, constraints): token automata run inside the argmax kernel.

  - an all-allowed automaton is the unconstrained call bit for bit (ids, logits, scores), in every decode regime and slot mode;
  - every emitted id is the first argmax of the call's own raw logits masked by the host walk of the fed ids, and every score
    the masked log_softmax, in every regime, for the event grammar and a random automaton;
  - teacher-forced ids against the constrained CPU oracle (tests/constraint_oracle.py);
  - the event grammar on the seeded random-weight model, continuous batching, combinations, abort recovery, errors and the
    end-to-end path.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from constraint_oracle import constrained_greedy_decode
from test_gpu_parity import _check_ids, _model
from test_task_prompts import REGIMES, SMALL, _prompt
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.constraint import TokenAutomaton
from yourmt3_amd.task_manager import MC13_GROUPS, TaskManager
from yourmt3_amd.vocab import EOS

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _random_automaton(V, seed, n_states=3, p=0.3):
    g = np.random.default_rng(seed)
    allowed = g.random((n_states, V)) < p
    return TokenAutomaton(allowed, g.integers(0, n_states, (n_states, V)).astype(np.int32))


def _walk_states(aut, fed, starts):
    """(B, K, n) fed ids + (B, K) start states -> (B, K, n) the state each position is chosen in (no EOS freezing)"""
    fed = fed.cpu().long().clamp(0, aut.vocab - 1)
    nxt = torch.from_numpy(aut.next).long()
    st = torch.as_tensor(starts).long().clone()
    out = torch.empty(fed.shape, dtype=torch.long)
    for i in range(fed.shape[-1]):
        out[..., i] = st
        st = nxt[st, fed[..., i]]
    return out


def _check_masked(aut, tokens, logits, scores, states, fed):
    """ids = first argmax of the masked raw logits; scores = the masked log_softmax at the fed ids (-inf where disallowed)"""
    allowed = torch.from_numpy(aut.allowed)
    mask = allowed[states]                                                    # (B, K, n, V)
    masked = logits.cpu().masked_fill(~mask, float("-inf"))
    assert torch.equal(tokens.cpu().long(), masked.argmax(-1))
    if scores is not None:
        ref = torch.log_softmax(masked.double(), -1).gather(-1, fed.cpu().long().clamp(0, aut.vocab - 1)[..., None])[..., 0]
        got = scores.cpu().double()
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), fin)
        d = (got[fin] - ref[fin]).abs()
        assert bool((d <= 1e-4 + 1e-5 * ref[fin].abs()).all()), float(d.max())


def _grammar(cfg, programs=None):
    tm = TaskManager("mc13_full_plus_256" if cfg.n_channels == 13 else "mt3_full_plus")
    return tm.event_automaton(programs)


@pytest.mark.parametrize("name,cfg_kw,env,B", REGIMES, ids=[r[0] for r in REGIMES])
def test_constraints_in_every_regime(name, cfg_kw, env, B, monkeypatch):
    cfg = SMALL.with_(**cfg_kw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(cfg, max_batch=B)
    for k in env:
        monkeypatch.delenv(k)
    K, V = cfg.n_channels, cfg.vocab
    a = O.synthetic_audio(8, cfg, seed=11)
    a = (a.repeat(-(-B // 8), 1)[:B] * torch.linspace(0.5, 1.0, B)[:, None]).cuda()
    e = m.encode(m.logmel(a))
    N = 24 if cfg.max_decode_len <= 32 else 40
    # 1. an all-allowed automaton: the unconstrained call bit for bit
    every = m.compile_constraint(TokenAutomaton(np.ones((1, V), bool), np.zeros((1, V), np.int32)))
    t0, l0, s0 = m.decode(e, N, return_logits=True, return_scores=True)
    t1, l1, s1 = m.decode(e, N, return_logits=True, return_scores=True, constraint=every)
    assert torch.equal(t1, t0) and torch.equal(l1, l0) and torch.equal(s1, s0)
    if name == "two_chains":
        assert m.last_decode_chains == 2
    nseg = min(B, 4)
    ref_t, ref_s = m.inference(a[:nseg], max_token_length=N, return_scores=True)
    got_t, got_s = m.inference(a[:nseg], max_token_length=N, return_scores=True, constraint=every)
    assert torch.equal(got_t, ref_t) and torch.equal(got_s, ref_s)
    st_t, st_s = m.inference_stream(a[:nseg], max_token_length=N, slots=2, interval=4, return_scores=True, constraint=every)
    assert torch.equal(st_t, ref_t) and torch.allclose(st_s, ref_s, rtol=0, atol=1e-5)
    # 2. self-consistency: the event grammar (per-channel starts) and a random 3-state automaton (random per-row starts)
    gram, gstart = _grammar(cfg)
    rnd = _random_automaton(V, seed=B + K)
    g = torch.Generator().manual_seed(B)
    for aut, starts in ((gram, torch.as_tensor(gstart).long().expand(B, K)), (rnd, torch.randint(0, 3, (B, K), generator=g))):
        c = m.compile_constraint(aut)
        t, lg, sc = m.decode(e, N, return_logits=True, return_scores=True, constraint=c, start_states=starts)
        if name == "two_chains":
            assert m.last_decode_chains == 2
        _check_masked(aut, t, lg, sc, _walk_states(aut, t, starts), t)
        assert torch.equal(m.decode(e, N, constraint=c, start_states=starts), t)      # with and without scores / logits
        seg = m.inference(a[:nseg], max_token_length=N, constraint=c, start_states=starts[:nseg])
        assert torch.equal(seg, t[:nseg]) if nseg == B else torch.equal(seg, m.decode(e[:nseg], N, constraint=c, start_states=starts[:nseg]))
        assert torch.equal(m.inference_stream(a[:nseg], max_token_length=N, slots=2, interval=4, constraint=c, start_states=starts[:nseg]), seg)
        assert not torch.equal(t, t0)                                  # the constraint is not ignored
        c.close()
    every.close()
    m.close()


def _masked_oracle_logits(aut, logits, fed, starts):
    states = _walk_states(aut, fed, starts)
    return logits.masked_fill(~torch.from_numpy(aut.allowed)[states], float("-inf"))


@pytest.mark.parametrize("case", ["small", "mc13", "prompted"])
def test_constrained_ids_match_the_oracle(case):
    """teacher-forced with the oracle's own free-running constrained ids; the margin rule over the masked logits"""
    cfg = YMT3Config(segment_samples=8191, max_decode_len=96 if case != "mc13" else 32, eos_id=-1)
    if case == "mc13":
        cfg = cfg.with_(n_channels=13)
    m = _model(cfg, max_batch=2)
    K = cfg.n_channels
    a = O.synthetic_audio(2, cfg, seed=3)
    _, enc = O.encode(a, m.weights, cfg, True)
    if case == "mc13":
        aut, st = _grammar(cfg)
        starts = torch.as_tensor(st).long().expand(2, K)
    else:
        aut = _random_automaton(cfg.vocab, seed=4, p=0.4)
        starts = torch.tensor([[1], [2]])
    prompt = torch.tensor([[[599, 598]], [[601, 598]]], dtype=torch.int32) if case == "prompted" else None
    n = 24 if case == "mc13" else 64
    feed, _, _ = constrained_greedy_decode(enc, m.weights, cfg, n, True, aut, start_states=starts, prompt=prompt)
    ref_t, _, ref_l = constrained_greedy_decode(enc, m.weights, cfg, n, True, aut, start_states=starts, prompt=prompt, forced=feed)
    c = m.compile_constraint(aut)
    got_t = m.decode(enc.bfloat16().cuda(), n, forced=feed.cuda(), constraint=c, start_states=starts,
                     prompt=None if prompt is None else prompt.cuda())
    _check_ids(f"constrained_{case}_teacher_forced", got_t, ref_t, _masked_oracle_logits(aut, ref_l, feed, starts))
    c.close()
    m.close()


def _n_invalid(tm, tokens):
    tok = tokens.cpu().numpy()
    bad, progs = 0, [set() for _ in range(tok.shape[1])]
    for b in range(tok.shape[0]):
        for ch in range(tok.shape[1]):
            ev, ties, n = tm.tokenizer.decode_segment(tok[b, ch], 0.0)
            bad += n
            progs[ch] |= {e.program for e in ev} | {p for p, _ in ties}
    return bad, progs


def test_event_grammar_on_the_random_weight_model():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=96)
    assert cfg.eos_id == EOS
    m = _model(cfg, max_batch=4)
    tm = TaskManager()
    a = O.synthetic_audio(4, cfg, seed=9).cuda()
    free = m.inference(a, max_token_length=80)
    bad, _ = _n_invalid(tm, free)
    assert bad > 0                                                 # the precondition: unconstrained, the model says invalid things
    for programs in (None, [0, 1, 128]):
        aut, st = tm.event_automaton(programs)
        c = m.compile_constraint(aut)
        t = m.inference(a, max_token_length=80, constraint=c, start_states=st)
        bad, progs = _n_invalid(tm, t)
        assert bad == 0
        if programs is not None:
            assert progs[0] <= set(programs), progs
        c.close()
    m.close()


def test_event_grammar_keeps_the_13_channels_apart():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=32, n_channels=13)
    m = _model(cfg, max_batch=2)
    tm = TaskManager("mc13_full_plus_256")
    a = O.synthetic_audio(2, cfg, seed=4).cuda()
    free = m.inference(a, max_token_length=30)
    aut, st = tm.event_automaton()
    c = m.compile_constraint(aut)
    t = m.inference(a, max_token_length=30, constraint=c, start_states=st)
    bad, progs = _n_invalid(tm, t)
    assert bad == 0
    for ch, (_, group) in enumerate(MC13_GROUPS):
        assert progs[ch] <= set(group), (ch, progs[ch])
    assert not torch.equal(t, free)
    c.close()
    aut, st = tm.event_automaton([0])
    c = m.compile_constraint(aut)
    t = m.inference(a, max_token_length=30, constraint=c, start_states=st).cpu()
    tie = tm.codec.range_of("tie")[0]
    rest = torch.tensor([tie, EOS] + [cfg.pad_id] * 28, dtype=torch.int32)
    assert bool((t[:, 1:] == rest).all())
    bad, progs = _n_invalid(tm, t)
    assert bad == 0 and progs[0] <= {0}
    c.close()
    m.close()


def test_continuous_batching_seeds_each_admitted_segment():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=48)
    m = _model(cfg, max_batch=5)
    a = (O.synthetic_audio(5, cfg, seed=2) * torch.linspace(0.4, 1.0, 5)[:, None]).cuda()
    aut = _random_automaton(cfg.vocab, seed=8, n_states=4, p=0.35)
    aut.allowed[:, EOS] = aut.allowed[:, EOS] | (np.arange(4) == 3)      # state 3 may stop a row: segments retire at different times
    aut = TokenAutomaton(aut.allowed, aut.next)
    c = m.compile_constraint(aut)
    starts = torch.tensor([[0], [1], [2], [3], [1]])
    lock_t, lock_s = m.inference(a, max_token_length=40, constraint=c, start_states=starts, return_scores=True)
    for slots, interval in ((2, 4), (3, 8)):
        st_t, st_s = m.inference_stream(a, max_token_length=40, slots=slots, interval=interval, constraint=c, start_states=starts,
                                        return_scores=True)
        assert torch.equal(st_t, lock_t), (slots, interval)
        assert torch.allclose(st_s, lock_s, rtol=0, atol=1e-5)
    # different start states give different rows: admission seeding is what the equality above checks
    same = m.inference(a, max_token_length=40, constraint=c, start_states=torch.zeros(5, 1, dtype=torch.long))
    assert not torch.equal(same, lock_t)
    c.close()
    m.close()


def test_prompt_scores_forced_and_early_stop_with_a_constraint():
    m = _model(SMALL, max_batch=3)
    V = SMALL.vocab
    a = O.synthetic_audio(3, SMALL, seed=5).cuda()
    e = m.encode(m.logmel(a))
    N, P = 40, 2
    aut = _random_automaton(V, seed=21)
    c = m.compile_constraint(aut)
    starts = torch.tensor([[0], [1], [2]])
    p = _prompt(3, 1, P, seed=6).cuda()
    # prompt + constraint + scores, unforced
    t, lg, sc = m.decode(e, N, prompt=p, return_logits=True, return_scores=True, constraint=c, start_states=starts)
    _check_masked(aut, t, lg, sc, _walk_states(aut, t, starts), t)
    # + forced ids, some of them disallowed where the walk of the forced ids has them: -inf, and the state still moves by next
    g = torch.Generator().manual_seed(2)
    f = torch.randint(3, V, (3, 1, N), generator=g, dtype=torch.int32)
    states = _walk_states(aut, f, starts)
    dis = ~torch.from_numpy(aut.allowed)[states, f.long()]
    assert dis.any() and (~dis).any()
    tf, lf, sf = m.decode(e, N, prompt=p, forced=f.cuda(), return_logits=True, return_scores=True, constraint=c, start_states=starts)
    _check_masked(aut, tf, lf, sf, states, f)
    assert bool(torch.isneginf(sf.cpu()[dis]).all()) and bool(torch.isfinite(sf.cpu()[~dis]).all())
    c.close()
    m.close()
    # early stop: an automaton that ends every row with EOS after 5 + start tokens
    cfg = SMALL.with_(eos_id=EOS)
    m = _model(cfg, max_batch=3)
    n_st = 8
    allowed = np.ones((n_st, V), bool)
    allowed[:, EOS] = False
    allowed[n_st - 1] = False
    allowed[n_st - 1, EOS] = True
    nxt = np.tile(np.minimum(np.arange(n_st) + 1, n_st - 1)[:, None], (1, V)).astype(np.int32)
    cnt = TokenAutomaton(allowed, nxt)
    c = m.compile_constraint(cnt)
    full_t, full_s = m.decode(e, N, return_scores=True, constraint=c, start_states=starts)
    for b in range(3):
        k = n_st - 1 - b
        assert int(full_t[b, 0, k]) == EOS and bool((full_t[b, 0, k + 1:] == cfg.pad_id).all())
        assert bool((full_s[b, 0, k + 1:] == 0.0).all()) and bool((full_t[b, 0, :k] != EOS).all())
    m.set_early_stop(2)
    tok = torch.empty(3, 1, N, device=m.device, dtype=torch.int32)
    es = torch.full((3, 1, N), float("nan"), device=m.device)
    _lib.check(m._lib.ymt3_decode_constrained(m._handle, _p(e), 3, N, None, 0, _p(tok), _p(es), None, None, c.ptr,
                                              _p(starts.to(m.device, torch.int32)), m._stream()))
    assert m.last_decode_steps < N
    assert torch.equal(tok, full_t) and torch.equal(es, full_s)
    m.set_early_stop(0)
    c.close()
    m.close()


def test_abort_recovery_reseeds_the_states(monkeypatch):
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    m = _model(SMALL)
    m.fallback_expected = True
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    a = O.synthetic_audio(3, SMALL, seed=2).cuda()
    aut = _random_automaton(SMALL.vocab, seed=5)
    c = m.compile_constraint(aut)
    starts = torch.tensor([[2], [0], [1]])
    ok = m.inference(a, max_token_length=24, constraint=c, start_states=starts)
    assert m.merged_fallbacks == 0
    _lib.check(m._lib.ymt3_debug_force_stage_abort(m._handle))
    got = m.inference(a, max_token_length=24, constraint=c, start_states=starts)
    assert torch.equal(got, ok) and m.merged_fallbacks == 1             # the re-run started from the same states
    c.close()
    m.close()


def test_constraint_errors():
    m = _model(SMALL, max_batch=2)
    other = _model(SMALL, max_batch=2)
    V = SMALL.vocab
    a = O.synthetic_audio(2, SMALL).cuda()
    aut = _random_automaton(V, seed=1)
    c = m.compile_constraint(aut)
    c_other = other.compile_constraint(aut)
    with pytest.raises(_lib.YMT3Error, match="another handle"):
        m.inference(a, max_token_length=8, constraint=c_other)
    # the C layer validates on its own: a vocabulary mismatch, a next state out of range, a state that allows nothing
    bits = np.ascontiguousarray(aut.bits())
    nxt = np.ascontiguousarray(aut.next)
    out = ctypes.c_void_p()
    assert m._lib.ymt3_constraint_create(m._handle, 3, V + 32, bits.ctypes.data, nxt.ctypes.data, ctypes.byref(out)) != 0
    assert b"vocab" in m._lib.ymt3_last_error()
    bad_next = nxt.copy()
    bad_next[1, 7] = 3
    assert m._lib.ymt3_constraint_create(m._handle, 3, V, bits.ctypes.data, bad_next.ctypes.data, ctypes.byref(out)) != 0
    bad_bits = bits.copy()
    bad_bits[2] = 0
    assert m._lib.ymt3_constraint_create(m._handle, 3, V, bad_bits.ctypes.data, nxt.ctypes.data, ctypes.byref(out)) != 0
    assert m._lib.ymt3_constraint_create(m._handle, 1025, V, bits.ctypes.data, nxt.ctypes.data, ctypes.byref(out)) != 0
    assert not out.value
    with pytest.raises(ValueError):
        m.compile_constraint(TokenAutomaton(np.ones((1, V + 1), bool), np.zeros((1, V + 1), np.int32)))
    # start states: out of range, wrong shape, or without a constraint
    with pytest.raises(ValueError):
        m.inference(a, max_token_length=8, constraint=c, start_states=[3])
    with pytest.raises(ValueError):
        m.inference(a, max_token_length=8, constraint=c, start_states=[[0, 1]])
    with pytest.raises(ValueError):
        m.inference(a, max_token_length=8, start_states=[0])
    # device side: a start state out of range is clamped, as fed ids are
    tok = torch.empty(2, 1, 8, device=m.device, dtype=torch.int32)
    wild = torch.tensor([[99], [-5]], dtype=torch.int32, device=m.device)
    _lib.check(m._lib.ymt3_transcribe_segments_constrained(m._handle, _p(a), 2, 8, None, 0, _p(tok), None, c.ptr, _p(wild), m._stream()))
    assert torch.equal(tok, m.inference(a, max_token_length=8, constraint=c, start_states=[[2], [0]]))
    c.close()
    with pytest.raises(ValueError, match="closed"):
        m.inference(a, max_token_length=8, constraint=c)
    other.close()
    assert not c_other._c.value                                          # the model's close() frees its constraints
    m.close()


def test_transcribe_with_programs_end_to_end(tmp_path):
    from yourmt3_amd.midi import read_midi_notes
    from yourmt3_amd.transcribe import transcribe
    cfg = YMT3Config(segment_samples=8191, max_decode_len=64)
    m = _model(cfg, max_batch=3)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=3 * 8191))[0].numpy()
    kw = dict(bsz=2, max_token_length=48, return_notes=True)
    for continuous in (False, True):
        path, notes = transcribe(m, audio, output_dir=str(tmp_path / f"p{continuous}"), programs=[0, 1], continuous=continuous,
                                 confidence=True, **kw)
        assert all(n.program in (0, 1) for n in notes)
        back = read_midi_notes(open(path, "rb").read())
        assert all(n.program in (0, 1) for n in back)
    # constrained=True: the ids carry no invalid token
    tm = TaskManager()
    segs = m.ingest(torch.from_numpy(audio), cfg.sample_rate)
    aut, st = tm.event_automaton()
    c = m.compile_constraint(aut)
    batches = m.inference_file(2, segs, max_token_length=48, constraint=c, start_states=st)
    starts = [0.0] * sum(b.shape[0] for b in batches)
    _, bad = tm.detokenize_list_batches([b[:, 0, :] for b in batches], starts, return_events=True)
    assert bad == 0
    c.close()
    path, _ = transcribe(m, audio, output_dir=str(tmp_path / "c"), constrained=True, **kw)
    m.close()
