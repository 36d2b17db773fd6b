"""Beam search under continuous batching (include/ymt3.h, ymt3_transcribe_stream_beam; YourMT3.inference_stream(num_beams=...)).

  1. the stream's results equal the lock-step beam call's on the same segments: ids always (the kernels are row-independent bit for bit),
     scores bit for bit where the stream runs as many rows per step as the lock-step batch, within 1e-5 otherwise (the tolerance
     tests/test_constraints.py uses for stream scores);
  2. retirement and refill happen when they should whatever the numerics: a countdown automaton fixes the step at which every group is
     done, and the launched steps equal the host model's (tests/beam_stream_model.py);
  3. the ancestry-addressed attention reads the right history at per-row positions and in reused slots: the device's trace of a stream
     call is fed to the CPU oracle and the raw logits compared at every recorded step, with tests/test_beam.py's bounds;
  4. isolation of a non-finite segment, argument errors."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from beam_oracle import beam_search
from beam_stream_model import lockstep_steps, stream_steps
from oracle import ymt3_oracle as O
from test_beam import _ancestry_stats, _separate
from test_gpu_parity import MC3, SMALL, _model, _pick_eos
from yourmt3_amd.constraint import TokenAutomaton

pytestmark = pytest.mark.gpu
EOS = 7
LENGTHS = [24, 3, 17, 0, 9, 24, 5]                       # free tokens before the EOS, per segment (its slowest group)


def _cpu(x):
    return [t.cpu().numpy() for t in x] if isinstance(x, (tuple, list)) else x.cpu().numpy()


def _lockstep(m, audio, bsz, prompt=None, starts=None, **kw):
    """inference(num_beams=...) on batches of bsz segments, concatenated: (tokens, token_scores, seq_scores)"""
    parts = []
    for i in range(0, audio.shape[0], bsz):
        extra = dict(kw)
        if prompt is not None:
            extra["task_tokens"] = prompt[i:i + bsz]
        if starts is not None:
            extra["start_states"] = starts[i:i + bsz]
        parts.append(_cpu(m.inference(audio[i:i + bsz], return_scores=True, **extra)))
    return [np.concatenate([p[k] for p in parts], 0) for k in range(3)]


# ----------------------------------------------------------------------------- 1. equals lock-step
@pytest.mark.parametrize("base", [SMALL, MC3], ids=["single-channel", "3-channel"])
def test_stream_with_beams_equals_lockstep_batches(base):
    n_seg, bsz = 9, 3
    audio = O.synthetic_audio(n_seg, base)
    free = _model(dataclasses.replace(base, eos_id=-1))
    toks = np.concatenate(free.inference_file(4, audio), 0)
    free.close()
    eos, spread = _pick_eos(toks)
    assert spread >= 3, "the synthetic decode offers no token that stops rows at >= 3 different lengths"
    cfg = dataclasses.replace(base, eos_id=eos)
    K, L = cfg.n_channels, cfg.max_decode_len
    m = _model(cfg, max_batch=12)
    greedy_before = m.inference(audio[:4]).cpu()
    prompt2 = (torch.arange(n_seg * K * 2).reshape(n_seg, K, 2) * 5 % 89 + 3).int()
    for W, N, alpha, prompted in [(2, 2, 0.0, False), (4, 1, 1.0, True), (4, 4, 1.0, False), (2, 1, 1.0, True), (4, 2, 0.0, False)]:
        prompt = prompt2 if prompted else None
        Ls = L - 2 if prompted else L
        kw = dict(num_beams=W, num_return_sequences=N, length_penalty=alpha, max_token_length=Ls)
        ref = _lockstep(m, audio, bsz, prompt=prompt, **kw)
        assert ref[0].shape == (n_seg, K, N, Ls)
        lens = sorted({int(np.argmax(r == eos)) if (r == eos).any() else Ls for r in ref[0][:, :, 0].reshape(-1, Ls)})
        print(f"W={W} N={N} alpha={alpha} prompted={prompted}: best-hypothesis lengths {lens}")
        for slots, interval in [(3, 4), (1, 1), (2, 7), (0, 0)]:
            got = _cpu(m.inference_stream(audio, slots=slots, interval=interval, task_tokens=prompt, return_scores=True, **kw))
            steps = m.last_decode_steps
            assert got[0].shape == ref[0].shape and np.array_equal(got[0], ref[0]), (W, N, alpha, prompted, slots, interval)
            rows_equal = (slots if slots > 0 else 12 // W) == bsz and n_seg % bsz == 0
            err = [float(np.abs(got[k] - ref[k]).max()) for k in (1, 2)]
            print(f"  slots={slots} interval={interval}: {steps} steps, score differences {err}, exact expected: {rows_equal}")
            if rows_equal:
                assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), (W, N, alpha, prompted, slots, interval, err)
            else:
                assert np.allclose(got[1], ref[1], rtol=0, atol=1e-5) and np.allclose(got[2], ref[2], rtol=0, atol=1e-5), (slots, interval, err)
            assert np.array_equal(_cpu(m.inference_stream(audio, slots=slots, interval=interval, task_tokens=prompt, **kw)), ref[0])
    kw = dict(num_beams=4, num_return_sequences=2, length_penalty=1.0)
    ref = _lockstep(m, audio, bsz, **kw)
    few = _cpu(m.inference_stream(audio[:2], slots=3, return_scores=True, **kw))                   # fewer segments than slots
    assert np.array_equal(few[0], ref[0][:2]) and np.allclose(few[1], ref[1][:2], rtol=0, atol=1e-5) and np.allclose(few[2], ref[2][:2], rtol=0, atol=1e-5)
    none = m.inference_stream(audio[:0], return_scores=True, **kw)                                  # zero segments
    assert none[0].shape == (0, K, 2, L) and none[1].shape == (0, K, 2, L) and none[2].shape == (0, K, 2)
    short = _lockstep(m, audio, bsz, max_token_length=16, **kw)                                     # a length cap below max_decode_len
    got = _cpu(m.inference_stream(audio, slots=3, interval=4, max_token_length=16, return_scores=True, **kw))
    assert all(np.array_equal(x, y) for x, y in zip(got, short))
    # a lock-step beam call and a greedy call after stream calls give their usual bits
    again = _lockstep(m, audio, bsz, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(again, ref))
    assert torch.equal(m.inference(audio[:4]).cpu(), greedy_before)
    assert np.array_equal(m.inference_stream(audio, slots=4, interval=4).cpu().numpy(), np.concatenate(m.inference_file(4, audio), 0))
    m.close()


# ----------------------------------------------------------------------------- 2. retirement and refill
def _countdown(V, eos):
    """25 states: state s < 24 allows everything but EOS and moves to s + 1; state 24 allows only EOS.  A group started in state s is done
    at emitted step 24 - s whatever the logits: until then nothing finishes, and there each beam's only candidate is its EOS, so the
    W candidates of the group all finish and fill its W slots."""
    S = 25
    allowed = np.ones((S, V), bool)
    allowed[:, eos] = False
    allowed[S - 1] = False
    allowed[S - 1, eos] = True
    nxt = np.minimum(np.arange(S)[:, None] + 1, S - 1).repeat(V, 1).astype(np.int32)
    return TokenAutomaton(allowed, nxt)


def _starts(K):
    """(n_seg, K) start states: channel c of a segment is done 2c steps before channel 0, which is done at LENGTHS[segment]"""
    first = 24 - np.asarray(LENGTHS)
    return torch.from_numpy(np.minimum(first[:, None] + 2 * np.arange(K)[None, :], 24).astype(np.int32))


def _check_countdown_shape(tokens, done, pad):
    """every hypothesis of group g: done[g] free tokens, then EOS, then PAD"""
    G = done.size
    t = tokens.reshape(G, -1, tokens.shape[-1])
    for g in range(G):
        d = int(done[g])
        assert (t[g, :, :d] != EOS).all() and (t[g, :, d] == EOS).all() and (t[g, :, d + 1:] == pad).all(), (g, d, t[g])


@pytest.mark.parametrize("base,W", [(SMALL, 2), (SMALL, 4), (MC3, 2), (MC3, 4)], ids=["dense-w2", "dense-w4", "mc3-w2", "mc3-w4"])
def test_groups_retire_and_slots_refill_on_schedule(base, W):
    cfg = base.with_(eos_id=EOS)
    K, n, n_seg = cfg.n_channels, 32, len(LENGTHS)
    aut = _countdown(cfg.vocab, EOS)
    starts = _starts(K)
    done = 24 - starts.numpy().reshape(-1)               # per group
    done_seg = [int(x) for x in (24 - starts.numpy()).max(1)]
    assert done_seg == LENGTHS
    m = _model(cfg, max_batch=12)
    audio = O.synthetic_audio(n_seg, cfg)
    # the premise, on the CPU oracle: every group is done at 24 - start
    _, enc = O.encode(audio, m.weights, cfg, True)
    ref = beam_search(enc, m.weights, cfg, n, True, W, W, 1.0, automaton=aut, start_states=starts)
    assert (ref.done_step == done).all(), (ref.done_step, done)
    c = m.compile_constraint(aut)
    kw = dict(num_beams=W, num_return_sequences=W, length_penalty=1.0, max_token_length=n, constraint=c)
    zero = _cpu(m.inference_stream(audio, slots=2, interval=4, start_states=torch.zeros(K, dtype=torch.int32), **kw))
    _check_countdown_shape(zero, np.full(n_seg * K, 24), cfg.pad_id)
    for slots, interval in [(2, 4), (3, 8)]:
        lock = _lockstep(m, audio, slots, starts=starts, **kw)
        got = _cpu(m.inference_stream(audio, slots=slots, interval=interval, start_states=starts, return_scores=True, **kw))
        steps = m.last_decode_steps
        expected, lockstep = stream_steps(done_seg, slots, interval), lockstep_steps(done_seg, slots, interval, 0, n)
        print(f"slots={slots} interval={interval}: launched {steps}, model {expected}, lock-step batches with early stop {lockstep}")
        _check_countdown_shape(got[0], done, cfg.pad_id)
        assert np.array_equal(got[0], lock[0])
        assert np.allclose(got[1], lock[1], rtol=0, atol=1e-5) and np.allclose(got[2], lock[2], rtol=0, atol=1e-5)
        assert steps == expected, (steps, expected)
        assert steps < lockstep, (steps, lockstep)
        # the start states are the admitted segment's own: every segment but the two of length 24 differs from the all-zero run
        for s in range(n_seg):
            assert np.array_equal(got[0][s, 0], zero[s, 0]) == (LENGTHS[s] == 24), s
    # with a prompt of two ids every segment needs two more steps
    prompt = (torch.arange(n_seg * K * 2).reshape(n_seg, K, 2) * 3 % 71 + 9).int()
    kw["max_token_length"] = n - 2
    lock = _lockstep(m, audio, 2, prompt=prompt, starts=starts, **kw)
    got = _cpu(m.inference_stream(audio, slots=2, interval=4, start_states=starts, task_tokens=prompt, **kw))
    assert np.array_equal(got, lock[0]) and m.last_decode_steps == stream_steps(done_seg, 2, 4, n_prompt=2)
    # segments of length 0 (start state 24) retire at the first check after their admission
    got = _cpu(m.inference_stream(audio[:3], slots=1, interval=4, start_states=torch.full((K,), 24, dtype=torch.int32), **kw))
    assert m.last_decode_steps == 3 * 4 == stream_steps([0, 0, 0], 1, 4, n_prompt=0)
    _check_countdown_shape(got, np.zeros(3 * K, int), cfg.pad_id)
    c.close()
    m.close()


# ----------------------------------------------------------------------------- 3. the right history at per-row positions
@pytest.mark.parametrize("base", [SMALL, MC3], ids=["single-channel", "3-channel"])
def test_attention_reads_the_right_history_in_reused_slots(base, monkeypatch):
    """slots < segments: rows of different slots sit at different positions, and every slot is reused.  Thresholds: tests/test_beam.py's
    parity test (its measured figures: max 0.0101-0.0131, mean 1.4e-3-1.8e-3 of the logits' standard deviation)."""
    _separate(monkeypatch)
    cfg = base.with_(eos_id=EOS)
    K, W, n, n_seg, slots = cfg.n_channels, 4, 32, len(LENGTHS), 2
    G, V = n_seg * K, cfg.vocab
    aut = _countdown(V, EOS)
    starts = _starts(K)
    done = 24 - starts.numpy().reshape(-1)
    m = _model(cfg, max_batch=slots * W)
    audio = O.synthetic_audio(n_seg, cfg)
    enc = m.encode(m.logmel(audio.cuda())).float().cpu()          # the decoder is what is compared: both sides start from the same encoding
    c = m.compile_constraint(aut)
    tr, run, lg = m.beam_trace(n, G, W, logits=True)
    tok = m.inference_stream(audio, slots=slots, interval=4, num_beams=W, num_return_sequences=W, max_token_length=n, constraint=c,
                             start_states=starts).cpu().numpy()
    _check_countdown_shape(tok, done, cfg.pad_id)
    assert m.last_decode_steps == stream_steps(LENGTHS, slots, 4)
    trace, logits = tr.cpu().numpy().astype(np.int64), lg.cpu().numpy()
    assert m._lib.ymt3_debug_beam_trace(m._handle, None, None, None, 0, 0) == 0
    # indexed by the group's place in the queue: group g recorded its steps 0 .. done[g] and nothing after them
    rec = np.zeros((n, G), bool)
    for g in range(G):
        rec[:done[g] + 1, g] = True
    assert ((trace >= 0).all((2, 3)) == rec).all() and ((trace == -1).all((2, 3)) == ~rec).all()
    assert (trace[rec][..., 0] < W).all() and (trace[rec][..., 1] < V).all()
    assert (np.isfinite(logits).all((2, 3)) == rec).all()
    ref = beam_search(enc, m.weights, cfg, n, True, W, W, 1.0, automaton=aut, start_states=starts, forced_trace=trace, return_logits=True)
    assert (ref.done_step == done).all() and ref.steps_run == 25
    ref_l = ref.logits.numpy()                           # (25, G, W, V)
    r25 = rec[:25]
    std = float(ref_l[r25].std())
    d = np.abs(logits[:25][r25] - ref_l[r25]) / std
    moved = float((trace[rec][..., 0] != np.arange(W)[None, :]).mean())
    spans = max(_ancestry_stats(trace[:done[g] + 1, g:g + 1], W)[1] for g in range(slots * K, G))      # groups admitted into a reused slot
    fig = {"records": int(rec.sum()), "logits_std": std, "logits_max_abs": float(d.max()), "logits_mean_abs": float(d.mean()),
           "parent_moved_share": moved, "max_rows_in_a_history_after_a_refill": spans}
    print(fig)
    assert moved >= 0.25 and spans >= 3, fig
    assert fig["logits_max_abs"] < 0.06 and fig["logits_mean_abs"] < 6e-3, fig
    c.close()
    m.close()


# ----------------------------------------------------------------------------- 4. isolation and errors
def test_a_non_finite_segment_stays_in_its_groups():
    cfg = SMALL.with_(eos_id=EOS)
    m = _model(cfg, max_batch=8)
    audio = O.synthetic_audio(6, cfg)
    kw = dict(slots=2, interval=4, num_beams=4, num_return_sequences=4, max_token_length=24, return_scores=True)
    good = _cpu(m.inference_stream(audio, **kw))
    bad_audio = audio.clone()
    bad_audio[1] = float("nan")
    bad = _cpu(m.inference_stream(bad_audio, **kw))
    assert bad[0].min() >= 0 and bad[0].max() < cfg.vocab
    assert np.isnan(bad[2][1]).all(), bad[2][1]
    for s in (0, 2, 3, 4, 5):                            # the slot of segment 1 is taken by a later segment: that one too
        assert all(np.array_equal(x[s], y[s]) for x, y in zip(bad, good)), s
    again = _cpu(m.inference_stream(audio, **kw))
    assert all(np.array_equal(x, y) for x, y in zip(again, good))
    m.close()


def test_argument_errors_name_the_limit_and_leave_the_handle_usable():
    from yourmt3_amd import _lib
    cfg = SMALL.with_(eos_id=EOS)
    m = _model(cfg, max_batch=8)
    audio = O.synthetic_audio(3, cfg).cuda().contiguous()
    n = 16
    kw = dict(slots=2, interval=4, num_beams=4, num_return_sequences=2, max_token_length=n, return_scores=True)
    before = _cpu(m.inference_stream(audio, **kw))
    tok = torch.empty(3, 1, 2, n, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p

    def call(handle, params, slots=2):
        return m._lib.ymt3_transcribe_stream_beam(handle, vp(audio.data_ptr()), 3, n, None, 0, params, vp(tok.data_ptr()), None, None, slots, 4,
                                                  None, None, None)
    assert call(m._handle, ctypes.byref(_lib.BeamParams(9, 1, 1.0))) == 1 and b"num_beams=9 outside [1, 8]" in m._lib.ymt3_last_error()
    assert call(m._handle, ctypes.byref(_lib.BeamParams(4, 5, 1.0))) == 1 and b"num_return" in m._lib.ymt3_last_error()
    assert call(m._handle, ctypes.byref(_lib.BeamParams(4, 1, -1.0))) == 1 and b"length_penalty" in m._lib.ymt3_last_error()
    assert call(m._handle, None) == 1 and b"null beam parameters" in m._lib.ymt3_last_error()
    tiny = _model(cfg, max_batch=2)
    rc = m._lib.ymt3_transcribe_stream_beam(tiny._handle, vp(audio.data_ptr()), 3, n, None, 0, ctypes.byref(_lib.BeamParams(4, 1, 1.0)),
                                            vp(tok.data_ptr()), None, None, 0, 0, None, None, None)
    assert rc == 1 and b"max_batch=2" in m._lib.ymt3_last_error()
    one_by_one = np.concatenate([tiny.inference(audio[i:i + 1], max_token_length=8, num_beams=2).cpu().numpy() for i in range(2)], 0)
    assert np.array_equal(tiny.inference_stream(audio[:2], max_token_length=8, num_beams=2).cpu().numpy(), one_by_one)      # (the handle is usable)
    tiny.close()
    with pytest.raises(ValueError, match="max_batch"):
        m.inference_stream(audio, slots=3, num_beams=4)
    # slots beyond what fits are clamped, as in the greedy stream; the handle gives its usual bits after the refused calls
    assert call(m._handle, ctypes.byref(_lib.BeamParams(4, 2, 1.0)), slots=100) == 0
    torch.cuda.synchronize()
    assert np.array_equal(tok.cpu().numpy(), before[0])
    after = _cpu(m.inference_stream(audio, **kw))
    assert all(np.array_equal(x, y) for x, y in zip(after, before))
    m.close()
