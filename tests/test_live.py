"""Live transcription on the GPU (include/ymt3.h: streaming ingest, incremental detokeniser; yourmt3_amd/transcribe.py: LiveTranscriber).
Every comparison is against the one-shot path of the same build -- model.ingest, the host NoteStream / note_events_to_notes, transcribe() --
and every one is exact: the streaming forms promise the one-shot result bit for bit for any way of cutting the input.

  6. streaming ingest == model.ingest (torch.equal) for four rate / channel / format combinations and every chunking that crosses a rule;
  7. incremental detokeniser: every push returns exactly what NoteStream returns for it, the union is the host reference;
  8. LiveTranscriber == transcribe(device_detok=True): notes and MIDI bytes;
  9. a decode is the same bits before and after a whole live cycle on the same handle, and the same as on a fresh handle."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import detok_cases as C
import live_cases as LC
from oracle import ingest_oracle as IO
from oracle import ymt3_oracle as O
from test_gpu_parity import SMALL, _model
from yourmt3_amd._lib import YMT3Error
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.model import NOTE_RECORD

pytestmark = pytest.mark.gpu

S = SMALL.segment_samples
CFG = {1: dataclasses.replace(SMALL, max_decode_len=1024), 13: YMT3Config(segment_samples=8191, max_decode_len=256, n_channels=13)}


@pytest.fixture(scope="module")
def small():
    m = _model(SMALL, max_batch=2)
    yield m
    m.close()


# ---------------------------------------------------------------------------------------------- 6. streaming ingest
def _pcm(sr, n, ch, dtype, seed=0):
    rng = np.random.default_rng([sr, n, seed])
    t = np.arange(n)[:, None] / sr
    x = 0.4 * np.sin(2 * np.pi * 440.0 * (1 + np.arange(ch)[None, :]) * t) + 0.1 * rng.standard_normal((n, ch))
    return (np.clip(x, -1, 1) * 32767).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)


def _chunkings(sr, n):
    """name -> chunk lengths summing to n; every rule of the issue's list"""
    first = LC.first_frame_completing(1, sr, SMALL.sample_rate, S)          # the frame count at which segment 0 becomes whole
    assert 600 < first < n
    prime = [997] * (n // 997) + ([n % 997] if n % 997 else [])
    out = {"one": [n], "prime997": prime, "frames600": [1] * 600 + [n - 600]}
    for name, at in (("at", first), ("before", first - 1), ("after", first + 1)):
        out[f"boundary-{name}"] = [at, 0, n - at - 5, 0, 0, 5]
    out["boundary-steps"] = [first - 1, 1, 1, 0, n - first - 1]
    return out


def _stream(st, pcm, chunks, sr, ref):
    """push `chunks`, finish; after every call the rows so far are the one-shot rows and n_ready is the plan's"""
    t = torch.from_numpy(pcm)
    rows, at = [], 0
    for c in chunks:
        want = LC.plan_ready(at + c, sr, SMALL.sample_rate, S) - len(rows)
        assert st.plan(c) == want
        got = st.push(t[at:at + c])
        at += c
        assert got.shape == (want, 1, S)
        if want:
            rows += list(got)
            assert torch.equal(torch.stack(rows), ref[:len(rows)]), f"rows up to {len(rows)} after {at} frames"
    last, n_out = st.finish()
    rows += list(last)
    assert at == pcm.shape[0] and n_out == -(-at * SMALL.sample_rate // sr)
    assert len(rows) == ref.shape[0] and torch.equal(torch.stack(rows), ref)


@pytest.mark.parametrize("sr,ch,dtype", [(44100, 2, np.int16), (48000, 1, np.float32), (8000, 1, np.int16), (16000, 2, np.int16)],
                         ids=["44100-2ch-s16", "48000-1ch-f32", "8000-1ch-s16-up", "16000-2ch-s16-identity"])
def test_streaming_ingest_is_the_one_shot_ingest(small, sr, ch, dtype):
    n = int(2.5 * S * sr / SMALL.sample_rate) + 3
    pcm = _pcm(sr, n, ch, dtype)
    ref = small.ingest(torch.from_numpy(pcm), sr)
    assert ref.shape[0] == 3
    st = small.compile_ingest_stream(sr, ch, torch.from_numpy(pcm).dtype, max_chunk_frames=n)
    for i, (name, chunks) in enumerate(_chunkings(sr, n).items()):
        assert sum(chunks) == n, name
        if i:
            st.reset()                                     # the same object again: a reset stream gives the same bits
        _stream(st, pcm, chunks, sr, ref)
    st.close()


def test_streaming_ingest_short_and_empty_streams(small):
    pcm = _pcm(44100, 37, 2, np.int16)                     # shorter than the filter: nothing is final before the finish
    ref = small.ingest(torch.from_numpy(pcm), 44100)
    st = small.compile_ingest_stream(44100, 2, torch.int16, max_chunk_frames=64)
    for chunks in ([37], [1] * 37, [0, 36, 0, 1]):
        _stream(st, pcm, chunks, 44100, ref)
        st.reset()
    last, n_out = st.finish()                              # no frame at all: one all-zero segment, as the one-shot call
    assert n_out == 0 and last.shape == (1, 1, S) and float(last.abs().max()) == 0.0
    assert torch.equal(last, small.ingest(torch.zeros(0, 2, dtype=torch.int16), 44100))
    st.close()


def test_streaming_ingest_far_from_a_nan_frame_equals_the_one_shot_call(small):
    sr, n = 48000, int(2.5 * S * 3) + 3
    pcm = _pcm(sr, n, 1, np.float32)
    k_nan = n // 2 + 11
    pcm[k_nan, 0] = np.nan
    ref = small.ingest(torch.from_numpy(pcm), sr).reshape(-1).cpu().numpy()
    st = small.compile_ingest_stream(sr, 1, torch.float32, max_chunk_frames=997)
    t = torch.from_numpy(pcm)
    rows = [st.push(t[a:a + 997]) for a in range(0, n, 997)]
    got = torch.cat(rows + [st.finish()[0]]).reshape(-1).cpu().numpy()
    st.close()
    up, down = IO.rates(sr, SMALL.sample_rate)
    n_out, r, hp = IO.plan(n, up, down)
    J = -(-len(hp) // up)
    W = (255 * down) // up + J + 2
    k0 = (np.arange(n_out) + r) * down // up                                   # output n reads frames k0 - J + 1 .. k0
    far = (k0 < k_nan - W) | (k0 - J + 1 > k_nan + W)
    assert far.sum() > n_out - 3 * W and (~far).sum() > J * up // down
    assert np.isfinite(ref[:n_out][far]).all() and np.isnan(ref[:n_out][~far]).any()
    assert np.array_equal(got[:n_out][far], ref[:n_out][far])
    assert got.shape == ref.shape and np.all(got[n_out:] == 0)


def test_streaming_ingest_errors_leave_object_and_handle_usable(small):
    sr, n = 44100, 30000
    pcm = _pcm(sr, n, 2, np.int16, seed=3)
    ref = small.ingest(torch.from_numpy(pcm), sr)
    st = small.compile_ingest_stream(sr, 2, torch.int16, max_chunk_frames=n)
    lib, h = small._lib, small._handle
    dev = torch.from_numpy(pcm).cuda()
    rows = torch.empty(2, S, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    k = ctypes.c_int(-1)
    assert st.plan(n) == 1
    with pytest.raises(YMT3Error, match="max_chunk_frames"):
        st.plan(n + 1)
    for args, word in [((p(dev), n + 1, p(rows), 2), "max_chunk_frames"), ((p(dev), -1, p(rows), 2), "n_frames"),
                       ((p(dev), n, p(rows), 0), "max_segments"), ((None, n, p(rows), 2), "null buffer"), ((p(dev), n, None, 2), "null buffer")]:
        rc = lib.ymt3_ingest_stream_push(h, st.ptr, args[0], args[1], args[2], args[3], ctypes.byref(k), small._stream())
        assert rc == 1 and word in lib.ymt3_last_error().decode(), (args[1:], rc, lib.ymt3_last_error().decode())
    assert lib.ymt3_ingest_stream_push(None, st.ptr, p(dev), n, p(rows), 2, ctypes.byref(k), small._stream()) == 1
    assert lib.ymt3_ingest_stream_finish(h, st.ptr, p(rows), 0, ctypes.byref(k), None, small._stream()) == 1      # one row is due
    _stream(st, pcm, [n], sr, ref)                          # nothing above moved the stream
    with pytest.raises(YMT3Error, match="finished"):
        st.push(torch.from_numpy(pcm[:10]))
    with pytest.raises(YMT3Error, match="finished"):
        st.finish()
    st.reset()
    _stream(st, pcm, [n // 2, n - n // 2], sr, ref)
    with pytest.raises(ValueError):
        st.push(torch.zeros(4, 1, dtype=torch.int16))       # the channel count is the stream's
    with pytest.raises(ValueError):
        st.push(torch.zeros(4, 2, dtype=torch.float32))
    st.close()
    with pytest.raises(ValueError, match="closed"):
        st.ptr
    lib.ymt3_ingest_stream_destroy(None)                    # a no-op
    for bad in (dict(sample_rate=44101), dict(sample_rate=0), dict(n_channels=0), dict(max_chunk_frames=0), dict(max_chunk_frames=(1 << 24) + 1)):
        kw = dict(sample_rate=sr, n_channels=2, dtype=torch.int16, max_chunk_frames=64)
        kw.update(bad)
        with pytest.raises(YMT3Error) as e:
            small.compile_ingest_stream(**kw)
        if bad == dict(sample_rate=44101):                  # the rate pair the one-shot call refuses, with its code
            with pytest.raises(YMT3Error) as e1:
                small.ingest(torch.zeros(10, 2, dtype=torch.int16), 44101)
            assert str(e.value).split(":")[0] == str(e1.value).split(":")[0] == "ymt3 error 4"
    assert torch.equal(small.ingest(torch.from_numpy(pcm), sr), ref)


# ---------------------------------------------------------------------------------------------- 7. incremental detokeniser
MAX_SEGMENTS = 65


@pytest.fixture(scope="module")
def rigs():
    """per channel count: the model; per task a detokeniser; per (task, max_held) a state"""
    out = {K: (_model(cfg, max_batch=1), {}, {}) for K, cfg in CFG.items()}
    yield out
    for m, _, _ in out.values():
        m.close()


def _rig(rigs, case):
    tm = C.task_manager(case["task"])
    m, detoks, states = rigs[tm.num_decoding_channels]
    if case["task"] not in detoks:
        detoks[case["task"]] = m.compile_detokenizer(tm, MAX_SEGMENTS, min(tm.max_note_token_length, m.cfg.max_decode_len))
    d = detoks[case["task"]]
    key = (case["task"], case["max_held"])
    if key not in states:
        states[key] = d.new_state(max_held=case["max_held"])
    return tm, m, d, states[key]


def _device_pushes(tm, m, d, st, case, groups, scores="case", beams=False):
    """the case cut into `groups` through the device -> [(notes, n_invalid, n_forced)] per push, then the finish"""
    st.reset()
    tokens = torch.from_numpy(case["tokens"]).cuda()
    sc = case["scores"] if scores == "case" else None
    sc = None if sc is None else torch.from_numpy(sc).cuda()
    if beams:                                                # hypothesis 0 of a beam call's (n, K, N, L), read in place
        n, K, L = tokens.shape
        wide = torch.randint(0, tm.vocab_size, (n, K, 2, L), dtype=torch.int32, device="cuda")
        wide[:, :, 0] = tokens
        tokens = wide[:, :, 0]
        if sc is not None:
            wsc = -torch.rand(n, K, 2, L, device="cuda")
            wsc[:, :, 0] = sc
            sc = wsc[:, :, 0]
        assert not tokens.is_contiguous()
    out = []
    for g, idx in enumerate(groups):
        lo, hi = idx[0], idx[-1] + 1
        out.append(tm.tokens_to_notes_stream(m, d, st, tokens[lo:hi], case["starts"][lo:hi], LC.horizon(case, groups, g),
                                             scores=None if sc is None else sc[lo:hi]))
    out.append(tm.tokens_to_notes_stream(m, d, st, end_sec=case["end_sec"], scored=sc is not None))
    return out


@pytest.mark.parametrize("case", [c for c in LC.cases() if c["id"] != "hand-max-held"], ids=lambda c: c["id"])
def test_every_push_returns_what_note_stream_returns(rigs, case):
    tm, m, d, st = _rig(rigs, case)
    ref_notes, ref_bad, _ = LC.reference(case)
    for name, groups in LC.splits(case["tokens"].shape[0]):
        pushes, last = LC.stream_reference(case, name)
        got = _device_pushes(tm, m, d, st, case, groups)
        assert [f for _, _, f in got] == [0] * len(got), name
        for g, ((want, want_bad, _), (notes, bad, _)) in enumerate(zip(pushes, got)):
            diff = C.same_notes(notes, list(want))            # finality timing, not only the union
            assert diff is None and bad == want_bad, (name, g, diff)
        assert C.same_notes(got[-1][0], list(last)) is None and got[-1][1] == 0, name
        union = sorted(n for notes, _, _ in got for n in notes)
        assert C.same_notes(union, ref_notes) is None and sum(b for _, b, _ in got) == ref_bad, name
        assert all((n.confidence is None) == (case["scores"] is None) for n in union)


@pytest.mark.parametrize("case", [c for c in LC.cases() if c["family"] == "hand" or c["id"].startswith("mc13_full_plus_256-dense-L65")],
                         ids=lambda c: c["id"])
def test_without_scores_and_through_beam_strides(rigs, case):
    tm, m, d, st = _rig(rigs, case)
    import live_model as LM
    groups = [[i] for i in range(case["tokens"].shape[0])]
    plain = _device_pushes(tm, m, d, st, case, groups, scores=None)
    assert all(n.confidence is None for notes, _, _ in plain for n in notes)
    strided = _device_pushes(tm, m, d, st, case, groups, beams=True)
    contiguous = _device_pushes(tm, m, d, st, case, groups)
    for a, b in zip(strided, contiguous):
        assert C.same_notes(a[0], b[0]) is None and a[1:] == b[1:]
    if case["id"] != "hand-max-held":
        pushes, last = LC.stream_reference(case, "every")
        for (want, _, _), (notes, _, _) in zip(list(pushes) + [(last, 0, 0)], plain):
            assert notes == list(want)                        # == on Note leaves the confidence out: the same notes without scores
    else:                                                     # the bound is reached: the model of the kernel predicts what is forced
        model = LM.DetokCarry(tm.token_table(), 1, tm.codec.steps_per_second, 128, case["max_held"])
        forced = []
        for g, idx in enumerate(groups):
            rec, bad, f = model.push(case["tokens"][idx], [case["starts"][i] for i in idx], LC.horizon(case, groups, g), scores=case["scores"][idx])
            forced.append(f)
            import detok_model as M
            assert C.same_notes(contiguous[g][0], M.to_notes(rec)) is None and contiguous[g][1:] == (bad, f), g
        rec, _, _ = model.finish(case["end_sec"])
        assert C.same_notes(contiguous[-1][0], M.to_notes(rec)) is None
        assert forced[0] == 3 and sum(forced) == 3


def test_detok_push_errors_leave_everything_usable(rigs):
    case = next(c for c in LC.hand_cases() if c["id"] == "hand-pitched-carry")
    tm, m, d, st = _rig(rigs, case)
    n, K, L = case["tokens"].shape
    tokens = torch.from_numpy(case["tokens"]).cuda()
    starts = torch.tensor(case["starts"], dtype=torch.float64).cuda()
    carry = int(m._lib.ymt3_detok_state_carry(st.ptr))
    assert carry == st.carry == K * 128 * (130 - 1 + case["max_held"])        # programs 0 .. 129
    notes = torch.empty((n * K * L + carry) * NOTE_RECORD.itemsize, dtype=torch.uint8).cuda()
    counts = torch.zeros(3, dtype=torch.int32).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st.reset()

    def push(horizon, capacity=n * K * L + carry, seg=n, **over):
        a = dict(tokens=p(tokens), starts=p(starts), notes=p(notes), counts=p(counts))
        a.update(over)
        rc = m._lib.ymt3_detokenize_push(m._handle, d.ptr, st.ptr, a["tokens"], None, seg, L, K * L, L, a["starts"], horizon, a["notes"], capacity,
                                         a["counts"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    assert push(2.0, seg=1)[0] == 0
    for kw, word in [(dict(horizon=1.5, seg=0), "horizon"), (dict(horizon=-math.inf, seg=0), "horizon"), (dict(horizon=math.nan, seg=0), "horizon"),
                     (dict(horizon=8.0, capacity=n * K * L + carry - 1), "capacity"), (dict(horizon=8.0, tokens=None), "tokens_dev"),
                     (dict(horizon=8.0, starts=None), "start_sec_dev"), (dict(horizon=8.0, notes=None), "notes_dev"),
                     (dict(horizon=8.0, counts=None), "counts_dev"), (dict(horizon=8.0, seg=MAX_SEGMENTS + 1, capacity=1 << 40), "n_segments")]:
        rc, msg = push(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
    rc = m._lib.ymt3_detokenize_finish(m._handle, d.ptr, st.ptr, 9.0, p(notes), carry - 1, p(counts), m._stream())
    assert rc == 1 and "capacity" in m._lib.ymt3_last_error().decode()
    other = d.new_state(max_held=2)
    d2 = m.compile_detokenizer(tm, 2, 8)
    rc = m._lib.ymt3_detokenize_finish(m._handle, d2.ptr, other.ptr, 9.0, p(notes), 1 << 30, p(counts), m._stream())
    assert rc == 1 and "another detokeniser" in m._lib.ymt3_last_error().decode()
    d2.close()
    other.close()
    with pytest.raises(ValueError, match="closed"):
        other.ptr
    # the C state knows horizons only (start times are device memory); the wrapper keeps the last start it pushed itself, so after a raw
    # call that went past it the test has to tell it where the stream stands
    st.last_start = case["starts"][0]
    with pytest.raises(ValueError, match="strictly increasing"):
        tm.tokens_to_notes_stream(m, d, st, tokens[0:1], [case["starts"][0]], 4.0)          # segment 0 again
    with pytest.raises(ValueError, match="horizon"):
        tm.tokens_to_notes_stream(m, d, st, tokens[1:2], [case["starts"][1]], 1.0)
    # after all of that the stream goes on as if nothing had happened: segment 0 was pushed, the rest follows
    pushes, last = LC.stream_reference(case, "every")
    rest = tm.tokens_to_notes_stream(m, d, st, tokens[1:], case["starts"][1:], math.inf, scores=None)
    fin = tm.tokens_to_notes_stream(m, d, st, end_sec=case["end_sec"])
    want = sorted([n for want, _, _ in pushes[1:] for n in want] + list(last))
    assert sorted(rest[0] + fin[0]) == want and rest[2] == fin[2] == 0
    with pytest.raises(YMT3Error, match="finished"):
        tm.tokens_to_notes_stream(m, d, st, end_sec=case["end_sec"])
    with pytest.raises(YMT3Error, match="finished"):
        tm.tokens_to_notes_stream(m, d, st, tokens[0:0], [], math.inf)
    one_shot, _ = tm.tokens_to_notes_device(m, tokens, case["starts"], case["end_sec"], detokenizer=d)      # the one-shot call, same scratch
    assert one_shot == LC.reference(case)[0]


# ---------------------------------------------------------------------------------------------- 8. the session
N_AUDIO = int(2.6 * S)                                       # three segments, the last one zero padded


@pytest.fixture(scope="module")
def e2e():
    models = {1: _model(SMALL, max_batch=2), 13: _model(CFG[13], max_batch=2)}
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=3 * S))[0].numpy()[:N_AUDIO]
    yield models, audio
    for m in models.values():
        m.close()


def _live_equals_transcribe(m, audio, tmp_path, chunks, bsz, max_chunk, **mode):
    from yourmt3_amd.transcribe import LiveTranscriber, transcribe
    ref_path, ref = transcribe(m, audio, bsz=bsz, device_detok=True, max_token_length=40, return_notes=True, output_dir=str(tmp_path / "ref"), **mode)
    with LiveTranscriber(m, SMALL.sample_rate, 1, torch.float32, max_chunk_frames=max_chunk, bsz=bsz, max_token_length=40, **mode) as live:
        got, at, per_push = [], 0, []
        for c in chunks:
            new = live.push(audio[at:at + c])
            at += c
            per_push.append(len(new))
            got += new
        assert at == len(audio)
        got += live.finish()
        assert live.forced == 0 and live.n_segments == 3 and got == live.notes
        with pytest.raises(ValueError, match="finished"):
            live.push(audio[:10])
        path = live.write_midi(output_dir=str(tmp_path / "live"))
    assert C.same_notes(sorted(got), ref) is None, C.same_notes(sorted(got), ref)
    assert open(path, "rb").read() == open(ref_path, "rb").read()
    return ref, per_push


@pytest.mark.parametrize("mode", [{}, {"confidence": True}, {"constrained": True}, {"subtask": "drum-only"}, {"num_beams": 2},
                                  {"confidence": True, "min_confidence": 0.02}, {"channels": 13}],
                         ids=["plain", "confidence", "constrained", "subtask", "beams", "min-confidence", "13-channels"])
def test_live_transcriber_equals_transcribe(e2e, tmp_path, mode):
    from yourmt3_amd.task_manager import TaskManager
    models, audio = e2e
    mode = dict(mode)
    m = models[mode.pop("channels", 1)]
    if "subtask" in mode:
        mode["task_manager"] = TaskManager("singing_drum_v1")
    chunks = [3000] * (N_AUDIO // 3000) + [N_AUDIO % 3000]                      # shorter than a segment: at most one segment per push
    ref, per_push = _live_equals_transcribe(m, audio, tmp_path, chunks, 1, 3000, **mode)
    print(f"{mode}: {len(ref)} notes, per push {per_push}")
    if not mode or mode == {"confidence": True}:
        assert len(ref) > 0 and sum(per_push) > 0          # notes do come out before the finish (the other modes' counts are the model's)


def test_a_chunk_that_completes_two_segments_decodes_them_together(e2e, tmp_path):
    models, audio = e2e
    ref, per_push = _live_equals_transcribe(models[1], audio, tmp_path, [2 * S + 5, N_AUDIO - 2 * S - 5], 2, 2 * S + 5, confidence=True)
    assert len(ref) > 0


# ---------------------------------------------------------------------------------------------- 9. handle state
def test_a_live_cycle_leaves_the_decode_bits_of_a_fresh_handle(rigs):
    case = next(c for c in LC.hand_cases() if c["id"] == "hand-pitched-carry")
    tm, m, d, st = _rig(rigs, case)
    audio = O.synthetic_audio(1, m.cfg)

    def decode(model):
        enc = model.encode(model.logmel(audio))
        return model.decode(enc, 24, return_logits=True)

    fresh = _model(CFG[1], max_batch=1)
    want = [t.clone() for t in decode(fresh)]
    fresh.close()
    before = [t.clone() for t in decode(m)]
    pcm = _pcm(44100, 40000, 2, np.int16)
    ing = m.compile_ingest_stream(44100, 2, torch.int16, max_chunk_frames=40000)
    rows = [ing.push(torch.from_numpy(pcm[:25000])), ing.push(torch.from_numpy(pcm[25000:])), ing.finish()[0]]
    assert torch.equal(torch.cat(rows), m.ingest(torch.from_numpy(pcm), 44100))
    ing.close()
    _device_pushes(tm, m, d, st, case, [[0], [1, 2], [3]])
    after = decode(m)
    for a, b, w in zip(after, before, want):
        assert torch.equal(a, b) and torch.equal(a, w)
