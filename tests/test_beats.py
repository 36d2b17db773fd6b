"""The device beat tracker (include/ymt3.h, beat tracking; yourmt3_amd/csrc/beats.hip) against the host specification, yourmt3_amd/beats.py,
which is always the reference:
  1. every case of tests/beat_cases.py: beats, n_beats, tempo, result and ticks EQUAL, the outputs pre-filled with sentinels, with and
     without tempo_dev, records given on the device and on the host;
  2. the same call twice, a small call after a large one against a fresh object, two parameter sets alive together;
  3. the refused arguments with their texts, the object usable afterwards; destroy before and after the handle's destruction;
  4. the handle's decode state left alone; transcribe(beats=True) and estimate_beats() end to end."""
import ctypes

import numpy as np
import pytest
import torch

import beat_cases as BC
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd import beats as B
from yourmt3_amd import midi as M
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.task_manager import Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
CASES = BC.all_cases()
IDS = [c[0] for c in CASES]
MAX_FRAMES = 3000
SENTINEL = -7
_p = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rig():
    """the model, and one tracker per parameter set"""
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


@pytest.fixture(scope="module")
def reference():
    """the specification's answer of every case, computed once: (beats, tempo, result, {divisions: ticks})"""
    out = {}
    for name, rec, n_frames, params, count in CASES:
        p = B.check_params(**params)
        live = BC.live(rec, count)
        beats, tempo, result = B.track_beats(live, n_frames, **params)
        ticks = {}
        for q in (0, 4):
            t = np.full((len(rec), 2), -1, np.int32)
            t[:len(live)] = B.beat_positions(live, beats, p["frames_per_second"], q, p["n_programs"], p["drum_program"])
            ticks[q] = t
        out[name] = (beats, tempo, result, ticks)
    return out


def _tracker(rig, params):
    m, objs = rig
    key = repr(sorted(params.items()))
    if key not in objs:
        objs[key] = m.compile_beat_tracker(MAX_FRAMES, **params)
    return m, objs[key]


def _bytes(rec: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


def _count(count):
    return None if count is None else torch.tensor([count, 12345], dtype=torch.int32).cuda()     # (a detokeniser's counter has a second element)


def _raw(m, bt, rec, n_frames, count=None, tempo=True, divisions=0):
    """the two C calls themselves -> (beats, tempo or None, result, ticks), every output pre-filled with the sentinel and 8 entries longer"""
    n = rec.numel() // 32
    cap = B.max_beats(n_frames, bt.lag_min)
    beats = torch.full((cap + 8,), SENTINEL, dtype=torch.int32).cuda()
    lags = torch.full((B.n_windows(n_frames, bt.params["hop_frames"]) + 8,), SENTINEL, dtype=torch.int32).cuda() if tempo else None
    result = torch.full((4 + 8,), SENTINEL, dtype=torch.int64).cuda()
    ticks = torch.full((n + 8, 2), SENTINEL, dtype=torch.int32).cuda()
    rc = m._lib.ymt3_track_beats(m._handle, bt.ptr, _p(rec) if n else None, n, None if count is None else _p(count), n_frames, _p(beats), cap,
                                 None if lags is None else _p(lags), _p(result), m._stream())
    assert rc == 0, m._lib.ymt3_last_error().decode()
    rc = m._lib.ymt3_beat_positions(m._handle, bt.ptr, _p(beats), _p(result), _p(rec) if n else None, n, None if count is None else _p(count), divisions,
                                    _p(ticks), m._stream())
    assert rc == 0, m._lib.ymt3_last_error().decode()
    return beats, lags, result, ticks


def check(ref, out, n, divisions=0):
    """the device's outputs (as _raw returns them) against the specification's, sentinels included"""
    want_beats, want_tempo, want_result, want_ticks = ref
    beats, lags, result, ticks = (None if t is None else t.cpu().numpy() for t in out)
    assert result[:4].tolist() == want_result.tolist() and (result[4:] == SENTINEL).all()
    k = int(want_result[0])
    assert beats[:k].tolist() == want_beats.tolist() and (beats[k:] == SENTINEL).all()            # beyond n_beats: left alone
    if lags is not None:
        assert lags[:want_tempo.size].tolist() == want_tempo.tolist() and (lags[want_tempo.size:] == SENTINEL).all()
    assert ticks[:n].tolist() == want_ticks[divisions].tolist() and (ticks[n:] == SENTINEL).all()  # at or beyond the count: -1, written


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_equals_the_specification(rig, reference, case):
    name, rec, n_frames, params, count = case
    m, bt = _tracker(rig, params)
    dev = _bytes(rec).cuda()
    check(reference[name], _raw(m, bt, dev, n_frames, _count(count)), len(rec))
    check(reference[name], _raw(m, bt, dev, n_frames, _count(count), tempo=False, divisions=4), len(rec), 4)
    # the wrapper, records given on the host, one copy back
    beats, tempo, result, ticks = bt.run(_bytes(rec), n_frames, count=_count(count))
    want = reference[name]
    assert beats.tolist() == want[0].tolist() and tempo.tolist() == want[1].tolist() and result.tolist() == want[2].tolist()
    assert ticks.tolist() == want[3][0].tolist()


def _named(name):
    return next(c for c in CASES if c[0] == name)


def test_the_same_call_twice_a_small_call_after_a_large_one_and_two_objects(rig, reference):
    m = rig[0]
    big, small, other = _named("tempo_step"), _named("frames13"), _named("second_params")
    bt = m.compile_beat_tracker(MAX_FRAMES)
    second = m.compile_beat_tracker(MAX_FRAMES, **other[3])                # another parameter set, alive at the same time
    for case in (big, big, small, big):
        check(reference[case[0]], _raw(m, bt, _bytes(case[1]).cuda(), case[2]), len(case[1]))
        check(reference[other[0]], _raw(m, second, _bytes(other[1]).cuda(), other[2]), len(other[1]))
    fresh = m.compile_beat_tracker(MAX_FRAMES)                             # the small call after the large one against a fresh object
    a, b = _raw(m, bt, _bytes(small[1]).cuda(), small[2]), _raw(m, fresh, _bytes(small[1]).cuda(), small[2])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for o in (bt, second, fresh):
        o.close()


def test_argument_errors_leave_everything_usable(rig, reference):
    name, rec_np, n_frames, params, _ = _named("music_like")
    m, bt = _tracker(rig, params)
    n = len(rec_np)
    rec = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _bytes(rec_np).cuda()])[16:]       # (a view: its misaligned neighbours exist)
    cap = B.max_beats(n_frames, bt.lag_min)
    beats, lags = torch.empty(cap + 8, dtype=torch.int32).cuda(), torch.empty(B.n_windows(n_frames, 100) + 8, dtype=torch.int32).cuda()
    result, ticks, cnt = torch.empty(12, dtype=torch.int64).cuda(), torch.empty((n + 8, 2), dtype=torch.int32).cuda(), torch.tensor([n, 0, 0], dtype=torch.int32).cuda()
    m2 = _model(CFG, max_batch=1)
    foreign = m2.compile_beat_tracker(100)

    def track(**over):
        a = dict(h=m._handle, obj=bt.ptr, notes=_p(rec), n=n, count=_p(cnt), n_frames=n_frames, beats=_p(beats), cap=cap, tempo=_p(lags), result=_p(result))
        a.update(over)
        rc = m._lib.ymt3_track_beats(a["h"], a["obj"], a["notes"], a["n"], a["count"], a["n_frames"], a["beats"], a["cap"], a["tempo"], a["result"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def positions(**over):
        a = dict(h=m._handle, obj=bt.ptr, beats=_p(beats), result=_p(result), notes=_p(rec), n=n, count=_p(cnt), q=0, ticks=_p(ticks))
        a.update(over)
        rc = m._lib.ymt3_beat_positions(a["h"], a["obj"], a["beats"], a["result"], a["notes"], a["n"], a["count"], a["q"], a["ticks"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def fill():
        beats.fill_(SENTINEL), lags.fill_(SENTINEL), result.fill_(SENTINEL), ticks.fill_(SENTINEL)

    def untouched():
        return all(int((t != SENTINEL).sum()) == 0 for t in (beats, lags, result, ticks))

    def good():
        fill()
        rc, msg = track()
        assert rc == 0, msg
        rc, msg = positions()
        assert rc == 0, msg
        check(reference[name], (beats, lags, result, ticks), n)

    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    track_table = [({"n_frames": 0}, f"n_frames=0 outside [1, max_frames={MAX_FRAMES}]"),
                   ({"n_frames": MAX_FRAMES + 1}, f"n_frames={MAX_FRAMES + 1} outside [1, max_frames={MAX_FRAMES}]"),
                   ({"n": -1}, "n_notes=-1 outside [0, 536870912]"), ({"notes": None}, "notes_dev is NULL"), ({"notes": off(rec, 4)}, "notes_dev is not aligned to 8 bytes"),
                   ({"count": off(cnt, 2)}, "count_dev is not aligned to 4 bytes"), ({"beats": None}, "beats_dev is NULL"),
                   ({"beats": off(beats, 2)}, "beats_dev is not aligned to 4 bytes"),
                   ({"cap": cap - 1}, f"max_beats={cap - 1} below n_frames / ceil(lag_min / 2) + 1 = {cap}"),
                   ({"tempo": off(lags, 2)}, "tempo_dev is not aligned to 4 bytes"), ({"result": None}, "result_dev is NULL"),
                   ({"result": off(result, 4)}, "result_dev is not aligned to 8 bytes"), ({"obj": None}, "null beat tracker"), ({"h": None}, "null handle"),
                   ({"obj": foreign.ptr}, "the beat tracker belongs to another handle")]
    for over, text in track_table:
        fill()
        rc, msg = track(**over)
        assert rc == 1 and msg == text and untouched(), (over, rc, msg)     # YMT3_ERR_ARG and its text
        good()                                                              # the object's next call is right
    good()
    kept = [t.clone() for t in (beats, lags, result)]
    position_table = [({"q": 7}, "divisions=7 must be 0 or a divisor of 480"), ({"q": -1}, "divisions=-1 must be 0 or a divisor of 480"),
                      ({"n": (1 << 29) + 1}, "n_notes=536870913 outside [0, 536870912]"), ({"notes": None}, "notes_dev is NULL"),
                      ({"beats": None}, "beats_dev is NULL"), ({"result": None}, "result_dev is NULL"), ({"result": off(result, 4)}, "result_dev is not aligned to 8 bytes"),
                      ({"ticks": None}, "ticks_dev is NULL"), ({"ticks": off(ticks, 4)}, "ticks_dev is not aligned to 8 bytes"),
                      ({"obj": foreign.ptr}, "the beat tracker belongs to another handle")]
    for over, text in position_table:
        ticks.fill_(SENTINEL)
        rc, msg = positions(**over)
        assert rc == 1 and msg == text and int((ticks != SENTINEL).sum()) == 0, (over, rc, msg)
        assert positions()[0] == 0
        check(reference[name], (beats, lags, result, ticks), n)
    assert all(torch.equal(a, b) for a, b in zip(kept, (beats, lags, result)))
    # no records: no beats, and no record pointer is needed
    fill()
    assert track(n=0, notes=None, count=None)[0] == 0 and result[:4].tolist() == [0, 0, 0, 0] and int((beats != SENTINEL).sum()) == 0
    assert positions(n=0, notes=None, ticks=None)[0] == 0
    # ymt3_beats_create refuses what it cannot serve, and the handle goes on
    base = dict(B.DEFAULTS)
    for change, text in [({"frames_per_second": 0.0}, "frames_per_second=0 must be finite and > 0"), ({"bpm_prior": float("nan")}, "bpm_prior=nan must be finite and > 0"),
                         ({"bpm_min": 250.0}, "bpm_min=250 above bpm_max=240"), ({"tightness": 1e5}, "tightness=100000 above 10000"),
                         ({"bpm_max": 2400.0}, "lag_min=3, lag_max=150 (60 frames_per_second / bpm_max, / bpm_min) must satisfy 4 <= lag_min <= lag_max <= 512"),
                         ({"window_frames": 299}, "window_frames=299 outside [2 * lag_max=300, 2048]"), ({"hop_frames": 0}, "hop_frames=0 outside [1, window_frames=800]"),
                         ({"lag_step_max": -1}, "lag_step_max=-1 outside [0, 512]"), ({"onset_cap": 256}, "onset_cap=256 outside [1, 255]"),
                         ({"n_programs": 257}, "n_programs=257: at most 256 programs"), ({"drum_program": 130}, "drum_program=130 outside [0, n_programs=130)")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_beat_tracker(100, **change)
        assert str(e.value) == "ymt3 error " + ("4" if "n_programs" in change else "1") + ": " + text
        with pytest.raises(ValueError):                                    # the specification refuses the same
            B.check_params(**{**base, **change})
    for frames, kw, text in [(0, {}, "max_frames=0 outside [1, 1048576]"), ((1 << 20) + 1, {}, "max_frames=1048577 outside [1, 1048576]"),
                             (1 << 20, dict(hop_frames=1, onset_cap=255, window_frames=2048), "max_frames=1048576 with hop_frames=1: the tempo path's sums could pass 2^62")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_beat_tracker(frames, **kw)
        assert str(e.value) == "ymt3 error 1: " + text
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_beats_create(m._handle, None, 100, ctypes.byref(obj)) == 1 and m._lib.ymt3_last_error().decode() == "params is NULL" and obj.value is None
    m._lib.ymt3_beats_destroy(None)                                        # NULL is a no-op
    m2.close()
    good()


def test_destroy_before_and_after_the_handle_and_close_with_the_model(rig, reference):
    m2 = _model(CFG, max_batch=1)
    early = m2.compile_beat_tracker(500)
    early.close()                                                           # before the handle's destruction
    kept = m2.compile_beat_tracker(500, hop_frames=50)
    raw = ctypes.c_void_p()
    p = B.DEFAULTS
    params = _lib.BeatParams(*(float(p[k]) for k in ("frames_per_second", "bpm_min", "bpm_max", "bpm_prior", "prior_octaves", "tightness")),
                             *(int(p[k]) for k in ("window_frames", "hop_frames", "lag_step_max", "onset_cap", "n_programs", "drum_program")))
    assert m2._lib.ymt3_beats_create(m2._handle, ctypes.byref(params), 500, ctypes.byref(raw)) == 0 and raw.value
    assert kept in m2._owned
    m2.close()                                                              # closes `kept` with the model
    with pytest.raises(ValueError, match="^the beat tracker has been closed$"):
        kept.ptr
    m2._lib.ymt3_beats_destroy(raw)                                         # after the handle's destruction
    name, rec, n_frames, params, _ = _named("metronome120")                 # the first model is untouched
    m, bt = _tracker(rig, params)
    check(reference[name], _raw(m, bt, _bytes(rec).cuda(), n_frames), len(rec))


def test_decode_is_the_same_before_and_after(rig, reference):
    name, rec, n_frames, params, _ = _named("accelerando")
    m, bt = _tracker(rig, params)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    out = _raw(m, bt, _bytes(rec).cuda(), n_frames)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    check(reference[name], out, len(rec))


def _music():
    """known music for the small configuration: 120 bpm for 6 s, an off-beat note every second"""
    return [Note(0.3 + 0.5 * k, 0.5 + 0.5 * k, False, 0, 60 + k % 5) for k in range(12)] + [Note(0.56 + 1.0 * k, 0.7 + 1.0 * k, False, 0, 72) for k in range(5)]


def test_transcribe_on_the_beats_end_to_end(rig, tmp_path, monkeypatch):
    from yourmt3_amd import transcribe as T
    from yourmt3_amd.task_manager import TaskManager
    transcribe = T.transcribe
    m = rig[0]
    out = lambda name: str(tmp_path / name)
    read = lambda path: open(path, "rb").read()
    # the switch is off: the bytes of a call that never heard of the argument, on the model's own ids
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191), seed=3)[0].numpy()      # 5 segments, as tests/test_velocity.py transcribes them
    never, flat = transcribe(m, audio, bsz=2, output_dir=out("never"), return_notes=True)
    off, flat_off = transcribe(m, audio, bsz=2, output_dir=out("off"), return_notes=True, beats=False)
    assert read(never) == read(off) and flat == flat_off and len(flat) > 0
    # Random weights transcribe no music, so from here on the decode is replaced by the ids of known music (the tokeniser's): ingest, both
    # detokenisers, the tracker, the positions and the writer run as they are.
    tm = TaskManager("mt3_full_plus")

    def ids(model, segments, L):
        n = int(segments.shape[0])
        starts = [i * model.cfg.segment_samples / model.cfg.sample_rate for i in range(n)]
        return tm.notes_to_tokens(_music(), starts, model.last_ingest_samples / model.cfg.sample_rate, max_len=L)[0]

    def decode(model, segments, bsz, L, continuous, scored, kw):
        t = ids(model, segments, L)
        return [t], ([np.zeros(t.shape, np.float32)] if scored else None)

    def decode_device(model, segments, bsz, L, continuous, scored, kw):
        t = torch.from_numpy(ids(model, segments, L)).cuda()
        return t, (torch.zeros(t.shape, dtype=torch.float32).cuda() if scored else None)

    monkeypatch.setattr(T, "_decode", decode)
    monkeypatch.setattr(T, "_decode_device", decode_device)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=13 * 8191), seed=3)[0].numpy()
    plain, notes_plain = transcribe(m, audio, bsz=2, output_dir=out("plain"), return_notes=True)
    assert len(notes_plain) == len(_music())
    host, notes_host, info_host = transcribe(m, audio, bsz=2, output_dir=out("host"), return_notes=True, beats=True)
    dev, notes_dev, info_dev = transcribe(m, audio, bsz=2, output_dir=out("dev"), return_notes=True, beats=True, device_detok=True)
    scored, notes_scored, info_scored = transcribe(m, audio, bsz=2, output_dir=out("scored"), return_notes=True, beats=True, device_detok=True, min_confidence=0.0)
    vel, notes_vel, info_vel = transcribe(m, audio, bsz=2, output_dir=out("vel"), return_notes=True, beats=True, device_detok=True, velocity=True)
    assert read(host) == read(dev) == read(scored) != read(plain) and notes_host == notes_dev == notes_plain
    for a in (info_dev, info_scored, info_vel):
        assert a["beats_sec"] == info_host["beats_sec"] and a["tempo_bpm"] == info_host["tempo_bpm"] and a["lead_sec"] == info_host["lead_sec"]
        assert a["ticks"].tolist() == info_host["ticks"].tolist()
    # against the specification on the same notes
    n_frames = B.n_frames_of(m.last_ingest_samples / CFG.sample_rate, 100.0)
    beats, tempo, _ = B.track_beats(notes_host, n_frames)
    print(f"{len(notes_host)} notes, {beats.size} beats, tempo {sorted(set(tempo.tolist()))}")
    assert beats.size >= 10 and set(tempo.tolist()) == {50}
    assert info_host["beats_sec"] == [b / 100.0 for b in beats.tolist()] and info_host["tempo_bpm"] == [120.0] * tempo.size
    assert info_host["ticks"].tolist() == B.beat_positions(notes_host, beats).tolist() and info_host["lead_sec"] == B.lead_sec(beats)
    assert read(host) == M.notes_to_midi_bytes_on_beats(notes_host, B.beat_positions(notes_host, beats), beats, 100.0)
    back, tempos = M.read_midi_on_beats(read(host))                         # the file holds the map, and playback the performance
    assert tempos == B.tempo_map(beats, 100.0) and len(back) == len(notes_host)
    assert max(abs(a.onset - b.onset - info_host["lead_sec"]) for a, b in zip(back, notes_host)) <= float(np.diff(beats).max()) / 100.0 / 960 + 0.5e-6 * beats.size
    assert any(t % 120 for t in M.note_on_ticks(read(host)))
    # quantised: every note-on on a sixteenth, with both detokenisers the same bytes
    quant, _, info_q = transcribe(m, audio, bsz=2, output_dir=out("quant"), return_notes=True, beats=True, quantize=4, device_detok=True)
    quant_host = transcribe(m, audio, bsz=2, output_dir=out("quant_host"), beats=True, quantize=4)[0]
    assert info_q["ticks"].tolist() == B.beat_positions(notes_host, beats, divisions=4).tolist() and read(quant) == read(quant_host)
    ons = M.note_on_ticks(read(quant))
    assert len(ons) == len(notes_host) and all(t % 120 == 0 for t in ons)
    # other parameters reach the kernels; parameters without the switch are refused
    _, _, slow = transcribe(m, audio, bsz=2, output_dir=out("params"), return_notes=True, beats=True, beat_params={"bpm_prior": 60.0, "bpm_max": 100.0})
    assert set(slow["tempo_bpm"]) == {60.0}
    with pytest.raises(ValueError, match="beat_params or quantize without beats=True"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), quantize=4)


def test_the_detokenisers_records_are_tracked_in_place(rig):
    """TaskManager.tokens_to_notes_device(beats=, quantize=) on the ids of known music: the count read on the device, one copy back, the
    bytes those of the host detokeniser's notes through the same kernels, and with quantize=4 every note-on on a sixteenth"""
    from yourmt3_amd.metrics import to_records
    from yourmt3_amd.task_manager import TaskManager
    m = rig[0]
    tm = TaskManager("mt3_full_plus")
    seg = CFG.segment_samples / CFG.sample_rate
    starts = [i * seg for i in range(13)]
    end_sec = 13 * seg
    notes = _music()
    tokens, _ = tm.notes_to_tokens(notes, starts, end_sec, max_len=CFG.max_decode_len)
    host_notes = tm.tokens_to_notes([tokens], starts, end_sec=end_sec)
    n_frames = B.n_frames_of(end_sec, 100.0)
    beats, tempo, _ = B.track_beats(host_notes, n_frames)
    assert len(host_notes) == len(notes) and beats.size >= 10 and set(tempo.tolist()) == {50}
    with m.compile_beat_tracker(n_frames) as bt:
        for q in (0, 4):
            dev_notes, bad, tracked = tm.tokens_to_notes_device(m, torch.from_numpy(tokens).cuda(), starts, end_sec, beats=bt, quantize=q)
            want = B.beat_positions(host_notes, beats, divisions=q)
            assert dev_notes == host_notes and bad == 0
            assert tracked["beats"].tolist() == beats.tolist() and tracked["tempo"].tolist() == tempo.tolist() and tracked["ticks"].tolist() == want.tolist()
            b2, t2, _, ticks2 = bt.run(_bytes(to_records(host_notes)), n_frames, divisions=q)         # the host detokeniser's notes, uploaded
            data = M.notes_to_midi_bytes_on_beats(dev_notes, tracked["ticks"], tracked["beats"], 100.0)
            assert data == M.notes_to_midi_bytes_on_beats(host_notes, ticks2, b2, 100.0) == M.notes_to_midi_bytes_on_beats(host_notes, want, beats, 100.0)
            assert data != M.notes_to_midi_bytes(host_notes)
            ons = M.note_on_ticks(data)
            assert len(ons) == len(notes) and (q == 0 or all(t % 120 == 0 for t in ons))
        assert any(t % 120 for t in M.note_on_ticks(M.notes_to_midi_bytes_on_beats(host_notes, B.beat_positions(host_notes, beats), beats, 100.0)))


def test_estimate_beats_finds_a_metronome(rig, tmp_path):
    from yourmt3_amd.transcribe import estimate_beats
    m = rig[0]
    notes = [Note(0.5 + 0.5 * k, 0.6 + 0.5 * k, False, 0, 60) for k in range(24)]
    path = str(tmp_path / "flat.mid")
    M.write_midi(notes, path)
    for source in (notes, path):
        got = estimate_beats(m, source, end_sec=12.5, output_path=str(tmp_path / "beats.mid"))
        assert set(got["tempo_bpm"]) == {120.0} and got["lead_sec"] == 0.0
        assert set(np.rint(np.diff(got["beats_sec"]) * 100).tolist()) == {50.0} and set(got["beats_sec"]) <= {0.5 + 0.5 * k for k in range(24)}
        assert all(t % 480 == 0 for t in got["ticks"][:, 0].tolist())
        back, tempos = M.read_midi_on_beats(open(str(tmp_path / "beats.mid"), "rb").read())
        assert tempos == [(0, 500000)] and [round(n.onset, 6) for n in back] == [round(n.onset, 6) for n in notes]
    assert estimate_beats(m, [], end_sec=1.0)["beats_sec"] == []
