"""The device bar tracker (include/ymt3.h, bars and key; yourmt3_amd/csrc/bars.hip) against the host specification, yourmt3_amd/bars.py,
which is always the reference:
  1. every case of tests/bar_cases.py: metre and result EQUAL, the outputs pre-filled with sentinels and 8 entries longer, records given
     on the device and on the host, with and without a count;
  2. the same call twice, a small call after a large one against a fresh object, two parameter sets alive together;
  3. the refused arguments with their texts, the object usable afterwards; destroy before and after the handle's destruction;
  4. the handle's decode state left alone; transcribe(beats=True, bars=True) and estimate_bars() end to end."""
import ctypes

import numpy as np
import pytest
import torch

import bar_cases as BC
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T
from yourmt3_amd import midi as M
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.task_manager import Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
CASES = BC.all_cases()
IDS = [c[0] for c in CASES]
MAX_BEATS, MAX_NOTES = 1024, 1024
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
    """the specification's answer of every case, computed once: (metre, result)"""
    return {name: B.track_bars(BC.live(rec, count), beats, n_frames, **params) for name, rec, beats, n_frames, params, count in CASES}


def _tracker(rig, params):
    m, objs = rig
    key = repr(sorted(params.items()))
    if key not in objs:
        objs[key] = m.compile_bar_tracker(MAX_BEATS, MAX_NOTES, **params)
    return m, objs[key]


def _bytes(rec: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


def _count(count):
    return None if count is None else torch.tensor([count, 12345], dtype=torch.int32).cuda()     # (a detokeniser's counter has a second element)


def _beats(beats):
    """-> (beats on the device, one spare entry so that K = 0 has a pointer; the beat tracker's result with K in it)"""
    b = torch.from_numpy(np.concatenate([np.asarray(beats, np.int32), np.array([SENTINEL], np.int32)])).cuda()
    return b, torch.tensor([len(beats), 11, 22, 33], dtype=torch.int64).cuda()


def _raw(m, br, rec, beats, n_frames, count=None):
    """the C call itself -> (metre, result), both pre-filled with the sentinel and 8 entries longer"""
    n = rec.numel() // 32
    b, beat_result = _beats(beats)
    metre = torch.full((br.max_beats + 8,), SENTINEL, dtype=torch.int32).cuda()
    result = torch.full((8 + 8,), SENTINEL, dtype=torch.int64).cuda()
    rc = m._lib.ymt3_track_bars(m._handle, br.ptr, _p(b), _p(beat_result), _p(rec) if n else None, n, None if count is None else _p(count), n_frames,
                                _p(metre), br.max_beats, _p(result), m._stream())
    assert rc == 0, m._lib.ymt3_last_error().decode()
    return metre, result


def check(ref, out):
    """the device's outputs (as _raw returns them) against the specification's, sentinels included"""
    want_metre, want_result = ref
    metre, result = (t.cpu().numpy() for t in out)
    assert result[:8].tolist() == want_result.tolist() and (result[8:] == SENTINEL).all()
    k = want_metre.size
    assert metre[:k].tolist() == want_metre.tolist() and (metre[k:] == SENTINEL).all()           # beyond K: left alone


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_equals_the_specification(rig, reference, case):
    name, rec, beats, n_frames, params, count = case
    m, br = _tracker(rig, params)
    dev = _bytes(rec).cuda()
    check(reference[name], _raw(m, br, dev, beats, n_frames, _count(count)))
    if count is None:                                                       # a count that leaves every record: the same
        check(reference[name], _raw(m, br, dev, beats, n_frames, _count(len(rec) + 3)))
    # the wrapper, records given on the host, one copy back
    metre, result = br.run(beats, _bytes(rec), n_frames, count=_count(count))
    want = reference[name]
    assert metre.dtype == np.int32 and result.dtype == np.int64
    assert metre.tolist() == want[0].tolist() and result.tolist() == want[1].tolist()


def _named(name):
    return next(c for c in CASES if c[0] == name)


def test_the_same_call_twice_a_small_call_after_a_large_one_and_two_objects(rig, reference):
    m = rig[0]
    big, small, other = _named("four_three_four"), _named("beats3"), _named("second_params")
    br = m.compile_bar_tracker(MAX_BEATS, MAX_NOTES)
    second = m.compile_bar_tracker(MAX_BEATS, MAX_NOTES, **other[4])       # another parameter set, alive at the same time
    for case in (big, big, small, big):
        check(reference[case[0]], _raw(m, br, _bytes(case[1]).cuda(), case[2], case[3]))
        check(reference[other[0]], _raw(m, second, _bytes(other[1]).cuda(), other[2], other[3]))
    fresh = m.compile_bar_tracker(MAX_BEATS, MAX_NOTES)                    # the small call after the large one against a fresh object
    a, b = _raw(m, br, _bytes(small[1]).cuda(), small[2], small[3]), _raw(m, fresh, _bytes(small[1]).cuda(), small[2], small[3])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for o in (br, second, fresh):
        o.close()


def test_argument_errors_leave_everything_usable(rig, reference):
    name, rec_np, beats_np, n_frames, params, _ = _named("four4_to_three4")
    m, br = _tracker(rig, params)
    n = len(rec_np)
    rec = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _bytes(rec_np).cuda()])[16:]       # (a view: its misaligned neighbours exist)
    beats, beat_result = _beats(beats_np)
    metre, result = torch.empty(MAX_BEATS + 8, dtype=torch.int32).cuda(), torch.empty(16, dtype=torch.int64).cuda()
    cnt = torch.tensor([n, 0, 0], dtype=torch.int32).cuda()
    m2 = _model(CFG, max_batch=1)
    foreign = m2.compile_bar_tracker(16, 16)

    def track(**over):
        a = dict(h=m._handle, obj=br.ptr, beats=_p(beats), beat_result=_p(beat_result), notes=_p(rec), n=n, count=_p(cnt), n_frames=n_frames,
                 metre=_p(metre), cap=MAX_BEATS, result=_p(result))
        a.update(over)
        rc = m._lib.ymt3_track_bars(a["h"], a["obj"], a["beats"], a["beat_result"], a["notes"], a["n"], a["count"], a["n_frames"], a["metre"], a["cap"],
                                    a["result"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def fill():
        metre.fill_(SENTINEL), result.fill_(SENTINEL)

    def good():
        fill()
        rc, msg = track()
        assert rc == 0, msg
        check(reference[name], (metre, result))

    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    table = [({"beats": None}, "beats_dev is NULL"), ({"beats": off(beats, 2)}, "beats_dev is not aligned to 4 bytes"),
             ({"beat_result": None}, "beat_result_dev is NULL"), ({"beat_result": off(beat_result, 4)}, "beat_result_dev is not aligned to 8 bytes"),
             ({"n": -1}, f"n_notes=-1 outside [0, max_notes={MAX_NOTES}]"), ({"n": MAX_NOTES + 1}, f"n_notes={MAX_NOTES + 1} outside [0, max_notes={MAX_NOTES}]"),
             ({"notes": None}, "notes_dev is NULL"), ({"notes": off(rec, 4)}, "notes_dev is not aligned to 8 bytes"),
             ({"count": off(cnt, 2)}, "count_dev is not aligned to 4 bytes"),
             ({"n_frames": 0}, "n_frames=0 outside [1, 1048576]"), ({"n_frames": (1 << 20) + 1}, "n_frames=1048577 outside [1, 1048576]"),
             ({"metre": None}, "metre_dev is NULL"), ({"metre": off(metre, 2)}, "metre_dev is not aligned to 4 bytes"),
             ({"cap": MAX_BEATS - 1}, f"max_beats={MAX_BEATS - 1} below the bar tracker's max_beats={MAX_BEATS}"),
             ({"result": None}, "result_dev is NULL"), ({"result": off(result, 4)}, "result_dev is not aligned to 8 bytes"),
             ({"obj": None}, "null bar tracker"), ({"h": None}, "null handle"), ({"obj": foreign.ptr}, "the bar tracker belongs to another handle")]
    for over, text in table:
        fill()
        rc, msg = track(**over)
        assert rc == 1 and msg == text and int((metre != SENTINEL).sum()) == 0 and int((result != SENTINEL).sum()) == 0, (over, rc, msg)
        good()                                                              # the object's next call is right
    # no records: no pointer is needed; the beats alone give a path over zeros and no key
    fill()
    assert track(n=0, notes=None, count=None)[0] == 0
    want = B.track_bars([], beats_np, n_frames)
    check(want, (metre, result))
    assert want[1][3] == -1 and want[1][0] > 0
    # ymt3_bars_create refuses what it cannot serve, and the handle goes on
    for change, text in [({"frames_per_second": 0.0}, "frames_per_second=0 must be finite and > 0"), ({"metres": (4, 7)}, "metres[1]=7 outside [2, 6]"),
                         ({"metres": (4, 3, 4)}, "metres[2]=4 is given twice"), ({"near_div": 1}, "near_div=1 outside [2, 64]"),
                         ({"accent_cap": 256}, "accent_cap=256 outside [1, 255]"), ({"w_long": 16}, "w_long=16 outside [0, 15]"),
                         ({"w_kick": -1}, "w_kick=-1 outside [0, 15]"), ({"w_accent": 1025}, "w_accent=1025 outside [0, 1024]"),
                         ({"switch_cost": 4097}, "switch_cost=4097 outside [0, 4096]"),
                         ({"kick_lo": 37}, "kick_lo=37, kick_hi=36 must satisfy 0 <= kick_lo <= kick_hi <= 127"),
                         ({"n_programs": 257}, "n_programs=257: at most 256 programs"), ({"drum_program": 130}, "drum_program=130 outside [0, n_programs=130)")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_bar_tracker(16, 16, **change)
        assert str(e.value) == "ymt3 error " + ("4" if "n_programs" in change else "1") + ": " + text
        with pytest.raises(ValueError):                                    # the specification refuses the same
            B.check_params(**{**B.DEFAULTS, **change})
    for sizes, text in [((0, 1), "max_beats=0 outside [1, 1048577]"), (((1 << 20) + 2, 1), "max_beats=1048578 outside [1, 1048577]"),
                        ((1, 0), "max_notes=0 outside [1, 1048576]"), ((1, (1 << 20) + 1), "max_notes=1048577 outside [1, 1048576]")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_bar_tracker(*sizes)
        assert str(e.value) == "ymt3 error 1: " + text
        with pytest.raises(ValueError):
            B.check_sizes(*sizes)
    params_c = _lib.BarParams(100.0, 0, (ctypes.c_int32 * 5)(), 4, 15, 1, 2, 35, 36, 64, 4, 130, 128)
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_bars_create(m._handle, ctypes.byref(params_c), 16, 16, ctypes.byref(obj)) == 1 and obj.value is None
    assert m._lib.ymt3_last_error().decode() == "n_metres=0 outside [1, 5]"
    assert m._lib.ymt3_bars_create(m._handle, None, 16, 16, ctypes.byref(obj)) == 1 and m._lib.ymt3_last_error().decode() == "params is NULL"
    m._lib.ymt3_bars_destroy(None)                                         # NULL is a no-op
    m2.close()
    good()


def test_destroy_before_and_after_the_handle_and_close_with_the_model(rig, reference):
    m2 = _model(CFG, max_batch=1)
    early = m2.compile_bar_tracker(64, 64)
    early.close()                                                           # before the handle's destruction
    kept = m2.compile_bar_tracker(64, 64, metres=(3, 4))
    raw = ctypes.c_void_p()
    params = _lib.BarParams(100.0, 3, (ctypes.c_int32 * 5)(4, 3, 2), 4, 15, 1, 2, 35, 36, 64, 4, 130, 128)
    assert m2._lib.ymt3_bars_create(m2._handle, ctypes.byref(params), 64, 64, ctypes.byref(raw)) == 0 and raw.value
    assert kept in m2._owned
    m2.close()                                                              # closes `kept` with the model
    with pytest.raises(ValueError, match="^the bar tracker has been closed$"):
        kept.ptr
    m2._lib.ymt3_bars_destroy(raw)                                          # after the handle's destruction
    name, rec, beats, n_frames, params, _ = _named("three4")               # the first model is untouched
    m, br = _tracker(rig, params)
    check(reference[name], _raw(m, br, _bytes(rec).cuda(), beats, n_frames))


def test_decode_is_the_same_before_and_after(rig, reference):
    name, rec, beats, n_frames, params, _ = _named("one_two4_bar")
    m, br = _tracker(rig, params)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    out = _raw(m, br, _bytes(rec).cuda(), beats, n_frames)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    check(reference[name], out)


def _music():
    """known music for the small configuration: a waltz at 120 bpm for 6 s, a long bass note and a kick on every downbeat"""
    out = []
    for k in range(12):
        t = 0.3 + 0.5 * k
        out.append(Note(t, t + 0.2, False, 0, 64 + (k // 3) % 3))
        if k % 3 == 0:
            out += [Note(t, t + 1.4, False, 0, 40 + (k // 3) % 3 * 5), Note(t, t + 0.01, True, 128, 36)]
    return out


def test_transcribe_on_the_bars_end_to_end(rig, tmp_path, monkeypatch):
    from yourmt3_amd import transcribe as Tr
    from yourmt3_amd.task_manager import TaskManager
    transcribe = Tr.transcribe
    m = rig[0]
    out = lambda name: str(tmp_path / name)
    read = lambda path: open(path, "rb").read()
    # Random weights transcribe no music, so the decode is replaced by the ids of known music (the tokeniser's): ingest, both detokenisers,
    # the two trackers, the positions and the writer run as they are.
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

    monkeypatch.setattr(Tr, "_decode", decode)
    monkeypatch.setattr(Tr, "_decode_device", decode_device)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=13 * 8191), seed=3)[0].numpy()
    beats_only, notes_beats, info_beats = transcribe(m, audio, bsz=2, output_dir=out("beats"), return_notes=True, beats=True)
    off, notes_off, info_off = transcribe(m, audio, bsz=2, output_dir=out("off"), return_notes=True, beats=True, bars=False)
    assert read(beats_only) == read(off) and set(info_off) == set(info_beats) == {"beats_sec", "tempo_bpm", "lead_sec", "ticks"}
    host, notes_host, info_host = transcribe(m, audio, bsz=2, output_dir=out("host"), return_notes=True, beats=True, bars=True)
    dev, notes_dev, info_dev = transcribe(m, audio, bsz=2, output_dir=out("dev"), return_notes=True, beats=True, bars=True, device_detok=True)
    scored, _, info_scored = transcribe(m, audio, bsz=2, output_dir=out("scored"), return_notes=True, beats=True, bars=True, device_detok=True, min_confidence=0.0)
    cont, _, info_cont = transcribe(m, audio, bsz=2, output_dir=out("cont"), return_notes=True, beats=True, bars=True, continuous=True)
    assert read(host) == read(dev) == read(scored) == read(cont) != read(off) and notes_host == notes_dev == notes_beats
    for a in (info_dev, info_scored, info_cont):
        assert set(a) == set(info_host) and all(a[k] == info_host[k] for k in a if k != "ticks") and a["ticks"].tolist() == info_host["ticks"].tolist()
    # against the specification on the same notes
    n_frames = T.n_frames_of(m.last_ingest_samples / CFG.sample_rate, 100.0)
    beats, tempo, _ = T.track_beats(notes_host, n_frames)
    metre, result = B.track_bars(notes_host, beats, n_frames)
    print(f"{len(notes_host)} notes, {beats.size} beats, runs {B.metre_runs(metre)}, key {B.key_name(result[3])}")
    assert beats.size >= 10 and B.metre_runs(metre)[0][0] == 3 and len(B.metre_runs(metre)) == 1
    assert info_host["downbeats_sec"] == [b / 100.0 for b, v in zip(beats.tolist(), metre.tolist()) if v & 255 == 0]
    assert info_host["time_signatures"] == B.time_signatures(metre, beats) and info_host["key"] == B.key_name(result[3])
    assert info_host["key_margin"] == int(result[4] - result[5])
    ticks = T.beat_positions(notes_host, beats)
    assert read(host) == M.notes_to_midi_bytes_on_bars(notes_host, ticks, beats, metre, int(result[3]), 100.0)
    back, tempos, signatures, key = M.read_midi_on_bars(read(host))
    assert signatures == info_host["time_signatures"] and signatures[-1][1] == 3 and key == B.key_signature(int(result[3]))
    assert M.read_midi_on_beats(read(host)) == M.read_midi_on_beats(read(off))
    # other parameters reach the kernels; the switches are checked
    _, _, only4 = transcribe(m, audio, bsz=2, output_dir=out("params"), return_notes=True, beats=True, bars=True, bar_params={"metres": (4,)}, device_detok=True)
    assert {nn for _, nn in only4["time_signatures"][-1:]} == {4}
    with pytest.raises(ValueError, match="bars=True without beats=True"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), bars=True)
    with pytest.raises(ValueError, match="bar_params without bars=True"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), beats=True, bar_params={})


def test_the_detokenisers_records_are_barred_in_place(rig):
    from yourmt3_amd.task_manager import TaskManager
    m = rig[0]
    tm = TaskManager("mt3_full_plus")
    seg = CFG.segment_samples / CFG.sample_rate
    starts = [i * seg for i in range(13)]
    end_sec = 13 * seg
    tokens, _ = tm.notes_to_tokens(_music(), starts, end_sec, max_len=CFG.max_decode_len)
    host_notes = tm.tokens_to_notes([tokens], starts, end_sec=end_sec)
    n_frames = T.n_frames_of(end_sec, 100.0)
    beats, tempo, _ = T.track_beats(host_notes, n_frames)
    metre, result = B.track_bars(host_notes, beats, n_frames)
    with m.compile_beat_tracker(n_frames) as bt, m.compile_bar_tracker(T.max_beats(n_frames, bt.lag_min), 13 * 48) as br:
        dev_notes, bad, tracked = tm.tokens_to_notes_device(m, torch.from_numpy(tokens).cuda(), starts, end_sec, beats=bt, bars=br)
        assert dev_notes == host_notes and bad == 0 and tracked["beats"].tolist() == beats.tolist()
        assert tracked["metre"].tolist() == metre.tolist() and tracked["bar_result"].tolist() == result.tolist()
        plain = tm.tokens_to_notes_device(m, torch.from_numpy(tokens).cuda(), starts, end_sec, beats=bt)[2]
        assert set(plain) == {"beats", "tempo", "ticks"}
        with pytest.raises(ValueError, match="bars without beats"):
            tm.tokens_to_notes_device(m, torch.from_numpy(tokens).cuda(), starts, end_sec, bars=br)


def test_estimate_bars_finds_a_waltz(rig, tmp_path):
    from yourmt3_amd.transcribe import estimate_bars
    m = rig[0]
    rec, beats, n_frames, downs, runs, _ = BC.known("three4")
    notes = sorted(Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"])) for r in rec)
    path = str(tmp_path / "flat.mid")
    M.write_midi(notes, path)
    end_sec = n_frames / 100.0
    n_frames = T.n_frames_of(end_sec, 100.0)
    beats = T.track_beats(notes, n_frames)[0]
    got = estimate_bars(m, notes, end_sec=end_sec, output_path=str(tmp_path / "bars.mid"))
    metre, result = B.track_bars(notes, beats, n_frames)
    assert [round(t * 100) for t in got["beats_sec"]] == beats.tolist() and got["metre"].tolist() == metre.tolist()
    assert BC.f_measure(got["downbeats_sec"], downs) >= 0.95 and [nn for _, nn in got["time_signatures"]][-1] == 3
    assert got["key"] == B.key_name(result[3]) and got["key_margin"] == int(result[4] - result[5]) > 0
    back, tempos, signatures, key = M.read_midi_on_bars(open(str(tmp_path / "bars.mid"), "rb").read())
    assert signatures == got["time_signatures"] and key == B.key_signature(int(result[3])) and len(back) > 0
    from_file = estimate_bars(m, path)                                      # a flat .mid: its ticks round the times, so only the metre is asserted
    assert {v >> 8 for v in from_file["metre"].tolist()} == {3} and from_file["midi"][:4] == b"MThd"
    empty = estimate_bars(m, [], end_sec=1.0)
    assert empty["beats_sec"] == [] and empty["downbeats_sec"] == [] and empty["key"] == "none" and empty["time_signatures"] == []
