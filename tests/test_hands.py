"""The device hand splitter (include/ymt3.h, hands; yourmt3_amd/csrc/hands.hip) against the host specification, yourmt3_amd/hands.py,
which is always the reference:
  1. every case of tests/hand_cases.py: hand, split and result EQUAL, the outputs pre-filled with sentinels and 8 entries longer, with
     split_dev given and NULL, with and without a count; the wrapper's run the same;
  2. the same call twice, a small call after a large one against a fresh object, two parameter sets alive together;
  3. the refused arguments with their texts, the object usable afterwards; destroy before and after the handle's destruction;
  4. the handle's decode state left alone; transcribe(hands=True), alone and with the beats and the bars, and estimate_hands() end to end."""
import ctypes

import numpy as np
import pytest
import torch

import hand_cases as HC
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd import hands as H
from yourmt3_amd import midi as M
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.task_manager import Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
CASES = HC.all_cases()
IDS = [c[0] for c in CASES]
MAX_FRAMES, MAX_NOTES = 32768, 16384
SENTINEL = 77                                                               # (no hand is 77, no split of these cases either)
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rig():
    """the model, and one splitter per parameter set"""
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


@pytest.fixture(scope="module")
def reference():
    """the specification's answer of every case, computed once: name -> (hand, split, result), the hand as long as the case's records"""
    out = {}
    for name, rec, n_frames, params, count in CASES:
        hand, split, result = H.split_hands(HC.live(rec, count), n_frames, **params)
        out[name] = (hand, split, result)
    return out


def _splitter(rig, params):
    m, objs = rig
    key = repr(sorted(params.items()))
    if key not in objs:
        objs[key] = m.compile_hand_splitter(MAX_FRAMES, MAX_NOTES, **params)
    return m, objs[key]


def _bytes(rec: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


def _count(count):
    return None if count is None else torch.tensor([count, 12345], dtype=torch.int32).cuda()     # (a detokeniser's counter has a second element)


def _raw(m, hs, rec, n_frames, count=None, splits=True):
    """the C call itself -> (hand, split or None, result), pre-filled with the sentinel and 8 entries longer"""
    n = rec.numel() // 32
    cap = hs.max_slices(n, n_frames)
    hand = torch.full((n + 8,), SENTINEL, dtype=torch.uint8).cuda()
    split = torch.full((cap + 8,), SENTINEL, dtype=torch.int32).cuda() if splits else None
    result = torch.full((8 + 8,), SENTINEL, dtype=torch.int64).cuda()
    rc = m._lib.ymt3_split_hands(m._handle, hs.ptr, _p(rec) if n else None, n, _p(count), n_frames, _p(hand), _p(split), cap, _p(result), m._stream())
    assert rc == 0, m._lib.ymt3_last_error().decode()
    return hand, split, result


def check(ref, out):
    """the device's outputs (as _raw returns them) against the specification's, sentinels included: beyond the live records and beyond
    T everything is left alone"""
    want_hand, want_split, want_result = ref
    hand, split, result = (None if t is None else t.cpu().numpy() for t in out)
    assert result[:8].tolist() == want_result.tolist() and (result[8:] == SENTINEL).all()
    n = want_hand.size
    assert hand[:n].tolist() == want_hand.tolist() and (hand[n:] == SENTINEL).all()
    if split is not None:
        k = want_split.size
        assert split[:k].tolist() == want_split.tolist() and (split[k:] == SENTINEL).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_equals_the_specification(rig, reference, case):
    name, rec, n_frames, params, count = case
    m, hs = _splitter(rig, params)
    dev = _bytes(rec).cuda()
    ref = reference[name]
    check(ref, _raw(m, hs, dev, n_frames, _count(count)))
    check(ref, _raw(m, hs, dev, n_frames, _count(count), splits=False))     # split_dev NULL
    if count is None:                                                       # a count that leaves every record: the same
        check(ref, _raw(m, hs, dev, n_frames, _count(len(rec) + 3)))
    # the wrapper, records given on the host
    hand, split, result = hs.run(_bytes(rec), n_frames, count=_count(count))
    assert hand.dtype == np.uint8 and split.dtype == np.int32 and result.dtype == np.int64 and hand.size == len(rec)
    live = ref[0].size
    assert hand[:live].tolist() == ref[0].tolist() and (hand[live:] == H.NONE).all()
    assert split.tolist() == ref[1].tolist() and result.tolist() == ref[2].tolist()


def _named(name):
    return next(c for c in CASES if c[0] == name)


def test_no_records_and_a_null_pointer(rig):
    m, hs = _splitter(rig, {})
    hand, split, result = _raw(m, hs, torch.zeros(0, dtype=torch.uint8).cuda(), 400)
    check(H.split_hands([], 400), (hand, split, result))
    assert result[:8].tolist() == [0] * 8


def test_the_same_call_twice_a_small_call_after_a_large_one_and_two_objects(rig, reference):
    m = rig[0]
    big, small, other = _named("dense2049"), _named("two_slices"), _named("second_params")
    hs = m.compile_hand_splitter(MAX_FRAMES, MAX_NOTES)
    second = m.compile_hand_splitter(MAX_FRAMES, MAX_NOTES, **other[3])     # another parameter set, alive at the same time
    for case in (big, big, small, big):
        check(reference[case[0]], _raw(m, hs, _bytes(case[1]).cuda(), case[2]))
        check(reference[other[0]], _raw(m, second, _bytes(other[1]).cuda(), other[2]))
    fresh = m.compile_hand_splitter(MAX_FRAMES, MAX_NOTES)                  # the small call after the large one against a fresh object
    a = _raw(m, hs, _bytes(small[1]).cuda(), small[2])
    b = _raw(m, fresh, _bytes(small[1]).cuda(), small[2])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for o in (hs, second, fresh):
        o.close()


def test_argument_errors_leave_everything_usable(rig, reference):
    name, rec_np, n_frames, params, _ = _named("melody_over_alberti")
    m, hs = _splitter(rig, params)
    n = len(rec_np)
    rec = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _bytes(rec_np).cuda()])[16:]       # (a view: its misaligned neighbours exist)
    cap = hs.max_slices(n, n_frames)
    hand, split, result = torch.empty(n + 8, dtype=torch.uint8).cuda(), torch.empty(cap + 8, dtype=torch.int32).cuda(), torch.empty(16, dtype=torch.int64).cuda()
    cnt = torch.tensor([n, 0, 0], dtype=torch.int32).cuda()
    m2 = _model(CFG, max_batch=1)
    foreign = m2.compile_hand_splitter(16, 16)

    def split_hands(**over):
        a = dict(h=m._handle, obj=hs.ptr, notes=_p(rec), n=n, count=_p(cnt), n_frames=n_frames, hand=_p(hand), split=_p(split), cap=cap, result=_p(result))
        a.update(over)
        rc = m._lib.ymt3_split_hands(a["h"], a["obj"], a["notes"], a["n"], a["count"], a["n_frames"], a["hand"], a["split"], a["cap"], a["result"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def fill():
        hand.fill_(SENTINEL), split.fill_(SENTINEL), result.fill_(SENTINEL)

    def good():
        fill()
        rc, msg = split_hands()
        assert rc == 0, msg
        check(reference[name], (hand, split, result))

    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    table = [({"n": -1}, f"n_notes=-1 outside [0, max_notes={MAX_NOTES}]"), ({"n": MAX_NOTES + 1}, f"n_notes={MAX_NOTES + 1} outside [0, max_notes={MAX_NOTES}]"),
             ({"notes": None}, "notes_dev is NULL"), ({"notes": off(rec, 4)}, "notes_dev is not aligned to 8 bytes"),
             ({"count": off(cnt, 2)}, "count_dev is not aligned to 4 bytes"),
             ({"n_frames": 0}, f"n_frames=0 outside [1, max_frames={MAX_FRAMES}]"), ({"n_frames": MAX_FRAMES + 1}, f"n_frames={MAX_FRAMES + 1} outside [1, max_frames={MAX_FRAMES}]"),
             ({"hand": None}, "hand_dev is NULL"), ({"split": off(split, 2)}, "split_dev is not aligned to 4 bytes"),
             ({"cap": cap - 1}, f"max_slices={cap - 1} below min(n_notes, ceil(n_frames / slice_frames)) = {cap}"),
             ({"result": None}, "result_dev is NULL"), ({"result": off(result, 4)}, "result_dev is not aligned to 8 bytes"),
             ({"obj": None}, "null hand splitter"), ({"h": None}, "null handle"), ({"obj": foreign.ptr}, "the hand splitter belongs to another handle")]
    for over, text in table:
        fill()
        rc, msg = split_hands(**over)
        assert rc == 1 and msg == text and int((hand != SENTINEL).sum()) == 0 and int((split != SENTINEL).sum()) == 0 and int((result != SENTINEL).sum()) == 0, \
            (over, rc, msg)
        good()                                                              # the object's next call is right
    fill()
    assert split_hands(split=None, cap=0)[0] == 0                           # without split_dev max_slices is not looked at
    check((reference[name][0], np.zeros(0, np.int32), reference[name][2]), (hand, split, result))
    # ymt3_hands_create refuses what it cannot serve, and the handle goes on
    changes = [({"frames_per_second": 0.0}, "frames_per_second=0 must be finite and > 0"), ({"slice_frames": 0}, "slice_frames=0 outside [1, 64]"),
               ({"slice_frames": 65}, "slice_frames=65 outside [1, 64]"), ({"span": 0}, "span=0 outside [1, 127]"), ({"span": 128}, "span=128 outside [1, 127]"),
               ({"cut_min": -1}, "cut_min=-1 outside [0, 127]"), ({"cut_min": 128}, "cut_min=128 outside [0, 127]"),
               ({"middle": -1}, "middle=-1 outside [0, 128]"), ({"middle": 129}, "middle=129 outside [0, 128]"),
               ({"mid_free": -1}, "mid_free=-1 outside [0, 128]"), ({"mid_free": 129}, "mid_free=129 outside [0, 128]"),
               ({"rest_slots": 0}, "rest_slots=0 outside [1, 1048576]"), ({"rest_slots": (1 << 20) + 1}, "rest_slots=1048577 outside [1, 1048576]"),
               ({"program_lo": -1}, "program_lo=-1, program_hi=7 must satisfy 0 <= program_lo <= program_hi < n_programs=130"),
               ({"program_lo": 8}, "program_lo=8, program_hi=7 must satisfy 0 <= program_lo <= program_hi < n_programs=130"),
               ({"program_hi": 130}, "program_lo=0, program_hi=130 must satisfy 0 <= program_lo <= program_hi < n_programs=130"),
               ({"n_programs": 257}, "n_programs=257: at most 256 programs"), ({"drum_program": 130}, "drum_program=130 outside [0, n_programs=130)")]
    for w in ("w_span", "w_cut", "w_centre", "w_mid", "w_move", "w_switch"):
        changes += [({w: -1}, f"{w}=-1 outside [0, 1024]"), ({w: 1025}, f"{w}=1025 outside [0, 1024]")]
    for change, text in changes:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_hand_splitter(16, 16, **change)
        assert str(e.value) == "ymt3 error " + ("4" if "n_programs" in change else "1") + ": " + text
        with pytest.raises(ValueError) as v:                                # the specification refuses the same
            H.check_params(**{**H.DEFAULTS, **change})
        if "n_programs" not in change:
            assert str(v.value) == (text if "frames_per_second" not in change else "frames_per_second=0.0 must be finite and > 0")
    for sizes, text in [((0, 1), "max_frames=0 outside [1, 1048576]"), (((1 << 20) + 1, 1), "max_frames=1048577 outside [1, 1048576]"),
                        ((1, 0), "max_notes=0 outside [1, 1048576]"), ((1, (1 << 20) + 1), "max_notes=1048577 outside [1, 1048576]")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_hand_splitter(*sizes)
        assert str(e.value) == "ymt3 error 1: " + text
        with pytest.raises(ValueError, match=text.replace("[", r"\[").replace("]", r"\]")):
            H.check_sizes(*sizes)
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_hands_create(m._handle, None, 16, 16, ctypes.byref(obj)) == 1 and m._lib.ymt3_last_error().decode() == "params is NULL"
    assert obj.value is None
    m._lib.ymt3_hands_destroy(None)                                         # NULL is a no-op
    m2.close()
    good()


def test_destroy_before_and_after_the_handle_and_close_with_the_model(rig, reference):
    m2 = _model(CFG, max_batch=1)
    early = m2.compile_hand_splitter(64, 64)
    early.close()                                                           # before the handle's destruction
    kept = m2.compile_hand_splitter(64, 64, span=10)
    raw = ctypes.c_void_p()
    params = _lib.HandParams(100.0, *(int(H.DEFAULTS[k]) for k in H._INTS))
    assert m2._lib.ymt3_hands_create(m2._handle, ctypes.byref(params), 64, 64, ctypes.byref(raw)) == 0 and raw.value
    assert kept in m2._owned
    m2.close()                                                              # closes `kept` with the model
    with pytest.raises(ValueError, match="^the hand splitter has been closed$"):
        kept.ptr
    m2._lib.ymt3_hands_destroy(raw)                                         # after the handle's destruction
    name, rec, n_frames, params, _ = _named("sparse300")                    # the first model is untouched
    m, hs = _splitter(rig, params)
    check(reference[name], _raw(m, hs, _bytes(rec).cuda(), n_frames))


def test_decode_is_the_same_before_and_after(rig, reference):
    name, rec, n_frames, params, _ = _named("random_2000")
    m, hs = _splitter(rig, params)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    out = _raw(m, hs, _bytes(rec).cuda(), n_frames)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    check(reference[name], out)


def _music():
    """known music for the small configuration: a melody over an Alberti bass at 120 bpm for 6 s, a kick on every bar"""
    out = []
    for k in range(24):
        t = 0.3 + 0.25 * k
        out += [Note(t, t + 0.2, False, 0, (48, 55, 52, 55)[k % 4])]
        if k % 4 == 0:
            out += [Note(t, t + 0.9, False, 0, 72 + (k // 4) % 3), Note(t, t + 0.01, True, 128, 36)]
    return out


def _patched(monkeypatch):
    """Random weights transcribe no music, so the decode is replaced by the ids of known music (the tokeniser's): ingest, both
    detokenisers, the splitter and the writer run as they are."""
    from yourmt3_amd import transcribe as Tr
    from yourmt3_amd.task_manager import TaskManager
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
    return Tr.transcribe


def _paired(data):
    """every note-on of every track of a format-1 file has its note-off: the tracks' open notes at their ends"""
    return all(n == 0 for n in M.read_midi_open_notes(data))


def test_transcribe_with_hands_end_to_end(rig, tmp_path, monkeypatch):
    from yourmt3_amd import beats as T
    transcribe = _patched(monkeypatch)
    m = rig[0]
    out = lambda name: str(tmp_path / name)
    read = lambda path: open(path, "rb").read()
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=13 * 8191), seed=3)[0].numpy()
    plain, notes_plain = transcribe(m, audio, bsz=2, output_dir=out("plain"), return_notes=True)[:2]
    off, notes_off = transcribe(m, audio, bsz=2, output_dir=out("off"), return_notes=True, hands=False)[:2]
    assert read(plain) == read(off) and notes_plain == notes_off
    host, notes_host, info_host = transcribe(m, audio, bsz=2, output_dir=out("host"), return_notes=True, hands=True)
    dev, notes_dev, info_dev = transcribe(m, audio, bsz=2, output_dir=out("dev"), return_notes=True, hands=True, device_detok=True)
    scored, _, info_scored = transcribe(m, audio, bsz=2, output_dir=out("scored"), return_notes=True, hands=True, device_detok=True, min_confidence=0.0)
    assert read(host) == read(dev) == read(scored) != read(off) and notes_host == notes_dev == notes_plain
    assert set(info_host) == set(info_dev) == set(info_scored) == {"hand", "hand_splits", "hand_result"}
    assert info_host == info_dev and {k: info_scored[k] for k in info_host} == info_host
    # against the specification on the same notes
    n_frames = T.n_frames_of(m.last_ingest_samples / CFG.sample_rate, 100.0)
    hand, split, result = H.split_hands(notes_host, n_frames)
    want = H.hand_summary(hand, split, result, H.DEFAULTS)
    print(f"{len(notes_host)} notes, {result[0]} slices, left {result[2]}, right {result[3]}, total {result[4]}")
    assert info_host == want and result[2] > 0 and result[3] > 0
    pitched = [(n, h) for n, h in zip(notes_host, info_host["hand"]) if not n.is_drum]
    assert all(h == (H.RIGHT if n.pitch >= 72 else H.LEFT) for n, h in pitched)        # the melody right, the accompaniment left
    assert [h for n, h in zip(notes_host, info_host["hand"]) if n.is_drum] == [H.NONE] * sum(n.is_drum for n in notes_host)
    assert read(host) == M.notes_to_midi_bytes(notes_host, hands=info_host["hand"])
    names = M.read_midi_track_names(read(host))
    assert [x for x in names if x in ("R.H.", "L.H.")] == ["R.H.", "L.H."] and _paired(read(host))
    back = M.read_midi_hands(read(host))
    assert sorted((n.pitch, h) for n, h in back if not n.is_drum) == sorted((n.pitch, h) for n, h in pitched)
    assert M.read_midi_notes(read(host)) == M.read_midi_notes(read(off))
    # with the beats and the bars: the same hands, the file on the bars, two staves in it
    kw = dict(bsz=2, return_notes=True, beats=True, bars=True)
    bars_off, _, info_bars_off = transcribe(m, audio, output_dir=out("bars_off"), **kw)
    bars_host, _, info_bars = transcribe(m, audio, output_dir=out("bars_host"), hands=True, **kw)
    bars_dev, _, info_bars_dev = transcribe(m, audio, output_dir=out("bars_dev"), hands=True, device_detok=True, **kw)
    assert read(bars_host) == read(bars_dev) != read(bars_off) and set(info_bars) == set(info_bars_off) | {"hand", "hand_splits", "hand_result"}
    assert all(info_bars[k] == want[k] == info_bars_dev[k] for k in want)
    assert all(info_bars[k] == info_bars_off[k] for k in info_bars_off if k != "ticks") and info_bars["ticks"].tolist() == info_bars_off["ticks"].tolist()
    assert [x for x in M.read_midi_track_names(read(bars_host)) if x in ("R.H.", "L.H.")] == ["R.H.", "L.H."] and _paired(read(bars_host))
    assert M.read_midi_on_bars(read(bars_host)) == M.read_midi_on_bars(read(bars_off))
    # other parameters reach the kernels; the switches are checked
    _, _, high = transcribe(m, audio, bsz=2, output_dir=out("params"), return_notes=True, hands=True, hand_params={"program_lo": 1}, device_detok=True)
    assert set(high["hand"]) == {H.NONE} and high["hand_result"][0] == 0
    with pytest.raises(ValueError, match="hand_params without hands=True"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), hand_params={})


def test_the_detokenisers_records_get_their_hands_in_place(rig):
    from yourmt3_amd import beats as T
    from yourmt3_amd.task_manager import TaskManager
    m = rig[0]
    tm = TaskManager("mt3_full_plus")
    seg = CFG.segment_samples / CFG.sample_rate
    starts = [i * seg for i in range(13)]
    end_sec = 13 * seg
    tokens, _ = tm.notes_to_tokens(_music(), starts, end_sec, max_len=CFG.max_decode_len)
    host_notes = tm.tokens_to_notes([tokens], starts, end_sec=end_sec)
    n_frames = T.n_frames_of(end_sec, 100.0)
    hand, split, result = H.split_hands(host_notes, n_frames)
    toks = torch.from_numpy(tokens).cuda()
    with m.compile_hand_splitter(n_frames, 13 * 48) as hs:
        dev_notes, bad, tracked = tm.tokens_to_notes_device(m, toks, starts, end_sec, hands=hs)
        assert dev_notes == host_notes and bad == 0 and set(tracked) == {"hand", "hand_result", "hand_split"}
        assert tracked["hand"].tolist() == hand.tolist() and tracked["hand_result"].tolist() == result.tolist() and tracked["hand_split"].tolist() == split.tolist()
        with m.compile_beat_tracker(n_frames) as bt:
            both = tm.tokens_to_notes_device(m, toks, starts, end_sec, beats=bt, hands=hs)[2]
            assert set(both) == {"beats", "tempo", "ticks", "hand", "hand_result", "hand_split"} and both["hand"].tolist() == hand.tolist()
            assert set(tm.tokens_to_notes_device(m, toks, starts, end_sec, beats=bt)[2]) == {"beats", "tempo", "ticks"}


def test_estimate_hands_on_a_midi_file(rig, tmp_path):
    from yourmt3_amd.transcribe import estimate_hands
    m = rig[0]
    made = sorted(_music())
    path = M.write_midi(made, str(tmp_path / "piano_in.mid"))
    notes = M.read_midi_notes(open(path, "rb").read())                      # what the file holds: its ticks' times
    got = estimate_hands(m, path, end_sec=6.5, output_path=str(tmp_path / "hands.mid"))
    hand, split, result = H.split_hands(notes, 650)
    assert set(got) == {"hand", "splits", "result", "midi"}
    assert got["hand"] == hand.tolist() and got["result"] == result.tolist() and got["splits"] == H.hand_splits(split, 100.0, 4)
    data = open(str(tmp_path / "hands.mid"), "rb").read()
    assert data == got["midi"] == M.notes_to_midi_bytes(notes, hands=got["hand"]) and _paired(data)
    assert [x for x in M.read_midi_track_names(data) if x in ("R.H.", "L.H.")] == ["R.H.", "L.H."]
    assert sorted((n.onset, n.pitch, h) for n, h in M.read_midi_hands(data)) == sorted((n.onset, n.pitch, h if not n.is_drum else H.NONE) for n, h in zip(notes, got["hand"]))
    other = estimate_hands(m, notes, end_sec=6.5, middle=100, mid_free=0, w_mid=1024)      # a split point far up: everything left
    assert set(h for n, h in zip(notes, other["hand"]) if not n.is_drum) == {H.LEFT}
    empty = estimate_hands(m, [], end_sec=1.0)
    assert empty["hand"] == [] and empty["splits"] == [] and empty["result"] == [0] * 8 and M.read_midi_notes(empty["midi"]) == []
