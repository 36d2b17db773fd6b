"""The hand rules on the host (yourmt3_amd/hands.py): the specification against the loop model of tests/hand_model.py
on every case and on seeded random ones, the musical outcomes, the refusals with their texts, the MIDI writer's two tracks, the
switches' defaults and the ABI.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bar_cases as BC
import hand_cases as HC
from hand_model import split_hands as model_split
from yourmt3_amd import hands as H
from yourmt3_amd import midi as M
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = HC.all_cases()
MODEL_SLICES = 150                   # the loop model tries 129 x 129 transitions per slice in Python: longer cases are held to it on their first slices


@pytest.fixture(scope="module")
def found():
    """the specification's result of every case, computed once"""
    return {name: H.split_hands(HC.live(rec, count), n_frames, **params) for name, rec, n_frames, params, count in CASES}


def _head(rec, n_frames, p, slices):
    """the records of a case that fall into its first `slices` occupied slots, and the frames that hold them"""
    idx, q, _ = H.select(rec, n_frames, p)
    slots = np.unique(q)
    if slots.size <= slices:
        return rec, n_frames
    keep = np.ones(rec.size, bool)
    keep[idx[q >= slots[slices]]] = False
    return rec[keep], n_frames


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_specification_equals_the_loop_model(case, found):
    name, rec, n_frames, params, count = case
    p = H.check_params(**params)
    hand, split, result = found[name]
    assert hand.dtype == np.uint8 and split.dtype == np.int32 and result.dtype == np.int64 and result.shape == (8,)
    assert hand.shape == (len(HC.live(rec, count)),) and split.shape == (result[0],) and result[7] == 0
    assert result[1] == result[2] + result[3] == int((hand != H.NONE).sum()) and result[2] == int((hand == H.LEFT).sum())
    assert (np.diff(split >> 8) > 0).all() and ((split & 255) <= 128).all() and 0 <= result[4] < 1 << 40
    live, frames = _head(HC.live(rec, count), n_frames, p, MODEL_SLICES)
    if live is not HC.live(rec, count) and len(live) != len(HC.live(rec, count)):
        hand, split, result = H.split_hands(live, frames, **params)
        assert result[0] == MODEL_SLICES
    m_hand, m_split, m_result, ties = model_split(live, frames, p)
    assert hand.tolist() == m_hand and split.tolist() == m_split and result.tolist() == m_result
    if name in HC.TIE_CASES:
        print(f"{name}: {ties} tied steps")
        assert ties > 0


def test_specification_equals_the_loop_model_on_seeded_random_pieces():
    """300 small random pieces with random parameters inside their ranges, the extremes among them"""
    rng = np.random.default_rng(3232)
    for k in range(300):
        frames = int(rng.integers(1, 120))
        n = int(rng.integers(0, 14))
        rec = HC.random_notes(n, frames, seed=1000 + k)
        edge = k % 7 == 0
        params = dict(slice_frames=int(rng.choice([1, 2, 4, 7, 64])), span=int(rng.integers(1, 128)), cut_min=int(rng.integers(0, 128)),
                      middle=int(rng.integers(0, 129)), mid_free=int(rng.integers(0, 129)), rest_slots=int(rng.integers(1, 12)),
                      program_lo=int(rng.integers(0, 4)), program_hi=int(rng.integers(4, 12)))
        params.update({w: int(rng.choice([0, 1024])) if edge else int(rng.integers(0, 30)) for w in ("w_span", "w_cut", "w_centre", "w_mid", "w_move", "w_switch")})
        hand, split, result = H.split_hands(rec, frames, **params)
        m_hand, m_split, m_result, _ = model_split(rec, frames, H.check_params(**params))
        assert hand.tolist() == m_hand and split.tolist() == m_split and result.tolist() == m_result, (k, params)


def _case(name):
    return next(c for c in CASES if c[0] == name)


def test_the_musical_cases_come_out_as_the_issue_says(found):
    hand, split, result = found["climbing_line"]                            # a lone line climbing 50..72: all right, no hand-over, total 0
    assert set(hand.tolist()) == {H.RIGHT} and result.tolist() == [23, 23, 0, 23, 0, 0, 0, 0]
    rec = _case("melody_over_alberti")[1]
    hand, split, result = found["melody_over_alberti"]                      # melody right, accompaniment left, every split 61, total 1
    assert hand.tolist() == [H.RIGHT if x >= 72 else H.LEFT for x in rec["pitch"].tolist()] and set((split & 255).tolist()) == {61}
    assert result.tolist() == [16, 20, 16, 4, 1, 0, 0, 0]
    assert (found["wide_chord"][1] & 255).tolist() == [56] and found["wide_chord"][0].tolist() == [0, 0, 0, 1, 1, 1]
    assert set(found["right_triad"][0].tolist()) == {H.RIGHT}
    assert set(found["left_triad"][0].tolist()) == {H.LEFT} and (found["left_triad"][1] & 255).tolist() == [53]
    assert (found["high_chord"][1] & 255).tolist() == [72] and found["high_chord"][0].tolist() == [0, 0, 1, 1, 1]
    hand, split, result = found["rest_then_left"]                           # right, right, a rest, left, left: free
    assert hand.tolist() == [1, 1, 0, 0] and result[4] == 0 and result[6] == 0


def test_the_edge_cases_are_what_they_say(found):
    assert found["no_records"][2].tolist() == [0] * 8 and found["no_records"][0].size == 0 and found["no_records"][1].size == 0
    hand, split, result = found["none_selected"]
    assert set(hand.tolist()) == {H.NONE} and split.size == 0 and result.tolist() == [0] * 8
    assert found["one_slice"][2][0] == 1 and found["two_slices"][2][0] == 2
    for T in (HC.SCAN - 1, HC.SCAN, HC.SCAN + 1, 2 * HC.SCAN + 1):
        split = found[f"dense{T}"][1]
        assert split.size == T and (split >> 8).tolist() == list(range(T))  # every slot occupied
    gaps = np.diff(found["sparse300"][1] >> 8)
    assert gaps.max() >= H.DEFAULTS["rest_slots"] > gaps.min() and found["sparse300"][2][0] == 300
    assert (found["state128_wins"][1] & 255).tolist() == [128] * 3 and set(found["state128_wins"][0].tolist()) == {H.LEFT}
    assert (found["state0_wins"][1] & 255).tolist() == [0] * 3 and set(found["state0_wins"][0].tolist()) == {H.RIGHT}
    assert {0, 127} <= set(_case("pitch0_and_127")[1]["pitch"].tolist())
    hand, split, result = found["duplicates"]                               # nine records, three slices, duplicates get the same hand
    assert result[:2].tolist() == [3, 9] and hand[0] == hand[1] == hand[2] and hand[4] == hand[5]
    assert found["all_equal_costs"][2][4] == 0 and (found["all_equal_costs"][1] & 255).tolist() == [0] * 20     # every path is free: the smallest state
    near, far = found["gap_rest_minus_1"], found["gap_rest"]                # one slot decides whether the hands may jump
    r = H.DEFAULTS["rest_slots"]
    assert np.diff(near[1] >> 8).tolist() == [4, r - 1, 4] and np.diff(far[1] >> 8).tolist() == [4, r, 4]
    assert near[2][4] > 0 and far[2][4] == 0 and far[0].tolist() == [1, 1, 0, 0]
    hand, split, result = found["frame_edges"]                              # before frame 0 with and without a span inside; the last frame; beyond
    assert hand.tolist() == [0, 0, 1, 1, H.NONE, H.NONE, H.NONE, H.NONE] and (split >> 8).tolist() == [0, 24] and result[5] == 0
    hand, split, result = found["nan_drums_programs"]
    assert hand.tolist() == [1, 1] + [H.NONE] * 7 + [H.NONE, 1, H.NONE, 1, 1, H.NONE, H.NONE] and result[5] == 6
    assert found["programs_at_the_edges"][0].tolist() == [H.NONE, 1, 1, 1, H.NONE, H.NONE, 1, 1]
    assert found["count_below_n"][0].size == 13 and found["count_zero"][0].size == 0 and found["count_zero"][2].tolist() == [0] * 8
    assert found["weights_zero"][2][4] == 0
    heavy = found["weights_1024_5000"]
    assert heavy[2][0] == 5000 and heavy[2][4] > 1 << 28 and heavy[2][6] > 0       # a total far beyond 32 bits' comfort, hand-overs paid
    assert found["random_2000"][2][5] > 0 and found["random_2000"][2][0] > 500


def test_the_bounds_of_the_device_keys_hold_at_the_extreme_parameters():
    """csrc/hands.hip keeps a step's costs in 32 bits relative to the step before's minimum: e <= 454 656 and x <= 132 096"""
    p = H.check_params(**{**HC.HEAVY, "span": 1, "cut_min": 127, "mid_free": 0, "middle": 0})
    worst = 0
    for pitches in ([0, 127], [0, 1, 127], [0, 126, 127], [0, 63, 64, 127], [0], [127], list(range(128))):
        for middle in (0, 128):
            worst = max(worst, int(H.emission(np.array(pitches), {**p, "middle": middle}).max()))
    assert worst <= 454656 and 1024 * 128 + 1024 == 132096
    assert ((454656 + 132096) << 8) + (1024 << 8) + ((1024 << 8) * 128) < 0x3fffffff       # a key with its two additions stays below the pad


@pytest.mark.parametrize("params,text", [
    ({"frames_per_second": 0.0}, "frames_per_second=0.0 must be finite and > 0"), ({"frames_per_second": float("nan")}, "frames_per_second=nan must be finite and > 0"),
    ({"slice_frames": 0}, "slice_frames=0 outside [1, 64]"), ({"slice_frames": 65}, "slice_frames=65 outside [1, 64]"),
    ({"span": 0}, "span=0 outside [1, 127]"), ({"span": 128}, "span=128 outside [1, 127]"),
    ({"cut_min": -1}, "cut_min=-1 outside [0, 127]"), ({"cut_min": 128}, "cut_min=128 outside [0, 127]"),
    ({"middle": -1}, "middle=-1 outside [0, 128]"), ({"middle": 129}, "middle=129 outside [0, 128]"),
    ({"mid_free": -1}, "mid_free=-1 outside [0, 128]"), ({"mid_free": 129}, "mid_free=129 outside [0, 128]"),
    ({"w_span": 1025}, "w_span=1025 outside [0, 1024]"), ({"w_cut": -1}, "w_cut=-1 outside [0, 1024]"), ({"w_centre": 1025}, "w_centre=1025 outside [0, 1024]"),
    ({"w_mid": 1025}, "w_mid=1025 outside [0, 1024]"), ({"w_move": -1}, "w_move=-1 outside [0, 1024]"), ({"w_switch": 1025}, "w_switch=1025 outside [0, 1024]"),
    ({"rest_slots": 0}, "rest_slots=0 outside [1, 1048576]"), ({"rest_slots": (1 << 20) + 1}, "rest_slots=1048577 outside [1, 1048576]"),
    ({"n_programs": 0}, "n_programs=0 outside [1, 256]"), ({"n_programs": 257}, "n_programs=257 outside [1, 256]"),
    ({"drum_program": 130}, "drum_program=130 outside [0, n_programs=130)"),
    ({"program_lo": -1}, "program_lo=-1, program_hi=7 must satisfy 0 <= program_lo <= program_hi < n_programs=130"),
    ({"program_lo": 8}, "program_lo=8, program_hi=7 must satisfy 0 <= program_lo <= program_hi < n_programs=130"),
    ({"program_hi": 130}, "program_lo=0, program_hi=130 must satisfy 0 <= program_lo <= program_hi < n_programs=130")])
def test_parameters_outside_the_limits_are_refused(params, text):
    with pytest.raises(ValueError) as e:
        H.split_hands([], 10, **params)
    assert str(e.value) == text


def test_frames_sizes_and_unknown_parameters_are_refused():
    for n_frames in (0, H.MAX_FRAMES + 1):
        with pytest.raises(ValueError, match=rf"^n_frames={n_frames} outside \[1, 1048576\]$"):
            H.split_hands([], n_frames)
    with pytest.raises(TypeError, match=r"unknown hand parameter\(s\): \['near_div'\]"):
        H.split_hands([], 10, near_div=4)
    with pytest.raises(ValueError, match=r"^max_frames=0 outside \[1, 1048576\]$"):
        H.check_sizes(0, 1)
    with pytest.raises(ValueError, match=r"^max_notes=1048577 outside \[1, 1048576\]$"):
        H.check_sizes(1, (1 << 20) + 1)
    assert list(H.DEFAULTS) == ["frames_per_second", "slice_frames", "program_lo", "program_hi", "span", "w_span", "cut_min", "w_cut", "w_centre", "middle",
                                "mid_free", "w_mid", "w_move", "w_switch", "rest_slots", "n_programs", "drum_program"]
    assert [H.DEFAULTS[k] for k in H.DEFAULTS] == [100.0, 4, 0, 7, 12, 16, 9, 16, 1, 60, 12, 1, 2, 64, 25, 130, 128]
    assert H.split_hands([Note(0.0, 0.5, False, 0, 60)], 100)[0].tolist() == [1]             # a list of Note is taken too
    assert H.hand_splits(np.array([256 * 3 + 61], np.int32), 100.0, 4) == [(0.12, 61)]


def _notes(rec):
    return [Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"])) for r in rec]


def _tracks(data):
    """per track: (its name or None, its program changes, its note events as (tick, on, pitch))"""
    out = {}
    for track, tick, st, payload in M._track_events(data)[1]:
        name, progs, ev = out.setdefault(track, [None, [], []])
        if st == 0xFF and payload[0] == 0x03:
            out[track][0] = bytes(payload[1:]).decode()
        elif st & 0xF0 == 0xC0:
            progs.append((st & 15, payload[0]))
        elif st & 0xF0 in (0x90, 0x80):
            ev.append((tick, st & 0xF0 == 0x90 and payload[1] > 0, payload[0], st & 15))
    return [tuple(out[t]) for t in sorted(out)]


def test_a_split_program_is_two_named_tracks_on_one_channel():
    rec = HC.melody_over_alberti()
    drums = BC.records([0.0, 0.5], pitch=36, program=128, drum=True)
    strings = BC.records([0.1, 0.6], pitch=np.array([50, 80]), program=40, length=0.3)
    notes = sorted(_notes(np.concatenate([rec, drums, strings])))
    hand = H.split_hands(notes, 400)[0].tolist()
    assert set(h for n, h in zip(notes, hand) if n.program == 0 and not n.is_drum) == {0, 1} and all(h == H.NONE for n, h in zip(notes, hand) if n.program != 0)
    plain, data = M.notes_to_midi_bytes(notes), M.notes_to_midi_bytes(notes, hands=hand)
    assert M.notes_to_midi_bytes(notes, hands=None) == plain and M.notes_to_midi_bytes(notes, hands=[H.NONE] * len(notes)) == plain      # nobody has a hand: today's bytes
    tracks, before = _tracks(data), _tracks(plain)
    assert len(tracks) == len(before) + 1 and M.read_midi_track_names(data) == ["R.H.", "L.H."] and M.read_midi_track_names(plain) == []
    right, left = tracks[1], tracks[2]                                      # after the conductor: program 0's two, then 40, then the drums
    assert right[0] == "R.H." and left[0] == "L.H." and right[1] == [(0, 0)] and left[1] == [] and tracks[3][1] == [(1, 40)] and tracks[4][1] == []
    assert {e[3] for e in right[2]} == {e[3] for e in left[2]} == {0} and {e[2] for e in right[2]} == {72, 73, 74, 75} and {e[2] for e in left[2]} == {48, 52, 55}
    assert tracks[3:] == before[2:] and sorted(right[2] + left[2]) == sorted(before[1][2])       # the same events, divided; the other tracks untouched
    assert M.read_midi_open_notes(data) == [0] * 5 and M.read_midi_notes(data) == M.read_midi_notes(plain)
    back = M.read_midi_hands(data)
    assert [n for n, _ in back] == M.read_midi_notes(data)
    assert sorted((n.pitch, round(n.onset, 3), h) for n, h in back) == sorted((n.pitch, round(n.onset, 3), h) for n, h in zip(notes, hand))
    # a track opens with its name, FF 03 04 "R.H.", then the program change; the left one with its name, then its first note
    assert b"\x00\xff\x03\x04R.H.\x00\xc0\x00" in data and b"\x00\xff\x03\x04L.H.\x00\x90" in data
    with pytest.raises(ValueError, match="3 hands"):
        M.notes_to_midi_bytes(notes, hands=[0, 1, 0])


def test_one_pitch_changing_hand_while_sounding_stays_paired():
    """pitch 60 sounds in the left hand until 1.0 s and starts again in the right at 0.5 s: the one-voice rule ends the first span at the
    second's onset BEFORE the notes are divided, so each track's note-ons and note-offs pair up; a note of hand 255 goes with the right;
    a second note on the same tick is dropped whatever its hand and lengthens the span that the first one opened"""
    notes = [Note(0.0, 1.0, False, 0, 60), Note(0.5, 1.5, False, 0, 60), Note(0.0, 0.4, False, 0, 40), Note(0.2, 0.6, False, 0, 90),
             Note(0.5, 1.7, False, 0, 60)]
    hand = [0, 1, 0, 255, 0]
    data = M.notes_to_midi_bytes(notes, hands=hand)
    conductor, right, left = _tracks(data)
    on = lambda sec: M._ticks(sec)
    assert left[2] == [(0, True, 40, 0), (0, True, 60, 0), (on(0.4), False, 40, 0), (on(0.5), False, 60, 0)]
    assert right[2] == [(on(0.2), True, 90, 0), (on(0.5), True, 60, 0), (on(0.6), False, 90, 0), (on(1.7), False, 60, 0)]
    assert M.read_midi_open_notes(data) == [0, 0, 0]
    assert sorted((n.pitch, h) for n, h in M.read_midi_hands(data)) == [(40, 0), (60, 0), (60, 1), (90, 1)]
    assert M.read_midi_notes(data) == M.read_midi_notes(M.notes_to_midi_bytes(notes))
    only_left = M.notes_to_midi_bytes(notes[:1], hands=[0])                 # a hand without a span gets no track; the first track has the program
    assert _tracks(only_left)[1:] == [("L.H.", [(0, 0)], [(0, True, 60, 0), (on(1.0), False, 60, 0)])]
    other = M.notes_to_midi_bytes([Note(0.0, 1.0, False, 5, 60), Note(0.0, 1.0, False, 5, 40)], hands=[1, 0])       # the left track's program is its channel's
    assert [n.program for n in M.read_midi_notes(other)] == [5, 5] and [n.program for n, _ in M.read_midi_hands(other)] == [5, 5]
    assert [n.program for n in M.read_midi_on_beats(other)[0]] == [5, 5]


def test_the_writers_on_the_beats_and_on_the_bars_take_the_hands_and_render_passes_them_on():
    from yourmt3_amd import bars as B
    from yourmt3_amd import beats as T
    from yourmt3_amd import tracking as Tk
    rec, n_frames = BC.piece([4] * 6)[:2]
    notes = sorted(_notes(rec))
    beats = T.track_beats(notes, n_frames)[0]
    metre, bar_result = B.track_bars(notes, beats, n_frames)
    ticks = T.beat_positions(notes, beats)
    hand = H.split_hands(notes, n_frames)[0].tolist()
    assert {0, 1, 255} == set(hand)
    on_beats, on_bars = M.notes_to_midi_bytes_on_beats(notes, ticks, beats), M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, int(bar_result[3]))
    assert M.notes_to_midi_bytes_on_beats(notes, ticks, beats, hands=None) == on_beats
    assert M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, int(bar_result[3]), hands=None) == on_bars
    tracked = {"beats": beats, "ticks": ticks, "tempo": np.zeros(0, np.int32), "metre": metre, "bar_result": bar_result}
    assert Tk.render(notes, tracked, 100.0)[0] == Tk.render(notes, tracked, 100.0, hands=None)[0] == on_bars                 # off: today's bytes
    for data, plain in ((M.notes_to_midi_bytes_on_beats(notes, ticks, beats, hands=hand), on_beats),
                        (M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, int(bar_result[3]), hands=hand), on_bars),
                        (Tk.render(notes, tracked, 100.0, hands=hand)[0], on_bars)):
        assert data != plain and [x for x in M.read_midi_track_names(data)] == ["R.H.", "L.H."] and not any(M.read_midi_open_notes(data))
        assert M.read_midi_on_bars(data) == M.read_midi_on_bars(plain)     # the same notes at the same times, the same conductor track
    assert Tk.render(notes, tracked, 100.0, hands=hand)[0] == M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, int(bar_result[3]), hands=hand)
    assert Tk.render(notes, tracked, 100.0, hands=hand)[1].keys() == Tk.render(notes, tracked, 100.0)[1].keys()
    late = notes + [Note(float("nan"), 1.0, False, 0, 60)]                  # a note without ticks is left out, with its hand
    t2 = np.concatenate([ticks, np.array([[-1, -1]], np.int32)])
    assert M.notes_to_midi_bytes_on_beats(late, t2, beats, hands=hand + [1]) == M.notes_to_midi_bytes_on_beats(notes, ticks, beats, hands=hand)
    assert Tk.ORDER == ("ticks", "beat_result", "tempo", "beats", "bar_result", "metre", "chord_result", "chord", "section_result", "section", "novelty")


def test_hands_are_off_by_default():
    from yourmt3_amd import tracking as Tk
    from yourmt3_amd.task_manager import TaskManager
    from yourmt3_amd.transcribe import LiveTranscriber, estimate_hands, transcribe
    sig = inspect.signature(transcribe).parameters
    assert sig["hands"].default is False and sig["hand_params"].default is None
    assert inspect.signature(TaskManager.tokens_to_notes_device).parameters["hands"].default is None
    assert "hands" not in inspect.signature(LiveTranscriber.__init__).parameters and "estimate_hands()" in LiveTranscriber.__doc__
    assert estimate_hands is H.estimate_hands
    assert list(inspect.signature(estimate_hands).parameters) == ["model", "notes_or_mid_path", "end_sec", "output_path", "params"]
    for f in (M._smf_bytes, M.notes_to_midi_bytes, M.notes_to_midi_bytes_on_beats, M.notes_to_midi_bytes_on_bars, Tk.render):
        assert inspect.signature(f).parameters["hands"].default is None
    with pytest.raises(ValueError, match="hand_params without hands=True"):
        transcribe(None, np.zeros(8, np.float32), hand_params={})


def test_the_abi_declares_lists_and_exports_the_entry_points(tmp_path):
    import shutil
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    names = {"ymt3_hands_create", "ymt3_hands_destroy", "ymt3_split_hands"}
    declared = set(re.findall(r"\b(ymt3_[a-z_0-9]+)\s*\(", header))
    assert names <= declared and names <= set(_lib.SYMBOLS) and declared == set(_lib.SYMBOLS)
    assert "typedef struct ymt3_hands_s* ymt3_hands;" in header and "} ymt3_hand_params;" in header
    assert header.index("ymt3_track_sections(") < header.index("ymt3_hands_create(") < header.index("Measurement hook")      # after the sections
    body = header[header.index("typedef struct ymt3_hand_params {"):header.index("} ymt3_hand_params;")]
    fields = [f.strip() for line in body.splitlines()[1:] for f in re.sub(r"^\s*(double|int32_t)\s+", "", line).rstrip(";").split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.HandParams._fields_] and ctypes.sizeof(_lib.HandParams) == 72          # no implicit padding
    assert fields[1:] == list(H._INTS) and fields == list(H.DEFAULTS)
    gcc = shutil.which("gcc")
    if gcc is not None:
        src = tmp_path / "abi.c"
        src.write_text('#include "ymt3.h"\ntypedef char size_is_72[sizeof(ymt3_hand_params) == 72 ? 1 : -1];\n'
                       'int main(void) { int (*f)(ymt3_handle, const ymt3_hand_params*, long long, long long, ymt3_hands*) = ymt3_hands_create;\n'
                       'int (*g)(ymt3_handle, ymt3_hands, const void*, long long, const int32_t*, long long, uint8_t*, int32_t*, long long, long long*, void*)\n'
                       '= ymt3_split_hands; void (*d)(ymt3_hands) = ymt3_hands_destroy;\n'
                       '(void)f; (void)g; (void)d; return 0; }\n')
        r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    import yourmt3_amd
    for n in ("split_hands", "HandSplitter", "estimate_hands"):
        assert n in yourmt3_amd.__all__ and getattr(yourmt3_amd, n) is getattr(H, n)
    hip = open(os.path.join(ROOT, "yourmt3_amd", "csrc", "hands.hip")).read()
    assert f"constexpr int HAND_SCAN_THREADS = {HC.SCAN};" in hip           # the cases straddle the scan's block
    assert '#include "note_rule.h"' in hip and "note_classify(" in hip and "note_frame_span(" in hip and "note_live_count(" in hip
    from yourmt3_amd import build
    assert "hands.hip" in build.SOURCES


def test_the_object_shares_the_lifecycle_and_stays_out_of_the_models_namespace():
    from yourmt3_amd import model as Mo
    assert issubclass(H.HandSplitter, Mo._Owned) and (H.HandSplitter._destroy, H.HandSplitter._noun) == ("ymt3_hands_destroy", "hand splitter")
    assert "HandSplitter" not in vars(Mo) and "from .hands import HandSplitter" in inspect.getsource(Mo.YourMT3.compile_hand_splitter)
    obj = H.HandSplitter.__new__(H.HandSplitter)
    obj.close()                                      # before _own: nothing to free


def test_the_package_does_not_import_the_oracle():
    code = "import sys, yourmt3_amd, yourmt3_amd.hands, yourmt3_amd.transcribe; assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
