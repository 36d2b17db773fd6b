"""Chords without a GPU: the host specification (yourmt3_amd/chords.py) against the loop model (tests/chord_model.py) on every case, what
the rules find on music whose chords are known, names, segments and .lab text, the markers in the MIDI file, the parameter refusals and
the ABI surface."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bar_cases as BC
import chord_cases as CC
from chord_model import track_chords as model_track
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T
from yourmt3_amd import chords as Ch
from yourmt3_amd import midi as M
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = CC.all_cases()

# Per-beat label accuracy of the specification on the known music, over the tracked beats within 70 ms of a generated beat, as (hits,
# beats) computed by test_known_music_gets_its_chords_as_recorded when these rules were written: with the bar tracker's metre, and
# without one.  The test asserts the recorded ratio minus 0.05.
RECORDED = {name: (1.0, 1.0) for name in CC.MUSIC}
RECORDED.update(silence=(39 / 40, 39 / 40), fast_changes=(45 / 48, 45 / 48), mixed=(60 / 60, 58 / 60))


def _both(case):
    """a case's metres to run: its own and, if it has one, none as well"""
    return [case[4]] if case[4] is None else [case[4], None]


@pytest.fixture(scope="module")
def tracked():
    """the specification's result of every case with its metre, computed once"""
    return {name: Ch.track_chords(CC.live(rec, count), beats, n_frames, metre=metre, **params) for name, rec, beats, n_frames, metre, params, count in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_specification_equals_the_loop_model(case, tracked):
    name, rec, beats, n_frames, metre, params, count = case
    for m in _both(case):
        chord, result = tracked[name] if m is metre else Ch.track_chords(CC.live(rec, count), beats, n_frames, metre=m, **params)
        m_chord, m_result, ties = model_track(CC.live(rec, count), beats, n_frames, m, Ch.check_params(**params))
        assert chord.dtype == np.int32 and result.dtype == np.int64 and result.shape == (8,)
        assert chord.shape == ((len(beats),) if len(beats) >= 2 else (0,))
        assert chord.tolist() == m_chord and result.tolist() == m_result
        assert result[1] < 1 << 42 and result[4:].tolist() == [0, 0, 0, 0]
    if name in CC.TIE_CASES:
        print(f"{name}: {ties} tied beats")
        assert ties > 0


def test_the_edge_cases_are_what_they_say(tracked):
    for k in (0, 1):
        assert tracked[f"beats{k}"][0].size == 0 and tracked[f"beats{k}"][1].tolist() == [0] * 8
    for k in (2, 63, 64, 65, 128, 129):
        assert tracked[f"beats{k}"][0].size == k
    names = lambda name: {Ch.QUALITIES[(v & 255) // 12] for v in tracked[name][0].tolist() if v & 255 != 255}
    assert names("qualities1") == {"maj"} and names("qualities5") <= set(Ch.QUALITIES[:5]) and "7" in names("qualities6")
    assert {"min7", "7", "maj7"} <= names("qualities8")
    for name in ("no_records", "drums_only"):                              # nothing pitched: N on every beat, one run
        chord, result = tracked[name]
        assert (chord == 255 * 256 + 255).all() and result[:3].tolist() == [1, 1024 * 300 * chord.size, chord.size]
    assert {v & 255 for v in tracked["one_pitch_class"][0].tolist()} == {2}                       # D: the root of its major triad, the first state
    assert {v & 255 for v in tracked["root_and_fifth"][0].tolist()} == {0}                        # C major before C minor
    assert {v & 255 for v in tracked["aug_no_bass"][0].tolist()} == {36}                          # C aug before E aug and Ab aug
    assert {v & 255 for v in tracked["aug_with_bass"][0].tolist()} == {36 + 4} and tracked["aug_with_bass"][0][0] >> 8 == 40      # the bass E names the root
    assert tracked["w_none_0"][1][2] == 0 and tracked["silence"][1][2] > 0                        # N costs nothing to leave out
    assert tracked["change_cost_0"][1][0] >= tracked["mixed"][1][0] >= tracked["change_cost_4096"][1][0] == 1
    assert tracked["nonfinite_and_out_of_range"][1][3] == 5
    late = tracked["beats_beyond_frames"][0]
    assert late[-1] == 255 * 256 + 255 and late[0] & 255 != 255
    assert tracked["count_zero"][1][2] == tracked["count_zero"][0].size and tracked["count_below_n"][0].tolist() != tracked["pop"][0].tolist()
    assert len(next(c for c in CASES if c[0] == "records_1024")[1]) == 1024


def test_known_music_gets_its_chords_as_recorded(tracked):
    for name in CC.MUSIC:
        rec, beats, n_frames, metre, truth = CC.music(name)
        hits, n = CC.accuracy(tracked[name][0], beats, truth)
        hits0, n0 = CC.accuracy(Ch.track_chords(rec, beats, n_frames)[0], beats, truth)
        print(f"{name}: {beats.size} beats, with the metre {hits}/{n}, without {hits0}/{n0}, {tracked[name][1][0]} runs")
        assert n == n0 >= 0.9 * len(truth)
        assert hits / n >= RECORDED[name][0] - 0.05 and hits0 / n0 >= RECORDED[name][1] - 0.05


def test_names_segments_and_lab_text():
    assert [Ch.chord_name(v) for v in (0, 21, 35, 36, 48, 67, 72, 86, 255)] == ["C", "Am", "Bdim", "Caug", "Csus4", "G7", "Cmaj7", "Dm7", "N"]
    assert Ch.chord_name(0, 52) == "C/E" and Ch.chord_name(0, 43) == "C/G" and Ch.chord_name(0, 48) == "C" and Ch.chord_name(0, 50) == "C"
    assert Ch.chord_name(67, 41) == "G7/F" and Ch.chord_name(0, 255) == "C" and Ch.chord_name(255, 40) == "N" and Ch.chord_name(10 + 12) == "Bbm"
    assert [Ch.harte_label(v) for v in (0, 93, 67, 48, 255)] == ["C:maj", "A:min7", "G:7", "C:sus4", "N"]
    for bad in (96, -1, 254):
        with pytest.raises(ValueError):
            Ch.chord_name(bad)
    beats = BC.steady(6, 100, 50)
    chord = np.array([256 * 52 + 0, 256 * 48 + 0, 256 * 255 + 255, 256 * 45 + 21, 256 * 45 + 21, 256 * 43 + 67], np.int32)
    seg = Ch.chord_segments(chord, beats)
    assert seg == [(0, 2, 0, 52), (2, 3, 255, 255), (3, 5, 21, 45), (5, 6, 67, 43)]
    assert Ch.chord_lab(seg, beats, 100.0) == "1.000 2.000 C:maj\n2.000 2.500 N\n2.500 3.500 A:min\n3.500 4.000 G:7\n"
    assert Ch.chord_markers(seg, beats) == [(960, "C/E"), (1920, "N"), (2400, "Am"), (3360, "G7")] and T.lead_beats(beats) == 2
    summary = Ch.chord_summary(chord, None, beats, 100.0)
    assert summary == {"chords": [(1.0, 2.0, "C/E"), (2.0, 2.5, "N"), (2.5, 3.5, "Am"), (3.5, 4.0, "G7")], "chord_labels": [0, 0, 255, 21, 21, 67]}
    assert Ch.chord_segments(np.zeros(0, np.int32), beats) == [] and Ch.chord_lab([], beats) == "" and Ch.chord_markers([], beats[:1]) == []
    with pytest.raises(ValueError, match="7 chords for 6 beats"):
        Ch.chord_segments(np.zeros(7, np.int32), beats)


def _notes(rec):
    return [Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"]), 64 + i % 32) for i, r in enumerate(rec)
            if r["onset"] >= 0]


@pytest.mark.parametrize("name", ["jazz", "inversions", "pickup1_three4"])
def test_markers_round_trip_and_bytes_without_them_are_the_present_ones(name, tracked):
    rec, beats, n_frames, metre, truth = CC.music(name)
    key = int(B.track_bars(rec, beats, n_frames)[1][3])
    notes = _notes(rec)
    ticks = T.beat_positions(notes, beats)
    seg = Ch.chord_segments(tracked[name][0], beats)
    markers = Ch.chord_markers(seg, beats)
    assert len(markers) == tracked[name][1][0]                              # one per run of equal label
    on_beats, on_bars = M.notes_to_midi_bytes_on_beats(notes, ticks, beats, CC.FPS), M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, key, CC.FPS)
    with_b = M.notes_to_midi_bytes_on_beats(notes, ticks, beats, CC.FPS, markers)
    with_m = M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, key, CC.FPS, markers=markers)
    assert M.read_midi_markers(with_b) == M.read_midi_markers(with_m) == markers and M.read_midi_markers(on_bars) == []
    assert len(with_m) > len(on_bars) and b"\xff\x06" in with_m and b"\xff\x06" not in on_bars
    n0 = T.lead_beats(beats)
    assert all(tick == (n0 + s) * 480 for (tick, _), (s, _, _, _) in zip(markers, seg))
    # no markers: the bytes of the writers as they were
    assert M.notes_to_midi_bytes_on_beats(notes, ticks, beats, CC.FPS, ()) == M.notes_to_midi_bytes_on_beats(notes, ticks, beats, CC.FPS, []) == on_beats
    assert M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, key, CC.FPS, markers=()) == on_bars
    kept = [(n, (int(a), int(b))) for n, (a, b) in zip(notes, ticks) if a >= 0 and (b >= 0 or n.is_drum)]
    assert on_beats == M._smf_bytes([n for n, _ in kept], {id(n): t for n, t in kept}, T.tempo_map(beats, CC.FPS))
    # the older readers skip the markers: the same notes, tempo map and signatures
    assert M.read_midi_notes(with_m) == M.read_midi_notes(on_bars) and M.read_midi_on_bars(with_m) == M.read_midi_on_bars(on_bars)
    assert M.read_midi_on_beats(with_b) == M.read_midi_on_beats(on_beats)
    conductor = [(tick, payload[0]) for track, tick, st, payload in M._track_events(with_m)[1] if track == 0 and st == 0xFF and tick == markers[0][0]]
    assert 0x06 in [t for _, t in conductor] and (0x51 not in [t for _, t in conductor] or [t for _, t in conductor].index(0x06) < [t for _, t in conductor].index(0x51))
    # without downbeats the file on the bars falls back to the one on the beats, markers kept
    assert M.notes_to_midi_bytes_on_bars(notes, ticks, beats, np.zeros(0, np.int32), -1, CC.FPS, markers) == with_b
    with pytest.raises(ValueError, match="1 to 127 bytes"):
        M.notes_to_midi_bytes_on_beats(notes, ticks, beats, CC.FPS, [(0, "")])
    assert inspect.signature(M.notes_to_midi_bytes_on_beats).parameters["markers"].default == ()
    assert inspect.signature(M.notes_to_midi_bytes_on_bars).parameters["markers"].default == ()


def test_chords_are_off_by_default():
    from yourmt3_amd.task_manager import TaskManager
    from yourmt3_amd.transcribe import LiveTranscriber, estimate_chords, transcribe
    sig = inspect.signature(transcribe).parameters
    assert sig["chords"].default is False and sig["chord_params"].default is None
    assert inspect.signature(TaskManager.tokens_to_notes_device).parameters["chords"].default is None
    assert "chords" not in inspect.signature(LiveTranscriber.__init__).parameters and "estimate_chords()" in LiveTranscriber.__doc__
    assert estimate_chords is Ch.estimate_chords
    assert list(inspect.signature(estimate_chords).parameters)[:6] == ["model", "notes_or_mid_path", "end_sec", "divisions", "output_path", "lab_path"]
    with pytest.raises(ValueError, match="chords=True without beats=True"):
        transcribe(None, np.zeros(8, np.float32), chords=True)
    with pytest.raises(ValueError, match="chord_params without chords=True"):
        transcribe(None, np.zeros(8, np.float32), beats=True, chord_params={})
    with pytest.raises(ValueError, match="chords without beats"):
        TaskManager("mt3_full_plus").tokens_to_notes_device(None, None, [], 0.0, chords=object())


REFUSALS = [
    (dict(frames_per_second=0.0), "frames_per_second=0.0 must be finite and > 0"),
    (dict(frames_per_second=float("nan")), "frames_per_second=nan must be finite and > 0"),
    (dict(qualities=()), r"qualities=\(\) must hold 1 to 8 names"),
    (dict(qualities=Ch.QUALITIES + ("maj",)), r"must hold 1 to 8 names"),
    (dict(qualities=("maj", "min6")), r"qualities=\('maj', 'min6'\) must be distinct names of"),
    (dict(qualities=("maj", "min", "maj")), r"qualities=\('maj', 'min', 'maj'\) must be distinct names of"),
    (dict(qualities="maj"), r"qualities='maj' must be a tuple of names"),
    (dict(near_div=1), r"near_div=1 outside \[2, 64\]"),
    (dict(near_div=65), r"near_div=65 outside \[2, 64\]"),
    (dict(bass_div=0), r"bass_div=0 outside \[1, 64\]"),
    (dict(bass_div=65), r"bass_div=65 outside \[1, 64\]"),
    (dict(w_bass=1025), r"w_bass=1025 outside \[0, 1024\]"),
    (dict(w_none=-1), r"w_none=-1 outside \[0, 1024\]"),
    (dict(change_cost=4097), r"change_cost=4097 outside \[0, 4096\]"),
    (dict(change_cost_down=-1), r"change_cost_down=-1 outside \[0, 4096\]"),
    (dict(n_programs=257), r"n_programs=257 outside \[1, 256\]"),
    (dict(drum_program=130), r"drum_program=130 outside \[0, n_programs=130\)"),
]


@pytest.mark.parametrize("params,text", REFUSALS, ids=[next(iter(r[0])) + str(i) for i, r in enumerate(REFUSALS)])
def test_parameters_outside_the_limits_are_refused(params, text):
    with pytest.raises(ValueError, match=text):
        Ch.track_chords([], [], 100, **params)


def test_frames_sizes_and_unknown_parameters_are_refused():
    with pytest.raises(TypeError, match="unknown chord parameter"):
        Ch.track_chords([], [], 100, metres=(4,))
    with pytest.raises(ValueError, match=r"n_frames=0 outside \[1, 1048576\]"):
        Ch.track_chords([], [], 0)
    with pytest.raises(ValueError, match=r"n_frames=1048577 outside"):
        Ch.track_chords([], [], (1 << 20) + 1)
    with pytest.raises(ValueError, match="beats must ascend strictly"):
        Ch.track_chords([], [10, 10, 20], 100)
    with pytest.raises(ValueError, match="2 metre entries for 3 beats"):
        Ch.track_chords([], [10, 20, 30], 100, metre=[1024, 1025])
    with pytest.raises(ValueError, match=r"max_beats=0 outside \[1, 1048577\]"):
        Ch.check_sizes(0, 1)
    with pytest.raises(ValueError, match=r"max_notes=1048577 outside"):
        Ch.check_sizes(1, (1 << 20) + 1)
    Ch.check_sizes((1 << 20) + 1, 1 << 20)
    d = Ch.DEFAULTS
    assert (d["near_div"], d["bass_div"], d["w_bass"], d["w_none"], d["change_cost"], d["change_cost_down"]) == (4, 2, 64, 300, 160, 48)
    assert d["qualities"] == ("maj", "min", "dim", "aug", "sus4", "7", "maj7", "min7") and Ch.check_params(qualities=["min", "maj"])["qualities"] == ("min", "maj")
    assert Ch.WEIGHTS == (591, 591, 591, 591, 591, 512, 512, 512) and Ch.INTERVALS == CC.TONES
    # the weights are 1024 / sqrt(n), and an emission stays below 2^21
    assert [round(1024 / len(t) ** 0.5) for t in Ch.INTERVALS] == list(Ch.WEIGHTS) and 591 * 1024 + 1024 * 1024 < 1 << 21


def test_the_abi_declares_lists_and_exports_the_entry_points(tmp_path):
    import shutil
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    names = {"ymt3_chords_create", "ymt3_chords_destroy", "ymt3_track_chords"}
    assert names <= set(re.findall(r"\b(ymt3_[a-z_0-9]+)\s*\(", header)) and names <= set(_lib.SYMBOLS)
    assert "typedef struct ymt3_chords_s* ymt3_chords;" in header and "} ymt3_chord_params;" in header
    assert re.search(r"#define YMT3_ABI_VERSION 3\b", header)
    assert header.index("ymt3_track_bars(") < header.index("ymt3_chords_create(") < header.index("Measurement hook")      # after bars and key
    body = header[header.index("typedef struct ymt3_chord_params {"):header.index("} ymt3_chord_params;")]
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for line in body.splitlines()[1:] for f in re.sub(r"^\s*(double|int32_t)\s+", "", line).rstrip(";").split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.ChordParams._fields_] and ctypes.sizeof(_lib.ChordParams) == 80
    assert _lib.ChordParams.qualities.size == 32 and "qualities[8]" in body
    gcc = shutil.which("gcc")
    if gcc is not None:
        src = tmp_path / "abi.c"
        src.write_text('#include "ymt3.h"\ntypedef char size_is_80[sizeof(ymt3_chord_params) == 80 ? 1 : -1];\n'
                       'int main(void) { int (*f)(ymt3_handle, const ymt3_chord_params*, long long, long long, ymt3_chords*) = ymt3_chords_create;\n'
                       'int (*g)(ymt3_handle, ymt3_chords, const int32_t*, const long long*, const int32_t*, const void*, long long, const int32_t*,\n'
                       'long long, int32_t*, long long, long long*, void*) = ymt3_track_chords; void (*d)(ymt3_chords) = ymt3_chords_destroy;\n'
                       '(void)f; (void)g; (void)d; return 0; }\n')
        r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.ymt3_abi_version() == 3
    import yourmt3_amd
    for n in ("track_chords", "ChordTracker", "estimate_chords"):
        assert n in yourmt3_amd.__all__ and getattr(yourmt3_amd, n) is getattr(Ch, n)
    hip = open(os.path.join(ROOT, "yourmt3_amd", "csrc", "chords.hip")).read()
    for q, tones in enumerate(Ch.INTERVALS):                               # the kernel's templates are the specification's
        args = ", ".join(str(v) for v in (tones[1:] + (-1,))[:3]) + f", {Ch.WEIGHTS[q]}"
        assert f"chord_base(a, {q})) >= 0) chord_emit<{args}>" in hip, (q, args)
    from yourmt3_amd import build
    assert "chords.hip" in build.SOURCES


def test_the_object_shares_the_lifecycle_and_stays_out_of_the_models_namespace():
    from yourmt3_amd import model as Mo
    assert issubclass(Ch.ChordTracker, Mo._Owned) and (Ch.ChordTracker._destroy, Ch.ChordTracker._noun) == ("ymt3_chords_destroy", "chord tracker")
    assert "ChordTracker" not in vars(Mo) and "from .chords import ChordTracker" in inspect.getsource(Mo.YourMT3.compile_chord_tracker)
    obj = Ch.ChordTracker.__new__(Ch.ChordTracker)
    obj.close()                                      # before _own: nothing to free


def test_the_package_does_not_import_the_oracle():
    code = "import sys, yourmt3_amd, yourmt3_amd.chords, yourmt3_amd.transcribe; assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
