"""Beat tracking without a GPU: the host specification (yourmt3_amd/beats.py) against the loop model (tests/beat_model.py) on every case,
what the rules find on music whose beats are known, the positions, the MIDI file on the beats, the parameter refusals and the ABI surface."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import beat_cases as BC
from beat_model import model_ticks, model_track
from yourmt3_amd import beats as B
from yourmt3_amd import midi as M
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = BC.all_cases()

# Beat F-measure (one-to-one within 70 ms) of the specification against the generating beats, as computed by
# test_known_music_is_tracked_as_recorded when these rules were written; the test asserts the recorded value minus 0.05.
RECORDED_F = {"tempo_step": 0.938, "accelerando": 1.0, "music_like": 1.0}


@pytest.fixture(scope="module")
def tracked():
    """the specification's result of every case, computed once"""
    return {name: B.track_beats(BC.live(rec, count), n_frames, **params) for name, rec, n_frames, params, count in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_specification_equals_the_loop_model(case, tracked):
    name, rec, n_frames, params, count = case
    rec = BC.live(rec, count)
    p = B.check_params(**params)
    beats, tempo, result = tracked[name]
    m_beats, m_tempo, m_result, _ = model_track(rec, n_frames, p)
    assert beats.dtype == np.int32 and tempo.dtype == np.int32 and result.dtype == np.int64
    assert beats.tolist() == m_beats and tempo.tolist() == m_tempo and result.tolist() == m_result
    assert len(m_beats) <= B.max_beats(n_frames, p["lag_min"]) and tempo.size == B.n_windows(n_frames, p["hop_frames"])
    for q in (0, 4, 480):
        ticks = B.beat_positions(rec, beats, p["frames_per_second"], q, p["n_programs"], p["drum_program"])
        assert ticks.dtype == np.int32 and ticks.tolist() == model_ticks(rec, m_beats, p, q), q


def test_the_tie_cases_have_ties():
    by_name = {c[0]: c for c in CASES}
    _, rec, n_frames, params, _ = by_name["equal_predecessors"]
    assert model_track(rec, n_frames, B.check_params(**params))[3][0] > 0
    _, rec, n_frames, params, _ = by_name["silence_10s"]
    assert model_track(rec, n_frames, B.check_params(**params))[3][1] > 0


@pytest.mark.parametrize("bpm,lag", list(zip(BC.METRONOME_BPM, (100, 75, 60, 50, 40))))
def test_a_metronome_is_tracked_click_by_click(bpm, lag, tracked):
    beats, tempo, result = tracked[f"metronome{bpm}"]
    click_frames = BC.metronome(bpm)[2]
    assert set(tempo.tolist()) == {lag}
    assert set(beats.tolist()) <= set(click_frames.tolist())                                  # every beat lies on a click
    inside = click_frames[(click_frames >= beats[0]) & (click_frames <= beats[-1])]
    assert beats.tolist() == inside.tolist() and beats.size >= click_frames.size - 2           # and every click between them is a beat
    assert result[0] == beats.size and result[3] == 0


def test_200_bpm_is_tracked_at_half_tempo(tracked):
    """the documented octave choice: the prior (120 bpm, one octave) prefers 100 bpm to 200"""
    beats, tempo, _ = tracked["metronome200"]
    assert set(tempo.tolist()) == {60}
    assert set(np.diff(beats).tolist()) == {60} and set(beats.tolist()) <= set(BC.metronome(200)[2].tolist())


@pytest.mark.parametrize("name,make", [("tempo_step", BC.tempo_step), ("accelerando", BC.accelerando), ("music_like", BC.music_like)])
def test_known_music_is_tracked_as_recorded(name, make, tracked):
    f = BC.beat_f_measure(tracked[name][0] / BC.FPS, make()[2])
    print(f"{name}: beat F-measure {f:.3f} (recorded {RECORDED_F[name]})")
    assert f >= RECORDED_F[name] - 0.05


def test_positions_are_monotone_and_beats_land_on_whole_beats(tracked):
    beats = tracked["accelerando"][0]
    t = np.sort(np.random.default_rng(3).uniform(-1.0, 32.0, 500))
    rec = BC.records(t, length=0.0)
    ticks = B.beat_positions(rec, beats)
    assert (np.diff(ticks[:, 0]) >= 0).all() and (ticks[:, 1] >= ticks[:, 0] + 1).all()
    on_beats = B.beat_positions(BC.records(beats / BC.FPS), beats)[:, 0]
    n0 = B.lead_beats(beats)
    assert on_beats.tolist() == [(n0 + i) * 480 for i in range(beats.size)]
    assert B.beat_positions(BC.records([0.0]), beats)[0, 0] >= 0 and B.lead_sec(beats) * BC.FPS < beats[1] - beats[0]
    snapped = B.beat_positions(rec, beats, divisions=4)
    assert (snapped % 120 == 0).all() and (snapped[:, 1] >= snapped[:, 0] + 120).all()
    assert (np.abs(snapped[:, 0] - ticks[:, 0]) <= 60).all()
    flat = B.beat_positions(rec, beats[:1])
    assert flat[:, 0].tolist() == [max(0, int(np.rint(v * 960.0))) for v in t]
    with pytest.raises(ValueError, match="divisions=7 must be 0 or a divisor of 480"):
        B.beat_positions(rec, beats, divisions=7)


def test_the_midi_file_on_the_beats_keeps_the_performance(tracked):
    for name, make in (("accelerando", BC.accelerando), ("music_like", BC.music_like), ("tempo_step", BC.tempo_step)):
        rec = make()[0]
        beats = tracked[name][0]
        notes = [Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"]), 64 + i % 32) for i, r in enumerate(rec)
                 if r["onset"] >= 0]
        ticks = B.beat_positions(notes, beats)
        data = M.notes_to_midi_bytes_on_beats(notes, ticks, beats, BC.FPS)
        back, tempos = M.read_midi_on_beats(data)
        assert tempos == B.tempo_map(beats, BC.FPS) and tempos[0][0] == 0
        assert all(a[1] != b[1] and a[0] < b[0] for a, b in zip(tempos, tempos[1:]))
        lead = B.lead_sec(beats, BC.FPS)
        assert 0.0 <= lead < (beats[1] - beats[0]) / BC.FPS
        bound = float(np.diff(beats).max()) / BC.FPS / 960 + 0.5e-6 * beats.size        # half a tick, plus the tempo events' rounding
        # the writer gives each (channel, pitch) one voice: compare onsets, which it never moves
        want = sorted((n.pitch, n.is_drum, n.onset + lead) for n in notes)
        got = sorted((n.pitch, n.is_drum, n.onset) for n in back)
        assert len(got) == len(want)
        worst = max(abs(g[2] - w[2]) for g, w in zip(got, want))
        print(f"{name}: worst onset error {worst * 1e6:.1f} us, bound {bound * 1e6:.1f} us")
        assert all(g[:2] == w[:2] for g, w in zip(got, want)) and worst <= bound
        assert {n.velocity for n in back} == {n.velocity for n in notes}


def test_without_two_beats_the_file_is_the_flat_one():
    notes = [Note(0.5, 1.0, False, 0, 60), Note(1.0, 1.2, True, 128, 36)]
    flat = M.notes_to_midi_bytes(notes)
    for beats in ([], [50]):
        assert M.notes_to_midi_bytes_on_beats(notes, B.beat_positions(notes, beats), beats, 100.0) == flat
        assert B.tempo_map(beats) == [] and B.lead_sec(beats) == 0.0
    back, tempos = M.read_midi_on_beats(flat)
    assert tempos == [(0, 500000)] and back == M.read_midi_notes(flat)


def test_beats_are_off_by_default():
    from yourmt3_amd.task_manager import TaskManager
    from yourmt3_amd.transcribe import LiveTranscriber, transcribe
    sig = inspect.signature(transcribe).parameters
    assert sig["beats"].default is False and sig["quantize"].default == 0
    assert inspect.signature(TaskManager.tokens_to_notes_device).parameters["beats"].default is None
    assert "beats" not in inspect.signature(LiveTranscriber.__init__).parameters and "Beats" in LiveTranscriber.__doc__
    assert M.TEMPO_US == 500000 and M.TICKS_PER_BEAT == B.TICKS_PER_BEAT == 480


REFUSALS = [
    (dict(frames_per_second=0.0), "frames_per_second=0.0 must be finite and > 0"),
    (dict(bpm_prior=float("nan")), "bpm_prior=nan must be finite and > 0"),
    (dict(bpm_min=250.0), r"bpm_min=250.0 above bpm_max=240.0"),
    (dict(tightness=1e5), "tightness=100000.0 above 10000"),
    (dict(bpm_max=2400.0), r"lag_min=3, lag_max=150 .* must satisfy 4 <= lag_min <= lag_max <= 512"),
    (dict(bpm_min=10.0), r"lag_min=25, lag_max=600 .* must satisfy"),
    (dict(window_frames=299), r"window_frames=299 outside \[2 \* lag_max=300, 2048\]"),
    (dict(window_frames=2049), r"window_frames=2049 outside"),
    (dict(hop_frames=0), r"hop_frames=0 outside \[1, window_frames=800\]"),
    (dict(hop_frames=801), r"hop_frames=801 outside"),
    (dict(lag_step_max=-1), r"lag_step_max=-1 outside \[0, 512\]"),
    (dict(onset_cap=256), r"onset_cap=256 outside \[1, 255\]"),
    (dict(n_programs=257), r"n_programs=257 outside \[1, 256\]"),
    (dict(drum_program=130), r"drum_program=130 outside \[0, n_programs=130\)"),
]


@pytest.mark.parametrize("params,text", REFUSALS, ids=[next(iter(r[0])) + str(i) for i, r in enumerate(REFUSALS)])
def test_parameters_outside_the_limits_are_refused(params, text):
    with pytest.raises(ValueError, match=text):
        B.track_beats([], 100, **params)


def test_frames_and_unknown_parameters_are_refused():
    with pytest.raises(TypeError, match="unknown beat parameter"):
        B.track_beats([], 100, tempo=3)
    with pytest.raises(ValueError, match=r"n_frames=0 outside \[1, 1048576\]"):
        B.track_beats([], 0)
    with pytest.raises(ValueError, match=r"n_frames=1048577 outside"):
        B.track_beats([], (1 << 20) + 1)
    with pytest.raises(ValueError, match=r"n_frames=1048576 with hop_frames=1: the tempo path's sums could pass 2\^62"):
        B.track_beats([], 1 << 20, hop_frames=1, onset_cap=255, window_frames=2048)
    assert B.max_beats(1250, 25) == 1250 // 13 + 1 and B.n_windows(1, 100) == 1 and B.n_windows(101, 100) == 2


def test_the_tables_are_integers_of_the_stated_form():
    p = B.check_params()
    prior, pen = B.beat_tables(p)
    assert (p["lag_min"], p["lag_max"]) == (25, 150) and prior.shape == (126,) and pen.shape == (126, 301)
    assert prior[50 - 25] == 65535 and prior[25 - 25] == prior[100 - 25] == int(np.rint(65535 * math.exp(-0.5)))
    assert pen[50 - 25, 50] == 0 and pen[50 - 25, 100] == int(np.rint(100 * 1024 * math.log(2) ** 2)) and pen[50 - 25, 24] == 0 and pen[50 - 25, 25] > 0


def test_the_abi_declares_lists_and_exports_the_entry_points(tmp_path):
    import shutil
    import subprocess
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    names = {"ymt3_beats_create", "ymt3_beats_destroy", "ymt3_track_beats", "ymt3_beat_positions"}
    assert names <= set(re.findall(r"\b(ymt3_[a-z_0-9]+)\s*\(", header)) and names <= set(_lib.SYMBOLS)
    assert "typedef struct ymt3_beats_s* ymt3_beats;" in header and "} ymt3_beat_params;" in header
    assert re.search(r"#define YMT3_ABI_VERSION 3\b", header)
    body = header[header.index("typedef struct ymt3_beat_params {"):header.index("} ymt3_beat_params;")]
    fields = [f.strip() for line in body.splitlines()[1:] for f in re.sub(r"^\s*(double|int32_t)\s+", "", line).rstrip(";").split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.BeatParams._fields_] and ctypes.sizeof(_lib.BeatParams) == 72
    gcc = shutil.which("gcc")
    if gcc is not None:
        src = tmp_path / "abi.c"
        src.write_text('#include "ymt3.h"\ntypedef char size_is_72[sizeof(ymt3_beat_params) == 72 ? 1 : -1];\n'
                       'int main(void) { int (*f)(ymt3_handle, const ymt3_beat_params*, long long, ymt3_beats*) = ymt3_beats_create;\n'
                       '(void)f; return 0; }\n')
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
    for n in ("track_beats", "beat_positions", "BeatTracker", "estimate_beats"):
        assert n in yourmt3_amd.__all__ and getattr(yourmt3_amd, n) is getattr(B, n)


def test_the_object_shares_the_lifecycle_and_stays_out_of_the_models_namespace():
    from yourmt3_amd import model as Mo
    assert issubclass(B.BeatTracker, Mo._Owned) and (B.BeatTracker._destroy, B.BeatTracker._noun) == ("ymt3_beats_destroy", "beat tracker")
    assert "BeatTracker" not in vars(Mo) and "from .beats import BeatTracker" in inspect.getsource(Mo.YourMT3.compile_beat_tracker)
    obj = B.BeatTracker.__new__(B.BeatTracker)
    obj.close()                                      # before _own: nothing to free
