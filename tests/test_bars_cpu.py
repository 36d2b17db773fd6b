"""Bars and key without a GPU: the host specification (yourmt3_amd/bars.py) against the loop model (tests/bar_model.py) on every case, what
the rules find on music whose bars and keys are known, the MIDI file on the bars, the parameter refusals and the ABI surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import bar_cases as BC
from bar_model import track_bars as model_track
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T
from yourmt3_amd import midi as M
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = BC.all_cases()

# Downbeat F-measure (one-to-one within 70 ms) of the specification against the generating downbeats, as computed by
# test_known_music_is_barred_as_recorded when these rules were written; the test asserts the recorded value minus 0.05.
RECORDED_F = {name: 1.0 for name in BC.KNOWN}


@pytest.fixture(scope="module")
def tracked():
    """the specification's result of every case, computed once"""
    return {name: B.track_bars(BC.live(rec, count), beats, n_frames, **params) for name, rec, beats, n_frames, params, count in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_specification_equals_the_loop_model(case, tracked):
    name, rec, beats, n_frames, params, count = case
    metre, result = tracked[name]
    m_metre, m_result, ties = model_track(BC.live(rec, count), beats, n_frames, B.check_params(**params))
    assert metre.dtype == np.int32 and result.dtype == np.int64 and result.shape == (8,)
    assert metre.shape == ((len(beats),) if len(beats) >= 2 else (0,))
    assert metre.tolist() == m_metre and result.tolist() == m_result
    if name in BC.TIE_CASES:
        print(f"{name}: {ties} ties")
        assert ties > 0


def test_the_edge_cases_are_what_they_say(tracked):
    for k in (0, 1):
        assert tracked[f"beats{k}"][0].size == 0 and tracked[f"beats{k}"][1].tolist() == [0, 0, 0, -1, 0, 0, 0, 0]
    assert tracked["beats2"][0].size == 2 and tracked["beats3"][0].size == 3
    assert set((tracked["metres_3_only"][0] >> 8).tolist()) == {3}
    for name in ("metronome", "metronome_flat"):                          # metres[0] from beat 0
        assert tracked[name][0].tolist() == [1024 + i % 4 for i in range(25)]
    assert tracked["metronome_flat"][1][1:3].tolist() == [0, 0]
    assert tracked["drums_only"][1][3] == -1 and tracked["drums_only"][1][0] > 0
    assert tracked["count_zero"][1].tolist() == [tracked["count_zero"][1][0], 0, 0, -1, 0, 0, 0, 0]
    assert tracked["nonfinite_and_out_of_range"][1][6] == 5               # a NaN onset, two programs, a pitch, a pitched note's NaN offset
    # 300 onsets on one beat count as accent_cap: the salience of that beat is the cap's
    p = B.check_params()
    name, rec, beats, n_frames, _, _ = next(c for c in CASES if c[0] == "cap_300_on_one_beat")
    a, c, _ = B.bar_features(rec, beats, n_frames, p)
    assert a.max() == 301 and int(B.salience(a, c, p).max()) <= 64 * 15 + 2048
    assert tracked["one_note_key_tie"][1][3:6].tolist() == [6, 671 * 50, 671 * 50]      # F# major before F# minor


def test_known_music_is_barred_as_recorded(tracked):
    for name, (kw, clean) in BC.KNOWN.items():
        rec, beats, n_frames, downs, runs, pickup = BC.known(name)
        metre, result = tracked[name]
        est = [int(b) / BC.FPS for b, v in zip(beats, metre.tolist()) if v & 255 == 0]
        f = BC.f_measure(est, downs)
        print(f"{name}: {beats.size} beats, runs {B.metre_runs(metre)}, downbeat F {f:.3f}, key {B.key_name(result[3])}")
        if clean:
            assert B.metre_runs(metre) == runs
        assert f >= RECORDED_F[name] - 0.05
        assert result[0] == len(est) and B.bar_list(metre)[-1][0] + B.bar_list(metre)[-1][1] == beats.size
        if pickup:
            m = runs[0][0]
            assert metre[0] == 256 * m + (m - pickup) and B.bar_list(metre)[0] == (0, pickup, m)


@pytest.mark.parametrize("key", range(24))
def test_all_24_keys_and_their_signatures(key):
    rec = BC.melody(key)
    metre, result = B.track_bars(rec, BC.steady(16), 900)
    assert result[3] == key and result[4] > result[5]
    mode, tonic = divmod(key, 12)
    major = (tonic + 3) % 12 if mode else tonic
    sharps = {0: 0, 7: 1, 2: 2, 9: 3, 4: 4, 11: 5, 6: 6, 5: -1, 10: -2, 3: -3, 8: -4, 1: -5}[major]      # the circle of fifths, written out
    assert B.key_signature(key) == (sharps, mode)
    assert B.key_name(key).endswith(" minor" if mode else " major")


def test_key_names_ties_and_none():
    assert B.key_name(18) == "F# minor" and B.key_name(0) == "C major" and B.key_name(10) == "Bb major" and B.key_name(-1) == "none"
    assert B.key_of([0] * 12) == (-1, 0, 0)
    one = [0] * 12
    one[9] = 7                                                             # one pitch class: its major and its minor tie, major first
    assert B.key_of(one) == (9, 7 * 671, 7 * 671)
    both = [5 if pc in (0, 6) else 0 for pc in range(12)]                  # a tritone: C and F# tie in both modes; the smaller tonic of the major
    key, best, second = B.key_of(both)
    assert key == 0 and best == second
    with pytest.raises(ValueError):
        B.key_signature(-1)
    assert sum(B.KEY_MAJOR) in range(-6, 7) and sum(B.KEY_MINOR) in range(-6, 7)                 # centred, up to rounding
    assert abs(sum(v * v for v in B.KEY_MAJOR) - 1024 ** 2) < 4096 and abs(sum(v * v for v in B.KEY_MINOR) - 1024 ** 2) < 4096


def _notes(rec):
    return [Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"]), 64 + i % 32) for i, r in enumerate(rec)
            if r["onset"] >= 0]


@pytest.mark.parametrize("name", ["four_three_four", "pickup1_three4", "one_two4_bar", "two4"])
def test_the_midi_file_on_the_bars(name, tracked):
    rec, beats, n_frames, downs, runs, pickup = BC.known(name)
    metre, result = tracked[name]
    notes = _notes(rec)
    ticks = T.beat_positions(notes, beats)
    data = M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, int(result[3]), BC.FPS)
    plain = M.notes_to_midi_bytes_on_beats(notes, ticks, beats, BC.FPS)
    back, tempos, signatures, key = M.read_midi_on_bars(data)
    assert signatures == B.time_signatures(metre, beats) and key == B.key_signature(int(result[3])) and tempos == T.tempo_map(beats, BC.FPS)
    n0 = T.lead_beats(beats)
    down_ticks = sorted((n0 + i) * 480 for i, v in enumerate(metre.tolist()) if v & 255 == 0)
    m0 = int(metre[(down_ticks[0] // 480) - n0]) >> 8
    for tick, nn in signatures:                                            # on a downbeat's tick; before the first one: tick 0, or a bar line of m0
        assert tick in down_ticks or tick == 0 or (tick < down_ticks[0] and (down_ticks[0] - tick) % (480 * m0) == 0 and nn == m0)
    assert [nn for _, nn in signatures][-len(runs):] == [m for m, _ in runs]
    # the older readers still parse the file to the same notes
    assert M.read_midi_on_beats(data) == (back, tempos) == M.read_midi_on_beats(plain) and M.read_midi_notes(data) == M.read_midi_notes(plain)
    assert data != plain
    assert b"\xff\x58\x04" + bytes([signatures[0][1], 2, 24, 8]) in data and b"\xff\x59\x02" in data
    # bars off, or no downbeats: the bytes of the file on the beats
    assert M.notes_to_midi_bytes_on_bars(notes, ticks, beats, np.zeros(0, np.int32), -1, BC.FPS) == plain
    assert M.notes_to_midi_bytes_on_bars(notes, ticks, beats, np.full(beats.size, 1025, np.int32), 3, BC.FPS) == plain
    no_key = M.notes_to_midi_bytes_on_bars(notes, ticks, beats, metre, -1, BC.FPS)
    assert M.read_midi_on_bars(no_key)[2:] == (signatures, None) and len(no_key) == len(data) - 6


def test_time_signatures_open_with_a_short_bar_for_a_late_start():
    beats = BC.steady(12, first=130, step=50)                              # n0 = ceil(130 / 50) = 3
    assert T.lead_beats(beats) == 3
    four = np.array([1024 + (i + 2) % 4 for i in range(12)], np.int32)     # the first downbeat is beat 2: (3 + 2) mod 4 = 1
    assert B.time_signatures(four, beats) == [(0, 1), (480, 4)]
    three = np.array([768 + i % 3 for i in range(12)], np.int32)           # the first downbeat is beat 0: (3 + 0) mod 3 = 0
    assert B.time_signatures(three, beats) == [(0, 3)]
    mixed = np.array([1024, 1025, 1026, 1027, 768, 769, 770, 768, 769, 770, 512, 513], np.int32)
    assert B.time_signatures(mixed, beats) == [(0, 3), (1440, 4), ((3 + 4) * 480, 3), ((3 + 10) * 480, 2)]
    assert B.bar_list(mixed) == [(0, 4, 4), (4, 3, 3), (7, 3, 3), (10, 2, 2)] and B.metre_runs(mixed) == [(4, 1), (3, 2), (2, 1)]
    assert B.time_signatures(np.zeros(0, np.int32), beats[:1]) == [] and B.time_signatures(np.array([1025, 1026], np.int32), beats[:2]) == []
    notes = [Note(1.3 + 0.5 * i, 1.5 + 0.5 * i, False, 0, 60 + i) for i in range(12)]
    data = M.notes_to_midi_bytes_on_bars(notes, T.beat_positions(notes, beats), beats, four, 7, 100.0)
    assert M.read_midi_on_bars(data)[2:] == ([(0, 1), (480, 4)], (1, 0))
    conductor = [(tick, payload[0]) for track, tick, st, payload in M._track_events(data)[1] if track == 0 and st == 0xFF and payload[0] != 0x2F]
    assert conductor == [(0, 0x58), (0, 0x59), (0, 0x51), (480, 0x58)]


def test_existing_writers_keep_their_bytes():
    notes = [Note(0.5, 1.0, False, 0, 60), Note(1.0, 1.2, True, 128, 36)]
    ticks = {id(n): (M._ticks(n.onset), M._ticks(n.offset)) for n in notes}
    assert M._smf_bytes(notes, ticks, [(0, M.TEMPO_US)]) == M._smf_bytes(notes, ticks, [(0, M.TEMPO_US)], ()) == M.notes_to_midi_bytes(notes)
    assert inspect.signature(M._smf_bytes).parameters["conductor_events"].default == ()


def test_bars_are_off_by_default():
    from yourmt3_amd.task_manager import TaskManager
    from yourmt3_amd.transcribe import LiveTranscriber, estimate_bars, transcribe
    sig = inspect.signature(transcribe).parameters
    assert sig["bars"].default is False and sig["bar_params"].default is None
    assert inspect.signature(TaskManager.tokens_to_notes_device).parameters["bars"].default is None
    assert "bars" not in inspect.signature(LiveTranscriber.__init__).parameters and "Bars and key" in LiveTranscriber.__doc__
    assert estimate_bars is B.estimate_bars
    assert list(inspect.signature(estimate_bars).parameters)[:6] == ["model", "notes_or_mid_path", "end_sec", "divisions", "output_path", "beat_params"]
    with pytest.raises(ValueError, match="bars=True without beats=True"):
        transcribe(None, np.zeros(8, np.float32), bars=True)
    with pytest.raises(ValueError, match="bar_params without bars=True"):
        transcribe(None, np.zeros(8, np.float32), beats=True, bar_params={})
    with pytest.raises(ValueError, match="bars without beats"):
        TaskManager("mt3_full_plus").tokens_to_notes_device(None, None, [], 0.0, bars=object())


REFUSALS = [
    (dict(frames_per_second=0.0), "frames_per_second=0.0 must be finite and > 0"),
    (dict(frames_per_second=float("inf")), "frames_per_second=inf must be finite and > 0"),
    (dict(metres=()), r"metres=\(\) must hold 1 to 5 metres"),
    (dict(metres=(2, 3, 4, 5, 6, 2)), r"metres=\(2, 3, 4, 5, 6, 2\) must hold 1 to 5 metres"),
    (dict(metres=(4, 7)), r"metres=\(4, 7\) must be distinct integers in \[2, 6\]"),
    (dict(metres=(1, 4)), r"metres=\(1, 4\) must be distinct integers in \[2, 6\]"),
    (dict(metres=(4, 3, 4)), r"metres=\(4, 3, 4\) must be distinct integers in \[2, 6\]"),
    (dict(metres=4), r"metres=4 must be a tuple of integers"),
    (dict(near_div=1), r"near_div=1 outside \[2, 64\]"),
    (dict(near_div=65), r"near_div=65 outside \[2, 64\]"),
    (dict(accent_cap=0), r"accent_cap=0 outside \[1, 255\]"),
    (dict(accent_cap=256), r"accent_cap=256 outside \[1, 255\]"),
    (dict(w_long=16), r"w_long=16 outside \[0, 15\]"),
    (dict(w_kick=-1), r"w_kick=-1 outside \[0, 15\]"),
    (dict(w_accent=1025), r"w_accent=1025 outside \[0, 1024\]"),
    (dict(switch_cost=4097), r"switch_cost=4097 outside \[0, 4096\]"),
    (dict(kick_lo=37), r"kick_lo=37, kick_hi=36 must satisfy 0 <= kick_lo <= kick_hi <= 127"),
    (dict(kick_hi=128), r"kick_lo=35, kick_hi=128 must satisfy"),
    (dict(n_programs=257), r"n_programs=257 outside \[1, 256\]"),
    (dict(drum_program=130), r"drum_program=130 outside \[0, n_programs=130\)"),
]


@pytest.mark.parametrize("params,text", REFUSALS, ids=[next(iter(r[0])) + str(i) for i, r in enumerate(REFUSALS)])
def test_parameters_outside_the_limits_are_refused(params, text):
    with pytest.raises(ValueError, match=text):
        B.track_bars([], [], 100, **params)


def test_frames_sizes_and_unknown_parameters_are_refused():
    with pytest.raises(TypeError, match="unknown bar parameter"):
        B.track_bars([], [], 100, tempo=3)
    with pytest.raises(ValueError, match=r"n_frames=0 outside \[1, 1048576\]"):
        B.track_bars([], [], 0)
    with pytest.raises(ValueError, match=r"n_frames=1048577 outside"):
        B.track_bars([], [], (1 << 20) + 1)
    with pytest.raises(ValueError, match="beats must ascend strictly"):
        B.track_bars([], [10, 10, 20], 100)
    for kw, text in [(dict(max_beats=0, max_notes=1), r"max_beats=0 outside \[1, 1048577\]"), (dict(max_beats=(1 << 20) + 2, max_notes=1), "max_beats=1048578 outside"),
                     (dict(max_beats=1, max_notes=0), r"max_notes=0 outside \[1, 1048576\]"), (dict(max_beats=1, max_notes=(1 << 20) + 1), "max_notes=1048577 outside")]:
        with pytest.raises(ValueError, match=text):
            B.check_sizes(**kw)
    B.check_sizes((1 << 20) + 1, 1 << 20)
    assert B.check_params(metres=[3, 4])["metres"] == (3, 4) and B.DEFAULTS["metres"] == (4, 3, 2) and B.DEFAULTS["switch_cost"] == 4


def test_the_abi_declares_lists_and_exports_the_entry_points(tmp_path):
    import shutil
    import subprocess
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    names = {"ymt3_bars_create", "ymt3_bars_destroy", "ymt3_track_bars"}
    assert names <= set(re.findall(r"\b(ymt3_[a-z_0-9]+)\s*\(", header)) and names <= set(_lib.SYMBOLS)
    assert "typedef struct ymt3_bars_s* ymt3_bars;" in header and "} ymt3_bar_params;" in header
    assert re.search(r"#define YMT3_ABI_VERSION 3\b", header)
    body = header[header.index("typedef struct ymt3_bar_params {"):header.index("} ymt3_bar_params;")]
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for line in body.splitlines()[1:] for f in re.sub(r"^\s*(double|int32_t)\s+", "", line).rstrip(";").split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.BarParams._fields_] and ctypes.sizeof(_lib.BarParams) == 72
    assert _lib.BarParams.metres.size == 20 and "metres[5]" in body
    gcc = shutil.which("gcc")
    if gcc is not None:
        src = tmp_path / "abi.c"
        src.write_text('#include "ymt3.h"\ntypedef char size_is_72[sizeof(ymt3_bar_params) == 72 ? 1 : -1];\n'
                       'int main(void) { int (*f)(ymt3_handle, const ymt3_bar_params*, long long, long long, ymt3_bars*) = ymt3_bars_create;\n'
                       'int (*g)(ymt3_handle, ymt3_bars, const int32_t*, const long long*, const void*, long long, const int32_t*, long long, int32_t*,\n'
                       'long long, long long*, void*) = ymt3_track_bars; (void)f; (void)g; return 0; }\n')
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
    for n in ("track_bars", "BarTracker", "estimate_bars"):
        assert n in yourmt3_amd.__all__ and getattr(yourmt3_amd, n) is getattr(B, n)
    hip = open(os.path.join(ROOT, "yourmt3_amd", "csrc", "bars.hip")).read()
    for table in (B.KEY_MAJOR, B.KEY_MINOR):                               # the kernel's tables are the specification's
        assert "{" + ", ".join(str(v) for v in table) + "}" in hip
    from yourmt3_amd import build
    assert "bars.hip" in build.SOURCES


def test_the_object_shares_the_lifecycle_and_stays_out_of_the_models_namespace():
    from yourmt3_amd import model as Mo
    assert issubclass(B.BarTracker, Mo._Owned) and (B.BarTracker._destroy, B.BarTracker._noun) == ("ymt3_bars_destroy", "bar tracker")
    assert "BarTracker" not in vars(Mo) and "from .bars import BarTracker" in inspect.getsource(Mo.YourMT3.compile_bar_tracker)
    obj = B.BarTracker.__new__(B.BarTracker)
    obj.close()                                      # before _own: nothing to free
