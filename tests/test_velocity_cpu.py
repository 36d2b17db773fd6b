"""The note velocities without a GPU: the host specification itself (yourmt3_amd/velocity.py), the conditions tests/velocity_cases.py
must meet for the device test to be sharp (the measured f32 error that sets its tolerance; few records with more than one admissible
velocity), and the feature's plumbing: header, symbol list, exports, object lifecycle, signature defaults."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import velocity_cases as C
from yourmt3_amd import velocity as V
from yourmt3_amd.midi import notes_to_midi_bytes, read_midi_notes
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = C.SR
CASES = C.cases()
IDS = [c["id"] for c in CASES]


def _case(name):
    return next(c for c in CASES if c["id"] == name)


def _sine(amp, pitch, n=8000, phase=0.3):
    return (amp * np.sin(2 * np.pi * V.pitch_hz(pitch) * np.arange(n) / SR + phase)).astype(np.float32)


# ---------------------------------------------------------------- the rules
@pytest.mark.parametrize("pitch,amp", [(45, 0.5), (69, 0.25), (69, 1e-3), (96, 0.7)])
def test_a_steady_sinusoid_of_amplitude_a_has_energy_a_squared(pitch, amp):
    vel, E, peaks, counts = V.note_velocities(_sine(amp, pitch), SR, C.records([C.rec(0.1, pitch)]))
    print(f"pitch {pitch} amplitude {amp}: E = {E[0]:.6g}, A^2 = {amp * amp:.6g}")
    assert abs(E[0] - amp * amp) <= 0.01 * amp * amp
    assert vel.tolist() == [120] and peaks.tolist() == [E[0], 0.0] and counts.tolist() == [1, 0]
    assert vel.dtype == np.uint8 and E.dtype == np.float64


def test_doubling_the_amplitude_raises_the_velocity_by_the_slope():
    x = np.concatenate([_sine(0.1, 60, 4000), _sine(0.2, 60, 4000), _sine(0.4, 60, 4000)])
    notes = C.records([C.rec(0.05, 60), C.rec(0.30, 60), C.rec(0.55, 60)])
    for slope in (2.0, 3.0):
        vel = V.note_velocities(x, SR, notes, velocity_per_db=slope)[0].astype(int)
        step = int(np.rint(slope * 6.02))
        assert vel[2] == 120 and vel[2] - vel[1] == step and vel[1] - vel[0] == step, vel


def test_the_loudest_note_gets_peak_velocity_and_both_ends_clamp():
    x = np.concatenate([_sine(0.5, 60, 4000), _sine(0.5e-3, 60, 4000), _sine(1.0, 60, 4000)])
    notes = C.records([C.rec(0.05, 60), C.rec(0.30, 60), C.rec(0.55, 60)])
    assert V.note_velocities(x, SR, notes, peak_velocity=90)[0].tolist() == [78, 1, 90]                 # -6 dB: 12 down; -66 dB: the floor
    assert V.note_velocities(x, SR, notes, peak_velocity=90, min_velocity=30)[0].tolist() == [78, 30, 90]
    # an absolute reference 20 dB under the loudest note: 40 above peak_velocity, clamped at 127; the quiet one 46 dB under it
    assert V.note_velocities(x, SR, notes, peak_db=-20.0)[0].tolist() == [127, 28, 127]
    assert V.note_velocities(x, SR, notes, peak_db=0.0, peak_velocity=127)[0].tolist() == [115, 1, 127]
    # drums and pitched notes have their own peaks
    rng = np.random.default_rng(0)
    y = x.copy()
    y[4000:8000] = (1e-3 * rng.standard_normal(4000)).astype(np.float32)
    both = C.records([C.rec(0.05, 60), C.rec(0.30, 38, program=128, is_drum=1), C.rec(0.55, 60)])
    vel, E, peaks, counts = V.note_velocities(y, SR, both)
    assert vel.tolist() == [108, 120, 120] and peaks[1] == E[1] and peaks[0] == E[2] and counts.tolist() == [3, 0]


def test_the_unmeasured_rules_and_counts():
    case = _case("edges")
    ref = C.reference(case)
    n_edges = C.edge_records().size
    E, vel = ref["E"][:n_edges], ref["vel"][:n_edges]
    unmeasured = np.isnan(E)
    #            inf -inf nan       pitch -1, 128    127 pitched    drum pitch 128, drum onset NaN
    assert np.flatnonzero(unmeasured).tolist() == [5, 6, 7, 12, 13, 16, 20, 21]
    assert (vel[unmeasured] == 100).all() and ref["counts"].tolist() == [n_edges - 8 + 20, 8]
    assert E[1] == 0.0 and E[3] == 0.0 and E[4] == 0.0 and E[8] == 0.0 and E[9] == 0.0       # windows that meet no audio: measured, silent
    assert (vel[[1, 3, 4, 8, 9]] == 1).all()
    assert E[0] > 0 and E[2] > 0 and E[14] >= 0 and E[15] > 0
    assert E[17] == ref["P"][17] and E[18] == ref["P"][18] == E[19]                             # drums have E = P, by either rule
    assert E[22] == E[23] > 0                                                                  # the offset is not read
    other = C.reference(_case("drum_program_5"))
    assert np.flatnonzero(np.isnan(other["E"][:n_edges])).tolist() == [5, 6, 7, 12, 13, 16, 20, 21]
    assert not other["drum"][19] and other["drum"][18] and other["E"][19] != other["E"][18]      # program 128 is an instrument there
    assert int(other["drum"][n_edges:].sum()) == int((case["rec"][n_edges:n_edges + 12]["program"] == 5).sum()
                                                      + (case["rec"][n_edges:n_edges + 12]["is_drum"] != 0).sum())
    for name in ("nan_sample", "inf_sample", "minus_inf_sample"):
        bad, clean = C.reference(_case(name)), V.note_velocities(C._base()[0], SR, _case(name)["rec"])
        assert np.flatnonzero(np.isnan(bad["E"])).tolist() == [30] and bad["counts"].tolist() == [40, 1] and bad["vel"][30] == 100
        keep = np.arange(41) != 30
        assert np.array_equal(bad["E"][keep], clean[1][keep]) and not np.isnan(clean[1][30])              # the other records are untouched
    only = C.reference(_case("only_drums"))
    assert only["peaks"][0] == 0.0 and only["peaks"][1] > 0
    only = C.reference(_case("only_pitched"))
    assert only["peaks"][1] == 0.0 and only["peaks"][0] > 0
    zero = C.reference(_case("zero_audio"))
    assert (zero["E"] == 0).all() and (zero["vel"] == 120).all() and zero["peaks"].tolist() == [0.0, 0.0]


def test_windows_at_the_file_edges_and_half_samples():
    x = C._base()[0]
    W = 1024
    w = V.velocity_tables(SR, W, 4)[0].astype(np.float64)
    power = lambda seg: 2.0 * np.sum((w * seg) ** 2) / np.sum(w * w)
    drum = lambda onset: C.records([C.rec(onset, 40, is_drum=1)])
    e = lambda onset: V.note_velocities(x, SR, drum(onset))[1][0]
    # before sample 0: the first 160 samples of the window are zeros
    assert e(-0.01) == pytest.approx(power(np.concatenate([np.zeros(160), x[:W - 160]])), rel=1e-12)
    # across the end
    assert e((x.size - 300) / SR) == pytest.approx(power(np.concatenate([x[-300:], np.zeros(W - 300)])), rel=1e-12)
    assert e((x.size - 1) / SR) > 0 and e(x.size / SR) == 0.0 and e(-(W - 1) / SR) > 0 and e(-W / SR) == 0.0
    # half samples round to even: the multiply gives exactly 0.5, 1.5 and 2.5
    assert [(k + 0.5) / SR * SR for k in range(3)] == [0.5, 1.5, 2.5]
    assert e(0.5 / SR) == e(0.0) and e(1.5 / SR) == e(2.0 / SR) and e(2.5 / SR) == e(2.0 / SR) and e(0.0) != e(2.0 / SR)
    # the roll's frame rule: 0.57 * 100 is below 57 in f64 and still lands there
    assert 0.57 * 100 < 57 and V.note_velocities(x, 100, drum(0.57), window_samples=64)[1][0] == V.note_velocities(x, 100, drum(57 / 100), window_samples=64)[1][0]


def test_the_spec_does_not_depend_on_the_order_of_the_records():
    case = _case("n_257")
    ref = C.reference(case)
    perm = np.random.default_rng(1).permutation(case["rec"].size)
    vel, E, peaks, counts = V.note_velocities(case["audio"], SR, case["rec"][perm])
    assert np.array_equal(vel, ref["vel"][perm]) and np.array_equal(E, ref["E"][perm]) and np.array_equal(peaks, ref["peaks"])
    assert np.array_equal(counts, ref["counts"])
    # a list of Note is the same input
    notes = [Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"])) for r in case["rec"][:40]]
    assert np.array_equal(V.note_velocities(case["audio"], SR, notes)[1], V.note_velocities(case["audio"], SR, case["rec"][:40])[1])


def test_parameters_outside_their_ranges_are_refused():
    x, notes = np.zeros(100, np.float32), C.records([C.rec(0.0, 60)])
    for bad in ({"window_samples": 63}, {"window_samples": 4097}, {"n_harmonics": 0}, {"n_harmonics": 9}, {"velocity_per_db": 0.0},
                {"velocity_per_db": float("nan")}, {"velocity_per_db": float("inf")}, {"peak_velocity": 0}, {"peak_velocity": 128},
                {"min_velocity": 0}, {"min_velocity": 121}, {"default_velocity": 0}, {"default_velocity": 128}, {"peak_db": float("inf")},
                {"drum_program": -1}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            V.note_velocities(x, SR, notes, **bad)
    with pytest.raises(TypeError, match="window"):
        V.note_velocities(x, SR, notes, window=64)


# ---------------------------------------------------------------- what the cases must meet
def test_the_f32_restatement_sets_the_tolerance():
    """TAU is 16 times the error of the specification restated in f32, measured against the f64 specification over every case"""
    worst, where = 0.0, None
    for case in CASES:
        ref = C.reference(case)
        m = ~np.isnan(ref["E"])
        if not m.any():
            continue
        e32 = C.energies_f32(case)
        assert not np.isnan(e32[m]).any()
        err = np.abs(e32[m].astype(np.float64) - ref["E"][m]) / np.maximum(ref["P"][m], 1e-12)
        if err.max() > worst:
            worst, where = float(err.max()), case["id"]
    print(f"largest |E_f32 - E_f64| / P = {worst:.3g} ({where}); F32_ERROR = {C.F32_ERROR:.3g}, TAU = {C.TAU:.3g}")
    assert C.F32_ERROR / 2 < worst <= C.F32_ERROR and C.TAU == 16 * C.F32_ERROR


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_few_records_have_more_than_one_admissible_velocity(case):
    ref = C.reference(case)
    spans = C.admissible(case)
    measured = ~np.isnan(ref["E"])
    assert len(spans) == C.live(case) == ref["vel"].size
    wide = [i for i, (lo, hi) in enumerate(spans) if hi > lo]
    print(f"{case['id']}: {int(measured.sum())} measured, {len(wide)} with two admissible velocities")
    assert all(lo <= v <= hi for (lo, hi), v in zip(spans, ref["vel"].tolist()))
    assert all(measured[i] and spans[i][1] - spans[i][0] == 1 for i in wide)
    assert len(wide) <= 0.05 * max(int(measured.sum()), 1)


def test_the_cases_cover_what_they_claim():
    sizes = {C.live(c) for c in CASES}
    assert {0, 1, 4, 5, 65, 257} <= sizes
    assert {c["params"].get("window_samples", 1024) for c in CASES} == {64, 96, 1000, 1024, 4096}
    assert {c["params"].get("n_harmonics", 4) for c in CASES} >= {1, 4, 8}
    steps = V.velocity_tables(SR, 1024, 8)[1]
    assert (steps[108] != 0).sum() == 1 and (steps[127] == 0).all() and (steps[0] != 0).all() and (steps[60, :4] != 0).all()
    ref = C.reference(_case("n_257"))
    db = 10 * np.log10(ref["E"][~ref["drum"]])
    assert db.max() - db.min() > 40                                         # the dynamics the velocities are to carry
    assert len(set(ref["vel"].tolist())) > 40


# ---------------------------------------------------------------- MIDI, header, exports, lifecycle, defaults
def test_midi_round_trips_the_velocities():
    case = _case("n_65")
    vel = C.reference(case)["vel"].tolist()
    notes = sorted(Note(float(r["onset"]), float(r["onset"]) + 0.25, bool(r["is_drum"]), 128 if r["is_drum"] else 0, int(r["pitch"]), velocity=v)
                   for r, v in zip(case["rec"], vel))
    back = sorted(read_midi_notes(notes_to_midi_bytes(notes)))
    key = lambda n: (round(n.onset, 2), n.is_drum, n.program, n.pitch)
    assert len(back) == len(notes) and {key(n): n.velocity for n in back} == {key(n): n.velocity for n in notes}
    assert len({n.velocity for n in back}) > 10


def test_the_abi_declares_lists_and_exports_the_entry_points(tmp_path):
    import shutil
    import subprocess
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    names = {"ymt3_velocity_create", "ymt3_velocity_destroy", "ymt3_note_velocities"}
    assert names <= set(re.findall(r"\b(ymt3_[a-z_0-9]+)\s*\(", header)) and names <= set(_lib.SYMBOLS)
    assert "typedef struct ymt3_velocity_s* ymt3_velocity;" in header and "} ymt3_velocity_params;" in header
    assert re.search(r"#define YMT3_ABI_VERSION 3\b", header)
    # the params struct: the header's field order and the size a C compiler gives it
    body = header[header.index("typedef struct ymt3_velocity_params {"):header.index("} ymt3_velocity_params;")]
    fields = [f.strip() for line in body.splitlines()[1:] for f in re.sub(r"^\s*(double|int32_t)\s+", "", line).rstrip(";").split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.VelocityParams._fields_] and ctypes.sizeof(_lib.VelocityParams) == 48
    gcc = shutil.which("gcc")
    if gcc is not None:
        src = tmp_path / "abi.c"
        src.write_text('#include "ymt3.h"\ntypedef char size_is_48[sizeof(ymt3_velocity_params) == 48 ? 1 : -1];\n'
                       'int main(void) { ymt3_velocity_params p; int (*f)(ymt3_handle, const ymt3_velocity_params*, ymt3_velocity*) = ymt3_velocity_create;\n'
                       '(void)p; (void)f; return 0; }\n')
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
    for n in ("note_velocities", "NoteVelocity", "estimate_velocities"):
        assert n in yourmt3_amd.__all__ and getattr(yourmt3_amd, n) is getattr(V, n)


def test_the_object_shares_the_lifecycle_and_stays_out_of_the_models_namespace():
    """tests/test_cpu_host.py::test_closed_and_orphaned_objects_say_so_and_free_once for NoteVelocity (its doubles, copied)"""
    from yourmt3_amd import model as M
    assert issubclass(V.NoteVelocity, M._Owned) and (V.NoteVelocity._destroy, V.NoteVelocity._noun) == ("ymt3_velocity_destroy", "note velocity object")
    assert "NoteVelocity" not in vars(M) and V.NoteVelocity not in vars(M).values()
    assert "from .velocity import NoteVelocity" in inspect.getsource(M.YourMT3.compile_note_velocity)

    class Lib:
        def __init__(self):
            self.freed = []

        def __getattr__(self, name):
            if not name.startswith("ymt3_"):
                raise AttributeError(name)
            return lambda c: self.freed.append((name, c.value))

    class Model:                                     # what _own asks of a model
        def __init__(self):
            self._lib = Lib()
            self._owned = __import__("weakref").WeakSet()

    noun, destroy = "note velocity object", "ymt3_velocity_destroy"
    obj = V.NoteVelocity.__new__(V.NoteVelocity)
    obj.close()                                      # before _own: nothing to free
    model = Model()
    obj._own(model)
    assert obj in model._owned
    with pytest.raises(ValueError, match=f"^the {noun} has been closed$"):
        obj.ptr
    assert obj._live_model() is model
    obj._c = ctypes.c_void_p(0x1000)
    assert obj.ptr.value == 0x1000
    with obj as same:
        assert same is obj
    obj.close()
    assert model._lib.freed == [(destroy, 0x1000)]
    with pytest.raises(ValueError, match=f"^the {noun} has been closed$"):
        obj.ptr
    freed = model._lib.freed
    del model
    with pytest.raises(ValueError, match=f"^the {noun}'s model is gone$"):
        obj._live_model()
    assert freed == [(destroy, 0x1000)]


def test_velocity_is_off_by_default():
    from yourmt3_amd.task_manager import TaskManager
    from yourmt3_amd.transcribe import LiveTranscriber, estimate_velocities, transcribe
    sig = inspect.signature(transcribe).parameters
    assert sig["velocity"].default is False and sig["velocity_params"].default is None
    sig = inspect.signature(TaskManager.tokens_to_notes_device).parameters
    assert sig["velocity"].default is None and sig["audio"].default is None
    assert "velocity" not in inspect.signature(LiveTranscriber.__init__).parameters and "velocities" in LiveTranscriber.__doc__
    assert estimate_velocities is V.estimate_velocities
    assert Note(0.0, 1.0, False, 0, 60).velocity == 100
    assert math.isnan(V.DEFAULTS["peak_db"]) and {k: v for k, v in V.DEFAULTS.items() if k != "peak_db"} == dict(
        window_samples=1024, n_harmonics=4, velocity_per_db=2.0, peak_velocity=120, min_velocity=1, default_velocity=100, drum_program=128)
