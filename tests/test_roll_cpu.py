"""Piano roll and frame metrics, the parts that need no GPU (include/ymt3.h, piano roll and frame metrics):
  1. piano_roll and frame_metrics (yourmt3_amd/metrics.py), the specification, equal tests/roll_model.py -- the rules as a plain Python
     loop -- on every case of tests/roll_cases.py, byte for byte and integer for integer;
  2. the rounding examples as literal numbers, the derived values on hand-computed counts, the refused arguments;
  3. the cases are not vacuous: some case has TP, SUB, MISS and FA all > 0 in the agnostic row, some has skipped records on both sides;
  4. the C ABI: the four entry points and both typedefs are declared, listed and exported, the ABI version is still 3;
  5. evaluate() takes frames=False."""
import inspect
import os
import re

import numpy as np
import pytest

import roll_cases as C
import roll_model as M
from yourmt3_amd.metrics import FA, MISS, N_EST, N_REF, SUB, TP, FrameMetricCounts, frame_metrics, frame_of, piano_roll
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.cases()
IDS = [c["id"] for c in CASES]


def _p(case):
    return case["n_frames"], case["n_programs"], case["drum_program"], case["fps"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_piano_roll_equals_the_model(case):
    _, rolls = C.reference(case)
    for side, got in zip(("ref", "est"), rolls):
        assert got.dtype == np.uint8 and got.shape == (case["n_programs"] + 1, case["n_frames"], 128)
        assert np.array_equal(got, M.model_roll(case[side], *_p(case))), side


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frame_metrics_equals_the_model(case):
    got, _ = C.reference(case)
    flat = got.flat()
    assert flat.dtype == np.int64 and flat.size == (case["n_programs"] + 1) * 6 + 2
    assert flat.tolist() == M.model_counts(case["ref"], case["est"], *_p(case))


def test_frame_counts_follow_from_the_rolls():
    """the counts are sums over the two rolls, and N_REF - MISS = N_EST - FA = TP + SUB in every row"""
    for case in CASES:
        got, (r, e) = C.reference(case)
        r, e = r.astype(np.int64), e.astype(np.int64)
        nr, ne, tp = r.sum(2), e.sum(2), (r & e).sum(2)
        want = np.stack([tp.sum(1), nr.sum(1), ne.sum(1), (np.minimum(nr, ne) - tp).sum(1), np.maximum(0, nr - ne).sum(1),
                         np.maximum(0, ne - nr).sum(1)], 1)
        assert np.array_equal(got.counts, want), case["id"]
        c = got.counts
        assert np.array_equal(c[:, N_REF] - c[:, MISS], c[:, TP] + c[:, SUB]) and np.array_equal(c[:, N_EST] - c[:, FA], c[:, TP] + c[:, SUB])


def test_the_cases_are_not_vacuous():
    full, skipped_both, shapes = [], [], set()
    for case in CASES:
        got, _ = C.reference(case)
        a = got.counts[case["n_programs"]]
        if min(a[TP], a[SUB], a[MISS], a[FA]) > 0:
            full.append(case["id"])
        if got.skipped[0] > 0 and got.skipped[1] > 0:
            skipped_both.append(case["id"])
        shapes.add(case["n_frames"])
    print("TP, SUB, MISS, FA all > 0 in:", full, "; skipped on both sides in:", skipped_both)
    assert "random_400" in full and "polyphony" in full and "skipped_records" in skipped_both
    assert set(C.FRAME_COUNTS) <= shapes and {1, 256} <= {c["n_programs"] for c in CASES}
    by_id = {c["id"]: C.reference(c)[0] for c in CASES}
    assert by_id["skipped_records"].skipped.tolist() == [8, 10]
    assert by_id["both_empty"].flat().sum() == 0
    assert by_id["1_program"].counts[1].sum() == 0 and by_id["1_program"].counts[0, N_REF] == 2 and by_id["1_program"].skipped.tolist() == [1, 0]
    # nr > ne, nr < ne, nr == ne != tp: 10 frames each
    assert by_id["polyphony"].counts[3].tolist() == [30, 60, 60, 10, 20, 20]


def test_rounding_examples():
    assert frame_of(1.05, 100.0) == 105
    assert 0.57 * 100 == 56.99999999999999 and frame_of(0.57, 100.0) == 57      # f64 noise below the step
    assert 1.1 * 100 == 110.00000000000001 and frame_of(1.1, 100.0) == 110       # and above it
    assert 2.675 * 100 == 267.5 and frame_of(2.675, 100.0) == 268                # a half-way product: to even
    assert 0.04 * 62.5 == 2.5 and frame_of(0.04, 62.5) == 2                       # half to even: down
    assert 0.056 * 62.5 == 3.5 and frame_of(0.056, 62.5) == 4                     # half to even: up
    assert frame_of(float("inf"), 100.0) == float("inf") and frame_of(float("-inf"), 100.0) == float("-inf")
    n = lambda on, off, pitch=60, program=0, drum=False: Note(on, off, drum, 128 if drum else program, pitch)
    roll = piano_roll([n(1.05, 1.07), n(0.04, 0.04, 61), n(0.5, 0.3, 62), n(0.2, float("nan"), 36, drum=True)], 200, 130)
    assert np.flatnonzero(roll[130, :, 60]).tolist() == [105, 106] and np.flatnonzero(roll[0, :, 60]).tolist() == [105, 106]
    assert np.flatnonzero(roll[130, :, 61]).tolist() == [4] and np.flatnonzero(roll[130, :, 62]).tolist() == [50]      # the one-frame rule
    assert np.flatnonzero(roll[128, :, 36]).tolist() == [20] and roll[130, :, 36].sum() == 0 and roll.sum() == 2 * 4 + 1
    inf = float("inf")
    roll = piano_roll([n(inf, inf), n(-inf, 0.03, 61), n(0.08, inf, 62)], 10, 130)
    assert roll[130, :, 60].sum() == 0 and np.flatnonzero(roll[130, :, 61]).tolist() == [0, 1, 2] and np.flatnonzero(roll[130, :, 62]).tolist() == [8, 9]
    assert piano_roll([n(0.0, 1.0)], 0, 130).shape == (131, 0, 128)


def test_derived_values_on_hand_computed_counts():
    counts = np.zeros((4, 6), np.int64)
    counts[3] = [30, 60, 40, 10, 20, 0]                                           # TP, N_REF, N_EST, SUB, MISS, FA
    counts[0] = [10, 20, 40, 10, 0, 20]
    counts[2] = [20, 20, 20, 0, 0, 0]
    m = FrameMetricCounts(counts, [1, 2], drum_program=1)
    assert m.precision(3) == 0.75 and m.recall(3) == 0.5 and m.f_measure(3) == 2 * 0.75 * 0.5 / 1.25 == m.frame_f
    assert m.accuracy(3) == 30 / 70 and m.error(3) == {"sub": 10 / 60, "miss": 20 / 60, "fa": 0.0, "total": 30 / 60}
    assert m.precision(slice(0, 3)) == 0.5 and m.recall(slice(0, 3)) == 0.75 and m.multi_frame_f == 2 * 0.5 * 0.75 / 1.25
    assert m.f_measure(1) == 0.0 and m.accuracy(1) == 0.0 and m.error(1)["total"] == 0.0            # empty denominators
    assert set(m.per_program()) == {0, 2} and m.per_program()[2]["frame_f"] == 1.0 and m.per_program()[0]["n_est"] == 40
    s = m.summary()
    assert set(s) == {"frame_f", "frame_p", "frame_r", "frame_acc", "frame_err", "multi_frame_f", "frame_counts"}
    assert s["frame_p"] == 0.75 and s["frame_acc"] == 30 / 70 and s["frame_err"]["miss"] == 20 / 60 and s["frame_counts"] is m.counts
    assert FrameMetricCounts.from_flat(m.flat(), 3, 1) == m and m.flat().tolist() == counts.reshape(-1).tolist() + [1, 2]
    assert FrameMetricCounts.from_flat(m.flat(), 3, 2) != m
    with pytest.raises(ValueError, match="integers"):
        FrameMetricCounts.from_flat(m.flat(), 4)
    # from notes: the reference sounds 60 and 62 for 10 frames, the estimate 60 for 5 of them and 64 for all
    n = lambda on, off, pitch: Note(on, off, False, 0, pitch)
    got = frame_metrics([n(0.0, 0.1, 60), n(0.0, 0.1, 62)], [n(0.0, 0.05, 60), n(0.0, 0.1, 64)], 10, 130)
    assert got.counts[130].tolist() == [5, 20, 15, 10, 5, 0] and got.counts[0].tolist() == got.counts[130].tolist()
    assert got.frame_f == 2 * (5 / 15) * (5 / 20) / (5 / 15 + 5 / 20) and got.skipped.tolist() == [0, 0]


def test_refused_arguments():
    notes = [Note(0.0, 1.0, False, 0, 60)]
    for f in (piano_roll, lambda *a, **k: frame_metrics(notes, *a, **k)):
        for fps in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="frames_per_second"):
                f(notes, 10, 130, frames_per_second=fps)
        with pytest.raises(ValueError, match="n_frames"):
            f(notes, -1, 130)
        with pytest.raises(ValueError, match="n_programs"):
            f(notes, 10, 0, drum_program=0)
        for dp in (-1, 130):
            with pytest.raises(ValueError, match="drum_program"):
                f(notes, 10, 130, drum_program=dp)


def test_the_c_abi_declares_lists_and_exports_the_entry_points():
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    lib = _lib.load()
    for name in ("ymt3_roll_create", "ymt3_roll_destroy", "ymt3_piano_roll", "ymt3_frame_metrics"):
        assert re.search(r"\b" + name + r"\s*\(ymt3_", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ymt3_roll_s* ymt3_roll;" in header and "} ymt3_roll_params;" in header
    assert lib.ymt3_abi_version() == 3 and "#define YMT3_ABI_VERSION 3" in header
    body = header[header.index("typedef struct ymt3_roll_params {"):header.index("} ymt3_roll_params;")]
    assert re.findall(r"\b([a-z_]+)(?=[,;])", body) == [n for n, _ in _lib.RollParams._fields_]
    doc = header[header.index("/* Device piano roll and frame metrics"):header.index("typedef struct ymt3_roll_params {")]
    for rule in ("rint(t * frames_per_second)", "[F(on), max(F(off), F(on) + 1))", "[F(on), F(on) + 1)", "before any conversion to an integer",
                 "a set member, not a count", "SUB = sum (min(nr, ne) - tp)", "read ON THE DEVICE", "min(n, max(*count, 0))",
                 "2 x (n_programs + 1) x max_frames x 16 bytes", "126 MB per side", "(n_programs + 1) * 6 + 2", "YMT3_ERR_UNSUPPORTED"):
        assert rule in doc, rule


def test_evaluate_and_the_package_take_the_new_names():
    import importlib
    import yourmt3_amd
    transcribe = importlib.import_module("yourmt3_amd.transcribe")
    sig = inspect.signature(transcribe.evaluate)
    assert sig.parameters["frames"].default is False and sig.parameters["frames_per_second"].default == 100.0
    assert list(inspect.signature(transcribe.piano_roll).parameters) == ["model", "notes", "end_sec", "frames_per_second", "per_program", "task_manager"]
    for name in ("piano_roll", "frame_metrics", "FrameMetricCounts", "PianoRoll"):
        assert name in yourmt3_amd.__all__
    assert yourmt3_amd.frame_metrics is frame_metrics and yourmt3_amd.FrameMetricCounts is FrameMetricCounts
