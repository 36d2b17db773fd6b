"""Alignment, the parts that need no GPU (include/ymt3.h, alignment):
  1. dtw_align (yourmt3_amd/metrics.py), the specification, equals tests/align_model.py -- the rules as plain loops over every cell -- on
     every small case of tests/align_cases.py: total, path, warp and skipped;
  2. the band: at band_frames = 1 the end cell, and every in-band cell, is reachable for every shape 1 ... 40 x 1 ... 40;
  3. properties: a set against itself gives the exact diagonal with total 0; warp is non-decreasing from 0 to the lowest j of the last row; the transposed problem
     has the same total;
  4. W as literal numbers, warp_notes, the refused arguments;
  5. recovery: on the tempo-curve case the onset F of the warped reference against the unwarped one;
  6. the C ABI and the Python names."""
import inspect
import os
import re

import numpy as np
import pytest

import align_cases as C
import align_model as M
from yourmt3_amd.metrics import ALIGN_INF, Alignment, dtw_align, note_metrics, warp_notes, warp_times
from yourmt3_amd.task_manager import NOTE_RECORD, Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.cases()
SMALL = [c for c in CASES if C.small(c)]


@pytest.mark.parametrize("case", SMALL, ids=[c["id"] for c in SMALL])
def test_dtw_align_equals_the_model(case):
    got = C.reference(case)
    total, path, warp, skipped = M.align(case["ref"], case["est"], case["na"], case["nb"], case["n_programs"], case["drum_program"], case["fps"],
                                         case["band"])
    assert got.path.dtype == np.int32 and got.warp.dtype == np.int32 and got.warp.shape == (case["na"],)
    assert got.total == total and got.path.tolist() == [list(c) for c in path] and got.warp.tolist() == warp
    assert got.skipped.tolist() == list(skipped)
    assert Alignment.from_flat(got.flat(), case["na"]) == got and got.flat().dtype == np.int64


def test_the_cases_cover_what_they_should():
    ids = {c["id"] for c in CASES}
    shapes = {(c["na"], c["nb"]) for c in CASES}
    for a in C.FRAME_COUNTS:
        for b in C.OTHER_SIDE:
            assert (a, b) in shapes and (b, a) in shapes
    assert set(C.SQUARES) <= shapes and {(3, 200), (200, 3), (3000, 2750)} <= shapes
    for name in ("both_empty", "empty_ref", "empty_est", "one_note_at_the_end", "identical_sets", "drums_only", "skipped_records",
                 "infinite_and_nan_times", "tempo_curve"):
        assert name in ids
    assert {c["band"] for c in CASES} >= set(C.BANDS)
    by_id = {c["id"]: C.reference(c) for c in CASES if C.small(c)}
    assert by_id["skipped_records"].skipped.tolist() == [8, 10] and by_id["infinite_and_nan_times"].skipped.tolist() == [2, 1]
    assert by_id["both_empty"].total == 0 and by_id["empty_ref"].total > 0 and by_id["empty_est"].total > 0
    # ties everywhere: the diagonal first, then (i-1, j) until the band's edge
    assert by_id["both_empty"].path_len == 90 and by_id["drums_only"].total > 0
    for c in CASES:
        if C.small(c):
            assert 0 <= by_id[c["id"]].total < ALIGN_INF, c["id"]


def test_band_one_reaches_the_end_and_every_cell_of_the_band():
    for na in range(1, 41):
        for nb in range(1, 41):
            band = {(i, j) for i in range(na) for j in range(nb) if M.in_band(i, j, na, nb, 1)}
            assert (0, 0) in band and (na - 1, nb - 1) in band
            assert M.reachable(na, nb, 1) == band, (na, nb)
    # and the specification agrees on a few of them, with nothing sounding: the total is 0 and the path exists
    none = np.zeros(0, NOTE_RECORD)
    for na, nb in ((1, 1), (1, 40), (40, 1), (2, 39), (17, 23), (40, 40), (39, 40)):
        got = dtw_align(none, none, na, nb, 3, 1, band_frames=1)
        assert got.total == 0 and got.path[0].tolist() == [0, 0] and got.path[-1].tolist() == [na - 1, nb - 1]
        assert got.path.tolist() == [list(c) for c in M.align(none, none, na, nb, 3, 1, 100.0, 1)[1]]


def test_a_set_against_itself_is_the_diagonal():
    """the diagonal predecessor always ties at 0 and is first in the tie order"""
    for name, n in (("identical_sets", 90), ("tempo_curve", 700)):
        case = C.case(name)
        for band in (1, 7, 1 << 20):
            got = dtw_align(case["ref"], case["ref"], n, n, band_frames=band, **C.params(case))
            assert got.total == 0 and got.path.tolist() == [[i, i] for i in range(n)] and got.warp.tolist() == list(range(n))


def test_warp_is_monotone_and_the_transposed_problem_has_the_same_total():
    """(cost and band are symmetric, so D is; paths may differ where the two non-diagonal steps tie, so only totals are compared)

    The issue asks for warp's ends to be 0 and p, and defines warp[i] = min { j : (i, j) on the path }.  The two contradict each other
    whenever the path ends along the last row (every 1 x N case: warp[0] = 0 although p = N - 1).  The min rule is kept; what replaces
    "warp[q] = p" is exact: the path's last cell is (q, p), and warp[i], for EVERY i, is the lowest j of the path in row i."""
    for case in CASES:
        got = C.reference(case)
        p, q = case["nb"] - 1, case["na"] - 1
        assert got.warp[0] == 0 and np.all(np.diff(got.warp) >= 0), case["id"]
        assert got.path[0].tolist() == [0, 0] and got.path[-1].tolist() == [q, p] and got.path_len <= case["na"] + case["nb"] - 1
        steps = np.diff(got.path, axis=0)
        assert steps.min(initial=0) >= 0 and steps.max(initial=1) <= 1 and np.all(steps.sum(1) >= 1)
        rows, first = np.unique(got.path[:, 0], return_index=True)       # the path is sorted: a row's first cell has its lowest j
        assert rows.tolist() == list(range(q + 1)) and np.array_equal(got.warp, got.path[first, 1]), case["id"]
        assert got.warp[q] == got.path[got.path[:, 0] == q, 1].min() and (got.warp[q] == p) == (got.path[-2:, 0].tolist() != [q, q])
        if C.small(case):
            other = dtw_align(case["est"], case["ref"], case["nb"], case["na"], band_frames=case["band"], **C.params(case))
            assert other.total == got.total and other.skipped.tolist() == got.skipped.tolist()[::-1], case["id"]


def test_warp_examples():
    warp = np.array([0, 2, 4, 4, 7], np.int32)                                   # q = 4
    W = lambda t, fps=100.0: float(warp_times(t, warp, fps))
    assert W(0.0) == 0.0 and W(0.01) == 0.02 and W(0.02) == 0.04 and W(0.03) == 0.04 and W(0.04) == 0.07      # grid times
    assert 0.005 * 100 == 0.5 and W(0.005) == 0.01                               # half a frame: (0 + 0.5 * 2) / 100
    assert 0.035 * 100 == 3.5000000000000004 and W(0.035) == (4 + 0.5000000000000004 * 3) / 100
    assert W(-1.0) == 0.0 and W(float("-inf")) == 0.0                            # clamped below
    assert W(0.05) == 0.07 and W(1e300) == 0.07 and W(float("inf")) == 0.07      # at or past the end: warp[q] / fps
    assert np.isnan(W(float("nan")))
    assert W(0.032, 62.5) == 4 / 62.5 and W(0.04, 62.5) == (4 + 0.5 * 0) / 62.5  # 0.032 * 62.5 = 2, 0.04 * 62.5 = 2.5
    one = np.array([0], np.int32)                                                # a single frame: everything maps to 0
    assert warp_times([-1.0, 0.0, 0.5, float("inf")], one, 100.0).tolist() == [0.0, 0.0, 0.0, 0.0]
    for t in (0.0, 0.005, 0.0123, 0.035, 0.04, -3.0, 7.0, float("inf"), float("-inf")):
        assert W(t) == M.warp_time(t, warp.tolist(), 100.0), t
    # warp_notes: both times of every record, everything else copied, nothing filtered
    rec = np.zeros(4, NOTE_RECORD)
    rec[0] = (0.01, 0.035, 5, 60, 0, 0.25)
    rec[1] = (float("nan"), 0.02, -7, 999, 0, float("nan"))
    rec[2] = (0.02, float("nan"), 1, 36, 1, -1.5)
    rec[3] = (float("-inf"), float("inf"), 0, 0, 0, 0.0)
    out = warp_notes(rec, warp)
    assert out.dtype == NOTE_RECORD and out is not rec and rec["onset"][0] == 0.01
    assert out["onset"][[0, 2, 3]].tolist() == [0.02, 0.04, 0.0] and np.isnan(out["onset"][1])
    assert out["offset"][[0, 1, 3]].tolist() == [W(0.035), 0.04, 0.07] and np.isnan(out["offset"][2])
    for name in ("program", "pitch", "is_drum"):
        assert out[name].tolist() == rec[name].tolist()
    assert np.array_equal(out["score"], rec["score"], equal_nan=True)
    notes = [Note(0.01, 0.035, False, 5, 60), Note(0.02, 0.03, True, 128, 36)]
    assert warp_notes(notes, warp)["onset"].tolist() == [0.02, 0.04]


def test_refused_arguments():
    notes = [Note(0.0, 1.0, False, 0, 60)]
    for fps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="frames_per_second"):
            dtw_align(notes, notes, 10, 10, 130, frames_per_second=fps, band_frames=5)
        with pytest.raises(ValueError, match="frames_per_second"):
            warp_notes(notes, np.zeros(3, np.int32), fps)
    for bad in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="n_ref_frames"):
            dtw_align(notes, notes, bad, 10, 130, band_frames=5)
        with pytest.raises(ValueError, match="n_est_frames"):
            dtw_align(notes, notes, 10, bad, 130, band_frames=5)
    for band in (0, -3):
        with pytest.raises(ValueError, match="band_frames"):
            dtw_align(notes, notes, 10, 10, 130, band_frames=band)
    with pytest.raises(ValueError, match="n_programs"):
        dtw_align(notes, notes, 10, 10, 0, drum_program=0, band_frames=5)
    for dp in (-1, 130):
        with pytest.raises(ValueError, match="drum_program"):
            dtw_align(notes, notes, 10, 10, 130, drum_program=dp, band_frames=5)
    with pytest.raises(ValueError, match="warp"):
        warp_notes(notes, np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="integers"):
        Alignment.from_flat(np.zeros(5, np.int64), 3)


def test_alignment_recovers_the_note_metrics_on_the_tempo_curve():
    """The tempo-curve case of tests/align_cases.py (its own generator, seed 20261019): 3000 x 2750 frames, band 400.  The host
    specification gives onset F 0.0237 before the warp and 0.8629 after it (onset+offset F 0.0034 -> 0.8528, drum F 0.1614 -> 0.8969), total
    4795, path length 3499.  The bounds: before <= 0.1; after >= 0.8129, the specification's value minus 0.05."""
    case = C.case("tempo_curve")
    got = C.reference(case)
    before = note_metrics(case["ref"], case["est"], 130)
    after = note_metrics(warp_notes(case["ref"], got.warp, case["fps"]), case["est"], 130)
    b, a = before.summary(), after.summary()
    print(f"tempo curve: total {got.total}, path_len {got.path_len}; onset F {b['onset_f']:.4f} -> {a['onset_f']:.4f}, "
          f"offset F {b['offset_f']:.4f} -> {a['offset_f']:.4f}, drum F {b['drum_onset_f']:.4f} -> {a['drum_onset_f']:.4f}")
    assert b["onset_f"] <= 0.1 and a["onset_f"] >= 0.8129
    assert a["drum_onset_f"] > b["drum_onset_f"] and a["offset_f"] > b["offset_f"]


def test_the_c_abi_declares_lists_and_exports_the_entry_points():
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    lib = _lib.load()
    for name in ("ymt3_aligner_create", "ymt3_aligner_destroy", "ymt3_align_notes", "ymt3_warp_notes"):
        assert re.search(r"\b" + name + r"\s*\(ymt3_", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ymt3_aligner_s* ymt3_aligner;" in header and "} ymt3_align_params;" in header
    assert lib.ymt3_abi_version() == 3 and "#define YMT3_ABI_VERSION 3" in header
    body = header[header.index("typedef struct ymt3_align_params {"):header.index("} ymt3_align_params;")]
    assert re.findall(r"\b([a-z_]+)(?=[,;])", body) == [n for n, _ in _lib.AlignParams._fields_]
    doc = header[header.index("/* Device alignment"):header.index("typedef struct ymt3_align_params {")]
    for rule in ("256 bits per frame", "rint(t * frames_per_second)", "before any conversion to an integer", "OWN frame counts",
                 "popc(ref_i XOR est_j)", "|i * p - j * q| <= band_frames * m", "m = max(p, q, 1)", "INF = 2^30", "D = min(best + c, INF)",
                 "FIRST of", "(diagonal, (i-1, j), (i, j-1))", "warp[i] = min { j : (i, j) on the path }", "path_len <= Na + Nb - 1",
                 "every warp[i] = -1", "warp[q] <= p", "The path's last cell is (q, p)", "k = floor(x) clamped to", "f = x - k clamped to [0, 1]", "W = (a + f * (b - a)) / frames_per_second",
                 "A NaN stays NaN", "-inf gives 0", "read ON THE DEVICE", "min(n, max(*count, 0))", "4 x M x (B / 8 + 2)", "64 x M",
                 "8 x (2 x M - 1)", "max_frames in [1, 2^20]", "YMT3_ERR_UNSUPPORTED", "notes_out_dev may equal notes_dev",
                 "No kernel waits on another", "One object serves one call at a"):
        assert rule in doc, rule


def test_evaluate_and_the_package_take_the_new_names():
    import importlib
    import yourmt3_amd
    transcribe = importlib.import_module("yourmt3_amd.transcribe")
    sig = inspect.signature(transcribe.evaluate)
    assert sig.parameters["align"].default is False and sig.parameters["band_sec"].default == 10.0
    names = list(inspect.signature(transcribe.align).parameters)
    assert names[:8] == ["model", "audio_info", "reference", "task_manager", "bsz", "frames_per_second", "band_sec", "output_dir"]
    for name in ("dtw_align", "warp_notes", "Alignment", "Aligner", "align"):
        assert name in yourmt3_amd.__all__
    assert yourmt3_amd.dtw_align is dtw_align and yourmt3_amd.Alignment is Alignment and yourmt3_amd.align is transcribe.align
    from yourmt3_amd.model import Aligner, YourMT3
    assert yourmt3_amd.Aligner is Aligner and list(inspect.signature(YourMT3.compile_aligner).parameters)[1:] == [
        "n_programs", "max_frames", "frames_per_second", "band_frames", "drum_program"]
