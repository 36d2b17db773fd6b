"""Named cases for the piano roll and the frame metrics, shared by tests/test_roll_cpu.py and tests/test_roll.py.  A case is a dict: id,
ref and est (NOTE_RECORD arrays), n_frames, n_programs, drum_program, fps.  reference(case) is the host specification's result
(yourmt3_amd/metrics.py: frame_metrics, and piano_roll of both sides), computed once per case and never changed."""
import functools

import numpy as np

from yourmt3_amd.metrics import frame_metrics, piano_roll
from yourmt3_amd.task_manager import NOTE_RECORD

SEED = 20261018
NAN, INF = float("nan"), float("inf")
FRAME_COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 257)          # around the wave (64), the expansion's tile (32 frames) and 256
EDGE_PITCHES = (0, 31, 32, 63, 64, 127)                       # the ends of the four 32-bit words of a frame


def records(rows) -> np.ndarray:
    """[(onset, offset, program, pitch, is_drum)] -> NOTE_RECORD array (score NaN: it is not read)"""
    rec = np.zeros(len(rows), NOTE_RECORD)
    for i, (on, off, program, pitch, drum) in enumerate(rows):
        rec[i] = (on, off, program, pitch, int(drum), NAN)
    return rec


def _case(name, ref, est, n_frames, n_programs=3, drum_program=1, fps=100.0):
    return {"id": name, "ref": records(ref), "est": records(est), "n_frames": n_frames, "n_programs": n_programs, "drum_program": drum_program,
            "fps": fps}


def params(case) -> dict:
    return {"n_programs": case["n_programs"], "drum_program": case["drum_program"], "frames_per_second": case["fps"]}


def _boundary_notes(nf):
    """notes around the ends and the tile boundaries of a roll of nf frames at 100 frames per second"""
    end = nf / 100
    ref = [(0.0, end, 0, 0, False),                           # the whole range
           (0.60, 0.70, 0, 31, False),                        # across frame 64
           (2.50, 2.62, 2, 32, False),                        # across frame 256
           (-0.50, 0.05, 0, 63, False),                       # clipped at the start: onset < 0
           (end - 0.02, end + 0.50, 2, 64, False),            # clipped at the end
           (end, end + 1.0, 0, 127, False),                   # onset >= n_frames / fps: no cell
           (0.01, 0.02, 1, 36, True), (end - 0.01, NAN, 0, 38, True)]
    est = [(0.01, end - 0.01, 0, 0, False), (0.62, 0.66, 0, 31, False), (2.55, 2.70, 2, 32, False), (-0.50, 0.03, 2, 63, False),
           (end - 0.03, end + 0.50, 2, 65, False), (end + 0.01, end + 1.0, 0, 127, False), (0.01, 0.5, 1, 36, True), (end, NAN, 0, 38, True)]
    return ref, est


def random_case(rng, n=400, n_frames=1000, n_programs=130, drum_program=128):
    """a reference of n notes and an estimate that is the reference with jitter, deletions and insertions"""
    def note():
        on = int(rng.integers(-20, n_frames + 20)) / 100
        prog = int(rng.integers(0, n_programs))
        return (on, on + int(rng.integers(0, 120)) / 100, prog, int(rng.choice([0, 31, 32, 36, 60, 61, 62, 63, 64, 127])), prog == drum_program)
    ref = [note() for _ in range(n)]
    est = []
    for on, off, prog, pitch, drum in ref:
        u = rng.random()
        if u < 0.1:
            continue
        if u > 0.95:
            pitch = (pitch + 1) % 128
        est.append((on + int(rng.integers(-3, 4)) / 100, off + int(rng.integers(-10, 11)) / 100, prog, pitch, drum))
    est += [note() for _ in range(n - len(est) + 10)]
    return ref, [est[i] for i in rng.permutation(len(est))]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    out = []
    for nf in FRAME_COUNTS:
        out.append(_case(f"frames_{nf}", *_boundary_notes(nf), nf))
    # every edge pitch on both sides, partly overlapping in time, and one pitch per word on one side only
    ref = [(0.10 + 0.01 * i, 0.40, 0, p, False) for i, p in enumerate(EDGE_PITCHES)] + [(0.2, 0.3, 2, 1, False)]
    est = [(0.12, 0.35 + 0.02 * i, 0, p, False) for i, p in enumerate(EDGE_PITCHES)] + [(0.2, 0.3, 2, 33, False), (0.2, 0.3, 2, 126, False)]
    out.append(_case("edge_pitches", ref, est, 50))
    # intervals: infinite times, an offset before its onset, F(on) == F(off) (the one-frame rule), a note shorter than a frame
    ref = [(INF, INF, 0, 60, False), (-INF, 0.10, 0, 61, False), (0.20, INF, 0, 62, False), (-INF, INF, 2, 63, False), (0.30, 0.10, 0, 64, False),
           (0.40, 0.40, 0, 65, False), (0.502, 0.504, 0, 66, False), (0.30, -INF, 0, 67, False), (INF, 0.3, 1, 36, True), (-INF, 0.3, 1, 37, True),
           (1e300, 2e300, 0, 68, False), (-1e300, 1e300, 0, 69, False)]
    est = [(0.05, 0.10, 0, 61, False), (0.20, 0.60, 0, 62, False), (0.0, 0.3, 2, 63, False), (0.30, 0.31, 0, 64, False), (0.40, 0.42, 0, 65, False),
           (0.50, 0.51, 0, 66, False), (0.31, 0.2, 0, 67, False), (0.0, INF, 1, 36, True), (-1e300, 0.2, 0, 69, False)]
    out.append(_case("intervals", ref, est, 64))
    # rounding: grid times at 100 frames per second; half-way products at 62.5 (0.04 -> 2.5 -> 2, 0.056 -> 3.5 -> 4)
    ref = [(1.05, 1.06, 0, 60, False), (0.57, 0.58, 0, 61, False), (2.675, 2.68, 0, 62, False), (0.29, 0.57, 0, 63, False)]
    est = [(1.05, 1.07, 0, 60, False), (0.56, 0.57, 0, 61, False), (2.67, 2.675, 0, 62, False), (0.28, 0.58, 0, 63, False)]
    out.append(_case("rounding_100", ref, est, 300))
    ref = [(0.04, 0.056, 0, 60, False), (0.056, 0.2, 0, 61, False), (0.04, NAN, 1, 36, True)]
    est = [(0.032, 0.064, 0, 60, False), (0.04, 0.056, 0, 61, False), (0.056, NAN, 1, 36, True)]
    out.append(_case("rounding_62_5", ref, est, 20, fps=62.5))
    # a cell is a set member: duplicates and overlaps of one key; one pitch under two programs (the agnostic row is their union)
    ref = [(0.10, 0.30, 0, 60, False), (0.10, 0.30, 0, 60, False), (0.20, 0.50, 0, 60, False), (0.10, 0.30, 2, 61, False), (0.25, 0.45, 0, 61, False)]
    est = [(0.10, 0.50, 0, 60, False), (0.15, 0.40, 2, 60, False), (0.10, 0.45, 0, 61, False), (0.10, 0.45, 0, 61, False)]
    out.append(_case("sets_and_unions", ref, est, 70))
    # drums: through is_drum with stray programs, through the drum program without the flag, NaN offsets, beside pitched notes of the pitch
    ref = [(0.10, 0.11, 1, 36, True), (0.20, 0.90, 7, 38, True), (0.30, NAN, -3, 42, True), (0.40, 0.41, 1, 36, False), (0.40, 0.80, 0, 36, False),
           (0.50, NAN, 1, 46, False), (0.10, 0.60, 2, 36, False)]
    est = [(0.10, 0.90, 1, 36, True), (0.21, 0.22, 1, 38, False), (0.30, 0.31, 1, 42, True), (0.41, NAN, 999, 36, True), (0.40, 0.70, 0, 36, False),
           (0.50, 0.51, 1, 46, True), (0.12, 0.55, 2, 36, False)]
    out.append(_case("drums", ref, est, 100))
    # records that do not count, every kind, on both sides
    good = [(0.10, 0.30, 0, 60, False), (0.20, 0.40, 2, 61, False)]
    bad = [(NAN, 0.5, 0, 60, False), (0.1, 0.5, 0, -1, False), (0.1, 0.5, 0, 128, False), (0.1, 0.5, -1, 60, False), (0.1, 0.5, 3, 60, False),
           (0.1, NAN, 0, 60, False), (NAN, NAN, 1, 36, True), (0.1, 0.2, 1, 128, True)]
    out.append(_case("skipped_records", good + bad, bad[:3] + good + bad[3:] + bad[:2], 60))
    # polyphony: frames with nr > ne, nr < ne, and nr == ne with other pitches
    ref = [(0.00, 0.10, 0, 60, False), (0.00, 0.10, 0, 62, False), (0.00, 0.10, 0, 64, False), (0.10, 0.20, 0, 60, False), (0.20, 0.30, 0, 60, False),
           (0.20, 0.30, 0, 62, False)]
    est = [(0.00, 0.10, 0, 60, False), (0.10, 0.20, 0, 60, False), (0.10, 0.20, 0, 65, False), (0.10, 0.20, 0, 67, False), (0.20, 0.30, 0, 60, False),
           (0.20, 0.30, 0, 63, False)]
    out.append(_case("polyphony", ref, est, 33))
    some = [(0.10, 0.30, 0, 60, False), (0.20, 0.21, 1, 36, True), (0.1, 0.5, 5, 60, False)]
    out += [_case("empty_ref", [], some, 40), _case("empty_est", some, [], 40), _case("both_empty", [], [], 40)]
    # one program, which is the drum program: every counted record is a drum hit and the agnostic row stays empty
    out.append(_case("1_program", [(0.1, 0.5, 0, 60, False), (0.2, NAN, 9, 61, True), (0.3, 0.4, 1, 62, False)],
                     [(0.1, 0.2, 0, 60, False), (0.21, NAN, 0, 61, False), (0.3, 0.4, 0, 62, True)], 50, n_programs=1, drum_program=0))
    ref = [(0.1, 0.5, 0, 60, False), (0.1, 0.5, 254, 61, False), (0.2, 0.3, 255, 36, False), (0.1, 0.5, 256, 60, False)]
    est = [(0.1, 0.4, 0, 60, False), (0.2, 0.6, 254, 61, False), (0.2, 0.9, 3, 36, True), (0.1, 0.5, 255, 127, False)]
    out.append(_case("256_programs", ref, est, 70, n_programs=256, drum_program=255))
    out.append(_case("random_400", *random_case(rng), 1000, n_programs=130, drum_program=128))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    case = next(c for c in cases() if c["id"] == case_id)
    rolls = tuple(piano_roll(case[side], case["n_frames"], **params(case)) for side in ("ref", "est"))
    for r in rolls:
        r.setflags(write=False)
    return frame_metrics(case["ref"], case["est"], case["n_frames"], **params(case)), rolls


def reference(case):
    """-> (frame_metrics of the case: a FrameMetricCounts, (piano_roll of ref, piano_roll of est)), computed once"""
    return _reference(case["id"])
