"""The rules of the piano roll and the frame metrics (include/ymt3.h, piano roll and frame metrics), stated independently of
yourmt3_amd/metrics.py: a plain Python loop over records and frames into sets of (row, frame, pitch), and a loop over rows and frames
for the counts.  It shares no code with the specification it checks; Python floats are f64 and round() rounds half to even."""
import math

import numpy as np


def _frame(t: float, fps: float) -> float:
    x = t * fps
    return x if math.isinf(x) else float(round(x))


def cells_of(rec, n_frames: int, n_programs: int, drum_program: int, fps: float):
    """-> (the set of sounding (row, frame, pitch) of a NOTE_RECORD array, the number of records that do not count)"""
    cells, skipped = set(), 0
    for on, off, program, pitch, is_drum in zip(rec["onset"].tolist(), rec["offset"].tolist(), rec["program"].tolist(), rec["pitch"].tolist(),
                                                rec["is_drum"].tolist()):
        prog = drum_program if is_drum else program
        drum = prog == drum_program
        if math.isnan(on) or not 0 <= pitch < 128 or not 0 <= prog < n_programs or (not drum and math.isnan(off)):
            skipped += 1
            continue
        first = _frame(on, fps)
        end = first + 1.0 if drum else max(_frame(off, fps), first + 1.0)
        first, end = max(first, 0.0), min(end, float(n_frames))
        if not first < end:
            continue
        for frame in range(int(first), int(end)):
            cells.add((prog, frame, pitch))
            if not drum:
                cells.add((n_programs, frame, pitch))
    return cells, skipped


def model_roll(rec, n_frames, n_programs, drum_program, fps) -> np.ndarray:
    roll = np.zeros((n_programs + 1, n_frames, 128), np.uint8)
    for row, frame, pitch in cells_of(rec, n_frames, n_programs, drum_program, fps)[0]:
        roll[row, frame, pitch] = 1
    return roll


def model_counts(ref, est, n_frames, n_programs, drum_program, fps):
    """-> the flat result as a list of Python integers: counts[row][TP, N_REF, N_EST, SUB, MISS, FA], then skipped[2]"""
    (rc, rs), (ec, es) = (cells_of(s, n_frames, n_programs, drum_program, fps) for s in (ref, est))
    sounding = [{}, {}]
    for side, cells in enumerate((rc, ec)):
        for row, frame, pitch in cells:
            sounding[side].setdefault((row, frame), set()).add(pitch)
    counts = [[0] * 6 for _ in range(n_programs + 1)]
    for row, frame in set(sounding[0]) | set(sounding[1]):
        r, e = sounding[0].get((row, frame), set()), sounding[1].get((row, frame), set())
        nr, ne, tp = len(r), len(e), len(r & e)
        for k, v in enumerate((tp, nr, ne, min(nr, ne) - tp, max(0, nr - ne), max(0, ne - nr))):
            counts[row][k] += v
    return [v for row in counts for v in row] + [rs, es]
