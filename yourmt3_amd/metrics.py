"""Note-level transcription metrics: onset, onset+offset and drum F1 of an estimate against a reference, plain numpy on the host.

This file is the SPECIFICATION of the device path (include/ymt3.h, note metrics; yourmt3_amd/csrc/metrics.hip), which reproduces its
integers exactly.  The rules are this repository's own.  They are shaped after the widely used note-transcription metric (an onset within
50 ms; an offset within max(50 ms, 20 % of the reference's duration); one-to-one matching), written from memory: that package is not
available here (UNVERIFIED against it, as SURVEY.md section 9 marks its recollections), so nothing below claims to equal its numbers.

Counted records.  A record counts if its onset is not NaN, its pitch lies in [0, 128), its effective program p lies in [0, n_programs)
(p = drum_program if is_drum != 0, else program: the tokeniser's rule) and, if it is pitched, its offset is not NaN.  A record whose
effective program is drum_program is a DRUM note whatever is_drum says (the detokeniser reads a pitch under the drum program as a drum
hit); every other counted record is PITCHED.  The other records are skipped: tallied in skipped[2] (ref, est), in no other number.

Distance.  d(a, b) = rint(|a - b| * 1e4) / 1e4 in f64: that subtract, multiply, round-half-even and divide, nothing contracted.  Times are
start + step / 100, and |1.05 - 1.00| is 0.050000000000000044 in f64: with the rule, grid distances of 50 ms hit and 60 ms miss, and
1.05004 hits while 1.05006 misses.

Hits, for reference i and estimate j of one key.  onset: d(on_i, on_j) <= onset_tol.  offset: the onset hit, and d(off_i, off_j) <=
max(offset_min_tol, offset_ratio * (off_i - on_i)), the tolerance not rounded (a reference whose offset lies before its onset gets the
minimum).  Drum notes never look at offsets: their offset metric equals their onset metric.

Rows.  counts[n_programs + 1][2][3] int32: row x metric (0 onset, 1 onset+offset) x (TP, n_ref, n_est).  Row p < n_programs is
instrument-aware: the notes of effective program p, matched only under the same pitch.  Row n_programs is instrument-agnostic: all pitched
notes, keyed by pitch alone; drums have only their own row.  TP is the size of a MAXIMUM matching of the hit graph, which is unique
whatever matching attains it.

FRAME METRICS AND THE PIANO ROLL (piano_roll, frame_metrics below; the device path: include/ymt3.h, piano roll and frame metrics;
yourmt3_amd/csrc/roll.hip).  How much of the sounding (frame, pitch) area is right.  These rules too are this repository's own, shaped after
the usual multi-pitch frame metric (precision, recall, accuracy and the substitution / miss / false-alarm error of frame-wise pitch
sets), written from memory: UNVERIFIED against the package they resemble, which is not available here.

Counted records.  Exactly the rule above (classify): skipped[2] keeps its meaning, and a drum record counts even with a NaN offset.

Frame of a time.  F(t) = rint(t * frames_per_second) in f64: that one multiply, round half to even -- the tokeniser's step rule.  At 100
frames per second a time on the 10 ms grid lands on its own step despite f64 noise: 0.57 * 100 = 56.99999999999999 -> 57 and 1.1 * 100 = 110.00000000000001 -> 110.

Cells of a note.  A counted pitched note sounds in frames [F(on), max(F(off), F(on) + 1)) clipped to [0, n_frames): it always shows in its
onset frame, even when it is shorter than a frame or its offset lies before its onset.  A counted drum note sounds in [F(on), F(on) + 1),
clipped; its offset is not read.  The clipping is done in f64 before any conversion to an integer, so +-inf and huge times are defined:
an onset of +inf gives no cell, an onset of -inf starts at frame 0, an offset of +inf ends at n_frames.

Rows.  Those of the note metrics: row p < n_programs holds the notes of effective program p, row n_programs all pitched notes whatever
their program; drums have only their own row.  A cell is a set member, not a count: overlapping or duplicate notes of one (row, pitch)
sound once.  roll[row][frame][pitch] in {0, 1}, shape (n_programs + 1, n_frames, 128).

Frame counts.  For each row and frame, nr and ne are the numbers of sounding pitches of reference and estimate and tp the number sounding
in both.  Per row, summed over frames, six int64: TP = sum tp, N_REF = sum nr, N_EST = sum ne, SUB = sum (min(nr, ne) - tp), MISS = sum
max(0, nr - ne), FA = sum max(0, ne - nr).  The flat result is counts[n_programs + 1][6] then skipped[2], all int64.  Derived (0 where a
denominator is 0): precision TP / N_EST, recall TP / N_REF, F, accuracy TP / (N_REF + N_EST - TP), and the error rates SUB / N_REF,
MISS / N_REF, FA / N_REF and their sum."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .task_manager import DRUM_PROGRAM, NOTE_RECORD, Note

PITCHES = 128
ONSET, OFFSET = 0, 1
TP, N_REF, N_EST = 0, 1, 2
SUB, MISS, FA = 3, 4, 5               # frame counts only: a row of FrameMetricCounts is TP, N_REF, N_EST, SUB, MISS, FA


def to_records(notes) -> np.ndarray:
    """a list of Note (or an array of NOTE_RECORD, returned as it is) -> NOTE_RECORD array; a Note's is_drum and program are kept as given"""
    if isinstance(notes, np.ndarray):
        if notes.dtype != NOTE_RECORD:
            raise ValueError("a note array must have dtype NOTE_RECORD")
        return notes
    rec = np.zeros(len(notes), NOTE_RECORD)
    for i, n in enumerate(notes):
        if not isinstance(n, Note):
            raise ValueError(f"{n!r} is not a Note")
        rec[i] = (n.onset, n.offset, n.program, n.pitch, bool(n.is_drum), float("nan"))
    return rec


def _ratio(num: int, den: int) -> float:
    return num / den if den else 0.0


class NoteMetricCounts:
    """The integers of one comparison and the values derived from them.  `counts`: (n_programs + 1, 2, 3) int32 as laid out above;
    `skipped`: (2,) int32.  flat() is the device layout, counts then skipped: (n_programs + 1) * 6 + 2 integers."""

    def __init__(self, counts, skipped, drum_program: int = DRUM_PROGRAM):
        self.counts = np.asarray(counts, np.int32)
        self.skipped = np.asarray(skipped, np.int32)
        if self.counts.ndim != 3 or self.counts.shape[1:] != (2, 3) or self.counts.shape[0] < 2 or self.skipped.shape != (2,):
            raise ValueError(f"counts {self.counts.shape} / skipped {self.skipped.shape} are not (n_programs + 1, 2, 3) / (2,)")
        self.n_programs = self.counts.shape[0] - 1
        self.drum_program = int(drum_program)

    @classmethod
    def from_flat(cls, flat, n_programs: int, drum_program: int = DRUM_PROGRAM) -> "NoteMetricCounts":
        flat = np.asarray(flat, np.int32).reshape(-1)
        if flat.size != (n_programs + 1) * 6 + 2:
            raise ValueError(f"{flat.size} integers, expected {(n_programs + 1) * 6 + 2}")
        return cls(flat[:-2].reshape(n_programs + 1, 2, 3), flat[-2:], drum_program)

    def flat(self) -> np.ndarray:
        return np.concatenate([self.counts.reshape(-1), self.skipped]).astype(np.int32)

    def _triple(self, row, metric):
        c = self.counts[row, metric].astype(np.int64)
        if c.ndim == 2:
            c = c.sum(0)
        return int(c[TP]), int(c[N_REF]), int(c[N_EST])

    def precision(self, row, metric: int) -> float:
        tp, _, n_est = self._triple(row, metric)
        return _ratio(tp, n_est)

    def recall(self, row, metric: int) -> float:
        tp, n_ref, _ = self._triple(row, metric)
        return _ratio(tp, n_ref)

    def f_measure(self, row, metric: int) -> float:
        """F = 2PR / (P + R) of a row, or of several rows summed (a slice or a list of rows); 0 where a denominator is 0"""
        p, r = self.precision(row, metric), self.recall(row, metric)
        return 2.0 * p * r / (p + r) if p + r else 0.0

    @property
    def onset_f(self) -> float:
        return self.f_measure(self.n_programs, ONSET)

    @property
    def offset_f(self) -> float:
        return self.f_measure(self.n_programs, OFFSET)

    @property
    def drum_onset_f(self) -> float:
        return self.f_measure(self.drum_program, ONSET) if 0 <= self.drum_program < self.n_programs else 0.0

    @property
    def multi_f(self) -> float:
        """onset+offset F over the instrument-aware rows summed (build-defined: drums enter with their onset matches)"""
        return self.f_measure(slice(0, self.n_programs), OFFSET)

    def per_program(self) -> Dict[int, Dict[str, float]]:
        """program -> derived values, for the programs that have a note on either side"""
        out = {}
        for p in range(self.n_programs):
            if self.counts[p, ONSET, N_REF] or self.counts[p, ONSET, N_EST]:
                out[p] = {"onset_p": self.precision(p, ONSET), "onset_r": self.recall(p, ONSET), "onset_f": self.f_measure(p, ONSET),
                          "offset_p": self.precision(p, OFFSET), "offset_r": self.recall(p, OFFSET), "offset_f": self.f_measure(p, OFFSET),
                          "n_ref": int(self.counts[p, ONSET, N_REF]), "n_est": int(self.counts[p, ONSET, N_EST])}
        return out

    def summary(self) -> Dict[str, object]:
        a = self.n_programs
        return {"onset_f": self.onset_f, "onset_p": self.precision(a, ONSET), "onset_r": self.recall(a, ONSET),
                "offset_f": self.offset_f, "offset_p": self.precision(a, OFFSET), "offset_r": self.recall(a, OFFSET),
                "drum_onset_f": self.drum_onset_f, "multi_f": self.multi_f, "per_program": self.per_program(),
                "skipped": (int(self.skipped[0]), int(self.skipped[1])), "counts": self.counts}

    def __eq__(self, other):
        return isinstance(other, NoteMetricCounts) and np.array_equal(self.flat(), other.flat()) and self.drum_program == other.drum_program

    def __repr__(self):
        return f"NoteMetricCounts(onset_f={self.onset_f:.4f}, offset_f={self.offset_f:.4f}, drum_onset_f={self.drum_onset_f:.4f}, multi_f={self.multi_f:.4f})"


def distance(a, b):
    """d(a, b) of the rules, elementwise in f64"""
    with np.errstate(invalid="ignore"):
        return np.rint(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) * 1e4) / 1e4


def hit_matrices(ref_on, ref_off, est_on, est_off, onset_tol: float, offset_min_tol: float, offset_ratio: float):
    """(n, m) boolean onset hits and onset+offset hits of one key's references and estimates"""
    with np.errstate(invalid="ignore"):
        onset = distance(ref_on[:, None], est_on[None, :]) <= onset_tol
        tol = offset_ratio * (ref_off - ref_on)
        tol = np.where(tol > offset_min_tol, tol, offset_min_tol)
        both = onset & (distance(ref_off[:, None], est_off[None, :]) <= tol[:, None])
    return onset, both


def _augmenting_paths(hits: np.ndarray) -> int:
    """size of a maximum matching of a boolean (n, m) matrix: Kuhn's algorithm, iterative (used where scipy is not importable)"""
    n, m = hits.shape
    adj = [np.flatnonzero(hits[i]).tolist() for i in range(n)]
    match = [-1] * m
    size = 0
    for root in range(n):
        seen = [False] * m
        stack = [[root, 0]]
        while stack:
            u, c = stack[-1]
            if c == len(adj[u]):
                stack.pop()
                continue
            stack[-1][1] = c + 1
            v = adj[u][c]
            if seen[v]:
                continue
            seen[v] = True
            if match[v] < 0:
                for w, cw in stack:
                    match[adj[w][cw - 1]] = w
                size += 1
                break
            stack.append([match[v], 0])
    return size


def max_matching(hits: np.ndarray) -> int:
    """size of a maximum matching of the bipartite graph given as a boolean (n, m) matrix"""
    if not hits.size or not hits.any():
        return 0
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import maximum_bipartite_matching
    except ImportError:
        return _augmenting_paths(hits)
    return int((maximum_bipartite_matching(csr_matrix(hits), perm_type="column") >= 0).sum())


def classify(rec: np.ndarray, n_programs: int, drum_program: int):
    """-> (counted mask, effective program, drum mask) of a NOTE_RECORD array, by the rules above"""
    prog = np.where(rec["is_drum"] != 0, np.int64(drum_program), rec["program"].astype(np.int64))
    drum = prog == drum_program
    counted = ~np.isnan(rec["onset"]) & (rec["pitch"] >= 0) & (rec["pitch"] < PITCHES) & (prog >= 0) & (prog < n_programs)
    counted &= drum | ~np.isnan(rec["offset"])
    return counted, prog, drum


def note_metrics(ref, est, n_programs: int, drum_program: int = DRUM_PROGRAM, onset_tol: float = 0.05, offset_min_tol: float = 0.05,
                 offset_ratio: float = 0.2) -> NoteMetricCounts:
    """Compare the estimate `est` with the reference `ref` (lists of Note, or NOTE_RECORD arrays) by the rules of this module."""
    for name, v in (("onset_tol", onset_tol), ("offset_min_tol", offset_min_tol), ("offset_ratio", offset_ratio)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{name}={v} must be finite and >= 0")
    if n_programs < 1 or not 0 <= drum_program < n_programs:
        raise ValueError(f"n_programs={n_programs} must be >= 1 and drum_program={drum_program} inside [0, n_programs)")
    sides = []
    skipped = np.zeros(2, np.int32)
    for s, notes in enumerate((ref, est)):
        rec = to_records(notes)
        counted, prog, drum = classify(rec, n_programs, drum_program)
        skipped[s] = int((~counted).sum())
        sides.append((rec[counted], prog[counted], drum[counted]))
    counts = np.zeros((n_programs + 1, 2, 3), np.int32)
    tol = (float(onset_tol), float(offset_min_tol), float(offset_ratio))
    for row in range(n_programs + 1):
        sel = [(~drum if row == n_programs else prog == row) for _, prog, drum in sides]
        r, e = sides[0][0][sel[0]], sides[1][0][sel[1]]
        counts[row, :, N_REF], counts[row, :, N_EST] = r.size, e.size
        if not r.size or not e.size:
            continue
        for pitch in np.intersect1d(r["pitch"], e["pitch"]):
            rk, ek = r[r["pitch"] == pitch], e[e["pitch"] == pitch]
            onset, both = hit_matrices(rk["onset"], rk["offset"], ek["onset"], ek["offset"], *tol)
            tp = max_matching(onset)
            counts[row, ONSET, TP] += tp
            counts[row, OFFSET, TP] += tp if row == drum_program else max_matching(both)
    return NoteMetricCounts(counts, skipped, drum_program)


class FrameMetricCounts:
    """The integers of one frame-level comparison and the values derived from them.  `counts`: (n_programs + 1, 6) int64, a row being TP,
    N_REF, N_EST, SUB, MISS, FA; `skipped`: (2,) int64.  flat() is the device layout, counts then skipped: (n_programs + 1) * 6 + 2 integers."""

    def __init__(self, counts, skipped, drum_program: int = DRUM_PROGRAM):
        self.counts = np.asarray(counts, np.int64)
        self.skipped = np.asarray(skipped, np.int64)
        if self.counts.ndim != 2 or self.counts.shape[1] != 6 or self.counts.shape[0] < 2 or self.skipped.shape != (2,):
            raise ValueError(f"counts {self.counts.shape} / skipped {self.skipped.shape} are not (n_programs + 1, 6) / (2,)")
        self.n_programs = self.counts.shape[0] - 1
        self.drum_program = int(drum_program)

    @classmethod
    def from_flat(cls, flat, n_programs: int, drum_program: int = DRUM_PROGRAM) -> "FrameMetricCounts":
        flat = np.asarray(flat, np.int64).reshape(-1)
        if flat.size != (n_programs + 1) * 6 + 2:
            raise ValueError(f"{flat.size} integers, expected {(n_programs + 1) * 6 + 2}")
        return cls(flat[:-2].reshape(n_programs + 1, 6), flat[-2:], drum_program)

    def flat(self) -> np.ndarray:
        return np.concatenate([self.counts.reshape(-1), self.skipped]).astype(np.int64)

    def _six(self, row):
        c = self.counts[row]
        if c.ndim == 2:
            c = c.sum(0)
        return [int(v) for v in c]

    def precision(self, row) -> float:
        c = self._six(row)
        return _ratio(c[TP], c[N_EST])

    def recall(self, row) -> float:
        c = self._six(row)
        return _ratio(c[TP], c[N_REF])

    def f_measure(self, row) -> float:
        """F = 2PR / (P + R) of a row, or of several rows summed (a slice or a list of rows); 0 where a denominator is 0"""
        p, r = self.precision(row), self.recall(row)
        return 2.0 * p * r / (p + r) if p + r else 0.0

    def accuracy(self, row) -> float:
        c = self._six(row)
        return _ratio(c[TP], c[N_REF] + c[N_EST] - c[TP])

    def error(self, row) -> Dict[str, float]:
        """the error rates of a row (or of several rows summed): substitutions, misses and false alarms over N_REF, and their sum"""
        c = self._six(row)
        return {"sub": _ratio(c[SUB], c[N_REF]), "miss": _ratio(c[MISS], c[N_REF]), "fa": _ratio(c[FA], c[N_REF]),
                "total": _ratio(c[SUB] + c[MISS] + c[FA], c[N_REF])}

    @property
    def frame_f(self) -> float:
        return self.f_measure(self.n_programs)

    @property
    def multi_frame_f(self) -> float:
        """frame F over the instrument-aware rows summed (drums enter with their one-frame hits)"""
        return self.f_measure(slice(0, self.n_programs))

    def per_program(self) -> Dict[int, Dict[str, float]]:
        """program -> derived values, for the programs that sound on either side"""
        out = {}
        for p in range(self.n_programs):
            if self.counts[p, N_REF] or self.counts[p, N_EST]:
                out[p] = {"frame_p": self.precision(p), "frame_r": self.recall(p), "frame_f": self.f_measure(p), "frame_acc": self.accuracy(p),
                          "n_ref": int(self.counts[p, N_REF]), "n_est": int(self.counts[p, N_EST])}
        return out

    def summary(self) -> Dict[str, object]:
        a = self.n_programs
        return {"frame_f": self.frame_f, "frame_p": self.precision(a), "frame_r": self.recall(a), "frame_acc": self.accuracy(a),
                "frame_err": self.error(a), "multi_frame_f": self.multi_frame_f, "frame_counts": self.counts}

    def __eq__(self, other):
        return isinstance(other, FrameMetricCounts) and np.array_equal(self.flat(), other.flat()) and self.drum_program == other.drum_program

    def __repr__(self):
        return f"FrameMetricCounts(frame_f={self.frame_f:.4f}, frame_acc={self.accuracy(self.n_programs):.4f}, multi_frame_f={self.multi_frame_f:.4f})"


def frame_of(t, fps: float):
    """F(t) of the rules, elementwise in f64 (not yet an integer: +-inf stay what they are)"""
    with np.errstate(invalid="ignore"):
        return np.rint(np.asarray(t, np.float64) * np.float64(fps))


def _check_frames(n_frames: int, n_programs: int, drum_program: int, frames_per_second: float):
    if not (np.isfinite(frames_per_second) and frames_per_second > 0):
        raise ValueError(f"frames_per_second={frames_per_second} must be finite and > 0")
    if n_frames < 0:
        raise ValueError(f"n_frames={n_frames} must be >= 0")
    if n_programs < 1 or not 0 <= drum_program < n_programs:
        raise ValueError(f"n_programs={n_programs} must be >= 1 and drum_program={drum_program} inside [0, n_programs)")


def _cells(notes, n_frames: int, n_programs: int, drum_program: int, fps: float):
    """-> (the sorted, unique cells of a note set as keys (row * n_frames + frame) * 128 + pitch, the number of skipped records)"""
    rec = to_records(notes)
    counted, prog, drum = classify(rec, n_programs, drum_program)
    rec, prog, drum = rec[counted], prog[counted], drum[counted]
    f0 = frame_of(rec["onset"], fps)
    f1 = np.where(drum, f0 + 1.0, np.maximum(frame_of(np.where(drum, 0.0, rec["offset"]), fps), f0 + 1.0))
    lo, hi = np.maximum(f0, 0.0), np.minimum(f1, np.float64(n_frames))        # the clipping, still in f64
    some = lo < hi
    lo, hi = lo[some].astype(np.int64), hi[some].astype(np.int64)
    prog, drum, pitch = prog[some], drum[some], rec["pitch"][some].astype(np.int64)
    # every note once under its own row, every pitched note once more under the agnostic row
    lo, hi = np.concatenate([lo, lo[~drum]]), np.concatenate([hi, hi[~drum]])
    row = np.concatenate([prog, np.full(int((~drum).sum()), n_programs, np.int64)])
    pitch = np.concatenate([pitch, pitch[~drum]])
    length = hi - lo
    first = np.cumsum(length) - length
    frame = np.repeat(lo - first, length) + np.arange(int(length.sum()), dtype=np.int64)
    keys = (np.repeat(row, length) * n_frames + frame) * PITCHES + np.repeat(pitch, length)
    return np.unique(keys), int((~counted).sum())


def piano_roll(notes, n_frames: int, n_programs: int, drum_program: int = DRUM_PROGRAM, frames_per_second: float = 100.0) -> np.ndarray:
    """The roll of a note set (a list of Note, or a NOTE_RECORD array) by the rules of this module -> (n_programs + 1, n_frames, 128) uint8."""
    _check_frames(n_frames, n_programs, drum_program, frames_per_second)
    keys, _ = _cells(notes, int(n_frames), n_programs, drum_program, float(frames_per_second))
    roll = np.zeros((n_programs + 1) * int(n_frames) * PITCHES, np.uint8)
    roll[keys] = 1
    return roll.reshape(n_programs + 1, int(n_frames), PITCHES)


def frame_metrics(ref, est, n_frames: int, n_programs: int, drum_program: int = DRUM_PROGRAM, frames_per_second: float = 100.0) -> FrameMetricCounts:
    """Compare the estimate `est` with the reference `ref` (lists of Note, or NOTE_RECORD arrays) frame by frame, by the rules of this module."""
    _check_frames(n_frames, n_programs, drum_program, frames_per_second)
    n_frames, rows = int(n_frames), n_programs + 1
    (kr, skipped_r), (ke, skipped_e) = (_cells(s, n_frames, n_programs, drum_program, float(frames_per_second)) for s in (ref, est))
    both = np.intersect1d(kr, ke, assume_unique=True)
    nr, ne, tp = (np.bincount(k // PITCHES, minlength=rows * n_frames).reshape(rows, n_frames) for k in (kr, ke, both))
    counts = np.stack([tp.sum(1), nr.sum(1), ne.sum(1), (np.minimum(nr, ne) - tp).sum(1), np.maximum(0, nr - ne).sum(1),
                       np.maximum(0, ne - nr).sum(1)], 1)
    return FrameMetricCounts(counts, (skipped_r, skipped_e), drum_program)


# ---------------------------------------------------------------- alignment: banded DTW over pitch sets (the rules: DESIGN.md section 20)
# The device path (include/ymt3.h, alignment; yourmt3_amd/csrc/align.hip) reproduces every integer of dtw_align and every byte of
# warp_notes.  Features: per side and frame 256 bits, the instrument-agnostic row of the frame metrics (all pitched counted notes) and
# the drum row, each side at its OWN frame count.  Cost c(i, j) = popc(ref_i XOR est_j), 0 ... 256.  Band: with q = Na - 1, p = Nb - 1,
# m = max(p, q, 1), cell (i, j) is in the band iff |i * p - j * q| <= band_frames * m (int64).  D(0, 0) = c(0, 0); every other in-band
# cell: best = min(D(i-1, j-1), D(i-1, j), D(i, j-1)), a predecessor outside the rectangle or the band being INF = 2^30, D = min(best + c,
# INF), and the cell's step is the FIRST of (diagonal, (i-1, j), (i, j-1)) whose D equals best.  The path follows the steps from (q, p)
# back to (0, 0); warp[i] is the lowest j of the path in row i: warp[0] = 0, and warp[q] <= p, below p when the path ends along row q.
ALIGN_INF = 1 << 30
ALIGN_MAX_FRAMES = 1 << 20
_POPC8 = np.array([bin(v).count("1") for v in range(256)], np.int32)


class Alignment:
    """One alignment: `total` = D(q, p); `path`: (n, 2) int32, the cells (i, j) from (0, 0) to (q, p); `warp`: (Na,) int32, the lowest j of
    the path per i; `skipped`: (2,) int64 (ref, est) records not counted.  flat() is total, path_len, skipped[2], warp[Na], path[n][2] as
    int64; from_flat reads it back."""

    def __init__(self, total, path, warp, skipped):
        self.total = int(total)
        self.path = np.asarray(path, np.int32).reshape(-1, 2)
        self.warp = np.asarray(warp, np.int32).reshape(-1)
        self.skipped = np.asarray(skipped, np.int64)
        if self.skipped.shape != (2,) or self.warp.size < 1:
            raise ValueError(f"warp {self.warp.shape} / skipped {self.skipped.shape} are not (Na >= 1,) / (2,)")

    @property
    def path_len(self) -> int:
        return int(self.path.shape[0])

    def flat(self) -> np.ndarray:
        return np.concatenate([[self.total, self.path_len], self.skipped, self.warp.astype(np.int64), self.path.reshape(-1).astype(np.int64)]).astype(np.int64)

    @classmethod
    def from_flat(cls, flat, n_ref_frames: int) -> "Alignment":
        flat = np.asarray(flat, np.int64).reshape(-1)
        if flat.size < 4 + n_ref_frames or flat.size != 4 + n_ref_frames + 2 * int(flat[1]):
            raise ValueError(f"{flat.size} integers do not hold 4 + {n_ref_frames} + 2 * path_len")
        return cls(flat[0], flat[4 + n_ref_frames:], flat[4:4 + n_ref_frames], flat[2:4])

    def __eq__(self, other):
        return isinstance(other, Alignment) and np.array_equal(self.flat(), other.flat())

    def __repr__(self):
        return f"Alignment(total={self.total}, path_len={self.path_len}, n_ref_frames={self.warp.size})"


def _check_align(n_ref_frames, n_est_frames, n_programs, drum_program, frames_per_second, band_frames):
    if not (np.isfinite(frames_per_second) and frames_per_second > 0):
        raise ValueError(f"frames_per_second={frames_per_second} must be finite and > 0")
    for name, v in (("n_ref_frames", n_ref_frames), ("n_est_frames", n_est_frames)):
        if v < 1 or v > ALIGN_MAX_FRAMES:
            raise ValueError(f"{name}={v} outside [1, {ALIGN_MAX_FRAMES}]")
    if band_frames < 1:
        raise ValueError(f"band_frames={band_frames} must be >= 1")
    if n_programs < 1 or not 0 <= drum_program < n_programs:
        raise ValueError(f"n_programs={n_programs} must be >= 1 and drum_program={drum_program} inside [0, n_programs)")


def align_features(notes, n_frames: int, n_programs: int, drum_program: int = DRUM_PROGRAM, frames_per_second: float = 100.0):
    """-> ((n_frames, 4) uint64: the 256 bits of every frame, agnostic row then drum row, bit `pitch` of each; skipped records)"""
    keys, skipped = _cells(notes, int(n_frames), n_programs, drum_program, float(frames_per_second))
    row, rest = np.divmod(keys, int(n_frames) * PITCHES)
    frame, pitch = np.divmod(rest, PITCHES)
    feat = np.zeros((int(n_frames), 4), np.uint64)
    for r, half in ((n_programs, 0), (drum_program, 2)):
        sel = row == r
        np.bitwise_or.at(feat, (frame[sel], half + pitch[sel] // 64), np.uint64(1) << (pitch[sel] % 64).astype(np.uint64))
    return feat, skipped


def _popc_rows(x: np.ndarray) -> np.ndarray:
    """(n, 4) uint64 -> (n,) int32 set bits"""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).sum(1, dtype=np.int32)
    return _POPC8[np.ascontiguousarray(x).view(np.uint8)].sum(1, dtype=np.int32)


def _diag_range(d: int, p: int, q: int, bm: int):
    """the in-band i of anti-diagonal d = i + j: i * p - (d - i) * q in [-bm, bm], inside the rectangle"""
    lo, hi = max(0, d - p), min(d, q)
    if p + q:
        lo, hi = max(lo, -((bm - d * q) // (p + q))), min(hi, (d * q + bm) // (p + q))
    return lo, hi


def _take(prev, lo: int, n: int) -> np.ndarray:
    """D of a stored anti-diagonal (its first i, its values) at i = lo ... lo + n - 1; INF outside"""
    out = np.full(n, ALIGN_INF, np.int32)
    if prev is not None:
        plo, vals = prev
        a, b = max(lo, plo), min(lo + n, plo + vals.size)
        if a < b:
            out[a - lo:b - lo] = vals[a - plo:b - plo]
    return out


def dtw_align(ref, est, n_ref_frames: int, n_est_frames: int, n_programs: int, drum_program: int = DRUM_PROGRAM, frames_per_second: float = 100.0,
              band_frames: int = 1000) -> Alignment:
    """Align the reference `ref` (n_ref_frames frames) to the estimate `est` (n_est_frames frames) by the rules above, one anti-diagonal
    of the band at a time."""
    _check_align(n_ref_frames, n_est_frames, n_programs, drum_program, frames_per_second, band_frames)
    na, nb = int(n_ref_frames), int(n_est_frames)
    fr, skipped_r = align_features(ref, na, n_programs, drum_program, frames_per_second)
    fe, skipped_e = align_features(est, nb, n_programs, drum_program, frames_per_second)
    q, p = na - 1, nb - 1
    bm = int(band_frames) * max(p, q, 1)
    prev1 = prev2 = None
    steps = []                                                           # per anti-diagonal: (first i, uint8 steps) or None
    for d in range(q + p + 1):
        lo, hi = _diag_range(d, p, q, bm)
        if lo > hi:
            prev2, prev1 = prev1, None
            steps.append(None)
            continue
        n = hi - lo + 1
        i = np.arange(lo, hi + 1)
        cost = _popc_rows(fr[i] ^ fe[d - i])
        diag, up, left = _take(prev2, lo - 1, n), _take(prev1, lo - 1, n), _take(prev1, lo, n)
        best = np.minimum(np.minimum(diag, up), left)
        step = np.where(diag == best, 0, np.where(up == best, 1, 2)).astype(np.uint8)
        if d == 0:
            best = np.zeros(1, np.int32)
        val = np.minimum(best.astype(np.int64) + cost, ALIGN_INF).astype(np.int32)
        prev2, prev1 = prev1, (lo, val)
        steps.append((lo, step))
    total = int(prev1[1][0]) if prev1 is not None else ALIGN_INF
    if total >= ALIGN_INF:
        return Alignment(ALIGN_INF, np.zeros((0, 2), np.int32), np.full(na, -1, np.int32), (skipped_r, skipped_e))
    path = []
    i, j = q, p
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        lo, step = steps[i + j]
        s = int(step[i - lo])
        i, j = i - (s != 2), j - (s != 1)
    path = np.array(path[::-1], np.int32)
    warp = np.zeros(na, np.int32)
    first = np.concatenate([[True], path[1:, 0] != path[:-1, 0]])
    warp[path[first, 0]] = path[first, 1]
    return Alignment(total, path, warp, (skipped_r, skipped_e))


def warp_times(t, warp, frames_per_second: float) -> np.ndarray:
    """W(t) of the rules in f64, elementwise: x = t * fps; k = floor(x) clamped to [0, q]; f = x - k clamped to [0, 1];
    W = (warp[k] + f * (warp[min(k + 1, q)] - warp[k])) / fps.  NaN stays NaN, -inf gives 0, a time at or past the end warp[q] / fps."""
    warp = np.asarray(warp, np.int32).reshape(-1)
    if warp.size < 1:
        raise ValueError("warp must hold at least one frame")
    if not (np.isfinite(frames_per_second) and frames_per_second > 0):
        raise ValueError(f"frames_per_second={frames_per_second} must be finite and > 0")
    fps, q = np.float64(frames_per_second), warp.size - 1
    with np.errstate(invalid="ignore"):
        x = np.asarray(t, np.float64) * fps
        nan = np.isnan(x)
        k = np.minimum(np.maximum(np.floor(np.where(nan, 0.0, x)), 0.0), np.float64(q))
        f = np.minimum(np.maximum(np.where(nan, 0.0, x) - k, 0.0), 1.0)
        ki = k.astype(np.int64)
        a, b = warp[ki].astype(np.float64), warp[np.minimum(ki + 1, q)].astype(np.float64)
        w = (a + f * (b - a)) / fps
    return np.where(nan, np.float64("nan"), w)


def warp_notes(records, warp, frames_per_second: float = 100.0) -> np.ndarray:
    """Carry a note set (a list of Note, or a NOTE_RECORD array) onto the estimate's time axis: W applied to onset and offset of every
    record, everything else copied, nothing filtered -> a new NOTE_RECORD array."""
    out = to_records(records).copy()
    out["onset"] = warp_times(out["onset"], warp, frames_per_second)
    out["offset"] = warp_times(out["offset"], warp, frames_per_second)
    return out
