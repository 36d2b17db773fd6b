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
whatever matching attains it."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .task_manager import DRUM_PROGRAM, NOTE_RECORD, Note

PITCHES = 128
ONSET, OFFSET = 0, 1
TP, N_REF, N_EST = 0, 1, 2


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
