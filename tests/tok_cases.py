"""Cases of the tokeniser tests, shared by tests/test_tok_cpu.py (the host path and the plain-Python model of the kernels) and tests/test_tok.py
(the kernels).  The reference of every case is the host path, TaskManager.notes_to_tokens, computed once per case.

  special_cases()   hand-written notes, one case per rule that the issue lists (zero notes, one note, a note over all segments, an offset on a
                    segment start, onset and offset in one step, a note touching its successor, duplicates, drums at equal times, programs
                    128 / 129, programs 96-127 with 13 channels, a gap longer than max_shift_steps, a row of exactly L tokens);
  grid_cases()      seeded random notes that meet the round-trip preconditions (on the 10 ms grid of their segment, no overlap per key, no
                    duplicate drum hit), for 1 and 13 channels, regular and irregular start times;
  matrix_case()     seeded random notes at arbitrary f64 times plus the special notes, thinned until every row fits L: one per combination
                    of n, K, L and max_shift_steps of the GPU comparison."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

from yourmt3_amd.task_manager import DRUM_NOTE_SEC, DRUM_PROGRAM, MC13_GROUPS, Note, TaskManager

SEED = 20261018
TASK_OF_K = {1: "mt3_full_plus", 13: "mc13_full_plus_256"}


@lru_cache(maxsize=None)
def task_manager(task: str, max_shift_steps: int = 206) -> TaskManager:
    return TaskManager(task, max_shift_steps=max_shift_steps)


def regular(n: int) -> List[float]:
    return [i * 8191 / 16000 for i in range(n)]


def drum(t: float, pitch: int) -> Note:
    return Note(t, t + DRUM_NOTE_SEC, True, DRUM_PROGRAM, pitch)


def special_notes(starts: List[float], end_sec: float) -> Dict[str, List[Note]]:
    """the issue's cases as notes over `starts` (at least one segment); times on the grid unless the case is about leaving it"""
    s0, last = starts[0], starts[-1]
    mid = starts[len(starts) // 2]
    out = {
        "zero_notes": [],
        "one_note": [Note(s0 + 0.03, s0 + 0.21, False, 0, 60)],
        "spans_all_segments": [Note(s0 + 0.05, end_sec, False, 40, 55)],
        "offset_on_segment_start": [Note(s0 + 0.1, mid if mid > s0 else end_sec, False, 24, 52)],
        "onset_and_offset_in_one_step": [Note(s0 + 0.100, s0 + 0.102, False, 0, 64), Note(last + 0.2, last + 0.2, False, 1, 65)],
        "touches_its_successor": [Note(s0 + 0.02, s0 + 0.12, False, 0, 48), Note(s0 + 0.12, s0 + 0.3, False, 0, 48)],
        "duplicate_notes_and_ties": [Note(s0 + 0.07, end_sec, False, 32, 40)] * 3 + [Note(s0 + 0.08, end_sec, False, 32, 40)],
        "drums_at_equal_times": [drum(s0 + 0.11, 36), drum(s0 + 0.11, 42), drum(s0 + 0.11, 36), drum(last + 0.01, 38)],
        "programs_128_and_129": [drum(s0 + 0.04, 35), Note(s0 + 0.04, s0 + 0.09, False, 128, 50), Note(s0 + 0.05, end_sec, False, 129, 62)],
        "programs_96_to_127": [Note(s0 + 0.01 * (p - 95), s0 + 0.01 * (p - 94), False, p, 30 + (p % 50)) for p in (96, 100, 111, 127)],
    }
    return out


def fits(tm: TaskManager, notes, starts, end_sec, L) -> bool:
    try:
        tm.notes_to_tokens(notes, starts, end_sec, max_len=L)
        return True
    except ValueError:
        return False


@lru_cache(maxsize=None)
def special_cases() -> Tuple[dict, ...]:
    out = []
    for K in (1, 13):
        for ms in (7, 206):
            for n in (1, 3):
                starts = regular(n)
                end_sec = starts[-1] + 0.4
                for name, notes in special_notes(starts, end_sec).items():
                    out.append(dict(id=f"{name}-K{K}-ms{ms}-n{n}", name=name, task=TASK_OF_K[K], ms=ms, notes=notes, starts=starts, end_sec=end_sec, L=64))
            # a gap longer than max_shift_steps: one segment of 3 s, events 2.5 s apart (250 steps > 206 > 7)
            starts = [0.25, 3.25, 3.75]
            out.append(dict(id=f"gap_longer_than_max_shift-K{K}-ms{ms}", name="gap_longer_than_max_shift", task=TASK_OF_K[K], ms=ms,
                            notes=[Note(0.26, 0.30, False, 0, 60), Note(2.80, 3.30, False, 0, 62), drum(2.76, 40)], starts=starts, end_sec=4.0, L=64))
        # a row of exactly L = 8 tokens: TIE, velocity, program, pitch, shift, pitch, pitch, EOS
        notes = [Note(0.0, 9.0, False, 0, 60), Note(0.05, 9.0, False, 0, 62), Note(0.05, 9.0, False, 0, 64)]
        out.append(dict(id=f"row_of_exactly_L-K{K}", name="row_of_exactly_L", task=TASK_OF_K[K], ms=206, notes=notes, starts=[0.0], end_sec=0.4, L=8))
    return tuple(out)


def grid_point(starts, end_sec, rng) -> Tuple[float, int]:
    """a time on the 10 ms grid of the segment it falls in, below end_sec -> (time, segment)"""
    while True:
        s = int(rng.integers(0, len(starts)))
        nxt = starts[s + 1] if s + 1 < len(starts) else end_sec
        k = int(rng.integers(0, max(1, int((nxt - starts[s]) * 100) + 1)))
        t = starts[s] + k / 100
        if t < nxt:
            return t, s


def grid_notes(rng, tm: TaskManager, starts, end_sec, n_keys: int, per_key: int) -> List[Note]:
    """notes that meet the round-trip preconditions"""
    K = tm.num_decoding_channels
    progs = [0, 1, 24, 40, 100, 129] if K == 1 else [g[1][0] for g in MC13_GROUPS[:12]] + [MC13_GROUPS[5][1][3]]
    notes, keys, hits = [], set(), set()
    while len(keys) < n_keys:
        keys.add((int(rng.choice(progs)), int(rng.integers(30, 90))))
    for prog, pitch in sorted(keys):
        pts = sorted({grid_point(starts, end_sec, rng)[0] for _ in range(2 * per_key)})
        i = 0
        while i < len(pts):
            on = pts[i]
            r = rng.random()
            if i + 1 < len(pts) and r < 0.8:
                off = pts[i + 1]
                i += 1 if rng.random() < 0.35 else 2                    # (i + 1: the next note of the key touches this one)
            else:
                off, i = end_sec, len(pts)                              # sounding to the end of the file
            notes.append(Note(on, off, False, prog, pitch))
    for _ in range(n_keys):
        t, _ = grid_point(starts, end_sec, rng)
        pitch = int(rng.choice([35, 36, 38, 42]))
        if (t, pitch) not in hits:
            hits.add((t, pitch))
            notes.append(drum(t, pitch))
    # two notes that start or end exactly on a segment start
    if len(starts) > 1:
        notes.append(Note(starts[0] + 0.01, starts[1], False, progs[0], 100))
        notes.append(Note(starts[1], starts[-1], False, progs[0], 101) if len(starts) > 2 else Note(starts[1], end_sec, False, progs[0], 101))
    order = rng.permutation(len(notes))
    return [notes[i] for i in order]


@lru_cache(maxsize=None)
def grid_cases() -> Tuple[dict, ...]:
    out = []
    i = 0
    for K in (1, 13):
        for ms in (7, 206):
            for n in (1, 2, 5):
                for irregular in (False, True):
                    rng = np.random.default_rng([SEED, i])
                    i += 1
                    tm = task_manager(TASK_OF_K[K], ms)
                    starts = [float(v) for v in np.round(np.cumsum(rng.uniform(0.3, 3.0, n)), 3)] if irregular else regular(n)
                    end_sec = starts[-1] + (0.37 if irregular else 0.4)
                    notes = grid_notes(rng, tm, starts, end_sec, n_keys=int(rng.integers(1, 9)), per_key=int(rng.integers(1, 4)))
                    out.append(dict(id=f"grid-K{K}-ms{ms}-n{n}-{'irregular' if irregular else 'regular'}", name="grid", task=TASK_OF_K[K], ms=ms,
                                    notes=notes, starts=starts, end_sec=end_sec, L=1024 if ms == 7 else 256))
    return tuple(out)


MATRIX = [(n, K, L, ms) for n in (1, 2, 5) for K in (1, 13) for L in (8, 64, 65, 256, 1024) for ms in (7, 206)]


@lru_cache(maxsize=None)
def matrix_case(n: int, K: int, L: int, ms: int) -> dict:
    """random notes at arbitrary f64 times (out of range ones included) plus the special notes, thinned until every row fits L"""
    rng = np.random.default_rng([SEED, n, K, L, ms])
    tm = task_manager(TASK_OF_K[K], ms)
    starts = regular(n) if (n + L) % 2 else [float(v) for v in np.cumsum(rng.uniform(0.2, 2.5, n)) - 0.1]
    end_sec = starts[-1] + 0.45
    progs = [0, 1, 24, 40, 100, 127, 128, 129] if K == 1 else [g[1][0] for g in MC13_GROUPS] + [96, 127]
    notes: List[Note] = []
    for _ in range(max(2, L // 3) * n):
        on = float(rng.uniform(starts[0] - 0.2, end_sec + 0.2))
        if rng.random() < 0.5:
            on = round(on, 2)
        r = rng.random()
        off = on + float(rng.exponential(0.3)) if r < 0.7 else (on if r < 0.75 else float(rng.choice(starts)) if r < 0.85 else end_sec + (r - 0.9))
        prog = int(rng.choice(progs))
        if prog == DRUM_PROGRAM and rng.random() < 0.8:
            notes.append(drum(on, int(rng.integers(35, 50))))
        else:
            notes.append(Note(on, off, False, prog, int(rng.integers(40, 52))))
    for extra in special_notes(starts, end_sec).values():
        notes += extra
    notes = [notes[i] for i in rng.permutation(len(notes))]
    if L <= 65:                                                         # few notes: keep every one that still fits
        kept: List[Note] = []
        for nt in notes:
            if fits(tm, kept + [nt], starts, end_sec, L):
                kept.append(nt)
        notes = kept
    while not fits(tm, notes, starts, end_sec, L):
        notes = notes[:len(notes) * 3 // 4]
    return dict(id=f"matrix-n{n}-K{K}-L{L}-ms{ms}", name="matrix", task=TASK_OF_K[K], ms=ms, notes=notes, starts=starts, end_sec=end_sec, L=L)


_REF: Dict[str, tuple] = {}


def reference(case) -> Tuple[np.ndarray, np.ndarray]:
    """the host path -> (tokens (n, K, L), lengths (n, K)); computed once per case"""
    if case["id"] not in _REF:
        tm = task_manager(case["task"], case["ms"])
        _REF[case["id"]] = tm.notes_to_tokens(case["notes"], case["starts"], case["end_sec"], max_len=case["L"])
    return _REF[case["id"]]
