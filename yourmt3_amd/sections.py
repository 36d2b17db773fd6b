"""Sections over note records and tracked beats: where the song's form changes, which sections return, rehearsal marks for the MIDI file
(include/ymt3.h, sections).

The chord tracker (yourmt3_amd/chords.py) gives every beat a chord; this module gives the file its form: section boundaries from a
checkerboard novelty over the beats' self-similarity, and a letter per section from comparing sections beat by beat along their diagonal.
The rules below are this repository's own and UNVERIFIED against any package.  `track_sections` is their host specification: numpy,
integers throughout.  `SectionTracker` is the device object (YourMT3.compile_section_tracker; yourmt3_amd/csrc/sections.hip), which
equals it bit for bit.  tests/section_model.py states the same rules as plain loops.

The rules.  Every division of integers is a floor division.  Inputs: the records, the beats b[0 .. K) in frames, ascending
(beats.track_beats), optionally the bar tracker's metre (256 m + k per beat), and n_frames.  w = context, L = kernel_beats, m = min_len,
M = max_sections.

  chroma      c[i][pc] is the bars' and the chords': a counted pitched record's span, clipped to the frames, adds the frames it shares with
              slot i to c[i][pitch mod 12].  n[i][pc] = c[i][pc] 1024 / max(sum of c[i], 1) (64 bits); empty[i] = (sum of c[i] = 0).
  context     f[i][pc] = sum over d < w of n[min(i + d, K - 1)][pc]: the sum of f[i] is at most 1024 w <= 16384.
  similarity  D(i, j) = sum over pc of |f[i][pc] - f[j][pc]| <= 2048 w <= 32768; S(i, j) = 2048 w - D(i, j) >= 0.
  novelty     L_i = min(L, i, K - i), t[u] = L - u;
              nov[i] = sum over u, v < L_i of t[u] t[v] (S(i-1-u, i-1-v) + S(i+u, i+v) - S(i-1-u, i+v) - S(i+u, i-1-v)): signed, 64 bits,
              nov[0] = 0.  The four quadrants are cut to the same size at the ends; nothing is zero-padded.  |nov| < 2^41.
  boundaries  the candidates C: every i in [1, K), with a metre only those with metre[i] & 255 = 0.  top = the largest nov among C (0 if
              C is empty).  i in C is a peak if nov[i] > 0, peak_div nov[i] >= top, and no j in C with 0 < |j - i| <= m has the larger key
              (nov[j], -j).  More than M - 1 peaks: the M - 1 with the largest key (nov, -i) are kept.  The section starts are beat 0 and
              the kept peaks in time order; section s is [a_s, a_{s+1}), a_n = K.
  labels      a section is silent if all its beats are empty: label 255, and it neither takes nor gives a letter.  For two others,
              m_st = min(len_s, len_t), d(s, t) = (sum over k < m_st of D(a_s + k, a_t + k)) / m_st; they are the same if
              len_num m_st >= max(len_s, len_t) and d(s, t) <= same_dist.  In time order, s takes the label of the earliest earlier
              non-silent t that is the same as it, else the next unused label from 0.
  outputs     section[i] = 65536 start + 256 s + label for i < K (start = 1 on a section's first beat); novelty[i] = nov[i] (int64);
              result int64 (8,): sections, distinct letters, top, skipped records, peaks before the cap, silent sections, 0, 0.
              With K < 2: no section, no novelty, result = (0, 0, 0, skipped, 0, 0, 0, 0).

The comparison runs along the diagonal: the same chords in another order are another section.  Transposed repeats and functional names
("verse", "chorus") are out of scope."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np

from .bars import (MAX_BEATS, MAX_FRAMES, MAX_NOTES, MAX_PROGRAMS, _records, _to_device, check_inputs, check_shared,  # noqa: F401
                   check_sizes, pitched_spans, run_on_beats, share_spans, slot_edges)  # (the sizes and the slot rule are the bars')
from .beats import TICKS_PER_BEAT, lead_beats, with_defaults
from .model import _Owned
from .task_manager import DRUM_PROGRAM

SILENT = 255
DEFAULTS = dict(frames_per_second=100.0, near_div=4, context=1, kernel_beats=4, min_len=8, peak_div=2, same_dist=512, len_num=2,
                max_sections=32, n_programs=DRUM_PROGRAM + 2, drum_program=DRUM_PROGRAM)
_RANGES = (("near_div", 2, 64), ("context", 1, 16), ("kernel_beats", 2, 64), ("min_len", 1, 256), ("peak_div", 1, 1024),
           ("same_dist", 0, 32768), ("len_num", 1, 16), ("max_sections", 1, 64))
_INTS = ("near_div", "n_programs", "drum_program", "context", "kernel_beats", "min_len", "peak_div", "same_dist", "len_num", "max_sections")


def check_params(**params) -> dict:
    """the parameters with their defaults, refused (ValueError naming the parameter) outside what the C ABI accepts"""
    return check_shared(params, DEFAULTS, _RANGES, "section")


def section_features(notes, beats, n_frames: int, p: dict) -> Tuple[np.ndarray, int]:
    """-> (c int64 (K, 12), the number of skipped records); K >= 2"""
    from .metrics import classify
    rec = _records(notes)
    _, e = slot_edges(np.asarray(beats, np.int64), int(p["near_div"]))
    counted, _, drum = classify(rec, int(p["n_programs"]), int(p["drum_program"]))
    return share_spans(*pitched_spans(rec[counted], drum[counted], n_frames, float(p["frames_per_second"])), e), int((~counted).sum())


def context_features(c: np.ndarray, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (f int64 (K, 12), empty bool (K,))"""
    total = c.sum(1)
    n = c * 1024 // np.maximum(total, 1)[:, None]
    K = c.shape[0]
    f = np.zeros_like(n)
    for d in range(int(w)):
        f += n[np.minimum(np.arange(K) + d, K - 1)]
    return f, total == 0


def novelty_curve(f: np.ndarray, w: int, L: int) -> np.ndarray:
    """-> nov int64 (K,): with g = (t[L_i - 1] .. t[0], -t[0] .. -t[L_i - 1]) over the rows [i - L_i, i + L_i), nov[i] = g S g"""
    K = f.shape[0]
    nov = np.zeros(K, np.int64)
    t = int(L) - np.arange(int(L), dtype=np.int64)
    for i in range(1, K):
        n = min(int(L), i, K - i)
        rows = f[i - n:i + n]
        S = 2048 * int(w) - np.abs(rows[:, None, :] - rows[None, :, :]).sum(2)
        g = np.concatenate([t[:n][::-1], -t[:n]])
        nov[i] = int(g @ S @ g)
    return nov


def pick_boundaries(nov: np.ndarray, metre, p: dict) -> Tuple[List[int], int, int]:
    """-> (the kept peaks ascending, top, the number of peaks before the cap)"""
    K, m = nov.size, int(p["min_len"])
    cand = np.zeros(K, bool)
    cand[1:] = True
    if metre is not None:
        cand &= (np.asarray(metre[:K], np.int64) & 255) == 0
    idx = np.flatnonzero(cand)
    if idx.size == 0:
        return [], 0, 0
    top = int(nov[idx].max())
    peaks = []
    for i in idx.tolist():
        v = int(nov[i])
        if v <= 0 or int(p["peak_div"]) * v < top:
            continue
        near = idx[(np.abs(idx - i) <= m) & (idx != i)]
        if any(int(nov[j]) > v or (int(nov[j]) == v and j < i) for j in near.tolist()):
            continue
        peaks.append(i)
    kept = sorted(sorted(peaks, key=lambda i: (-int(nov[i]), i))[:int(p["max_sections"]) - 1])
    return kept, top, len(peaks)


def label_sections(f: np.ndarray, empty: np.ndarray, starts: List[int], p: dict) -> Tuple[List[int], int, int]:
    """-> (the label of every section, the number of letters, the number of silent sections)"""
    K = f.shape[0]
    ends = starts[1:] + [K]
    silent = [bool(empty[a:e].all()) for a, e in zip(starts, ends)]
    labels: List[int] = []
    letters = 0
    for s, (a, e) in enumerate(zip(starts, ends)):
        if silent[s]:
            labels.append(SILENT)
            continue
        found = None
        for t in range(s):
            if silent[t]:
                continue
            ls, lt = e - a, ends[t] - starts[t]
            n = min(ls, lt)
            if int(p["len_num"]) * n < max(ls, lt):
                continue
            if int(np.abs(f[a:a + n] - f[starts[t]:starts[t] + n]).sum()) // n <= int(p["same_dist"]):
                found = labels[t]
                break
        if found is None:
            found, letters = letters, letters + 1
        labels.append(found)
    return labels, letters, sum(silent)


def track_sections(notes, beats, n_frames: int, metre=None, **params) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host specification -> (section int32 (K,): 65536 start + 256 s + label of every beat, novelty int64 (K,), result int64 (8,):
    sections, letters, top, skipped records, peaks before the cap, silent sections, 0, 0).  `notes`: a list of Note or a NOTE_RECORD
    array, in any order; `beats`: the beats' frames, ascending (beats.track_beats); `metre`: bars.track_bars' metre of the same beats, or
    None; `params`: DEFAULTS' keys."""
    p = check_params(**params)
    rec, b, skipped = check_inputs(notes, beats, n_frames, p, metre)
    if b.size < 2:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.array([0, 0, 0, skipped, 0, 0, 0, 0], np.int64)
    c, skipped = section_features(rec, b, int(n_frames), p)
    f, empty = context_features(c, int(p["context"]))
    nov = novelty_curve(f, int(p["context"]), int(p["kernel_beats"]))
    kept, top, n_peaks = pick_boundaries(nov, metre, p)
    starts = [0] + kept
    labels, letters, n_silent = label_sections(f, empty, starts, p)
    section = np.zeros(b.size, np.int64)
    for s, a in enumerate(starts):
        section[a:] = 256 * s + labels[s]
        section[a] += 65536
    return section.astype(np.int32), nov, np.array([len(starts), letters, top, skipped, n_peaks, n_silent, 0, 0], np.int64)


def section_segments(section, beats) -> List[Tuple[int, int, int]]:
    """-> [(first beat, end beat (exclusive), label)] of every section"""
    v = [int(x) for x in np.asarray(section).tolist()]
    if len(v) > len(beats):
        raise ValueError(f"{len(v)} section entries for {len(beats)} beats")
    out: List[List[int]] = []
    for i, x in enumerate(v):
        if x >> 16 or not out:
            out.append([i, i + 1, x & 255])
        else:
            out[-1][1] = i + 1
    return [tuple(r) for r in out]


def section_names(label: int) -> str:
    """0 -> "A" .. 25 -> "Z", 26 -> "A2" .. 51 -> "Z2", 52 -> "A3"; 255 -> "N" (a silent section)"""
    label = int(label)
    if label == SILENT:
        return "N"
    if not 0 <= label < SILENT:
        raise ValueError(f"label={label} outside [0, {SILENT}]")
    return chr(ord("A") + label % 26) + (str(label // 26 + 1) if label >= 26 else "")


def _edge_sec(beats, i: int, fps: float) -> float:
    """the time of beat i; of one beat after the last for i = K"""
    b = [int(x) for x in beats]
    return (b[i] if i < len(b) else b[-1] + (b[-1] - b[-2] if len(b) > 1 else 0)) / fps


def section_lab(segments, beats, fps: float = 100.0) -> str:
    """the text of a .lab file: one line `start_sec end_sec name` per section, silent ones as N"""
    return "".join(f"{_edge_sec(beats, s, fps):.3f} {_edge_sec(beats, e, fps):.3f} {section_names(label)}\n" for s, e, label in segments)


def section_markers(segments, beats) -> List[Tuple[int, str]]:
    """-> [(tick, "[A]")] for midi's writers on the beats: every non-silent section's name in brackets at the tick of its first beat"""
    if len(beats) < 2:
        return []
    n0 = lead_beats(beats)
    return [((n0 + s) * TICKS_PER_BEAT, f"[{section_names(label)}]") for s, _, label in segments if label != SILENT]


def merge_markers(section_marks, other_marks) -> List[Tuple[int, str]]:
    """both lists in tick order, a section's mark before another mark of the same tick"""
    tagged = [(tick, 0, j, text) for j, (tick, text) in enumerate(section_marks)] + [(tick, 1, j, text) for j, (tick, text) in enumerate(other_marks)]
    return [(tick, text) for tick, _, _, text in sorted(tagged)]


def section_summary(section, result, beats, frames_per_second: float) -> dict:
    """what transcribe(sections=True) and estimate_sections add to a result: sections ([(start_sec, end_sec, name)]) and section_labels
    (every beat's label, 255 in a silent section)"""
    fps = float(frames_per_second)
    return {"sections": [(_edge_sec(beats, s, fps), _edge_sec(beats, e, fps), section_names(label)) for s, e, label in section_segments(section, beats)],
            "section_labels": [int(x) & 255 for x in np.asarray(section).tolist()]}


class SectionTracker(_Owned):
    """The device section tracker of one model (YourMT3.compile_section_tracker; include/ymt3.h, sections): the parameters and scratch for
    `max_beats` beats on the device; a call takes at most `max_notes` records.  `params`: DEFAULTS' keys, checked by the C ABI.  Freed by
    close(), by leaving a `with` block, or by the model's close()."""
    _destroy, _noun = "ymt3_sections_destroy", "section tracker"

    def __init__(self, model, max_beats: int, max_notes: int, **params):
        from . import _lib
        self.params = p = with_defaults(params, DEFAULTS, "section")
        self.max_beats, self.max_notes = int(max_beats), int(max_notes)
        self._own(model)
        c = _lib.SectionParams(float(p["frames_per_second"]), *(int(p[k]) for k in _INTS))
        _lib.check(self._lib.ymt3_sections_create(model._handle, ctypes.byref(c), self.max_beats, self.max_notes, ctypes.byref(self._c)))

    def track(self, beats, beat_result, metre, records, n_frames: int, count=None, novelty: bool = True):
        """`beats`, `beat_result`: what BeatTracker.track returned, device tensors (the number of beats is read from `beat_result` on the
        device); `metre`: what BarTracker.track returned, or None; `records`, `count` as BeatTracker.track.  -> (section int32
        (max_beats,), only the first n_beats written; result int64 (8,); novelty int64 (max_beats,) or None without `novelty`): device
        tensors.  Asynchronous: nothing is copied back."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        section = torch.zeros(self.max_beats, device=model.device, dtype=torch.int32)
        nov = torch.zeros(self.max_beats, device=model.device, dtype=torch.int64) if novelty else None
        result = torch.zeros(8, device=model.device, dtype=torch.int64)
        _lib.check(self._lib.ymt3_track_sections(model._handle, self.ptr, _ptr(beats), _ptr(beat_result), _ptr(metre), _ptr(rec) if n else None, n,
                                                 _ptr(cnt), int(n_frames), _ptr(section), self.max_beats, _ptr(nov), _ptr(result), model._stream()))
        return section, result, nov

    def run(self, beats, records, n_frames: int, metre=None, count=None):
        """`beats`: the beats' frames, `metre`: their metre or None (sequences or int32 tensors, uploaded if on the host), all of them
        live.  track(), then the sections and the result in run_on_beats' copy and the novelty in a second one -> (section int32
        (n_beats,), novelty int64 (n_beats,), result int64 (8,)) as numpy arrays"""
        kept = []

        def track(b, beat_result, k):
            m = None
            if metre is not None and k >= 2:
                m = _to_device(b.device, metre)
                if int(m.numel()) < k:
                    raise ValueError(f"{int(m.numel())} metre entries for {k} beats")
            section, result, nov = self.track(b, beat_result, m, records, n_frames, count)
            kept.append(nov)
            return section, result

        section, result = run_on_beats(self, beats, track)
        return section, kept[0][:section.size].cpu().numpy().copy(), result


def estimate_sections(model, notes_or_mid_path, end_sec: Optional[float] = None, divisions: int = 0, output_path: Optional[str] = None,
                      lab_path: Optional[str] = None, beat_params: Optional[dict] = None, bar_params: Optional[dict] = None, **params) -> dict:
    """Find the beats, the bars, the key and the sections of notes that have none: `notes_or_mid_path` (a list of Note, or the path of a
    flat .mid file) tracked on the device (BeatTracker, BarTracker, then SectionTracker with the bars' metre; the rules: this module's
    docstring).  `end_sec`, `divisions`, `beat_params` as estimate_bars; `bar_params`: bars.DEFAULTS' keys; `params`: DEFAULTS' keys.  ->
    estimate_bars' dict plus {"sections", "section_labels", "section" (int32 (n_beats,)), "novelty", "lab" (the text of a .lab file)},
    "midi" being the bytes of the file on the bars with one marker per section; with `output_path` / `lab_path` the bytes and the text
    are written there too."""
    from .tracking import beats_fps, estimate
    out, tracked = estimate(model, notes_or_mid_path, end_sec, divisions, output_path, beat_params, dict(bar_params or {}), None, params)
    out.update(metre=tracked["metre"], section=tracked["section"], novelty=tracked["novelty"],
               lab=section_lab(section_segments(tracked["section"], tracked["beats"]), tracked["beats"], beats_fps(beat_params)))
    if lab_path is not None:
        with open(lab_path, "w") as f:
            f.write(out["lab"])
    return out
