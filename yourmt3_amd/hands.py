"""Hands over note records: which hand plays every piano note, from a split point that moves with the music; two staves for the MIDI file
(include/ymt3.h, hands).

Every piano note of a transcription sits in one track, and a notation program opens that as one staff.  This module gives every note of
the piano programs a hand: at every onset slice the keyboard is cut at a split point, the notes below it are the left hand's, and the
split points of the whole piece are one cheapest path.  The rules below are this repository's own and UNVERIFIED against any package.
`split_hands` is their host specification: numpy, integers throughout.  `HandSplitter` is the device object
(YourMT3.compile_hand_splitter; yourmt3_amd/csrc/hands.hip), which equals it bit for bit.  tests/hand_model.py states the same rules as
plain loops.

The rules.  Every division of integers is a floor division.  Inputs: the records, n_frames and the parameters (DEFAULTS' keys).

  selected    record i is selected if the note rule counts it (metrics.classify, csrc/note_rule.h), it is not a drum,
              program_lo <= program <= program_hi, and its span [F(on), max(F(off), F(on) + 1)), clipped to [0, n_frames) in f64
              (bars.pitched_spans), is not empty.  lo_i is the span's first frame, its slot q_i = lo_i / slice_frames.  The skipped
              records are those the note rule does not count.
  slices      the occupied slots in ascending order, t = 0 .. T-1; slice t has slot Q_t, and P_t is the SET of pitches selected into it
              (duplicates collapse).
  states      a state s is a split point in [0, 128]: L = {p in P_t : p < s}, R = {p in P_t : p >= s}; span(X) = max X - min X, 0 for an
              empty X.  class_t(s) = 0 if L is empty (right hand only), 2 if R is empty (left hand only), 1 otherwise.
  emission    e_t(s) = w_span (max(0, span(L) - span) + max(0, span(R) - span)) + cut_t(s) + w_mid max(0, |s - middle| - mid_free);
              cut_t(s) = w_cut max(0, cut_min - (min R - max L)) + w_centre (|2 s - (max L + min R + 1)| / 2) where class_t(s) = 1, else 0.
              A hand stretched beyond `span` costs; cutting a chord through a gap narrower than `cut_min` costs; a cut prefers the middle
              of its gap; the split is free within `mid_free` of `middle`.
  transition  x_t(s', s) = 0 if Q_t - Q_{t-1} >= rest_slots (after a rest both hands may be anywhere); else
              w_move |s - s'| + w_switch [{class_{t-1}(s'), class_t(s)} = {0, 2}]: the second term is a hand-over, everything was in one
              hand and is now in the other.
  path        C_0 = e_0; C_t(s) = e_t(s) + min over s' of (C_{t-1}(s') + x_t(s', s)), back_t(s) the SMALLEST minimiser; s_{T-1} the
              smallest minimiser of C_{T-1}, s_{t-1} = back_t(s_t); total = min C_{T-1}.  Costs are 64-bit.
  outputs     hand uint8, one per record: 1 (right) if its pitch >= s_t of its slice, 0 (left) otherwise, 255 if it is not selected.
              split int32 (T,): split[t] = 256 Q_t + s_t.  result int64 (8,): slices, selected records, left records, right records,
              total, skipped records, hand-overs on the path (the t >= 1 with Q_t - Q_{t-1} < rest_slots and
              {class_{t-1}(s_{t-1}), class_t(s_t)} = {0, 2}), 0.  With T = 0 every hand is 255 and result = (0, 0, 0, 0, 0, skipped, 0, 0).

The ranges (check_params; the C ABI refuses the same): slice_frames in [1, 64]; 0 <= program_lo <= program_hi < n_programs; span in
[1, 127]; cut_min in [0, 127]; middle and mid_free in [0, 128]; every w_* in [0, 1024]; rest_slots in [1, 2^20]; n_programs and
drum_program as bars.check_shared; n_frames in [1, MAX_FRAMES], at most MAX_NOTES records.  Within them e_t(s) <= 454 656 and
x_t <= 132 096, so the costs of one step lie within 2^20 of each other and the total stays below 2^40.

Sounding notes are not held across slices, there are two voices and no more, and only the program range is split."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np

from .bars import MAX_FRAMES, MAX_NOTES, _records, check_shared, pitched_spans
from .beats import with_defaults
from .model import _Owned
from .task_manager import DRUM_PROGRAM

NONE, LEFT, RIGHT = 255, 0, 1
STATES = 129
DEFAULTS = dict(frames_per_second=100.0, slice_frames=4, program_lo=0, program_hi=7, span=12, w_span=16, cut_min=9, w_cut=16, w_centre=1,
                middle=60, mid_free=12, w_mid=1, w_move=2, w_switch=64, rest_slots=25, n_programs=DRUM_PROGRAM + 2, drum_program=DRUM_PROGRAM)
_RANGES = (("slice_frames", 1, 64), ("span", 1, 127), ("w_span", 0, 1024), ("cut_min", 0, 127), ("w_cut", 0, 1024), ("w_centre", 0, 1024),
           ("middle", 0, 128), ("mid_free", 0, 128), ("w_mid", 0, 1024), ("w_move", 0, 1024), ("w_switch", 0, 1024), ("rest_slots", 1, 1 << 20))
_INTS = tuple(k for k in DEFAULTS if k != "frames_per_second")


def check_params(**params) -> dict:
    """the parameters with their defaults, refused (ValueError naming the parameter) outside what the C ABI accepts"""
    p = check_shared(params, DEFAULTS, _RANGES, "hand")
    if not 0 <= int(p["program_lo"]) <= int(p["program_hi"]) < int(p["n_programs"]):
        raise ValueError(f"program_lo={p['program_lo']}, program_hi={p['program_hi']} must satisfy 0 <= program_lo <= program_hi < n_programs={p['n_programs']}")
    return p


def check_sizes(max_frames: int, max_notes: int) -> None:
    if not 1 <= int(max_frames) <= MAX_FRAMES:
        raise ValueError(f"max_frames={max_frames} outside [1, {MAX_FRAMES}]")
    if not 1 <= int(max_notes) <= MAX_NOTES:
        raise ValueError(f"max_notes={max_notes} outside [1, {MAX_NOTES}]")


def n_slots(n_frames: int, slice_frames: int) -> int:
    return (int(n_frames) + int(slice_frames) - 1) // int(slice_frames)


def select(rec: np.ndarray, n_frames: int, p: dict) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (the indices of the selected records, their slots, the number of skipped records)"""
    from .metrics import classify
    counted, prog, drum = classify(rec, int(p["n_programs"]), int(p["drum_program"]))
    cand = np.flatnonzero(counted & ~drum & (prog >= int(p["program_lo"])) & (prog <= int(p["program_hi"])))
    sub = rec[cand].copy()
    sub["pitch"] = np.arange(cand.size)                                     # pitched_spans hands the pitch through: here, the record's place
    lo, _, k = pitched_spans(sub, np.zeros(cand.size, bool), n_frames, float(p["frames_per_second"]))
    return cand[k], lo // int(p["slice_frames"]), int((~counted).sum())


def pitch_classes(pitches: np.ndarray) -> np.ndarray:
    """class_t(s) of every state for the sorted, distinct pitches of a slice -> int64 (129,)"""
    s = np.arange(STATES, dtype=np.int64)
    return np.where(s <= pitches[0], 0, np.where(s > pitches[-1], 2, 1))


def emission(pitches: np.ndarray, p: dict) -> np.ndarray:
    """e_t(s) of every state for the sorted, distinct pitches of a slice -> int64 (129,)"""
    s = np.arange(STATES, dtype=np.int64)
    n_left = np.searchsorted(pitches, s, side="left")                       # the pitches below s
    n = pitches.size
    some_l, some_r = n_left > 0, n_left < n
    max_l, min_r = pitches[np.maximum(n_left - 1, 0)], pitches[np.minimum(n_left, n - 1)]
    span_l = np.where(some_l, max_l - pitches[0], 0)
    span_r = np.where(some_r, pitches[-1] - min_r, 0)
    e = int(p["w_span"]) * (np.maximum(0, span_l - int(p["span"])) + np.maximum(0, span_r - int(p["span"])))
    cut = int(p["w_cut"]) * np.maximum(0, int(p["cut_min"]) - (min_r - max_l)) + int(p["w_centre"]) * (np.abs(2 * s - (max_l + min_r + 1)) // 2)
    e += np.where(some_l & some_r, cut, 0)
    return e + int(p["w_mid"]) * np.maximum(0, np.abs(s - int(p["middle"])) - int(p["mid_free"]))


def hand_path(slots: np.ndarray, sets: List[np.ndarray], p: dict) -> Tuple[np.ndarray, int, int]:
    """the slices' slots and pitch sets -> (s_t int64 (T,), total, the hand-overs on the path); T >= 1"""
    T = len(sets)
    s = np.arange(STATES, dtype=np.int64)
    move = int(p["w_move"]) * np.abs(s[:, None] - s[None, :])               # [s'][s]
    cost = emission(sets[0], p)
    cls = pitch_classes(sets[0])
    classes = [cls]
    rest = np.zeros(T, bool)
    back = np.zeros((T, STATES), np.int64)
    for t in range(1, T):
        new_cls = pitch_classes(sets[t])
        rest[t] = int(slots[t] - slots[t - 1]) >= int(p["rest_slots"])
        if rest[t]:
            via = np.broadcast_to(cost[:, None], (STATES, STATES))
        else:
            via = cost[:, None] + move + int(p["w_switch"]) * (cls[:, None] + new_cls[None, :] == 2) * (cls[:, None] != 1)
        back[t] = np.argmin(via, axis=0)                                    # the first minimum: the smallest s'
        cost = emission(sets[t], p) + via[back[t], s]
        cls = new_cls
        classes.append(cls)
    path = np.zeros(T, np.int64)
    path[-1] = int(np.argmin(cost))
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    overs = sum(1 for t in range(1, T) if not rest[t] and {int(classes[t - 1][path[t - 1]]), int(classes[t][path[t]])} == {0, 2})
    return path, int(cost.min()), overs


def split_hands(notes, n_frames: int, **params) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host specification -> (hand uint8 (n,): 1 right, 0 left, 255 not selected; split int32 (T,): 256 Q_t + s_t of every slice;
    result int64 (8,): slices, selected, left, right, total, skipped records, hand-overs, 0).  `notes`: a list of Note or a NOTE_RECORD
    array, in any order; `params`: DEFAULTS' keys."""
    p = check_params(**params)
    if not 1 <= int(n_frames) <= MAX_FRAMES:
        raise ValueError(f"n_frames={n_frames} outside [1, {MAX_FRAMES}]")
    rec = _records(notes)
    if rec.size > MAX_NOTES:
        raise ValueError(f"{rec.size} notes: at most {MAX_NOTES}")
    idx, q, skipped = select(rec, int(n_frames), p)
    hand = np.full(rec.size, NONE, np.uint8)
    if idx.size == 0:
        return hand, np.zeros(0, np.int32), np.array([0, 0, 0, 0, 0, skipped, 0, 0], np.int64)
    slots, t_of = np.unique(q, return_inverse=True)
    pitch = rec["pitch"][idx].astype(np.int64)
    sets = [np.unique(pitch[t_of == t]) for t in range(slots.size)] if slots.size < 64 else _sets(pitch, t_of, slots.size)
    path, total, overs = hand_path(slots, sets, p)
    hand[idx] = np.where(pitch >= path[t_of], RIGHT, LEFT)
    right = int((hand[idx] == RIGHT).sum())
    return hand, (256 * slots + path).astype(np.int32), np.array([slots.size, idx.size, idx.size - right, right, total, skipped, overs, 0], np.int64)


def _sets(pitch: np.ndarray, t_of: np.ndarray, T: int) -> List[np.ndarray]:
    """the sorted, distinct pitches of every slice, in one sort"""
    keys = np.unique(t_of.astype(np.int64) * 128 + pitch)
    return np.split(keys % 128, np.searchsorted(keys // 128, np.arange(1, T)))


def hand_splits(split, frames_per_second: float, slice_frames: int) -> List[Tuple[float, int]]:
    """-> [(sec, split point)] of every slice: the time of its slot's first frame"""
    return [((int(v) >> 8) * int(slice_frames) / float(frames_per_second), int(v) & 255) for v in np.asarray(split).tolist()]


def hand_summary(hand, split, result, p: dict) -> dict:
    """what transcribe(hands=True) adds to its info dict"""
    return {"hand": [int(h) for h in np.asarray(hand).tolist()], "hand_splits": hand_splits(split, p["frames_per_second"], p["slice_frames"]),
            "hand_result": [int(v) for v in np.asarray(result).tolist()]}


class HandSplitter(_Owned):
    """The device hand splitter of one model (YourMT3.compile_hand_splitter; include/ymt3.h, hands): the parameters and scratch for
    `max_frames` frames and calls of up to `max_notes` records on the device.  `params`: DEFAULTS' keys, checked by the C ABI.  Freed by
    close(), by leaving a `with` block, or by the model's close()."""
    _destroy, _noun = "ymt3_hands_destroy", "hand splitter"

    def __init__(self, model, max_frames: int, max_notes: int, **params):
        from . import _lib
        self.params = p = with_defaults(params, DEFAULTS, "hand")
        self.max_frames, self.max_notes = int(max_frames), int(max_notes)
        self._own(model)
        c = _lib.HandParams(float(p["frames_per_second"]), *(int(p[k]) for k in _INTS))
        _lib.check(self._lib.ymt3_hands_create(model._handle, ctypes.byref(c), self.max_frames, self.max_notes, ctypes.byref(self._c)))

    def max_slices(self, n_notes: int, n_frames: int) -> int:
        """what a call of `n_notes` records over `n_frames` frames asks of split_dev"""
        return min(int(n_notes), n_slots(n_frames, self.params["slice_frames"]))

    def split(self, records, n_frames: int, count=None, splits: bool = True):
        """`records`: NOTE_RECORDs as a 1-D uint8 tensor, `count`: an int32 device tensor whose first element says how many of them are
        live, or None.  -> (hand uint8 (n,), only the live ones written, the rest 255; split int32 (max_slices,), only the first T
        written, or None without `splits`; result int64 (8,)): device tensors.  Asynchronous: nothing is copied back."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        cap = self.max_slices(n, n_frames) if 1 <= int(n_frames) <= MAX_FRAMES else 0
        hand = torch.full((n,), NONE, device=model.device, dtype=torch.uint8)
        split = torch.zeros(max(cap, 1), device=model.device, dtype=torch.int32) if splits else None
        result = torch.zeros(8, device=model.device, dtype=torch.int64)
        _lib.check(self._lib.ymt3_split_hands(model._handle, self.ptr, _ptr(rec) if n else None, n, _ptr(cnt), int(n_frames), _ptr(hand) if n else None,
                                              _ptr(split), cap, _ptr(result), model._stream()))
        return hand, split, result

    def run(self, records, n_frames: int, count=None):
        """split(), then ONE copy back -> (hand uint8 (n,), split int32 (T,), result int64 (8,)) as numpy arrays"""
        import torch
        hand, split, result = self.split(records, n_frames, count)
        n = int(hand.numel())
        flat = torch.cat([result.view(torch.uint8), split.view(torch.uint8), hand]).cpu().numpy()
        res = flat[:64].view(np.int64).copy()
        at = 64 + 4 * int(split.numel())
        return flat[at:at + n].copy(), flat[64:at].view(np.int32)[:int(res[0])].copy(), res


def estimate_hands(model, notes_or_mid_path, end_sec: Optional[float] = None, output_path: Optional[str] = None, **params) -> dict:
    """Give the piano notes of a transcription their hands: `notes_or_mid_path` (a list of Note, or the path of a flat .mid file) split on
    the device (HandSplitter; the rules: this module's docstring).  `end_sec`: the length of the music (None: the last note's end);
    `params`: DEFAULTS' keys.  -> {"hand" (one per note, in the notes' order; a file's notes are in midi.read_midi_notes' order),
    "splits" ([(sec, split point)] of every slice), "result" (the eight numbers), "midi" (the bytes of the file, two tracks per split
    program)}; with `output_path` the bytes are written there too."""
    import math
    import os
    import torch
    from .beats import n_frames_of
    from .metrics import to_records
    from .midi import notes_to_midi_bytes, read_midi_notes
    notes = notes_or_mid_path
    if isinstance(notes, (str, os.PathLike)):
        with open(notes, "rb") as f:
            notes = read_midi_notes(f.read())
    notes = list(notes)
    p = with_defaults(params, DEFAULTS, "hand")
    if end_sec is None:
        end_sec = max([0.0] + [max(n.onset, n.offset) for n in notes if math.isfinite(n.onset) and math.isfinite(n.offset)])
    n_frames = n_frames_of(float(end_sec), float(p["frames_per_second"]))
    rec = to_records(notes)
    with model.compile_hand_splitter(n_frames, max(1, len(notes)), **params) as hs:
        hand, split, result = hs.run(torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()), n_frames)
    out = {"hand": [int(h) for h in hand.tolist()], "splits": hand_splits(split, p["frames_per_second"], p["slice_frames"]),
           "result": [int(v) for v in result.tolist()]}
    out["midi"] = notes_to_midi_bytes(notes, hands=out["hand"])
    if output_path is not None:
        with open(output_path, "wb") as f:
            f.write(out["midi"])
    return out
