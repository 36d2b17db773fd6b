"""Cases and host-side arithmetic of the live-transcription tests (tests/test_live_cpu.py, tests/test_live.py).

Ingest: the finality rule of include/ymt3.h (streaming ingest) restated -- final_samples, plan_ready, first_frame_completing.

Incremental detokeniser: the fuzz cases of tests/detok_cases.py that have a boundary to cut at, plus hand-built cases for the held-hit
rules (random ids rarely shift past a segment's end onto another hit's exact f64 time); the ways of cutting a case into pushes; the host
reference per push (NoteStream, one per channel); and the coverage count that says which carry rules a (case, split) exercises, counted on
the host specification alone."""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

import detok_cases as C
from oracle import ingest_oracle as IO
from yourmt3_amd.task_manager import DRUM_NOTE_SEC, DRUM_PROGRAM, Note, NoteEvent, NoteStream

MAX_HELD = 256                      # the state's bound in every case but the one built to reach it (a dense fuzz row shifts far past its segment)
SMALL_MAX_HELD = 4


# ---------------------------------------------------------------------------------------------- ingest
def final_samples(n_frames: int, sr_in: int, sr_out: int) -> int:
    """output samples that are final once n_frames input frames have arrived: max(0, ceil(N * up / down) - r)"""
    up, down = IO.rates(sr_in, sr_out)
    r = IO.plan(0, up, down)[1]
    return max(0, -(-n_frames * up // down) - r)


def plan_ready(n_frames: int, sr_in: int, sr_out: int, segment_samples: int) -> int:
    """whole segments final after n_frames frames (ymt3_ingest_stream_plan reports this minus the segments already delivered)"""
    return final_samples(n_frames, sr_in, sr_out) // segment_samples


def first_frame_completing(k: int, sr_in: int, sr_out: int, segment_samples: int) -> int:
    """the smallest frame count at which k whole segments are final"""
    up, down = IO.rates(sr_in, sr_out)
    n = (k * segment_samples * down) // up
    while plan_ready(n, sr_in, sr_out, segment_samples) >= k:
        n -= 1
    while plan_ready(n, sr_in, sr_out, segment_samples) < k:
        n += 1
    return n


# ---------------------------------------------------------------------------------------------- cases
def _grid_match(base: int) -> int:
    """a step k with 0.0 + (base + k) / 100 == base / 100 + k / 100 in f64: a hit `base` steps into one segment lands exactly on step k of
    the segment that starts base / 100 s later"""
    for k in range(3, 60):
        if 0.0 + (base + k) / 100 == base / 100 + k / 100:
            return k
    raise AssertionError("no matching step")


def _hand(name, rows, max_held=MAX_HELD, scored=True):
    """rows: per segment (events [(step, kind, program, pitch, score)], ties); starts are 0, 2, 4, ...; kind 'drum' | 'on' | 'off'"""
    tm = C.task_manager("mt3_full_plus")
    L = 40
    n = len(rows)
    starts = [2.0 * i for i in range(n)]
    tokens = np.zeros((n, 1, L), np.int32)
    scores = np.full((n, 1, L), -3.0, np.float32)
    for s, (events, ties) in enumerate(rows):
        evs = [NoteEvent(starts[s] + step / 100, kind == "drum", DRUM_PROGRAM if kind == "drum" else prog, 0 if kind == "off" else 1, pitch)
               for step, kind, prog, pitch, _ in events]
        row = tm.tokenizer.encode_segment(evs, ties, starts[s], max_len=L)
        tokens[s, 0] = row
        # the score of an event's own token: events come out of encode_segment in sorted order, one pitch / drum token each after the TIE
        cols = [c for c in range(row.index(tm.codec.encode(C.Event("tie", 0))) + 1, L)
                if tm.codec.decode(row[c]).type in ("pitch", "drum")]
        order = sorted(range(len(evs)), key=lambda i: evs[i])
        assert len(cols) == len(evs)
        for c, i in zip(cols, order):
            scores[s, 0, c] = events[i][4]
    return {"id": f"hand-{name}", "task": "mt3_full_plus", "family": "hand", "tokens": tokens, "scores": scores if scored else None,
            "starts": starts, "end_sec": starts[-1] + 1.0, "max_held": max_held}


@lru_cache(maxsize=None)
def hand_cases() -> Tuple[dict, ...]:
    k2, k4 = _grid_match(200), _grid_match(400)
    D = lambda step, score, pitch=38: (step, "drum", DRUM_PROGRAM, pitch, score)
    out = [
        # a hit past the segment's end, repeated by the next segment with a smaller score: held, de-duplicated, confidence kept
        _hand("dedup-next-push", [([D(10, -1.0), D(200 + k2, -1.0)], []), ([D(k2, -2.0), D(50, -1.5)], []), ([D(5, -0.5)], [])]),
        # the same with a larger score: the held hit's confidence is raised
        _hand("raised-next-push", [([D(200 + k2, -2.0)], []), ([D(k2, -0.25)], []), ([], [])]),
        # a hit two segments ahead: held over more than one push, then raised by the third segment
        _hand("held-two-pushes", [([D(400 + k4, -2.0), D(30, -1.0, 42)], []), ([D(7, -1.0)], []), ([D(k4, -0.5)], []), ([], [])]),
        # without scores: the same rules, nothing to raise
        _hand("dedup-unscored", [([D(200 + k2, 0.0), D(400 + k4, 0.0)], []), ([D(k2, 0.0)], []), ([D(k4, 0.0)], [])], scored=False),
        # pitched notes around the same boundaries: tied over two pushes, closed by a missing tie, re-triggered after a tie
        _hand("pitched-carry", [([(10, "on", 0, 60, -1.0), (20, "on", 0, 64, -1.2), (30, "on", 1, 60, -0.7), D(200 + k2, -1.0)], []),
                                ([(40, "on", 0, 60, -0.4), D(k2, -0.9)], [(0, 60), (1, 60)]),
                                ([(15, "off", 1, 60, 0.0)], [(0, 60), (1, 60)]),
                                ([], [(0, 60)])]),
    ]
    # more hits ahead of the horizon than a state of SMALL_MAX_HELD holds: the earliest leave early and count as forced
    ahead = [D(200 + 3 * i, -1.0 - 0.1 * i) for i in range(SMALL_MAX_HELD + 3)]
    out.append(_hand("max-held", [(ahead, []), ([D(3, -0.5)], []), ([], [])], max_held=SMALL_MAX_HELD))
    return tuple(out)


@lru_cache(maxsize=None)
def cases() -> Tuple[dict, ...]:
    """fuzz cases with 2..7 segments (every family, both channel counts), one 65-segment case per channel count, and the hand-built ones"""
    fuzz = [c for c in C.cases() if 2 <= c["tokens"].shape[0] <= 7 and c["tokens"].size <= 20000]
    long = [c for c in C.cases() if c["tokens"].shape[0] == 65 and c["tokens"].shape[2] == 5 and c["family"] == "dense"]
    return tuple(dict(c, max_held=MAX_HELD) for c in fuzz + long) + hand_cases()


def reference(case):
    """(sorted notes, n_invalid, per-channel segments) of the one-shot host path; hand-built cases go through the same functions"""
    return C.reference(case)


def splits(n: int, seed: int = 0) -> List[Tuple[str, List[List[int]]]]:
    """ways of cutting n segments into pushes: at every boundary, at none, at seeded random boundaries (twice)"""
    out = [("every", [[i] for i in range(n)]), ("none", [list(range(n))])]
    for r in range(2):
        rng = np.random.default_rng([20261018, n, seed, r])
        cuts = [i for i in range(1, n) if rng.random() < 0.4]
        groups = [list(range(a, b)) for a, b in zip([0] + cuts, cuts + [n])]
        if n > 2 and groups not in [g for _, g in out]:
            out.append((f"random{r}", groups))
    return out


def horizon(case, groups, g: int) -> float:
    """the start of the first segment after push g, +inf after the last"""
    return case["starts"][groups[g + 1][0]] if g + 1 < len(groups) else math.inf


@lru_cache(maxsize=None)
def _stream_ref(case_id: str, split_name: str):
    case = next(c for c in cases() + tuple(C.cases()) if c["id"] == case_id)
    groups = dict(splits(case["tokens"].shape[0]))[split_name]
    _, _, per_channel = reference(case)
    tm = C.task_manager(case["task"])
    streams = [NoteStream() for _ in per_channel]
    pushes = []
    for g, idx in enumerate(groups):
        notes: List[Note] = []
        for st, segs in zip(streams, per_channel):
            notes += st.push([segs[i] for i in idx], horizon(case, groups, g))
        bad = sum(tm.detokenize_list_batches([case["tokens"][idx, ch]], [case["starts"][i] for i in idx], return_events=True)[1]
                  for ch in range(tm.num_decoding_channels))
        pushes.append((sorted(notes), bad, sum(st.n_held for st in streams)))
    last: List[Note] = []
    for st in streams:
        last += st.finish(case["end_sec"])
    return tuple(pushes), sorted(last)


def stream_reference(case, split_name: str):
    """NoteStream over the case cut by the named split -> ([(notes, n_invalid, hits held after the push) per push], notes of the finish)"""
    return _stream_ref(case["id"], split_name)


KINDS = ("tie_across_push", "closed_at_push_boundary", "retrigger_across_push", "held_dedup_next_push", "held_raised", "held_over_two_pushes")


def coverage(case, groups) -> Dict[str, int]:
    """How often every carry rule fires when the case is cut into `groups`: a tagged restatement of note_events_to_notes over the HOST's
    events that knows which push an onset or a hit came from, kept honest by asserting that its notes are the host's notes."""
    notes_ref, _, per_channel = reference(case)
    push_of = {i: g for g, idx in enumerate(groups) for i in idx}
    hz = [horizon(case, groups, g) for g in range(len(groups))]
    count = dict.fromkeys(KINDS, 0)
    mine: List[Note] = []
    for segs in per_channel:
        active: Dict[Tuple[int, int], Tuple[float, Optional[float], int]] = {}       # key -> (onset, confidence, push of the onset)
        notes: List[Note] = []
        hits: Dict[Tuple[float, int], Tuple[int, int]] = {}                          # (time, pitch) -> (index in notes, push first seen)
        for si, (start, events, ties) in enumerate(segs):
            p = push_of[si]
            first_of_push = groups[p][0] == si and si > 0
            tie_set = set(ties)
            for key in list(active):
                on, conf, _ = active[key]
                if key in tie_set:
                    count["tie_across_push"] += first_of_push
                    continue
                del active[key]
                if start > on:
                    notes.append(Note(on, start, False, key[0], key[1], confidence=conf))
                    count["closed_at_push_boundary"] += first_of_push
            for ev in sorted(events):
                conf = None if ev.score is None else math.exp(ev.score)
                if ev.is_drum:
                    hit = (ev.time, ev.pitch)
                    if hit not in hits:
                        hits[hit] = (len(notes), p)
                        notes.append(Note(ev.time, ev.time + DRUM_NOTE_SEC, True, DRUM_PROGRAM, ev.pitch, confidence=conf))
                        # still held after the NEXT push as well: its time is not below that push's horizon either
                        count["held_over_two_pushes"] += p + 1 < len(groups) and not ev.time < hz[p + 1]
                    else:
                        i, p0 = hits[hit]
                        count["held_dedup_next_push"] += p > p0
                        if conf is not None and (notes[i].confidence is None or conf > notes[i].confidence):
                            notes[i] = Note(notes[i].onset, notes[i].offset, True, DRUM_PROGRAM, notes[i].pitch, confidence=conf)
                            count["held_raised"] += p > p0
                    continue
                key = (ev.program, ev.pitch)
                if ev.velocity:
                    if key in active and ev.time > active[key][0]:
                        notes.append(Note(active[key][0], ev.time, False, key[0], key[1], confidence=active[key][1]))
                        count["retrigger_across_push"] += p > active[key][2]
                    active[key] = (ev.time, conf, p)
                elif key in active:
                    on, oconf, _ = active.pop(key)
                    if ev.time > on:
                        notes.append(Note(on, ev.time, False, key[0], key[1], confidence=oconf))
        for key, (on, conf, _) in active.items():
            if case["end_sec"] > on:
                notes.append(Note(on, case["end_sec"], False, key[0], key[1], confidence=conf))
        mine += notes
    assert C.same_notes(sorted(mine), notes_ref) is None, "the tagged restatement left the host path"
    return count
