"""Fuzz cases of the device detokeniser, shared by tests/test_detok_cpu.py (the plain-Python model of the kernels) and tests/test_detok.py
(the kernels): seeded synthetic ids, the host reference (TaskManager.detokenize_list_batches + note_events_to_notes), computed once per
case, and the coverage count that says which merge rules the reference notes exercise.

Families: `uniform` ids over [0, vocab); `dense` on 6 pitches x programs {0, 1, 128, 129} x 3 drums with shifts {1, 2, 6, 101, 206},
velocities, TIE, stray EOS / PAD and ids around codec.size; `grammar` rows from encode_segment with ties carried over several segments."""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

from yourmt3_amd.task_manager import DRUM_NOTE_SEC, DRUM_PROGRAM, Note, NoteEvent, TaskManager, note_events_to_notes
from yourmt3_amd.vocab import EOS, PAD, UNK, Event

SEED = 20261017
SEGMENT_SEC = 32767 / 16000
TASK_OF_K = {1: "mt3_full_plus", 13: "mc13_full_plus_256"}

# (task, L, n_segments); every L in {1, 5, 64, 65, 130, 1024} (13 channels: up to the task's 256 columns) and every n in {1, 2, 3, 7, 65}
# occurs; each shape runs all three families, scores and the two start-time sets alternate
SHAPES = [
    ("mt3_full_plus", 1, 1), ("mt3_full_plus", 1, 7), ("mt3_full_plus", 5, 2), ("mt3_full_plus", 5, 65), ("mt3_full_plus", 64, 3),
    ("mt3_full_plus", 64, 1), ("mt3_full_plus", 65, 7), ("mt3_full_plus", 65, 2), ("mt3_full_plus", 130, 3), ("mt3_full_plus", 130, 65),
    ("mt3_full_plus", 1024, 1), ("mt3_full_plus", 1024, 2), ("mt3_full_plus", 1024, 7), ("singing_drum_v1", 65, 3), ("singing_drum_v1", 130, 7),
    ("mc13_full_plus_256", 1, 2), ("mc13_full_plus_256", 5, 3), ("mc13_full_plus_256", 64, 7), ("mc13_full_plus_256", 65, 1),
    ("mc13_full_plus_256", 130, 7), ("mc13_full_plus_256", 5, 65),
]
BIG = [("mt3_full_plus", 1024, 65, "dense"), ("mc13_full_plus_256", 130, 65, "grammar")]       # one full-size case each


@lru_cache(maxsize=None)
def task_manager(name: str) -> TaskManager:
    return TaskManager(name)


def _uniform(rng, tm, n, K, L):
    return rng.integers(0, tm.vocab_size, (n, K, L)).astype(np.int32)


def _dense(rng, tm, n, K, L):
    c = tm.codec
    enc = lambda t, v: c.encode(Event(t, v))
    pitches = [enc("pitch", p) for p in (36, 60, 61, 64, 72, 127)]
    pool = (pitches * 6 + [enc("program", p) for p in (0, 1, 128, 129)] * 2 + [enc("drum", p) for p in (35, 38, 42)] * 3 +
            [enc("shift", s) for s in (1, 1, 2, 2, 6, 6, 101, 206)] + [enc("velocity", 0), enc("velocity", 1)] * 3 + [enc("tie", 0)] * 2)
    rare = [EOS, PAD, UNK, c.size - 1, c.size, c.size + 1, tm.vocab_size - 1]
    t = rng.choice(np.array(pool), (n, K, L))
    r = rng.random((n, K, L))
    t = np.where(r < 0.004, rng.choice(np.array(rare), (n, K, L)), t)
    return t.astype(np.int32)


def _grammar(rng, tm, n, K, L, starts):
    """well-formed rows: notes keep sounding over several segments and are tied across them; now and then a tie is left out (the note
    then ends at the boundary) or the row is cut short (no EOS)"""
    tok = tm.tokenizer
    out = np.zeros((n, K, L), np.int32)
    n_ev = max(0, min(40, (L - 6) // 3))
    for ch in range(K):
        progs = [0, 1, 129] if K == 1 else list(tm_groups(tm)[ch])[:2]
        sounding = set()
        for s in range(n):
            ties = [k for k in sorted(sounding) if rng.random() > 0.15]
            sounding = set(ties)
            events = []
            for _ in range(int(rng.integers(0, n_ev + 1))):
                step = int(rng.integers(0, 205))
                t = starts[s] + step / tm.codec.steps_per_second
                if rng.random() < 0.2 and (K == 1 or DRUM_PROGRAM in progs):
                    events.append(NoteEvent(t, True, DRUM_PROGRAM, 1, int(rng.choice([35, 38]))))
                    continue
                prog = int(rng.choice(progs))
                if prog == DRUM_PROGRAM:
                    continue
                key = (prog, int(rng.choice([48, 50, 52, 53])))
                if key in sounding and rng.random() < 0.3:
                    sounding.discard(key)
                    events.append(NoteEvent(t, False, key[0], 0, key[1]))
                else:
                    sounding.add(key)
                    events.append(NoteEvent(t, False, key[0], 1, key[1]))
            # the set of sounding notes must be what the events leave in TIME order: recompute it as the host will see it
            state = set(ties)
            for ev in sorted(events):
                if not ev.is_drum:
                    (state.add if ev.velocity else state.discard)((ev.program, ev.pitch))
            sounding = state
            row = tok.encode_segment(events, ties, starts[s])[:L]
            out[s, ch, :len(row)] = row
    return out


def tm_groups(tm):
    from yourmt3_amd.task_manager import MC13_GROUPS
    return [progs for _, progs in MC13_GROUPS]


def _scores(rng, shape):
    sc = (-np.abs(rng.standard_normal(shape)) * 2).astype(np.float32)
    r = rng.random(shape)
    sc[r < 0.02] = np.nan
    sc[(r >= 0.02) & (r < 0.04)] = -np.inf
    sc[(r >= 0.04) & (r < 0.05)] = 0.0
    return sc


def _starts(rng, n, irregular):
    if not irregular:
        return [i * 32767 / 16000 for i in range(n)]
    return [float(v) for v in np.cumsum(rng.uniform(0.4, 3.0, n)) - 0.3]


@lru_cache(maxsize=None)
def cases() -> Tuple[dict, ...]:
    out = []
    todo = [(task, L, n, fam) for (task, L, n) in SHAPES for fam in ("uniform", "dense", "grammar")] + BIG
    for i, (task, L, n, fam) in enumerate(todo):
        rng = np.random.default_rng([SEED, i])
        tm = task_manager(task)
        K = tm.num_decoding_channels
        starts = _starts(rng, n, irregular=bool((i // 3 + i) % 2))
        if fam == "uniform":
            tokens = _uniform(rng, tm, n, K, L)
        elif fam == "dense":
            tokens = _dense(rng, tm, n, K, L)
        else:
            tokens = _grammar(rng, tm, n, K, L, starts)
        scores = _scores(rng, tokens.shape) if i % 2 == 0 else None
        out.append({"id": f"{task}-{fam}-L{L}-n{n}-{'scored' if scores is not None else 'plain'}", "task": task, "family": fam, "tokens": tokens,
                    "scores": scores, "starts": starts, "end_sec": starts[-1] + 0.37 * SEGMENT_SEC})
    return tuple(out)


_REF: Dict[str, tuple] = {}


def reference(case) -> Tuple[List[Note], int, List[list]]:
    """the host path -> (sorted notes, n_invalid, per-channel segments (start, events, ties)); computed once per case"""
    if case["id"] not in _REF:
        tm = task_manager(case["task"])
        tokens, scores = case["tokens"], case["scores"]
        per_channel, bad = [], 0
        for ch in range(tm.num_decoding_channels):
            segs, b = tm.detokenize_list_batches([tokens[:, ch]], case["starts"], return_events=True,
                                                 list_batch_score_arrays=None if scores is None else [scores[:, ch]])
            per_channel.append(segs)
            bad += b
        if tm.num_decoding_channels == 1:
            notes = note_events_to_notes(per_channel[0], case["end_sec"])
        else:
            notes = tm.tokens_to_notes([tokens], case["starts"], case["end_sec"], None if scores is None else [scores])
        _REF[case["id"]] = (notes, bad, per_channel)
    return _REF[case["id"]]


def same_notes(got: List[Note], ref: List[Note]) -> Optional[str]:
    """None if the lists are equal (== on Note) and the confidences are equal as Python floats (NaN matching NaN), else what differs"""
    if got != ref:
        extra = [n for n in got if n not in ref][:3]
        missing = [n for n in ref if n not in got][:3]
        return f"{len(got)} notes against {len(ref)}; only in got {extra}; only in the reference {missing}"
    # equal notes may still stand in another order where they tie on every compared field: compare confidences as multisets per note
    key = lambda n: (n, -1.0 if n.confidence is None else (2.0 if math.isnan(n.confidence) else n.confidence))
    for a, b in zip(sorted(got, key=key), sorted(ref, key=key)):
        ca, cb = a.confidence, b.confidence
        if not (ca == cb or (ca is not None and cb is not None and math.isnan(ca) and math.isnan(cb))):
            return f"confidence {ca!r} against {cb!r} for {b}"
    return None


KINDS = ("offset", "retrigger", "segment_start", "tie_two_boundaries", "end_sec", "drum_dedup_larger", "onset_dropped_overshoot")


def coverage(case) -> Dict[str, int]:
    """How many reference notes of every kind the case holds.  A tagged restatement of note_events_to_notes over the HOST's events, kept
    honest by asserting that its notes are the host's notes; nothing of the device path or of tests/detok_model.py is involved."""
    notes_ref, _, per_channel = reference(case)
    count = dict.fromkeys(KINDS, 0)
    end_sec = case["end_sec"]
    mine: List[Note] = []
    for segs in per_channel:
        active: Dict[Tuple[int, int], Tuple[float, Optional[float], int]] = {}      # key -> (onset, confidence, boundaries survived)
        notes: List[Note] = []
        hits: Dict[Tuple[float, int], int] = {}
        for start, events, ties in segs:
            tie_set = set(ties)
            for key in list(active):
                on, conf, nb = active[key]
                if key in tie_set:
                    active[key] = (on, conf, nb + 1)
                    continue
                del active[key]
                if start > on:
                    notes.append(Note(on, start, False, key[0], key[1], confidence=conf))
                    count["segment_start"] += 1
                    count["tie_two_boundaries"] += nb >= 2
                else:
                    count["onset_dropped_overshoot"] += 1
            for ev in sorted(events):
                conf = None if ev.score is None else math.exp(ev.score)
                if ev.is_drum:
                    hit = (ev.time, ev.pitch)
                    if hit not in hits:
                        hits[hit] = len(notes)
                        notes.append(Note(ev.time, ev.time + DRUM_NOTE_SEC, True, DRUM_PROGRAM, ev.pitch, confidence=conf))
                    elif conf is not None and (notes[hits[hit]].confidence is None or conf > notes[hits[hit]].confidence):
                        old = notes[hits[hit]]
                        notes[hits[hit]] = Note(old.onset, old.offset, True, DRUM_PROGRAM, old.pitch, confidence=conf)
                        count["drum_dedup_larger"] += 1
                    continue
                key = (ev.program, ev.pitch)
                if ev.velocity:
                    if key in active and ev.time > active[key][0]:
                        notes.append(Note(active[key][0], ev.time, False, key[0], key[1], confidence=active[key][1]))
                        count["retrigger"] += 1
                        count["tie_two_boundaries"] += active[key][2] >= 2
                    active[key] = (ev.time, conf, 0)
                elif key in active:
                    on, oconf, nb = active.pop(key)
                    if ev.time > on:
                        notes.append(Note(on, ev.time, False, key[0], key[1], confidence=oconf))
                        count["offset"] += 1
                        count["tie_two_boundaries"] += nb >= 2
        for key, (on, conf, nb) in active.items():
            if end_sec > on:
                notes.append(Note(on, end_sec, False, key[0], key[1], confidence=conf))
                count["end_sec"] += 1
                count["tie_two_boundaries"] += nb >= 2
        mine += notes
    assert same_notes(sorted(mine), notes_ref) is None, "the tagged restatement left the host path"
    return count
