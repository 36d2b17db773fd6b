"""The device detokeniser's algorithm (yourmt3_amd/csrc/detok.hip) in plain Python: not the host path re-used, but the kernels'
own formulation -- rows as 64-lane scans, items bucketed per (program, pitch) key, one walk per key.  tests/test_detok_cpu.py checks
it against the host path (TaskManager.detokenize_list_batches + note_events_to_notes); a GPU disagreement is then either "model
wrong" (this file fails its CPU test) or "kernel wrong" (the kernel differs from this file).

    detokenize(table, tokens (n, K, L), starts, end_sec, steps_per_second, drum_program, scores=None)
        -> (records [(onset, offset, program, pitch, is_drum, score or None)], n_invalid)        record order unspecified
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

INVALID, STOP, SKIP, SHIFT, PITCH, VELOCITY, TIE, PROGRAM, DRUM = range(9)
WAVE = 64
KIND_TIE, KIND_PITCHED, KIND_DRUM = 0, 1, 2


def _walk_columns(ent, c0, c1, step, vel, prog, in_tie, drum_program, seg):
    """one lane's columns from its entry state -> (items, bad); an item is (seg, kind, step, vel, col, program, pitch)"""
    items, bad = [], 0
    for c in range(c0, c1):
        cls, v = ent[c] >> 12, ent[c] & 0xFFF
        if cls == STOP:
            break
        if cls == INVALID:
            bad += 1
        elif cls == SHIFT:
            in_tie, step = False, step + v
        elif cls == VELOCITY:
            vel = v
        elif cls == TIE:
            in_tie = False
        elif cls == PROGRAM:
            prog = v
        elif cls == PITCH:
            if prog == drum_program:
                if in_tie:
                    bad += 1
                elif vel:
                    items.append((seg, KIND_DRUM, step, 1, c, prog, v))
            elif in_tie:
                items.append((seg, KIND_TIE, 0, 0, c, prog, v))
            else:
                items.append((seg, KIND_PITCHED, step, 1 if vel else 0, c, prog, v))
        elif cls == DRUM:
            if in_tie:
                bad += 1
            else:
                items.append((seg, KIND_DRUM, step, 1, c, drum_program, v))
    return items, bad


def row_items(table, row: Sequence[int], seg: int, drum_program: int):
    """kernel (a): one wave over one row -> (items in column order, bad)"""
    L = len(row)
    ent = [int(table[t]) if 0 <= t < len(table) else 0 for t in (int(t) for t in row)]
    per = -(-L // WAVE)
    bounds = [(min(l * per, L), min(min(l * per, L) + per, L)) for l in range(WAVE)]
    agg = []                                      # lane-local: (shift sum, last velocity or -1, last program or -1, opened, stop)
    for c0, c1 in bounds:
        s, lv, lp, opened, stop = 0, -1, -1, False, False
        for c in range(c0, c1):
            cls, v = ent[c] >> 12, ent[c] & 0xFFF
            if cls == STOP:
                stop = True
                break
            if cls == SHIFT:
                s, opened = s + v, True
            elif cls == TIE:
                opened = True
            elif cls == VELOCITY:
                lv = v
            elif cls == PROGRAM:
                lp = v
        agg.append((s, lv, lp, opened, stop))
    items, bad = [], 0
    for l, (c0, c1) in enumerate(bounds):
        lower = agg[:l]
        if any(a[4] for a in lower):              # a lower lane ended the row
            continue
        step0 = sum(a[0] for a in lower)                                  # exclusive prefix sum
        vel0 = next((a[1] for a in reversed(lower) if a[1] >= 0), 1)      # last writer below, else the initial value
        prog0 = next((a[2] for a in reversed(lower) if a[2] >= 0), 0)
        in_tie0 = not any(a[3] for a in lower)
        it, b = _walk_columns(ent, c0, c1, step0, vel0, prog0, in_tie0, drum_program, seg)
        items += it
        bad += b
    return items, bad


def _gt(a: Optional[float], b: Optional[float]) -> bool:
    return a is not None and b is not None and a > b


def merge_key(items, program: int, pitch: int, starts, end_sec: float, sps: int, drum_program: int, score_of):
    """kernel (b), one lane: the bucket of one (program, pitch) key -> records"""
    def t_of(it):
        return starts[it[0]] + it[2] / sps

    out = []
    order = sorted(items, key=lambda it: (it[0], it[1] != KIND_TIE, it[2], it[3], it[4]))
    if program == drum_program:
        order = sorted(order, key=t_of)           # stable: equal times stay in processing order
        i = 0
        while i < len(order):
            t, sc = t_of(order[i]), score_of(order[i])
            i += 1
            while i < len(order) and t_of(order[i]) == t:
                s2 = score_of(order[i])
                if _gt(s2, sc):
                    sc = s2
                i += 1
            out.append((t, t + 0.01, program, pitch, True, sc))
        return out
    active, on, score, q = False, 0.0, None, 0
    for it in order:
        s, tie = it[0], it[1] == KIND_TIE
        if active and s > q:
            if tie and s == q + 1:
                q = s
                continue
            if starts[q + 1] > on:
                out.append((on, starts[q + 1], program, pitch, False, score))
            active = False
        if tie:
            continue
        t = t_of(it)
        if it[3]:
            if active and t > on:
                out.append((on, t, program, pitch, False, score))
            active, on, score, q = True, t, score_of(it), s
        elif active:
            if t > on:
                out.append((on, t, program, pitch, False, score))
            active = False
    if active:
        end = starts[q + 1] if q != len(starts) - 1 else end_sec
        if end > on:
            out.append((on, end, program, pitch, False, score))
    return out


def detokenize(table, tokens, starts: Sequence[float], end_sec: float, steps_per_second: int, drum_program: int, scores=None):
    n, K = len(tokens), len(tokens[0]) if len(tokens) else 0
    starts = [float(s) for s in starts]
    records: List[Tuple] = []
    n_invalid = 0
    for ch in range(K):
        buckets = {}
        for seg in range(n):
            items, bad = row_items(table, tokens[seg][ch], seg, drum_program)
            n_invalid += bad
            for it in items:
                buckets.setdefault((it[5], it[6]), []).append(it)

        def score_of(it, ch=ch):
            return None if scores is None else float(scores[it[0]][ch][it[4]])

        for (program, pitch), items in buckets.items():
            records += merge_key(items, program, pitch, starts, float(end_sec), steps_per_second, drum_program, score_of)
    return records, n_invalid


def to_notes(records):
    """records -> sorted List[Note] with confidence = exp(score), as TaskManager.tokens_to_notes_device builds them"""
    from yourmt3_amd.task_manager import Note
    return sorted(Note(on, off, dr, pg, pt, confidence=None if sc is None else math.exp(sc)) for on, off, pg, pt, dr, sc in records)
