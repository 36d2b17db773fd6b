"""The device tokeniser's algorithm (yourmt3_amd/csrc/tok.hip) in plain Python, lane by lane: item words, the per-segment tie bitmap, the
per-row counters, the sort, the scans over 64 lanes' chunks of events and the guarded writes.  tests/test_tok_cpu.py compares it with the host
path (TaskManager.notes_to_tokens), which is the specification; a disagreement on the GPU is then this model's or the kernels'."""
from __future__ import annotations

import bisect
from typing import Dict, List, Sequence, Tuple

import numpy as np

WAVE = 64
PITCHES = 128
BODY = 1 << 49
STEP_MAX = 2147483646


def pack_item(body: bool, step: int, drum: int, prog: int, vel: int, pitch: int) -> int:
    return (BODY if body else 0) | (step << 17) | (drum << 16) | (prog << 8) | (vel << 7) | pitch


def unpack(x: int) -> Tuple[int, int, int, int, int]:
    """-> (step, drum, prog, vel, pitch)"""
    return (x >> 17) & 0x7FFFFFFF, (x >> 16) & 1, (x >> 8) & 0xFF, (x >> 7) & 1, x & 0x7F


def to_step(t: float, t0: float, sps: int) -> int:
    d = (np.float64(t) - np.float64(t0)) * np.float64(sps)
    r = np.rint(d)
    if r >= STEP_MAX:
        return STEP_MAX
    return int(r) if r > 0.0 else 0


def items_of(p: Dict[str, int], chan: Sequence[int], records, starts: Sequence[float], end_sec: float, K: int, L: int):
    """tok_items_kernel -> (items[row] (the first L appended), count[row])"""
    n = len(starts)
    items: List[List[int]] = [[] for _ in range(n * K)]
    count = [0] * (n * K)
    seen = [set() for _ in range(n)]                    # the bitmap, one set of keys per segment

    def append(seg, ch, w):
        row = seg * K + ch
        if count[row] < L:
            items[row].append(w)
        count[row] += 1

    for onset, offset, program, pitch, is_drum in records:
        drum = bool(is_drum)
        prog = p["drum_program"] if drum else int(program)
        if not (onset >= starts[0] and onset < end_sec):
            continue
        if not (0 <= prog < len(chan) and 0 <= pitch < PITCHES):
            continue
        if not drum and offset != offset:
            continue
        ch = int(chan[prog])
        s = bisect.bisect_right(starts, onset) - 1
        step = to_step(onset, starts[s], p["steps_per_second"])
        append(s, ch, pack_item(True, step, int(drum), prog, 1, pitch))
        if drum:
            continue
        key = prog * PITCHES + pitch
        s2 = s + 1
        while s2 < n and starts[s2] < offset:
            if key not in seen[s2]:
                seen[s2].add(key)
                append(s2, ch, pack_item(False, 0, 0, prog, 0, pitch))
            s2 += 1
        if offset >= end_sec:
            continue
        so = bisect.bisect_right(starts, offset) - 1
        if so <= s:
            so = s
            ostep = to_step(offset, starts[s], p["steps_per_second"])
            if ostep <= step:
                ostep = step + 1
        else:
            if offset == starts[so]:
                continue
            ostep = to_step(offset, starts[so], p["steps_per_second"])
        append(so, ch, pack_item(True, ostep, 0, prog, 0, pitch))
    return items, count


def walk_events(p, S, c0, c1, prev_step, prev_vel, cur_prog, L, out, pos):
    """one lane's events -> number of tokens; out is None: count only"""
    n = 0
    ms = p["max_shift_steps"]

    def put(tok):
        nonlocal n
        if out is not None and pos + n < L:
            out[pos + n] = tok
        n += 1

    for c in range(c0, c1):
        step, drum, prog, vel, pitch = unpack(S[c])
        vel = 1 if drum else vel
        d = step - prev_step
        assert d >= 0
        if d > 0:
            ns = min((d - 1) // ms + 1, L + 1)
            if out is not None:
                k = 0
                while k < ns and pos + n + k < L:
                    out[pos + n + k] = p["shift_base"] + min(d, ms) - 1
                    d -= ms
                    k += 1
            n += ns
        prev_step = step
        if vel != prev_vel:
            put(p["velocity_base"] + vel)
            prev_vel = vel
        if drum:
            put(p["drum_base"] + pitch)
            continue
        if prog != cur_prog:
            put(p["program_base"] + prog)
            cur_prog = prog
        put(p["pitch_base"] + pitch)
    return n


def row_tokens(p: Dict[str, int], words: List[int], count: int, L: int) -> Tuple[List[int], int]:
    """tok_rows_kernel -> (L ids, length)"""
    out = [p["pad_id"]] * L
    if count > L:
        return out, count + 2
    S = sorted(words)
    T = sum(1 for x in S if not x & BODY)
    for i in range(T):
        _, _, prog, _, pitch = unpack(S[i])
        if 2 * i < L:
            out[2 * i] = p["program_base"] + prog
        if 2 * i + 1 < L:
            out[2 * i + 1] = p["pitch_base"] + pitch
    if 2 * T < L:
        out[2 * T] = p["tie_base"]
    E = count - T
    per = (E + WAVE - 1) // WAVE
    chunks = [(T + min(l * per, E), T + min(l * per + per, E)) for l in range(WAVE)]
    lprog = []
    for c0, c1 in chunks:
        lp = -1
        for c in range(c0, c1):
            if not unpack(S[c])[1]:
                lp = unpack(S[c])[2]
        lprog.append(lp)
    entry = []
    for l, (c0, c1) in enumerate(chunks):
        prog0 = next((lprog[m] for m in range(l - 1, -1, -1) if lprog[m] >= 0), -1)
        step0, vel0 = 0, -1
        if c0 > T and c0 < c1:
            st, drum, _, vel, _ = unpack(S[c0 - 1])
            step0, vel0 = st, (1 if drum else vel)
        entry.append((step0, vel0, prog0))
    counts = [walk_events(p, S, c0, c1, *entry[l], L, None, 0) for l, (c0, c1) in enumerate(chunks)]
    incl = list(np.cumsum(counts))
    total = 2 * T + 1 + int(incl[-1]) + 1
    for l, (c0, c1) in enumerate(chunks):
        if counts[l]:
            walk_events(p, S, c0, c1, *entry[l], L, out, 2 * T + 1 + int(incl[l]) - counts[l])
    if total <= L:
        out[total - 1] = p["eos_id"]
    return out, total


def tokenize(p: Dict[str, int], chan: Sequence[int], records, starts: Sequence[float], end_sec: float, K: int, L: int):
    """records: (onset, offset, program, pitch, is_drum) tuples -> (tokens (n, K, L) int32, lengths (n, K) int32)"""
    n = len(starts)
    tokens = np.zeros((n, K, L), np.int32)
    lengths = np.zeros((n, K), np.int64)
    if n == 0:
        return tokens, lengths.astype(np.int32)
    items, count = items_of(p, chan, records, [float(s) for s in starts], float(end_sec), K, L)
    for row in range(n * K):
        ids, ln = row_tokens(p, items[row], count[row], L)
        tokens[row // K, row % K] = ids
        lengths[row // K, row % K] = ln
    return tokens, lengths.astype(np.int32)


def records_of(notes) -> list:
    return [(float(nt.onset), float(nt.offset), int(nt.program), int(nt.pitch), int(bool(nt.is_drum))) for nt in notes]

