"""The incremental device detokeniser's algorithm (yourmt3_amd/csrc/detok.hip, kernel (c)) in plain Python: not NoteStream re-used, but
the kernel's own formulation -- kernel (a)'s items (tests/detok_model.py) bucketed per key, and one walk per key that starts from the
carried state and stores it back; held drum hits as a bounded, time-ordered list per (channel, pitch) merged with the push's bucket in two
passes.  tests/test_live_cpu.py checks it per push against NoteStream; a GPU disagreement is then either "model wrong" or "kernel wrong".

    c = DetokCarry(table, n_channels, steps_per_second, drum_program, max_held)
    c.push(tokens (n, K, L), starts, horizon_sec, scores=None) -> (records, n_invalid, n_forced)       record order unspecified
    c.finish(end_sec)                                           -> (records, 0, 0)
    records: [(onset, offset, program, pitch, is_drum, score or None)]
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import detok_model as M


class DetokCarry:
    def __init__(self, table, n_channels: int, steps_per_second: int, drum_program: int, max_held: int):
        self.table, self.K, self.sps, self.drum_program, self.max_held = table, n_channels, steps_per_second, drum_program, max_held
        self.sounding: List[Dict[Tuple[int, int], Tuple[float, object]]] = [dict() for _ in range(n_channels)]   # key -> (onset, score)
        self.held: List[Dict[int, List[Tuple[float, object]]]] = [dict() for _ in range(n_channels)]             # pitch -> [(time, score)] ascending

    # pitched key: walk_pitched_carry
    def _pitched(self, ch, key, items, starts, n_seg, score_of, finish, end_sec):
        out = []
        st = self.sounding[ch].get(key)
        active, on, score = st is not None, (st[0] if st else 0.0), (st[1] if st else None)
        if n_seg > 0:
            q = -1                                    # the previous push's last segment
            for it in sorted(items, key=lambda it: (it[0], it[1] != M.KIND_TIE, it[2], it[3], it[4])):
                s, tie = it[0], it[1] == M.KIND_TIE
                if active and s > q:
                    if tie and s == q + 1:
                        q = s
                        continue
                    if starts[q + 1] > on:
                        out.append((on, starts[q + 1], key[0], key[1], False, score))
                    active = False
                if tie:
                    continue
                t = starts[s] + it[2] / self.sps
                if it[3]:
                    if active and t > on:
                        out.append((on, t, key[0], key[1], False, score))
                    active, on, score, q = True, t, score_of(it), s
                elif active:
                    if t > on:
                        out.append((on, t, key[0], key[1], False, score))
                    active = False
            if active and q != n_seg - 1:
                if starts[q + 1] > on:
                    out.append((on, starts[q + 1], key[0], key[1], False, score))
                active = False
        if active and finish:
            if end_sec > on:
                out.append((on, end_sec, key[0], key[1], False, score))
            active = False
        if active:
            self.sounding[ch][key] = (on, score)
        else:
            self.sounding[ch].pop(key, None)
        return out

    # drum pitch: walk_drum_carry
    def _drum(self, ch, pitch, items, starts, score_of, horizon):
        t_of = lambda it: starts[it[0]] + it[2] / self.sps
        order = sorted(items, key=lambda it: (it[0], it[2], it[3], it[4]))
        order = sorted(order, key=t_of)               # stable: equal times stay in processing order
        held = self.held[ch].get(pitch, [])
        merged: List[Tuple[float, object]] = []
        i = j = 0
        while i < len(held) or j < len(order):
            tj = t_of(order[j]) if j < len(order) else 0.0
            take_held = i < len(held) and (j >= len(order) or held[i][0] <= tj)
            take_new = j < len(order) and (not take_held or tj == held[i][0])
            t = held[i][0] if take_held else tj
            sc = held[i][1] if take_held else score_of(order[j])
            if take_held:
                i += 1
            if take_new:
                if take_held and M._gt(score_of(order[j]), sc):
                    sc = score_of(order[j])
                j += 1
                while j < len(order) and t_of(order[j]) == t:
                    if M._gt(score_of(order[j]), sc):
                        sc = score_of(order[j])
                    j += 1
            merged.append((t, sc))
        below = sum(1 for t, _ in merged if t < horizon)
        forced = max(0, len(merged) - below - self.max_held)
        n_emit = below + forced
        self.held[ch][pitch] = merged[n_emit:]
        return [(t, t + 0.01, self.drum_program, pitch, True, sc) for t, sc in merged[:n_emit]], forced

    def _walk(self, buckets, starts, n_seg, scores, horizon, finish, end_sec):
        records, n_forced = [], 0
        for ch in range(self.K):
            def score_of(it, ch=ch):
                return None if scores is None else float(scores[it[0]][ch][it[4]])

            b = buckets[ch]
            keys = set(b) | set(self.sounding[ch]) | {(self.drum_program, p) for p, h in self.held[ch].items() if h}
            for key in sorted(keys):
                if key[0] == self.drum_program:
                    rec, f = self._drum(ch, key[1], b.get(key, []), starts, score_of, horizon)
                    records += rec
                    n_forced += f
                else:
                    records += self._pitched(ch, key, b.get(key, []), starts, n_seg, score_of, finish, end_sec)
        return records, n_forced

    def push(self, tokens, starts: Sequence[float], horizon_sec: float, scores=None):
        n = len(tokens)
        starts = [float(s) for s in starts]
        buckets = [dict() for _ in range(self.K)]
        n_invalid = 0
        for ch in range(self.K):
            for seg in range(n):
                items, bad = M.row_items(self.table, tokens[seg][ch], seg, self.drum_program)
                n_invalid += bad
                for it in items:
                    buckets[ch].setdefault((it[5], it[6]), []).append(it)
        records, n_forced = self._walk(buckets, starts, n, scores, float(horizon_sec), False, 0.0)
        return records, n_invalid, n_forced

    def finish(self, end_sec: float):
        records, n_forced = self._walk([dict() for _ in range(self.K)], [], 0, None, math.inf, True, float(end_sec))
        assert n_forced == 0
        return records, 0, 0
