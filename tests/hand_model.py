"""The hand rules of yourmt3_amd/hands.py (include/ymt3.h, hands) a third time, as plain loops over Python integers:
no numpy beyond reading the records, no vector operation, nothing shared with the specification.  Every state's left and right hand are
formed as lists, every transition is tried.  tests/test_hands_cpu.py holds the specification to it; it also counts the steps whose
minimum is reached from more than one s', so that the tie case can show that it has some."""
import math


def _frame(t, fps):
    x = t * fps
    if math.isinf(x) or math.isnan(x):
        return x
    return float(round(x))                                  # Python's round is half to even


def _counted(on, off, program, pitch, is_drum, n_programs, drum_program):
    prog = drum_program if is_drum != 0 else program
    drum = prog == drum_program
    ok = not math.isnan(on) and 0 <= pitch < 128 and 0 <= prog < n_programs and (drum or not math.isnan(off))
    return ok, drum, prog


def _hands(pitches, s):
    return [x for x in pitches if x < s], [x for x in pitches if x >= s]


def _class(pitches, s):
    left, right = _hands(pitches, s)
    return 0 if not left else 2 if not right else 1


def _emission(pitches, s, p):
    left, right = _hands(pitches, s)
    span = lambda xs: max(xs) - min(xs) if xs else 0
    e = p["w_span"] * (max(0, span(left) - p["span"]) + max(0, span(right) - p["span"]))
    if left and right:
        e += p["w_cut"] * max(0, p["cut_min"] - (min(right) - max(left))) + p["w_centre"] * (abs(2 * s - (max(left) + min(right) + 1)) // 2)
    return e + p["w_mid"] * max(0, abs(s - p["middle"]) - p["mid_free"])


def split_hands(rec, n_frames, p):
    """-> (hand list, split list, result list of 8, the number of tied steps); `p`: every parameter (hands.check_params' dict)"""
    fps = float(p["frames_per_second"])
    skipped, chosen = 0, []                                 # chosen: (record, slot, pitch)
    for i, r in enumerate(rec):
        on, off, pitch = float(r["onset"]), float(r["offset"]), int(r["pitch"])
        ok, drum, prog = _counted(on, off, int(r["program"]), pitch, int(r["is_drum"]), p["n_programs"], p["drum_program"])
        if not ok:
            skipped += 1
            continue
        if drum or not p["program_lo"] <= prog <= p["program_hi"]:
            continue
        f0, f_off = _frame(on, fps), _frame(off, fps)
        start, end = max(f0, 0.0), min(max(f_off, f0 + 1.0), float(n_frames))
        if start < end:
            chosen.append((i, int(start) // p["slice_frames"], pitch))
    hand = [255] * len(rec)
    if not chosen:
        return hand, [], [0, 0, 0, 0, 0, skipped, 0, 0], 0
    slots = sorted({q for _, q, _ in chosen})
    sets = [sorted({x for _, q, x in chosen if q == slot}) for slot in slots]
    T = len(slots)
    cost = [_emission(sets[0], s, p) for s in range(129)]
    back, ties = [None], 0
    for t in range(1, T):
        rest = slots[t] - slots[t - 1] >= p["rest_slots"]
        before = [_class(sets[t - 1], s) for s in range(129)]
        new, row = [], []
        for s in range(129):
            now = _class(sets[t], s)
            best, arg, n_best = None, None, 0
            for s0 in range(129):
                x = 0 if rest else p["w_move"] * abs(s - s0) + (p["w_switch"] if {before[s0], now} == {0, 2} else 0)
                v = cost[s0] + x
                if best is None or v < best:
                    best, arg, n_best = v, s0, 1
                elif v == best:
                    n_best += 1
            ties += n_best > 1
            new.append(best + _emission(sets[t], s, p))
            row.append(arg)
        cost = new
        back.append(row)
    total = min(cost)
    path = [0] * T
    path[T - 1] = cost.index(total)
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t][path[t]]
    overs = 0
    for t in range(1, T):
        if slots[t] - slots[t - 1] < p["rest_slots"] and {_class(sets[t - 1], path[t - 1]), _class(sets[t], path[t])} == {0, 2}:
            overs += 1
    left = right = 0
    for i, q, x in chosen:
        hand[i] = 1 if x >= path[slots.index(q)] else 0
        right += hand[i]
        left += 1 - hand[i]
    return hand, [256 * q + s for q, s in zip(slots, path)], [T, len(chosen), left, right, total, skipped, overs, 0], ties
