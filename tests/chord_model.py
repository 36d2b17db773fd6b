"""The chord rules of yourmt3_amd/chords.py (include/ymt3.h, chords) a third time, as plain loops over Python integers: no
numpy beyond reading the records, no vector operation, nothing shared with the specification but the table's values, which are written out
again here.  tests/test_chords_cpu.py holds the specification to it; it also counts the ties it meets among the best states, so that the
tie cases can show that they have some."""
import math

NAMES = ["maj", "min", "dim", "aug", "sus4", "7", "maj7", "min7"]
TONES = [[0, 4, 7], [0, 3, 7], [0, 3, 6], [0, 4, 8], [0, 5, 7], [0, 4, 7, 10], [0, 4, 7, 11], [0, 3, 7, 10]]


def _frame(t, fps):
    """rint(t fps) as a float: half to even, +-inf kept"""
    x = t * fps
    if math.isinf(x) or math.isnan(x):
        return x
    return float(round(x))                                  # Python's round is half to even


def _counted(on, off, program, pitch, is_drum, n_programs, drum_program):
    """-> (counted, drum)"""
    prog = drum_program if is_drum != 0 else program
    drum = prog == drum_program
    ok = not math.isnan(on) and 0 <= pitch < 128 and 0 <= prog < n_programs and (drum or not math.isnan(off))
    return ok, drum


def track_chords(rec, beats, n_frames, metre, p):
    """-> (chord list, result list of 8, the number of beats whose best state was tied); `p`: every parameter (chords.check_params' dict)"""
    b = [int(v) for v in beats]
    K, nd, fps = len(b), p["near_div"], float(p["frames_per_second"])
    notes = [(float(r["onset"]), float(r["offset"]), int(r["program"]), int(r["pitch"]), int(r["is_drum"])) for r in rec]
    skipped = 0
    for on, off, program, pitch, is_drum in notes:
        if not _counted(on, off, program, pitch, is_drum, p["n_programs"], p["drum_program"])[0]:
            skipped += 1
    if K < 2:
        return [], [0, 0, 0, skipped, 0, 0, 0, 0], 0
    delta = [b[i + 1] - b[i] for i in range(K - 1)]
    delta.append(delta[K - 2])
    lo = [b[0] - delta[0] // nd] + [b[i] - delta[i - 1] // nd for i in range(1, K)]
    hi = [lo[i + 1] for i in range(K - 1)] + [b[K - 1] + delta[K - 1] - delta[K - 1] // nd]
    c = [[0] * 12 for _ in range(K)]
    bass = [255] * K
    for on, off, program, pitch, is_drum in notes:
        ok, drum = _counted(on, off, program, pitch, is_drum, p["n_programs"], p["drum_program"])
        if not ok or drum:
            continue
        f, f_off = _frame(on, fps), _frame(off, fps)
        start, end = max(f, 0.0), min(max(f_off, f + 1.0), float(n_frames))
        if not start < end:
            continue
        start, end = int(start), int(end)
        for i in range(K):
            share = min(end, hi[i]) - max(start, lo[i])
            if share > 0:
                c[i][pitch % 12] += share
                if p["bass_div"] * share >= hi[i] - lo[i] and pitch < bass[i]:
                    bass[i] = pitch
    states = [(NAMES.index(name), r) for name in p["qualities"] for r in range(12)]
    S = len(states) + 1
    e = []
    for i in range(K):
        total = max(sum(c[i]), 1)
        n = [c[i][pc] * 1024 // total for pc in range(12)]
        row = []
        for q, r in states:
            v = (591 if len(TONES[q]) == 3 else 512) * sum(n[(r + s) % 12] for s in TONES[q])
            if bass[i] < 128 and bass[i] % 12 == r:
                v += 1024 * p["w_bass"]
            row.append(v)
        row.append(1024 * p["w_none"])
        e.append(row)
    V = list(e[0])
    came = [[s for s in range(S)]]
    ties = 0
    for i in range(1, K):
        top = max(V)
        best = V.index(top)                                  # the first of them
        ties += V.count(top) > 1
        down = metre is not None and int(metre[i]) % 256 == 0
        jump = top - 1024 * (p["change_cost_down"] if down else p["change_cost"])
        new, row = [], []
        for s in range(S):
            if V[s] >= jump:
                new.append(V[s] + e[i][s])
                row.append(s)
            else:
                new.append(jump + e[i][s])
                row.append(best)
        V = new
        came.append(row)
    top = max(V)
    ties += V.count(top) > 1
    s = V.index(top)
    path = [0] * K
    for i in range(K - 1, -1, -1):
        path[i] = s
        s = came[i][s]
    label = [255 if s == S - 1 else 12 * states[s][0] + states[s][1] for s in path]
    runs = 1
    for i in range(1, K):
        if label[i] != label[i - 1]:
            runs += 1
    return [256 * bass[i] + label[i] for i in range(K)], [runs, top, label.count(255), skipped, 0, 0, 0, 0], ties
