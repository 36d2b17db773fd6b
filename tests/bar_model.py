"""The bar and key rules of yourmt3_amd/bars.py (include/ymt3.h, bars and key) a third time, as plain loops over Python
integers: no numpy beyond reading the records, no vector operation, nothing shared with the specification but the two key tables' values,
which are written out again here.  tests/test_bars_cpu.py holds the specification to it; it also counts the ties it meets, so that the tie
cases can show that they have some."""
import math

MAJOR = [671, -293, -1, -270, 210, 142, -225, 400, -256, 42, -279, -141]
MINOR = [671, -263, -48, 428, -284, -46, -299, 266, 69, -261, -94, -138]


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


def track_bars(rec, beats, n_frames, p):
    """-> (metre list, result list of 8, the number of ties met); `p`: every parameter (bars.check_params' dict)"""
    b = [int(v) for v in beats]
    K, nd, fps = len(b), p["near_div"], float(p["frames_per_second"])
    notes = [(float(r["onset"]), float(r["offset"]), int(r["program"]), int(r["pitch"]), int(r["is_drum"])) for r in rec]
    skipped = 0
    for on, off, program, pitch, is_drum in notes:
        if not _counted(on, off, program, pitch, is_drum, p["n_programs"], p["drum_program"])[0]:
            skipped += 1
    if K < 2:
        return [], [0, 0, 0, -1, 0, 0, skipped, 0], 0
    delta = [b[i + 1] - b[i] for i in range(K - 1)]
    delta.append(delta[K - 2])
    lo = [b[0] - delta[0] // nd] + [b[i] - delta[i - 1] // nd for i in range(1, K)]
    hi = [lo[i + 1] for i in range(K - 1)] + [b[K - 1] + delta[K - 1] - delta[K - 1] // nd]
    a = [0] * K
    c = [[0] * 12 for _ in range(K)]
    for on, off, program, pitch, is_drum in notes:
        ok, drum = _counted(on, off, program, pitch, is_drum, p["n_programs"], p["drum_program"])
        if not ok:
            continue
        f = _frame(on, fps)
        f_off = None if drum else _frame(off, fps)
        if not math.isinf(f):
            for i in range(K):
                if lo[i] <= f < hi[i] and f <= b[i] + delta[i] // nd:
                    a[i] += 1
                    if drum and p["kick_lo"] <= pitch <= p["kick_hi"]:
                        a[i] += p["w_kick"]
                    if not drum and f_off - f >= delta[i]:
                        a[i] += p["w_long"]
        if drum:
            continue
        start, end = max(f, 0.0), min(max(f_off, f + 1.0), float(n_frames))
        if not start < end:
            continue
        start, end = int(start), int(end)
        for i in range(K):
            share = min(end, hi[i]) - max(start, lo[i])
            if share > 0:
                c[i][pitch % 12] += share
    d = []
    for i in range(K):
        h = 0
        if i > 0:
            now, before = sum(c[i]), sum(c[i - 1])
            if now > 0 and before > 0:
                for pc in range(12):
                    h += abs(c[i][pc] * 1024 // now - c[i - 1][pc] * 1024 // before)
        d.append(p["w_accent"] * min(a[i], p["accent_cap"]) + h)
    mean_d = sum(d) // K
    penalty = p["switch_cost"] * 60 * mean_d
    metres = list(p["metres"])
    ties = 0

    def reward(i, m, k):
        return (60 // m) * (m - 1) * d[i] if k == 0 else -(60 // m) * d[i]

    V = [{(m, k): reward(0, m, k) for m in metres for k in range(m)}]
    came = [{}]
    for i in range(1, K):
        row, back = {}, {}
        for m in metres:
            for k in range(1, m):
                row[m, k] = V[i - 1][m, k - 1] + reward(i, m, k)
            best, source = V[i - 1][m, m - 1], m
            for other in metres:
                if other == m:
                    continue
                value = V[i - 1][other, other - 1] - penalty
                if value > best:
                    best, source = value, other
                elif value == best:
                    ties += 1
            row[m, 0], back[m] = best + reward(i, m, 0), source
        V.append(row)
        came.append(back)
    top, state = None, None
    for m in metres:
        for k in range(m):
            if top is None or V[K - 1][m, k] > top:
                top, state = V[K - 1][m, k], (m, k)
            elif V[K - 1][m, k] == top:
                ties += 1
    metre = [0] * K
    downbeats = 0
    for i in range(K - 1, -1, -1):
        m, k = state
        metre[i] = 256 * m + k
        if k == 0:
            downbeats += 1
            if i > 0:
                source = came[i][m]
                state = (source, source - 1)
        else:
            state = (m, k - 1)
    tot = [sum(c[i][pc] for i in range(K)) for pc in range(12)]
    key, best, second = -1, 0, 0
    if sum(tot) > 0:
        scores = []
        for table in (MAJOR, MINOR):
            for t in range(12):
                scores.append(sum(tot[pc] * table[(pc - t) % 12] for pc in range(12)))
        key = 0
        for j in range(1, 24):
            if scores[j] > scores[key]:
                key = j
        best = scores[key]
        ties += sum(1 for j in range(24) if j != key and scores[j] == best)
        second = max(scores[j] for j in range(24) if j != key)
    return metre, [downbeats, top, mean_d, key, best, second, skipped, 0], ties
