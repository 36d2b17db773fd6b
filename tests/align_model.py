"""The rules of the alignment (include/ymt3.h, alignment), stated independently of yourmt3_amd/metrics.py: plain
Python loops over frames and over every cell of the rectangle, Python integers and sets, no numpy arithmetic.  It shares no code with the
specification it checks (the sounding cells come from tests/roll_model.py, the piano roll's own plain model).  For small cases only:
it visits all Na x Nb cells."""
import math

from roll_model import cells_of

INF = 1 << 30


def features(rec, n_frames, n_programs, drum_program, fps):
    """-> (per frame a frozenset of (half, pitch): half 0 the agnostic row, half 1 the drum row; skipped records)"""
    cells, skipped = cells_of(rec, n_frames, n_programs, drum_program, fps)
    frames = [set() for _ in range(n_frames)]
    for row, frame, pitch in cells:
        if row == n_programs:
            frames[frame].add((0, pitch))
        elif row == drum_program:
            frames[frame].add((1, pitch))
    return [frozenset(f) for f in frames], skipped


def in_band(i, j, na, nb, band):
    q, p = na - 1, nb - 1
    return abs(i * p - j * q) <= band * max(p, q, 1)


def table(ref, est, na, nb, n_programs, drum_program, fps, band):
    """-> (D as a list of rows, the steps as a list of rows (0 diagonal, 1 (i-1, j), 2 (i, j-1)), skipped (ref, est))"""
    fr, sr = features(ref, na, n_programs, drum_program, fps)
    fe, se = features(est, nb, n_programs, drum_program, fps)
    D = [[INF] * nb for _ in range(na)]
    S = [[0] * nb for _ in range(na)]
    for i in range(na):
        for j in range(nb):
            if not in_band(i, j, na, nb, band):
                continue
            cost = len(fr[i] ^ fe[j])
            if i == 0 and j == 0:
                D[0][0] = cost
                continue
            at = lambda a, b: D[a][b] if a >= 0 and b >= 0 else INF
            preds = (at(i - 1, j - 1), at(i - 1, j), at(i, j - 1))
            best = min(preds)
            S[i][j] = preds.index(best)                                  # the first that equals the minimum
            D[i][j] = min(best + cost, INF)
    return D, S, (sr, se)


def align(ref, est, na, nb, n_programs, drum_program, fps, band):
    """-> (total, path as a list of (i, j), warp as a list, skipped (ref, est))"""
    D, S, skipped = table(ref, est, na, nb, n_programs, drum_program, fps, band)
    total = D[na - 1][nb - 1]
    if total >= INF:
        return INF, [], [-1] * na, skipped
    i, j, path = na - 1, nb - 1, []
    while True:
        path.append((i, j))
        if (i, j) == (0, 0):
            break
        s = S[i][j]
        if s != 2:
            i -= 1
        if s != 1:
            j -= 1
    path.reverse()
    warp = [min(b for a, b in path if a == i) for i in range(na)]
    return total, path, warp, skipped


def reachable(na, nb, band):
    """-> the set of in-band cells that a monotone path from (0, 0) reaches through in-band cells"""
    seen = set()
    for i in range(na):
        for j in range(nb):
            if in_band(i, j, na, nb, band) and ((i, j) == (0, 0) or (i - 1, j - 1) in seen or (i - 1, j) in seen or (i, j - 1) in seen):
                seen.add((i, j))
    return seen


def warp_time(t, warp, fps):
    """W(t): Python floats are f64 and every operation below rounds once"""
    q = len(warp) - 1
    x = t * fps
    if math.isnan(x):
        return x
    k = 0.0 if x == -math.inf else (float(q) if x == math.inf else float(math.floor(x)))
    k = min(max(k, 0.0), float(q))
    f = min(max(x - k, 0.0), 1.0)
    a, b = warp[int(k)], warp[min(int(k) + 1, q)]
    return (a + f * (b - a)) / fps
