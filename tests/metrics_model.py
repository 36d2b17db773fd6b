"""The algorithm of yourmt3_amd/csrc/metrics.hip in plain Python (the specification is yourmt3_amd/metrics.py, which builds the whole hit
matrix and asks a library for the matching): records are keyed and bucketed, a key's buckets are sorted by onset, every reference gets
the interval of estimates it can hit by onset from two binary searches, the onset metric is a two-pointer walk, and the onset+offset
metric is Kuhn's algorithm over an explicit stack with per-search visited marks.  model_counts returns the device layout."""
import numpy as np

PITCHES = 128


def within(x: float, y: float, tol: float) -> bool:
    """d(x, y) <= tol, d = rint(|x - y| * 1e4) / 1e4 in f64; a NaN distance (inf - inf) misses"""
    return bool(np.rint(abs(x - y) * 1e4) / 1e4 <= tol)


def offset_tol(on: float, off: float, offset_min_tol: float, offset_ratio: float) -> float:
    t = offset_ratio * (off - on)
    return t if t > offset_min_tol else offset_min_tol


def buckets(rec, n_programs: int, drum_program: int):
    """-> ({key: [(onset, offset), ...]}, skipped): the aware key program * 128 + pitch, and for pitched notes n_programs * 128 + pitch"""
    out, skipped = {}, 0
    for on, off, program, pitch, is_drum in zip(rec["onset"].tolist(), rec["offset"].tolist(), rec["program"].tolist(), rec["pitch"].tolist(),
                                                rec["is_drum"].tolist()):
        prog = drum_program if is_drum != 0 else program
        drum = prog == drum_program
        if on != on or not 0 <= pitch < PITCHES or not 0 <= prog < n_programs or (not drum and off != off):
            skipped += 1
            continue
        out.setdefault(prog * PITCHES + pitch, []).append((on, off))
        if not drum:
            out.setdefault(n_programs * PITCHES + pitch, []).append((on, off))
    return out, skipped


def windows(R, E, onset_tol: float):
    """per reference of the sorted bucket R: [lo, hi) into the sorted bucket E -- before lo too early, from hi on too late"""
    win = []
    for on, _ in R:
        lo, h = 0, len(E)
        while lo < h:
            m = (lo + h) >> 1
            if E[m][0] < on and not within(on, E[m][0], onset_tol):
                lo = m + 1
            else:
                h = m
        l, h = lo, len(E)
        while l < h:
            m = (l + h) >> 1
            if E[m][0] > on and not within(on, E[m][0], onset_tol):
                h = m
            else:
                l = m + 1
        win.append((lo, l))
    return win


def onset_walk(R, E, win, onset_tol: float) -> int:
    """every reference in onset order takes the earliest free estimate of its interval"""
    tp = j = 0
    for (on, _), (lo, hi) in zip(R, win):
        j = max(j, lo)
        if j < hi and within(on, E[j][0], onset_tol):
            tp += 1
            j += 1
    return tp


def _both(r, e, onset_tol, offset_min_tol, offset_ratio) -> bool:
    return within(r[0], e[0], onset_tol) and within(r[1], e[1], offset_tol(r[0], r[1], offset_min_tol, offset_ratio))


def offset_kuhn(R, E, win, onset_tol, offset_min_tol, offset_ratio, limit=None) -> int:
    """augmenting paths, depth first, no recursion: a frame is [reference, next candidate]; visit[j] is the root that last saw j.
    `limit`: the onset matching's size, which an onset+offset matching cannot exceed -- the kernel stops searching once it is reached"""
    match, visit = [-1] * len(E), [-1] * len(E)
    tp = 0
    for root in range(len(R)):
        if tp == limit:
            break
        stack = [[root, win[root][0]]]
        while stack:
            u, c = stack[-1]
            hi = win[u][1]
            found = next((j for j in range(c, hi) if visit[j] != root and _both(R[u], E[j], onset_tol, offset_min_tol, offset_ratio)), -1)
            if found < 0:
                stack.pop()
                continue
            w = match[found]
            visit[found] = root
            stack[-1][1] = found + 1
            if w < 0:
                for fu, fc in stack:
                    match[fc - 1] = fu
                tp += 1
                break
            assert len(stack) < len(R)
            stack.append([w, win[w][0]])
    return tp


def offset_greedy(R, E, win, onset_tol, offset_min_tol, offset_ratio) -> int:
    """what a matching WITHOUT augmenting paths finds: every reference in onset order takes the earliest free estimate it hits"""
    used, tp = [False] * len(E), 0
    for r, (lo, hi) in zip(R, win):
        for j in range(lo, hi):
            if not used[j] and _both(r, E[j], onset_tol, offset_min_tol, offset_ratio):
                used[j] = True
                tp += 1
                break
    return tp


def keys_of(ref, est, n_programs, drum_program, onset_tol=0.05, offset_min_tol=0.05, offset_ratio=0.2):
    """-> [(key, R, E, win)] for the keys with notes on both sides, buckets sorted by onset; and the bucket dictionaries, the skip counts"""
    rb, rs = buckets(ref, n_programs, drum_program)
    eb, es = buckets(est, n_programs, drum_program)
    out = []
    for key in sorted(set(rb) & set(eb)):
        R, E = sorted(rb[key], key=lambda t: t[0]), sorted(eb[key], key=lambda t: t[0])
        out.append((key, R, E, windows(R, E, onset_tol)))
    return out, (rb, eb), (rs, es)


def model_counts(ref, est, n_programs, drum_program, onset_tol=0.05, offset_min_tol=0.05, offset_ratio=0.2) -> np.ndarray:
    keyed, sides, skipped = keys_of(ref, est, n_programs, drum_program, onset_tol, offset_min_tol, offset_ratio)
    counts = np.zeros((n_programs + 1, 2, 3), np.int32)
    for s, b in enumerate(sides):
        for key, items in b.items():
            counts[key // PITCHES, :, 1 + s] += len(items)
    for key, R, E, win in keyed:
        row = key // PITCHES
        tp = onset_walk(R, E, win, onset_tol)
        counts[row, 0, 0] += tp
        counts[row, 1, 0] += tp if row == drum_program else offset_kuhn(R, E, win, onset_tol, offset_min_tol, offset_ratio, limit=tp)
    return np.concatenate([counts.reshape(-1), np.asarray(skipped, np.int32)]).astype(np.int32)
