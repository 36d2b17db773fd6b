"""The section rules of yourmt3_amd/sections.py (include/ymt3.h, sections) a third time, as plain loops over Python
integers: no numpy beyond reading the records, no vector operation, nothing shared with the specification.  The novelty is summed term by
term over the four quadrants, as the rules write it.  tests/test_sections_cpu.py holds the specification to it; it also counts the
candidates whose novelty equals another candidate's within min_len, so that the tie case can show that it has some."""
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
    return ok, drum


def track_sections(rec, beats, n_frames, metre, p):
    """-> (section list, novelty list, result list of 8, the number of tied candidates); `p`: every parameter (sections.check_params' dict)"""
    b = [int(v) for v in beats]
    K, nd, fps = len(b), p["near_div"], float(p["frames_per_second"])
    w, L, m, M = p["context"], p["kernel_beats"], p["min_len"], p["max_sections"]
    notes = [(float(r["onset"]), float(r["offset"]), int(r["program"]), int(r["pitch"]), int(r["is_drum"])) for r in rec]
    skipped = 0
    for on, off, program, pitch, is_drum in notes:
        if not _counted(on, off, program, pitch, is_drum, p["n_programs"], p["drum_program"])[0]:
            skipped += 1
    if K < 2:
        return [], [], [0, 0, 0, skipped, 0, 0, 0, 0], 0
    delta = [b[i + 1] - b[i] for i in range(K - 1)]
    delta.append(delta[K - 2])
    lo = [b[0] - delta[0] // nd] + [b[i] - delta[i - 1] // nd for i in range(1, K)]
    hi = [lo[i + 1] for i in range(K - 1)] + [b[K - 1] + delta[K - 1] - delta[K - 1] // nd]
    c = [[0] * 12 for _ in range(K)]
    for on, off, program, pitch, is_drum in notes:
        ok, drum = _counted(on, off, program, pitch, is_drum, p["n_programs"], p["drum_program"])
        if not ok or drum:
            continue
        f0, f_off = _frame(on, fps), _frame(off, fps)
        start, end = max(f0, 0.0), min(max(f_off, f0 + 1.0), float(n_frames))
        if not start < end:
            continue
        start, end = int(start), int(end)
        for i in range(K):
            share = min(end, hi[i]) - max(start, lo[i])
            if share > 0:
                c[i][pitch % 12] += share
    n = [[c[i][pc] * 1024 // max(sum(c[i]), 1) for pc in range(12)] for i in range(K)]
    empty = [sum(c[i]) == 0 for i in range(K)]
    f = [[sum(n[min(i + d, K - 1)][pc] for d in range(w)) for pc in range(12)] for i in range(K)]

    seen = {}

    def dist(i, j):
        if (i, j) not in seen:                              # (looked up again for every term it appears in)
            seen[i, j] = sum(abs(f[i][pc] - f[j][pc]) for pc in range(12))
        return seen[i, j]

    def sim(i, j):
        return 2048 * w - dist(i, j)

    nov = [0] * K
    for i in range(1, K):
        Li = min(L, i, K - i)
        total = 0
        for u in range(Li):
            for v in range(Li):
                total += (L - u) * (L - v) * (sim(i - 1 - u, i - 1 - v) + sim(i + u, i + v) - sim(i - 1 - u, i + v) - sim(i + u, i - 1 - v))
        nov[i] = total
    cand = [i for i in range(1, K) if metre is None or int(metre[i]) % 256 == 0]
    top = max([nov[j] for j in cand]) if cand else 0
    peaks, ties = [], 0
    for i in cand:
        beaten = False
        for j in cand:
            if 0 < abs(j - i) <= m:
                ties += nov[j] == nov[i] and nov[i] > 0
                if nov[j] > nov[i] or (nov[j] == nov[i] and j < i):
                    beaten = True
        if nov[i] > 0 and p["peak_div"] * nov[i] >= top and not beaten:
            peaks.append(i)
    kept = list(peaks)
    while len(kept) > M - 1:                                 # drop the smallest key (nov, -i): the smallest novelty, then the largest index
        worst = kept[0]
        for i in kept:
            if nov[i] < nov[worst] or (nov[i] == nov[worst] and i > worst):
                worst = i
        kept.remove(worst)
    starts = [0] + kept
    ends = starts[1:] + [K]
    labels, letters, n_silent = [], 0, 0
    for s in range(len(starts)):
        if all(empty[i] for i in range(starts[s], ends[s])):
            labels.append(255)
            n_silent += 1
            continue
        label = None
        for t in range(s):
            if labels[t] == 255:
                continue
            ls, lt = ends[s] - starts[s], ends[t] - starts[t]
            mst = min(ls, lt)
            if p["len_num"] * mst >= max(ls, lt) and sum(dist(starts[s] + k, starts[t] + k) for k in range(mst)) // mst <= p["same_dist"]:
                label = labels[t]
                break
        if label is None:
            label, letters = letters, letters + 1
        labels.append(label)
    section = []
    for s in range(len(starts)):
        for i in range(starts[s], ends[s]):
            section.append((65536 if i == starts[s] else 0) + 256 * s + labels[s])
    return section, nov, [len(starts), letters, top, skipped, len(peaks), n_silent, 0, 0], ties
