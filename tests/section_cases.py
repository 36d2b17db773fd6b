"""Case sets for the section tracker (tests/test_sections_cpu.py, tests/test_sections.py): NOTE_RECORD arrays, beats, frame counts, metres
and parameter sets, all small.  A case: (name, records, beats int32, n_frames, metre int32 or None, params, count) with `count` the
device count to pass (None: all records).  The known music is generated here in chord_cases' style: every section has its own chord
loop; its beats are the beat tracker's own (beats.track_beats) and its metre the bar tracker's (bars.track_bars), found once."""
import functools

import numpy as np

import bar_cases as BC
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T

FPS = BC.FPS
TILE = 64                                                                   # the novelty kernel's tile (csrc/sections.hip, SECTION_TILE)
SECOND = dict(near_div=3, context=3, kernel_beats=5, min_len=3, peak_div=9, same_dist=900, len_num=3, max_sections=7)
MAJ, MIN = (0, 4, 7), (0, 3, 7)
C, D, E, F, G, A, Bb = 0, 2, 4, 5, 7, 9, 10
# A section's loop: [(root, tones)], four chords that share the section's beats equally and fall by thirds.  Inside a loop neighbouring
# chords share two tones; a loop's last chord shares none with its own first chord or with A's, and at most one with the next loop's: a
# section's start is a stronger change of harmony than anything inside a section.
LOOP_A = [(C, MAJ), (A, MIN), (F, MAJ), (D, MIN)]
LOOP_B = [(A, MAJ), (6, MIN), (D, MAJ), (11, MIN)]
LOOP_C = [(6, MAJ), (3, MIN), (11, MAJ), (8, MIN)]
LOOP_A_REORDERED = [(F, MAJ), (D, MIN), (C, MAJ), (A, MIN)]                   # A's chords in another order: its halves swapped
FORMS = {
    "AABA": [("A", LOOP_A, 16), ("A", LOOP_A, 16), ("B", LOOP_B, 16), ("A", LOOP_A, 16)],
    "ABAB": [("A", LOOP_A, 16), ("B", LOOP_B, 16), ("A", LOOP_A, 16), ("B", LOOP_B, 16)],
    "ABCA": [("A", LOOP_A, 32), ("B", LOOP_B, 16), ("C", LOOP_C, 16), ("A", LOOP_A, 32)],
    "ABAB_reordered": [("A", LOOP_A, 16), ("B", LOOP_A_REORDERED, 16), ("A", LOOP_A, 16), ("B", LOOP_A_REORDERED, 16)],
    "A_silence_A": [("A", LOOP_A, 16), ("N", None, 16), ("A", LOOP_A, 16)],
}


def form(sections, clean=False, seed=0, bpm=100.0, first=0.6):
    """Known music -> (records, n_frames, [(the section's first beat's time, its letter, its beats)]).  `sections`: [(letter, loop,
    beats)], loop None for silence.  The chord's tones on every beat and a drum on every beat; unless
    `clean`, an off-beat melody note on 60 % of the beats and 10 ms jitter."""
    rng = np.random.default_rng(3100 + seed)
    period = 60.0 / bpm
    jit = (lambda: 0.0) if clean else (lambda: float(rng.normal(0, 0.01)))
    rows, truth, t = [], [], first
    for letter, loop, n in sections:
        truth.append((t, letter, n))
        for k in range(n):
            rows.append((t + jit(), t + 0.01, 128, 36 if k % 2 == 0 else 38, True))
            if loop is not None:
                root, tones = loop[k // (n // len(loop))]
                for s in tones:
                    rows.append((t + jit(), t + 0.8 * period, 0, 60 + (root + s) % 12, False))
                if not clean and rng.random() < 0.6:
                    pc = int(rng.integers(0, 12)) if rng.random() < 0.3 else (root + tones[int(rng.integers(0, 3))]) % 12
                    rows.append((t + period / 2 + jit(), t + 0.75 * period, 0, 72 + pc, False))
            t += period
    return BC._rec(rows), int(round((t + 0.6) * FPS)), truth


@functools.lru_cache(maxsize=None)
def music(name, clean=False):
    """-> (records, beats int32, n_frames, the bar tracker's metre, the truth)"""
    rec, n_frames, truth = form(FORMS[name], clean, seed=sorted(FORMS).index(name))
    beats = T.track_beats(rec, n_frames)[0]
    return rec, beats, n_frames, B.track_bars(rec, beats, n_frames)[0], truth


MUSIC = tuple(FORMS)


def musical_cases():
    return [(name, *music(name)[:4], {}, None) for name in MUSIC] + [(name + "_clean", *music(name, True)[:4], {}, None) for name in ("AABA", "ABAB")]


def truth_beats(beats, truth, tol=0.07):
    """-> [(the tracked beat nearest the section's start, its letter)]; a start with no beat within `tol` gives None"""
    sec = np.asarray(beats, np.float64) / FPS
    out = []
    for t, letter, _ in truth:
        j = int(np.argmin(np.abs(sec - t)))
        out.append((j if abs(sec[j] - t) <= tol else None, letter))
    return out


def agreement(section, beats, truth):
    """-> (boundary hits, boundaries, beats whose letters agree, beats compared): a generated boundary (not the piece's start) is hit if a
    tracked section starts within 2 beats of it; the letters agree on a beat if the tracked letters partition the compared beats as the
    truth's do, under the best one-to-one renaming found greedily by overlap"""
    section = np.asarray(section)
    starts = np.flatnonzero(section >> 16)
    marks = truth_beats(beats, truth)
    wanted = [j for j, _ in marks[1:] if j is not None]
    hits = sum(1 for j in wanted if starts.size and int(np.min(np.abs(starts - j))) <= 2)
    sec = np.asarray(beats, np.float64) / FPS
    times = [t for t, _, _ in truth] + [truth[-1][0] + truth[-1][2] * (truth[1][0] - truth[0][0]) / truth[0][2]]
    got, want = [], []
    for i, t in enumerate(sec.tolist()):
        s = int(np.searchsorted(times, t + 0.07, side="right")) - 1
        if 0 <= s < len(truth):
            got.append(int(section[i]) & 255)
            want.append(truth[s][1])
    pairs = sorted({(g, w) for g, w in zip(got, want)}, key=lambda gw: -sum(1 for g, w in zip(got, want) if (g, w) == gw))
    name, used = {}, set()
    for g, w in pairs:
        if g not in name and w not in used:
            name[g] = w
            used.add(w)
    return hits, len(wanted), sum(1 for g, w in zip(got, want) if name.get(g) == w), len(got)


def _filler(seconds, seed=7):
    rng = np.random.default_rng(seed)
    n = int(seconds * 6)
    return BC.records(rng.uniform(0.0, seconds, n), pitch=rng.integers(36, 84, n), length=rng.uniform(0.1, 1.5, n))


def blocks(k, block=8, step=50):
    """k steady beats, one pitch class per block of `block` beats (a new one each block): a novelty peak at every block's start"""
    on = 0.5 + step / FPS * np.arange(k)
    return BC.records(on, pitch=60 + (np.arange(k) // block * 5) % 12, length=0.8 * step / FPS), BC.steady(k, 50, step), 50 + step * k + 50


def edge_cases():
    out = []
    fill = _filler(80.0)
    for k in (0, 1, 2, 3, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):              # nothing, below L, the novelty tile's edges
        out.append((f"beats{k}", fill, BC.steady(k, 60, 60), 8000, None if k % 2 else (1024 + np.arange(k) % 4).astype(np.int32), {}, None))
    out.append(("kernel64_full", fill, BC.steady(140, 60, 50), 8000, None, dict(kernel_beats=64, context=16), None))      # whole 128-row windows, three tiles
    aaba = music("AABA")
    abca = music("ABCA")
    for name, p in (("kernel2", dict(kernel_beats=2)), ("kernel64", dict(kernel_beats=64)), ("context1", dict(context=1)), ("context16", dict(context=16)),
                    ("min_len1", dict(min_len=1)), ("min_len256", dict(min_len=256)), ("peak_div1", dict(peak_div=1)),
                    ("same_dist0", dict(same_dist=0)), ("same_dist_max", dict(same_dist=32768, len_num=16))):
        out.append((name, *abca[:4], p, None))
    rec, b, n_frames = blocks(200, block=2)
    for M in (1, 2, 64):                                                            # 99 block starts: more peaks than M - 1 for every M
        out.append((f"cap{M}", rec, b, n_frames, None, dict(max_sections=M, min_len=1, peak_div=1024, kernel_beats=2, context=1), None))
    out.append(("mirrored_ties", *tie_piece(), None, dict(min_len=64, peak_div=1, context=1, kernel_beats=4), None))
    out.append(("metre_no_candidate", *aaba[:3], (1024 + 1 + np.arange(aaba[1].size) % 3).astype(np.int32), {}, None))
    one = (1024 + 1 + np.arange(aaba[1].size) % 3).astype(np.int32)
    one[33] = 1024
    out.append(("metre_one_downbeat", *aaba[:3], one, {}, None))
    drums = BC.records(0.5 + 0.25 * np.arange(60), pitch=np.tile([36, 42, 38, 42], 15), program=128, drum=True)
    out.append(("drums_only", drums, BC.steady(31), 1700, None, {}, None))
    skipped = BC.records(0.5 + 0.5 * np.arange(20), pitch=200)
    out.append(("all_skipped", skipped, BC.steady(20), 1200, None, {}, None))
    out.append(("no_records", BC.records([]), BC.steady(12), 700, None, {}, None))
    bad = next(c for c in BC.edge_cases() if c[0] == "nonfinite_and_out_of_range")
    out.append(("nonfinite_and_out_of_range", bad[1], bad[2], bad[3], None, {}, None))
    out.append(("count_below_n", *aaba[:4], {}, 150))
    out.append(("count_zero", *aaba[:4], {}, 0))
    out.append(("second_params", *abca[:4], SECOND, None))
    out.append(("second_params_random", *BC._random(5), None, SECOND, None))
    rng = np.random.default_rng(97)                                                 # 1024 records in random order, ten tiles of beats
    many = BC.records(rng.uniform(-1.0, 68.0, 1024), pitch=rng.integers(28, 96, 1024), length=rng.uniform(0.05, 4.0, 1024))
    many["is_drum"][::9], many["pitch"][::9] = 1, 36
    out.append(("records_1024", many, BC.steady(600, 5, 11), 6700, (768 + np.arange(600) % 3).astype(np.int32), {}, None))
    return out


def tie_piece():
    """one pitch class per block of 6 steady beats, the blocks' pitch classes a palindrome: the piece is its own mirror image, so the
    novelties at i and K - i are equal and the earlier index must win -> (records, beats, n_frames)"""
    pcs = [0, 5, 10, 5, 0]
    k = 6 * len(pcs)
    on = 0.5 + 0.5 * np.arange(k)
    return BC.records(on, pitch=60 + np.repeat(pcs, 6), length=0.3), BC.steady(k), 50 + 50 * k + 50       # (every note inside its own slot)


def random_cases():
    out = []
    for seed in range(12):
        rec, b, frames = BC._random(seed)
        rng = np.random.default_rng(6000 + seed)
        metre = (256 * 4 + rng.integers(0, 4, b.size)).astype(np.int32) if seed % 2 else None
        out.append((f"random{seed}", rec, b, frames, metre, {}, None))
    return out


TIE_CASES = ("mirrored_ties",)


def all_cases():
    return musical_cases() + edge_cases() + random_cases()


live = BC.live
