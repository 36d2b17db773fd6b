"""Case sets for the chord tracker (tests/test_chords_cpu.py, tests/test_chords.py): NOTE_RECORD arrays, beats, frame counts, metres and
parameter sets, all small.  A case: (name, records, beats int32, n_frames, metre int32 or None, params, count) with `count` the device
count to pass (None: all records).  The known music is bar_cases' twelve pieces (a major triad on ROOTS[bar]) and six progressions
generated here in the same style; its beats are the beat tracker's own (beats.track_beats) and its metre the bar tracker's
(bars.track_bars), found once."""
import functools

import numpy as np

import bar_cases as BC
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T

FPS = BC.FPS
MAJ, MIN, DIM, AUG, SUS4, DOM7, MAJ7, MIN7 = range(8)
TONES = ((0, 4, 7), (0, 3, 7), (0, 3, 6), (0, 4, 8), (0, 5, 7), (0, 4, 7, 10), (0, 4, 7, 11), (0, 3, 7, 10))
SECOND = dict(near_div=3, qualities=("min7", "maj", "dim"), bass_div=3, w_bass=200, w_none=100, change_cost=40, change_cost_down=90)


def progression(chords, seed=0, bpm=100.0, first=0.6):
    """Known music -> (records, n_frames, [(beat time, label)]).  `chords`: [(root, quality, bass tone index, beats)], root None for
    silence.  The chord's tones on every beat, a long bass note on each change (the root, or the inversion's tone), a drum on every beat,
    an off-beat melody note on 60 % of the beats that is a random pitch class 30 % of the time (else a chord tone), 10 ms jitter."""
    rng = np.random.default_rng(2600 + seed)
    period = 60.0 / bpm
    jit = lambda: float(rng.normal(0, 0.01))
    rows, truth, t = [], [], first
    for root, quality, inversion, n in chords:
        if root is not None:
            tones = TONES[quality]
            rows.append((t + jit(), t + n * period * 0.95, 0, 36 + (root + tones[inversion]) % 12, False))
        for k in range(n):
            truth.append((t, 255 if root is None else 12 * quality + root))
            rows.append((t + jit(), t + 0.01, 128, 36 if k % 2 == 0 else 38, True))
            if root is not None:
                for s in tones:
                    rows.append((t + jit(), t + 0.8 * period, 0, 60 + (root + s) % 12, False))
                if rng.random() < 0.6:
                    pc = int(rng.integers(0, 12)) if rng.random() < 0.3 else (root + tones[int(rng.integers(0, len(tones)))]) % 12
                    rows.append((t + period / 2 + jit(), t + 0.75 * period, 0, 72 + pc, False))
            t += period
    return BC._rec(rows), int(round((t + 0.6) * FPS)), truth


C, D, E, F, G, A, Bb, Bn = 0, 2, 4, 5, 7, 9, 10, 11
PROGRESSIONS = {
    "pop": [(C, MAJ, 0, 4), (A, MIN, 0, 4), (F, MAJ, 0, 4), (G, MAJ, 0, 4)] * 4,
    "jazz": [(D, MIN7, 0, 4), (G, DOM7, 0, 4), (C, MAJ7, 0, 4), (A, MIN7, 0, 4)] * 4,
    "mixed": [(C, MAJ, 0, 4), (C, SUS4, 0, 2), (C, MAJ, 0, 2), (Bn, DIM, 0, 4), (E, DOM7, 0, 4), (A, MIN, 0, 4), (F, MAJ7, 0, 4), (G, SUS4, 0, 2),
              (G, MAJ, 0, 2), (C, AUG, 0, 4), (F, MAJ, 0, 4), (D, DIM, 0, 2), (G, DOM7, 0, 2), (C, MAJ7, 0, 4), (A, MIN, 0, 2), (D, DOM7, 0, 2),
              (G, MAJ, 0, 4), (C, MAJ, 0, 4), (E, AUG, 0, 2), (A, MIN, 0, 2)],
    "inversions": [(C, MAJ, 1, 4), (F, MAJ, 1, 4), (G, MAJ, 1, 4), (C, MAJ, 2, 4), (A, MIN, 1, 4), (D, MIN, 2, 4), (G, MAJ, 2, 4), (C, MAJ, 0, 4)] * 2,
    "silence": [(C, MAJ, 0, 4), (F, MAJ, 0, 4), (G, MAJ, 0, 4), (A, MIN, 0, 4), (None, 0, 0, 8), (F, MAJ, 0, 4), (G, MAJ, 0, 4), (C, MAJ, 0, 4), (C, MAJ, 0, 4)],
    "fast_changes": [(C, MAJ, 0, 2), (G, MAJ, 0, 2), (A, MIN, 0, 1), (F, MAJ, 0, 1), (G, MAJ, 0, 2), (C, MAJ, 0, 1), (E, MIN, 0, 1), (F, MAJ, 0, 2),
                     (D, MIN, 0, 1), (G, MAJ, 0, 1), (C, MAJ, 0, 2)] * 3,
}


def known_truth(name):
    """bar_cases.piece's beats again -> [(beat time, label)]: a major triad on ROOTS[bar]"""
    kw = BC.KNOWN[name][0]
    bars, pickup, period = kw["bars"], kw.get("pickup", 0), 60.0 / kw.get("bpm", 100.0)
    layout = [-1] * pickup + [n for n, m in enumerate(bars) for _ in range(m)]
    return [(0.6 + i * period, BC.ROOTS[max(bar, 0) % len(BC.ROOTS)]) for i, bar in enumerate(layout)]


@functools.lru_cache(maxsize=None)
def music(name):
    """-> (records, beats int32, n_frames, the bar tracker's metre, [(beat time, label)])"""
    if name in BC.KNOWN:
        rec, beats, n_frames = BC.known(name)[:3]
        truth = known_truth(name)
    else:
        rec, n_frames, truth = progression(PROGRESSIONS[name], seed=sorted(PROGRESSIONS).index(name))
        beats = T.track_beats(rec, n_frames)[0]
    return rec, beats, n_frames, B.track_bars(rec, beats, n_frames)[0], truth


MUSIC = tuple(BC.KNOWN) + tuple(PROGRESSIONS)


def musical_cases():
    return [(name, *music(name)[:4], {}, None) for name in MUSIC]


def accuracy(chord, beats, truth, tol=0.07):
    """-> (hits, beats compared): the tracked beats within `tol` of a generated beat, and those of them that carry its label"""
    times = np.array([t for t, _ in truth])
    hits = n = 0
    for b, v in zip(np.asarray(beats).tolist(), np.asarray(chord).tolist()):
        j = int(np.argmin(np.abs(times - b / FPS)))
        if abs(times[j] - b / FPS) <= tol:
            n += 1
            hits += (v & 255) == truth[j][1]
    return hits, n


def _filler(seconds, seed=7):
    """chords and a melody over `seconds`, seeded: content for the steady-beat cases"""
    rng = np.random.default_rng(seed)
    n = int(seconds * 6)
    return BC.records(rng.uniform(0.0, seconds, n), pitch=rng.integers(36, 84, n), length=rng.uniform(0.1, 1.5, n))


def edge_cases():
    out = []
    fill = _filler(80.0)
    for k in (0, 1, 2, 63, 64, 65, 128, 129):                                      # the path's chunk edges
        out.append((f"beats{k}", fill, BC.steady(k, 60, 60), 8000, None if k % 2 else (1024 + np.arange(k) % 4).astype(np.int32), {}, None))
    jazz = music("jazz")
    for q in (("maj",), ("maj", "min", "dim", "aug", "sus4"), ("maj", "min", "dim", "aug", "sus4", "7"), ("min7", "7", "maj7", "sus4", "aug", "dim", "min", "maj")):
        out.append((f"qualities{len(q)}", *jazz[:4], dict(qualities=q), None))        # S = 13, 61, 73, 97: either side of 64 lanes
    out.append(("no_records", BC.records([]), BC.steady(12), 700, None, {}, None))
    drums = BC.records(0.5 + 0.25 * np.arange(60), pitch=np.tile([36, 42, 38, 42], 15), program=128, drum=True)
    out.append(("drums_only", drums, BC.steady(31), 1700, None, {}, None))
    out.append(("one_pitch_class", BC.records(0.5 + 0.5 * np.arange(12), pitch=np.tile([50, 62], 6), length=0.4), BC.steady(12), 700, None, {}, None))
    fifth = BC.records(np.repeat(0.5 + 0.5 * np.arange(12), 2), pitch=np.tile([60, 67], 12), length=0.4)
    out.append(("root_and_fifth", fifth, BC.steady(12), 700, None, {}, None))      # maj and min tie: maj, the earlier state
    aug = BC.records(np.repeat(0.5 + 0.5 * np.arange(12), 3), pitch=np.tile([60, 64, 68], 12), length=0.4)
    out.append(("aug_no_bass", aug, BC.steady(12), 700, None, dict(bass_div=64, w_bass=0), None))      # C, E and Ab aug tie: the smallest root
    out.append(("aug_with_bass", np.concatenate([aug, BC.records([0.5], pitch=40, length=6.0)]), BC.steady(12), 700, None, {}, None))
    silence = music("silence")
    out.append(("w_none_0", *silence[:4], dict(w_none=0), None))
    out.append(("change_cost_0", *music("mixed")[:4], dict(change_cost=0, change_cost_down=0), None))
    out.append(("change_cost_4096", *music("mixed")[:4], dict(change_cost=4096, change_cost_down=4096), None))
    bad = next(c for c in BC.edge_cases() if c[0] == "nonfinite_and_out_of_range")
    neg = BC.records([-3.0, -0.2, 0.52, 7.9, 9.0], pitch=[50, 53, 64, 67, 70], length=[30.0, 0.1, 0.01, 5.0, 1.0])
    out.append(("nonfinite_and_out_of_range", np.concatenate([bad[1], neg]), bad[2], bad[3], None, {}, None))
    two4 = music("two4")
    out.append(("beats_beyond_frames", two4[0], two4[1], 700, two4[3], {}, None))   # spans are clipped to the frames: N from there on
    pop = music("pop")
    out.append(("count_below_n", *pop[:4], {}, 150))
    out.append(("count_zero", *pop[:4], {}, 0))
    out.append(("second_params", *jazz[:4], SECOND, None))
    out.append(("second_params_random", *BC._random(5), None, SECOND, None))
    rng = np.random.default_rng(98)                                                 # 1024 records, more than one block of them, ten chunks of beats
    many = BC.records(rng.uniform(-1.0, 68.0, 1024), pitch=rng.integers(28, 96, 1024), length=rng.uniform(0.05, 4.0, 1024))
    many["is_drum"][::9], many["pitch"][::9] = 1, 36
    out.append(("records_1024", many, BC.steady(600, 5, 11), 6700, (768 + np.arange(600) % 3).astype(np.int32), {}, None))
    return out


def random_cases():
    out = []
    for seed in range(16):
        rec, b, frames = BC._random(seed)
        rng = np.random.default_rng(5000 + seed)
        metre = (256 * 4 + rng.integers(0, 4, b.size)).astype(np.int32) if seed % 2 else None
        out.append((f"random{seed}", rec, b, frames, metre, {}, None))
    return out


TIE_CASES = ("root_and_fifth", "aug_no_bass")


def all_cases():
    return musical_cases() + edge_cases() + random_cases()


live = BC.live
