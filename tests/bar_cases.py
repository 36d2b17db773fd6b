"""Case sets for the bar tracker (tests/test_bars_cpu.py, tests/test_bars.py): NOTE_RECORD arrays, beats, frame counts and parameter sets,
all small.  A case: (name, records, beats int32, n_frames, params, count) with `count` the device count to pass (None: all records).
The known music is generated here and its beats are the beat tracker's own (beats.track_beats), found once."""
import functools

import numpy as np

from yourmt3_amd import beats as T
from yourmt3_amd.task_manager import NOTE_RECORD

FPS = 100.0
SECOND = dict(metres=(3, 2, 5), near_div=3, accent_cap=4, w_long=3, w_kick=0, kick_lo=36, kick_hi=38, w_accent=100, switch_cost=1)
ROOTS = (0, 5, 7, 9, 2, 4)


def _rec(rows):
    rec = np.zeros(len(rows), NOTE_RECORD)
    for i, (on, off, prog, pitch, drum) in enumerate(rows):
        rec[i] = (on, off, prog, pitch, drum, np.nan)
    return rec


def records(onsets, pitch=60, length=0.1, program=0, drum=False):
    rec = np.zeros(len(onsets), NOTE_RECORD)
    rec["onset"] = onsets
    rec["offset"] = np.asarray(onsets, np.float64) + length
    rec["program"], rec["pitch"], rec["is_drum"], rec["score"] = program, pitch, drum, np.nan
    return rec


def piece(bars, bpm=100.0, seed=0, pickup=0, kick3=False, bare=False, first=0.6, tonic=0, minor=False):
    """Known music -> (records, n_frames, the downbeats' times, the metre runs [(m, bars)]).  `bars`: the metre of every bar; `pickup`:
    beats before the first bar line.  A chord on every beat whose root changes each bar, a long bass note and a kick on every downbeat, a
    snare on odd beats, an off-beat eighth on half the beats, 10 ms jitter.  `kick3`: a second kick on beat 3 of a 4/4 bar; `bare`:
    neither bass nor drums."""
    rng = np.random.default_rng(2500 + seed)
    period = 60.0 / bpm
    jit = lambda: float(rng.normal(0, 0.01))
    third = 3 if minor else 4
    rows, downs, t = [], [], first
    layout = ([(bars[0], bars[0] - pickup + j, -1) for j in range(pickup)] if pickup else []) + [(m, k, n) for n, m in enumerate(bars) for k in range(m)]
    root = ROOTS[0]
    for m, k, bar in layout:
        if k == 0:
            downs.append(t)
            root = ROOTS[bar % len(ROOTS)]
            if not bare:
                rows.append((t + jit(), t + m * period * 0.95, 0, 36 + (tonic + root) % 12, False))
                rows.append((t + jit(), t + 0.01, 128, 36, True))
        for step in (0, third, 7):
            rows.append((t + jit(), t + 0.8 * period, 0, 60 + (tonic + root + step) % 12, False))
        if not bare and k % 2 == 1:
            rows.append((t + jit(), t + 0.01, 128, 38, True))
        if not bare and kick3 and m == 4 and k == 2:
            rows.append((t + jit(), t + 0.01, 128, 36, True))
        if rng.random() < 0.5:
            rows.append((t + period / 2 + jit(), t + 0.75 * period, 0, 72 + (tonic + root + 7) % 12, False))
        t += period
    runs = []
    for m in bars:
        if runs and runs[-1][0] == m:
            runs[-1][1] += 1
        else:
            runs.append([m, 1])
    return _rec(rows), int(round((t + 0.6) * FPS)), downs, [tuple(r) for r in runs]


# name -> (piece arguments, clean: the metre runs must be found exactly)
KNOWN = {
    "three4": (dict(bars=[3] * 16, seed=1), True),
    "four4": (dict(bars=[4] * 12, seed=2), True),
    "two4": (dict(bars=[2] * 24, seed=3), True),
    "four4_kick3": (dict(bars=[4] * 12, seed=4, kick3=True), True),
    "four4_bare": (dict(bars=[4] * 12, seed=5, bare=True), True),
    "pickup1_three4": (dict(bars=[3] * 14, seed=6, pickup=1), True),
    "pickup2_four4": (dict(bars=[4] * 11, seed=7, pickup=2), True),
    "four4_to_three4": (dict(bars=[4] * 8 + [3] * 12, seed=8), True),
    "four_three_four": (dict(bars=[4] * 8 + [3] * 8 + [4] * 8, seed=9), True),
    # An odd bar costs two switches, 2 P = 480 mean_d.  Reading the n bars of 4/4 on one side of it as 2/4 instead costs one switch less and
    # loses 15 (D0 - d) a bar (D0: a downbeat's salience, d: another beat's; bars.py, bar path).  The rules can place the odd bar only where
    # 15 n (D0 - d) > P = 240 mean_d: with this music's D0 - d of about 2 mean_d, n > 8.  Hence ten bars on either side.
    "one_two4_bar": (dict(bars=[4] * 10 + [2] + [4] * 10, seed=10), True),
    "four4_80bpm": (dict(bars=[4] * 10, seed=11, bpm=80.0), True),
    "three4_140bpm": (dict(bars=[3] * 16, seed=12, bpm=140.0), True),
}


@functools.lru_cache(maxsize=None)
def known(name):
    """-> (records, beats int32, n_frames, the downbeats' times, the metre runs, the pickup)"""
    kw, _ = KNOWN[name]
    rec, n_frames, downs, runs = piece(**kw)
    return rec, T.track_beats(rec, n_frames)[0], n_frames, downs, runs, kw.get("pickup", 0)


def musical_cases():
    return [(name, known(name)[0], known(name)[1], known(name)[2], {}, None) for name in KNOWN]


def steady(k, first=50, step=50):
    return (first + step * np.arange(k)).astype(np.int32)


def melody(key, seed=0, n=160):
    """a seeded melody weighted by the scale of `key` (12 mode + tonic): tonic, fifth and third most, the other scale notes less,
    nothing outside the scale -> records over 8 s"""
    rng = np.random.default_rng(700 + 31 * key + seed)
    mode, tonic = divmod(key, 12)
    scale = (0, 2, 3, 5, 7, 8, 10) if mode else (0, 2, 4, 5, 7, 9, 11)
    weight = np.array([6, 2, 4, 3, 5, 2, 2], np.float64)
    steps = rng.choice(7, n, p=weight / weight.sum())
    on = np.sort(rng.uniform(0.3, 7.7, n))
    return records(on, pitch=np.array([60 + (tonic + scale[s]) % 12 for s in steps]), length=rng.uniform(0.1, 0.4, n))


def _random(seed, max_notes=400, max_frames=3000):
    rng = np.random.default_rng(4000 + seed)
    n, frames = int(rng.integers(0, max_notes + 1)), int(rng.integers(1, max_frames + 1))
    gaps = rng.integers(1, 8, 400) if seed % 5 == 4 else rng.integers(13, 120, 400)        # (a few with beats a frame or so apart)
    b = np.cumsum(gaps)
    b = b[b < frames][:int(rng.integers(0, 60))].astype(np.int32)
    period = rng.uniform(0.3, 1.2)
    on = np.where(rng.random(n) < 0.6, np.rint(rng.uniform(0, frames / FPS / period, n)) * period, rng.uniform(-0.5, frames / FPS + 0.5, n))
    on = on + rng.normal(0, 0.008, n)
    rec = records(on, pitch=rng.integers(-2, 130, n), length=rng.uniform(0.02, 3.0, n), program=rng.integers(-1, 132, n))
    rec["is_drum"] = rng.random(n) < 0.2
    rec["pitch"] = np.where((rec["is_drum"] != 0) & (rng.random(n) < 0.5), rng.integers(34, 38, n), rec["pitch"])
    return rec, b, frames


def edge_cases():
    out = []
    some = known("four4")[0]
    for k in (0, 1, 2, 3):
        out.append((f"beats{k}", some, steady(k, 60, 60), 900, {}, None))
    out.append(("metres_3_only", known("three4")[0], known("three4")[1], known("three4")[2], dict(metres=(3,)), None))
    click = records(0.5 + 0.5 * np.arange(25))
    out.append(("metronome", click, steady(25), 1300, {}, None))
    out.append(("metronome_flat", click, steady(25), 1300, dict(w_accent=0), None))          # d = 0 everywhere: every path ties
    out.append(("switch_cost_0", known("four_three_four")[0], known("four_three_four")[1], known("four_three_four")[2], dict(switch_cost=0), None))
    drums = records(0.5 + 0.25 * np.arange(60), pitch=np.tile([36, 42, 38, 42], 15), program=128, drum=True)
    out.append(("drums_only", drums, steady(31), 1700, {}, None))
    out.append(("one_long_note", records([0.0], pitch=57, length=20.0), steady(30), 1600, {}, None))
    out.append(("long_note_from_before", records([-3.0, 0.52], pitch=[50, 64], length=[30.0, 0.01]), steady(12), 500, {}, None))
    out.append(("cap_300_on_one_beat", np.concatenate([records([2.0] * 300, pitch=np.arange(300) % 128), click]), steady(25), 1300, {}, None))
    bad = records([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5])
    bad["onset"][1], bad["onset"][3], bad["onset"][5] = np.nan, np.inf, -np.inf
    bad["program"][6], bad["program"][7], bad["pitch"][8] = 130, -1, 128
    bad["offset"][9], bad["offset"][10], bad["offset"][11], bad["onset"][12] = np.nan, np.inf, -np.inf, 1e300
    bad["offset"][5] = 3.0                                                                   # from -inf to 3 s: a span without an accent
    out.append(("nonfinite_and_out_of_range", bad, steady(14), 800, {}, None))
    out.append(("count_below_n", known("four4")[0], known("four4")[1], known("four4")[2], {}, 40))
    out.append(("count_zero", known("four4")[0], known("four4")[1], known("four4")[2], {}, 0))
    out.append(("second_params", known("three4")[0], known("three4")[1], known("three4")[2], SECOND, None))
    out.append(("second_params_random", *_random(5), SECOND, None))
    out.append(("one_note_key_tie", records([1.0], pitch=66, length=0.5), steady(6), 400, {}, None))
    rng = np.random.default_rng(99)                                                          # more than one block of beats, many chunks of the path
    many = records(rng.uniform(0.0, 66.0, 500), pitch=rng.integers(30, 90, 500), length=rng.uniform(0.05, 2.0, 500))
    many["is_drum"][::7], many["pitch"][::7] = 1, 36
    out.append(("many_beats", many, steady(600, 5, 11), 6700, {}, None))
    out.append(("beats_beyond_frames", known("two4")[0], known("two4")[1], 700, {}, None))     # spans are clipped to the frames, accents are not
    return out


def random_cases():
    return [(f"random{seed}", *_random(seed), {}, None) for seed in range(20)]


TIE_CASES = ("metronome_flat", "one_note_key_tie")


def all_cases():
    return musical_cases() + edge_cases() + random_cases()


def live(rec, count):
    """the records a case's count leaves"""
    return rec if count is None else rec[:max(0, min(len(rec), count))]


def f_measure(est_sec, ref_sec, tol=0.07):
    """one-to-one within `tol`: both lists ascend, so the greedy sweep is a maximum matching"""
    est, ref = list(est_sec), list(ref_sec)
    i = j = hits = 0
    while i < len(est) and j < len(ref):
        if abs(est[i] - ref[j]) <= tol:
            hits, i, j = hits + 1, i + 1, j + 1
        elif est[i] < ref[j]:
            i += 1
        else:
            j += 1
    return 2.0 * hits / (len(est) + len(ref)) if est and ref else 0.0
