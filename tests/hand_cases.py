"""Case sets for the hand splitter (tests/test_hands_cpu.py, tests/test_hands.py): NOTE_RECORD arrays, frame counts and parameter sets.
A case: (name, records, n_frames, params, count) with `count` the device count to pass (None: all records).  The musical cases are the
issue's, with onsets 16 frames apart (slot 4 k at the default slice_frames)."""
import numpy as np

import bar_cases as BC
from yourmt3_amd.hands import DEFAULTS

FPS = BC.FPS
SCAN = 1024                                                                 # the compaction scan's block (csrc/hands.hip, HAND_SCAN_THREADS)
STEP = 0.16                                                                 # 16 frames
SECOND = dict(slice_frames=3, program_lo=1, program_hi=4, span=9, w_span=7, cut_min=12, w_cut=5, w_centre=3, middle=55, mid_free=4, w_mid=2,
              w_move=5, w_switch=11, rest_slots=6)
ZERO = {k: 0 for k in DEFAULTS if k.startswith("w_")}
HEAVY = {k: 1024 for k in DEFAULTS if k.startswith("w_")}


def chords(sets, step=STEP, first=0.0, length=0.12, program=0):
    """one chord per step -> records: every pitch of sets[k] at first + k step"""
    rows = [(first + k * step, first + k * step + length, program, int(x), False) for k, chord in enumerate(sets) for x in chord]
    return BC._rec(rows)


def frames_of(rec, tail=50):
    return int(np.nanmax(np.where(np.isfinite(rec["offset"]), rec["offset"], 0.0)) * FPS) + tail if len(rec) else tail


def climbing_line():
    return chords([[x] for x in range(50, 73)])


def melody_over_alberti(bars=4):
    sets = []
    for k in range(4 * bars):
        sets.append([(48, 55, 52, 55)[k % 4]] + ([72 + k // 4] if k % 4 == 0 else []))
    return chords(sets)


def rest_piece(gap_slots):
    """{72}, {74}, then {40}, {43} with the third chord `gap_slots` slots after the second"""
    on = [0.0, STEP, STEP + gap_slots * 0.04, 2 * STEP + gap_slots * 0.04]
    return BC.records(on, pitch=np.array([72, 74, 40, 43]), length=0.1)


def musical_cases():
    out = [("climbing_line", climbing_line()), ("melody_over_alberti", melody_over_alberti()), ("wide_chord", chords([[36, 43, 48, 64, 67, 72]])),
           ("right_triad", chords([[60, 64, 67]])), ("left_triad", chords([[40, 47, 52]])), ("high_chord", chords([[64, 67, 76, 79, 84]])),
           ("rest_then_left", rest_piece(DEFAULTS["rest_slots"] + 5))]
    return [(name, rec, frames_of(rec), {}, None) for name, rec in out]


def dense(T, seed=0, slice_frames=4, lo=30, hi=96, per=3):
    """T occupied slots in a row, up to `per` pitches in each -> records"""
    rng = np.random.default_rng(3200 + seed)
    k = rng.integers(1, per + 1, T)
    slot = np.repeat(np.arange(T), k)
    on = (slot * slice_frames + rng.integers(0, slice_frames, slot.size)) / FPS
    return BC.records(on, pitch=rng.integers(lo, hi, slot.size), length=rng.uniform(0.02, 0.5, slot.size))


def sparse(T, seed=0, max_gap=40):
    """T occupied slots with random gaps of 1 .. max_gap slots: some are rests at the default rest_slots, most are not"""
    rng = np.random.default_rng(3300 + seed)
    slot = np.cumsum(rng.integers(1, max_gap + 1, T))
    k = rng.integers(1, 4, T)
    on = np.repeat(slot, k) * 4 / FPS
    return BC.records(on, pitch=rng.integers(24, 108, on.size), length=0.05)


def random_notes(n, frames, seed=0):
    rng = np.random.default_rng(3400 + seed)
    rec = BC.records(rng.uniform(-0.5, frames / FPS + 0.5, n), pitch=rng.integers(-3, 131, n), length=rng.uniform(0.01, 2.0, n),
                     program=rng.integers(-1, 12, n))
    rec["is_drum"][::11] = 1
    rec["onset"][5::53] = np.nan
    rec["offset"][7::59] = np.nan
    rec["offset"][9::61] = np.inf
    return rec


def edge_cases():
    out = [("no_records", BC.records([]), 400, {}, None)]
    out.append(("none_selected", BC.records(0.1 * np.arange(12), pitch=60, program=9), 400, {}, None))
    out.append(("one_slice", chords([[55, 62]]), 100, {}, None))
    out.append(("two_slices", chords([[30], [90]]), 100, {}, None))
    for T in (SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 1):                     # the compaction scan's block edges, dense slots
        rec = dense(T, seed=T)
        out.append((f"dense{T}", rec, 4 * T + 60, {}, None))
    rec = sparse(300)
    out.append(("sparse300", rec, frames_of(rec), {}, None))
    out.append(("pitch0_and_127", chords([[0], [0, 1], [127], [126, 127], [0, 127], [0], [127]]), 200, dict(middle=0, mid_free=0), None))
    out.append(("state128_wins", chords([[127], [120, 127], [127]]), 100, dict(middle=128, mid_free=0, w_mid=50), None))
    out.append(("state0_wins", chords([[0], [0, 9], [0]]), 100, dict(middle=0, mid_free=0, w_mid=50), None))
    dup = chords([[60, 60, 60, 64], [48, 48], [64, 64, 48]])
    out.append(("duplicates", dup, 100, {}, None))
    out.append(("all_equal_costs", chords([[60], [61], [59], [60, 61], [62]] * 4), 400, ZERO, None))
    r = DEFAULTS["rest_slots"]
    out.append(("gap_rest_minus_1", rest_piece(r - 1), frames_of(rest_piece(r)), {}, None))
    out.append(("gap_rest", rest_piece(r), frames_of(rest_piece(r)), {}, None))
    # onsets before frame 0 (clipped in), at n_frames - 1, at n_frames and beyond (empty spans)
    edge = BC.records([-0.5, -0.02, 0.0, 0.99, 1.0, 1.5, 3.0, -0.5], pitch=np.array([50, 52, 70, 71, 72, 73, 74, 75]),
                      length=np.array([0.2, 0.1, 0.1, 0.5, 0.1, 0.1, 0.1, 0.2]))
    edge["offset"][0] = 0.3                                                 # sounding into the frames: its span starts at frame 0; the last one ends before it
    out.append(("frame_edges", edge, 100, {}, None))
    bad = BC.records(0.1 * np.arange(16), pitch=np.array([60, 61, 62, 63, 64, 65, 66, 67, 48, 49, 50, 51, 52, 53, 128, -1]),
                     program=np.array([0, 7, 8, -1, 0, 0, 128, 129, 200, 3, 3, 3, 7, 0, 0, 0]))
    bad["onset"][4], bad["offset"][5] = np.nan, np.nan
    bad["is_drum"][9] = 1
    bad["offset"][10] = np.inf
    bad["onset"][11] = np.inf
    out.append(("nan_drums_programs", bad, 300, {}, None))
    out.append(("programs_at_the_edges", BC.records(0.1 * np.arange(8), pitch=40 + 5 * np.arange(8), program=np.array([0, 1, 2, 4, 5, 6, 1, 4])), 200,
                dict(program_lo=1, program_hi=4), None))
    alberti = melody_over_alberti()
    out.append(("count_below_n", alberti, frames_of(alberti), {}, 13))
    out.append(("count_zero", alberti, frames_of(alberti), {}, 0))
    out.append(("slice_frames1", dense(200, seed=1, slice_frames=1), 300, dict(slice_frames=1), None))
    out.append(("slice_frames64", dense(40, seed=2, slice_frames=64), 64 * 40 + 10, dict(slice_frames=64, rest_slots=2), None))
    out.append(("weights_zero", sparse(120, seed=3), frames_of(sparse(120, seed=3)), ZERO, None))
    heavy = dense(5000, seed=4, lo=0, hi=128, per=5)
    out.append(("weights_1024_5000", heavy, 4 * 5000 + 60, {**HEAVY, "span": 1, "cut_min": 127, "mid_free": 0}, None))
    out.append(("second_params", random_notes(400, 900, seed=5), 900, SECOND, None))
    out.append(("random_2000", random_notes(2000, 3000, seed=6), 3000, {}, None))
    return out


def random_cases(n=12):
    out = []
    for seed in range(n):
        rng = np.random.default_rng(3500 + seed)
        frames = int(rng.integers(50, 700))
        params = {} if seed % 3 == 0 else dict(slice_frames=int(rng.integers(1, 9)), span=int(rng.integers(1, 30)), w_span=int(rng.integers(0, 40)),
                                               cut_min=int(rng.integers(0, 20)), w_cut=int(rng.integers(0, 40)), w_centre=int(rng.integers(0, 4)),
                                               middle=int(rng.integers(40, 80)), mid_free=int(rng.integers(0, 20)), w_mid=int(rng.integers(0, 4)),
                                               w_move=int(rng.integers(0, 6)), w_switch=int(rng.integers(0, 100)), rest_slots=int(rng.integers(1, 40)))
        out.append((f"random{seed}", random_notes(int(rng.integers(1, 160)), frames, seed=100 + seed), frames, params, None))
    return out


TIE_CASES = ("all_equal_costs", "weights_zero")


def all_cases():
    return musical_cases() + edge_cases() + random_cases()


live = BC.live
