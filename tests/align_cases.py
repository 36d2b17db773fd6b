"""Named cases for the alignment, shared by tests/test_align_cpu.py and tests/test_align.py.  A case is a dict: id, ref and est (NOTE_RECORD
arrays), na and nb (the two frame counts), band, n_programs, drum_program, fps.  reference(case) is the host specification's result
(yourmt3_amd/metrics.py: dtw_align), computed once per case and never changed.

The device's tiles are 256 frames of the shorter side by 64 frames of the longer one (yourmt3_amd/csrc/align.hip), so besides the listed
frame counts against 1, 64 and 200 there are pairs whose SHORTER side crosses 256 and 512."""
import functools

import numpy as np

from roll_cases import EDGE_PITCHES, INF, NAN, records
from yourmt3_amd.metrics import dtw_align

SEED = 20261018
FRAME_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)      # the edges of a 64-lane strip and of power-of-two tiles up to 256
OTHER_SIDE = (1, 64, 200)
SQUARES = ((255, 256), (256, 256), (257, 256), (256, 257), (257, 257), (300, 257), (512, 513), (513, 512), (513, 520))
BANDS = (1, 7, 1 << 20)                                                  # the narrowest; one that cuts through tiles; one without effect
SMALL_CELLS = 60000                                                      # cases up to this many cells are also run through tests/align_model.py


def _case(name, ref, est, na, nb, band, n_programs=3, drum_program=1, fps=100.0):
    return {"id": name, "ref": records(ref), "est": records(est), "na": na, "nb": nb, "band": band, "n_programs": n_programs,
            "drum_program": drum_program, "fps": fps}


def params(case) -> dict:
    return {"n_programs": case["n_programs"], "drum_program": case["drum_program"], "frames_per_second": case["fps"]}


def polyphony(rng, na, nb, n=None):
    """random notes at the word-edge pitches over na frames, and the same notes stretched to nb frames with jitter, misses and extras"""
    n = n if n is not None else max(4, min(60, na // 4))
    scale = nb / na
    ref, est = [], []
    for _ in range(n):
        on = int(rng.integers(0, na)) / 100
        off = on + int(rng.integers(1, 40)) / 100
        prog = int(rng.integers(0, 3))
        pitch = int(rng.choice(EDGE_PITCHES + (36, 60)))
        ref.append((on, off, prog, pitch, prog == 1))
        u = rng.random()
        if u < 0.1:
            continue
        if u > 0.9:
            pitch = (pitch + 12) % 128
        est.append((round(on * scale + int(rng.integers(-1, 2)) / 100, 2), round(off * scale, 2), prog, pitch, prog == 1))
    est += [(int(rng.integers(0, nb)) / 100, int(rng.integers(0, nb + 20)) / 100, 0, 64, False) for _ in range(2)]
    return ref, est


def tempo_curve_case():
    """300 pitched notes and a drum pattern over 30 s; the estimate is the same music under a piecewise tempo curve (30 s -> 27.5 s, up to
    3.5 s off the straight line) with 10 ms jitter, 10 % misses, 5 % octave errors and 20 false alarms: 3000 x 2750 frames, band 400"""
    rng = np.random.default_rng(SEED + 1)
    knots_ref, knots_est = [0.0, 7.5, 15.0, 22.5, 30.0], [0.0, 10.375, 14.5, 18.0, 27.5]
    curve = lambda t: float(np.interp(t, knots_ref, knots_est))
    ref = []
    for _ in range(300):
        on = float(rng.uniform(0.0, 29.5))
        ref.append((round(on, 3), round(on + float(rng.uniform(0.1, 1.2)), 3), int(rng.integers(0, 8)), int(rng.integers(36, 96)), False))
    ref += [(round(0.25 * k, 3), NAN, 128, (36, 42, 38, 42)[k % 4], True) for k in range(120)]
    est = []
    for on, off, prog, pitch, drum in ref:
        u = rng.random()
        if u < 0.10:
            continue
        if u > 0.95 and not drum:
            pitch += 12
        jit = lambda: float(rng.normal(0.0, 0.010))
        est.append((curve(on) + jit(), NAN if drum else curve(off) + jit(), prog, pitch, drum))
    for _ in range(20):
        on = float(rng.uniform(0.0, 27.0))
        est.append((on, on + 0.3, int(rng.integers(0, 8)), int(rng.integers(36, 96)), False))
    return _case("tempo_curve", ref, [est[i] for i in rng.permutation(len(est))], 3000, 2750, 400, n_programs=130, drum_program=128)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    out, k = [], 0
    shapes = [(a, b) for a in FRAME_COUNTS for b in OTHER_SIDE] + [(b, a) for a in FRAME_COUNTS for b in OTHER_SIDE]
    for na, nb in list(dict.fromkeys(shapes)) + list(SQUARES):
        band = BANDS[k % 3]
        k += 1
        out.append(_case(f"frames_{na}x{nb}_band{min(band, 9999)}", *polyphony(rng, na, nb), na, nb, band))
    # every band on one shape of each orientation that crosses the 64-lane strips and the 256-frame tiles
    for na, nb in ((300, 257), (200, 513)):
        for band in BANDS + (40,):
            name = f"frames_{na}x{nb}_band{min(band, 9999)}"
            if all(c["id"] != name for c in out):
                out.append(_case(name, *polyphony(rng, na, nb), na, nb, band))
    out.append(_case("ratio_3_200", *polyphony(rng, 3, 200, 6), 3, 200, 1))
    out.append(_case("ratio_200_3", *polyphony(rng, 200, 3, 40), 200, 3, 1))
    ref, est = polyphony(rng, 90, 70, 30)
    out += [_case("both_empty", [], [], 90, 70, 7), _case("empty_ref", [], est, 90, 70, 7), _case("empty_est", ref, [], 90, 70, 7)]
    out.append(_case("one_note_at_the_end", [(0.89, 0.95, 0, 60, False)], [(0.69, 0.75, 0, 60, False)], 90, 70, 7))
    out.append(_case("identical_sets", ref, ref, 90, 90, 7))
    drums = [(0.05 * k, NAN, 1, (36, 38, 42)[k % 3], True) for k in range(18)]
    out.append(_case("drums_only", drums, [(on * 0.8 + 0.01, NAN, 5, p, True) for on, _, _, p, _ in drums], 90, 72, 7))
    good = [(0.10, 0.30, 0, 60, False), (0.20, 0.40, 2, 61, False), (0.5, NAN, 1, 36, True)]
    bad = [(NAN, 0.5, 0, 60, False), (0.1, 0.5, 0, -1, False), (0.1, 0.5, 0, 128, False), (0.1, 0.5, -1, 60, False), (0.1, 0.5, 3, 60, False),
           (0.1, NAN, 0, 60, False), (NAN, NAN, 1, 36, True), (0.1, 0.2, 1, 128, True)]
    out.append(_case("skipped_records", good + bad, bad[:3] + [(on + 0.05, off + 0.05, p, q, d) for on, off, p, q, d in good] + bad[3:] + bad[:2], 60, 66, 7))
    ref = [(INF, INF, 0, 60, False), (-INF, 0.10, 0, 61, False), (0.20, INF, 0, 62, False), (-INF, INF, 2, 63, False), (0.30, -INF, 0, 67, False),
           (INF, 0.3, 1, 36, True), (-INF, 0.3, 1, 37, True), (1e300, 2e300, 0, 68, False), (NAN, 0.2, 0, 69, False), (0.4, NAN, 0, 70, False)]
    est = [(0.05, 0.10, 0, 61, False), (0.25, INF, 0, 62, False), (-INF, 0.5, 2, 63, False), (0.31, 0.2, 0, 67, False), (0.0, INF, 1, 37, True),
           (NAN, NAN, 0, 60, False)]
    out.append(_case("infinite_and_nan_times", ref, est, 64, 80, 7))
    out.append(_case("rate_62_5", *polyphony(rng, 70, 65, 20), 70, 65, 3, fps=62.5))
    out.append(_case("256_programs", [(0.1, 0.5, 0, 60, False), (0.2, 0.3, 255, 36, False), (0.1, 0.5, 256, 60, False)],
                     [(0.15, 0.6, 254, 60, False), (0.25, 0.9, 3, 36, True)], 70, 80, 7, n_programs=256, drum_program=255))
    out.append(tempo_curve_case())
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


def small(case) -> bool:
    return case["na"] * case["nb"] <= SMALL_CELLS


def case(name):
    return next(c for c in cases() if c["id"] == name)


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    c = case(case_id)
    got = dtw_align(c["ref"], c["est"], c["na"], c["nb"], band_frames=c["band"], **params(c))
    for a in (got.path, got.warp, got.skipped):
        a.setflags(write=False)
    return got


def reference(c):
    """-> dtw_align of the case (an Alignment), computed once"""
    return _reference(c["id"])
