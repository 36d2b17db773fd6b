"""Seeded cases for the note metrics, shared by tests/test_metrics_cpu.py and tests/test_metrics.py.  A case is a dict: id, ref and est
(NOTE_RECORD arrays), params (n_programs, drum_program and the three tolerances).  Times lie on the codec's 10 ms grid and are computed
as the detokeniser computes them, start + step / 100 with segment-shaped starts, so that the grid's f64 arithmetic appears (|1.05 - 1.00|
exceeds 0.05 in f64).  reference(case) is note_metrics' flat result, computed once per case and never changed."""
import functools

import numpy as np

from yourmt3_amd.metrics import note_metrics
from yourmt3_amd.task_manager import NOTE_RECORD

SEED = 20261018
SEGMENT_SEC = 32767 / 16000           # the start of segment s is s * SEGMENT_SEC
DEFAULT = dict(n_programs=130, drum_program=128, onset_tol=0.05, offset_min_tol=0.05, offset_ratio=0.2)
SMALL = dict(n_programs=3, drum_program=1, onset_tol=0.03, offset_min_tol=0.02, offset_ratio=0.5)
NAN = float("nan")


def t(seg: int, step: int) -> float:
    """the detokeniser's event time"""
    return seg * SEGMENT_SEC + step / 100


def records(rows) -> np.ndarray:
    """[(onset, offset, program, pitch, is_drum)] -> NOTE_RECORD array (score NaN: it is not read)"""
    rec = np.zeros(len(rows), NOTE_RECORD)
    for i, (on, off, program, pitch, drum) in enumerate(rows):
        rec[i] = (on, off, program, pitch, int(drum), NAN)
    return rec


def perturbed(rng, rows, drop=0.1, extra=0.1, max_shift=7, rekey=0.05):
    """an estimate for the reference `rows`: onsets and offsets moved by whole grid steps (up to max_shift, so both sides of the 50 ms
    boundary occur), some notes dropped, some re-keyed, some added; shuffled"""
    out = []
    for on, off, program, pitch, drum in rows:
        u = rng.random()
        if u < drop:
            continue
        d_on = int(rng.integers(-max_shift, max_shift + 1)) if rng.random() < 0.6 else 0
        d_off = int(rng.integers(-30, 31)) if rng.random() < 0.6 else 0
        if u > 1.0 - rekey:
            pitch = (pitch + 1) % 128
        out.append((on + d_on / 100, off + d_off / 100, program, pitch, drum))
    for _ in range(int(len(rows) * extra) + 1):
        on, off, program, pitch, drum = rows[int(rng.integers(len(rows)))]
        out.append((on + int(rng.integers(-20, 21)) / 100, off + int(rng.integers(-20, 21)) / 100, program, pitch, drum))
    return [out[i] for i in rng.permutation(len(out))]


def one_key(rng, n, program=0, pitch=60, gap=(2, 12)):
    """n notes of one key, a few grid steps apart, on segment-shaped times"""
    rows, step = [], 0
    for _ in range(n):
        step += int(rng.integers(*gap))
        seg, s = divmod(step, 204)
        on = t(seg, s)
        rows.append((on, on + int(rng.integers(1, 80)) / 100, program, pitch, False))
    return [rows[i] for i in rng.permutation(n)]


def _case(name, ref, est, params=DEFAULT):
    return {"id": name, "ref": records(ref), "est": records(est), "params": dict(params)}


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    out = []
    some = one_key(rng, 5)
    out += [_case("0_vs_0", [], []), _case("0_vs_n", [], some), _case("n_vs_0", some, []),
            _case("1_vs_1", [(t(1, 5), t(1, 30), 0, 60, False)], [(t(1, 6), t(1, 33), 0, 60, False)])]
    # one key with 1, 63, 64, 65 and 257 notes; 438 / 440 and 438 / 441 lie either side of what a workgroup keeps on chip, 700 / 700 beyond it
    for n in (1, 63, 64, 65, 257):
        ref = one_key(rng, n)
        out.append(_case(f"bucket_{n}", ref, perturbed(rng, ref)))
    for nr, ne in ((438, 440), (438, 441), (700, 700)):
        ref = one_key(rng, max(nr, ne))
        est = perturbed(rng, ref, drop=0.0, extra=0.0, rekey=0.0)[:-1]             # (one note is added: one is left out again)
        out.append(_case(f"bucket_{nr}_vs_{ne}", ref[:nr], est[:ne]))
    # 130 programs x a few pitches: most keys are empty
    ref = []
    for _ in range(400):
        seg, step = int(rng.integers(0, 6)), int(rng.integers(0, 204))
        prog = int(rng.integers(0, 130))
        on = t(seg, step)
        ref.append((on, on + int(rng.integers(1, 150)) / 100, prog, int(rng.choice([36, 60, 61, 127, 0])), prog == 128))
    out.append(_case("130_programs", ref, perturbed(rng, ref)))
    # a dense key: 64 x 64 notes inside one onset window; the offset tolerance grows with the reference's duration, so a long reference
    # can take the only estimate a short one hits
    ref = [(t(0, 100 + i % 5), t(0, 100 + i % 5) + 0.5 + i * 0.11, 0, 64, False) for i in range(64)]
    est = [(t(0, 100 + int(rng.integers(0, 5))), t(0, 100) + 0.5 + j * 0.11 + int(rng.integers(-25, 60)) / 100, 0, 64, False) for j in range(64)]
    out.append(_case("dense_64_x_64", [ref[i] for i in rng.permutation(64)], [est[i] for i in rng.permutation(64)]))
    # the smallest case an earliest-free greedy gets wrong: A (tolerance 0.2) takes X, the only estimate B (tolerance 0.18) can hit
    out.append(_case("augmenting_path_2_x_2", [(1.00, 2.00, 0, 60, False), (1.01, 1.91, 0, 60, False)],
                     [(1.00, 1.85, 0, 60, False), (1.01, 2.15, 0, 60, False)]))
    # boundaries of the onset window: 50 ms hits and 60 ms misses on the grid (in both segments), 1.05004 hits and 1.05006 misses
    ref = [(t(s, 100), t(s, 150), 0, p, False) for s in (0, 1) for p in (60, 61, 62, 63)] + [(1.0, 1.5, 0, 70, False), (1.0, 1.5, 0, 71, False)]
    est = [(t(s, 100 + d), t(s, 150), 0, p, False) for s in (0, 1) for p, d in ((60, 5), (61, 6), (62, -5), (63, -6))]
    est += [(1.05004, 1.5, 0, 70, False), (1.05006, 1.5, 0, 71, False)]
    out.append(_case("onset_boundaries", ref, est))
    # offset tolerance: exactly 20 % of a 10 s note and one grid step beyond it; the 50 ms minimum on a short note; a reference whose
    # offset lies BEFORE its onset keeps the minimum
    ref = [(1.0, 11.0, 0, 60, False), (1.0, 11.0, 0, 61, False), (1.0, 1.1, 0, 62, False), (1.0, 1.1, 0, 63, False),
           (2.0, 1.5, 0, 64, False), (2.0, 1.5, 0, 65, False)]
    est = [(1.0, 13.0, 0, 60, False), (1.0, 13.01, 0, 61, False), (1.0, 1.15, 0, 62, False), (1.0, 1.16, 0, 63, False),
           (2.0, 1.54, 0, 64, False), (2.0, 1.56, 0, 65, False)]
    out.append(_case("offset_boundaries", ref, est))
    # drums: stray program fields, different offsets (they still match), a pitch under the drum program without the flag, NaN offsets
    ref = [(t(0, 10), t(0, 11), 128, 36, True), (t(0, 50), t(0, 51), 5, 38, True), (t(1, 0), t(1, 1), 999, 42, True),
           (t(1, 20), t(1, 21), 128, 36, False), (t(2, 0), NAN, -3, 36, True), (t(2, 50), t(2, 51), 128, 46, True)]
    est = [(t(0, 11), t(0, 90), 128, 36, True), (t(0, 50), t(0, 99), 128, 38, True), (t(1, 5), t(1, 1), 128, 42, True),
           (t(1, 26), t(1, 27), -1, 36, True), (t(2, 0), t(5, 0), 128, 36, True), (t(2, 50), NAN, 7, 46, True), (t(2, 50), t(2, 51), 7, 46, False)]
    out.append(_case("drums", ref, est))
    # records that do not count: NaN onset, NaN offset of a pitched note, pitch 128 and -1, program n_programs and -1
    good = [(1.0, 1.5, 0, 60, False), (2.0, 2.5, 129, 61, False)]
    bad = [(NAN, 1.5, 0, 60, False), (1.0, NAN, 0, 60, False), (1.0, 1.5, 0, 128, False), (1.0, 1.5, 0, -1, False), (1.0, 1.5, 130, 60, False),
           (1.0, 1.5, -1, 60, False), (NAN, NAN, 128, 36, True), (1.0, 1.5, 128, 128, True)]
    out.append(_case("skipped_records", good + bad, bad[:5] + good + bad[5:] + bad[:2]))
    # infinite times: they count, sort to the ends and hit nothing (inf - inf is no distance); an infinite offset tolerance hits a finite offset's miss
    inf = float("inf")
    ref = [(inf, inf, 0, 60, False), (-inf, 1.0, 0, 60, False), (1.0, inf, 0, 60, False), (2.0, 2.5, 0, 60, False), (inf, inf, 128, 36, True)]
    est = [(inf, inf, 0, 60, False), (-inf, 1.0, 0, 60, False), (1.0, inf, 0, 60, False), (1.0, 9.0, 0, 60, False), (2.0, 2.5, 0, 60, False),
           (inf, inf, 128, 36, True)]
    out.append(_case("infinite_times", ref, est))
    # other parameters: 3 programs, drums at 1, tighter windows
    ref = []
    for _ in range(150):
        on = t(int(rng.integers(0, 3)), int(rng.integers(0, 204)))
        prog = int(rng.integers(0, 4))
        ref.append((on, on + int(rng.integers(1, 60)) / 100, prog, int(rng.integers(59, 62)), bool(rng.integers(0, 5) == 0)))
    out.append(_case("3_programs_other_tolerances", ref, perturbed(rng, ref, max_shift=4), SMALL))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    case = next(c for c in cases() if c["id"] == case_id)
    return note_metrics(case["ref"], case["est"], **case["params"])


def reference(case):
    """note_metrics of the case (a NoteMetricCounts), computed once"""
    return _reference(case["id"])
