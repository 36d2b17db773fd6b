"""Note metrics, the parts that need no GPU (include/ymt3.h, note metrics):
  1. note_metrics (yourmt3_amd/metrics.py), the specification, equals a brute-force oracle written here -- the full hit matrix of every key
     and networkx' Hopcroft-Karp matching -- on every case of tests/metrics_cases.py;
  2. tests/metrics_model.py -- the kernels' algorithm in plain Python -- equals note_metrics on every case; the cases keep their teeth: on
     at least one of them a matching without augmenting paths falls short on the onset+offset metric, on none on the onset metric;
  3. the derived values on hand-written cases with literal numbers;
  4. the C ABI: the three entry points are declared, listed and exported, the ABI version is still 3.
Every comparison of counts is an integer equality."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import metrics_cases as C
import metrics_model as M
from yourmt3_amd.metrics import NoteMetricCounts, max_matching, note_metrics, _augmenting_paths
from yourmt3_amd.task_manager import Note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.cases()
IDS = [c["id"] for c in CASES]


def _matching_size(hits) -> int:
    """maximum matching of a boolean matrix: networkx if importable, else exhaustive search (keys of at most 8 x 8 notes only)"""
    n, m = len(hits), len(hits[0]) if hits else 0
    edges = [(i, j) for i in range(n) for j in range(m) if hits[i][j]]
    if not edges:
        return 0
    try:
        import networkx as nx
    except ImportError:
        if n > 8 or m > 8:
            return None
        best = 0
        for k in range(1, min(n, m) + 1):
            for rows in itertools.combinations(range(n), k):
                if any(all(hits[i][j] for i, j in zip(rows, cols)) for cols in itertools.permutations(range(m), k)):
                    best = k
                    break
            else:
                break
        return best
    g = nx.Graph()
    left = [("r", i) for i in range(n)]
    g.add_nodes_from(left, bipartite=0)
    g.add_nodes_from([("e", j) for j in range(m)], bipartite=1)
    g.add_edges_from((("r", i), ("e", j)) for i, j in edges)
    matching = nx.bipartite.hopcroft_karp_matching(g, top_nodes=left)
    return sum(1 for k in matching if k[0] == "r")


def _d(a, b):
    return float(np.rint(abs(a - b) * 1e4)) / 1e4


def oracle(case):
    """the rules of include/ymt3.h, record by record and pair by pair -> the flat result, or None if a key was too large for the fallback"""
    p = case["params"]
    NP, DP = p["n_programs"], p["drum_program"]
    counts = np.zeros((NP + 1, 2, 3), np.int64)
    skipped = [0, 0]
    keyed = [{}, {}]
    for s, rec in enumerate((case["ref"], case["est"])):
        for on, off, program, pitch, is_drum in zip(rec["onset"].tolist(), rec["offset"].tolist(), rec["program"].tolist(), rec["pitch"].tolist(),
                                                    rec["is_drum"].tolist()):
            prog = DP if is_drum else program
            drum = prog == DP
            if math.isnan(on) or not 0 <= pitch < 128 or not 0 <= prog < NP or (not drum and math.isnan(off)):
                skipped[s] += 1
                continue
            rows = [prog] if drum else [prog, NP]
            for row in rows:
                counts[row, :, 1 + s] += 1
                keyed[s].setdefault((row, pitch), []).append((on, off))
    for key in set(keyed[0]) & set(keyed[1]):
        R, E = keyed[0][key], keyed[1][key]
        onset = [[_d(r[0], e[0]) <= p["onset_tol"] for e in E] for r in R]
        both = [[onset[i][j] and _d(r[1], e[1]) <= max(p["offset_min_tol"], p["offset_ratio"] * (r[1] - r[0])) for j, e in enumerate(E)]
                for i, r in enumerate(R)]
        a, b = _matching_size(onset), _matching_size(both)
        if a is None or b is None:
            return None
        counts[key[0], 0, 0] += a
        counts[key[0], 1, 0] += a if key[0] == DP else b
    return np.concatenate([counts.reshape(-1), skipped]).astype(np.int32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_note_metrics_equals_the_brute_force_oracle(case):
    want = oracle(case)
    if want is None:
        pytest.skip("networkx is not importable and the case has a key of more than 8 x 8 notes")
    got = C.reference(case)
    assert got.flat().dtype == np.int32 and got.flat().size == (case["params"]["n_programs"] + 1) * 6 + 2
    assert np.array_equal(got.flat(), want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_kernel_model_equals_note_metrics(case):
    assert np.array_equal(M.model_counts(case["ref"], case["est"], **case["params"]), C.reference(case).flat())


def test_note_lists_and_record_arrays_give_the_same_counts():
    case = next(c for c in CASES if c["id"] == "130_programs")
    as_notes = [[Note(r["onset"], r["offset"], bool(r["is_drum"]), int(r["program"]), int(r["pitch"])) for r in case[side]] for side in ("ref", "est")]
    assert note_metrics(*as_notes, **case["params"]) == C.reference(case)


def test_the_cases_keep_their_teeth():
    """On some case a matching without augmenting paths falls short of the maximum on the onset+offset metric; on no case does the
    two-pointer walk fall short on the onset metric (the maximum is note_metrics', through the library's matching)."""
    short_offset, sizes = [], set()
    for case in CASES:
        p = case["params"]
        tol = (p["onset_tol"], p["offset_min_tol"], p["offset_ratio"])
        keyed, (rb, eb), _ = M.keys_of(case["ref"], case["est"], **p)
        sizes |= {len(v) for v in rb.values()} | {len(v) for v in eb.values()}
        walk = greedy = 0
        for key, R, E, win in keyed:
            if key // 128 == p["n_programs"]:
                walk += M.onset_walk(R, E, win, tol[0])
                greedy += M.offset_greedy(R, E, win, *tol)
        ref = C.reference(case).counts[p["n_programs"]]
        assert walk == ref[0, 0], case["id"]
        assert greedy <= ref[1, 0], case["id"]
        if greedy < ref[1, 0]:
            short_offset.append(case["id"])
    print("greedy falls short on onset+offset in:", short_offset)
    assert "augmenting_path_2_x_2" in short_offset and "dense_64_x_64" in short_offset
    assert {1, 63, 64, 65, 257, 438, 440, 441, 700} <= sizes


def test_skipped_records_and_empty_sides():
    by_id = {c["id"]: C.reference(c) for c in CASES}
    assert by_id["0_vs_0"].flat().sum() == 0
    assert by_id["0_vs_n"].counts[130].tolist() == [[0, 0, 5], [0, 0, 5]] and by_id["n_vs_0"].counts[0].tolist() == [[0, 5, 0], [0, 5, 0]]
    sk = by_id["skipped_records"]
    assert sk.skipped.tolist() == [8, 10] and sk.counts[130].tolist() == [[2, 2, 2], [2, 2, 2]] and int(sk.counts[:, 0, 1].sum()) == 4
    on = by_id["onset_boundaries"].counts[130]
    assert on[0].tolist() == [5, 10, 10]                                 # 50 ms hits, 60 ms misses, 1.05004 hits, 1.05006 misses
    off = by_id["offset_boundaries"].counts[130]
    assert off.tolist() == [[6, 6, 6], [3, 6, 6]]
    dr = by_id["drums"]
    assert dr.counts[128].tolist() == [[5, 6, 6], [5, 6, 6]] and dr.counts[130].tolist() == [[0, 0, 1], [0, 0, 1]] and dr.skipped.tolist() == [0, 0]
    inf = by_id["infinite_times"].counts
    assert inf[130].tolist() == [[2, 4, 5], [2, 4, 5]] and inf[128].tolist() == [[0, 1, 1], [0, 1, 1]]


def test_the_fallback_matching_agrees_with_the_library():
    rng = np.random.default_rng(5)
    for _ in range(200):
        hits = rng.random((int(rng.integers(1, 9)), int(rng.integers(1, 9)))) < 0.3
        assert _augmenting_paths(hits) == max_matching(hits) == _matching_size(hits.tolist())


def test_derived_values_on_hand_written_cases():
    n = lambda on, off, pitch=60, program=0, drum=False: Note(on, off, drum, 128 if drum else program, pitch)
    ref = [n(0.0, 1.0), n(1.0, 2.0, 62), n(0.5, 0.51, 36, drum=True)]
    perfect = note_metrics(ref, list(ref), 130)
    assert (perfect.onset_f, perfect.offset_f, perfect.drum_onset_f, perfect.multi_f) == (1.0, 1.0, 1.0, 1.0)
    assert perfect.counts[130].tolist() == [[2, 2, 2], [2, 2, 2]] and perfect.counts[128].tolist() == [[1, 1, 1], [1, 1, 1]]
    disjoint = note_metrics(ref, [n(5.0, 6.0), n(1.0, 2.0, 63), n(0.6, 0.61, 36, drum=True)], 130)
    assert (disjoint.onset_f, disjoint.offset_f, disjoint.drum_onset_f, disjoint.multi_f) == (0.0, 0.0, 0.0, 0.0)
    # 4 pitched references, 2 estimates: both onsets hit, one offset does; the right pitch under another program is agnostic-only
    ref = [n(0.0, 1.0), n(1.0, 2.0), n(2.0, 3.0), n(3.0, 4.0, 64)]
    est = [n(0.02, 1.5), n(3.0, 4.0, 64, program=7)]
    m = note_metrics(ref, est, 130)
    assert m.counts[130].tolist() == [[2, 4, 2], [1, 4, 2]]
    assert m.precision(130, 0) == 1.0 and m.recall(130, 0) == 0.5 and m.onset_f == 2 * 1.0 * 0.5 / 1.5
    assert m.precision(130, 1) == 0.5 and m.recall(130, 1) == 0.25 and m.offset_f == 2 * 0.5 * 0.25 / 0.75
    assert m.counts[0].tolist() == [[1, 4, 1], [0, 4, 1]] and m.counts[7].tolist() == [[0, 0, 1], [0, 0, 1]]
    assert m.multi_f == 0.0 and m.drum_onset_f == 0.0
    assert m.per_program()[0]["onset_f"] == 2 * 1.0 * 0.25 / 1.25 and set(m.per_program()) == {0, 7}
    assert m.summary()["onset_f"] == m.onset_f and m.summary()["skipped"] == (0, 0)
    assert NoteMetricCounts.from_flat(m.flat(), 130) == m
    with pytest.raises(ValueError, match="onset_tol"):
        note_metrics(ref, est, 130, onset_tol=float("nan"))
    with pytest.raises(ValueError, match="drum_program"):
        note_metrics(ref, est, 128)


def test_the_c_abi_declares_lists_and_exports_the_entry_points():
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    lib = _lib.load()
    for name in ("ymt3_metrics_create", "ymt3_metrics_destroy", "ymt3_note_metrics"):
        assert re.search(r"\b" + name + r"\s*\(ymt3_", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ymt3_metrics_s* ymt3_metrics;" in header and "} ymt3_metrics_params;" in header
    assert lib.ymt3_abi_version() == 3 and "#define YMT3_ABI_VERSION 3" in header
    body = header[header.index("typedef struct ymt3_metrics_params {"):header.index("} ymt3_metrics_params;")]
    assert re.findall(r"\b([a-z_]+)(?=[,;])", body) == [n for n, _ in _lib.MetricsParams._fields_]
    doc = header[header.index("/* Device note metrics"):header.index("typedef struct ymt3_metrics_params {")]
    for rule in ("rint(|a - b| * 1e4) / 1e4", "Drum notes never look at offsets", "drum_program if is_drum != 0", "read ON THE DEVICE",
                 "min(n, max(*count, 0))", "MAXIMUM one-to-one matching", "(n_programs + 1) * 6 + 2"):
        assert rule in doc, rule
