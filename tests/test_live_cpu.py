"""Live transcription, the parts that need no GPU (include/ymt3.h: streaming ingest, incremental detokeniser):
  1. NoteStream -- the incremental form of note_events_to_notes and the specification of the device path -- returns, over every way of
     cutting every fuzz case of tests/detok_cases.py into pushes, exactly the one-shot notes (confidences and invalid count included), and
     never returns a note twice or changes one;
  2. the cases of tests/live_cases.py exercise every carry rule (counted on the host specification alone), and none but the one built for
     it reaches the held-hit bound;
  3. tests/live_model.py -- the kernel's algorithm in plain Python -- equals NoteStream push by push;
  4. ingest finality: the oracle's output for a prefix of the PCM agrees exactly with its output for the whole on the first
     max(0, ceil(N * up / down) - r) samples and not on the next, and the plan arithmetic equals a brute-force count;
  5. the C ABI: the new entry points are declared, listed and exported, the version stays 3, the package never imports the oracle."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import detok_cases as C
import live_cases as LC
import live_model as LM
from oracle import ingest_oracle as IO
from yourmt3_amd.task_manager import DRUM_PROGRAM, NoteStream, note_events_to_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. NoteStream
def _stream_case(case, groups_of_channel):
    """push the case through one NoteStream per channel -> (all notes returned, their count per call)"""
    _, _, per_channel = C.reference(case)
    tm = C.task_manager(case["task"])
    returned, bad = [], 0
    for ch, segs in enumerate(per_channel):
        groups = groups_of_channel(ch)
        st = NoteStream()
        seen = []
        for g, idx in enumerate(groups):
            got = st.push([segs[i] for i in idx], LC.horizon(case, groups, g))
            assert all(n.onset < LC.horizon(case, groups, g) or not n.is_drum for n in got)       # a hit at or past the horizon is held
            seen.append(got)
            bad += tm.detokenize_list_batches([case["tokens"][idx, ch]], [case["starts"][i] for i in idx], return_events=True)[1]
        seen.append(st.finish(case["end_sec"]))
        assert st.n_held == 0
        with pytest.raises(ValueError):
            st.push([], math.inf)
        returned += [n for got in seen for n in got]
    return returned, bad


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c["id"])
def test_note_stream_equals_the_one_shot_merge_for_every_split(case):
    ref_notes, ref_bad, _ = C.reference(case)
    n = case["tokens"].shape[0]
    named = LC.splits(n)
    for name, groups in named:
        got, bad = _stream_case(case, lambda ch: groups)
        # the union is the one-shot result; a note returned twice or altered after it was returned would make the multiset differ
        diff = C.same_notes(sorted(got), ref_notes)
        assert diff is None and bad == ref_bad, (name, diff)
    # another seeded split per channel
    got, bad = _stream_case(case, lambda ch: LC.splits(n, seed=ch + 1)[-1][1])
    assert C.same_notes(sorted(got), ref_notes) is None and bad == ref_bad


def test_note_stream_is_the_one_shot_function_on_one_push_and_checks_its_arguments():
    case = next(c for c in C.cases() if c["task"] == "mt3_full_plus" and c["family"] == "grammar" and c["tokens"].shape[0] == 7)
    segs = C.reference(case)[2][0]
    st = NoteStream()
    got = st.push(segs, math.inf) + st.finish(case["end_sec"])
    assert C.same_notes(sorted(got), note_events_to_notes(segs, case["end_sec"])) is None
    st.reset()
    st.push(segs[:3], segs[3][0])
    with pytest.raises(ValueError, match="strictly increasing"):
        st.push(segs[2:4], math.inf)                        # a segment not later than what was pushed
    with pytest.raises(ValueError, match="horizon"):
        st.push([], segs[1][0])                             # a horizon before the last pushed start
    with pytest.raises(ValueError, match="horizon"):
        NoteStream().push([], -math.inf)
    with pytest.raises(ValueError, match="horizon"):
        NoteStream().push([], math.nan)
    st.push(segs[3:], math.inf)
    st.finish(case["end_sec"])
    with pytest.raises(ValueError, match="finished"):
        st.finish(case["end_sec"])


# ---------------------------------------------------------------------------------------------- 2. coverage of live_cases
def test_live_cases_cover_every_carry_rule_and_stay_below_the_bound():
    total = dict.fromkeys(LC.KINDS, 0)
    for case in LC.cases():
        ref_notes, _, _ = LC.reference(case)
        for name, groups in LC.splits(case["tokens"].shape[0]):
            for k, v in LC.coverage(case, groups).items():
                total[k] += v
            pushes, last = LC.stream_reference(case, name)
            assert C.same_notes(sorted([n for p in pushes for n in p[0]] + list(last)), ref_notes) is None, (case["id"], name)
    print(total)
    assert all(total[k] > 0 for k in LC.KINDS), total
    # the hand-built cases alone already hold the three held-hit rules
    hand = dict.fromkeys(LC.KINDS, 0)
    for case in LC.hand_cases():
        for k, v in LC.coverage(case, [[i] for i in range(case["tokens"].shape[0])]).items():
            hand[k] += v
    assert hand["held_dedup_next_push"] and hand["held_raised"] and hand["held_over_two_pushes"], hand


def _model_pushes(case, groups):
    tm = C.task_manager(case["task"])
    m = LM.DetokCarry(tm.token_table(), tm.num_decoding_channels, tm.codec.steps_per_second, DRUM_PROGRAM, case["max_held"])
    out = []
    for g, idx in enumerate(groups):
        sc = None if case["scores"] is None else case["scores"][idx]
        out.append(m.push(case["tokens"][idx], [case["starts"][i] for i in idx], LC.horizon(case, groups, g), scores=sc))
    out.append(m.finish(case["end_sec"]))
    return out


def _to_notes(records):
    import detok_model as M
    return M.to_notes(records)


# ---------------------------------------------------------------------------------------------- 3. the kernel's algorithm == NoteStream
@pytest.mark.parametrize("case", LC.cases(), ids=lambda c: c["id"])
def test_model_equals_note_stream_push_by_push(case):
    built_for_the_bound = case["id"] == "hand-max-held"
    forced_total = 0
    for name, groups in LC.splits(case["tokens"].shape[0]):
        pushes, last = LC.stream_reference(case, name)
        got = _model_pushes(case, groups)
        forced = [f for _, _, f in got]
        forced_total += sum(forced)
        if not built_for_the_bound:
            assert sum(forced) == 0, (name, forced)           # no case but the one built for it reaches max_held
        if sum(forced):
            continue                                          # exactness is given up there: test_model_forces_the_earliest_hits
        for g, ((ref_notes, ref_bad, _), (records, bad, _)) in enumerate(zip(pushes, got)):
            diff = C.same_notes(_to_notes(records), list(ref_notes))
            assert diff is None and bad == ref_bad, (name, g, diff)
        assert C.same_notes(_to_notes(got[-1][0]), list(last)) is None, name
    assert (forced_total > 0) == built_for_the_bound


def test_model_forces_the_earliest_hits_when_the_bound_is_reached():
    case = next(c for c in LC.hand_cases() if c["id"] == "hand-max-held")
    groups = [[i] for i in range(case["tokens"].shape[0])]
    pushes, _ = LC.stream_reference(case, "every")
    got = _model_pushes(case, groups)
    held_by_host = pushes[0][2]                               # the unbounded host stream holds them all
    assert held_by_host == LC.SMALL_MAX_HELD + 3 and got[0][2] == 3
    first = sorted(r[0] for r in got[0][0] if r[4])
    all_ahead = sorted(n.onset for n in LC.reference(case)[0] if n.is_drum and n.onset >= case["starts"][1])
    assert first == all_ahead[:3]                             # earliest time first


# ---------------------------------------------------------------------------------------------- 4. ingest finality
RATE_PAIRS = [(44100, 100000), (48000, 70001), (8000, 20000), (22050, 30000), (16000, 20000), (44100, 37)]      # test_ingest_matches_oracle's


@pytest.mark.parametrize("sr,n", RATE_PAIRS)
def test_a_prefix_of_the_pcm_fixes_exactly_the_final_samples(sr, n):
    rng = np.random.default_rng(sr + n)
    x = (0.4 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr) + 0.1 * rng.standard_normal(n)).astype(np.float32)[:, None]
    S = 8191
    whole = IO.ingest(x, sr, 16000, S).reshape(-1)
    beyond = 0
    for N in sorted({0, 1, 2, n // 7, n // 3, n // 2, n - 1, n}):
        part = IO.ingest(x[:N], sr, 16000, S).reshape(-1)
        f = LC.final_samples(N, sr, 16000)
        assert f <= -(-N * 16000 // sr)
        assert np.array_equal(part[:f], whole[:f]), N         # the missing terms are exact zeros in the oracle's f64 sum
        # index f is the first sample that is NOT final, but it need not differ: it reads the one missing frame through tap 0 of its phase,
        # and the filter's zero pre-padding makes that tap exactly 0.0 for some phases.  The sample after it reads the frame through a
        # non-zero tap somewhere in the loop; that F itself is exact is pinned by the brute-force count over k0 below.
        if f < min(part.size, whole.size) - 1:
            beyond += part[f + 1] != whole[f + 1]
    if n > 1000:
        assert beyond > 0                                     # the rule is tight: the sample after the next one does differ somewhere


@pytest.mark.parametrize("sr", [44100, 48000, 8000, 22050, 16000, 11025, 96000])
def test_plan_arithmetic_equals_a_brute_force_count(sr):
    up, down = IO.rates(sr, 16000)
    _, r, hp = IO.plan(0, up, down)
    S = 257
    for N in list(range(0, 400)) + [4001, 30011]:
        n_out = -(-N * up // down)
        k0 = (np.arange(n_out + r + 4, dtype=np.int64) + r) * down // up          # the newest frame output n reads
        final = int(np.searchsorted(k0, N, side="left"))                          # outputs with k0 <= N - 1 (k0 is non-decreasing)
        assert LC.final_samples(N, sr, 16000) == final == max(0, n_out - r), (N, final)
        assert LC.plan_ready(N, sr, 16000, S) == final // S
    for k in (1, 2, 5):
        f = LC.first_frame_completing(k, sr, 16000, S)
        assert LC.plan_ready(f, sr, 16000, S) >= k > LC.plan_ready(f - 1, sr, 16000, S)


# ---------------------------------------------------------------------------------------------- 5. ABI
NEW = ("ymt3_ingest_stream_create", "ymt3_ingest_stream_destroy", "ymt3_ingest_stream_reset", "ymt3_ingest_stream_plan", "ymt3_ingest_stream_push",
       "ymt3_ingest_stream_finish", "ymt3_detok_state_create", "ymt3_detok_state_destroy", "ymt3_detok_state_reset", "ymt3_detok_state_carry",
       "ymt3_detokenize_push", "ymt3_detokenize_finish")


def test_entry_points_declared_listed_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(ymt3_", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ymt3_ingest_stream_s* ymt3_ingest_stream;" in header and "typedef struct ymt3_detok_state_s* ymt3_detok_state;" in header
    assert lib.ymt3_abi_version() == 3 and "#define YMT3_ABI_VERSION 3" in header
    assert lib.ymt3_detok_state_carry(None) == 0
    lib.ymt3_ingest_stream_destroy(None)
    lib.ymt3_detok_state_destroy(None)


def test_header_states_the_callers_obligations():
    header = " ".join(open(os.path.join(ROOT, "include", "ymt3.h")).read().split())
    ingest = header[header.index("/* Streaming ingest"):header.index("ymt3_ingest_stream_finish(ymt3_handle")]
    assert "max(0, ceil(N * up / down) - r)" in ingest and "BIT FOR BIT" in ingest and "non-finite" in ingest and "YMT3_ERR_ARG" in ingest
    detok = header[header.index("/* Incremental detokeniser"):header.index("ymt3_detokenize_finish(ymt3_handle")]
    assert "capacity >= n_segments * n_channels * n_steps + ymt3_detok_state_carry(st)" in detok
    assert "n_forced" in detok and "horizon_sec" in detok and "+inf" in detok and "YMT3_ERR_ARG" in detok


def test_the_package_never_imports_the_oracle():
    code = ("import sys; import yourmt3_amd, yourmt3_amd.transcribe, yourmt3_amd.task_manager, yourmt3_amd.model; "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for root, _, files in os.walk(os.path.join(ROOT, "yourmt3_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
