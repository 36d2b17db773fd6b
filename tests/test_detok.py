"""Device detokeniser on the GPU (include/ymt3.h, device detokeniser; yourmt3_amd/csrc/detok.hip).  The reference of every comparison is the
host path (TaskManager.detokenize_list_batches + note_events_to_notes; tokens_to_notes for 13 channels), never the device path itself:

  1. fuzz: the cases of tests/detok_cases.py (three token families, L in {1, 5, 64, 65, 130, 1024}, 1..65 segments, 1 and 13 channels, with
     and without scores, NaN and -inf among them, regular and irregular start times) give equal notes (== on Note), equal confidences as
     Python floats and an equal invalid-token count -- after the cases were checked, on the reference alone, to cover every merge rule;
  2. strides (a beam call's hypothesis 0 read in place), poisoned ids, argument errors, non-increasing start times, the handle's decode
     state left alone;
  3. transcribe(device_detok=True) writes the same notes and the same MIDI bytes as the host path in every mode."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import detok_cases as C
from oracle import ymt3_oracle as O
from test_gpu_parity import SMALL, _model
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.model import NOTE_RECORD

pytestmark = pytest.mark.gpu

CFG = {1: dataclasses.replace(SMALL, max_decode_len=1024), 13: YMT3Config(segment_samples=8191, max_decode_len=256, n_channels=13)}
MAX_SEGMENTS = 65


@pytest.fixture(scope="module")
def rigs():
    """per channel count: the model, and per task a detokeniser with room for the largest case"""
    out = {}
    for K, cfg in CFG.items():
        m = _model(cfg, max_batch=1)
        out[K] = (m, {})
    yield out
    for m, _ in out.values():
        m.close()


def _rig(rigs, task):
    tm = C.task_manager(task)
    m, detoks = rigs[tm.num_decoding_channels]
    if task not in detoks:
        detoks[task] = m.compile_detokenizer(tm, MAX_SEGMENTS, min(tm.max_note_token_length, m.cfg.max_decode_len))
    return tm, m, detoks[task]


def test_reference_covers_every_merge_rule():
    total = dict.fromkeys(C.KINDS, 0)
    for case in C.cases():
        for k, v in C.coverage(case).items():
            total[k] += v
    assert all(total[k] > 0 for k in C.KINDS), total


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c["id"])
def test_fuzz_equals_host_path(rigs, case):
    tm, m, d = _rig(rigs, case["task"])
    ref_notes, ref_bad, _ = C.reference(case)
    tokens = torch.from_numpy(case["tokens"]).cuda()
    scores = None if case["scores"] is None else torch.from_numpy(case["scores"]).cuda()
    notes, bad = tm.tokens_to_notes_device(m, tokens, case["starts"], case["end_sec"], scores=scores, detokenizer=d)
    print(f"{case['id']}: {case['tokens'].size} tokens, {len(ref_notes)} notes, {ref_bad} invalid")
    assert bad == ref_bad
    diff = C.same_notes(notes, ref_notes)
    assert diff is None, diff
    assert all((n.confidence is None) == (scores is None) for n in notes)


def test_own_detokenizer_per_call_and_close_with_the_model(rigs):
    case = next(c for c in C.cases() if c["task"] == "mt3_full_plus" and c["family"] == "dense" and c["tokens"].shape[2] == 130)
    tm, m, _ = _rig(rigs, case["task"])
    notes, bad = tm.tokens_to_notes_device(m, torch.from_numpy(case["tokens"]).cuda(), case["starts"], case["end_sec"])
    ref_notes, ref_bad, _ = C.reference(case)
    assert bad == ref_bad and C.same_notes(notes, ref_notes) is None
    m2 = _model(SMALL, max_batch=1)
    d2 = m2.compile_detokenizer(tm, 2, 8)
    m2.close()
    with pytest.raises(ValueError, match="closed"):
        d2.ptr


def test_hypothesis_zero_strides_equal_the_contiguous_copy(rigs):
    case = next(c for c in C.cases() if c["task"] == "mc13_full_plus_256" and c["family"] == "dense" and c["tokens"].shape[2] == 65)
    tm, m, d = _rig(rigs, case["task"])
    rng = np.random.default_rng(5)
    n, K, L = case["tokens"].shape
    beams = torch.from_numpy(rng.integers(0, tm.vocab_size, (n, K, 2, L)).astype(np.int32)).cuda()
    beams[:, :, 0] = torch.from_numpy(case["tokens"]).cuda()
    sc = torch.from_numpy((-rng.random((n, K, 2, L))).astype(np.float32)).cuda()
    view, sview = beams[:, :, 0], sc[:, :, 0]
    assert not view.is_contiguous() and view.stride() == (K * 2 * L, 2 * L, 1)
    got = tm.tokens_to_notes_device(m, view, case["starts"], case["end_sec"], scores=sview, detokenizer=d)
    ref = tm.tokens_to_notes_device(m, view.contiguous(), case["starts"], case["end_sec"], scores=sview.contiguous(), detokenizer=d)
    assert got[1] == ref[1] and C.same_notes(got[0], ref[0]) is None
    host = tm.tokens_to_notes([case["tokens"]], case["starts"], case["end_sec"], [sview.cpu().numpy()])
    assert C.same_notes(got[0], host) is None


def test_poisoned_ids_are_invalid_and_give_no_notes(rigs):
    tm, m, d = _rig(rigs, "mt3_full_plus")
    tokens = np.full((3, 1, 130), np.iinfo(np.int32).min, np.int32)
    starts = [0.0, 2.0, 4.0]
    _, ref_bad = tm.detokenize_list_batches([tokens[:, 0]], starts, return_events=True)
    notes, bad = tm.tokens_to_notes_device(m, torch.from_numpy(tokens).cuda(), starts, 5.0, detokenizer=d)
    assert notes == [] and bad == ref_bad == 3 * 130


def test_argument_errors_leave_everything_usable(rigs):
    tm, m, d = _rig(rigs, "mt3_full_plus")
    case = next(c for c in C.cases() if c["task"] == "mt3_full_plus" and c["family"] == "grammar" and c["tokens"].shape[2] == 65)
    n, K, L = case["tokens"].shape
    tokens = torch.from_numpy(case["tokens"]).cuda()
    scores = None if case["scores"] is None else torch.from_numpy(case["scores"]).cuda()
    starts = torch.tensor(case["starts"], dtype=torch.float64).cuda()
    notes = torch.empty(n * K * L * NOTE_RECORD.itemsize, dtype=torch.uint8).cuda()
    counts = torch.zeros(2, dtype=torch.int32).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(**over):
        a = dict(tokens=p(tokens), scores=None if scores is None else p(scores), n=n, L=L, starts=p(starts), notes=p(notes), capacity=n * K * L, counts=p(counts))
        a.update(over)
        rc = m._lib.ymt3_detokenize(m._handle, d.ptr, a["tokens"], a["scores"], a["n"], a["L"], K * L, L, a["starts"], case["end_sec"],
                                    a["notes"], a["capacity"], a["counts"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    for over, word in [({"n": MAX_SEGMENTS + 1, "capacity": 1 << 40}, "n_segments"), ({"L": d.max_steps + 1, "capacity": 1 << 40}, "n_steps"),
                       ({"tokens": None}, "tokens_dev"), ({"starts": None}, "start_sec_dev"), ({"notes": None}, "notes_dev"),
                       ({"counts": None}, "counts_dev"), ({"capacity": n * K * L - 1}, "capacity")]:
        rc, msg = call(**over)
        assert rc == 1 and word in msg, (over, rc, msg)                  # YMT3_ERR_ARG, naming the argument
        rc, msg = call()
        assert rc == 0, msg
        torch.cuda.synchronize()
        ref_notes, ref_bad, _ = C.reference(case)
        assert counts.tolist() == [len(ref_notes), ref_bad]
    got, bad = tm.tokens_to_notes_device(m, tokens, case["starts"], case["end_sec"], scores=scores, detokenizer=d)
    assert C.same_notes(got, C.reference(case)[0]) is None


def test_non_increasing_start_times_raise(rigs):
    tm, m, d = _rig(rigs, "mt3_full_plus")
    tokens = torch.zeros(3, 1, 8, dtype=torch.int32).cuda()
    for starts in ([0.0, 2.0, 2.0], [0.0, 3.0, 1.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            tm.tokens_to_notes_device(m, tokens, starts, 9.0, detokenizer=d)
    with pytest.raises(ValueError, match="start times"):
        tm.tokens_to_notes_device(m, tokens, [0.0, 1.0], 9.0, detokenizer=d)


def test_decode_is_the_same_before_and_after(rigs):
    tm, m, d = _rig(rigs, "mt3_full_plus")
    audio = O.synthetic_audio(1, m.cfg)
    before = m.inference(audio, max_token_length=24)
    case = next(c for c in C.cases() if c["task"] == "mt3_full_plus" and c["family"] == "dense" and c["tokens"].shape[2] == 1024)
    tm.tokens_to_notes_device(m, torch.from_numpy(case["tokens"]).cuda(), case["starts"], case["end_sec"], detokenizer=d)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    notes, bad = tm.tokens_to_notes_device(m, after, [0.0], 2.0, detokenizer=d)          # decoded ids, straight from the device
    segs, ref_bad = tm.detokenize_list_batches([after[:, 0].cpu().numpy()], [0.0], return_events=True)
    from yourmt3_amd.task_manager import note_events_to_notes
    assert bad == ref_bad and notes == note_events_to_notes(segs, 2.0)


@pytest.mark.parametrize("mode", [{}, {"continuous": True}, {"confidence": True}, {"num_beams": 2}, {"confidence": True, "num_beams": 2},
                                  {"constrained": True, "continuous": True, "confidence": True}],
                         ids=["default", "continuous", "confidence", "beams", "beams-confidence", "constrained-continuous-confidence"])
def test_transcribe_device_detok_equals_host_path(e2e, tmp_path, mode):
    from yourmt3_amd.transcribe import transcribe
    m, audio = e2e
    kw = dict(bsz=2, max_token_length=40, return_notes=True, **mode)
    host_path, host = transcribe(m, audio, output_dir=str(tmp_path / "host"), **kw)
    dev_path, dev = transcribe(m, audio, output_dir=str(tmp_path / "dev"), device_detok=True, **kw)
    assert C.same_notes(dev, host) is None, C.same_notes(dev, host)
    assert open(dev_path, "rb").read() == open(host_path, "rb").read()
    print(f"{mode}: {len(host)} notes")


@pytest.fixture(scope="module")
def e2e():
    m = _model(SMALL, max_batch=4)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191))[0].numpy()         # 5 segments of the small config
    yield m, audio
    m.close()
