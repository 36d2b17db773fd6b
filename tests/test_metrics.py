"""Note metrics on the GPU (include/ymt3.h, note metrics; yourmt3_amd/csrc/metrics.hip).  The reference of every comparison is the host
specification, note_metrics of yourmt3_amd/metrics.py, never the device path itself, and every comparison is an integer equality:

  1. every case of tests/metrics_cases.py: all (n_programs + 1) * 6 + 2 integers, with the sides' sizes given by the host and again by
     count pointers read on the device (smaller than the buffer, zero, negative);
  2. ymt3_detokenize's records and counter fed straight in as the estimate; evaluate() against the model's own transcription and against a
     reference shifted by 60 ms; a caller's stream; the handle's decode state left alone;
  3. the refused arguments, with handle and object usable afterwards."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import detok_cases as D
import metrics_cases as C
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.metrics import NoteMetricCounts, note_metrics, to_records
from yourmt3_amd.task_manager import NOTE_RECORD, Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
MAX_NOTES = 2048
CASES = C.cases()
IDS = [c["id"] for c in CASES]
_p = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rig():
    """the model, and per parameter set a metrics object with room for the largest case"""
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


def _metrics(rig, params):
    m, objs = rig
    key = tuple(sorted(params.items()))
    if key not in objs:
        objs[key] = m.compile_note_metrics(max_ref=MAX_NOTES, max_est=MAX_NOTES, **params)
    return m, objs[key]


def _dev(rec: np.ndarray, capacity: int = 0) -> torch.Tensor:
    """the records' bytes on the device, padded with records of garbage up to `capacity`"""
    pad = np.zeros(max(capacity - rec.size, 0), NOTE_RECORD)
    pad["onset"], pad["offset"], pad["pitch"] = 1.0, 1.5, 60                             # would count, and hit, if they were read
    return torch.from_numpy(np.concatenate([rec, pad]).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_equal_note_metrics(rig, case):
    m, nm = _metrics(rig, case["params"])
    want = C.reference(case).flat()
    got = nm.run(_dev(case["ref"]), _dev(case["est"]))
    assert got.dtype == torch.int32 and got.is_cuda and got.numel() == (case["params"]["n_programs"] + 1) * 6 + 2
    got = got.cpu().numpy()
    print(f"{case['id']}: {case['ref'].size} vs {case['est'].size} notes, agnostic row {want[-8:-2].tolist()}, skipped {want[-2:].tolist()}")
    assert np.array_equal(got, want), np.flatnonzero(got != want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_with_the_sizes_read_on_the_device(rig, case):
    """n is the buffers' capacity; the count pointers say how many records each side has"""
    m, nm = _metrics(rig, case["params"])
    ref, est = case["ref"], case["est"]
    cap_r, cap_e = ref.size + 37, est.size + 5
    rd, ed = _dev(ref, cap_r), _dev(est, cap_e)
    count = lambda v: torch.tensor([v, 12345], dtype=torch.int32).cuda()                 # (a detokeniser's counter has a second element)
    got = nm.run(rd, ed, ref_count=count(ref.size), est_count=count(est.size)).cpu().numpy()
    assert np.array_equal(got, C.reference(case).flat())
    # smaller than the records given, zero, negative, and more than the buffer holds
    for cr, ce in ((ref.size // 2, est.size), (ref.size, est.size // 3), (0, est.size), (ref.size, -4), (cap_r + 100, cap_e + 100)):
        want = note_metrics(np.concatenate([ref, to_pad(cap_r - ref.size)])[:max(cr, 0)], np.concatenate([est, to_pad(cap_e - est.size)])[:max(ce, 0)],
                            **case["params"]).flat()
        got = nm.run(rd, ed, ref_count=count(cr), est_count=count(ce)).cpu().numpy()
        assert np.array_equal(got, want), (cr, ce)


def to_pad(n: int) -> np.ndarray:
    pad = np.zeros(n, NOTE_RECORD)
    pad["onset"], pad["offset"], pad["pitch"] = 1.0, 1.5, 60
    return pad


def test_detokenizer_output_in_place_as_the_estimate(rig):
    """ids -> ymt3_detokenize -> its notes_dev and counts_dev, untouched, as the estimate: equal to note_metrics on the host-detokenised notes"""
    m = rig[0]
    case = next(c for c in D.cases() if c["task"] == "mt3_full_plus" and c["family"] == "dense" and c["tokens"].shape[2] == 130)
    tm = D.task_manager(case["task"])
    big = _model(dataclasses.replace(CFG, max_decode_len=130), max_batch=1)
    n, K, L = case["tokens"].shape
    d = big.compile_detokenizer(tm, n, L)
    host_notes = D.reference(case)[0]
    assert len(host_notes) > 50
    rng = np.random.default_rng(7)
    est_rows = [(x.onset, x.offset, x.program, x.pitch, x.is_drum) for x in host_notes]
    ref = C.records(C.perturbed(rng, est_rows))
    nm = big.compile_note_metrics(130, ref.size, d.capacity)
    notes_dev, counts_dev = d.run_device(torch.from_numpy(case["tokens"]).cuda(), None, torch.tensor(case["starts"], dtype=torch.float64), case["end_sec"])
    assert notes_dev.numel() == d.capacity * NOTE_RECORD.itemsize
    got = nm.run(_dev(ref), notes_dev, est_count=counts_dev).cpu().numpy()
    assert int(counts_dev[0]) == len(host_notes)
    want = note_metrics(ref, host_notes, 130)
    print(f"{len(host_notes)} notes: {want}")
    assert np.array_equal(got, want.flat()) and want.counts[130, 0, 0] > 10
    big.close()


@pytest.fixture(scope="module")
def e2e(rig, tmp_path_factory):
    from yourmt3_amd.transcribe import transcribe
    m = rig[0]
    # 5 segments of the small config; on the CPU oracle this seed transcribes into 17 notes, drum hits and one pitched note
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191), seed=3)[0].numpy()
    _, notes = transcribe(m, audio, bsz=2, output_dir=str(tmp_path_factory.mktemp("midi")), return_notes=True, device_detok=True)
    return m, audio, notes


def test_evaluate_against_the_models_own_transcription(e2e):
    from yourmt3_amd.transcribe import evaluate
    m, audio, notes = e2e
    assert len(notes) > 0
    res = evaluate(m, audio, notes, bsz=2)
    counts = res["counts"]
    print(f"{len(notes)} notes, rows with notes: {np.flatnonzero(counts[:, 0, 1]).tolist()}")
    assert np.array_equal(counts, note_metrics(notes, notes, 130).counts) and res["skipped"] == (0, 0)
    assert np.array_equal(counts[:, :, 0], counts[:, :, 1]) and np.array_equal(counts[:, :, 0], counts[:, :, 2])     # TP = n_ref = n_est
    full = NoteMetricCounts(counts, res["skipped"])
    for row in np.flatnonzero(counts[:, 0, 1]):
        assert full.f_measure(int(row), 0) == 1.0 and full.f_measure(int(row), 1) == 1.0
    pitched, drums = sum(not x.is_drum for x in notes), sum(x.is_drum for x in notes)
    assert res["onset_f"] == res["offset_f"] == (1.0 if pitched else 0.0) and res["drum_onset_f"] == (1.0 if drums else 0.0)
    assert res["multi_f"] == 1.0 and set(res["per_program"]) == {128 if x.is_drum else x.program for x in notes}


def test_evaluate_against_a_reference_shifted_by_60_ms(e2e, tmp_path):
    from yourmt3_amd.midi import write_midi
    from yourmt3_amd.transcribe import evaluate
    m, audio, notes = e2e
    shifted = [dataclasses.replace(x, onset=x.onset + 0.06, offset=x.offset + 0.06) for x in notes]
    res = evaluate(m, audio, shifted, bsz=2, continuous=True)
    want = note_metrics(shifted, notes, 130)
    assert np.array_equal(res["counts"], want.counts)
    assert int(res["counts"][:, :, 0].sum()) == 0 and res["onset_f"] == 0.0                # no onset within 50 ms any more
    assert np.array_equal(res["counts"][:, :, 1:], note_metrics(notes, notes, 130).counts[:, :, 1:])
    wide = evaluate(m, audio, shifted, bsz=2, onset_tol=0.06, offset_min_tol=0.06)      # a wider window finds them again
    assert np.array_equal(wide["counts"], note_metrics(shifted, notes, 130, onset_tol=0.06, offset_min_tol=0.06).counts)
    assert np.array_equal(wide["counts"][:, :, 0], wide["counts"][:, :, 1])
    # a .mid path is read into the same notes as the list it was written from
    path = write_midi(notes, str(tmp_path / "ref.mid"))
    from yourmt3_amd.midi import read_midi_notes
    back = read_midi_notes(open(path, "rb").read())
    assert np.array_equal(evaluate(m, audio, path, bsz=2)["counts"], note_metrics(back, notes, 130).counts)


def test_a_callers_stream_and_close_with_the_model(rig):
    case = next(c for c in CASES if c["id"] == "130_programs")
    m, nm = _metrics(rig, case["params"])
    stream = torch.cuda.Stream()
    rd, ed = _dev(case["ref"]), _dev(case["est"])
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = nm.run(rd, ed)
    stream.synchronize()
    assert np.array_equal(got.cpu().numpy(), C.reference(case).flat())
    m2 = _model(CFG, max_batch=1)
    nm2 = m2.compile_note_metrics(130, 8, 8)
    m2.close()
    with pytest.raises(ValueError, match="closed"):
        nm2.ptr


def test_decode_is_the_same_before_and_after(rig):
    case = next(c for c in CASES if c["id"] == "dense_64_x_64")
    m, nm = _metrics(rig, case["params"])
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    got = nm.run(_dev(case["ref"]), _dev(case["est"]))
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    assert np.array_equal(got.cpu().numpy(), C.reference(case).flat())


def test_argument_errors_leave_everything_usable(rig):
    case = next(c for c in CASES if c["id"] == "bucket_65")
    m, nm = _metrics(rig, case["params"])
    want = C.reference(case).flat()
    ref = torch.cat([torch.zeros(8, dtype=torch.uint8).cuda(), _dev(case["ref"])])[8:]    # (a view: its misaligned neighbours exist)
    est = torch.cat([torch.zeros(8, dtype=torch.uint8).cuda(), _dev(case["est"])])[8:]
    counts = torch.empty(want.size, dtype=torch.int32).cuda()

    def call(**over):
        a = dict(ref=_p(ref), n_ref=case["ref"].size, est=_p(est), n_est=case["est"].size, counts=_p(counts))
        a.update(over)
        rc = m._lib.ymt3_note_metrics(m._handle, nm.ptr, a["ref"], a["n_ref"], None, a["est"], a["n_est"], None, a["counts"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    for over, word in [({"n_ref": MAX_NOTES + 1}, "n_ref"), ({"n_est": MAX_NOTES + 1}, "n_est"), ({"n_ref": -1}, "n_ref"), ({"n_est": -1}, "n_est"),
                       ({"counts": None}, "counts_dev"), ({"ref": None}, "ref_notes_dev"), ({"est": None}, "est_notes_dev"),
                       ({"ref": ctypes.c_void_p(ref.data_ptr() + 4)}, "ref_notes_dev is not aligned"),
                       ({"est": ctypes.c_void_p(est.data_ptr() + 4)}, "est_notes_dev is not aligned")]:
        counts.fill_(-7)
        rc, msg = call(**over)
        assert rc == 1 and word in msg, (over, rc, msg)                  # YMT3_ERR_ARG, naming the argument
        assert int((counts != -7).sum()) == 0                            # nothing was launched
        rc, msg = call()
        assert rc == 0, msg
        assert np.array_equal(counts.cpu().numpy(), want)
    # an empty side needs no pointer
    assert call(ref=None, n_ref=0)[0] == 0
    assert np.array_equal(counts.cpu().numpy(), note_metrics(case["ref"][:0], case["est"], **case["params"]).flat())
    assert call(ref=None, n_ref=0, est=None, n_est=0)[0] == 0 and int(counts.abs().sum()) == 0
    # ymt3_metrics_create refuses what it cannot serve, and the handle goes on
    good = dict(onset_tol=0.05, offset_min_tol=0.05, offset_ratio=0.2, n_programs=130, drum_program=128)
    for change, max_ref, max_est, code, word in [({"onset_tol": float("nan")}, 8, 8, 1, "onset_tol"), ({"onset_tol": -0.01}, 8, 8, 1, "onset_tol"),
                                                 ({"offset_min_tol": float("inf")}, 8, 8, 1, "offset_min_tol"), ({"offset_ratio": -1.0}, 8, 8, 1, "offset_ratio"),
                                                 ({"n_programs": 0, "drum_program": 0}, 8, 8, 1, "n_programs"), ({"drum_program": 130}, 8, 8, 1, "drum_program"),
                                                 ({"drum_program": -1}, 8, 8, 1, "drum_program"), ({}, 0, 8, 1, "max_ref"), ({}, 8, 0, 1, "max_est"),
                                                 ({}, (1 << 24) + 1, 8, 1, "max_ref"), ({}, 8, (1 << 24) + 1, 1, "max_est"),
                                                 ({"n_programs": 257}, 8, 8, 4, "n_programs")]:
        params = _lib.MetricsParams(**{**good, **change})
        obj = ctypes.c_void_p(1)
        rc = m._lib.ymt3_metrics_create(m._handle, ctypes.byref(params), max_ref, max_est, ctypes.byref(obj))
        assert rc == code and obj.value is None and word in m._lib.ymt3_last_error().decode(), (change, rc, m._lib.ymt3_last_error().decode())
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_metrics_create(m._handle, None, 8, 8, ctypes.byref(obj)) == 1 and "params" in m._lib.ymt3_last_error().decode()
    m._lib.ymt3_metrics_destroy(None)                                    # NULL is a no-op
    assert call()[0] == 0 and np.array_equal(counts.cpu().numpy(), want)
    with pytest.raises(ValueError, match="NOTE_RECORD"):
        nm.run(torch.zeros(33, dtype=torch.uint8).cuda(), est)
    # 256 programs is the most the kernels key: accepted
    nm256 = m.compile_note_metrics(256, 8, 8, drum_program=255)
    rec = C.records([(1.0, 1.5, 254, 60, False), (1.0, 1.5, 255, 36, False), (1.0, 1.5, 256, 60, False)])
    assert np.array_equal(nm256.run(_dev(rec), _dev(rec)).cpu().numpy(), note_metrics(rec, rec, 256, drum_program=255).flat())
    nm256.close()
