"""Piano roll and frame metrics on the GPU (include/ymt3.h, piano roll and frame metrics; yourmt3_amd/csrc/roll.hip).  The reference of
every comparison is the host specification, piano_roll and frame_metrics of yourmt3_amd/metrics.py, never the device path itself, and
every comparison is an equality of bytes or of integers:

  1. every case of tests/roll_cases.py: all (n_programs + 1) * 6 + 2 integers, and the roll of both sides for all rows and for the
     agnostic row alone; the sides' sizes read on the device through count pointers;
  2. the object's state: the same call twice, a small call after a large one against a fresh object, n_frames == max_frames;
  3. the refused arguments, with handle and object usable afterwards; destroy before and after the handle's destruction;
  4. the handle's decode state left alone; evaluate(frames=True) and piano_roll() end to end."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import roll_cases as C
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.metrics import FrameMetricCounts, frame_metrics, piano_roll
from yourmt3_amd.task_manager import NOTE_RECORD, Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
MAX_FRAMES = 1000
CASES = C.cases()
IDS = [c["id"] for c in CASES]
_p = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rig():
    """the model, and per parameter set a roll object with room for the largest case"""
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


def _roll(rig, case):
    m, objs = rig
    key = (case["n_programs"], case["drum_program"], case["fps"])
    if key not in objs:
        objs[key] = m.compile_piano_roll(case["n_programs"], MAX_FRAMES, case["fps"], case["drum_program"])
    return m, objs[key]


def to_pad(n: int) -> np.ndarray:
    """records that would count, and sound, if they were read"""
    pad = np.zeros(n, NOTE_RECORD)
    pad["onset"], pad["offset"], pad["pitch"] = 0.0, 0.2, 60
    return pad


def _dev(rec: np.ndarray, capacity: int = 0) -> torch.Tensor:
    """the records' bytes on the device, padded with records up to `capacity`"""
    return torch.from_numpy(np.concatenate([rec, to_pad(max(capacity - rec.size, 0))]).view(np.uint8).reshape(-1).copy()).cuda()


def _case(name):
    return next(c for c in CASES if c["id"] == name)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_equal_frame_metrics(rig, case):
    m, pr = _roll(rig, case)
    want = C.reference(case)[0].flat()
    got = pr.metrics(_dev(case["ref"]), _dev(case["est"]), case["n_frames"])
    assert got.dtype == torch.int64 and got.is_cuda and got.numel() == (case["n_programs"] + 1) * 6 + 2
    got = got.cpu().numpy()
    print(f"{case['id']}: {case['ref'].size} vs {case['est'].size} notes, agnostic row {want[-8:-2].tolist()}, skipped {want[-2:].tolist()}")
    assert np.array_equal(got, want), np.flatnonzero(got != want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_roll_equals_piano_roll(rig, case):
    m, pr = _roll(rig, case)
    for side, want in zip(("ref", "est"), C.reference(case)[1]):
        rec = _dev(case[side])
        got = pr.roll(rec, case["n_frames"])
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), side
        last = pr.roll(rec, case["n_frames"], rows="agnostic")
        assert tuple(last.shape) == (1,) + want.shape[1:] and np.array_equal(last.cpu().numpy(), want[-1:]), side
    # a range of rows in the middle, and records given on the host
    first = case["drum_program"]
    got = pr.roll(torch.from_numpy(case["est"].view(np.uint8).reshape(-1).copy()), case["n_frames"], rows=(first, 1))
    assert np.array_equal(got.cpu().numpy(), C.reference(case)[1][1][first:first + 1])


@pytest.mark.parametrize("name", ["random_400", "skipped_records", "frames_65"])
def test_the_sizes_read_on_the_device(rig, name):
    """n is the buffers' capacity; the count pointers say how many records each side has"""
    case = _case(name)
    m, pr = _roll(rig, case)
    ref, est, nf = case["ref"], case["est"], case["n_frames"]
    cap_r, cap_e = ref.size + 37, est.size + 5
    rd, ed = _dev(ref, cap_r), _dev(est, cap_e)
    full_r, full_e = np.concatenate([ref, to_pad(37)]), np.concatenate([est, to_pad(5)])
    count = lambda v: torch.tensor([v, 12345], dtype=torch.int32).cuda()                 # (a detokeniser's counter has a second element)
    # equal to the records given, smaller, zero, negative, equal to the buffer and more than it holds
    for cr, ce in ((ref.size, est.size), (ref.size // 2, est.size), (ref.size, est.size // 3), (0, est.size), (ref.size, -4), (cap_r, cap_e),
                   (cap_r + 100, cap_e + 100)):
        hr, he = full_r[:max(cr, 0)], full_e[:max(ce, 0)]
        got = pr.metrics(rd, ed, nf, ref_count=count(cr), est_count=count(ce)).cpu().numpy()
        assert np.array_equal(got, frame_metrics(hr, he, nf, **C.params(case)).flat()), (cr, ce)
        got = pr.roll(ed, nf, count=count(ce)).cpu().numpy()
        assert np.array_equal(got, piano_roll(he, nf, **C.params(case))), ce
    assert np.array_equal(pr.metrics(rd, ed, nf, ref_count=count(ref.size), est_count=count(est.size)).cpu().numpy(), C.reference(case)[0].flat())


def test_the_same_call_twice_and_a_small_call_after_a_large_one(rig):
    big, small = _case("random_400"), _case("frames_33")
    m, pr = _roll(rig, big)
    three = {**small, "ref": small["ref"][:3], "est": small["est"][1:4], "n_programs": big["n_programs"], "drum_program": big["drum_program"]}
    rd, ed = _dev(big["ref"]), _dev(big["est"])
    first = pr.metrics(rd, ed, big["n_frames"]).cpu().numpy()
    again = pr.metrics(rd, ed, big["n_frames"]).cpu().numpy()
    assert np.array_equal(first, again) and np.array_equal(first, C.reference(big)[0].flat())
    r1, r2 = pr.roll(rd, big["n_frames"]), pr.roll(rd, big["n_frames"])
    assert torch.equal(r1, r2) and int(r1.sum()) > 1000
    # 33 frames and 3 notes on the object that has just held 1000 frames of 131 rows, and on a fresh one
    fresh = m.compile_piano_roll(three["n_programs"], MAX_FRAMES, three["fps"], three["drum_program"])
    sr, se = _dev(three["ref"]), _dev(three["est"])
    want = frame_metrics(three["ref"], three["est"], 33, **C.params(three))
    assert want.counts[:, 1].sum() > 0
    for obj in (pr, fresh):
        assert np.array_equal(obj.metrics(sr, se, 33).cpu().numpy(), want.flat())
        assert np.array_equal(obj.roll(se, 33).cpu().numpy(), piano_roll(three["est"], 33, **C.params(three)))
    assert pr.metrics(sr, se, 0).cpu().numpy().tolist() == [0] * (131 * 6) + [0, 0] and tuple(pr.roll(se, 0).shape) == (131, 0, 128)
    fresh.close()
    with pytest.raises(ValueError, match="closed"):
        fresh.ptr


def test_n_frames_up_to_max_frames(rig):
    case = _case("frames_65")
    m = rig[0]
    pr = m.compile_piano_roll(case["n_programs"], 65, case["fps"], case["drum_program"])
    rd, ed = _dev(case["ref"]), _dev(case["est"])
    want, rolls = C.reference(case)
    assert np.array_equal(pr.metrics(rd, ed, 65).cpu().numpy(), want.flat()) and np.array_equal(pr.roll(rd, 65).cpu().numpy(), rolls[0])
    for call in (lambda: pr.metrics(rd, ed, 66), lambda: pr.roll(rd, 66), lambda: pr.metrics(rd, ed, -1)):
        with pytest.raises(_lib.YMT3Error, match="ymt3 error 1: n_frames"):
            call()
    assert np.array_equal(pr.metrics(rd, ed, 65).cpu().numpy(), want.flat()) and np.array_equal(pr.roll(ed, 65).cpu().numpy(), rolls[1])
    # skipped records are counted without a frame
    sk = _case("skipped_records")
    got = pr.metrics(_dev(sk["ref"]), _dev(sk["est"]), 0).cpu().numpy()
    assert got.tolist() == [0] * 24 + [8, 10] and np.array_equal(got, frame_metrics(sk["ref"], sk["est"], 0, **C.params(sk)).flat())
    pr.close()


def test_argument_errors_leave_everything_usable(rig):
    case = _case("frames_257")
    m, pr = _roll(rig, case)
    want, rolls = C.reference(case)
    nf, rows = case["n_frames"], case["n_programs"] + 1
    ref = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _dev(case["ref"])])[16:]  # (a view: its misaligned neighbours exist)
    est = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _dev(case["est"])])[16:]
    counts = torch.empty(want.flat().size + 1, dtype=torch.int64).cuda()
    roll = torch.empty(16 + rows * nf * 128, dtype=torch.uint8).cuda()

    def metrics(**over):
        a = dict(ref=_p(ref), n_ref=case["ref"].size, est=_p(est), n_est=case["est"].size, n_frames=nf, counts=_p(counts))
        a.update(over)
        rc = m._lib.ymt3_frame_metrics(m._handle, pr.ptr, a["ref"], a["n_ref"], None, a["est"], a["n_est"], None, a["n_frames"], a["counts"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def rolled(**over):
        a = dict(notes=_p(ref), n=case["ref"].size, n_frames=nf, first=0, n_rows=rows, roll=_p(roll))
        a.update(over)
        rc = m._lib.ymt3_piano_roll(m._handle, pr.ptr, a["notes"], a["n"], None, a["n_frames"], a["first"], a["n_rows"], a["roll"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    for over, word in [({"n_frames": MAX_FRAMES + 1}, "n_frames"), ({"n_frames": -1}, "n_frames"), ({"n_ref": -1}, "n_ref"), ({"n_est": -1}, "n_est"),
                       ({"n_ref": (1 << 29) + 1}, "n_ref"), ({"n_est": (1 << 29) + 1}, "n_est"), ({"counts": None}, "counts_dev"),
                       ({"ref": None}, "ref_notes_dev"), ({"est": None}, "est_notes_dev"),
                       ({"ref": ctypes.c_void_p(ref.data_ptr() + 4)}, "ref_notes_dev is not aligned"),
                       ({"est": ctypes.c_void_p(est.data_ptr() + 4)}, "est_notes_dev is not aligned"),
                       ({"counts": ctypes.c_void_p(counts.data_ptr() + 4)}, "counts_dev is not aligned")]:
        counts.fill_(-7)
        rc, msg = metrics(**over)
        assert rc == 1 and word in msg, (over, rc, msg)                  # YMT3_ERR_ARG, naming the argument
        assert int((counts != -7).sum()) == 0                            # nothing was launched
        rc, msg = metrics()
        assert rc == 0, msg
        assert np.array_equal(counts[:-1].cpu().numpy(), want.flat())
    for over, word in [({"n_frames": MAX_FRAMES + 1}, "n_frames"), ({"n_frames": -1}, "n_frames"), ({"n": -1}, "n_notes"), ({"n": (1 << 29) + 1}, "n_notes"),
                       ({"roll": None}, "roll_dev"), ({"notes": None}, "notes_dev"), ({"notes": ctypes.c_void_p(ref.data_ptr() + 4)}, "notes_dev is not aligned"),
                       ({"roll": ctypes.c_void_p(roll.data_ptr() + 8)}, "roll_dev is not aligned"), ({"first": -1}, "first_row"), ({"n_rows": 0}, "n_rows"),
                       ({"first": 1}, "n_rows"), ({"first": rows, "n_rows": 1}, "first_row"), ({"n_rows": rows + 1}, "n_rows")]:
        roll.fill_(7)
        rc, msg = rolled(**over)
        assert rc == 1 and word in msg, (over, rc, msg)
        assert int((roll != 7).sum()) == 0
        rc, msg = rolled()
        assert rc == 0, msg
        assert np.array_equal(roll[:rows * nf * 128].cpu().numpy().reshape(rows, nf, 128), rolls[0]) and int((roll[rows * nf * 128:] != 7).sum()) == 0
    # an empty side needs no pointer
    assert metrics(ref=None, n_ref=0)[0] == 0
    assert np.array_equal(counts[:-1].cpu().numpy(), frame_metrics(case["ref"][:0], case["est"], nf, **C.params(case)).flat())
    assert metrics(ref=None, n_ref=0, est=None, n_est=0)[0] == 0 and int(counts[:-1].abs().sum()) == 0
    assert rolled(notes=None, n=0)[0] == 0 and int(roll[:rows * nf * 128].sum()) == 0
    # ymt3_roll_create refuses what it cannot serve, and the handle goes on
    good = dict(frames_per_second=100.0, n_programs=130, drum_program=128)
    for change, max_frames, code, word in [({"frames_per_second": float("nan")}, 8, 1, "frames_per_second"), ({"frames_per_second": 0.0}, 8, 1, "frames_per_second"),
                                           ({"frames_per_second": -1.0}, 8, 1, "frames_per_second"), ({"frames_per_second": float("inf")}, 8, 1, "frames_per_second"),
                                           ({"n_programs": 0, "drum_program": 0}, 8, 1, "n_programs"), ({"drum_program": 130}, 8, 1, "drum_program"),
                                           ({"drum_program": -1}, 8, 1, "drum_program"), ({}, 0, 1, "max_frames"), ({}, (1 << 24) + 1, 1, "max_frames"),
                                           ({"n_programs": 257}, 8, 4, "n_programs")]:
        params = _lib.RollParams(**{**good, **change})
        obj = ctypes.c_void_p(1)
        rc = m._lib.ymt3_roll_create(m._handle, ctypes.byref(params), max_frames, ctypes.byref(obj))
        assert rc == code and obj.value is None and word in m._lib.ymt3_last_error().decode(), (change, rc, m._lib.ymt3_last_error().decode())
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_roll_create(m._handle, None, 8, ctypes.byref(obj)) == 1 and "params" in m._lib.ymt3_last_error().decode()
    m._lib.ymt3_roll_destroy(None)                                       # NULL is a no-op
    assert metrics()[0] == 0 and np.array_equal(counts[:-1].cpu().numpy(), want.flat())
    with pytest.raises(ValueError, match="NOTE_RECORD"):
        pr.metrics(torch.zeros(33, dtype=torch.uint8).cuda(), est, nf)
    with pytest.raises(ValueError, match="agnostic"):
        pr.roll(est, nf, rows="all")


def test_destroy_before_and_after_the_handle(rig):
    m2 = _model(CFG, max_batch=1)
    early = m2.compile_piano_roll(130, 8)
    early.close()                                                        # before the handle's destruction
    kept = m2.compile_piano_roll(130, 8)
    raw = ctypes.c_void_p()
    params = _lib.RollParams(100.0, 130, 128)
    assert m2._lib.ymt3_roll_create(m2._handle, ctypes.byref(params), 8, ctypes.byref(raw)) == 0 and raw.value
    m2.close()                                                           # closes `kept` with the model
    with pytest.raises(ValueError, match="closed"):
        kept.ptr
    m2._lib.ymt3_roll_destroy(raw)                                       # after the handle's destruction
    # the first model is untouched
    case = _case("polyphony")
    m, pr = _roll(rig, case)
    assert np.array_equal(pr.metrics(_dev(case["ref"]), _dev(case["est"]), case["n_frames"]).cpu().numpy(), C.reference(case)[0].flat())


def test_decode_is_the_same_before_and_after(rig):
    case = _case("random_400")
    m, pr = _roll(rig, case)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    counts = pr.metrics(_dev(case["ref"]), _dev(case["est"]), case["n_frames"])
    roll = pr.roll(_dev(case["est"]), case["n_frames"])
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    want, rolls = C.reference(case)
    assert np.array_equal(counts.cpu().numpy(), want.flat()) and np.array_equal(roll.cpu().numpy(), rolls[1])


TODAYS_KEYS = {"onset_f", "onset_p", "onset_r", "offset_f", "offset_p", "offset_r", "drum_onset_f", "multi_f", "per_program", "skipped", "counts"}


def test_evaluate_with_frames_and_piano_roll_end_to_end(rig, tmp_path):
    from yourmt3_amd.midi import write_midi
    from yourmt3_amd.transcribe import evaluate, piano_roll as device_roll, transcribe
    m = rig[0]
    # 5 segments of the small config, as tests/test_metrics.py transcribes them
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191), seed=3)[0].numpy()
    _, notes = transcribe(m, audio, bsz=2, output_dir=str(tmp_path), return_notes=True, device_detok=True)
    assert len(notes) > 0
    end_sec = audio.shape[-1] / CFG.sample_rate
    n_frames = max(1, math.ceil(end_sec * 100.0))
    # every second onset a few frames late, every offset late, every fourth pitch wrong, and three notes the model cannot have heard
    reference = [dataclasses.replace(x, onset=x.onset + 0.03 * (i % 2), offset=x.offset + 0.06, pitch=(x.pitch + 1) % 128 if i % 4 == 3 else x.pitch)
                 for i, x in enumerate(notes)]
    reference += [Note(0.10, 0.50, False, 7, 1), Note(1.00, 1.20, False, 99, 126), Note(0.30, 0.31, True, 128, 127)]
    res = evaluate(m, audio, reference, bsz=2, frames=True)
    want = frame_metrics(reference, notes, n_frames, 130)
    print(f"{len(notes)} notes over {n_frames} frames: {want}")
    assert res["n_frames"] == n_frames and np.array_equal(res["frame_counts"], want.counts)
    total = want.counts[:130].sum(0)
    assert 0 < total[0] < total[1]                                       # 0 < TP < N_REF over the aware rows: some cells right, some not
    for key, value in want.summary().items():
        if key != "frame_counts":
            assert res[key] == value, key
    assert set(res) == TODAYS_KEYS | {"frame_f", "frame_p", "frame_r", "frame_acc", "frame_err", "multi_frame_f", "frame_counts", "n_frames"}
    assert set(res["frame_err"]) == {"sub", "miss", "fa", "total"}
    plain = evaluate(m, audio, reference, bsz=2)
    assert set(plain) == TODAYS_KEYS and np.array_equal(plain["counts"], res["counts"])
    # another frame rate
    half = evaluate(m, audio, reference, bsz=2, frames=True, frames_per_second=50.0)
    assert half["n_frames"] == max(1, math.ceil(end_sec * 50.0))
    assert np.array_equal(half["frame_counts"], frame_metrics(reference, notes, half["n_frames"], 130, frames_per_second=50.0).counts)
    # against itself every sounding cell is right
    own = evaluate(m, audio, notes, bsz=2, frames=True)
    assert np.array_equal(own["frame_counts"], frame_metrics(notes, notes, n_frames, 130).counts) and own["multi_frame_f"] == 1.0
    # piano_roll(): the agnostic row, all rows, and a .mid path
    host = piano_roll(notes, n_frames, 130)
    got = device_roll(m, notes, end_sec)
    assert got.is_cuda and tuple(got.shape) == (n_frames, 128) and np.array_equal(got.cpu().numpy(), host[-1])
    assert np.array_equal(device_roll(m, notes, end_sec, per_program=True).cpu().numpy(), host)
    from yourmt3_amd.midi import read_midi_notes
    path = write_midi(notes, str(tmp_path / "ref.mid"))
    back = read_midi_notes(open(path, "rb").read())
    assert np.array_equal(device_roll(m, path, end_sec, frames_per_second=62.5).cpu().numpy(),
                          piano_roll(back, max(1, math.ceil(end_sec * 62.5)), 130, frames_per_second=62.5)[-1])
