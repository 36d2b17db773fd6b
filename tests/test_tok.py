"""Device tokeniser on the GPU (include/ymt3.h, device tokeniser; yourmt3_amd/csrc/tok.hip).  The reference of every comparison is the host
path, TaskManager.notes_to_tokens, never the device path itself:

  1. ids and lengths equal the host's exactly for every combination of n in {1, 2, 5}, K in {1, 13}, L in {8, 64, 65, 256, 1024} and
     max_shift_steps in {7, 206} (tests/tok_cases.py: random notes at arbitrary f64 times plus the listed special notes), and on every
     special and round-trip case of the CPU tests;
  2. overflowing rows, detokenise -> tokenise without a host copy of the records, a caller's stream, argument errors, the handle's decode
     state left alone;
  3. score_notes against model.score on the host's ids, a .mid path against its note list, the MoE refusal."""
import ctypes

import numpy as np
import pytest
import torch

import tok_cases as C
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd.config import FFN_MOE, YMT3Config
from yourmt3_amd.model import NOTE_RECORD
from yourmt3_amd.task_manager import Note

pytestmark = pytest.mark.gpu

CFG = {K: YMT3Config(segment_samples=8191, max_decode_len=1024, n_enc_layers=1, n_dec_layers=1, n_channels=K) for K in (1, 13)}
MAX_SEGMENTS = 5
_p = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rigs():
    """per channel count: the model, and per max_shift_steps a tokeniser with room for the largest case"""
    out = {K: (_model(cfg, max_batch=2 if K == 1 else 1), {}) for K, cfg in CFG.items()}
    yield out
    for m, _ in out.values():
        m.close()


def _rig(rigs, case):
    tm = C.task_manager(case["task"], case["ms"])
    m, toks = rigs[tm.num_decoding_channels]
    if case["ms"] not in toks:
        toks[case["ms"]] = m.compile_tokenizer(tm, MAX_SEGMENTS, 1024)
    return tm, m, toks[case["ms"]]


def _check(rigs, case):
    tm, m, t = _rig(rigs, case)
    ref_tokens, ref_lengths = C.reference(case)
    tokens, lengths = tm.notes_to_tokens_device(m, case["notes"], case["starts"], case["end_sec"], max_len=case["L"], tokenizer=t)
    print(f"{case['id']}: {len(case['notes'])} notes, {int(ref_lengths.sum())} tokens, longest row {int(ref_lengths.max())} of {case['L']}")
    assert tokens.dtype == torch.int32 and lengths.dtype == torch.int32 and tokens.is_cuda
    assert np.array_equal(lengths.cpu().numpy(), ref_lengths)
    assert np.array_equal(tokens.cpu().numpy(), ref_tokens)


@pytest.mark.parametrize("shape", C.MATRIX, ids=lambda s: "n%d-K%d-L%d-ms%d" % s)
def test_ids_and_lengths_equal_the_host_path(rigs, shape):
    _check(rigs, C.matrix_case(*shape))


@pytest.mark.parametrize("case", list(C.special_cases()) + list(C.grid_cases()), ids=lambda c: c["id"])
def test_special_and_round_trip_cases_equal_the_host_path(rigs, case):
    _check(rigs, case)


@pytest.mark.parametrize("K", [1, 13])
def test_overflowing_rows_report_their_length_and_the_wrapper_raises(rigs, K):
    case = next(c for c in C.special_cases() if c["name"] == "row_of_exactly_L" and c["task"] == C.TASK_OF_K[K])
    tm, m, t = _rig(rigs, case)
    _check(rigs, case)                                                                  # exactly L = 8 tokens: fits
    more = list(case["notes"]) + [Note(0.05, 9.0, False, 0, 65)]
    with pytest.raises(ValueError, match=r"segment 0 channel 0 needs 9 tokens > 8"):  # the host's error, word for word
        tm.notes_to_tokens_device(m, more, case["starts"], case["end_sec"], max_len=8, tokenizer=t)
    with pytest.raises(ValueError, match=r"segment 0 channel 0 needs 9 tokens > 8"):
        tm.notes_to_tokens(more, case["starts"], case["end_sec"], max_len=8)
    # more items than columns (40 copies of a note, L = 16), and a gap of more shift tokens than columns: a length > L, other rows intact
    crowd = [Note(0.1, 0.9, False, 0, 60)] * 40 + [Note(0.6, 0.7, False, 0, 61)]
    rec = torch.from_numpy(_records(crowd).view(np.uint8).reshape(-1)).cuda()
    tokens, lengths = t.run(rec, torch.tensor([0.0, 0.5], dtype=torch.float64), 1.0, 64)
    ref_tokens, ref_lengths = tm.notes_to_tokens(crowd, [0.0, 0.5], 1.0, max_len=64)
    assert np.array_equal(tokens.cpu().numpy(), ref_tokens) and np.array_equal(lengths.cpu().numpy(), ref_lengths)
    tokens, lengths = t.run(rec, torch.tensor([0.0, 0.5], dtype=torch.float64), 1.0, 16)
    assert int(lengths[0, 0]) > 16 and int(lengths[1, 0]) > 16
    if K == 13:
        assert np.array_equal(tokens[:, 1:].cpu().numpy(), ref_tokens[:, 1:, :16]) and np.array_equal(lengths[:, 1:].cpu().numpy(), ref_lengths[:, 1:])
    far = torch.from_numpy(_records([Note(0.0, 0.01, False, 0, 60), Note(400.0, 400.01, False, 0, 61)]).view(np.uint8).reshape(-1)).cuda()
    _, lengths = t.run(far, torch.tensor([0.0], dtype=torch.float64), 500.0, 32)
    assert int(lengths[0, 0]) > 32


def _records(notes) -> np.ndarray:
    rec = np.zeros(len(notes), NOTE_RECORD)
    for i, n in enumerate(notes):
        rec[i] = (n.onset, n.offset, n.program, n.pitch, bool(n.is_drum), float("nan"))
    return rec


@pytest.mark.parametrize("K", [1, 13])
def test_detokenize_then_tokenize_on_the_device_gives_the_ids_back(rigs, K):
    """ids the host tokeniser produced -> ymt3_detokenize -> its records, still on the device -> ymt3_tokenize: the same ids.  Only the
    note count crosses to the host."""
    case = next(c for c in C.grid_cases() if c["task"] == C.TASK_OF_K[K] and c["ms"] == 206 and len(c["starts"]) == 5 and "irregular" in c["id"])
    tm, m, t = _rig(rigs, case)
    ref_tokens, ref_lengths = C.reference(case)
    n, _, L = ref_tokens.shape
    d = m.compile_detokenizer(tm, n, L)
    tokens = torch.from_numpy(ref_tokens).cuda()
    starts = torch.tensor(case["starts"], dtype=torch.float64).cuda()
    records = torch.empty(n * K * L * NOTE_RECORD.itemsize, dtype=torch.uint8).cuda()
    counts = torch.zeros(2, dtype=torch.int32).cuda()
    _lib.check(m._lib.ymt3_detokenize(m._handle, d.ptr, _p(tokens), None, n, L, K * L, L, _p(starts), case["end_sec"], _p(records), n * K * L,
                                      _p(counts), m._stream()))
    n_notes, n_invalid = counts.tolist()
    assert n_notes == len(case["notes"]) and n_invalid == 0
    back, lengths = tm.notes_to_tokens_device(m, records[:n_notes * NOTE_RECORD.itemsize], case["starts"], case["end_sec"], max_len=L, tokenizer=t)
    assert torch.equal(back, tokens) and np.array_equal(lengths.cpu().numpy(), ref_lengths)
    d.close()


def test_a_callers_stream(rigs):
    case = C.matrix_case(5, 1, 256, 206)
    tm, m, t = _rig(rigs, case)
    ref_tokens, ref_lengths = C.reference(case)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tokens, lengths = tm.notes_to_tokens_device(m, case["notes"], case["starts"], case["end_sec"], max_len=256, tokenizer=t)
    stream.synchronize()
    assert np.array_equal(tokens.cpu().numpy(), ref_tokens) and np.array_equal(lengths.cpu().numpy(), ref_lengths)


def test_own_tokenizer_per_call_and_close_with_the_model(rigs):
    case = C.matrix_case(2, 1, 65, 7)
    tm = C.task_manager(case["task"], case["ms"])
    m = rigs[1][0]
    tokens, lengths = tm.notes_to_tokens_device(m, case["notes"], case["starts"], case["end_sec"], max_len=65)
    assert np.array_equal(tokens.cpu().numpy(), C.reference(case)[0])
    with pytest.raises(ValueError, match="strictly increasing"):
        tm.notes_to_tokens_device(m, [], [0.0, 1.0, 1.0], 2.0)
    with pytest.raises(ValueError, match="pitch"):
        tm.notes_to_tokens_device(m, [Note(0.0, 0.1, False, 0, 128)], [0.0], 2.0)
    m2 = _model(CFG[1], max_batch=1)
    t2 = m2.compile_tokenizer(tm, 2, 8)
    m2.close()
    with pytest.raises(ValueError, match="closed"):
        t2.ptr


def test_argument_errors_leave_everything_usable(rigs):
    case = C.matrix_case(5, 13, 64, 206)
    tm, m, t = _rig(rigs, case)
    ref_tokens, ref_lengths = C.reference(case)
    n, K, L = ref_tokens.shape
    rec = torch.from_numpy(np.concatenate([np.zeros(8, np.uint8), _records(case["notes"]).view(np.uint8).reshape(-1)])).cuda()
    notes, n_notes = rec[8:], len(case["notes"])
    starts = torch.tensor(case["starts"], dtype=torch.float64).cuda()
    tokens = torch.empty(n, K, L, dtype=torch.int32).cuda()
    lengths = torch.empty(n, K, dtype=torch.int32).cuda()

    def call(**over):
        a = dict(notes=_p(notes), n_notes=n_notes, starts=_p(starts), n=n, L=L, tokens=_p(tokens), lengths=_p(lengths))
        a.update(over)
        rc = m._lib.ymt3_tokenize(m._handle, t.ptr, a["notes"], a["n_notes"], a["starts"], a["n"], case["end_sec"], a["L"], a["tokens"], a["lengths"],
                                  m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    for over, word in [({"n": MAX_SEGMENTS + 1}, "n_segments"), ({"n": -1}, "n_segments"), ({"L": t.max_steps + 1}, "n_steps"), ({"L": 0}, "n_steps"),
                       ({"n_notes": -1}, "n_notes"), ({"notes": None}, "notes_dev"), ({"notes": ctypes.c_void_p(notes.data_ptr() + 4)}, "aligned"),
                       ({"starts": None}, "start_sec_dev"), ({"tokens": None}, "tokens_dev"), ({"lengths": None}, "lengths_dev")]:
        tokens.fill_(-7)
        rc, msg = call(**over)
        assert rc == 1 and word in msg, (over, rc, msg)                  # YMT3_ERR_ARG, naming the argument
        assert int((tokens != -7).sum()) == 0                            # nothing was launched
        rc, msg = call()
        assert rc == 0, msg
        assert np.array_equal(tokens.cpu().numpy(), ref_tokens) and np.array_equal(lengths.cpu().numpy(), ref_lengths)
    tokens.fill_(-7)
    assert call(n=0)[0] == 0 and int((tokens != -7).sum()) == 0          # no segments: a no-op
    assert call(n_notes=0, notes=None)[0] == 0                           # no notes: TIE, EOS rows
    empty = tm.notes_to_tokens([], case["starts"], case["end_sec"], max_len=L)
    assert np.array_equal(tokens.cpu().numpy(), empty[0]) and np.array_equal(lengths.cpu().numpy(), empty[1])
    # ymt3_tok_create refuses what it cannot serve, and the handle goes on
    fields, chan = tm.tok_params()
    for change, nprog, max_segments, max_steps, word in [({}, chan.size, 0, 8, "max_segments"), ({}, chan.size, 2, 1025, "max_steps"),
                                                         ({"drum_base": m.cfg.vocab - 100}, chan.size, 2, 8, "drum_base"),
                                                         ({"drum_program": 130}, chan.size, 2, 8, "drum_program"),
                                                         ({"steps_per_second": 0}, chan.size, 2, 8, "steps_per_second"), ({}, 0, 2, 8, "n_programs")]:
        params = _lib.TokParams(**{**fields, **change})
        obj = ctypes.c_void_p(1)
        rc = m._lib.ymt3_tok_create(m._handle, ctypes.byref(params), chan.ctypes.data, int(nprog), max_segments, max_steps, ctypes.byref(obj))
        assert rc == 1 and obj.value is None and word in m._lib.ymt3_last_error().decode(), (word, rc, m._lib.ymt3_last_error().decode())
    bad_chan = chan.copy()
    bad_chan[5] = 13
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_tok_create(m._handle, ctypes.byref(_lib.TokParams(**fields)), bad_chan.ctypes.data, int(chan.size), 2, 8, ctypes.byref(obj)) == 1
    assert "program_channel_host[5]" in m._lib.ymt3_last_error().decode()
    m._lib.ymt3_tok_destroy(None)                                        # NULL is a no-op
    assert call()[0] == 0


def test_decode_is_the_same_before_and_after(rigs):
    case = C.matrix_case(5, 1, 1024, 206)
    tm, m, t = _rig(rigs, case)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    _check(rigs, case)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)


@pytest.fixture(scope="module")
def e2e(rigs):
    m = rigs[1][0]
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191))[0].numpy()         # 5 segments of the small config
    d = lambda t, p: Note(t, t + 0.01, True, 128, p)
    notes = [Note(0.05, 0.31, False, 0, 60), Note(0.31, 0.9, False, 0, 60), Note(0.2, 2.1, False, 40, 55), d(0.1, 36), d(0.1, 42), d(1.3, 38),
             Note(0.62, 0.64, False, 24, 50), Note(1.1, 1.9, False, 24, 52), Note(1.15, 1.9, False, 24, 57), Note(2.2, 2.5, False, 0, 72),
             Note(2.3, 9.0, False, 40, 43)]
    return m, audio, notes


def test_score_notes_equals_score_on_the_hosts_ids(e2e):
    from yourmt3_amd.transcribe import score_notes
    m, audio, notes = e2e
    tm = C.task_manager("mt3_full_plus")
    res = score_notes(m, audio, notes, bsz=2)
    segments = m.ingest(torch.from_numpy(audio), m.cfg.sample_rate)
    n = segments.shape[0]
    assert n == 5
    starts = [i * m.cfg.segment_samples / m.cfg.sample_rate for i in range(n)]
    host_tokens, host_lengths = tm.notes_to_tokens(notes, starts, m.last_ingest_samples / m.cfg.sample_rate, max_len=1024)
    assert int(host_lengths.max()) > 10
    assert np.array_equal(res["tokens"].cpu().numpy(), host_tokens) and res["n_tokens"] == int(host_lengths.sum())
    ref = torch.cat([m.score(segments[i:i + 2], torch.from_numpy(host_tokens[i:i + 2]))[1] for i in range(0, n, 2)], 0).cpu().numpy()
    seg = res["segment_log_likelihood"]
    assert seg.dtype == np.float64 and seg.shape == (5, 1) and np.array_equal(seg, ref)       # bit for bit
    assert res["log_likelihood"] == float(ref.sum()) and np.isfinite(seg).all() and (seg < 0).all()
    print(f"log-likelihood {res['log_likelihood']:.3f} over {res['n_tokens']} tokens")


def test_score_notes_of_a_midi_file_equals_its_note_list(e2e, tmp_path):
    from yourmt3_amd.midi import write_midi
    from yourmt3_amd.transcribe import score_notes
    m, audio, notes = e2e
    # (a MIDI file holds the offset it is given, and the reader pairs a key's note-off with its latest note-on: no touching notes here)
    notes = [n for n in notes if n.offset < 5.0 and n.onset != 0.31]
    path = write_midi(notes, str(tmp_path / "notes.mid"))
    a, b = score_notes(m, audio, path, bsz=2), score_notes(m, audio, notes, bsz=2)
    assert torch.equal(a["tokens"], b["tokens"]) and a["n_tokens"] == b["n_tokens"]
    assert np.array_equal(a["segment_log_likelihood"], b["segment_log_likelihood"]) and a["log_likelihood"] == b["log_likelihood"]
    with pytest.raises(ValueError, match="no sub-tasks"):
        score_notes(m, audio, notes, subtask="drum-only")


def test_score_notes_refuses_the_moe_decoder():
    from yourmt3_amd.transcribe import score_notes
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, dec_ffn=FFN_MOE, n_experts=2, n_enc_layers=1, n_dec_layers=1, eos_id=-1)
    moe = _model(cfg, max_batch=1)
    audio = O.synthetic_audio(1, cfg, seed=1)[0].numpy()
    with pytest.raises(_lib.YMT3Error, match="dec_ffn"):
        score_notes(moe, audio, [Note(0.05, 0.2, False, 0, 60)])
    moe.close()
