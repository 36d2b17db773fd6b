"""Token scores on the host (include/ymt3.h, token scores): the scored oracle pinned to HF T5's `generate(output_scores=True)` +
`compute_transition_scores(normalize_logits=True)`, note confidences in TaskManager, min_confidence and the C header."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from score_oracle import scored_greedy_decode, scores_from_logits
from test_importer import CFG, _hf, _imported
from yourmt3_amd.task_manager import DRUM_NOTE_SEC, Note, NoteEvent, TaskManager, drop_low_confidence, note_events_to_notes
from yourmt3_amd.vocab import Event, EOS, PAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_setup():
    m = _hf()
    W = _imported(m)
    a = O.synthetic_audio(2, CFG)
    enc = O.encoder_t5(O.input_projection(O.logmel(a, CFG), W, bf16=False), W, CFG, bf16=False)
    return m, W, enc


@pytest.mark.parametrize("prompted", [False, True], ids=["plain", "prompted"])
def test_scored_oracle_matches_hf_transition_scores(prompted):
    """fp32 both sides: the same ids exactly, the scores to round-off (the importer's mapping of an HF T5)."""
    from transformers.modeling_outputs import BaseModelOutput
    m, W, enc = _hf_setup()
    n = 12
    prompt = torch.tensor([[[599, 598]], [[601, 598]]], dtype=torch.int32) if prompted else None
    toks, scores, _ = scored_greedy_decode(enc, W, CFG, n, bf16=False, prompt=prompt)
    start = torch.full((2, 1), CFG.pad_id, dtype=torch.long)
    dec_in = start if prompt is None else torch.cat([start, prompt[:, 0].long()], 1)
    with torch.no_grad():
        out = m.generate(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=dec_in, max_new_tokens=n,
                         do_sample=False, num_beams=1, output_scores=True, return_dict_in_generate=True)
        ref = m.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    ref_tokens = out.sequences[:, dec_in.shape[1]:]
    L = ref_tokens.shape[1]
    assert L >= 8                                           # (HF stops once every row has emitted EOS)
    assert torch.equal(toks[:, 0, :L].long(), ref_tokens)
    # HF goes on scoring PAD after a row's EOS; the rule here is 0.0 there: compare up to each row's EOS
    eos = (ref_tokens == CFG.eos_id).int()
    live = (eos.cumsum(-1) - eos) == 0
    d = (scores[:, 0, :L] - ref.double()).abs()[live]
    assert d.max().item() < 1e-4
    assert (scores <= 0).all()


def test_scored_oracle_teacher_forced_sum_is_hf_log_likelihood():
    """With forcing, the sum of a row is the log-likelihood of the forced sequence: HF's mean cross-entropy times its length."""
    from transformers.modeling_outputs import BaseModelOutput
    m, W, enc = _hf_setup()
    n = 10
    g = torch.Generator().manual_seed(7)
    forced = torch.randint(3, CFG.vocab, (2, 1, n), generator=g, dtype=torch.int32)
    _, scores, _ = scored_greedy_decode(enc, W, CFG, n, bf16=False, forced=forced)
    for b in range(2):
        with torch.no_grad():
            loss = m(encoder_outputs=BaseModelOutput(last_hidden_state=enc[b:b + 1]), labels=forced[b:b + 1, 0].long()).loss
        assert abs(scores[b, 0].sum().item() + n * loss.item()) < 1e-3 * n
    # forced ids are scored whatever the argmax was, so they are mostly not the maximum: scores well below 0
    assert scores.mean().item() < -1.0


def test_score_rules_eos_pad_and_forced():
    V = 8
    logits = torch.randn(1, 1, 5, V, generator=torch.Generator().manual_seed(0))
    cfg = CFG.with_(eos_id=1)
    toks = torch.tensor([[[4, 1, 0, 0, 0]]], dtype=torch.int32)          # EOS at column 1, then PAD
    s = scores_from_logits(logits, toks, cfg)
    lp = torch.log_softmax(logits.double(), -1)
    assert s[0, 0, 0] == lp[0, 0, 0, 4] and s[0, 0, 1] == lp[0, 0, 1, 1]
    assert (s[0, 0, 2:] == 0.0).all()
    # forced: every column scores the forced id (clamped), EOS or not
    forced = torch.tensor([[[1, 2, 99, -5, 3]]], dtype=torch.int32)
    sf = scores_from_logits(logits, toks, cfg, forced)
    ids = [1, 2, V - 1, 0, 3]
    assert all(sf[0, 0, i] == lp[0, 0, i, ids[i]] for i in range(5))
    # EOS off: no zeroing
    s_off = scores_from_logits(logits, toks, cfg.with_(eos_id=-1))
    assert (s_off != 0).all()


# ---------------------------------------------------------------- TaskManager confidences
def _two_segments(tm):
    """Segment 0 at 0 s: a piano onset (C4, scored -0.1), a drum hit twice at one time (-2.0, then -0.5: one hit), EOS.
    Segment 1 at 1 s: C4 in the tie section (still sounding), then its offset at 1.2 s, a second piano onset (E4, -0.3), EOS."""
    c = tm.codec
    e = lambda *a: c.encode(Event(*a))
    seg0 = [e("tie", 0), e("shift", 10), e("velocity", 1), e("program", 0), e("pitch", 60), e("drum", 36), e("drum", 36), EOS, PAD]
    sc0 = [-9.0, -9.0, -9.0, -9.0, -0.1, -2.0, -0.5, -9.0, 0.0]
    seg1 = [e("program", 0), e("pitch", 60), e("tie", 0), e("shift", 20), e("velocity", 0), e("program", 0), e("pitch", 60),
            e("velocity", 1), e("pitch", 64), EOS]
    sc1 = [-9.0, -9.0, -9.0, -9.0, -9.0, -9.0, -4.0, -9.0, -0.3, -9.0]
    L = 12
    toks = np.full((2, 1, L), PAD, np.int32)
    scores = np.zeros((2, 1, L), np.float32)
    toks[0, 0, :len(seg0)], scores[0, 0, :len(sc0)] = seg0, sc0
    toks[1, 0, :len(seg1)], scores[1, 0, :len(sc1)] = seg1, sc1
    return toks, scores


def test_decode_segment_stores_onset_scores():
    tm = TaskManager()
    toks, scores = _two_segments(tm)
    ev, ties, bad = tm.tokenizer.decode_segment(toks[1, 0], 1.0, scores[1, 0])
    assert bad == 0 and ties == [(0, 60)]
    assert [(e.velocity, e.pitch, e.score) for e in ev] == [(0, 60, None), (1, 64, pytest.approx(-0.3))]
    plain, _, _ = tm.tokenizer.decode_segment(toks[1, 0], 1.0)
    assert plain == ev and all(e.score is None for e in plain)          # the score takes no part in equality


def test_tokens_to_notes_confidence():
    tm = TaskManager()
    toks, scores = _two_segments(tm)
    starts = [0.0, 1.0]
    plain = tm.tokens_to_notes([toks[:1], toks[1:]], starts, end_sec=2.0)
    scored = tm.tokens_to_notes([toks[:1], toks[1:]], starts, end_sec=2.0, score_batches=[scores[:1], scores[1:]])
    # without scores: the notes as before, no confidence
    assert all(n.confidence is None for n in plain)
    assert plain == [Note(0.1, 0.1 + DRUM_NOTE_SEC, True, 128, 36), Note(0.1, 1.2, False, 0, 60), Note(1.2, 2.0, False, 0, 64)]
    # with scores: the same notes (equality ignores confidence), each with exp(score) of its onset
    assert scored == plain
    conf = {(n.is_drum, n.pitch): n.confidence for n in scored}
    assert conf[(True, 36)] == pytest.approx(math.exp(-0.5))            # the de-duplicated drum hit keeps the larger one
    assert conf[(False, 60)] == pytest.approx(math.exp(-0.1))           # onset in segment 0, tie and offset in segment 1
    assert conf[(False, 64)] == pytest.approx(math.exp(-0.3))
    assert len({hash(n) for n in scored} | {hash(n) for n in plain}) == 3


def test_note_events_to_notes_without_scores_unchanged():
    segs = [(0.0, [NoteEvent(0.1, False, 0, 1, 60), NoteEvent(0.2, True, 128, 1, 36), NoteEvent(0.2, True, 128, 1, 36)], []),
            (1.0, [NoteEvent(1.5, False, 0, 0, 60)], [(0, 60)])]
    notes = note_events_to_notes(segs, 2.0)
    assert notes == [Note(0.1, 1.5, False, 0, 60), Note(0.2, 0.2 + DRUM_NOTE_SEC, True, 128, 36)]
    assert all(n.confidence is None for n in notes)


def test_scores_must_match_tokens():
    tm = TaskManager()
    toks, scores = _two_segments(tm)
    with pytest.raises(ValueError, match="scores"):
        tm.tokens_to_notes([toks], [0.0, 1.0], end_sec=2.0, score_batches=[scores[:, :, :5]])


def test_min_confidence_filtering():
    notes = [Note(0.0, 1.0, False, 0, 60, confidence=0.9), Note(0.5, 1.0, False, 0, 62, confidence=0.2),
             Note(0.7, 0.71, True, 128, 36, confidence=0.5), Note(0.8, 1.0, False, 0, 64)]
    assert drop_low_confidence(notes, 0.5) == [notes[0], notes[2], notes[3]]
    assert drop_low_confidence(notes, 0.0) == notes
    assert drop_low_confidence(notes[:3], 1.01) == []


class _ScoreRecorder:
    """Stands in for YourMT3 on the CPU: records what transcribe() asks for; returns one C4 note per segment, scored -0.7."""
    def __init__(self, cfg, tm):
        self.cfg, self.tm, self.calls = cfg, tm, []

    def ingest(self, pcm, sample_rate):
        self.last_ingest_samples = pcm.shape[0]
        return torch.zeros(2, 1, self.cfg.segment_samples)

    def _out(self, n, L):
        c = self.tm.codec
        t = np.full((n, 1, L), PAD, np.int32)
        t[:, 0, :5] = [c.encode(Event("tie", 0)), c.encode(Event("velocity", 1)), c.encode(Event("program", 0)), c.encode(Event("pitch", 60)), EOS]
        s = np.zeros((n, 1, L), np.float32)
        s[:, 0, 3] = -0.7
        return t, s

    def inference_file(self, bsz, segments, max_token_length=None, **kw):
        self.calls.append(("file", sorted(kw)))
        t, s = self._out(segments.shape[0], max_token_length)
        return ([t], [s]) if kw.get("return_scores") else [t]

    def inference_stream(self, segments, max_token_length=None, slots=0, **kw):
        self.calls.append(("stream", sorted(kw)))
        t, s = self._out(segments.shape[0], max_token_length)
        return (torch.from_numpy(t), torch.from_numpy(s)) if kw.get("return_scores") else torch.from_numpy(t)


def test_transcribe_confidence_paths(tmp_path):
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.transcribe import transcribe
    tm = TaskManager()
    model = _ScoreRecorder(YMT3Config(), tm)
    audio = np.zeros(16000, np.float32)
    _, plain = transcribe(model, audio, task_manager=tm, output_dir=str(tmp_path), return_notes=True)
    assert model.calls == [("file", [])] and plain and all(n.confidence is None for n in plain)
    for continuous in (False, True):
        model.calls = []
        _, notes = transcribe(model, audio, task_manager=tm, output_dir=str(tmp_path), return_notes=True, confidence=True,
                              continuous=continuous)
        assert model.calls == [("stream" if continuous else "file", ["return_scores"])]
        assert notes == plain and all(n.confidence == pytest.approx(math.exp(-0.7)) for n in notes)
        _, kept = transcribe(model, audio, task_manager=tm, output_dir=str(tmp_path), return_notes=True, min_confidence=0.4,
                             continuous=continuous)
        assert kept == plain
        _, none = transcribe(model, audio, task_manager=tm, output_dir=str(tmp_path), return_notes=True, min_confidence=0.6,
                             continuous=continuous)
        assert none == []


def test_header_declares_the_scored_entry_points():
    from yourmt3_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    for name in ("ymt3_decode_scored", "ymt3_transcribe_segments_scored", "ymt3_transcribe_stream_scored"):
        assert f"int {name}(" in hdr, name
        assert name in _lib.SYMBOLS, name
    assert "#define YMT3_ABI_VERSION 3" in hdr
