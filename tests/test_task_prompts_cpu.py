"""Task prompts on the host (include/ymt3.h, task prompts): the prompted oracle loop pinned to HF T5's
`generate(decoder_input_ids=[[pad, *prompt]])`, the task tokens of TaskManager and what the detokenizer does with them."""
import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from prompt_oracle import prompted_greedy_decode
from test_importer import CFG, _hf, _imported
from yourmt3_amd.task_manager import TASK_TOKEN_NAMES, TaskManager
from yourmt3_amd.vocab import Codec, Event, EOS, PAD


def test_prompted_oracle_matches_hf_generate_with_decoder_input_ids():
    """fp32 both sides, the importer's mapping of an HF T5: same emitted ids, logits to round-off, per-row prompts of one length.
    This pins the start id / prompt / first emitted token alignment to third-party code."""
    from transformers.modeling_outputs import BaseModelOutput
    m = _hf()
    W = _imported(m)
    a = O.synthetic_audio(2, CFG)
    enc = O.encoder_t5(O.input_projection(O.logmel(a, CFG), W, bf16=False), W, CFG, bf16=False)
    prompt = torch.tensor([[[599, 598]], [[601, 598]]], dtype=torch.int32)          # (B, K, P): a different prefix per row
    n = 12
    toks, logits = prompted_greedy_decode(enc, W, CFG, prompt, n, bf16=False, return_logits=True)
    start = torch.full((2, 1), CFG.pad_id, dtype=torch.long)
    with torch.no_grad():
        out = m.generate(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=torch.cat([start, prompt[:, 0].long()], 1),
                         max_new_tokens=n, min_new_tokens=n, do_sample=False, num_beams=1, output_logits=True, return_dict_in_generate=True)
    ref_tokens = out.sequences[:, 1 + prompt.shape[-1]:]
    ref_logits = torch.stack(out.logits, 1)
    assert ref_tokens.shape == (2, n)
    assert (logits[:, 0] - ref_logits).abs().max().item() < 5e-4
    assert torch.equal(toks[:, 0].long(), ref_tokens)
    # the prompt matters: the unprompted stream is another one
    free = O.greedy_decode(enc, W, CFG, n, bf16=False)
    assert not torch.equal(free, toks)
    # P = 0 is the plain loop
    t0, l0 = prompted_greedy_decode(enc, W, CFG, prompt[..., :0], n, bf16=False, return_logits=True)
    f0, fl0 = O.greedy_decode(enc, W, CFG, n, bf16=False, return_logits=True)
    assert torch.equal(t0, f0) and torch.equal(l0, fl0)


def test_task_token_ids_and_prompts():
    tm = TaskManager("singing_drum_v1")
    size = Codec().size
    assert size == 598
    assert tm.task_token_ids == {n: size + i for i, n in enumerate(TASK_TOKEN_NAMES)}
    assert tm.task_token_ids == {"task": 598, "transcribe_all": 599, "transcribe_singing": 600, "transcribe_drum": 601}
    assert tm.num_decoding_channels == 1 and tm.max_note_token_length == 1024
    assert sorted(tm.subtasks) == ["default", "drum-only", "singing-only"]
    p = tm.task_prompt("drum-only", 3)
    assert p.shape == (3, 1, 2) and p.dtype == np.int32 and (p == np.array([601, 598])).all()
    assert (tm.task_prompt(None, 1) == tm.task_prompt("default", 1)).all() and tm.task_prompt(None, 1).tolist() == [[[599, 598]]]
    assert tm.task_prompt("singing-only", 2).tolist() == [[[600, 598]]] * 2
    with pytest.raises(ValueError, match="sub-task"):
        tm.task_prompt("piano-only", 1)
    with pytest.raises(ValueError, match="no task tokens"):
        TaskManager().task_prompt("default", 1)
    # the table entry a real checkpoint's ids would override
    tm2 = TaskManager("singing_drum_v1", task_token_ids={"transcribe_drum": 1000})
    assert tm2.task_prompt("drum-only", 1).tolist() == [[[1000, 598]]]
    with pytest.raises(ValueError, match="unknown task token"):
        TaskManager("singing_drum_v1", task_token_ids={"piano": 700})
    with pytest.raises(ValueError, match="codec event"):
        TaskManager("singing_drum_v1", task_token_ids={"task": 100})


def test_task_tokens_must_fit_the_vocabulary():
    with pytest.raises(ValueError, match="vocabulary of 600"):
        TaskManager("singing_drum_v1", vocab_size=600)
    TaskManager("singing_drum_v1", vocab_size=602)
    TaskManager("mt3_full_plus", vocab_size=600)           # a task without task tokens needs no room for them


def test_detokenizer_skips_task_tokens_only_for_tasks_that_define_them():
    tm = TaskManager("singing_drum_v1")
    c = tm.codec
    body = [c.encode(Event("tie", 0)), c.encode(Event("shift", 10)), c.encode(Event("velocity", 1)), c.encode(Event("program", 0)),
            c.encode(Event("pitch", 60)), EOS, PAD]
    plain, ties, bad = tm.tokenizer.decode_segment(body, 0.0)
    assert bad == 0 and len(plain) == 1
    with_tt = [601, 598] + body[:3] + [598] + body[3:]
    ev, ties2, bad2 = tm.tokenizer.decode_segment(with_tt, 0.0)
    assert (ev, ties2, bad2) == (plain, ties, 0)
    # the existing tasks: the same ids are invalid tokens, exactly as before
    for name in ("mt3_full_plus", "mc13_full_plus_256"):
        old = TaskManager(name)
        assert old.task_token_ids == {} and old.subtasks == {}
        ev3, _, bad3 = old.tokenizer.decode_segment(with_tt, 0.0)
        assert ev3 == plain and bad3 == 3


def test_existing_tasks_unchanged_on_the_known_answer_stream():
    """The known-answer stream of test_task_manager.py through both existing tasks and the new one."""
    from yourmt3_amd.task_manager import NoteEvent
    for name in ("mt3_full_plus", "mc13_full_plus_256", "singing_drum_v1"):
        tm = TaskManager(name)
        c = tm.codec
        toks = [c.encode(Event("program", 40)), c.encode(Event("pitch", 64)), c.encode(Event("tie", 0)),
                c.encode(Event("shift", 10)), c.encode(Event("velocity", 1)), c.encode(Event("program", 0)), c.encode(Event("pitch", 60)),
                c.encode(Event("shift", 40)), c.encode(Event("velocity", 0)), c.encode(Event("pitch", 60)), EOS] + [PAD] * 5
        ev, ties, bad = tm.tokenizer.decode_segment(toks, 0.0)
        assert ties == [(40, 64)] and bad == 0
        assert ev == [NoteEvent(0.1, False, 0, 1, 60), NoteEvent(0.5, False, 0, 0, 60)]
        arr = np.array(toks, np.int32)[None, None, :]
        segs = tm.detokenize_list_batches([arr[:, 0]], [0.0])
        assert segs == [(0.0, ev, ties)]


class _PromptRecorder:
    """Stands in for YourMT3 on the CPU: records the task tokens transcribe() passes and returns an empty stream."""
    def __init__(self, cfg):
        self.cfg, self.calls = cfg, []

    def ingest(self, pcm, sample_rate):
        self.last_ingest_samples = pcm.shape[0]
        return torch.zeros(2, 1, self.cfg.segment_samples)

    def inference_file(self, bsz, segments, max_token_length=None, task_tokens=None):
        self.calls.append(("file", max_token_length, None if task_tokens is None else task_tokens.tolist()))
        return [np.zeros((segments.shape[0], 1, max_token_length), np.int32)]

    def inference_stream(self, segments, max_token_length=None, slots=0, task_tokens=None):
        self.calls.append(("stream", max_token_length, None if task_tokens is None else task_tokens.tolist()))
        return torch.zeros(segments.shape[0], 1, max_token_length, dtype=torch.int32)


def test_transcribe_passes_the_subtask_prompt(tmp_path):
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.transcribe import transcribe
    model = _PromptRecorder(YMT3Config())
    audio = np.zeros(16000, np.float32)
    tm = TaskManager("singing_drum_v1")
    transcribe(model, audio, task_manager=tm, subtask="drum-only", output_dir=str(tmp_path))
    transcribe(model, audio, task_manager=tm, output_dir=str(tmp_path), continuous=True)
    transcribe(model, audio, task_manager=TaskManager(), output_dir=str(tmp_path))
    # the prompt's steps come out of the decode length: 2 + 1022 = the 1024-position cache
    assert model.calls == [("file", 1022, [601, 598]), ("stream", 1022, [599, 598]), ("file", 1024, None)]
    with pytest.raises(ValueError, match="no sub-tasks"):
        transcribe(model, audio, task_manager=TaskManager(), subtask="drum-only", output_dir=str(tmp_path))
