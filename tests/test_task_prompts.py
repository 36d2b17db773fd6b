"""Task prompts on the GPU (include/ymt3.h, task prompts): a prefix of task tokens fed to the decoder before it emits.

  - P = 0 through the *_prompted entry points is the unprompted call, bit for bit, in every decode regime;
  - a prompted call equals the unprompted call over P + N steps teacher-forced with [prompt, its own ids]: ids and logits of the
    emitted steps bit for bit (the prompt only changes what is fed, never the arithmetic);
  - prompted ids / logits against the prompted oracle loop (tests/prompt_oracle.py) and against HF T5 itself;
  - per-row prompts, EOS inside a prompt, early stop, continuous batching, argument errors and the end-to-end path.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from prompt_oracle import prompted_greedy_decode
from test_gpu_parity import _check_ids, _model
from yourmt3_amd import _lib
from yourmt3_amd.config import FFN_MOE, YMT3Config
from yourmt3_amd.task_manager import TaskManager

pytestmark = pytest.mark.gpu

SMALL = YMT3Config(segment_samples=8191, max_decode_len=64, eos_id=-1)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _prompt(B, K, P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 1536, (B, K, P), generator=g, dtype=torch.int32)


def _decode_p0(m, e, n, forced=None, logits=False):
    """ymt3_decode_prompted with n_prompt = 0 and a NULL prompt"""
    cfg = m.cfg
    B = e.shape[0]
    t = torch.empty(B, cfg.n_channels, n, device=m.device, dtype=torch.int32)
    lg = torch.empty(B, cfg.n_channels, n, cfg.vocab, device=m.device, dtype=torch.float32) if logits else None
    _lib.check(m._lib.ymt3_decode_prompted(m._handle, _p(e), B, n, None, 0, _p(t), _p(forced), _p(lg), m._stream()))
    return t, lg


# (name, config changes, environment at create, segments)
REGIMES = [
    ("merged", {}, {}, 4),
    ("separate", {}, {"YMT3_NO_ATTN_PAIR": "1", "YMT3_NO_GEMM_CHAIN": "1"}, 4),
    ("two_chains", {}, {}, 224),
    ("ticket_no_fold", {}, {}, 100),          # one chain beyond 96 rows: the argmax kernel's two-level ticket, the self-O GEMM launched
    ("two_wave_self_attn", {}, {}, 264),      # beyond 2048 (row, head) pairs: the 2-waves-per-(row, head) self-attention
    ("mc13", {"n_channels": 13, "max_decode_len": 32}, {}, 2),
    ("moe_fp8", {"dec_ffn": FFN_MOE, "moe_fp8": 1}, {}, 4),
    ("step_kernel", {}, {"YMT3_STEP_KERNEL": "1"}, 4),
    ("no_graph", {}, {"YMT3_NO_GRAPH": "1"}, 4),
]


@pytest.mark.parametrize("name,cfg_kw,env,B", REGIMES, ids=[r[0] for r in REGIMES])
def test_prompt_regimes_identity_and_self_consistency(name, cfg_kw, env, B, monkeypatch):
    cfg = SMALL.with_(**cfg_kw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(cfg, max_batch=B)
    for k in env:
        monkeypatch.delenv(k)
    K = cfg.n_channels
    a = O.synthetic_audio(8, cfg, seed=11)
    a = a.repeat(-(-B // 8), 1)[:B] * torch.linspace(0.5, 1.0, B)[:, None]      # B different segments
    a = a.cuda()
    e = m.encode(m.logmel(a))
    N = 24 if cfg.max_decode_len <= 32 else 40
    P = 3
    # 1. P = 0 through the new entry points: bit-identical ids and logits
    t_old, l_old = m.decode(e, N, return_logits=True)
    t_new, l_new = _decode_p0(m, e, N, logits=True)
    assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old)
    free = m.decode(e, N)
    assert torch.equal(_decode_p0(m, e, N)[0], free)
    if name == "two_chains":
        assert m.last_decode_chains == 2
    nseg = min(B, 4)
    seg = torch.empty(nseg, K, N, device=m.device, dtype=torch.int32)
    _lib.check(m._lib.ymt3_transcribe_segments_prompted(m._handle, _p(a[:nseg]), nseg, N, None, 0, _p(seg), m._stream()))
    ref_seg = m.inference(a[:nseg], max_token_length=N)
    assert torch.equal(seg, ref_seg)
    st = torch.empty(nseg, K, N, device=m.device, dtype=torch.int32)
    _lib.check(m._lib.ymt3_transcribe_stream_prompted(m._handle, _p(a[:nseg]), nseg, N, None, 0, _p(st), 2, 4, m._stream()))
    assert torch.equal(st, m.inference_stream(a[:nseg], max_token_length=N, slots=2, interval=4))
    assert torch.equal(st, ref_seg)
    # 2. prompted (prompt p, N steps) == unprompted over P + N steps teacher-forced with cat(p, prompted ids): bit for bit
    p = _prompt(B, K, P, seed=5).cuda()
    tp, lp = m.decode(e, N, prompt=p, return_logits=True)
    if name == "two_chains":
        assert m.last_decode_chains == 2
    assert m.last_decode_steps == P + N
    tf, lf = m.decode(e, P + N, forced=torch.cat([p, tp], -1), return_logits=True)
    assert torch.equal(tf[..., P:], tp) and torch.equal(lf[..., P:, :], lp)
    assert not torch.equal(tp, free)                                    # the prompt is not ignored
    assert torch.equal(m.decode(e, N, prompt=p), tp)                    # free-running prompted == its own teacher-forced run
    # the prompted whole path and the prompted stream give the same ids
    ps = p[:nseg]
    seg_p = m.inference(a[:nseg], task_tokens=ps, max_token_length=N)
    assert torch.equal(seg_p, tp[:nseg]) if nseg == B else torch.equal(seg_p, m.decode(e[:nseg], N, prompt=ps))
    assert torch.equal(m.inference_stream(a[:nseg], max_token_length=N, slots=2, interval=4, task_tokens=ps), seg_p)
    m.close()


def test_prompted_ids_and_logits_match_the_oracle_over_128_positions():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=160, eos_id=-1)
    m = _model(cfg, max_batch=2)
    a = O.synthetic_audio(2, cfg, seed=3)
    _, enc = O.encode(a, m.weights, cfg, True)
    p = torch.tensor([[[599, 598]], [[601, 598]]], dtype=torch.int32)
    n = 128
    feed = prompted_greedy_decode(enc, m.weights, cfg, p, n, True)
    ref_t, ref_l = prompted_greedy_decode(enc, m.weights, cfg, p, n, True, forced=feed, return_logits=True)
    got_t, got_l = m.decode(enc.bfloat16().cuda(), n, forced=feed.cuda(), return_logits=True, prompt=p.cuda())
    _check_ids("prompted_small_128_teacher_forced", got_t, ref_t, ref_l, got_l)
    m.close()


def test_prompted_13_channels_match_the_oracle():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=32, n_channels=13, eos_id=-1)
    m = _model(cfg, max_batch=2)
    a = O.synthetic_audio(2, cfg, seed=4)
    _, enc = O.encode(a, m.weights, cfg, True)
    p = _prompt(2, 13, 2, seed=9)                                        # a different prefix for every (segment, channel)
    n = 24
    feed = prompted_greedy_decode(enc, m.weights, cfg, p, n, True)
    ref_t, ref_l = prompted_greedy_decode(enc, m.weights, cfg, p, n, True, forced=feed, return_logits=True)
    got_t, got_l = m.decode(enc.bfloat16().cuda(), n, forced=feed.cuda(), return_logits=True, prompt=p.cuda())
    _check_ids("prompted_mc13_teacher_forced", got_t, ref_t, ref_l, got_l)
    m.close()


def test_prompted_hip_path_on_imported_weights_matches_hf_t5_directly():
    from transformers.modeling_outputs import BaseModelOutput
    from test_importer import CFG, _hf, _imported
    from yourmt3_amd.model import YourMT3
    hf = _hf()
    W = _imported(hf)
    model = YourMT3(CFG, W, device=0, max_batch=2)
    enc = model.encode(model.logmel(O.synthetic_audio(2, CFG).cuda()))
    p = torch.tensor([[[599, 598]], [[600, 598]]], dtype=torch.int32)
    n = 10
    start = torch.full((2, 1), CFG.pad_id, dtype=torch.long)
    with torch.no_grad():
        out = hf.generate(encoder_outputs=BaseModelOutput(last_hidden_state=enc.float().cpu()), decoder_input_ids=torch.cat([start, p[:, 0].long()], 1),
                          max_new_tokens=n, min_new_tokens=n, do_sample=False, num_beams=1, output_logits=True, return_dict_in_generate=True)
    hf_tokens = out.sequences[:, 1 + p.shape[-1]:]
    hf_logits = torch.stack(out.logits, 1)
    got_t, got_l = model.decode(enc, n, forced=hf_tokens[:, None, :].int().cuda(), return_logits=True, prompt=p.cuda())
    d = (got_l.cpu()[:, 0] - hf_logits).abs()
    assert d.max().item() < 0.25 and d.mean().item() < 0.03
    top2 = hf_logits.topk(2, -1).values
    safe = (top2[..., 0] - top2[..., 1]) > 0.5
    assert safe.any() and torch.equal(got_t.cpu()[:, 0][safe], hf_tokens[safe].int())
    model.close()


def test_per_row_subtask_prompts_equal_each_subtask_decoded_alone():
    tm = TaskManager("singing_drum_v1")
    m = _model(SMALL, max_batch=6)
    a = O.synthetic_audio(6, SMALL, seed=21).cuda()
    e = m.encode(m.logmel(a))
    subs = ["default", "singing-only", "drum-only"]
    alone = {s: m.decode(e, 40, prompt=torch.from_numpy(tm.task_prompt(s, 6))) for s in subs}
    assert not torch.equal(alone["default"], alone["drum-only"])
    mixed_prompt = np.concatenate([tm.task_prompt(subs[i % 3], 1) for i in range(6)], 0)
    mixed = m.decode(e, 40, prompt=torch.from_numpy(mixed_prompt))
    for i in range(6):
        assert torch.equal(mixed[i], alone[subs[i % 3]][i]), i
    # (B, P) is repeated over the channels; (P,) over every row
    assert torch.equal(m.decode(e, 40, prompt=torch.from_numpy(mixed_prompt[:, 0])), mixed)
    assert torch.equal(m.decode(e, 40, prompt=torch.from_numpy(tm.task_prompt("drum-only", 1)[0, 0])), alone["drum-only"])
    m.close()


def test_eos_in_the_prompt_does_not_finish_a_row_and_early_stop_counts_emitted_steps():
    base = _model(SMALL, max_batch=3)
    a = O.synthetic_audio(3, SMALL, seed=2).cuda()
    e = base.encode(base.logmel(a))
    N, P = 48, 2
    # a prompt made of the EOS id (1): with EOS on, the rows still emit their stream
    eos_cfg = SMALL.with_(eos_id=1)
    p_eos = torch.full((3, 1, P), 1, dtype=torch.int32)
    free = base.decode(e, N, prompt=p_eos).cpu()
    base.close()
    m = _model(eos_cfg, max_batch=3)
    got = m.decode(e, N, prompt=p_eos).cpu()
    for b in range(3):
        row, ref = got[b, 0].tolist(), free[b, 0].tolist()
        first = ref.index(1) if 1 in ref else N
        assert row[:first + 1] == ref[:first + 1] and all(t == SMALL.pad_id for t in row[first + 1:]), b
        assert first > 0 and row[0] != SMALL.pad_id
    m.close()
    # early stop with a prompt: same ids as without, and fewer steps launched once every row has emitted EOS
    p = torch.tensor([599, 598], dtype=torch.int32)
    base = _model(SMALL, max_batch=3)
    fr = base.decode(e, N, prompt=p).cpu()
    base.close()
    common = set(fr[0, 0, :12].tolist()) & set(fr[1, 0, :12].tolist()) & set(fr[2, 0, :12].tolist())
    assert common, "no id common to the three streams' starts"
    eos = min(common, key=lambda t: max(fr[b, 0].tolist().index(t) for b in range(3)))
    m = _model(SMALL.with_(eos_id=eos), max_batch=3)
    full = m.decode(e, N, prompt=p).cpu()
    assert m.last_decode_steps == P + N
    m.set_early_stop(4)
    early = m.decode(e, N, prompt=p).cpu()
    assert torch.equal(early, full)
    last = max(int((full[b, 0] == eos).nonzero()[0]) for b in range(3))
    expect = min(N, -(-(last + 1) // 4) * 4)
    assert m.last_decode_steps == P + expect < P + N, (m.last_decode_steps, last)
    m.set_early_stop(0)
    assert torch.equal(m.decode(e, N, prompt=p).cpu(), full) and m.last_decode_steps == P + N
    m.close()


def test_stream_with_task_tokens_through_fewer_slots_equals_lock_step():
    base = _model(SMALL, max_batch=5)
    a = O.synthetic_audio(5, SMALL, seed=31).cuda()
    p = _prompt(5, 1, 2, seed=17)
    fr = base.inference(a, task_tokens=p, max_token_length=48).cpu()
    base.close()
    eos = int(fr[0, 0, 5])                             # rows retire at different times, and some never
    m = _model(SMALL.with_(eos_id=eos), max_batch=5)
    lock = m.inference(a, task_tokens=p, max_token_length=48)
    for slots, interval in ((2, 4), (3, 8), (1, 16)):
        assert torch.equal(m.inference_stream(a, max_token_length=48, slots=slots, interval=interval, task_tokens=p), lock), (slots, interval)
    assert torch.equal(m.inference_stream(a, max_token_length=48, slots=2, task_tokens=p[:, 0]), lock)       # (N, P)
    assert (lock == SMALL.pad_id).any()
    m.close()


def test_prompt_argument_errors_leave_the_handle_usable(monkeypatch):
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    m = _model(SMALL, max_batch=2)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    a = O.synthetic_audio(2, SMALL, seed=1).cuda()
    e = m.encode(m.logmel(a))
    ref = m.decode(e, 16)
    p = torch.full((2, 1, 2), 598, device=m.device, dtype=torch.int32)
    t = torch.empty(2, 1, 64, device=m.device, dtype=torch.int32)
    L = m._lib
    cases = [
        lambda: L.ymt3_decode_prompted(m._handle, _p(e), 2, 63, _p(p), 2, _p(t), None, None, m._stream()),        # P + n_steps > 64
        lambda: L.ymt3_decode_prompted(m._handle, _p(e), 2, 16, _p(p), -1, _p(t), None, None, m._stream()),
        lambda: L.ymt3_decode_prompted(m._handle, _p(e), 2, 16, None, 2, _p(t), None, None, m._stream()),
        lambda: L.ymt3_transcribe_segments_prompted(m._handle, _p(a), 2, 63, _p(p), 2, _p(t), m._stream()),
        lambda: L.ymt3_transcribe_segments_prompted(m._handle, _p(a), 2, 16, None, 2, _p(t), m._stream()),
        lambda: L.ymt3_transcribe_stream_prompted(m._handle, _p(a), 2, 63, _p(p), 2, _p(t), 1, 8, m._stream()),
        lambda: L.ymt3_transcribe_stream_prompted(m._handle, _p(a), 2, 16, _p(p), -3, _p(t), 1, 8, m._stream()),
        lambda: L.ymt3_transcribe_stream_prompted(m._handle, _p(a), 2, 16, None, 1, _p(t), 1, 8, m._stream()),
    ]
    for i, call in enumerate(cases):
        assert call() == 1, (i, L.ymt3_last_error())                   # YMT3_ERR_ARG
        assert torch.equal(m.decode(e, 16), ref), i                    # the next call succeeds
    # the debug start hook does not combine with a prompt
    assert L.ymt3_debug_decode_start(m._handle, 8) == 0
    assert L.ymt3_decode_prompted(m._handle, _p(e), 2, 16, _p(p), 2, _p(t), None, None, m._stream()) == 1
    assert b"ymt3_debug_decode_start" in L.ymt3_last_error()
    assert torch.equal(m.decode(e, 16), ref)
    assert m.decode(e, 62, prompt=p).shape == (2, 1, 62)               # P + n_steps = max_decode_len fits
    # the host side refuses what the C ABI would
    with pytest.raises(ValueError):
        m.decode(e, 63, prompt=p)
    with pytest.raises(ValueError):
        m.decode(e, 16, prompt=torch.tensor([1536]))
    with pytest.raises(ValueError):
        m.decode(e, 16, prompt=torch.zeros(3, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        m.inference(a, task_tokens=torch.zeros(2, 1, 1, 1, dtype=torch.int32), max_token_length=16)
    m.close()


def test_inference_honours_task_tokens_end_to_end(tmp_path):
    from yourmt3_amd.midi import read_midi_notes
    from yourmt3_amd.transcribe import transcribe
    cfg = YMT3Config(segment_samples=8191, max_decode_len=64)
    m = _model(cfg, max_batch=3)
    tm = TaskManager("singing_drum_v1")
    a = O.synthetic_audio(3, cfg, seed=11).cuda()
    p = torch.from_numpy(tm.task_prompt("drum-only", 3))
    got = m.inference(a, task_tokens=p, max_token_length=32)
    assert torch.equal(got, m.decode(m.encode(m.logmel(a)), 32, prompt=p))
    assert not torch.equal(got, m.inference(a, max_token_length=32))
    parts = m.inference_file(2, a[:, None, :], max_token_length=32, task_tokens=p[:, 0])
    assert np.array_equal(np.concatenate(parts, 0), got.cpu().numpy())
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=3 * 8191))[0].numpy()
    path = transcribe(m, audio, task_manager=tm, subtask="drum-only", bsz=2, output_dir=str(tmp_path), max_token_length=32)
    data = open(path, "rb").read()
    assert data[:4] == b"MThd"
    read_midi_notes(data)
    path2 = transcribe(m, audio, task_manager=tm, subtask="drum-only", bsz=2, output_dir=str(tmp_path / "c"), max_token_length=32,
                       continuous=True)
    assert open(path2, "rb").read() == data
    m.close()
