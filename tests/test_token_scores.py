"""Token scores on the GPU (include/ymt3.h, token scores): log_softmax(logits)[fed id] per emitted token, written by the argmax kernel.

  - the scores equal float64 log_softmax of the call's own logits at the fed id, in every decode regime, and the ids are
    bit-identical with and without scores;
  - against the scored oracle (tests/score_oracle.py) over 128 positions, free-running and teacher-forced;
  - EOS then PAD (0.0), early stop (0.0 tail), prompts (nothing written at prompt positions), continuous batching, the
    poisoned ids of an aborted call (NaN scores) and the end-to-end note confidences.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from score_oracle import scored_greedy_decode, scores_from_logits
from test_gpu_parity import _model
from test_task_prompts import REGIMES, _prompt
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config

pytestmark = pytest.mark.gpu

SMALL = YMT3Config(segment_samples=8191, max_decode_len=64, eos_id=-1)
TOL_MAX, TOL_MEAN = 0.06, 6e-3          # test_gpu_parity._check_ids: the logits' tolerance against the oracle


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_own(scores, logits, tokens, cfg, forced=None):
    """scores against float64 log_softmax of the same call's logits at the fed ids"""
    ref = scores_from_logits(logits.cpu(), tokens.cpu(), cfg, None if forced is None else forced.cpu())
    d = (scores.cpu().double() - ref).abs()
    assert bool((d <= 1e-4 + 1e-5 * ref.abs()).all()), float(d.max())


def _eos_of(fr, within=12):
    """an id every row of the (B, 1, N) stream `fr` emits early: as eos_id, every row finishes, at different positions"""
    common = set(fr[0, 0, :within].tolist())
    for b in range(1, fr.shape[0]):
        common &= set(fr[b, 0, :within].tolist())
    assert common, "no id common to the streams' starts"
    return min(common, key=lambda t: max(fr[b, 0].tolist().index(t) for b in range(fr.shape[0])))


def test_scores_equal_log_softmax_of_own_logits():
    m = _model(SMALL, max_batch=3)
    a = O.synthetic_audio(3, SMALL, seed=5).cuda()
    e = m.encode(m.logmel(a))
    N = 48
    t, lg, sc = m.decode(e, N, return_logits=True, return_scores=True)
    assert sc.shape == (3, 1, N) and sc.dtype == torch.float32
    _check_own(sc, lg, t, SMALL)
    assert bool((sc <= 0).all())
    # teacher-forced, with out-of-range ids clamped like the feed
    g = torch.Generator().manual_seed(3)
    f = torch.randint(0, SMALL.vocab, (3, 1, N), generator=g, dtype=torch.int32)
    f[0, 0, 3], f[1, 0, 7] = -4, SMALL.vocab + 9
    tf, lf, sf = m.decode(e, N, forced=f.cuda(), return_logits=True, return_scores=True)
    _check_own(sf, lf, tf, SMALL, forced=f)
    assert torch.equal(m.decode(e, N, forced=f.cuda()), tf)
    m.close()


@pytest.mark.parametrize("name,cfg_kw,env,B", REGIMES, ids=[r[0] for r in REGIMES])
def test_scores_in_every_regime(name, cfg_kw, env, B, monkeypatch):
    cfg = SMALL.with_(**cfg_kw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(cfg, max_batch=B)
    for k in env:
        monkeypatch.delenv(k)
    K = cfg.n_channels
    a = O.synthetic_audio(8, cfg, seed=11)
    a = (a.repeat(-(-B // 8), 1)[:B] * torch.linspace(0.5, 1.0, B)[:, None]).cuda()
    e = m.encode(m.logmel(a))
    N = 24 if cfg.max_decode_len <= 32 else 40
    free, free_l = m.decode(e, N, return_logits=True)
    t, sc = m.decode(e, N, return_scores=True)
    if name == "two_chains":
        assert m.last_decode_chains == 2
    assert torch.equal(t, free)                                         # the score pass never changes an id
    t2, l2, sc2 = m.decode(e, N, return_logits=True, return_scores=True)
    assert torch.equal(t2, free) and torch.equal(l2, free_l) and torch.equal(sc2, sc)
    _check_own(sc, free_l, free, cfg)
    assert bool((sc <= 0).all())
    # teacher-forced
    f = _prompt(B, K, N, seed=2).cuda()
    tf, lf = m.decode(e, N, forced=f, return_logits=True)
    tf2, sf = m.decode(e, N, forced=f, return_scores=True)
    assert torch.equal(tf2, tf)
    _check_own(sf, lf, tf, cfg, forced=f)
    # prompted, the whole path and the stream: ids as without scores
    P = 3
    p = _prompt(B, K, P, seed=5).cuda()
    tp, lp, sp = m.decode(e, N, prompt=p, return_logits=True, return_scores=True)
    assert torch.equal(tp, m.decode(e, N, prompt=p))
    _check_own(sp, lp, tp, cfg)
    nseg = min(B, 4)
    seg = m.inference(a[:nseg], max_token_length=N)
    seg_t, seg_s = m.inference(a[:nseg], max_token_length=N, return_scores=True)
    assert torch.equal(seg_t, seg)
    st_t, st_s = m.inference_stream(a[:nseg], max_token_length=N, slots=2, interval=4, return_scores=True)
    assert torch.equal(st_t, seg)
    assert torch.allclose(st_s, seg_s, rtol=0, atol=1e-5)
    if nseg == B:
        assert torch.equal(seg_s, sc)
    m.close()


def test_scores_match_the_oracle_over_128_positions():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=160, eos_id=-1)
    m = _model(cfg, max_batch=2)
    a = O.synthetic_audio(2, cfg, seed=3)
    _, enc = O.encode(a, m.weights, cfg, True)
    n = 128
    e = enc.bfloat16().cuda()
    # free-running: the GPU's own ids, scored by the oracle teacher-forced with them
    got_t, got_s = m.decode(e, n, return_scores=True)
    _, ref_s, _ = scored_greedy_decode(enc, m.weights, cfg, n, True, forced=got_t.cpu())
    d = (got_s.cpu().double() - ref_s).abs()
    assert d.max().item() < 2 * TOL_MAX and d.mean().item() < 2 * TOL_MEAN, (d.max().item(), d.mean().item())
    # teacher-forced with the oracle's own ids: per position, and the log-likelihood of each row
    feed, _, _ = scored_greedy_decode(enc, m.weights, cfg, n, True)
    _, ref_f, _ = scored_greedy_decode(enc, m.weights, cfg, n, True, forced=feed)
    _, got_f = m.decode(e, n, forced=feed.cuda(), return_scores=True)
    d = (got_f.cpu().double() - ref_f).abs()
    assert d.max().item() < 2 * TOL_MAX and d.mean().item() < 2 * TOL_MEAN, (d.max().item(), d.mean().item())
    ll_got, ll_ref = got_f.cpu().double().sum(-1), ref_f.sum(-1)
    assert bool(((ll_got - ll_ref).abs() <= 2 * TOL_MEAN * n).all()), (ll_got, ll_ref)
    m.close()


def test_eos_pad_scores_zero_and_early_stop_tail():
    base = _model(SMALL, max_batch=3)
    a = O.synthetic_audio(3, SMALL, seed=2).cuda()
    e = base.encode(base.logmel(a))
    N = 48
    eos = _eos_of(base.decode(e, N).cpu())
    base.close()
    cfg = SMALL.with_(eos_id=eos)
    m = _model(cfg, max_batch=3)
    full, full_l = m.decode(e, N, return_logits=True)
    t, sc = m.decode(e, N, return_scores=True)
    assert torch.equal(t, full)
    after = torch.zeros_like(t, dtype=torch.bool)
    for b in range(3):
        first = t[b, 0].tolist().index(eos)
        after[b, 0, first + 1:] = True
    assert after.any()
    assert bool((t[after] == cfg.pad_id).all()) and bool((sc[after] == 0.0).all())
    _check_own(sc, full_l, full, cfg)
    assert bool((sc[~after] <= 0).all())
    # early stop: every column written (a NaN-filled buffer), the ids of the full run and its scores, 0.0 in the tail
    m.set_early_stop(4)
    tok = torch.empty(3, 1, N, device=m.device, dtype=torch.int32)
    es = torch.full((3, 1, N), float("nan"), device=m.device)
    _lib.check(m._lib.ymt3_decode_scored(m._handle, _p(e), 3, N, None, 0, _p(tok), _p(es), None, None, m._stream()))
    assert m.last_decode_steps < N
    assert torch.equal(tok, full) and torch.equal(es, sc)
    assert bool((es[:, :, m.last_decode_steps:] == 0.0).all())
    m.set_early_stop(0)
    m.close()


def test_prompted_scores_write_only_emitted_columns():
    m = _model(SMALL, max_batch=2)
    a = O.synthetic_audio(2, SMALL, seed=7).cuda()
    e = m.encode(m.logmel(a))
    N, P = 40, 3
    p = _prompt(2, 1, P, seed=8).cuda()
    sentinel = -12345.0
    tok = torch.empty(2, 1, N, device=m.device, dtype=torch.int32)
    buf = torch.full((2 * N + 64,), sentinel, device=m.device)          # 64 floats past the (2, 1, N) scores
    _lib.check(m._lib.ymt3_decode_scored(m._handle, _p(e), 2, N, _p(p), P, _p(tok), _p(buf), None, None, m._stream()))
    sc = buf[:2 * N].view(2, 1, N)
    assert bool((buf[2 * N:] == sentinel).all())
    assert bool((sc != sentinel).all()) and bool((sc <= 0).all())
    assert torch.equal(tok, m.decode(e, N, prompt=p))
    # the unprompted run over P + N steps, teacher-forced with [prompt, emitted ids], scores the same ids from the same logits
    _, sf = m.decode(e, P + N, forced=torch.cat([p, tok], -1), return_scores=True)
    assert torch.equal(sf[..., P:], sc)
    # the whole path and the stream, prompted
    seg_t, seg_s = m.inference(a, task_tokens=p, max_token_length=N, return_scores=True)
    assert torch.equal(seg_t, tok) and torch.equal(seg_s, sc)
    st = torch.empty(2, 1, N, device=m.device, dtype=torch.int32)
    sbuf = torch.full((2 * N + 64,), sentinel, device=m.device)
    _lib.check(m._lib.ymt3_transcribe_stream_scored(m._handle, _p(a), 2, N, _p(p), P, _p(st), _p(sbuf), 1, 8, m._stream()))
    assert bool((sbuf[2 * N:] == sentinel).all()) and torch.equal(st, tok)
    assert torch.allclose(sbuf[:2 * N].view(2, 1, N), sc, rtol=0, atol=1e-5)
    m.close()


def test_stream_scores_through_fewer_slots_equal_lock_step():
    base = _model(SMALL, max_batch=5)
    a = O.synthetic_audio(5, SMALL, seed=31).cuda()
    fr = base.inference(a, max_token_length=48).cpu()
    base.close()
    eos = int(fr[0, 0, 5])                             # rows retire at different times, and some never
    cfg = SMALL.with_(eos_id=eos)
    m = _model(cfg, max_batch=5)
    lock_t, lock_s = m.inference(a, max_token_length=48, return_scores=True)
    assert (lock_t == cfg.pad_id).any()
    for slots, interval in ((2, 4), (3, 8), (1, 16)):
        tok = torch.empty(5, 1, 48, device=m.device, dtype=torch.int32)
        sc = torch.full((5, 1, 48), float("nan"), device=m.device)       # the retired tails are written too
        _lib.check(m._lib.ymt3_transcribe_stream_scored(m._handle, _p(a), 5, 48, None, 0, _p(tok), _p(sc), slots, interval, m._stream()))
        assert torch.equal(tok, lock_t), (slots, interval)
        assert torch.allclose(sc, lock_s, rtol=0, atol=1e-5), (slots, interval)
        assert bool((sc[tok == cfg.pad_id] == 0.0).all())
    m.close()


def test_aborted_call_scores_are_nan(monkeypatch):
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    m = _model(SMALL)
    m.fallback_expected = True
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    a = O.synthetic_audio(2, SMALL).cuda()
    ok_t, ok_s = m.inference(a, max_token_length=8, return_scores=True)
    assert int(ok_t.min()) >= 0 and bool(torch.isfinite(ok_s).all())
    m.set_abort_recovery(0)
    _lib.check(m._lib.ymt3_debug_force_stage_abort(m._handle))
    bad_t, bad_s = m.inference(a, max_token_length=8, return_scores=True)
    assert bool((bad_t == torch.iinfo(torch.int32).min).all()) and bool(torch.isnan(bad_s).all())
    t, s = m.inference(a, max_token_length=8, return_scores=True)
    assert torch.equal(t, ok_t) and torch.equal(s, ok_s) and m.merged_fallbacks == 1
    m.close()


def test_transcribe_with_confidence_end_to_end(tmp_path):
    from yourmt3_amd.transcribe import transcribe
    cfg = YMT3Config(segment_samples=8191, max_decode_len=64)
    m = _model(cfg, max_batch=3)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=3 * 8191))[0].numpy()
    kw = dict(bsz=2, max_token_length=48, return_notes=True)
    path, plain = transcribe(m, audio, output_dir=str(tmp_path / "a"), **kw)
    data = open(path, "rb").read()
    for continuous in (False, True):
        p2, notes = transcribe(m, audio, output_dir=str(tmp_path / f"b{continuous}"), confidence=True, continuous=continuous, **kw)
        assert open(p2, "rb").read() == data and notes == plain
        assert notes and all(0.0 < n.confidence <= 1.0 for n in notes), notes
        _, none = transcribe(m, audio, output_dir=str(tmp_path / f"c{continuous}"), min_confidence=1.01, continuous=continuous, **kw)
        assert none == []
    # the confidences are exp(score) of the onset tokens of inference_file's batches
    segs = m.ingest(torch.from_numpy(audio), cfg.sample_rate)
    tb, sb = m.inference_file(2, segs, max_token_length=48, return_scores=True)
    assert all(np.array_equal(x, y) for x, y in zip(tb, m.inference_file(2, segs, max_token_length=48)))
    assert all(s.dtype == np.float32 and s.shape == t.shape for s, t in zip(sb, tb))
    m.close()
