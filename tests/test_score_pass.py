"""Sequence scoring on the GPU (include/ymt3.h): the teacher-forced log-probability of given ids, all positions in one pass.

  - parity with the full-sequence restatement (tests/teacher_oracle.py) at the project's tolerances -- logits max < 0.06, mean < 6e-3
    (test_gpu_parity._check_ids), scores at twice that (test_token_scores.py) --, with the call's own logits, and with the device's own
    sequential decode(forced=..., return_scores=True);
  - sequence lengths at the edges of the 64-key tile and the 128-query block; causality, bit for bit;
  - chunks of whole decoder rows (also through a segment's channels, and in the workspace grown for one long row);
  - prompts, lengths, clamped ids, score(lengths="eos"); 256 and 512 cross-attention keys; 1024 positions (16 key tiles);
  - a decode call before and after, a NaN segment, and every refusal.
"""
import ctypes

import pytest
import torch

from oracle import ymt3_oracle as O
from teacher_oracle import teacher_score
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd.config import FFN_MOE, YMT3Config

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=160, eos_id=-1)          # 64 frames
TOL_MAX, TOL_MEAN = 0.06, 6e-3


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ids(B, K, n, seed, vocab=CFG.vocab):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, vocab, (B, K, n), generator=g, dtype=torch.int32)


def _against_oracle(sc, lg, ref_s, ref_l, tag=""):
    dl = (lg.cpu() - ref_l).abs()
    ds = (sc.cpu().double() - ref_s).abs()
    print(f"{tag} logits max {float(dl.max()):.4f} mean {float(dl.mean()):.5f}; scores max {float(ds.max()):.4f} mean {float(ds.mean()):.5f}")
    assert float(dl.max()) < TOL_MAX and float(dl.mean()) < TOL_MEAN
    assert float(ds.max()) < 2 * TOL_MAX and float(ds.mean()) < 2 * TOL_MEAN


@pytest.fixture(scope="module")
def small():
    """one handle (64 frames, max_batch 2) and one oracle encoder output shared by the tests that need no other shape"""
    m = _model(CFG, max_batch=2)
    _, enc = O.encode(O.synthetic_audio(2, CFG, seed=3), m.weights, CFG, True)
    yield m, enc, enc.bfloat16().cuda()
    m.close()


def test_parity_with_the_oracle_own_logits_and_the_step_loop(small):
    m, enc, e = small
    n = 128
    ids = _ids(2, 1, n, seed=7)
    ref_s, ref_l = teacher_score(enc, m.weights, CFG, ids)
    sc, lg = m.decode_score(e, ids, return_logits=True)
    assert sc.shape == (2, 1, n) and sc.dtype == torch.float32 and lg.shape == (2, 1, n, CFG.vocab)
    _against_oracle(sc, lg, ref_s, ref_l, "pass vs oracle:")
    ll, ref_ll = sc.cpu().double().sum(-1), ref_s.sum(-1)
    assert bool(((ll - ref_ll).abs() < 2 * TOL_MEAN * n).all()), (ll, ref_ll)
    # the scores are float64 log_softmax of the call's own logits at the target (test_token_scores._check_own's bound)
    own = torch.log_softmax(lg.cpu().double(), -1).gather(-1, ids.long()[..., None])[..., 0]
    d = (sc.cpu().double() - own).abs()
    assert bool((d <= 1e-4 + 1e-5 * own.abs()).all()), float(d.max())
    assert torch.equal(m.decode_score(e, ids), sc)                    # with and without the logits
    # the device's own sequential evaluation: two correct orders, not bit-equal
    _, seq = m.decode(e, n, forced=ids.cuda(), return_scores=True)
    ds = (sc - seq).abs()
    print(f"pass vs step loop: scores max {float(ds.max()):.4f} mean {float(ds.mean()):.5f}")
    assert float(ds.max()) < 2 * TOL_MAX and float(ds.mean()) < 2 * TOL_MEAN


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 127, 129, 160])
def test_lengths_at_tile_edges(small, total):
    m, enc, e = small
    ids = _ids(2, 1, total, seed=total)
    ref_s, ref_l = teacher_score(enc, m.weights, CFG, ids)
    sc, lg = m.decode_score(e, ids, return_logits=True)
    _against_oracle(sc, lg, ref_s, ref_l, f"total {total}:")


def test_causality_is_exact(small):
    m, _, e = small
    n = 128
    ids = _ids(2, 1, n, seed=11)
    sc, lg = m.decode_score(e, ids, return_logits=True)
    for c in (0, 31, 63, 64, 100):
        ids2 = ids.clone()
        ids2[:, :, c + 1:] = (ids2[:, :, c + 1:] + 1 + c) % CFG.vocab
        sc2, lg2 = m.decode_score(e, ids2, return_logits=True)
        assert torch.equal(sc2[..., :c + 1], sc[..., :c + 1]), c
        assert torch.equal(lg2[..., :c + 2, :], lg[..., :c + 2, :]), c
        assert not torch.equal(lg2[..., c + 2:, :], lg[..., c + 2:, :]), c


@pytest.mark.parametrize("K,max_batch,total", [(1, 3, 80), (3, 2, 30)], ids=["rows_2_then_1", "boundary_inside_a_segment"])
def test_chunks_of_whole_rows(K, max_batch, total):
    """64 frames x max_batch activation rows: (1, 3, 80) runs chunks of 2 rows then 1, (3, 2, 30) chunks of 4 rows then 2 -- the
    boundary falls between the channels of the second segment.  Every segment scores as it does alone."""
    cfg = CFG.with_(n_channels=K)
    m = _model(cfg, max_batch=max_batch)
    B = max_batch
    e = m.encode(m.logmel(O.synthetic_audio(B, cfg, seed=5).cuda()))
    ids = _ids(B, K, total, seed=2)
    sc, lg = m.decode_score(e, ids, return_logits=True)
    assert bool(torch.isfinite(sc).all()) and bool((sc < 0).all())
    for b in range(B):
        s1, l1 = m.decode_score(e[b:b + 1], ids[b:b + 1], return_logits=True)
        assert torch.equal(s1, sc[b:b + 1]) and torch.equal(l1, lg[b:b + 1]), b
    m.close()


def test_one_long_row_uses_the_grown_workspace():
    """max_batch 1 x 64 frames is fewer activation rows than one decoder row of 160 positions: the buffers are grown at create"""
    m = _model(CFG, max_batch=1)
    _, enc = O.encode(O.synthetic_audio(1, CFG, seed=4), m.weights, CFG, True)
    ids = _ids(1, 1, 160, seed=6)
    ref_s, ref_l = teacher_score(enc, m.weights, CFG, ids)
    sc, lg = m.decode_score(enc.bfloat16().cuda(), ids, return_logits=True)
    _against_oracle(sc, lg, ref_s, ref_l)
    # the encoder still runs in the same (grown) buffers: the whole path equals its two halves
    a = O.synthetic_audio(1, CFG, seed=4).cuda()
    sc2, _ = m.score(a, ids, lengths=None)
    assert torch.equal(sc2, m.decode_score(m.encode(m.logmel(a)), ids)) and bool(torch.isfinite(sc2).all())
    m.close()


def test_prompt_lengths_and_clamped_ids(small):
    m, enc, e = small
    lib, P, n, V = m._lib, 3, 40, CFG.vocab
    ids = _ids(2, 1, n, seed=13)
    prompt = _ids(2, 1, P, seed=14)
    ref_s, ref_l = teacher_score(enc, m.weights, CFG, ids, prompt)
    # poisoned outputs with guard bands: the prompt's positions write nothing, in front of the buffers or anywhere else
    SENT, G = -12345.0, 2 * P
    sbuf = torch.full((G + 2 * n + G,), SENT, device="cuda")
    lbuf = torch.full(((G + 2 * n + G) * V,), SENT, device="cuda")
    sview, lview = sbuf[G:G + 2 * n], lbuf[G * V:(G + 2 * n) * V]
    d_ids, d_pr = ids.cuda(), prompt.cuda()
    _lib.check(lib.ymt3_score_tokens(m._handle, _p(e), 2, n, _p(d_pr), P, _p(d_ids), None, _p(sview), _p(lview), m._stream()))
    torch.cuda.synchronize()
    assert bool((sbuf[:G] == SENT).all()) and bool((sbuf[G + 2 * n:] == SENT).all())
    assert bool((lbuf[:G * V] == SENT).all()) and bool((lbuf[(G + 2 * n) * V:] == SENT).all())
    assert not bool((sview == SENT).any()) and not bool((lview == SENT).any())
    _against_oracle(sview.view(2, 1, n), lview.view(2, 1, n, V), ref_s, ref_l, "prompted:")
    sc_p = m.decode_score(e, ids, prompt=prompt)
    assert torch.equal(sc_p, sview.view(2, 1, n))
    # lengths: exactly 0.0 from the length on, the bits of lengths=None before it; out-of-range lengths are clamped
    for ln in ([[0], [17]], [[n], [1]], [[-3], [n + 50]]):
        got = m.decode_score(e, ids, prompt=prompt, lengths=torch.tensor(ln))
        for b in range(2):
            k = min(max(ln[b][0], 0), n)
            assert torch.equal(got[b, 0, :k], sc_p[b, 0, :k]) and bool((got[b, 0, k:] == 0).all()), (ln, b)
    # ids outside the vocabulary score as the clamped ids, as the forced path does
    bad, clamped = ids.clone(), ids.clone()
    bad[0, 0, 3], bad[1, 0, 7], bad[1, 0, n - 1] = -4, V + 9, V + 9
    clamped[0, 0, 3], clamped[1, 0, 7], clamped[1, 0, n - 1] = 0, V - 1, V - 1
    sb, lb = m.decode_score(e, bad, return_logits=True)
    sc, lc = m.decode_score(e, clamped, return_logits=True)
    assert torch.equal(sb, sc) and torch.equal(lb, lc)
    _, seq = m.decode(e, n, forced=bad.cuda(), return_scores=True)
    assert float((sb - seq).abs().max()) < 2 * TOL_MAX


def test_score_sums_to_the_likelihood_up_to_eos():
    cfg = CFG.with_(eos_id=1)
    m = _model(cfg, max_batch=2)
    a = O.synthetic_audio(2, cfg, seed=8).cuda()
    n = 24
    ids = _ids(2, 1, n, seed=15)
    ids[ids == cfg.eos_id] = 5
    ids[0, 0, 9] = cfg.eos_id
    ids[0, 0, 15] = cfg.eos_id                                        # only the first counts; row 1 has none
    full = m.decode_score(m.encode(m.logmel(a)), ids)
    sc, ll = m.score(a, ids)
    assert ll.dtype == torch.float64 and ll.shape == (2, 1)
    assert torch.equal(sc[0, 0, :10], full[0, 0, :10]) and bool((sc[0, 0, 10:] == 0).all()) and torch.equal(sc[1], full[1])
    assert torch.equal(ll, sc.double().sum(-1))
    assert abs(float(ll[0, 0]) - float(full[0, 0, :10].double().sum())) < 1e-9
    sc_all, ll_all = m.score(a, ids, lengths=None)
    assert torch.equal(sc_all, full)
    sc_t, _ = m.score(a, ids, lengths=torch.tensor([[4], [n]]))
    assert torch.equal(sc_t[0, 0, :4], full[0, 0, :4]) and bool((sc_t[0, 0, 4:] == 0).all())
    m.close()


@pytest.mark.parametrize("samples", [32767, 65535], ids=["256_frames", "512_frames"])
def test_cross_attention_over_256_and_512_frames(samples):
    cfg = YMT3Config(segment_samples=samples, max_decode_len=16, eos_id=-1)
    m = _model(cfg, max_batch=1)
    _, enc = O.encode(O.synthetic_audio(1, cfg, seed=2), m.weights, cfg, True)
    ids = _ids(1, 1, 16, seed=3)
    ref_s, ref_l = teacher_score(enc, m.weights, cfg, ids)
    sc, lg = m.decode_score(enc.bfloat16().cuda(), ids, return_logits=True)
    _against_oracle(sc, lg, ref_s, ref_l, f"{cfg.n_frames} frames:")
    m.close()


def test_one_row_over_1024_positions():
    """the far distance buckets and sixteen key tiles"""
    cfg = CFG.with_(max_decode_len=1024)
    m = _model(cfg, max_batch=1)
    _, enc = O.encode(O.synthetic_audio(1, cfg, seed=3), m.weights, cfg, True)
    ids = _ids(1, 1, 1024, seed=1)
    ref_s, ref_l = teacher_score(enc, m.weights, cfg, ids)
    sc, lg = m.decode_score(enc.bfloat16().cuda(), ids, return_logits=True)
    _against_oracle(sc, lg, ref_s, ref_l, "1024 positions:")
    assert abs(float(sc.double().sum()) - float(ref_s.sum())) < 2 * TOL_MEAN * 1024
    m.close()


def test_decode_is_untouched_and_a_nan_segment_stays_in_its_rows(small):
    m, _, e = small
    n = 48
    ids = _ids(2, 1, n, seed=21)
    t0, l0 = m.decode(e, n, return_logits=True)
    sc, lg = m.decode_score(e, ids, return_logits=True)
    t1, l1 = m.decode(e, n, return_logits=True)
    assert torch.equal(t1, t0) and torch.equal(l1, l0)
    bad = e.clone()
    bad[1, 5, 17] = float("nan")
    sc_n, lg_n = m.decode_score(bad, ids, return_logits=True)
    assert bool(torch.isnan(sc_n[1]).all()) and bool(torch.isnan(lg_n[1]).all())
    assert torch.equal(sc_n[0], sc[0]) and torch.equal(lg_n[0], lg[0])
    sc_c, lg_c = m.decode_score(e, ids, return_logits=True)            # the next call is clean
    assert torch.equal(sc_c, sc) and torch.equal(lg_c, lg)
    t2, l2 = m.decode(e, n, return_logits=True)
    assert torch.equal(t2, t0) and torch.equal(l2, l0)


def test_refusals(small):
    m, _, e = small
    lib, n = m._lib, 8
    ids = _ids(2, 1, n, seed=1).cuda()
    pr = _ids(2, 1, 2, seed=2).cuda()
    sc = torch.empty(2, 1, n, device="cuda")
    L = CFG.max_decode_len

    def call(n_steps=n, prompt=None, P=0, tokens=ids, scores=sc):
        rc = lib.ymt3_score_tokens(m._handle, _p(e), 2, n_steps, _p(prompt), P, _p(tokens), None, _p(scores), None, m._stream())
        return rc, lib.ymt3_last_error().decode()

    ERR_ARG, ERR_UNSUPPORTED = 1, 4
    for kw, word in ((dict(n_steps=0), "n_steps"), (dict(n_steps=-2), "n_steps"), (dict(P=-1), "n_prompt"),
                     (dict(n_steps=L + 1), "max_decode_len"), (dict(n_steps=L - 1, prompt=pr, P=2), "max_decode_len"),
                     (dict(tokens=None), "tokens"), (dict(scores=None), "scores"), (dict(P=2), "null prompt")):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)
    a = O.synthetic_audio(2, CFG, seed=1).cuda()
    rc = lib.ymt3_transcribe_segments_score(m._handle, _p(a), 2, L + 1, None, 0, _p(ids), None, _p(sc), m._stream())
    assert rc == ERR_ARG and "max_decode_len" in lib.ymt3_last_error().decode()
    rc, _ = call()                                                    # the handle is still usable
    assert rc == 0
    assert torch.equal(sc, m.decode_score(e, ids))
    # the MoE decoder FFN is refused, naming the field
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, dec_ffn=FFN_MOE, n_experts=2, n_enc_layers=1, n_dec_layers=1, eos_id=-1)
    moe = _model(cfg, max_batch=1)
    em = moe.encode(moe.logmel(O.synthetic_audio(1, cfg, seed=1).cuda()))
    rc = lib.ymt3_score_tokens(moe._handle, _p(em), 1, n, None, 0, _p(ids), None, _p(sc), None, moe._stream())
    assert rc == ERR_UNSUPPORTED and "dec_ffn" in lib.ymt3_last_error().decode()
    with pytest.raises(_lib.YMT3Error, match="dec_ffn"):
        moe.decode_score(em, ids[:1])
    assert moe.decode(em, 4).shape == (1, 1, 4)                       # and that handle goes on decoding
    moe.close()
