"""Sequence scoring without a GPU: the full-sequence restatement (tests/teacher_oracle.py) pinned to the step oracle, and the C ABI.

The restatement rounds the softmax numerators to bf16 (the MFMA attention's contract), the step oracle keeps them in f32: two
correct evaluation orders of one model.  They must agree within the project's parity tolerances -- logits max < 0.06 and mean <
6e-3 (test_gpu_parity._check_ids), scores at twice that (test_token_scores.py) -- at every position, over one key tile and over
sixteen, with channels and with a prompt.
"""
import os
import re

import torch

from oracle import ymt3_oracle as O
from score_oracle import scored_greedy_decode
from teacher_oracle import teacher_forward, teacher_score, teacher_scores
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config, FFN_MOE
from yourmt3_amd.weights import make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_MAX, TOL_MEAN = 0.06, 6e-3
CFG = YMT3Config(segment_samples=8191, max_decode_len=160, eos_id=-1)


def _pin(cfg, B, n, prompt=None, own_ids=True, seed=3):
    """restatement against scored_greedy_decode(forced=ids): logits and scores at every position"""
    W = make_weights(cfg, seed=1234)
    audio = O.synthetic_audio(B, cfg, seed=seed)
    _, enc = O.encode(audio, W, cfg, True)
    if own_ids and prompt is None:
        ids = O.greedy_decode(enc, W, cfg, n, True)                   # the audio's own greedy ids
    else:
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(0, cfg.vocab, (B, cfg.n_channels, n), generator=g, dtype=torch.int32)
    _, ref_s, ref_l = scored_greedy_decode(enc, W, cfg, n, True, prompt=prompt, forced=ids)
    got_s, got_l = teacher_score(enc, W, cfg, ids, prompt)
    dl = (got_l - ref_l).abs()
    ds = (got_s - ref_s).abs()
    print(f"logits max {float(dl.max()):.4f} mean {float(dl.mean()):.4f}; scores max {float(ds.max()):.4f} mean {float(ds.mean()):.4f}")
    assert got_l.shape == ref_l.shape and got_s.shape == ref_s.shape
    assert float(dl.max()) < TOL_MAX and float(dl.mean()) < TOL_MEAN
    assert float(ds.max()) < 2 * TOL_MAX and float(ds.mean()) < 2 * TOL_MEAN
    return enc, W, ids, got_s, got_l


def test_restatement_matches_the_step_oracle_over_128_positions():
    _pin(CFG, 2, 128)


def test_restatement_matches_the_step_oracle_with_channels():
    _pin(CFG.with_(n_channels=3), 2, 40)


def test_restatement_matches_the_step_oracle_prompted():
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(0, CFG.vocab, (2, 1, 3), generator=g, dtype=torch.int32)
    _pin(CFG, 2, 40, prompt=prompt)


def test_restatement_matches_the_step_oracle_over_1024_positions():
    _pin(CFG.with_(max_decode_len=1024), 1, 1024, own_ids=False)


def test_lengths_and_clamping_in_the_restatement():
    cfg = CFG
    W = make_weights(cfg, seed=1234)
    _, enc = O.encode(O.synthetic_audio(2, cfg, seed=3), W, cfg, True)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg.vocab, (2, 1, 12), generator=g, dtype=torch.int32)
    s, lg = teacher_score(enc, W, cfg, ids)
    ln = torch.tensor([[5], [40]])                                    # the second is clamped to 12
    s2 = teacher_scores(lg, ids, ln)
    assert torch.equal(s2[0, 0, :5], s[0, 0, :5]) and bool((s2[0, 0, 5:] == 0).all()) and torch.equal(s2[1], s[1])
    # causality: a later id never changes an earlier logit
    ids2 = ids.clone()
    ids2[:, :, 7:] = (ids2[:, :, 7:] + 1) % cfg.vocab
    lg2 = teacher_forward(enc, W, cfg, ids2)
    assert torch.equal(lg2[:, :, :8], lg[:, :, :8]) and not torch.equal(lg2[:, :, 8:], lg[:, :, 8:])
    # out-of-range ids are the clamped ids, as feed and as target
    bad, clamped = ids.clone(), ids.clone()
    bad[0, 0, 3], bad[1, 0, 6] = -4, cfg.vocab + 9
    clamped[0, 0, 3], clamped[1, 0, 6] = 0, cfg.vocab - 1
    sb, lb = teacher_score(enc, W, cfg, bad)
    sc, lc = teacher_score(enc, W, cfg, clamped)
    assert torch.equal(sb, sc) and torch.equal(lb, lc)


def test_header_and_symbols_carry_the_scoring_calls():
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    for name in ("ymt3_score_tokens", "ymt3_transcribe_segments_score"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
    assert "#define YMT3_ABI_VERSION 3" in header
    # the MoE limit is stated next to the declaration
    doc = header[header.index("Sequence scoring"):header.index("int ymt3_score_tokens")]
    assert "YMT3_ERR_UNSUPPORTED" in doc and "dec_ffn" in doc and "MoE" in doc
    assert FFN_MOE == 1

