"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the golden fixtures.

Tolerances (the numerics contract of DESIGN.md: bf16 GEMM operands, fp32 accumulate / residual):
  log-mel           abs 1e-3 on natural-log values (fp32 FFT vs pocketfft, sparse vs dense mel sum)
  encoder output    bf16 values of unit RMS: max abs 0.0625 (a few bf16 ulps), mean abs 4e-3
  logits            unit std fp32: max abs 0.06, mean abs 6e-3
  token ids         BIT EXACT wherever the oracle's top-2 logit margin exceeds TAU = 0.03 (a little over 2x the measured
                    max logit error of 0.013: an argmax can only move if the two errors sum to more than the margin);
                    a free-running stream must be identical up to its first sub-TAU step.  Every id check records the
                    fraction of steps it covered and how many sub-TAU steps differed (gpurun_out/r03_parity_report.json);
                    at least MIN_SAFE of the steps must be covered.
"""
import atexit
import json
import os

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.weights import make_weights, bf16_bits_to_f32

pytestmark = pytest.mark.gpu
TAU = 0.03
MIN_SAFE = 0.8
_REPORT = {}
GOLD = os.path.join(os.path.dirname(__file__), "golden")

SMALL = YMT3Config(segment_samples=8191, max_decode_len=64)
FULL = YMT3Config(max_decode_len=128)
MC3 = YMT3Config(segment_samples=8191, max_decode_len=32, n_channels=3)


def _model(cfg, max_batch=4, weights=None, **kw):
    """A model whose close() fails the test if a merged decode kernel gave up waiting and the call was silently re-run through the separate
    launches (include/ymt3.h, ymt3_set_abort_recovery): recovery must never be what makes a parity test pass.  Tests of the recovery
    itself set `fallback_expected`.  `weights`: another weight set than the seeded default (tests/value_regimes.py)."""
    from yourmt3_amd.model import YourMT3
    m = YourMT3(cfg, make_weights(cfg, seed=1234) if weights is None else weights, device=0, max_batch=max_batch, **kw)
    plain_close = m.close

    def close():
        if getattr(m, "_handle", None) and m._handle.value and not getattr(m, "fallback_expected", False):
            n = m.merged_fallbacks
            plain_close()
            assert n == 0, "a merged decode kernel gave up waiting; the ids came from the fallback path"
        else:
            plain_close()
    m.close = close
    return m


@pytest.fixture(scope="module")
def small():
    m = _model(SMALL)
    yield m
    m.close()


@pytest.fixture(scope="module")
def full():
    m = _model(FULL)
    yield m
    m.close()


def _dump_report():
    if _REPORT:
        try:
            os.makedirs("gpurun_out", exist_ok=True)
            with open(os.path.join("gpurun_out", "r03_parity_report.json"), "w") as f:
                json.dump(_REPORT, f, indent=1)
        except OSError:
            pass


atexit.register(_dump_report)


def _check_ids(name, got_t, ref_t, ref_l, got_l=None, tau=TAU, stable=None, tol_max=0.06, tol_mean=6e-3, min_safe=MIN_SAFE, curve=0):
    """Teacher-forced ids against the oracle: equal wherever the oracle's margin >= tau (and `stable`), with the share
    of steps that covers, the number of uncovered steps that differ, and the logits errors, recorded and bounded."""
    got_t, ref_t = got_t.cpu(), ref_t.cpu()
    safe = _margin(ref_l) >= tau
    if stable is not None:
        safe = safe & stable
    rec = {"tau": tau, "steps": int(safe.numel()), "safe_fraction": float(safe.float().mean()),
           "ids_differ_where_safe": int((got_t[safe] != ref_t[safe]).sum()),
           "ids_differ_below_tau": int((got_t[~safe] != ref_t[~safe]).sum())}
    if got_l is not None:
        d = (got_l.cpu() - ref_l).abs()
        rec["logits_max_abs"] = float(d.amax(-1)[stable].max()) if stable is not None else float(d.max())
        rec["logits_mean_abs"] = float(d.mean())
        if curve:
            rec["logits_error_by_position"] = _position_curve(got_l, ref_l, curve)
    _REPORT[name] = rec
    print(name, rec)
    assert rec["safe_fraction"] >= min_safe, rec
    assert rec["ids_differ_where_safe"] == 0, rec
    if got_l is not None:
        assert rec["logits_max_abs"] < tol_max and rec["logits_mean_abs"] < tol_mean, rec
    return rec


def _position_curve(got_l, ref_l, bucket=128):
    """logits error against the decode position: [first position of the bucket, max abs, mean abs] per `bucket` positions"""
    d = (got_l.cpu() - ref_l).abs()                       # (B, K, steps, V)
    out = []
    for t0 in range(0, d.shape[2], bucket):
        blk = d[:, :, t0:t0 + bucket]
        out.append([t0, round(float(blk.max()), 5), round(float(blk.mean()), 6)])
    return out


def _margin(logits):
    t = logits.topk(2, -1).values
    return t[..., 0] - t[..., 1]


def _check_stream_prefix(got, ref, margin):
    """identical up to (not including) the first step whose oracle margin is below TAU"""
    B, K, L = ref.shape
    for b in range(B):
        for k in range(K):
            low = (margin[b, k] < TAU).nonzero().flatten()
            stop = int(low[0]) if low.numel() else L
            assert torch.equal(got[b, k, :stop], ref[b, k, :stop]), (b, k, stop)
            if stop < L and not torch.equal(got[b, k], ref[b, k]):
                first = int((got[b, k] != ref[b, k]).nonzero()[0])
                assert first >= stop


# ----------------------------------------------------------------------------- front-end
def test_logmel_matches_oracle_and_edges(full):
    cfg = FULL
    a = O.synthetic_audio(4, cfg, seed=3)
    a[1] = 0.0                                   # silence -> log floor everywhere
    a[2] = 0.0
    a[2, 5 * cfg.hop] = 1.0                      # impulse
    a[3] = a[3].clamp(-0.01, 0.01)               # quiet
    ref = O.logmel(a, cfg)
    got = full.logmel(a.cuda()).cpu()
    assert got.shape == (4, 256, 128)
    assert (got - ref).abs().max().item() < 1e-3
    assert torch.allclose(got[1], torch.full_like(got[1], float(np.log(cfg.log_floor))))


def test_logmel_3d_input_and_bad_length(small):
    a = O.synthetic_audio(2, SMALL)
    assert torch.equal(small.logmel(a[:, None, :].cuda()), small.logmel(a.cuda()))
    with pytest.raises(ValueError):
        small.logmel(torch.zeros(1, 100).cuda())
    with pytest.raises(ValueError):
        small.logmel(torch.zeros(5, SMALL.segment_samples).cuda())     # > max_batch


# ----------------------------------------------------------------------------- GEMM kernel
@pytest.mark.parametrize("M,N,K", [(200, 256, 512), (128, 128, 64), (1, 128, 128), (300, 512, 2048), (4096, 1536, 512)])
def test_gemm_matches_fp32_matmul(small, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = torch.randn(N, K, generator=g).bfloat16()
    # A = I-like probe with an asymmetric W catches transposed / permuted fragment maps
    if M == 128 and K == 64:
        A = torch.zeros(M, K).bfloat16()
        A[torch.arange(64), torch.arange(64)] = 1
        W = (torch.arange(N)[:, None] * 3 + torch.arange(K)[None, :]).float().remainder(251).bfloat16()
    ref = A.float() @ W.float().T
    got = small.test_gemm(A.cuda(), W.cuda()).cpu()
    assert (got - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item()) * (K ** 0.5)


@pytest.mark.parametrize("M,N,K", [(4224, 1024, 512), (8192, 512, 64), (8192, 512, 128), (4100, 1024, 192), (4096, 1024, 2048), (16384, 2048, 512)])
def test_pipelined_large_m_gemm(small, M, N, K):
    """The 256 x 128 three-stage kernel (taken when its tiles fill >= half the chip): 1, 2, 3, 8 and 32 K-steps, ragged M,
    and a permutation probe (row i of A selects column i % K of W) that exposes any stage / fragment / swizzle mix-up exactly."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = torch.randn(N, K, generator=g).bfloat16()
    ref = A.float() @ W.float().T
    got = small.test_gemm(A.cuda(), W.cuda()).cpu()
    assert (got - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item()) * (K ** 0.5)
    P = torch.zeros(M, K).bfloat16()
    P[torch.arange(M), (torch.arange(M) * 7) % K] = 1
    Wp = (torch.arange(N)[:, None] * 3 + torch.arange(K)[None, :]).float().remainder(251).bfloat16()
    got = small.test_gemm(P.cuda(), Wp.cuda()).cpu()
    assert torch.equal(got, Wp.float()[:, (torch.arange(M) * 7) % K].T.contiguous())
    for _ in range(3):                                       # repeated launches: a stage read before its DMA landed would differ
        assert torch.equal(small.test_gemm(P.cuda(), Wp.cuda()).cpu(), got)


@pytest.mark.parametrize("M,N,K", [(200, 256, 512), (300, 512, 2048), (4224, 1024, 512), (4096, 1024, 2048)])
@pytest.mark.parametrize("kind", ["cancel", "negative", "scale_up", "scale_down", "scale_mixed", "signed_zeros", "subnormal"])
def test_gemm_operand_values(small, kind, M, N, K):
    """The plain and the pipelined large-M kernel on operands that are not randn (tests/value_regimes.py: cancelling pairs of 1e4,
    all-negative, 2^+-60 scales, signed zeros, bf16 subnormals, which MFMA does not flush), against the fp64 product of the bf16
    values at the derived bound of any fp32-accumulated dot product: K 2^-24 sum |a_k| |w_k| per element."""
    from value_regimes import gemm_operands, gemm_reference_and_bound
    A, W = gemm_operands(kind, M, N, K)
    ref, bound = gemm_reference_and_bound(A, W)
    got = small.test_gemm(A.cuda(), W.cuda()).cpu()
    assert bool(torch.isfinite(got).all())
    excess = ((got.double() - ref).abs() / bound)
    print(kind, M, N, K, "max error / bound", float(excess.max()))
    assert float(excess.max()) <= 1.0
    if kind == "subnormal":
        assert float(ref.abs().max()) > 0 and float((got.double() - ref).abs().max()) < 1e-3 * float(ref.abs().max())      # not flushed to 0


# ----------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("which", ["small", "full"])
def test_encoder_matches_oracle(which, request):
    m = request.getfixturevalue(which)
    cfg = m.cfg
    a = O.synthetic_audio(2, cfg)
    mel = O.logmel(a, cfg)
    ref = O.encoder_t5(O.input_projection(mel, m.weights, True), m.weights, cfg, True)
    got = m.encode(mel.cuda()).float().cpu()
    d = (got - ref).abs()
    assert d.max().item() <= 0.0625 and d.mean().item() <= 4e-3


def test_encoder_large_batch_takes_the_pipelined_gemm():
    """16 segments x 256 frames = 4096 rows: the QKV / FFN-in / cross-KV projections run the persistent 256 x 128 kernel with
    its LDS-turned bf16 epilogues (the 512-column projections stay on the 128 x 128 one).  Against the oracle, and bitwise
    against the same segments encoded in batches of 2 (all on the 128 x 128 kernel: same K order, so identical sums)."""
    m = _model(FULL, max_batch=16)
    a = O.synthetic_audio(16, FULL, seed=5)
    mel = O.logmel(a, FULL)
    got = m.encode(mel.cuda())
    ref = O.encoder_t5(O.input_projection(mel[:3], m.weights, True), m.weights, FULL, True)
    err = (got[:3].float().cpu() - ref).abs()
    assert err.max().item() <= 0.0625 and err.mean().item() <= 4e-3
    for i in range(0, 16, 2):
        assert torch.equal(m.encode(mel[i:i + 2].cuda()), got[i:i + 2])
    # cross-K/V (head-major epilogue) + decode: batch of 16 == batches of 2, bit for bit
    t16 = m.decode(got, 8)
    for i in range(0, 16, 2):
        assert torch.equal(m.decode(got[i:i + 2], 8), t16[i:i + 2])
    m.close()


# ----------------------------------------------------------------------------- decoder
def test_decode_teacher_forced_logits_and_argmax(small):
    cfg = SMALL
    a = O.synthetic_audio(2, cfg)
    _, enc = O.encode(a, small.weights, cfg, True)
    n = 48
    ref_t, ref_l = O.greedy_decode(enc, small.weights, cfg, n, True, return_logits=True)
    got_t, got_l = small.decode(enc.bfloat16().cuda(), n, forced=ref_t.cuda(), return_logits=True)
    _check_ids("small_teacher_forced", got_t, ref_t, ref_l, got_l)


def test_decode_free_running_prefix_and_determinism(small):
    cfg = SMALL
    a = O.synthetic_audio(2, cfg)
    _, enc = O.encode(a, small.weights, cfg, True)
    n = 48
    ref_t, ref_l = O.greedy_decode(enc, small.weights, cfg, n, True, return_logits=True)
    e = enc.bfloat16().cuda()
    got = small.decode(e, n).cpu()
    _check_stream_prefix(got, ref_t, _margin(ref_l))
    assert torch.equal(got, small.decode(e, n).cpu())          # bitwise reproducible run to run


def test_graph_replay_equals_eager_launches(small):
    cfg = SMALL
    a = O.synthetic_audio(2, cfg)
    e = small.encode(small.logmel(a.cuda()))
    t_graph = small.decode(e, 40).cpu()
    os.environ["YMT3_NO_GRAPH"] = "1"
    try:
        eager = _model(cfg)
    finally:
        del os.environ["YMT3_NO_GRAPH"]
    t_eager = eager.decode(e, 40).cpu()
    eager.close()
    assert torch.equal(t_graph, t_eager)


def test_eos_then_pad_fill():
    cfg = SMALL
    a = O.synthetic_audio(2, cfg)
    base = _model(cfg.with_(eos_id=-1))
    e = base.encode(base.logmel(a.cuda()))
    free = base.decode(e, 16).cpu()
    base.close()
    eos = int(free[0, 0, 4])
    m = _model(cfg.with_(eos_id=eos))
    got = m.decode(e, 16).cpu()
    m.close()
    for b in range(2):
        row, ref = got[b, 0].tolist(), free[b, 0].tolist()
        if eos in ref:
            first = ref.index(eos)
            assert row[:first + 1] == ref[:first + 1]
            assert all(t == cfg.pad_id for t in row[first + 1:])
        else:
            assert row == ref
    assert got[0, 0, 5:].eq(cfg.pad_id).all()


def test_early_stop_produces_the_same_tokens_and_stops_launching(small):
    cfg = SMALL
    a = O.synthetic_audio(3, cfg, seed=2)
    base = _model(cfg.with_(eos_id=-1))
    e = base.encode(base.logmel(a.cuda()))
    free = base.decode(e, 64).cpu()
    base.close()
    eos = int(free[0, 0, 3])                                # every row sees this id early in its stream?  make sure
    m = _model(cfg.with_(eos_id=eos))
    full = m.decode(e, 64).cpu()
    m.set_early_stop(4)
    early = m.decode(e, 64).cpu()
    assert torch.equal(early, full)
    # steps launched = the first multiple of the check interval at which every row has emitted EOS (never timing)
    last = max((full[b, 0] == eos).nonzero()[0].item() if (full[b, 0] == eos).any() else 64 for b in range(3))
    expect = min(64, -(-(last + 1) // 4) * 4)
    assert m.last_decode_steps == expect, (m.last_decode_steps, expect, last)
    m.set_early_stop(0)
    assert torch.equal(m.decode(e, 64).cpu(), full)
    assert m.last_decode_steps == 64
    m.close()


def test_rows_are_independent_of_batch_composition(small):
    cfg = SMALL
    a = O.synthetic_audio(4, cfg, seed=7).cuda()
    all4 = small.inference(a, max_token_length=24).cpu()
    for i in (0, 3):
        alone = small.inference(a[i:i + 1], max_token_length=24).cpu()
        assert torch.equal(alone[0], all4[i])
    assert small.inference(a[:0], max_token_length=8).shape == (0, 1, 8)          # empty batch


def test_inference_is_the_composition_of_the_stages(small):
    a = O.synthetic_audio(3, SMALL, seed=11).cuda()
    e2e = small.inference(a, max_token_length=32)
    staged = small.decode(small.encode(small.logmel(a)), 32)
    assert torch.equal(e2e, staged)
    parts = small.inference_file(2, a[:, None, :], max_token_length=32)
    assert [p.shape[0] for p in parts] == [2, 1]
    assert np.array_equal(np.concatenate(parts, 0), e2e.cpu().numpy())


def test_multichannel_rows_share_the_segment_encoder():
    cfg = MC3
    m = _model(cfg)
    a = O.synthetic_audio(2, cfg)
    _, enc = O.encode(a, m.weights, cfg, True)
    n = 24
    ref_t, ref_l = O.greedy_decode(enc, m.weights, cfg, n, True, return_logits=True)
    got_t, got_l = m.decode(enc.bfloat16().cuda(), n, forced=ref_t.cuda(), return_logits=True)
    m.close()
    assert got_t.shape == (2, 3, n)
    _check_ids("mc3_teacher_forced", got_t, ref_t, ref_l, got_l)
    assert not torch.equal(ref_t[:, 0], ref_t[:, 1])             # channels really differ


def test_multichannel_beyond_128_rows():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_channels=13)
    m = _model(cfg, max_batch=12)                      # 156 rows = 10 row tiles of 16
    a = O.synthetic_audio(12, cfg)
    _, enc = O.encode(a, m.weights, cfg, True)
    ref_t, ref_l = O.greedy_decode(enc, m.weights, cfg, 6, True, return_logits=True)
    got_t, got_l = m.decode(enc.bfloat16().cuda(), 6, forced=ref_t.cuda(), return_logits=True)
    m.close()
    _check_ids("mc13_156_rows", got_t, ref_t, ref_l, got_l)


def test_mid_tile_decode_gemms_match_oracle_at_520_rows():
    """From 512 rows on the decode GEMMs take the mid-size tile kernel (one MFMA chain over K instead of the 8-way split):
    40 segments x 13 channels = 520 rows, teacher-forced against the oracle with the usual tolerances; and the same rows in a
    batch of 48 segments (624 rows, same kernels) give the same bits."""
    cfg = YMT3Config(segment_samples=16383, max_decode_len=8, n_channels=13)        # 128 frames
    m = _model(cfg, max_batch=48)
    a = O.synthetic_audio(48, cfg, seed=4)
    _, enc = O.encode(a[:40], m.weights, cfg, True)
    n = 5
    ref_t, ref_l = O.greedy_decode(enc, m.weights, cfg, n, True, return_logits=True)
    e = enc.bfloat16().cuda()
    got_t, got_l = m.decode(e, n, forced=ref_t.cuda(), return_logits=True)
    _check_ids("mid_tile_520_rows", got_t, ref_t, ref_l, got_l)
    e48 = torch.cat([e, m.encode(m.logmel(a[40:].cuda()))], 0)
    assert torch.equal(m.decode(e48, n)[:40], m.decode(e, n))
    m.close()


@pytest.mark.parametrize("K", [13, 3, 16])
def test_multichannel_shared_kv_cross_attention(K):
    """n_frames in {128, 256, 512} routes the multi-channel cross-attention to the one-workgroup-per-(segment, head)
    MFMA kernel (mc_cross_attn.hip); same oracle, same tolerances as the per-row kernel."""
    cfg = YMT3Config(segment_samples=16383, max_decode_len=16, n_channels=K)        # 128 frames
    m = _model(cfg, max_batch=3)
    a = O.synthetic_audio(3, cfg)
    _, enc = O.encode(a, m.weights, cfg, True)
    n = 10
    ref_t, ref_l = O.greedy_decode(enc, m.weights, cfg, n, True, return_logits=True)
    got_t, got_l = m.decode(enc.bfloat16().cuda(), n, forced=ref_t.cuda(), return_logits=True)
    m.close()
    _check_ids(f"mc_shared_kv_K{K}", got_t, ref_t, ref_l, got_l)


def test_512_frame_segments():
    cfg = YMT3Config(segment_samples=65535, max_decode_len=16)
    m = _model(cfg, max_batch=2)
    a = O.synthetic_audio(2, cfg)
    mel_ref, enc_ref = O.encode(a, m.weights, cfg, True)
    mel = m.logmel(a.cuda())
    assert mel.shape == (2, 512, 128) and (mel.cpu() - mel_ref).abs().max().item() < 1e-3
    assert (m.encode(mel).float().cpu() - enc_ref).abs().max().item() <= 0.0625
    # decode with 512 cross-attention keys: the cross-attention loop beyond its first 256-key block
    n = 16
    ref_t, ref_l = O.greedy_decode(enc_ref, m.weights, cfg, n, True, return_logits=True)
    got_t, got_l = m.decode(enc_ref.bfloat16().cuda(), n, forced=ref_t.cuda(), return_logits=True)
    _check_ids("t512_teacher_forced", got_t, ref_t, ref_l, got_l)
    _check_stream_prefix(m.decode(enc_ref.bfloat16().cuda(), n).cpu(), ref_t, _margin(ref_l))
    m.close()


def test_transcribe_writes_a_midi_file(small, tmp_path):
    from yourmt3_amd.midi import read_midi_notes
    from yourmt3_amd.transcribe import transcribe
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=3 * 8191))[0].numpy()      # 3 segments of the small config
    path, notes = transcribe(small, audio, bsz=2, output_dir=str(tmp_path), max_token_length=32, return_notes=True)
    data = open(path, "rb").read()
    assert data[:4] == b"MThd"
    back = read_midi_notes(data)                           # random weights: any notes, but a well-formed file
    assert len(back) <= len(notes) and (len(back) > 0) == (len(notes) > 0)    # the writer merges same-pitch overlaps
    path2, notes2 = transcribe(small, audio, bsz=2, output_dir=str(tmp_path / "c"), max_token_length=32, return_notes=True, continuous=True)
    assert open(path2, "rb").read() == data               # continuous batching: same ids, same file



# ----------------------------------------------------------------------------- the whole decode length (round 3)
# Until round 3 no test compared the HIP decoder with the oracle beyond position 127.  The self-attention kernel walks the keys in
# blocks of 8 waves x 8 key groups x 6 = 384: its unmasked FULL-block path and its second loop iteration first run at position 383, and
# the relative-position bucket saturates from distance 128 on.  These tests run configs[1]'s shapes over all 1024 positions.
_LONG = {}


def _long_reference():
    """configs[1] shapes (256 frames), 2 segments x 1024 steps, EOS fill off: oracle ids + logits, computed once per session"""
    if not _LONG:
        cfg = YMT3Config(max_decode_len=1024, eos_id=-1)
        W = make_weights(cfg, seed=1234)
        _, enc = O.encode(O.synthetic_audio(2, cfg, seed=0), W, cfg, True)
        ref_t, ref_l = O.greedy_decode(enc, W, cfg, 1024, True, return_logits=True)
        _LONG.update(cfg=cfg, W=W, enc=enc, ref_t=ref_t, ref_l=ref_l)
    return _LONG


@pytest.mark.parametrize("variant,env", [
    ("merged", {}),                                                        # attention pair + GEMM chain (the 64-row regime's kernels)
    ("separate", {"YMT3_NO_ATTN_PAIR": "1", "YMT3_NO_GEMM_CHAIN": "1"}),   # dec_attn_kernel<SELF, OP> + fused cross-attention + four GEMM launches
    ("unfolded", {"YMT3_NO_FOLD_O": "1"}),                                 # dec_attn_kernel<SELF> without the folded O-projection (the form beyond 96 rows)
])
def test_decode_matches_oracle_over_all_1024_positions(variant, env, monkeypatch):
    """Teacher-forced on the oracle's stream: logits at EVERY one of the 1024 positions within the usual tolerance, ids equal wherever
    the oracle's margin >= TAU.  Then the HIP path free-running over 1024 steps, checked by teacher-forcing the ORACLE on the HIP
    stream: every id the HIP path emitted is the oracle's argmax given the same prefix, wherever the oracle's margin >= TAU -- a
    check of the free-running stream at every position, not only up to the first near-tie."""
    L = _long_reference()
    cfg = L["cfg"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(cfg, max_batch=2)
    for k in env:
        monkeypatch.delenv(k)
    e = L["enc"].bfloat16().cuda()
    got_t, got_l = m.decode(e, 1024, forced=L["ref_t"].cuda(), return_logits=True)
    rec = _check_ids(f"full_length_1024_{variant}", got_t, L["ref_t"], L["ref_l"], got_l, curve=128)
    assert rec["steps"] == 2048
    late = (got_l.cpu()[:, :, 383:] - L["ref_l"][:, :, 383:]).abs()
    assert late.max().item() < 0.06 and late.mean().item() < 6e-3
    free = m.decode(e, 1024).cpu()
    _check_stream_prefix(free, L["ref_t"], _margin(L["ref_l"]))
    if "free" in L and torch.equal(free, L["free"]):
        rec2 = dict(L["free_rec"], same_ids_as="the first variant run in this session, bit for bit")      # (the variants compute the same bits)
    else:
        ora_t, ora_l = O.greedy_decode(L["enc"], L["W"], cfg, 1024, True, forced=free, return_logits=True)
        safe = _margin(ora_l) >= TAU
        rec2 = {"tau": TAU, "steps": int(safe.numel()), "safe_fraction": float(safe.float().mean()),
                "ids_differ_where_safe": int((free[safe] != ora_t[safe]).sum()), "ids_differ_below_tau": int((free[~safe] != ora_t[~safe]).sum()),
                "first_sub_tau_step": [int((~safe[b, 0]).nonzero()[0]) if (~safe[b, 0]).any() else 1024 for b in range(2)]}
        if "free" not in L:
            L["free"], L["free_rec"] = free, rec2
    _REPORT[f"full_length_1024_{variant}_free_running_vs_oracle_on_the_same_prefix"] = rec2
    assert rec2["safe_fraction"] >= MIN_SAFE and rec2["ids_differ_where_safe"] == 0, rec2
    assert bool((free[:, :, 512:] != free[:, :, 512:513]).any())           # still a varied stream late in the decode
    m.close()


def test_full_length_golden_fixture():
    """tests/golden/full_t256_l1024.npz (tests/scripts/make_golden.py): ids and margins of all 1024 positions, logits at
    t = 0, 127, 382, 383, 384, 767, 1023; encoder output from full_t256.npz."""
    z = np.load(os.path.join(GOLD, "full_t256_l1024.npz"))
    base = np.load(os.path.join(GOLD, str(z["enc_from"]) + ".npz"))
    cfg = YMT3Config(max_decode_len=1024, eos_id=-1)
    m = _model(cfg, max_batch=2)
    enc = bf16_bits_to_f32(base["enc_bf16"]).view(2, cfg.n_frames, cfg.d_model).bfloat16().cuda()
    ref_t, margin = torch.from_numpy(z["tokens"]), torch.from_numpy(z["margin"])
    got_t, got_l = m.decode(enc, 1024, forced=ref_t.cuda(), return_logits=True)
    steps = z["logit_steps"].tolist()
    err = (got_l.cpu()[:, :, steps, :] - torch.from_numpy(z["logits"])).abs().amax(-1)           # (2, 1, len(steps))
    safe = margin >= TAU
    _REPORT["golden_full_t256_l1024"] = {"tau": TAU, "steps": 2048, "safe_fraction": float(safe.float().mean()), "logit_steps": steps,
                                         "logits_max_abs_at_those_steps": [round(float(v), 5) for v in err.amax((0, 1))],
                                         "ids_differ_below_tau": int((got_t.cpu()[~safe] != ref_t[~safe]).sum())}
    assert err.max().item() < 0.06
    assert safe.float().mean().item() >= MIN_SAFE and torch.equal(got_t.cpu()[safe], ref_t[safe])
    m.close()


def test_many_row_kernels_match_oracle_over_256_positions(monkeypatch):
    """configs[3]'s kernels -- the 2-waves-per-(row, head) self-attention (taken beyond 2048 (row, head) pairs), the mid-size tile decode
    GEMMs (from 512 rows on) and the shared-K/V multi-channel cross-attention -- had met the oracle at positions <= 4 only.  Two create-time
    knobs select them at a row count the CPU oracle decodes in seconds: 2 segments x 13 channels = 26 rows over all 256 positions of
    configs[3]'s decode length (the 2-wave kernel walks 96 keys per iteration: three iterations, its FULL-block path from position 95 on)."""
    cfg = YMT3Config(segment_samples=16383, max_decode_len=256, n_channels=13, eos_id=-1)          # 128 frames
    monkeypatch.setenv("YMT3_SELF_ATTN_2WAVE", "1")
    monkeypatch.setenv("YMT3_DEC_GEMM_MID_ROWS", "1")
    m = _model(cfg, max_batch=2)
    monkeypatch.delenv("YMT3_SELF_ATTN_2WAVE")
    monkeypatch.delenv("YMT3_DEC_GEMM_MID_ROWS")
    plain = _model(cfg, max_batch=2)                                       # the few-row kernels, for comparison
    a = O.synthetic_audio(2, cfg, seed=6)
    _, enc = O.encode(a, m.weights, cfg, True)
    ref_t, ref_l = O.greedy_decode(enc, m.weights, cfg, 256, True, return_logits=True)
    e = enc.bfloat16().cuda()
    got_t, got_l = m.decode(e, 256, forced=ref_t.cuda(), return_logits=True)
    _check_ids("many_row_kernels_26_rows_256_steps", got_t, ref_t, ref_l, got_l, curve=64)
    prof = m.profile_decode(e, 8, stride=4)
    assert prof["attn_pair"]["launches"] == 0 and prof["gemm_chain"]["launches"] == 0 and prof["self_attn"]["launches"] == 2 * cfg.n_dec_layers
    p_t, p_l = plain.decode(e, 256, forced=ref_t.cuda(), return_logits=True)
    _check_ids("few_row_kernels_26_rows_256_steps", p_t, ref_t, ref_l, p_l, curve=64)
    assert (p_l - got_l).abs().max().item() < 0.06 and not torch.equal(p_l, got_l)                  # other kernels, other summation order
    free = m.decode(e, 256).cpu()
    ora_t, ora_l = O.greedy_decode(enc, m.weights, cfg, 256, True, forced=free, return_logits=True)
    safe = _margin(ora_l) >= TAU
    assert safe.float().mean().item() >= MIN_SAFE and torch.equal(free[safe], ora_t[safe])
    m.close(); plain.close()


def test_unfit_merged_kernel_takes_the_separate_launches(small, monkeypatch):
    """ymt3_create enables a merged kernel only if its switch is on AND the occupancy query says its whole grid is resident at once.
    A device partition on which only ONE of the two fits (forced here through YMT3_TEST_CHAIN_UNFIT / YMT3_TEST_PAIR_UNFIT) must run
    the separate launches for the other one -- with the environment switches unset, which is where round 2 overwrote the decision."""
    a = O.synthetic_audio(3, SMALL, seed=12).cuda()
    e = small.encode(small.logmel(a))
    ref_t, ref_l = small.decode(e, 40, return_logits=True)
    for var, gone, kept, sep in (("YMT3_TEST_CHAIN_UNFIT", "gemm_chain", "attn_pair", "cross_o_gemm"),
                                 ("YMT3_TEST_PAIR_UNFIT", "attn_pair", "gemm_chain", "self_attn"),
                                 ("YMT3_TEST_STEP_UNFIT", "step_layers", "attn_pair", "gemm_chain")):      # (the per-step kernel needs both of the others)
        monkeypatch.setenv(var, "1")
        monkeypatch.setenv("YMT3_STEP_KERNEL", "1")           # asked for, and still not taken where a kernel it needs does not fit
        m = _model(SMALL)
        monkeypatch.delenv(var)
        monkeypatch.delenv("YMT3_STEP_KERNEL")
        prof = m.profile_decode(e, 16, stride=8)
        assert prof[gone]["launches"] == 0 and prof["step_layers"]["launches"] == 0 and prof[kept]["launches"] > 0 and prof[sep]["launches"] > 0, (var, prof)
        t, l = m.decode(e, 40, return_logits=True)
        assert torch.equal(t, ref_t) and torch.equal(l, ref_l), var
        assert m.merged_fallbacks == 0
        m.close()


def _moe_case(cfg, n, tol_max, tol_mean, tau, max_deficit, monkeypatch, min_safe=0.7, segments=4, enc=None, m=None, feed=None,
              name=None, out=None):
    """Teacher-forced MoE decode vs the oracle at EVERY step.  Routing is discrete: where the 2nd and 3rd router logits are closer than
    the numerical noise, the HIP path may legitimately pick another expert than the oracle, which moves that step's logits by ~0.2.
    Rounds 1-2 excluded such (row, step) pairs by a router-gap threshold (and so covered 52 % of the fp8 steps).  Now the router's
    choices are recorded (debug hook ymt3_debug_moe_trace) and fed to the ORACLE: each choice must lie within `max_deficit` of the
    oracle's own top-2 cut (a legitimate near-tie), and then logits and ids are compared at every step, with the usual argmax margin.
    By default `segments` synthetic segments go through the oracle encoder, a handle of that many rows is created and both sides are fed
    the oracle's own stream.  Any row count instead (tests/test_row_space.py): `enc` ((B, T, d_model) fp32, host) is the encoder output
    both sides decode, `m` a handle created under YMT3_DEBUG_HOOKS=1 with max_batch >= B, `feed` ((B, 1, n) ids) what both sides are fed;
    `name` names the report entry, and `out` (a dict) receives the recorded choices (steps, layers, rows, 2), ids, logits and chains."""
    if m is None:
        monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
        m = _model(cfg, max_batch=segments)
        monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    if enc is None:
        a = O.synthetic_audio(segments, cfg)
        _, enc = O.encode(a, m.weights, cfg, True)
    if feed is None:
        feed = O.greedy_decode(enc, m.weights, cfg, n, True)                 # the oracle's own stream (its own routing): the tokens both sides are fed
    feed = feed.cpu()
    rows = enc.shape[0] * cfg.n_channels
    trace = m.moe_trace(n)
    e = enc.bfloat16().cuda()
    got_t, got_l = m.decode(e, n, forced=feed.cuda(), return_logits=True)
    chains = m.last_decode_chains
    sel = trace.cpu()[:, :, :rows]                                           # (steps, layers, rows, 2)
    assert int(sel.min()) >= 0 and int(sel.max()) < cfg.n_experts and bool((sel[..., 0] != sel[..., 1]).all())
    O.MOE_FORCED_SEL = iter([sel[t, l] for t in range(n) for l in range(cfg.n_dec_layers)])
    O.MOE_FORCED_DEFICIT = []
    try:
        ref_t, ref_l = O.greedy_decode(enc, m.weights, cfg, n, True, forced=feed, return_logits=True)
        deficit = torch.stack(O.MOE_FORCED_DEFICIT)                          # (steps * layers, rows)
    finally:
        O.MOE_FORCED_SEL = None
        O.MOE_FORCED_DEFICIT = None
    name = name or f"moe_fp8{cfg.moe_fp8}_{n}_steps_routing_teacher_forced"
    rec = _check_ids(name, got_t, ref_t, ref_l, got_l, tau=tau, tol_max=tol_max, tol_mean=tol_mean, min_safe=min_safe, curve=32)
    rec["router_choices"] = int(deficit.numel())
    rec["router_choices_outside_the_oracle_top2"] = int((deficit > 0).sum())
    rec["max_router_deficit"] = float(deficit.max())
    assert rec["max_router_deficit"] <= max_deficit, rec                   # every differing choice was a near-tie
    assert torch.equal(m.decode(e, n), m.decode(e, n))        # routing + grouped GEMM are reproducible
    _lib_check = m._lib.ymt3_debug_moe_trace(m._handle, None, 0, 0)
    assert _lib_check == 0
    if out is not None:
        out.update(trace=sel, got_t=got_t.cpu(), got_l=got_l.cpu(), chains=chains, rec=rec)
    return m


def test_moe_decoder_ffn_matches_oracle(monkeypatch):
    """a11 (build-defined spec, parity unpinned w.r.t. the reference): router -> top-2 -> expert FFNs -> gated sum; 144 positions."""
    from yourmt3_amd.config import FFN_MOE
    cfg = YMT3Config(segment_samples=8191, max_decode_len=160, dec_ffn=FFN_MOE, eos_id=-1)
    m = _moe_case(cfg, 144, 0.06, 6e-3, TAU, 0.01, monkeypatch, min_safe=MIN_SAFE)
    assert "dec.0.router" in m.weights and m.weights["dec.0.wi"].shape == (8 * 2048, 512)
    m.close()


def test_moe_fp8_expert_gemms_match_oracle(monkeypatch):
    """BASELINE configs[4]: expert GEMMs on OCP e4m3 MFMA (per-expert weight scale, per-row activation scale); 144 positions.
    Tolerances above the bf16 ones: an fp8 rounding step is 16 bf16 steps, so the same ~1e-3 relative disagreement between two
    implementations moves an fp8 operand 16x as far when it flips a rounding (logits max 0.08, mean 8e-3; measured 0.036 / 5.9e-3),
    and TAU = 0.08 stays a little over twice the measured maximum."""
    from yourmt3_amd.config import FFN_MOE
    cfg = YMT3Config(segment_samples=8191, max_decode_len=160, dec_ffn=FFN_MOE, moe_fp8=1, eos_id=-1)
    m = _moe_case(cfg, 144, 0.08, 8e-3, 0.08, 0.04, monkeypatch)
    assert m.weights["dec.0.wi_q8"].dtype == torch.uint8 and "dec.0.wi" not in m.weights
    m.close()


@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_moe_chain_is_bit_identical_to_the_five_launches(fp8, monkeypatch):
    """Round 3: an MoE layer's cross O-projection -> router -> expert FFN-in -> expert FFN-out -> next QKV projection (or lm_head, combine folded
    in) run as ONE launch (moe_chain.hip) whose stages hand row tiles / expert pair sets over through arrival counters and agent-scope
    loads / stores.  Same arithmetic as the five launches (YMT3_NO_MOE_CHAIN=1), operation for operation: logits and ids must not move by
    one bit, for one row, ragged and full row tiles, lock-step and slot mode; the router's recorded choices are the same too."""
    from yourmt3_amd.config import FFN_MOE
    cfg = YMT3Config(segment_samples=8191, max_decode_len=64, dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    monkeypatch.setenv("YMT3_NO_MOE_CHAIN", "1")
    old = _model(cfg, max_batch=64)
    monkeypatch.delenv("YMT3_NO_MOE_CHAIN")
    new = _model(cfg, max_batch=64)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    a1 = O.synthetic_audio(2, cfg).cuda()
    e1 = new.encode(new.logmel(a1))
    assert new.profile_decode(e1, 8, stride=4)["gemm_chain"]["launches"] == 2 * cfg.n_dec_layers and new.profile_decode(e1, 8, stride=4)["ffn_wi_gemm"]["launches"] == 0
    assert old.profile_decode(e1, 8, stride=4)["gemm_chain"]["launches"] == 0 and old.profile_decode(e1, 8, stride=4)["ffn_wi_gemm"]["launches"] > 0
    tr_new, tr_old = new.moe_trace(48), old.moe_trace(48)
    for B, n in ((1, 48), (5, 48), (21, 32), (40, 24), (64, 48)):
        a = O.synthetic_audio(B, cfg, seed=40 + B).cuda()
        e = new.encode(new.logmel(a))
        t_new, l_new = new.decode(e, n, return_logits=True)
        t_old, l_old = old.decode(e, n, return_logits=True)
        assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old), (B, n)
        assert torch.equal(tr_new[:n, :, :B], tr_old[:n, :, :B]) and int(tr_new[:n, :, :B].min()) >= 0, (B, n)
        assert int(t_new.min()) >= 0 and torch.equal(new.decode(e, n), t_new)
    a = O.synthetic_audio(9, cfg, seed=77).cuda()
    assert torch.equal(new.inference_stream(a, slots=5, interval=4), old.inference_stream(a, slots=5, interval=4))
    assert torch.equal(new.inference_stream(a, slots=9, interval=8), old.inference(a))
    new.close()
    old.close()


@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_moe_chain_is_bit_identical_to_the_five_launches_under_one_sided_routing(fp8, monkeypatch):
    """The test above meets balanced routing only.  Here every layer's eight router rows are identical, so every logit of a row is the same
    fp32 value (experts 0..7 share one summation order) and every row picks experts (0, 1) with gates 0.5: at B = 64 two experts hold 64
    pairs each (four full chunks) and six hold none; B = 33 leaves a ragged chunk, B = 1 one pair each.  Ids, logits and the recorded
    choices must equal the five launches' bit for bit (tests/test_moe_kernels.py pins those launches to their contracts)."""
    from yourmt3_amd.config import FFN_MOE
    cfg = YMT3Config(segment_samples=8191, max_decode_len=64, dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
    W = make_weights(cfg, seed=1234)
    for k in [k for k in W if k.endswith(".router")]:
        W[k] = W[k][:1].expand_as(W[k]).contiguous()
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    monkeypatch.setenv("YMT3_NO_MOE_CHAIN", "1")
    old = _model(cfg, max_batch=64, weights=W)
    monkeypatch.delenv("YMT3_NO_MOE_CHAIN")
    new = _model(cfg, max_batch=64, weights=W)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    n = 16
    tr_new, tr_old = new.moe_trace(n), old.moe_trace(n)
    e1 = new.encode(new.logmel(O.synthetic_audio(2, cfg).cuda()))
    assert new.profile_decode(e1, 8, stride=4)["ffn_wi_gemm"]["launches"] == 0 and old.profile_decode(e1, 8, stride=4)["ffn_wi_gemm"]["launches"] > 0
    want = torch.tensor([0, 1], dtype=torch.int32, device=tr_new.device)
    for B in (1, 33, 64):
        a = O.synthetic_audio(B, cfg, seed=50 + B).cuda()
        e = new.encode(new.logmel(a))
        t_new, l_new = new.decode(e, n, return_logits=True)
        t_old, l_old = old.decode(e, n, return_logits=True)
        assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old), B
        assert torch.equal(tr_new[:n, :, :B], tr_old[:n, :, :B]), B
        assert bool((tr_new[:n, :, :B] == want).all()) and bool((tr_old[:n, :, :B] == want).all()), B
    new.close()
    old.close()


def _full_size_properties(cfg, B, seed, probe, probe_len=1):
    """Size-independent properties of one BASELINE config at its full size (far beyond what the CPU oracle checks in
    seconds): shape / id range, bitwise reproducibility, independence of a segment from the rest of the batch,
    idempotence under teacher forcing with the model's own output, and a stream that has not collapsed.
    `probe_len`: segments per independence probe.  Rows are independent inside every kernel, but two kernels have a
    many-row form with another summation order -- the self-attention (2 waves per (row, head) beyond 2048 pairs) and the
    decode GEMMs (mid-size tiles from 512 rows) -- so a probe must stay on the same side of those boundaries as the full
    batch to be comparable bit for bit."""
    m = _model(cfg, max_batch=B)
    a = O.synthetic_audio(B, cfg, seed=seed).cuda()
    L = cfg.max_decode_len
    t1 = m.inference(a)
    assert t1.shape == (B, cfg.n_channels, L) and t1.dtype == torch.int32
    assert int(t1.min()) >= 0 and int(t1.max()) < cfg.vocab
    assert torch.equal(t1, m.inference(a))                                   # bitwise reproducible
    for i in probe:                                                          # alone (or in a small batch) == inside the batch
        assert torch.equal(m.inference(a[i:i + probe_len]), t1[i:i + probe_len]), i
    enc = m.encode(m.logmel(a))
    forced = m.decode(enc, L, forced=t1)                                     # feeding back its own stream changes nothing
    assert torch.equal(forced, t1)
    assert len(torch.unique(t1)) > 200                                       # not a collapsed stream
    return m, a, t1


def test_moe_combine_folded_into_the_next_norm_gemm(monkeypatch):
    """Round 2: h += y0 + y1 after the expert GEMMs is no longer a launch; the next layer's QKV projection (or lm_head) forms
    h + (y0 + y1) while loading, takes sum(x^2) itself and stores the row for the rest of its layer.  Same arithmetic except the
    order of that sum of squares: against the kept-launch path (YMT3_MOE_COMBINE_LAUNCH=1, the round-1 sums) logits agree to 1e-2
    and ids wherever the margin allows; both paths are checked against the oracle by the tests above / the digests."""
    from yourmt3_amd.config import FFN_MOE
    for fp8 in (0, 1):
        cfg = YMT3Config(segment_samples=8191, max_decode_len=48, dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
        new = _model(cfg, max_batch=4)
        monkeypatch.setenv("YMT3_MOE_COMBINE_LAUNCH", "1")
        old = _model(cfg, max_batch=4)
        monkeypatch.delenv("YMT3_MOE_COMBINE_LAUNCH")
        a = O.synthetic_audio(4, cfg, seed=17).cuda()
        e = new.encode(new.logmel(a))
        t_old, l_old = old.decode(e, 48, return_logits=True)
        t_new, l_new = new.decode(e, 48, forced=t_old, return_logits=True)
        d = (l_new - l_old).abs().amax(-1).cpu()                # (B, 1, steps)
        # a flipped expert choice at a router near-tie moves a row's logits AND what that row caches for later steps, so rows are
        # compared up to their first large difference; flips are rare, so those prefixes must cover most of the steps
        big = d > 0.02
        first = torch.where(big.any(-1), big.float().argmax(-1), torch.full(big.shape[:-1], big.shape[-1]))
        prefix = torch.arange(big.shape[-1])[None, None, :] < first[..., None]
        assert prefix.float().mean().item() > 0.6, float(prefix.float().mean())
        assert d[prefix].max().item() < 0.02
        safe = (_margin(l_old.cpu()) >= TAU) & prefix
        assert torch.equal(t_new.cpu()[safe], t_old.cpu()[safe])
        assert torch.equal(new.decode(e, 48), new.decode(e, 48))             # reproducible
        assert torch.equal(new.inference_stream(a, slots=3, interval=4), new.inference(a))    # slot mode alternates the buffers too
        old.close(); new.close()


def test_full_size_properties_baseline_config_1():
    """BASELINE configs[1] at full size (64 segments, 256 frames, 1024 tokens), plus the EOS->PAD invariant and continuous
    batching at full size."""
    from yourmt3_amd.config import baseline_config
    cfg = baseline_config(1)
    m, a, t1 = _full_size_properties(cfg, 64, 21, (0, 37, 63))
    m.close()
    eos = int(t1[5, 0, 100])
    m2 = _model(cfg.with_(eos_id=eos), max_batch=64)
    t2 = m2.inference(a).cpu()
    # continuous batching at full size: 64 segments through 24 slots (ragged refills), and through all 64 -- same ids
    assert torch.equal(m2.inference_stream(a, slots=24, interval=16).cpu(), t2)
    assert torch.equal(m2.inference_stream(a, slots=64, interval=32).cpu(), t2)
    m2.close()
    t1c = t1.cpu()
    for b in range(64):
        row = t2[b, 0]
        hit = (row == eos).nonzero().flatten()
        if hit.numel():
            f = int(hit[0])
            assert torch.equal(row[:f + 1], t1c[b, 0, :f + 1]) and bool((row[f + 1:] == cfg.pad_id).all())
        else:
            assert torch.equal(row, t1c[b, 0])
    assert bool((t2[5, 0, 101:] == cfg.pad_id).all())


def test_full_size_properties_baseline_config_2():
    """BASELINE configs[2]: Perceiver-TF encoder + T5 decoder, 256 segments x 1024 tokens."""
    from yourmt3_amd.config import baseline_config
    m, _, _ = _full_size_properties(baseline_config(2), 256, 22, (0, 129, 255))
    m.close()


def test_full_size_properties_baseline_config_3():
    """BASELINE configs[3]: 13-channel decoder, 64 segments x 13 channels = 832 rows, 256 tokens per channel."""
    from yourmt3_amd.config import baseline_config
    m, _, t = _full_size_properties(baseline_config(3), 64, 23, (0, 11, 24), probe_len=40)     # 40 x 13 = 520 rows: same kernels as 832
    assert not torch.equal(t[:, 0], t[:, 1])                                 # channels decode different streams
    m.close()


def test_full_size_properties_baseline_config_4():
    """BASELINE configs[4]: MoE decoder FFN (8 experts, top-2, fp8 expert GEMMs), 64 segments x 1024 tokens."""
    from yourmt3_amd.config import baseline_config
    m, _, _ = _full_size_properties(baseline_config(4), 64, 24, (0, 30, 63))
    m.close()


def test_ids_bit_identical_to_round_1():
    """The decode kernels were restructured in round 2 (fewer dependent launches per step) under the constraint that
    every sum keeps its round-1 order: free-running greedy ids over hundreds of steps move with the last bit of a logit, so
    their digests (tests/golden/r01_id_hashes.json, written by the round-1 kernels: tests/scripts/gpu_id_hashes.py) pin it."""
    import hashlib
    import importlib.util
    path = os.path.join(os.path.dirname(__file__), "scripts", "gpu_id_hashes.py")
    spec = importlib.util.spec_from_file_location("gpu_id_hashes", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref = json.load(open(os.path.join(GOLD, "r01_id_hashes.json")))
    assert set(ref) <= set(mod.CASES)
    bad = []
    for name in ref:
        cfg, B, L, seed = mod.CASES[name]
        if mod.digest(cfg, B, L, seed, mod.ENV.get(name)) != ref[name]:
            bad.append(name)
    assert not bad, bad


def test_perceiver_tf_encoder_matches_oracle():
    """a9 (build-defined spec, parity unpinned w.r.t. the reference: oracle/perceiver_oracle.py): (B, T, F', C) spectral tokens,
    per block a spectral cross-attention from n_latents << F' latents per frame, a latent transformer and a temporal
    transformer, (B, T, n_latents, D) -> (B, T, d_model); decoder unchanged.  Two latent counts, neither tied to the 64 frames."""
    from yourmt3_amd.config import ENC_PERCEIVER_TF
    from yourmt3_amd._lib import YMT3Error
    for n_lat, blocks in ((32, 3), (64, 1)):
        cfg = YMT3Config(segment_samples=8191, max_decode_len=32, encoder_type=ENC_PERCEIVER_TF, n_latents=n_lat, n_enc_layers=0, ptf_blocks=blocks)
        m = _model(cfg, max_batch=4)
        a = O.synthetic_audio(3, cfg)
        mel_ref, enc_ref = O.encode(a, m.weights, cfg, True)
        assert enc_ref.shape == (3, cfg.n_frames, cfg.d_model)
        enc = m.encode(m.logmel(a.cuda()))
        d = (enc.float().cpu() - enc_ref).abs()
        # How far may two correct bf16 implementations of THIS model differ?  The oracle evaluated a second time with every sum in
        # double (same rounding points, oracle/perceiver_oracle.py::in_double) differs from its fp32 self by mean 3.7e-3 / max 0.031
        # for 3 blocks of 32 latents, 2.0e-3 / 0.016 for one block (the T5 encoder: 1.6e-3): 18 narrow (d = 128) sub-layers amplify
        # a last-bit difference in a sum to about one final bf16 rounding in every second output value.  The HIP path is held to
        # 1.25 x that intrinsic figure (measured: 1.01 x), and to the absolute cap of the T5 encoder's test on the maximum.
        from oracle.perceiver_oracle import encoder_perceiver_tf, in_double
        intrinsic = (encoder_perceiver_tf(mel_ref.double(), in_double(m.weights), cfg, True).float() - enc_ref).abs()
        _REPORT[f"perceiver_tf_enc_K{n_lat}"] = {"enc_max_abs": float(d.max()), "enc_mean_abs": float(d.mean()),
                                                 "oracle_fp32_vs_fp64_sums_max_abs": float(intrinsic.max()), "oracle_fp32_vs_fp64_sums_mean_abs": float(intrinsic.mean())}
        assert d.max().item() <= 0.0625 and d.mean().item() <= 1.25 * intrinsic.mean().item() + 1e-4, (n_lat, d.max().item(), d.mean().item(), intrinsic.mean().item())
        assert torch.equal(m.encode(m.logmel(a[1:2].cuda()))[0], enc[1])          # a segment alone == inside the batch
        if n_lat == 32:
            t5cfg = cfg.with_(encoder_type=0, n_enc_layers=6)
            n = 16
            ref_t, ref_l = O.greedy_decode(enc_ref, m.weights, cfg, n, True, return_logits=True)
            got_t, got_l = m.decode(enc_ref.bfloat16().cuda(), n, forced=ref_t.cuda(), return_logits=True)
            _check_ids("perceiver_tf_teacher_forced", got_t, ref_t, ref_l, got_l)
            e2e = m.inference(a.cuda(), max_token_length=8)
            assert torch.equal(e2e, m.decode(enc, 8))
            assert t5cfg.n_frames == cfg.n_frames
        m.close()
    with pytest.raises(YMT3Error):
        _model(cfg.with_(n_latents=24))                              # latents per frame: 32 or 64
    with pytest.raises(YMT3Error):
        _model(cfg.with_(ptf_d=96))


def test_automatic_two_chains_at_many_rows_give_the_single_chain_ids():
    """168-256 rows of one channel decode as two concurrent chains by default (runtime.hip: auto_chains -- 626 against 690 ms per batch of 256,
    profiles/r03_chains_many_rows.txt); YMT3_CHAINS=1 keeps one.  Both run the same kernels on every row, so the ids are bit-identical."""
    cfg = SMALL
    B = 224
    a = O.synthetic_audio(8, cfg, seed=11)
    a = a.repeat(B // 8, 1) * torch.linspace(0.5, 1.0, B)[:, None]     # 224 different segments from 8
    m_auto = _model(cfg, max_batch=B)
    os.environ["YMT3_CHAINS"] = "1"
    try:
        m_one = _model(cfg, max_batch=B)
    finally:
        del os.environ["YMT3_CHAINS"]
    e = m_one.encode(m_one.logmel(a.cuda()))
    t_one = m_one.decode(e, 48).cpu()
    t_auto = m_auto.decode(e, 48).cpu()
    assert torch.equal(t_auto, t_one)
    assert m_auto.last_decode_chains == 2 and m_one.last_decode_chains == 1
    assert len({tuple(r.flatten().tolist()) for r in t_one}) > 8                  # (the rows are not copies of each other)
    # teacher forcing with logits returned goes through the same two chains: same logits, bit for bit
    f_one, l_one = m_one.decode(e, 24, forced=t_one[..., :24].contiguous().cuda(), return_logits=True)
    f_auto, l_auto = m_auto.decode(e, 24, forced=t_one[..., :24].contiguous().cuda(), return_logits=True)
    assert m_auto.last_decode_chains == 2
    assert torch.equal(f_auto.cpu(), f_one.cpu()) and torch.equal(l_auto.cpu(), l_one.cpu())
    m_one.close(); m_auto.close()


def test_two_concurrent_chains_and_unfused_query_path_give_identical_tokens(small):
    """YMT3_CHAINS / YMT3_NO_FUSEQ are read at create: rows are independent, so any split must be bit-identical;
    the fused and the separate query projection follow the same rounding points (ids equal where margins allow)."""
    cfg = SMALL
    a = O.synthetic_audio(4, cfg, seed=5).cuda()
    e = small.encode(small.logmel(a))
    ref = small.decode(e, 40).cpu()
    os.environ["YMT3_CHAINS"] = "2"
    try:
        m2 = _model(cfg)
    finally:
        del os.environ["YMT3_CHAINS"]
    assert torch.equal(m2.decode(e, 40).cpu(), ref)
    m2.close()
    os.environ["YMT3_NO_FUSEQ"] = "1"
    try:
        m3 = _model(cfg)
    finally:
        del os.environ["YMT3_NO_FUSEQ"]
    t3, l3 = m3.decode(e, 40, forced=ref.cuda(), return_logits=True)
    t1, l1 = small.decode(e, 40, forced=ref.cuda(), return_logits=True)
    m3.close()
    assert (l3 - l1).abs().max().item() < 0.02
    safe = _margin(l1.cpu()) >= TAU
    assert torch.equal(t3.cpu()[safe], t1.cpu()[safe])


def test_folded_o_projection_is_bit_identical_to_the_separate_launch(small, monkeypatch):
    """Round 2: the self-attention kernel ends with its head's O-projection partial (the DG_RESID kernel's wave-h split-K
    partial, same MFMAs) and the consumers sum the eight partials in wave order: logits and ids must not move by one bit
    against YMT3_NO_FOLD_O=1 (the round-1 sequence with the separate O-projection launch)."""
    monkeypatch.setenv("YMT3_NO_FOLD_O", "1")
    old = _model(SMALL)
    monkeypatch.delenv("YMT3_NO_FOLD_O")
    a = O.synthetic_audio(4, SMALL, seed=9).cuda()
    e = small.encode(small.logmel(a))
    t_new, l_new = small.decode(e, 64, return_logits=True)
    t_old, l_old = old.decode(e, 64, return_logits=True)
    assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old)
    assert torch.equal(small.inference_stream(a, slots=3, interval=5), old.inference_stream(a, slots=3, interval=5))
    old.close()


def test_gemm_chain_is_bit_identical_to_the_four_launches(small, monkeypatch):
    """Round 2: cross O-projection -> FFN-in -> FFN-out -> next QKV projection (or lm_head) run as ONE launch whose stages hand
    16-row tiles to each other through arrival counters and agent-scope loads / stores (dec_chain.hip).  Same K-slices, MFMA chains
    and reduction orders as dec_gemm_kernel: logits and ids must not move by one bit against YMT3_NO_GEMM_CHAIN=1, for full and
    ragged row tiles, lock-step and slot mode."""
    monkeypatch.setenv("YMT3_NO_GEMM_CHAIN", "1")
    old = _model(SMALL, max_batch=40)
    monkeypatch.delenv("YMT3_NO_GEMM_CHAIN")
    new = _model(SMALL, max_batch=40)
    for B in (1, 4, 21, 40):
        a = O.synthetic_audio(B, SMALL, seed=30 + B).cuda()
        e = new.encode(new.logmel(a))
        t_new, l_new = new.decode(e, 48, return_logits=True)
        t_old, l_old = old.decode(e, 48, return_logits=True)
        assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old), B
        assert int(t_new.min()) >= 0
    a = O.synthetic_audio(9, SMALL, seed=77).cuda()
    assert torch.equal(new.inference_stream(a, slots=5, interval=4), old.inference_stream(a, slots=5, interval=4))
    new.close()
    old.close()


def test_attention_pair_is_bit_identical_to_the_two_launches(monkeypatch):
    """Round 2: a layer's self-attention (with its folded O-projection) and fused cross-attention run as ONE launch; the row's eight
    heads hand their partials over through a per-row arrival counter and agent-scope stores / loads.  Logits and ids must not move
    by one bit against YMT3_NO_ATTN_PAIR=1, at ragged and full row counts, short and long positions, lock-step and slot mode."""
    cfg = YMT3Config(segment_samples=8191, max_decode_len=160)
    monkeypatch.setenv("YMT3_NO_ATTN_PAIR", "1")
    old = _model(cfg, max_batch=64)
    monkeypatch.delenv("YMT3_NO_ATTN_PAIR")
    new = _model(cfg, max_batch=64)
    for B, n in ((1, 160), (5, 160), (37, 40), (64, 150)):
        a = O.synthetic_audio(B, cfg, seed=50 + B).cuda()
        e = new.encode(new.logmel(a))
        t_new, l_new = new.decode(e, n, return_logits=True)
        t_old, l_old = old.decode(e, n, return_logits=True)
        assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old), (B, n)
        assert int(t_new.min()) >= 0
    a = O.synthetic_audio(11, cfg, seed=78).cuda()
    assert torch.equal(new.inference_stream(a, slots=6, interval=4, max_token_length=48), old.inference_stream(a, slots=6, interval=4, max_token_length=48))
    new.close()
    old.close()


def test_step_kernel_is_bit_identical_to_the_per_layer_launches(monkeypatch):
    """Round 3, an OPTION (YMT3_STEP_KERNEL=1; measured slower than the default, profiles/r03_step_kernel.md): a step's six attention pairs and
    six GEMM chains as ONE launch (dec_step.hip): the attention -> chain and QKV -> attention boundaries are arrival counters + agent-scope
    data.  Same arithmetic as the 14-launch step: logits and ids must not move by one bit, at full and ragged row tiles, one row, short
    and long positions (the 384-key block boundary included), row tiles in step and as independent pipelines, lock-step and slot mode."""
    cfg = YMT3Config(segment_samples=8191, max_decode_len=448)
    old = _model(cfg, max_batch=64)
    monkeypatch.setenv("YMT3_STEP_KERNEL", "1")
    new = _model(cfg, max_batch=64)
    monkeypatch.setenv("YMT3_STEP_TILES_FREE", "1")
    free = _model(cfg, max_batch=64)
    monkeypatch.delenv("YMT3_STEP_TILES_FREE")
    monkeypatch.delenv("YMT3_STEP_KERNEL")
    assert new.profile_decode(old.encode(old.logmel(O.synthetic_audio(1, cfg).cuda())), 8, stride=4)["step_layers"]["launches"] == 2
    for B, n in ((1, 448), (5, 100), (16, 40), (17, 40), (37, 40), (64, 448)):
        a = O.synthetic_audio(B, cfg, seed=60 + B).cuda()
        e = new.encode(new.logmel(a))
        t_new, l_new = new.decode(e, n, return_logits=True)
        t_old, l_old = old.decode(e, n, return_logits=True)
        assert torch.equal(t_new, t_old) and torch.equal(l_new, l_old), (B, n)
        assert int(t_new.min()) >= 0 and new.merged_fallbacks == 0
        assert torch.equal(new.decode(e, n), t_new)
        assert torch.equal(free.decode(e, n), t_old) and free.merged_fallbacks == 0
    a = O.synthetic_audio(11, cfg, seed=79).cuda()
    assert torch.equal(new.inference_stream(a, slots=6, interval=4, max_token_length=48), old.inference_stream(a, slots=6, interval=4, max_token_length=48))
    assert torch.equal(new.inference_stream(a, slots=11, interval=16, max_token_length=64), old.inference(a, max_token_length=64))
    assert torch.equal(free.inference_stream(a, slots=6, interval=4, max_token_length=48), old.inference_stream(a, slots=6, interval=4, max_token_length=48))
    new.close()
    free.close()
    old.close()


def test_profile_hooks(small, monkeypatch):
    e = small.encode(small.logmel(O.synthetic_audio(2, SMALL).cuda()))
    prof = small.profile_decode(e, 32, stride=8)
    # a layer's self- and cross-attention are one launch (dec_attn_pair_kernel)
    assert prof["attn_pair"]["launches"] == 4 * SMALL.n_dec_layers and prof["attn_pair"]["ms_total"] > 0 and prof["self_attn"]["launches"] == 0
    # the last layer's GEMM-chain launch ends with lm_head (dec_chain.hip): one chain launch per layer, no lm_head launch of its own
    assert prof["gemm_chain"]["launches"] == 4 * SMALL.n_dec_layers and prof["lm_head_gemm"]["launches"] == 0 and prof["step_layers"]["launches"] == 0
    assert prof["qkv_cache_gemm"]["launches"] == 4 and prof["ffn_wi_gemm"]["launches"] == 0
    assert prof["unsampled_span"]["launches"] == 3
    monkeypatch.setenv("YMT3_STEP_KERNEL", "1")
    m = _model(SMALL)
    monkeypatch.delenv("YMT3_STEP_KERNEL")
    prof = m.profile_decode(e, 32, stride=8)
    # the option: a step as three launches -- layer 0's QKV projection, all six layers (dec_step_kernel, lm_head included), argmax + embedding
    assert prof["step_layers"]["launches"] == 4 and prof["step_layers"]["ms_total"] > 0
    assert prof["qkv_cache_gemm"]["launches"] == 4 and prof["argmax_embed"]["launches"] == 4
    for gone in ("attn_pair", "gemm_chain", "self_attn", "lm_head_gemm", "ffn_wi_gemm"):
        assert prof[gone]["launches"] == 0, gone
    m.close()


def test_decode_start_debug_hook_is_gated_and_one_shot(small, monkeypatch):
    """ymt3_debug_decode_start (late cache positions for short counter passes) is not product surface: a normal handle
    refuses it; under YMT3_DEBUG_HOOKS=1 it applies to ONE decode call, which reads zero-filled positions below step0."""
    from yourmt3_amd import _lib
    e = small.encode(small.logmel(O.synthetic_audio(2, SMALL).cuda()))
    ref = small.decode(e, 16).cpu()
    assert small._lib.ymt3_debug_decode_start(small._handle, 8) == 4                       # YMT3_ERR_UNSUPPORTED
    assert torch.equal(small.decode(e, 16).cpu(), ref)
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    m = _model(SMALL)
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    _lib.check(m._lib.ymt3_debug_decode_start(m._handle, 8))
    with pytest.raises(_lib.YMT3Error):
        m.decode(e, SMALL.max_decode_len)                      # 8 + 64 > max_decode_len; the hook is consumed by this call
    assert torch.equal(m.decode(e, 16).cpu(), ref)             # back to position 0 without being told
    _lib.check(m._lib.ymt3_debug_decode_start(m._handle, 8))
    late = m.decode(e, 16)                                     # runs from position 8 over zero keys; ids are not meaningful
    assert late.shape == (2, 1, 16) and torch.equal(m.decode(e, 16).cpu(), ref)
    _lib.check(m._lib.ymt3_debug_decode_start(m._handle, 8))
    assert torch.equal(m.decode(e, 16), late)                  # defined memory below step0: reproducible
    _lib.check(m._lib.ymt3_debug_decode_start(m._handle, 8))
    with pytest.raises(_lib.YMT3Error):
        m.inference_stream(O.synthetic_audio(2, SMALL).cuda(), max_token_length=8)
    m.close()


def test_a_stage_abort_is_recovered_through_the_separate_launches(small, monkeypatch):
    """The merged decode kernels bound every spin (1 s) behind a sticky abort word.  What an abort must trigger, checked through the
    gated debug hook that raises the word for the next decode call: that call still returns the CORRECT ids -- it is run again through
    the separate launches, which compute the same bits -- the handle stays on them (no merged launch afterwards), goes on working, and
    ymt3_merged_fallbacks reports it.  Lock-step and continuous-batching calls alike."""
    from yourmt3_amd import _lib
    assert small._lib.ymt3_debug_force_stage_abort(small._handle) == 4                    # YMT3_ERR_UNSUPPORTED on a normal handle
    a = O.synthetic_audio(3, SMALL, seed=2).cuda()
    ref = small.inference(a, max_token_length=24)
    e = small.encode(small.logmel(a))
    ref_t, ref_l = small.decode(e, 24, return_logits=True)
    assert torch.equal(ref_t, ref) and small.merged_fallbacks == 0
    for mode in ("lockstep", "stream"):
        monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
        m = _model(SMALL)
        m.fallback_expected = True
        monkeypatch.delenv("YMT3_DEBUG_HOOKS")
        assert torch.equal(m.inference(a, max_token_length=24), ref) and m.merged_fallbacks == 0
        assert m.profile_decode(e, 8, stride=4)["attn_pair"]["launches"] > 0
        _lib.check(m._lib.ymt3_debug_force_stage_abort(m._handle))
        got = m.inference(a, max_token_length=24) if mode == "lockstep" else m.inference_stream(a, max_token_length=24, slots=2, interval=4)
        assert torch.equal(got, ref), mode                        # the aborted call itself returns the right ids
        assert m.merged_fallbacks == 1
        prof = m.profile_decode(e, 8, stride=4)                   # ... and the handle now runs the separate launches
        assert prof["step_layers"]["launches"] == 0 and prof["attn_pair"]["launches"] == 0 and prof["gemm_chain"]["launches"] == 0 and prof["self_attn"]["launches"] > 0
        t, l = m.decode(e, 24, return_logits=True)
        assert torch.equal(t, ref_t) and torch.equal(l, ref_l)
        assert torch.equal(m.inference_stream(a, max_token_length=24, slots=2, interval=4), ref)
        assert m._lib.ymt3_debug_force_stage_abort(m._handle) == 4    # nothing merged left to abort
        assert m.merged_fallbacks == 1
        m.close()


def test_a_stage_abort_without_the_end_of_call_wait(monkeypatch):
    """ymt3_set_abort_recovery(h, 0): decode calls stay fully asynchronous.  An aborted call's ids are all INT32_MIN (never
    plausible ids); the next call on the handle notices, switches to the separate launches and returns correct ids."""
    from yourmt3_amd import _lib
    monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")
    m = _model(SMALL)
    m.fallback_expected = True
    monkeypatch.delenv("YMT3_DEBUG_HOOKS")
    a = O.synthetic_audio(2, SMALL).cuda()
    ok = m.inference(a, max_token_length=8)
    assert int(ok.min()) >= 0
    m.set_abort_recovery(0)
    _lib.check(m._lib.ymt3_debug_force_stage_abort(m._handle))
    bad = m.inference(a, max_token_length=8)
    assert bool((bad == torch.iinfo(torch.int32).min).all()) and m.merged_fallbacks == 0
    assert torch.equal(m.inference(a, max_token_length=8), ok) and m.merged_fallbacks == 1
    assert torch.equal(m.logmel(a), m.logmel(a))
    with pytest.raises(_lib.YMT3Error):
        m.set_abort_recovery(2)
    m.close()


def test_step_stamps_hook(small, monkeypatch):
    from yourmt3_amd._lib import YMT3Error
    with pytest.raises(YMT3Error):
        small.step_stamps()                                   # handle created without YMT3_STAMP: refused, not garbage
    monkeypatch.setenv("YMT3_STAMP", "1")
    m = _model(SMALL)
    monkeypatch.delenv("YMT3_STAMP")
    a = O.synthetic_audio(2, SMALL)
    plain = small.inference(a.cuda(), max_token_length=8)
    assert torch.equal(m.inference(a.cuda(), max_token_length=8), plain)       # stamping changes no result
    rows = m.step_stamps()
    assert len(rows) == 1 + 2 * 6 + 1 and rows[0][0] == "qkv_cache_gemm" and rows[-1][0] == "argmax_embed"  # 14 launches per step
    assert [r[0] for r in rows[:4]] == ["qkv_cache_gemm", "attn_pair", "gemm_chain", "attn_pair"]
    prev_exit = 0.0
    for name, grid, in0, in1, out0, out1 in rows:
        assert grid > 0 and in0 <= in1 and in0 <= out0 <= out1, (name, in0, in1, out0, out1)
        assert in0 >= prev_exit - 1e-6, name                  # a kernel starts after its predecessor's last workgroup has left
        prev_exit = out1
    assert 20.0 < rows[-1][5] < 5000.0                        # one step: tens of microseconds to a few hundred
    raw = m.kernel_stamps(1, rows[1][1])
    assert raw.shape == (rows[1][1], 2) and (raw[:, 1] >= raw[:, 0]).all()
    m.close()
    monkeypatch.setenv("YMT3_STAMP", "1")
    monkeypatch.setenv("YMT3_STEP_KERNEL", "1")
    m = _model(SMALL)
    monkeypatch.delenv("YMT3_STAMP")
    monkeypatch.delenv("YMT3_STEP_KERNEL")
    assert torch.equal(m.inference(a.cuda(), max_token_length=8), plain)
    rows = m.step_stamps()
    assert [r[0] for r in rows] == ["qkv_cache_gemm", "step_layers", "argmax_embed"]          # the option: 3 launches per step
    assert all(r[1] > 0 and r[2] <= r[4] <= r[5] for r in rows)
    m.close()


def test_bad_blob_and_config_are_rejected():
    import ctypes
    from yourmt3_amd import _lib
    from yourmt3_amd.config import to_c
    from yourmt3_amd.tables import derived_tables
    from yourmt3_amd.weights import pack_blob
    lib = _lib.load()
    cfg = SMALL
    W = make_weights(cfg)
    full = {**W, **derived_tables(W, cfg)}
    def create(blob, c=cfg):
        h = ctypes.c_void_p()
        cc = to_c(c, 2)
        rc = lib.ymt3_create(ctypes.byref(cc), ctypes.create_string_buffer(blob, len(blob)), len(blob), 0, ctypes.byref(h))
        if rc == 0:
            lib.ymt3_destroy(h)
        return rc, lib.ymt3_last_error().decode()
    assert create(pack_blob(full))[0] == 0
    rc, msg = create(b"NOTABLOB" + bytes(64))
    assert rc == 2 and "magic" in msg
    rc, msg = create(pack_blob({k: v for k, v in full.items() if k != "dec.3.wo"}))
    assert rc == 2 and "dec.3.wo" in msg
    rc, msg = create(pack_blob({k: v for k, v in full.items() if k != "fe.window"}))
    assert rc == 2 and "fe.window" in msg
    # corrupt directory entries: offset + size wrapping around 2^64, an entry pointing into the header, a truncated file
    import struct
    good = pack_blob(full)
    n_entries = struct.unpack_from("<I", good, 12)[0]
    for off, size in ((2 ** 64 - 16, 64), (16, 64), (len(good) - 16, 2 ** 63)):
        bad = bytearray(good)
        struct.pack_into("<QQ", bad, 16 + 5 * 88 + 72, off, size)                 # entry 5: {name[48], dtype, ndim, shape[4], offset, nbytes}
        rc, msg = create(bytes(bad))
        assert rc == 2 and "out of bounds" in msg, (off, size, rc, msg)
    rc, msg = create(good[:16 + n_entries * 88 - 8])
    assert rc == 2 and "truncated" in msg
    rc, msg = create(good[:len(good) // 2])
    assert rc == 2
    for bad_cfg in (cfg.with_(hop=0), cfg.with_(n_dec_layers=0), cfg.with_(vocab=-16), cfg.with_(max_decode_len=10 ** 6)):
        assert create(good, bad_cfg)[0] == 1                                        # YMT3_ERR_ARG, not a crash
    rc, msg = create(pack_blob(full), cfg.with_(d_kv=32, n_heads=16))
    assert rc == 4
    rc, msg = create(pack_blob(full), cfg.with_(segment_samples=8191 + 128))      # 65 frames: not a multiple of 64
    assert rc == 4 and "n_frames" in msg


def test_short_decoder_tensor_is_refused_at_create():
    """The decoder's weights are bound at create with their dtype and minimum size (runtime.hip: bind_dec_weights): a tensor that is present
    but holds too few bytes is a blob error of ymt3_create, naming the tensor -- not a failure of the first decode inside a stream capture."""
    from yourmt3_amd import _lib
    W = make_weights(SMALL, seed=1234)
    W["dec.0.wo"] = W["dec.0.wo"][: W["dec.0.wo"].shape[0] // 2].contiguous()
    with pytest.raises(_lib.YMT3Error, match=r"ymt3 error 2: .*'dec\.0\.wo' holds"):          # 2 = YMT3_ERR_BLOB
        _model(SMALL, weights=W)


def test_bad_arguments_raise(small):
    from yourmt3_amd._lib import YMT3Error
    e = torch.zeros(1, SMALL.n_frames, SMALL.d_model, dtype=torch.bfloat16).cuda()
    with pytest.raises(YMT3Error):
        small.decode(e, SMALL.max_decode_len + 1)
    with pytest.raises(ValueError):
        small.decode(e, 8, forced=torch.zeros(1, 1, 9, dtype=torch.int32))


# ----------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name,cfg", [("small_t64", SMALL), ("full_t256", FULL), ("mc3_t64", MC3)])
def test_against_golden_fixture(name, cfg):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    m = _model(cfg)
    a = O.synthetic_audio(2, cfg, seed=int(z["seed_audio"]))
    mel = m.logmel(a.cuda())
    assert (mel.cpu() - torch.from_numpy(z["mel"])).abs().max().item() < 1e-3
    enc_ref = bf16_bits_to_f32(z["enc_bf16"]).view(2, cfg.n_frames, cfg.d_model)
    enc = m.encode(mel).float().cpu()
    assert (enc - enc_ref).abs().max().item() <= 0.0625
    n = int(z["n_steps"])
    ref_t = torch.from_numpy(z["tokens"])
    margin = torch.from_numpy(z["margin"])
    got_t, got_l = m.decode(enc_ref.bfloat16().cuda(), n, forced=ref_t.cuda(), return_logits=True)
    steps = z["logit_steps"].tolist()
    assert (got_l.cpu()[:, :, steps, :] - torch.from_numpy(z["logits"])).abs().max().item() < 0.06
    safe = margin >= TAU
    _REPORT["golden_" + name] = {"tau": TAU, "safe_fraction": float(safe.float().mean()),
                                 "ids_differ_below_tau": int((got_t.cpu()[~safe] != ref_t[~safe]).sum())}
    assert safe.float().mean().item() >= MIN_SAFE
    assert torch.equal(got_t.cpu()[safe], ref_t[safe])
    free = m.decode(enc_ref.bfloat16().cuda(), n).cpu()
    _check_stream_prefix(free, ref_t, margin)
    m.close()


# ---------------------------------------------------------------------------------------------- audio ingest (8f rank 2)
# Tolerance: fp32 accumulation of <= 64 fp32 taps against the oracle's float64 accumulation of the same fp32 taps and
# samples: abs 5e-6 on unit-scale audio (observed ~5e-7).  Zero padding and segment layout are exact.
@pytest.mark.parametrize("sr,n,ch,dtype", [(44100, 100000, 2, np.int16), (48000, 70001, 1, np.float32), (8000, 20000, 1, np.int16),
                                           (22050, 30000, 3, np.float32), (16000, 20000, 2, np.int16), (44100, 37, 2, np.int16)])
def test_ingest_matches_oracle(small, sr, n, ch, dtype):
    from oracle import ingest_oracle as IO
    rng = np.random.default_rng(sr + n)
    t = np.arange(n)[:, None] / sr
    x = 0.4 * np.sin(2 * np.pi * 440.0 * (1 + np.arange(ch)[None, :]) * t) + 0.1 * rng.standard_normal((n, ch))
    pcm = (np.clip(x, -1, 1) * 32767).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)
    ref = IO.ingest(pcm, sr, SMALL.sample_rate, SMALL.segment_samples)
    got = small.ingest(torch.from_numpy(pcm), sr)
    assert got.shape == (ref.shape[0], 1, SMALL.segment_samples) and got.dtype == torch.float32
    g = got.cpu().numpy()[:, 0]
    assert np.abs(g - ref).max() < 5e-6
    n_out = small.last_ingest_samples
    assert n_out == -(-n * 16000 // sr) and np.all(g.reshape(-1)[n_out:] == 0)


def test_ingest_edges_and_errors(small):
    from yourmt3_amd._lib import YMT3Error
    empty = small.ingest(torch.zeros(0, 2, dtype=torch.int16), 44100)
    assert empty.shape == (1, 1, SMALL.segment_samples) and float(empty.abs().max()) == 0.0
    with pytest.raises(ValueError):
        small.ingest(torch.zeros(10, 1, dtype=torch.float64), 16000)
    with pytest.raises(YMT3Error):
        small.ingest(torch.zeros(10, 1, dtype=torch.int16), 0)
    with pytest.raises(YMT3Error):                                       # 16000/44101 are coprime: an 882 021-tap filter
        small.ingest(torch.zeros(10, 1, dtype=torch.int16), 44101)
    # exact multiple of the segment length: no extra padded segment
    seg = small.ingest(torch.ones(2 * SMALL.segment_samples, dtype=torch.float32), 16000)
    assert seg.shape[0] == 2 and float((seg - 1).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- continuous batching (8f rank 4)
def _pick_eos(tokens):
    """a token id whose first occurrence falls at different steps for different rows (so rows stop at different lengths)"""
    flat = tokens.reshape(-1, tokens.shape[-1])
    best, best_score = None, -1
    for cand in np.unique(flat):
        first = [int(np.argmax(row == cand)) if (row == cand).any() else -1 for row in flat]
        score = len(set(first))
        if score > best_score:
            best, best_score = int(cand), score
    return best, best_score


@pytest.mark.parametrize("base", [SMALL, MC3], ids=["single-channel", "3-channel"])
def test_continuous_batching_equals_lockstep_batches(base):
    import dataclasses
    n_seg = 9
    audio = O.synthetic_audio(n_seg, base)
    free = _model(dataclasses.replace(base, eos_id=-1))
    toks = np.concatenate(free.inference_file(4, audio), 0)
    free.close()
    eos, spread = _pick_eos(toks)
    assert spread >= 3, "the synthetic decode offers no token that stops rows at >= 3 different lengths"
    cfg = dataclasses.replace(base, eos_id=eos)
    m = _model(cfg)
    ref = np.concatenate(m.inference_file(4, audio), 0)                   # lock-step batches of 4, 4, 1 with EOS -> PAD fill
    L = ref.shape[-1]
    stops = [int(np.argmax(r == eos)) if (r == eos).any() else L for r in ref.reshape(-1, L)]
    assert len(set(stops)) >= 3 and (ref.reshape(-1, L)[0, stops[0] + 1:] == cfg.pad_id).all()
    for slots, interval in [(3, 4), (1, 1), (4, 7), (0, 0)]:
        got = m.inference_stream(audio, slots=slots, interval=interval).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), (slots, interval)
    assert np.array_equal(m.inference_stream(audio[:2], slots=4).cpu().numpy(), ref[:2])      # fewer segments than slots
    assert np.array_equal(m.inference_stream(audio, max_token_length=16, slots=2).cpu().numpy(),
                          np.concatenate(m.inference_file(4, audio, max_token_length=16), 0))  # length cap below max_decode_len
    assert m.inference_stream(audio[:0]).shape == (0, cfg.n_channels, cfg.max_decode_len)
    # the lock-step path is untouched by a stream call in between
    assert np.array_equal(np.concatenate(m.inference_file(4, audio), 0), ref)
    m.close()


def test_token_all_gather_over_rccl_on_one_gpu():
    """The data path's only collective, through RCCL itself: a one-rank `nccl` process group on this GPU runs
    dist.all_gather_into_tensor on the int32 device tensor the decode leaves (the builder's box has one GPU, so the ring is trivial;
    what this checks is that the backend initialises in this image and takes the call exactly as yourmt3_amd.dist makes it)."""
    import torch.distributed as dist
    from yourmt3_amd.dist import all_gather_tokens
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:29577", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        tok = torch.randint(0, 1536, (64, 1, 1024), dtype=torch.int32, device="cuda")
        out = all_gather_tokens(tok, 1, always_collective=True)
        torch.cuda.synchronize()
        assert out.shape == tok.shape and torch.equal(out, tok)
        dist.barrier()
    finally:
        dist.destroy_process_group()
