"""The encoder's kernels one by one, through the test doors of include/ymt3.h (ymt3_test_enc_attention / _seq_attention / _rmsnorm / _spec_embed /
_gemm_ex), against float64 references with the kernels' rounding points (tests/enc_kernel_model.py; tests/test_encoder_kernels_cpu.py shows
that model right and sharp):

  exact probes   inputs whose softmax is one-hot in any correct arithmetic: the output IS a row of V (bf16-exact integer codes), bit for bit
  criterion      an element whose reference value cannot round two ways under the derived bound beta must equal the reference bit for bit;
                 the others lie within beta plus one bf16 ulp.  Each test prints and records (parity report) its stable share, how many
                 unstable elements differ and the worst error / (beta + ulp) (fp32 outputs: error / beta).
  guards         every output buffer lies inside a larger one pre-filled with a sentinel: rows >= M, columns >= N, gaps between strided rows
                 and 64 elements before and after must come back untouched.
  values         huge scores stay finite, a NaN stays where it belongs, a launch repeated gives the same bits.
"""
import pytest
import torch

import enc_kernel_model as K
from oracle import ymt3_oracle as O
from test_gpu_parity import _REPORT, _model
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config

pytestmark = pytest.mark.gpu
CFG = YMT3Config(segment_samples=8191, max_decode_len=64, n_enc_layers=1, n_dec_layers=1)
SENT = 12352.0                      # exact in bf16 and fp32; no test input or result holds it
GUARD = 64


@pytest.fixture(scope="module")
def m():
    mod = _model(CFG, max_batch=2)
    yield mod
    mod.close()


def _record(name, rec):
    rec = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}
    _REPORT["enc_kernel_" + name] = rec
    print(name, rec)
    return rec


def _merge(recs):
    """one record for several checks of one test: the worst of each figure"""
    out = dict(elements=sum(r["elements"] for r in recs), ok=all(r["ok"] for r in recs))
    if "stable_share" not in recs[0]:
        out.update(worst_err_over_beta=max(r["worst_err_over_beta"] for r in recs))
    else:
        out.update(worst_err_over_allowance=max(r["worst_err_over_allowance"] for r in recs),
                   stable_share=min(r["stable_share"] for r in recs), stable_wrong=sum(r["stable_wrong"] for r in recs),
                   unstable_differ=sum(r["unstable_differ"] for r in recs), unstable_wrong=sum(r["unstable_wrong"] for r in recs))
    return out


class Guarded:
    """an output region of n elements inside a buffer of sentinels, GUARD elements on each side"""

    def __init__(self, m, n, dtype, fill=None):
        self.buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=m.device)
        self.view = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.view.copy_(fill.to(m.device))

    def read(self, written):
        """the region on the host after asserting that everything outside `written` (bool mask over the region, or flat indices) is untouched"""
        host = self.buf.cpu()                                             # (ordered behind the launch on the current stream)
        keep = torch.ones(host.numel(), dtype=torch.bool)
        if written.dtype == torch.bool:
            keep[GUARD:GUARD + written.numel()] = ~written.flatten()
        else:
            keep[GUARD + written.flatten()] = False
        assert bool((host[keep] == SENT).all()), "the kernel wrote outside its output"
        return host[GUARD:host.numel() - GUARD]


# ----------------------------------------------------------------------------- encoder attention
def _run_enc(m, q, k, v, bo, fused=True):
    """q, k, v (B, T, H, 64) bf16 on the host -> out (B, T, H, 64) on the host, through one fused qkv buffer (ld = 3 inner) or through
    a query buffer (ldq = inner) and a key/value buffer (ldkv = 2 inner)"""
    B, T, H, _ = q.shape
    inner = H * 64
    rows = lambda x: x.reshape(B * T, inner)
    if fused:
        qkv = torch.cat([rows(q), rows(k), rows(v)], 1).contiguous().to(m.device).flatten()
        qb, kb, vb, ldq, ldkv = qkv, qkv[inner:], qkv[2 * inner:], 3 * inner, 3 * inner
    else:
        qb = rows(q).contiguous().to(m.device).flatten()
        kv = torch.cat([rows(k), rows(v)], 1).contiguous().to(m.device).flatten()
        kb, vb, ldq, ldkv = kv, kv[inner:], inner, 2 * inner
    out = Guarded(m, B * T * inner, torch.bfloat16)
    m.test_enc_attention(qb, ldq, kb, vb, ldkv, bo.to(m.device).contiguous(), out.view, B, T, H)
    return out.read(torch.ones(B * T * inner, dtype=torch.bool)).reshape(B, T, H, 64)


def _exact_rows(got, v, key):
    """rows with a winning key equal that key's V bit for bit; key (B, T, H) with -1 where none.  Returns the checked share."""
    hit = key >= 0
    b, t, h = torch.nonzero(hit, as_tuple=True)
    assert torch.equal(got[hit], v[b, key[hit], h]), "a one-hot row did not return its key's V"
    return float(hit.double().mean())


@pytest.mark.parametrize("T", K.ENC_T)
def test_enc_attention_bias_and_v_probe_is_exact(m, T):
    """every table index 0 .. 2T-2 is the lone peak of some head once: the bias index map, the V address map and the query-tile split, exactly"""
    recs, shares = [], []
    for j in range(K.bias_probe_launches(T)):
        q, k, v, bo, peak, key = K.bias_probe_case(T, j)
        got = _run_enc(m, q, k, v, bo, fused=bool(j % 2))
        key = key.T[None].expand(q.shape[0], -1, -1)                      # (B, T, H)
        shares.append(_exact_rows(got, v, key))
        uo, ub = K.uniform_row(v)                                         # the rows without a peak: the mean of V
        miss = key < 0
        if bool(miss.any()):
            recs.append(K.check_bf16(got[miss], uo[:, None].expand(-1, T, -1, -1)[miss], ub[:, None].expand(-1, T, -1, -1)[miss]))
    rec = _record(f"attn_bias_probe_T{T}", dict(_merge(recs), launches=len(shares), exact_row_share=sum(shares) / len(shares)))
    assert rec["ok"] and rec["exact_row_share"] > 0.4, rec


@pytest.mark.parametrize("T", K.ENC_T)
def test_enc_attention_score_probe_is_exact(m, T):
    q, k, v, bo, key = K.score_probe_case(T)
    ref, beta, _ = K.enc_attention_reference(q, k, v, bo)
    got = _run_enc(m, q, k, v, bo)
    share = _exact_rows(got, v, key)
    rec = _record(f"attn_score_probe_T{T}", dict(K.check_bf16(got, ref["o"], beta), exact_row_share=share))
    assert rec["ok"] and share >= 0.7, rec


@pytest.mark.parametrize("case", K.enc_random_cases(), ids=lambda c: c[0])
def test_enc_attention_random_cases_meet_the_criterion(m, case):
    name, T, B, H, fused, qs, bs = case
    q, k, v, bo = K.enc_random_case(T, B, H, qs, bs)
    ref, beta, _ = K.enc_attention_reference(q, k, v, bo)
    got = _run_enc(m, q, k, v, bo, fused)
    rec = _record("attn_" + name, K.check_bf16(got, ref["o"], beta))
    assert rec["ok"] and rec["stable_share"] >= K.MIN_STABLE, rec


@pytest.mark.parametrize("T", K.ENC_T)
def test_enc_attention_values(m, T):
    """scores of +-3e4 stay finite; a NaN query row reaches only its own output row; a NaN in V stays inside its (segment, head); the same launch
    twice gives the same bits"""
    B, H = 2, 4
    g = torch.Generator().manual_seed(T)
    a = 21.625                                                            # 64 a^2 = 29929
    sign = torch.where(torch.rand(B, T, H, 1, generator=g) < 0.5, -1.0, 1.0)
    q = torch.full((B, T, H, 64), a).bfloat16()
    k = (sign * a).expand(B, T, H, 64).bfloat16()
    v = torch.randn(B, T, H, 64, generator=g).bfloat16()
    bo = torch.randn(H, 2 * T - 1, generator=g)
    ref, beta, _ = K.enc_attention_reference(q, k, v, bo)
    assert float(ref["s"].abs().max()) > 2.9e4
    got = _run_enc(m, q, k, v, bo)
    assert bool(torch.isfinite(got.float()).all())
    rec = _record(f"attn_huge_scores_T{T}", K.check_bf16(got, ref["o"], beta))
    assert rec["ok"], rec

    q, k, v, bo = K.enc_random_case(T, B, H, 0.5, 0.5, seed=9)
    clean = _run_enc(m, q, k, v, bo)
    assert torch.equal(_run_enc(m, q, k, v, bo).view(torch.int16), clean.view(torch.int16))
    b0, t0, h0 = 1, T - 3, 2
    qn = q.clone()
    qn[b0, t0, h0, 17] = float("nan")
    got = _run_enc(m, qn, k, v, bo)
    bad = torch.zeros(B, T, H, dtype=torch.bool)
    bad[b0, t0, h0] = True
    assert bool(got[bad].float().isnan().all()) and torch.equal(got[~bad].view(torch.int16), clean[~bad].view(torch.int16))
    vn = v.clone()
    vn[b0, 5, h0, 9] = float("nan")
    got = _run_enc(m, q, k, vn, bo)
    bad = torch.zeros(B, T, H, dtype=torch.bool)
    bad[b0, :, h0] = True
    assert bool(got[b0, :, h0, 9].float().isnan().all())
    assert torch.equal(got[~bad].view(torch.int16), clean[~bad].view(torch.int16))


# ----------------------------------------------------------------------------- sequence attention
def _place(buf, x, starts, step, at=0):
    """x (n_seq, T, D) into the flat buffer at starts[s] + t step + at"""
    n, T, D = x.shape
    idx = starts[:, None, None] + torch.arange(T)[None, :, None] * step + torch.arange(D)[None, None, :] + at
    buf[idx] = x
    return idx


def _run_seq(m, q, k, v, bo, inner_n, layout):
    """q (n_seq, Tq, H, 64), k / v (n_seq, Tk, H, 64) on the host, laid out as K.seq_layouts says (the gaps hold 999) -> out (n_seq, Tq, H, 64)"""
    n_seq, Tq, H, _ = q.shape
    Tk, D = k.shape[1], H * 64
    lay = K.seq_layouts(n_seq, inner_n, Tq, Tk, H)[layout]
    qbuf = torch.full((lay["q_size"],), 999.0).bfloat16()
    kvbuf = qbuf if lay["kv_size"] == 0 else torch.full((lay["kv_size"],), 999.0).bfloat16()
    _place(qbuf, q.reshape(n_seq, Tq, D), K.seq_starts(n_seq, inner_n, lay["q"]), lay["q"][2])
    _place(kvbuf, k.reshape(n_seq, Tk, D), K.seq_starts(n_seq, inner_n, lay["kv"]), lay["kv"][2], lay["k_at"])
    _place(kvbuf, v.reshape(n_seq, Tk, D), K.seq_starts(n_seq, inner_n, lay["kv"]), lay["kv"][2], lay["v_at"])
    qd = qbuf.to(m.device)
    kvd = qd if lay["kv_size"] == 0 else kvbuf.to(m.device)
    out = Guarded(m, lay["o_size"], torch.bfloat16)
    oidx = _place(torch.zeros(lay["o_size"]), torch.zeros(n_seq, Tq, D), K.seq_starts(n_seq, inner_n, lay["o"]), lay["o"][2])
    m.test_seq_attention(qd, kvd[lay["k_at"]:], kvd[lay["v_at"]:], out.view, None if bo is None else bo.to(m.device).contiguous(), n_seq, H, Tq, Tk,
                         inner_n, lay["q"], lay["kv"], lay["o"])
    return out.read(oidx)[oidx].reshape(n_seq, Tq, H, 64)


@pytest.mark.parametrize("case", K.seq_cases(), ids=lambda c: c[0])
def test_seq_attention_random_cases_meet_the_criterion(m, case):
    name, Tq, Tk, wb, n_seq, inner_n, layout, qs, bs = case
    q, k, v, bo = K.seq_random_case(Tq, Tk, wb, n_seq, qs, bs)
    ref, beta, _ = K.seq_attention_reference(q, k, v, bo)
    got = _run_seq(m, q, k, v, bo, inner_n, layout)
    rec = _record("seq_" + name, K.check_bf16(got, ref["o"], beta))
    assert rec["ok"] and rec["stable_share"] >= K.MIN_STABLE, rec


@pytest.mark.parametrize("T", [s[0] for s in K.SEQ_SHAPES if s[2]])
def test_seq_attention_bias_and_v_probe_is_exact(m, T):
    H, n_seq, inner_n = K.SEQ_PROBE_H, 5, 3
    recs, shares = [], []
    for j in range((2 * T - 1 + H - 1) // H):
        q, k, v, bo, peak, key = K.seq_bias_probe_case(T, n_seq, j)
        got = _run_seq(m, q, k, v, bo, inner_n, "temporal" if j % 2 else "padded")
        key = key.T[None].expand(n_seq, -1, -1)
        shares.append(_exact_rows(got, v, key))
        uo, ub = K.uniform_row(v)
        miss = key < 0
        if bool(miss.any()):
            recs.append(K.check_bf16(got[miss], uo[:, None].expand(-1, T, -1, -1)[miss], ub[:, None].expand(-1, T, -1, -1)[miss]))
    rec = _record(f"seq_bias_probe_T{T}", dict(_merge(recs), launches=len(shares), exact_row_share=sum(shares) / len(shares)))
    assert rec["ok"] and rec["exact_row_share"] > 0.4, rec


@pytest.mark.parametrize("shape", K.SEQ_SHAPES, ids=str)
def test_seq_attention_score_probe_is_exact(m, shape):
    Tq, Tk, wb = shape
    recs = []
    for n_seq, inner_n, layout in ((1, 1, "padded"), (5, 3, "temporal" if Tq == Tk else "padded")):
        q, k, v, bo, key = K.seq_score_probe_case(Tq, Tk, n_seq, wb)
        ref, beta, _ = K.seq_attention_reference(q, k, v, bo)
        got = _run_seq(m, q, k, v, bo, inner_n, layout)
        share = _exact_rows(got, v, key)
        assert share >= (0.7 if wb else 1.0)
        recs.append(K.check_bf16(got, ref["o"], beta))
    rec = _record(f"seq_score_probe_{Tq}x{Tk}", _merge(recs))
    assert rec["ok"], rec


def test_seq_attention_values(m):
    """as test_enc_attention_values, at the shape with more query tiles than waves (48 queries, 64 keys, two waves) and at (128, 128) with a bias"""
    for Tq, Tk, wb in ((48, 64, False), (128, 128, True)):
        n_seq, inner_n, layout = 5, 3, "padded"
        g = torch.Generator().manual_seed(Tq)
        a = 21.625
        sign = torch.where(torch.rand(n_seq, Tk, K.SEQ_H, 1, generator=g) < 0.5, -1.0, 1.0)
        q = torch.full((n_seq, Tq, K.SEQ_H, 64), a).bfloat16()
        k = (sign * a).expand(n_seq, Tk, K.SEQ_H, 64).bfloat16()
        v = torch.randn(n_seq, Tk, K.SEQ_H, 64, generator=g).bfloat16()
        bo = torch.randn(K.SEQ_H, 2 * Tk - 1, generator=g) if wb else None
        ref, beta, _ = K.seq_attention_reference(q, k, v, bo)
        got = _run_seq(m, q, k, v, bo, inner_n, layout)
        assert bool(torch.isfinite(got.float()).all())
        rec = _record(f"seq_huge_scores_{Tq}x{Tk}", K.check_bf16(got, ref["o"], beta))
        assert rec["ok"], rec

        q, k, v, bo = K.seq_random_case(Tq, Tk, wb, n_seq, 0.5, 0.5, seed=9)
        clean = _run_seq(m, q, k, v, bo, inner_n, layout)
        assert torch.equal(_run_seq(m, q, k, v, bo, inner_n, layout).view(torch.int16), clean.view(torch.int16))
        s0, t0, h0 = 3, Tq - 2, 1
        qn = q.clone()
        qn[s0, t0, h0, 3] = float("nan")
        got = _run_seq(m, qn, k, v, bo, inner_n, layout)
        bad = torch.zeros(n_seq, Tq, K.SEQ_H, dtype=torch.bool)
        bad[s0, t0, h0] = True
        assert bool(got[bad].float().isnan().all()) and torch.equal(got[~bad].view(torch.int16), clean[~bad].view(torch.int16))
        vn = v.clone()
        vn[s0, 7, h0, 9] = float("nan")
        got = _run_seq(m, q, k, vn, bo, inner_n, layout)
        bad = torch.zeros(n_seq, Tq, K.SEQ_H, dtype=torch.bool)
        bad[s0, :, h0] = True
        assert bool(got[s0, :, h0, 9].float().isnan().all())
        assert torch.equal(got[~bad].view(torch.int16), clean[~bad].view(torch.int16))


# ----------------------------------------------------------------------------- RMS norm, spectral embedding
def _run_rmsnorm(m, x, gain, eps):
    """x (M, d) fp32 -> out (M, d) bf16 on the host; the output buffer has three more rows, which must stay untouched"""
    M, d = x.shape
    out = Guarded(m, (M + 3) * d, torch.bfloat16)
    m.test_rmsnorm(x.contiguous().to(m.device).flatten(), gain.to(m.device), out.view, M, d, eps)
    written = torch.zeros(M + 3, d, dtype=torch.bool)
    written[:M] = True
    return out.read(written).reshape(M + 3, d)[:M]


@pytest.mark.parametrize("d", K.RMS_D)
def test_rmsnorm_meets_the_criterion_at_every_row_count(m, d):
    recs = []
    for i, M in enumerate(K.RMS_M):
        x, gain = K.rmsnorm_case(M, d)
        eps = (1e-6, 1e-3)[i % 2]
        out, o = K.rmsnorm_model(x, gain, eps)
        recs.append(K.check_bf16(_run_rmsnorm(m, x, gain, eps), o, K.rmsnorm_beta(o, d)))
    rec = _record(f"rmsnorm_d{d}", _merge(recs))
    assert rec["ok"] and rec["stable_share"] >= K.MIN_STABLE, rec


@pytest.mark.parametrize("M", [4096, 4097, 4127])
def test_rmsnorm_d128_kernel_equals_the_generic_kernel_bit_for_bit(m, M):
    """d = 128 with M >= 4096 takes the hand-scheduled kernel ("same arithmetic"): the same rows through two calls of fewer than 4096 rows
    take the generic one"""
    x, gain = K.rmsnorm_case(M, 128, seed=3)
    xv, _ = K.rmsnorm_value_rows(128)
    x[100:108] = xv
    x[M - 8:] = xv                                                        # the ragged tail too
    for eps in (1e-6, 1e-3):
        big = _run_rmsnorm(m, x, gain, eps)
        h = 2040
        two = torch.cat([_run_rmsnorm(m, x[:h], gain, eps), _run_rmsnorm(m, x[h:], gain, eps)])
        assert M - h < 4096 and torch.equal(big.view(torch.int16), two.view(torch.int16))
    _record(f"rmsnorm_d128_bit_equal_M{M}", {"rows": M, "equal": True})


@pytest.mark.parametrize("d", K.RMS_D)
def test_rmsnorm_values(m, d):
    """a zero row, rows whose squares overflow or are subnormal in fp32, negative and zero gains, both eps; a NaN row stays alone"""
    x, rows = K.rmsnorm_value_rows(d)
    _, gain = K.rmsnorm_case(8, d)
    for eps in (1e-6, 1e-3):
        got = _run_rmsnorm(m, x, gain, eps)
        out, o = K.rmsnorm_model(x, gain, eps)
        o32 = O._r(O.rmsnorm(x, gain, eps), True)                         # where x^2 overflows fp32 the contract is the fp32 oracle's: scale 0
        over = rows["overflow"]
        assert 6 in over.tolist() and (rows["huge"] in over.tolist()) == (d >= 512)
        assert torch.equal(got[over].float(), o32[over]) and bool((o32[over] == 0).all())
        assert bool(got[rows["nan"]].float().isnan().all())
        assert bool((got[rows["zero"]].float() == 0).all())
        rest = torch.ones(8, dtype=torch.bool)
        rest[over] = False
        rest[rows["nan"]] = False
        rec = K.check_bf16(got[rest], o[rest], K.rmsnorm_beta(o[rest], d))
        assert rec["ok"], rec
        assert bool((got[rows["tiny"]].float()[gain != 0] != 0).all())    # 1e-20 rows are scaled by rsqrt(eps), not flushed


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("F", [64, 128])
def test_spec_embed_meets_the_criterion(m, d, F):
    n_rows = 2 * F + 7                                                    # not a multiple of the four rows of a workgroup
    g = torch.Generator().manual_seed(d + F)
    mel = torch.randn(n_rows, generator=g) * 4 - 6
    w, gain = torch.randn(d, generator=g), torch.randn(d, generator=g)
    pos = torch.randn(F, d, generator=g).bfloat16()
    x = K.spec_embed_input(mel, w, pos, F)
    eps = 1e-6
    out, o = K.rmsnorm_model(x, gain, eps)
    buf = Guarded(m, (n_rows + 3) * d, torch.bfloat16)
    m.test_spec_embed(mel.to(m.device), w.to(m.device), pos.to(m.device).flatten(), gain.to(m.device), buf.view, n_rows, F, d, eps)
    written = torch.zeros(n_rows + 3, d, dtype=torch.bool)
    written[:n_rows] = True
    got = buf.read(written).reshape(n_rows + 3, d)[:n_rows]
    rec = _record(f"spec_embed_d{d}_F{F}", K.check_bf16(got, o, K.rmsnorm_beta(o, d)))
    assert rec["ok"] and rec["stable_share"] >= K.MIN_STABLE, rec


# ----------------------------------------------------------------------------- GEMM epilogues
_GEMM = {}
HEADMAJOR_SPLIT = {(1, 128, 64): (1, 2), (129, 128, 128): (43, 1), (200, 256, 512): (50, 2), (4224, 1024, 512): (64, 8), (4100, 1024, 192): (100, 4)}   # (T, H)


def _gemm_ref(M, N, K_):
    if (M, N, K_) not in _GEMM:
        A, W, bias, resid = K.gemm_case(M, N, K_)
        _GEMM[(M, N, K_)] = (A, W, bias, resid) + K.gemm_reference_and_bound(A, W)
    return _GEMM[(M, N, K_)]


def _run_gemm(m, epi, A, W, lda, ldc, bias=None, resid=None, T=0, H=0, launches=1):
    """A (M, K), W (N, K) bf16 on the host -> the (M, N) output (head-major: its own shape) on the host.  The pad columns of A hold NaN (a read
    of them poisons the result), the output lies in a Guarded buffer of M + 2 rows of ldc."""
    M, K_ = A.shape
    N = W.shape[0]
    Ab = torch.full((M, lda), float("nan")).bfloat16()
    Ab[:, :K_] = A
    f32 = epi in (K.EPI_F32, K.EPI_RESID)
    rows = M if epi == K.EPI_KV_HEADMAJOR else M + 2
    ldc = N if epi == K.EPI_KV_HEADMAJOR else ldc
    written = torch.zeros(rows, ldc, dtype=torch.bool)
    written[:M, :N] = True
    fill = None
    if resid is not None:
        fill = torch.full((rows, ldc), SENT)
        fill[:M, :N] = resid
        fill = fill.flatten()
    out = Guarded(m, rows * ldc, torch.float32 if f32 else torch.bfloat16, fill)
    Ad, Wd = Ab.to(m.device).flatten(), W.contiguous().to(m.device).flatten()
    bd = None if bias is None else bias.to(m.device)
    for _ in range(launches):
        m.test_gemm_ex(epi, Ad, Wd, out.view, M, N, K_, lda=lda, ldc=ldc, bias=bd, T=T, H=H, n_seg=M // T if T else 0)
    got = out.read(written).reshape(rows, ldc)[:M, :N]
    return got.reshape(N // (H * 64), M // T, H, T, 64) if epi == K.EPI_KV_HEADMAJOR else got


@pytest.mark.parametrize("epi", range(5), ids=["f32_bias", "bf16", "bf16_relu", "resid", "kv_headmajor"])
@pytest.mark.parametrize("M,N,K_", K.GEMM_SMALL + K.GEMM_BIG)
def test_gemm_epilogue_meets_the_criterion(m, epi, M, N, K_):
    """every epilogue on the 128 x 128 kernel (three shapes) and on the pipelined 256 x 128 one (two), with contiguous rows and with
    lda = K + 64, ldc = N + 128; EPI_RESID twice in a row on a non-zero residual"""
    A, W, bias, resid, ref, bound = _gemm_ref(M, N, K_)
    T, H = HEADMAJOR_SPLIT[(M, N, K_)]
    recs = []
    for lda, ldc in ((K_, N), (K_ + 64, N + 128)):
        if epi == K.EPI_F32:
            o, beta = K.gemm_epilogue_reference(epi, A, W, bias=bias)
            recs.append(K.check_f32(_run_gemm(m, epi, A, W, lda, ldc, bias=bias), o, beta))
        elif epi == K.EPI_RESID:
            o1, b1 = K.gemm_epilogue_reference(epi, A, W, resid=resid)
            recs.append(K.check_f32(_run_gemm(m, epi, A, W, lda, ldc, resid=resid), o1, b1))
            o2 = o1 + ref                                                  # the second launch adds the product again: two roundings, two bounds
            recs.append(K.check_f32(_run_gemm(m, epi, A, W, lda, ldc, resid=resid, launches=2), o2, b1 + bound + 2.0 ** -24 * o2.abs()))
        elif epi == K.EPI_KV_HEADMAJOR:
            o, beta = K.gemm_epilogue_reference(epi, A, W, T=T, H=H)
            recs.append(K.check_bf16(_run_gemm(m, epi, A, W, lda, ldc, T=T, H=H), o, beta))
        else:
            recs.append(K.check_bf16(_run_gemm(m, epi, A, W, lda, ldc), ref, bound, relu=epi == K.EPI_BF16_RELU))
    rec = _record(f"gemm_epi{epi}_{M}x{N}x{K_}", _merge(recs))
    assert rec["ok"], rec
    if "stable_share" in rec:
        assert rec["stable_share"] >= K.MIN_STABLE, rec


@pytest.mark.parametrize("M", [192, 4224])
def test_gemm_permutation_probe_through_the_bf16_epilogue(m, M):
    """tests/test_gpu_parity.py's probe (row i of A selects column 7 i mod K of W) through the LDS-turned bf16 store: exact"""
    P, Wp, exact = K.permutation_probe(M, 1024, 128)
    for lda, ldc in ((128, 1024), (192, 1152)):
        got = _run_gemm(m, K.EPI_BF16, P, Wp, lda, ldc)
        assert torch.equal(got.float(), exact)


@pytest.mark.parametrize("T", [64, 256])
@pytest.mark.parametrize("n_seg", [3, 66])
def test_gemm_permutation_probe_through_the_head_major_scatter(m, T, n_seg):
    """every element lands in [n / (H 64)][m / T][h][m % T][64], bit exact, from the 128 x 128 kernel (3 segments) and the pipelined one (66)"""
    M, H = n_seg * T, 8
    P, Wp, exact = K.permutation_probe(M, 1024, 128)
    got = _run_gemm(m, K.EPI_KV_HEADMAJOR, P, Wp, 128, 1024, T=T, H=H)
    assert torch.equal(got.float(), K.headmajor(exact, T, H))


# ----------------------------------------------------------------------------- the doors refuse what they must
def test_doors_refuse_bad_arguments_and_work_on_the_next_call(m):
    dev = m.device
    bf = lambda n: torch.zeros(n, dtype=torch.bfloat16, device=dev)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    lib, h, s = m._lib, m._handle, m._stream()
    p = lambda t, off=0: t.data_ptr() + off
    a, w, c, x, o = bf(128 * 64), bf(128 * 64), f32(128 * 128), f32(4 * 128), bf(4 * 128)
    raw = {
        "gemm null a": lambda: lib.ymt3_test_gemm_ex(h, 0, None, p(w), p(c), None, 128, 128, 64, 64, 64, 128, 0, 0, 0, s),
        "gemm null out": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w), None, None, 128, 128, 64, 64, 64, 128, 0, 0, 0, s),
        "gemm misaligned w": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w, 2), p(c), None, 1, 128, 64, 64, 64, 128, 0, 0, 0, s),
        "gemm misaligned bias": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w), p(c), p(c, 4), 1, 128, 64, 64, 64, 128, 0, 0, 0, s),
        "gemm N % 128": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w), p(c), None, 1, 64, 64, 64, 64, 64, 0, 0, 0, s),
        "gemm K % 64": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w), p(c), None, 1, 128, 32, 32, 32, 128, 0, 0, 0, s),
        "gemm lda < K": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w), p(c), None, 1, 128, 64, 56, 64, 128, 0, 0, 0, s),
        "gemm ldc < N": lambda: lib.ymt3_test_gemm_ex(h, 0, p(a), p(w), p(c), None, 1, 128, 64, 64, 64, 120, 0, 0, 0, s),
        "gemm epilogue 5": lambda: lib.ymt3_test_gemm_ex(h, 5, p(a), p(w), p(c), None, 1, 128, 64, 64, 64, 128, 0, 0, 0, s),
        "gemm head-major M != n_seg T": lambda: lib.ymt3_test_gemm_ex(h, 4, p(a), p(w), p(c), None, 128, 128, 64, 64, 64, 128, 64, 2, 3, s),
        "gemm bias with bf16": lambda: lib.ymt3_test_gemm_ex(h, 1, p(a), p(w), p(c), p(c), 1, 128, 64, 64, 64, 128, 0, 0, 0, s),
        "rmsnorm null gain": lambda: lib.ymt3_test_rmsnorm(h, p(x), None, p(o), 4, 128, 1e-6, s),
        "rmsnorm misaligned x": lambda: lib.ymt3_test_rmsnorm(h, p(x, 4), p(x), p(o), 3, 128, 1e-6, s),
        "rmsnorm d % 4": lambda: lib.ymt3_test_rmsnorm(h, p(x), p(x), p(o), 1, 130, 1e-6, s),
        "attention T = 96": lambda: lib.ymt3_test_enc_attention(h, p(a), 64, p(a), p(a), 64, p(c), p(w), 1, 96, 1, s),
        "attention null bias": lambda: lib.ymt3_test_enc_attention(h, p(a), 64, p(a), p(a), 64, None, p(w), 1, 64, 1, s),
        "attention ld < inner": lambda: lib.ymt3_test_enc_attention(h, p(a), 64, p(a), p(a), 64, p(c), p(w), 1, 64, 2, s),
        "attention misaligned v": lambda: lib.ymt3_test_enc_attention(h, p(a), 64, p(a), p(a, 8), 64, p(c), p(w), 1, 64, 1, s),
        "spec_embed d > 256": lambda: lib.ymt3_test_spec_embed(h, p(x), p(x), p(a), p(x), p(o), 1, 4, 260, 1e-6, s),
        "spec_embed d % 4": lambda: lib.ymt3_test_spec_embed(h, p(x), p(x), p(a), p(x), p(o), 1, 4, 130, 1e-6, s),
        "spec_embed null pos": lambda: lib.ymt3_test_spec_embed(h, p(x), p(x), None, p(x), p(o), 1, 4, 128, 1e-6, s),
        "seq null args": lambda: lib.ymt3_test_seq_attention(h, None, s),
    }

    def seq(**kw):
        base = dict(q=p(a), k=p(a), v=p(a), out=p(w), bias_off=None, n_seq=1, H=1, Tq=32, Tk=32, inner_n=1, q_outer=0, q_inner=0, q_step=64, kv_outer=0,
                    kv_inner=0, kv_step=64, o_outer=0, o_inner=0, o_step=64)
        base.update(kw)
        args = _lib.SeqAttnArgs(**base)
        return lambda: lib.ymt3_test_seq_attention(h, args, s)
    raw.update({"seq Tk = 16": seq(Tk=16), "seq Tq % 16": seq(Tq=24), "seq bias with Tq != Tk": seq(bias_off=p(c), Tq=16), "seq stride % 8": seq(q_step=68),
                "seq negative stride": seq(o_outer=-64), "seq zero step": seq(kv_step=0), "seq null v": seq(v=None), "seq misaligned out": seq(out=p(w, 2))})
    for name, call in raw.items():
        assert call() == 1, name                                          # YMT3_ERR_ARG
        assert len(lib.ymt3_last_error()) > 10, name
    with pytest.raises(_lib.YMT3Error):
        m.test_rmsnorm(x, x, o, 1, 130, 1e-6)

    small = {
        "gemm a": lambda: m.test_gemm_ex(0, bf(128 * 64 - 1), w, c, 128, 128, 64),
        "gemm a with lda": lambda: m.test_gemm_ex(0, a, w, f32(200 * 128), 100, 128, 64, lda=128),
        "gemm w": lambda: m.test_gemm_ex(0, a, bf(128 * 64 - 8), c, 128, 128, 64),
        "gemm out": lambda: m.test_gemm_ex(0, a, w, f32(128 * 128 - 1), 128, 128, 64),
        "gemm out with ldc": lambda: m.test_gemm_ex(0, a, w, c, 100, 128, 64, ldc=256),
        "gemm out dtype": lambda: m.test_gemm_ex(1, a, w, c, 128, 128, 64),
        "gemm bias": lambda: m.test_gemm_ex(0, a, w, c, 128, 128, 64, bias=f32(127)),
        "gemm head-major out": lambda: m.test_gemm_ex(4, a, w, bf(128 * 128 - 64), 128, 128, 64, T=64, H=2, n_seg=2),
        "rmsnorm x": lambda: m.test_rmsnorm(x, f32(128), o, 5, 128, 1e-6),
        "rmsnorm out": lambda: m.test_rmsnorm(x, f32(128), bf(3 * 128), 4, 128, 1e-6),
        "attention k": lambda: m.test_enc_attention(bf(64 * 64), 64, bf(64 * 64 - 8), bf(64 * 64), 64, f32(127), bf(64 * 64), 1, 64, 1),
        "attention v in a fused buffer": lambda: m.test_enc_attention(bf(64 * 192), 192, bf(64 * 192)[64:], bf(64 * 192)[136:], 192, f32(127), bf(64 * 64), 1, 64, 1),
        "attention bias": lambda: m.test_enc_attention(bf(64 * 64), 64, bf(64 * 64), bf(64 * 64), 64, f32(126), bf(64 * 64), 1, 64, 1),
        "attention out": lambda: m.test_enc_attention(bf(128 * 64), 64, bf(128 * 64), bf(128 * 64), 64, f32(127), bf(64 * 64), 2, 64, 1),
        "seq q": lambda: m.test_seq_attention(bf(5 * 32 * 64 - 8), bf(5 * 32 * 64), bf(5 * 32 * 64), bf(5 * 32 * 64), None, 5, 1, 32, 32, 1, (2048, 0, 64), (2048, 0, 64),
                                              (2048, 0, 64)),
        "seq out by inner": lambda: m.test_seq_attention(bf(6 * 32 * 64), bf(6 * 32 * 64), bf(6 * 32 * 64), bf(4 * 32 * 64), None, 5, 1, 32, 32, 3, (6144, 2048, 64),
                                                         (6144, 2048, 64), (6144, 2048, 64)),
        "spec_embed mel": lambda: m.test_spec_embed(f32(6), f32(128), bf(4 * 128), f32(128), bf(7 * 128), 7, 4, 128, 1e-6),
        "spec_embed pos": lambda: m.test_spec_embed(f32(7), f32(128), bf(3 * 128), f32(128), bf(7 * 128), 7, 4, 128, 1e-6),
        "spec_embed out": lambda: m.test_spec_embed(f32(7), f32(128), bf(4 * 128), f32(128), bf(6 * 128), 7, 4, 128, 1e-6),
    }
    for name, call in small.items():
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        m.test_rmsnorm(x.cpu(), f32(128), o, 4, 128, 1e-6)

    # every door still works
    P, Wp, exact = K.permutation_probe(128, 128, 64)
    assert torch.equal(_run_gemm(m, K.EPI_BF16, P, Wp, 64, 128).float(), exact)
    xr, gain = K.rmsnorm_case(4, 128)
    out, o64 = K.rmsnorm_model(xr, gain, 1e-6)
    assert K.check_bf16(_run_rmsnorm(m, xr, gain, 1e-6), o64, K.rmsnorm_beta(o64, 128))["ok"]
    q, k, v, bo, key = K.score_probe_case(64)
    _exact_rows(_run_enc(m, q, k, v, bo), v, key)
    q, k, v, bo, key = K.seq_score_probe_case(16, 32, 1, False)
    _exact_rows(_run_seq(m, q, k, v, bo, 1, "padded"), v, key)
