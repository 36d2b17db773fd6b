"""References, criteria and inputs for the per-kernel encoder tests (tests/test_encoder_kernels.py on the GPU, tests/test_encoder_kernels_cpu.py
for the model itself).  TEST INFRASTRUCTURE ONLY, CPU only.

Each reference is the kernel's CONTRACT written in float64 with the kernel's rounding points:

  attention    s = q.k + bias[key - q + T - 1] (no scale), e = exp(s - max), P = bf16(e), out = bf16((P.V) / sum(e))   (sum of the UNROUNDED e)
  rmsnorm      out = bf16(x rsqrt(mean(x^2) + eps) gain)                                                               (no mean subtraction)
  spec_embed   x = f32(f32(mel w) + pos)  (mul, then add: two fp32 roundings), then the rmsnorm above
  GEMM         value_regimes.gemm_reference_and_bound, then the epilogue

Evaluated with dtype=torch.float32 the same functions run the oracle's own operations in the oracle's order (oracle/ymt3_oracle.py::attention
/ rmsnorm): tests/test_encoder_kernels_cpu.py ties them to it.

Criterion for a bf16 output (the TAU idea of tests/test_gpu_parity.py, per element).  `o` is the reference's value BEFORE the final rounding and
`beta` a derived bound on how far a correct device's value before ITS final rounding can lie from o.  An element is STABLE when the whole
interval [o - beta, o + beta] rounds to one bf16 value: there the device must give that value bit for bit.  On the others it must lie within
beta plus one bf16 ulp of o.  beta is derived from the arithmetic (below, at each helper), never from what a device returned; the criterion is
only worth something while nearly everything is stable, so every random case must have a stable share >= MIN_STABLE under the reference alone.
"""
from __future__ import annotations

import functools

import torch

from oracle import ymt3_oracle as O
from value_regimes import gemm_reference_and_bound

MIN_STABLE = 0.95
EPI_F32, EPI_BF16, EPI_BF16_RELU, EPI_RESID, EPI_KV_HEADMAJOR = range(5)


# ----------------------------------------------------------------------------- bf16 helpers (float64 in, float64 out)
def rb(x):
    """round to nearest-even bf16, as the device does from its fp32 value"""
    return x.float().bfloat16().to(x.dtype)


def trunc_bf16(x):
    """the WRONG conversion (mutants): drop the low 16 bits of the fp32 value"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def ulp_bf16(x):
    """spacing of the bf16 values around |x| (8 significant bits); the subnormal spacing 2^-133 at and near zero"""
    _, ex = torch.frexp(x.double().abs())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex.clamp(min=-125) - 8)


def judge_bf16(got, o, beta, relu=False):
    """The criterion of the module docstring, per element: (stable, bad_stable, bad_unstable, err, allow, rounds_to) as tensors of o's shape.
    check_bf16 reduces them to figures; tests/dec_kernel_model.py reduces them per (row, head) for its candidate rule."""
    got, o, beta = got.double(), o.double(), beta.double()
    ref = o
    if relu:
        o = ref.clamp(min=0.0)
        lo, hi = rb((ref - beta).clamp(min=0.0)), rb((ref + beta).clamp(min=0.0))
    else:
        lo, hi = rb(o - beta), rb(o + beta)
    stable = lo == hi
    err = (got - o).abs()
    allow = beta + ulp_bf16(o.abs() + beta)
    bad_stable = stable & (got != lo)
    bad_unstable = ~stable & ~(err <= allow)
    if relu:
        bad_unstable &= ~((ref.abs() <= beta) & (got == 0))
    return stable, bad_stable, bad_unstable, err, allow, rb(o)


def check_bf16(got, o, beta, relu=False):
    """The criterion of the module docstring.  got: the device's bf16 values; o, beta: float64.  relu: o = max(ref, 0) was applied to a
    reference `o` passed UNclamped: an element with |ref| <= beta may be 0 or within beta.  Returns the figures and `ok`; worst_err_over_allowance
    is the largest |got - o| / (beta + ulp) over the unstable elements (a bf16 result hides the device's value before its rounding, so up to
    half an ulp of every figure is that rounding and 0.5 is what a perfect device shows on an unstable element)."""
    stable, bad_stable, bad_unstable, err, allow, ro = judge_bf16(got, o, beta, relu)
    n_un = int((~stable).sum())
    return dict(elements=int(stable.numel()), stable_share=float(stable.double().mean()), stable_wrong=int(bad_stable.sum()),
                unstable=n_un, unstable_differ=int((~stable & (got.double() != ro)).sum()), unstable_wrong=int(bad_unstable.sum()),
                worst_err_over_allowance=float((err / allow)[~stable].max()) if n_un else 0.0,
                ok=not bool(bad_stable.any() or bad_unstable.any()))


def check_f32(got, ref, bound):
    """an fp32 output against a float64 reference and its derived bound"""
    err = (got.double() - ref).abs()
    return dict(elements=int(ref.numel()), worst_err_over_beta=float((err / bound).max()), ok=bool((err <= bound).all()))


# ----------------------------------------------------------------------------- attention
def bias_from_table(bias_off, Tq, Tk, mutant=None):
    """(H, 2T-1) table -> (H, Tq, Tk) by key - q + T - 1.  Mutants: 'bias_off_by_one' (index + 1), 'bias_next_head' (table of head h + 1)."""
    if bias_off is None:
        return None
    assert Tq == Tk
    idx = torch.arange(Tk)[None, :] - torch.arange(Tq)[:, None] + Tk - 1
    if mutant == "bias_off_by_one":
        idx = (idx + 1).clamp(max=2 * Tk - 2)
    if mutant == "bias_next_head":
        bias_off = bias_off.roll(-1, 0)
    return bias_off[:, idx]


def attention_model(q, k, v, bias, dtype=torch.float64, mutant=None):
    """q (N, H, Tq, 64), k / v (N, H, Tk, 64), bias (H, Tq, Tk) or None -> dict(out bf16-rounded, o before that rounding, s, m, e, P, l), every
    sum in `dtype`.  The operations and their order are oracle.ymt3_oracle.attention(bf16=True, round_p=True)'s.  `mutant`: a WRONG kernel, for
    the tests that the criterion has teeth (tests/test_encoder_kernels_cpu.py)."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = q @ k.transpose(-1, -2)
    if bias is not None:
        s = s + bias.to(dtype)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    P = trunc_bf16(e) if mutant == "trunc_p" else O._r(e, True)
    l = (P if mutant == "norm_from_rounded" else e).sum(-1, keepdim=True)
    Tk = k.shape[-2]
    if mutant == "swap_keys":                 # keys 4j and 4j + 1 of one lane's accumulator taken for each other
        v = v[..., torch.arange(Tk) ^ 1, :]
    if mutant == "swap_v16":                  # the two transposed V reads (rows r0 and r0 + 16) taken for each other
        v = v[..., torch.arange(Tk) ^ 16, :]
    o = (P @ v) / l
    out = trunc_bf16(o) if mutant == "trunc_out" else O._r(o, True)
    if mutant == "other_group":               # the 64-query tile of the other wave group
        Tq = q.shape[-2]
        rows = torch.arange(Tq)
        rows = rows ^ 64 if Tq >= 128 else rows
        o, out = o[..., rows, :], out[..., rows, :]
    return dict(out=out, o=o, s=s, m=m, e=e, P=P, l=l)


def attention_beta(q, k, v, bias, parts):
    """beta of the attention output, float64, from the float64 `parts` of attention_model.

    delta_k = 2^-23 (sum_d |q_d k_d| + |bias| + 2 |s_k - max| + 4) bounds the relative error of a device's e_k: the fp32 accumulation of the 64
    exact products and the bias addition move s_k by at most 2^-24 (sum |q k| + |bias|)-ish each way for s_k and for the maximum, the product
    x log2(e) inside __expf rounds |s_k - max| log2(e) once (relative 2^-24 of the exponent: an absolute error of the exponent, a relative one
    of e), and v_exp_f32 is good to 1 ulp; the constant 4 covers those fixed ulps.
    A key is FLIPPABLE when e_k lies within delta_k e_k of a bf16 rounding boundary: a correct device may round its P_k the other way, which
    moves the numerator by ulp_bf16(e_k) |v_kd|.  Every other P_k is the reference's, bit for bit, and P_k v_kd is exact in fp32, so what is
    left is the fp32 accumulation of the P.V sum, the reciprocal of the normaliser, its own accumulation and the final product: together
    under 2^-20 sum_k P_k |v_kd| (sixteen fp32 roundings of a partial sum that never exceeds sum P |v|).
    The NORMALISER sums the unrounded e_k, each with its relative error delta_k, so a correct device's sum(e) lies within sum_k delta_k e_k of
    the reference's and its output moves by |o| sum_k delta_k e_k / sum(e).  (This term is easy to miss and is not small for sharp rows: the
    fp32 oracle on the CPU, a correct implementation, left the bound without it by up to 11 x at q std 4 -- its normaliser was 1e-5 off, its
    numerator 5e-8 -- and meets it with it.)
      beta = (sum over flippable k of ulp_bf16(e_k) |v_kd| + 2^-20 sum_k P_k |v_kd|) / sum(e) + |o| sum_k delta_k e_k / sum(e)"""
    q, k, v = q.double(), k.double(), v.double()
    s, m, e, P, l = parts["s"], parts["m"], parts["e"], parts["P"], parts["l"]
    ab = q.abs() @ k.abs().transpose(-1, -2)
    if bias is not None:
        ab = ab + bias.double().abs()
    delta = 2.0 ** -23 * (ab + 2 * (s - m).abs() + 4)
    flip = rb(e * (1 - delta)) != rb(e * (1 + delta))
    beta = ((flip * ulp_bf16(e)) @ v.abs() + 2.0 ** -20 * (P @ v.abs())) / l + parts["o"].abs() * ((delta * e).sum(-1, keepdim=True) / l)
    return beta, flip


def heads(x):
    """(B, T, H, 64) -> (B, H, T, 64)"""
    return x.transpose(1, 2)


def enc_attention_reference(q, k, v, bias_off, mutant=None, dtype=torch.float64):
    """q, k, v (B, T, H, 64) bf16, bias_off (H, 2T-1) f32 -> (parts with out / o as (B, T, H, 64), beta, flippable (B, H, T, T)); beta and
    flippable only for the float64 reference itself (no mutant)"""
    T = q.shape[1]
    bias = bias_from_table(bias_off, T, T, mutant)
    parts = attention_model(heads(q), heads(k), heads(v), bias, dtype, mutant)
    if dtype != torch.float64 or mutant:
        return {n: heads(parts[n]) for n in ("out", "o")}, None, None
    beta, flip = attention_beta(heads(q), heads(k), heads(v), bias, parts)
    res = dict(parts)
    res["out"], res["o"] = heads(parts["out"]), heads(parts["o"])
    return res, heads(beta), flip


def v_code(B, T, H):
    """V[b, key, h, d] = (3 key + d + 7 h + 11 b) mod 251: integers below 256 are exact in bf16, and a one-hot row returns them exactly"""
    b, t, h, d = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(H), torch.arange(64), indexing="ij")
    return ((3 * t + d + 7 * h + 11 * b) % 251).float().bfloat16()


BIAS_PROBE_H, BIAS_PROBE_B = 16, 2


@functools.lru_cache(maxsize=4)
def _probe_qkv(B, T, H, seed):
    """Q = 0, K random, V = v_code: the same for every launch of a sweep (only the table moves)"""
    g = torch.Generator().manual_seed(seed)
    return torch.zeros(B, T, H, 64).bfloat16(), torch.randn(B, T, H, 64, generator=g).bfloat16(), v_code(B, T, H)


def bias_probe_launches(T):
    return (2 * T - 1 + BIAS_PROBE_H - 1) // BIAS_PROBE_H


def bias_probe_case(T, launch, seed=0):
    """Q = 0, K random, V = v_code; head h's table is 0 at index p_h = (16 launch + h) mod (2T - 1) and -256 elsewhere: every query q with
    0 <= q + p_h - (T - 1) < T returns V[b, q + p_h - (T - 1), h] exactly (exp(-256) is 0 in fp32), the others the mean of V.  Over
    bias_probe_launches(T) launches every table index is the peak once.  Returns q, k, v, bias_off, peak (H,), and per (h, q) the winning
    key or -1."""
    H, B = BIAS_PROBE_H, BIAS_PROBE_B
    q, k, v = _probe_qkv(B, T, H, seed + 1000 * T)
    peak = (BIAS_PROBE_H * launch + torch.arange(H)) % (2 * T - 1)
    bias_off = torch.full((H, 2 * T - 1), -256.0)
    bias_off[torch.arange(H), peak] = 0.0
    key = torch.arange(T)[None, :] + peak[:, None] - (T - 1)
    key = torch.where((key >= 0) & (key < T), key, torch.full_like(key, -1))
    return q, k, v, bias_off, peak, key


SCORE_PROBE_H, SCORE_PROBE_B = 4, 2


def score_probe_case(T):
    """Q[b, q, h] = 16 e_{pi mod 64} with pi = q + d, d = (13 q + 7 h + 3 b) mod 63 - 31 in [-31, 31]; K[key] = 16 e_{key mod 64}; the bias is 0
    for |key - q| < 32 and -1024 beyond.  Inside the window of 63 keys every residue occurs at most once, so if key q + d exists (0 <= q + d < T)
    it alone scores 256 against 0 and wins by 256: P is one-hot and the row returns V[b, q + d, h] exactly.  Rows whose window does not hold
    the key are uniform over the window.  Returns q, k, v, bias_off and the winning key per (b, q, h) or -1."""
    H, B = SCORE_PROBE_H, SCORE_PROBE_B
    b, t, h = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(H), indexing="ij")
    key = t + (13 * t + 7 * h + 3 * b) % 63 - 31
    q = torch.zeros(B, T, H, 64)
    q.scatter_(3, (key % 64)[..., None], 16.0)
    k = torch.zeros(B, T, H, 64)
    k.scatter_(3, (t % 64)[..., None], 16.0)
    off = torch.arange(2 * T - 1) - (T - 1)
    bias_off = torch.where(off.abs() < 32, 0.0, -1024.0)[None].repeat(H, 1).contiguous()
    key = torch.where((key >= 0) & (key < T), key, torch.full_like(key, -1))
    return q.bfloat16(), k.bfloat16(), v_code(B, T, H), bias_off, key


# (q std, bias std): production-like, sharp, uniform (the mean of V) x a mild and a dominating bias
ATTN_REGIMES = [(0.5, 0.5), (0.5, 20.0), (4.0, 0.5), (4.0, 20.0), (0.0, 0.5), (0.0, 20.0)]
ENC_T = [64, 128, 256, 512]


def enc_random_cases():
    """(name, T, B, H, fused, q std, bias std): every T with every regime; B in {1, 3}, H in {1, 8} and the two addressings rotate so that each
    value meets each T and each regime"""
    out = []
    for ti, T in enumerate(ENC_T):
        for ri, (qs, bs) in enumerate(ATTN_REGIMES):
            B, H, fused = (1, 3)[(ti + ri) % 2], (1, 8)[(ti + ri // 2) % 2], (ti // 2 + ri // 3 + ri) % 2 == 0
            out.append((f"T{T}_q{qs:g}_b{bs:g}_B{B}_H{H}_{'fused' if fused else 'separate'}", T, B, H, fused, qs, bs))
    return out


def random_qkv(N, Tq, Tk, H, qs, seed):
    """q of std qs, k and v of std 1.  In the uniform regime (qs = 0) the output is the mean of V, for a zero-mean V a value near 0 with a bf16
    ulp down to 2^-15 while beta stays at 2^-20 mean |v|: at 512 keys 0.935 of the elements are stable.  V gets the mean 0.25 there, which puts
    the outputs in one binade (ulp 2^-9) without making any key's V irrelevant."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(N, Tq, H, 64, generator=g) * qs).bfloat16()
    k = torch.randn(N, Tk, H, 64, generator=g).bfloat16()
    v = (torch.randn(N, Tk, H, 64, generator=g) + (0.25 if qs == 0 else 0.0)).bfloat16()
    return q, k, v, g


def enc_random_case(T, B, H, qs, bs, seed=0):
    q, k, v, g = random_qkv(B, T, T, H, qs, seed + T + 7 * B + 13 * H + int(100 * qs) + int(10 * bs))
    return q, k, v, (torch.randn(H, 2 * T - 1, generator=g) * bs).contiguous()


# sequence attention: (Tq, Tk, with a bias)
SEQ_SHAPES = [(32, 32, True), (64, 64, True), (128, 128, True), (256, 256, True), (16, 32, False), (48, 64, False), (32, 128, False), (32, 256, False)]
SEQ_H = 2


def seq_layouts(n_seq, inner_n, Tq, Tk, H=SEQ_H):
    """Two placements of n_seq sequences, as element strides (outer, inner, step) for q, k/v and out plus the buffers' sizes and the offsets of
    q, k, v in theirs:
      'temporal'  the temporal transformer's: one fused qkv row of 3 H 64 per (position, inner index), positions inner_n rows apart (needs
                  Tq == Tk; k and v live in q's buffer at + H 64 and + 2 H 64)
      'padded'    separate q / kv / out buffers, rows wider than the heads need (gaps nobody may touch), inner-major: the sequences of one outer
                  index lie one whole sequence apart"""
    D = H * 64
    n_outer = (n_seq + inner_n - 1) // inner_n
    lay = {}
    if Tq == Tk:
        row = 3 * D
        lay["temporal"] = dict(q=(Tq * inner_n * row, row, inner_n * row), kv=(Tq * inner_n * row, row, inner_n * row),
                               o=(Tq * inner_n * D, D, inner_n * D), q_size=n_outer * Tq * inner_n * row, kv_size=0, k_at=D, v_at=2 * D,
                               o_size=n_outer * Tq * inner_n * D)
    qr, kr, orow = D + 8, 2 * D + 16, D + 24
    lay["padded"] = dict(q=(inner_n * Tq * qr + 64, Tq * qr, qr), kv=(inner_n * Tk * kr + 32, Tk * kr, kr), o=(inner_n * Tq * orow + 8, Tq * orow, orow),
                         q_size=n_outer * (inner_n * Tq * qr + 64), kv_size=n_outer * (inner_n * Tk * kr + 32), k_at=0, v_at=D + 8,
                         o_size=n_outer * (inner_n * Tq * orow + 8))
    return lay


def seq_cases():
    """(name, Tq, Tk, with_bias, n_seq, inner_n, layout, q std, bias std): every shape with n_seq in {1, 5} and inner_n in {1, 3}; the layout
    alternates where the shape allows both, the regimes rotate"""
    out, i = [], 0
    for Tq, Tk, wb in SEQ_SHAPES:
        for n_seq in (1, 5):
            for inner_n in (1, 3):
                layout = "temporal" if Tq == Tk and (i // 2 + i + i // 4) % 2 else "padded"
                qs, bs = ATTN_REGIMES[i % len(ATTN_REGIMES)]
                out.append((f"Tq{Tq}_Tk{Tk}_{'bias' if wb else 'nobias'}_n{n_seq}_in{inner_n}_{layout}_q{qs:g}_b{bs:g}", Tq, Tk, wb, n_seq, inner_n, layout, qs, bs))
                i += 1
    return out


def uniform_row(v):
    """(o, beta) of a row whose scores are all EQUAL, from v (N, T, H, 64) >= 0 alone: every e is exp(0) = 1 exactly, no key is flippable, and
    attention_beta's remaining terms are 2^-20 mean |v| + |o| 2^-23 (|bias| + 4) with q = 0; |bias| <= 256 in the probes that use this."""
    o = v.double().mean(1)
    return o, 2.0 ** -20 * o + o * 2.0 ** -23 * 260


def seq_starts(n_seq, inner_n, st):
    s = torch.arange(n_seq)
    return (s // inner_n) * st[0] + (s % inner_n) * st[1]


def seq_random_case(Tq, Tk, with_bias, n_seq, qs, bs, seed=0):
    q, k, v, g = random_qkv(n_seq, Tq, Tk, SEQ_H, qs, seed + 3 * Tq + 5 * Tk + 11 * n_seq + int(100 * qs) + int(10 * bs))
    return q, k, v, ((torch.randn(SEQ_H, 2 * Tk - 1, generator=g) * bs).contiguous() if with_bias else None)


def seq_attention_reference(q, k, v, bias_off, mutant=None, dtype=torch.float64):
    """q (N, Tq, H, 64), k / v (N, Tk, H, 64), bias_off (H, 2 Tk - 1) or None: as enc_attention_reference"""
    Tq, Tk = q.shape[1], k.shape[1]
    bias = bias_from_table(bias_off, Tq, Tk, mutant)
    parts = attention_model(heads(q), heads(k), heads(v), bias, dtype, mutant)
    if dtype != torch.float64 or mutant:
        return {n: heads(parts[n]) for n in ("out", "o")}, None, None
    beta, flip = attention_beta(heads(q), heads(k), heads(v), bias, parts)
    res = dict(parts)
    res["out"], res["o"] = heads(parts["out"]), heads(parts["o"])
    return res, heads(beta), flip


SEQ_PROBE_H = 8


def seq_bias_probe_case(T, n_seq, launch, H=SEQ_PROBE_H):
    """bias_probe_case for the sequence kernel: ceil((2T - 1) / H) launches cover every table index"""
    q, k, v = _probe_qkv(n_seq, T, H, 77 + 1000 * T)
    peak = (H * launch + torch.arange(H)) % (2 * T - 1)
    bias_off = torch.full((H, 2 * T - 1), -256.0)
    bias_off[torch.arange(H), peak] = 0.0
    key = torch.arange(T)[None, :] + peak[:, None] - (T - 1)
    key = torch.where((key >= 0) & (key < T), key, torch.full_like(key, -1))
    return q, k, v, bias_off, peak, key


def seq_score_probe_case(Tq, Tk, n_seq, with_bias):
    """The score probe for the sequence kernel.  With a bias (Tq == Tk): score_probe_case's construction (window of 63 keys).  Without one there
    is no window and up to 256 keys must differ in 64 coordinates: K[key] = 16 e_{key mod 48} + 16 e_{48 + key / 48} has TWO hot coordinates
    from disjoint ranges and Q[q] those of key (29 q + 7 h + 3 n + 5) mod Tk: that key scores 512, a key sharing one coordinate 256, the
    rest 0, so it wins by 256 and every row is one-hot."""
    H = SEQ_H
    n, t, h = torch.meshgrid(torch.arange(n_seq), torch.arange(Tq), torch.arange(H), indexing="ij")
    if with_bias:
        w = min(31, Tk // 4)                                    # short sequences: a narrower spread of winners, so that most exist
        key = t + (13 * t + 7 * h + 3 * n) % (2 * w + 1) - w
        q = torch.zeros(n_seq, Tq, H, 64).scatter_(3, (key % 64)[..., None], 16.0)
        kk = torch.arange(Tk)[None, :, None].expand(n_seq, Tk, H)
        k = torch.zeros(n_seq, Tk, H, 64).scatter_(3, (kk % 64)[..., None], 16.0)
        off = torch.arange(2 * Tk - 1) - (Tk - 1)
        bias_off = torch.where(off.abs() < 32, 0.0, -1024.0)[None].repeat(H, 1).contiguous()
        key = torch.where((key >= 0) & (key < Tk), key, torch.full_like(key, -1))
    else:
        key = (29 * t + 7 * h + 3 * n + 5) % Tk
        q = torch.zeros(n_seq, Tq, H, 64).scatter_(3, (key % 48)[..., None], 16.0).scatter_(3, (48 + key // 48)[..., None], 16.0)
        kk = torch.arange(Tk)[None, :, None].expand(n_seq, Tk, H)
        k = torch.zeros(n_seq, Tk, H, 64).scatter_(3, (kk % 48)[..., None], 16.0).scatter_(3, (48 + kk // 48)[..., None], 16.0)
        bias_off = None
    return q.bfloat16(), k.bfloat16(), v_code(n_seq, Tk, H), bias_off, key


# ----------------------------------------------------------------------------- rmsnorm / spec_embed
def rmsnorm_model(x, gain, eps, dtype=torch.float64, mutant=None):
    """x (M, d) fp32 values, gain (d,): (out bf16-rounded, o before that rounding), as oracle.ymt3_oracle.rmsnorm.  Mutants: 'mean_subtracted'
    (a LayerNorm), 'eps_outside' (x / (sqrt(mean x^2) + eps))."""
    x, gain = x.to(dtype), gain.to(dtype)
    if mutant == "mean_subtracted":
        x = x - x.mean(-1, keepdim=True)
    if mutant == "eps_outside":
        o = x / (x.pow(2).mean(-1, keepdim=True).sqrt() + eps) * gain
    else:
        o = O.rmsnorm(x, gain, eps)
    return O._r(o, True), o


def rmsnorm_beta(o, d):
    """(d / 64 + 8) 2^-24 relative: each lane sums d / 64 squares (a rounding per square and per addition, all positive: relative errors do not
    amplify), six butterfly additions, the division by d and the addition of eps, halved by the root (together under d / 64 + 4 roundings of the
    mean square, i.e. half as many of the scale), v_rsq_f32 at 1 ulp, and the two products x scale gain."""
    return (d / 64 + 8) * 2.0 ** -24 * o.double().abs()


def spec_embed_input(mel, w, pos, F):
    """the fp32 values the kernel norms: f32(f32(mel[row] w) + pos[row % F]) -- mul, then add, two roundings (no fma)"""
    rows = torch.arange(mel.shape[0]) % F
    return (mel.float()[:, None] * w.float()[None, :]) + pos.float()[rows]


RMS_D = [128, 132, 256, 512]
RMS_M = [1, 3, 4, 5, 4095, 4096, 4097, 4127]


def rmsnorm_case(M, d, seed=0):
    """random rows of mixed scale, and a gain with negative and zero entries"""
    g = torch.Generator().manual_seed(seed + 31 * M + d)
    x = torch.randn(M, d, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())
    gain = torch.randn(d, generator=g)
    gain[3::17] = 0.0
    gain[5::19] = -gain[5::19].abs()
    return x, gain


def rmsnorm_value_rows(d, seed=0):
    """rows 0.. : zeros, all 1e18 (the sum of d squares of 1e36 overflows fp32 from d = 512 on), all 1e-20 (x^2 is an fp32 subnormal), one 1e18 among
    ones, random, a NaN, all 3e19 (every square overflows), random.  Second result: the rows whose sum of squares exceeds the fp32 range in ANY
    summation order (decided in float64): there the contract is the fp32 oracle's, a scale of rsqrt(inf) = 0."""
    g = torch.Generator().manual_seed(seed + d)
    x = torch.randn(8, d, generator=g)
    x[0] = 0.0
    x[1] = 1e18
    x[2] = 1e-20
    x[3] = 1.0
    x[3, d // 2] = 1e18
    x[5, 7] = float("nan")
    x[6] = 3e19
    over = x.float().double().pow(2).sum(-1) > torch.finfo(torch.float32).max
    return x, {"zero": 0, "huge": 1, "tiny": 2, "one_huge": 3, "nan": 5, "overflow": torch.nonzero(over).flatten()}


# ----------------------------------------------------------------------------- GEMM epilogues
GEMM_SMALL = [(1, 128, 64), (129, 128, 128), (200, 256, 512)]
GEMM_BIG = [(4224, 1024, 512), (4100, 1024, 192)]           # tests/test_gpu_parity.py::test_pipelined_large_m_gemm: these take the 256 x 128 kernel


def gemm_case(M, N, K, seed=0):
    """A = |randn|, row n of W = sign_n |randn| / K: sign-coherent rows, so the result is +-sum |a||w| and the any-order bound K 2^-24 sum |a||w| is
    K 2^-24 RELATIVE (2^-15 at K = 512 against a bf16 ulp of 2^-8: 0.98 stable).  With plain randn operands the same bound is 15 % of a bf16 ulp
    of the result at K = 512 and only 0.85 of the elements are stable; cancelling operands have their own test (test_gemm_operand_values).
    Half the rows of W are negative: EPI_BF16_RELU clamps half the columns."""
    g = torch.Generator().manual_seed(seed + M + N + K)
    A = torch.randn(M, K, generator=g).abs().bfloat16()
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    W = (torch.randn(N, K, generator=g).abs() * sign[:, None] / K).bfloat16()
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g) * 4
    return A, W, bias, resid


def headmajor(x, T, H, mutant=None):
    """(M, N) -> [N / (H 64)][M / T][H][T][64] (GemmEpilogue EPI_KV_HEADMAJOR); mutant 'swap_h_slab': head and slab indices taken for each other"""
    M, N = x.shape
    slabs = N // (H * 64)
    y = x.reshape(M // T, T, slabs, H, 64)
    if mutant == "swap_h_slab":               # offset (((h n_seg + seg) slabs + slab) T + t) 64 + d
        return y.permute(3, 0, 2, 1, 4).contiguous().reshape(slabs, M // T, H, T, 64)
    return y.permute(2, 0, 3, 1, 4).contiguous()


def gemm_epilogue_reference(epi, A, W, bias=None, resid=None, T=0, H=0, mutant=None):
    """(o, beta): the float64 value before the epilogue's final rounding and its bound.  beta is gemm_reference_and_bound's K 2^-24 sum |a||w|
    (any fp32 summation order); + 2^-24 |result| for the one extra fp32 addition of EPI_F32's bias and of EPI_RESID's residual.  For
    EPI_BF16_RELU o is NOT clamped: check_bf16(relu=True) clamps and admits 0 where |o| <= beta."""
    ref, bound = gemm_reference_and_bound(A, W)
    if epi == EPI_F32:
        if bias is not None:
            ref = ref + bias.double()[None, :]
            bound = bound + 2.0 ** -24 * ref.abs()
    elif epi == EPI_RESID:
        ref = ref if mutant == "resid_overwrites" else ref + resid.double()
        bound = bound + 2.0 ** -24 * ref.abs()
    elif epi == EPI_KV_HEADMAJOR:
        ref, bound = headmajor(ref, T, H, mutant), headmajor(bound, T, H)
    return ref, bound


def permutation_probe(M, N, K):
    """tests/test_gpu_parity.py's probe: row i of A selects column (7 i) mod K of W, whose entries (3 n + k) mod 251 are bf16-exact: the
    product is W[:, 7 i mod K]^T exactly, in any summation order"""
    P = torch.zeros(M, K).bfloat16()
    sel = (torch.arange(M) * 7) % K
    P[torch.arange(M), sel] = 1
    Wp = (torch.arange(N)[:, None] * 3 + torch.arange(K)[None, :]).float().remainder(251).bfloat16()
    return P, Wp, Wp.float()[:, sel].T.contiguous()
