"""References, criteria and inputs for the per-kernel tests of the full-sequence scoring pass (csrc/dec_seq.hip: seq_embed_kernel,
dec_seq_attn_kernel<CAUSAL>, seq_lm_head_score_kernel; tests/test_seq_kernels.py on the GPU, tests/test_seq_kernels_cpu.py for the model itself).
TEST INFRASTRUCTURE ONLY, CPU only.  The criterion and its helpers are tests/enc_kernel_model.py's.

Contracts, float64 with the kernels' rounding points (R = round to nearest-even bf16):

  embed      position 0 feeds pad_id, 1 .. P the prompt, P + j + 1 tokens[j]; ids clamped into [0, V); the row is f32(embed[id]) (+
             f32(chan_embed[absolute row % n_channels])): one fp32 addition of two bf16 values.  Bit for bit.
  attention  THE TILE SCHEDULE.  Keys go through in tiles of 64 from key 0.  m_t = max(m_{t-1}, scores of the tile's unmasked keys);
             P = R(exp(s - m_t)); sum = sum exp(m_{t-1} - m_t) + sum_tile exp(s - m_t) (the UNROUNDED e); num = num exp(m_{t-1} - m_t) + P.V;
             out = R(num / sum).  Causal: s = q.k + bias[h][query - key] for key <= query, tiles beyond the query's are not visited; cross:
             s = q.k over n_keys keys.  No 1/sqrt(d).  oracle.attention(round_p=True) rounds exp(s - GLOBAL max): the same arithmetic for at
             most 64 keys, another one beyond (P is rounded on another grid whenever a later tile raises the maximum).
  lm head    logits = xn . W^T in fp32; score = logit[target clamped into [0, V)] - log sum exp(logits); exactly 0.0 for j >= lengths[row]
             clamped into [0, n_steps]; prompt positions and rows >= M write nothing.
"""
from __future__ import annotations

import functools
import math

import torch

import enc_kernel_model as K
from enc_kernel_model import MIN_STABLE, check_bf16, check_f32, judge_bf16, rb, trunc_bf16, ulp_bf16  # noqa: F401
from value_regimes import gemm_reference_and_bound

SENT = 12352.0
KT, QB = 64, 128
NEG0 = -3.0e38                       # the kernel's initial running maximum


# ============================================================================= embed
EMBED_MUTANTS = ["embed_no_shift", "embed_prompt_off_by_one", "embed_unclamped", "embed_channel_local_row"]


def embed_case(n_rows, L_steps, P, row0, n_channels, V=96, seed=0, chan=True):
    """random bf16 tables; ids with out-of-range entries (negative, >= V) in tokens and prompt; tables of rows below row0 hold other ids"""
    g = torch.Generator().manual_seed(seed + 7 * n_rows + 11 * L_steps + 13 * P + 17 * row0)
    rows = row0 + n_rows
    tokens = torch.randint(0, V, (rows, L_steps), generator=g, dtype=torch.int32)
    prompt = torch.randint(0, V, (rows, max(P, 1)), generator=g, dtype=torch.int32)
    tokens[row0:, ::3] = torch.tensor([-5, V, V + 40000, -1])[torch.arange(tokens[row0:, ::3].numel()) % 4].reshape(tokens[row0:, ::3].shape).int()
    if P:
        prompt[row0, 0], prompt[rows - 1, P - 1] = -2, V + 3
    return dict(n_rows=n_rows, n_steps=L_steps, P=P, L=P + L_steps, row0=row0, V=V, n_channels=n_channels, pad_id=V - 2,
                embed=torch.randn(V, 512, generator=g).bfloat16(), chan_embed=torch.randn(n_channels, 512, generator=g).bfloat16() if chan else None,
                tokens=tokens, prompt=prompt if P else None)


def embed_reference(c, mutant=None, dtype=torch.float32):
    """-> (n_rows * L, 512) fp32, exact (`dtype` float64: the same sum without the fp32 rounding, for the chained float64 comparison)"""
    P, L, V, row0 = c["P"], c["L"], c["V"], c["row0"]
    out = torch.empty(c["n_rows"], L, 512, dtype=dtype)
    for lr in range(c["n_rows"]):
        r = row0 + lr
        for pos in range(L):
            if pos == 0:
                i = c["pad_id"]
            elif pos <= P:
                i = int(c["prompt"][r, min(pos, P - 1) if mutant == "embed_prompt_off_by_one" else pos - 1])
            else:
                i = int(c["tokens"][r, min(pos - P, c["n_steps"] - 1) if mutant == "embed_no_shift" else pos - P - 1])
            i = i % V if mutant == "embed_unclamped" else min(max(i, 0), V - 1)
            row = c["embed"][i].to(dtype)
            if c["chan_embed"] is not None:
                row = row + c["chan_embed"][(lr if mutant == "embed_channel_local_row" else r) % c["n_channels"]].to(dtype)
            out[lr, pos] = row
    return out.reshape(-1, 512)


EMBED_CASES = [(1, 1, 0, 0, 1), (3, 1, 0, 2, 3), (1, 3, 1, 5, 2), (2, 2, 0, 1, 3), (1, 2, 3, 4, 5), (5, 7, 4, 3, 3)]   # n_rows, n_steps, P, row0, K


def check_embed(c, got):
    ref = embed_reference(c)
    return dict(elements=int(ref.numel()), ok=bool(torch.equal(got.reshape(ref.shape).view(torch.int32), ref.view(torch.int32))))


# ============================================================================= attention
ATTN_MUTANTS = ["bias_by_key", "bias_off_by_one", "bias_next_head", "bias_next_tile_window", "diag_lt", "wave_skips_diagonal", "keys_beyond_n_keys",
                "no_rescale", "rescale_num_only", "p_global_max", "norm_from_rounded", "trunc_p", "trunc_out", "rows_per_kv_ignored", "row0_ignored",
                "kv_next_head", "swap_v16"]


def slab_of_row(c, mutant=None):
    r = torch.arange(c["q"].shape[0])
    if mutant == "rows_per_kv_ignored":
        return (c["row0"] + r).clamp(max=c["k"].shape[0] - 1)
    if mutant == "row0_ignored":
        return r // c["rows_per_kv"]
    return (c["row0"] + r) // c["rows_per_kv"]


def attention_tiles(q, k, v, bias, causal, dtype=torch.float64, mutant=None, rounding=True):
    """q (N, H, Tq, 64), k / v (N, H, Tk, 64), bias (H, stride) f32 by distance or None -> parts of the tile schedule (module docstring), every sum
    in `dtype`: out, o, and per (query, key) s, mt (the running maximum its P was rounded against), et = exp(s - mt), P, carry = exp(mt - final
    maximum); per query l (the normaliser in the final scale), mfin, n_tiles."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    Tq, Tk = q.shape[-2], k.shape[-2]
    if mutant == "kv_next_head":
        k, v = k.roll(-1, 1), v.roll(-1, 1)
    if mutant == "keys_beyond_n_keys" and Tk % KT:                        # the zero rows of the LDS tile let in: score 0, value 0
        pad = KT - Tk % KT
        k = torch.cat([k, torch.zeros_like(k[..., :pad, :])], -2)
        v = torch.cat([v, torch.zeros_like(v[..., :pad, :])], -2)
        Tk += pad
    s = q @ k.transpose(-1, -2)
    qi, ki = torch.arange(Tq)[:, None], torch.arange(Tk)[None, :]
    if causal:
        idx = qi - ki
        if mutant == "bias_by_key":
            idx = ki.expand(Tq, Tk)
        elif mutant == "bias_off_by_one":
            idx = idx + 1
        elif mutant == "bias_next_tile_window":
            idx = idx - KT
        b = bias.roll(-1, 0) if mutant == "bias_next_head" else bias
        s = s + b.to(dtype)[:, idx.clamp(0, bias.shape[1] - 1)]
        mask = ki < qi if mutant == "diag_lt" else ki <= qi
        if mutant == "wave_skips_diagonal":                               # a tile taken only when it lies wholly at or below the wave's last query
            mask = mask & (ki < ((qi // 16) * 16 + 16) // KT * KT)
        s = s.masked_fill(~mask, float("-inf"))
    n_t = (Tk + KT - 1) // KT
    m = torch.full(s.shape[:-1] + (1,), NEG0, dtype=dtype)
    num = torch.zeros(q.shape, dtype=dtype)
    l = torch.zeros_like(m)
    mt, P = torch.empty_like(s), torch.empty_like(s)
    for t in range(n_t):
        sl = slice(t * KT, min((t + 1) * KT, Tk))
        mn = torch.maximum(m, s[..., sl].max(-1, keepdim=True).values)
        alpha = torch.ones_like(m) if mutant == "no_rescale" else torch.exp(m - mn)
        e = torch.exp(s[..., sl] - mn)
        p = e if not rounding else (trunc_bf16(e) if mutant == "trunc_p" else rb(e))
        vt = v[..., sl, :]
        if mutant == "swap_v16":
            vt = vt[..., (torch.arange(vt.shape[-2]) ^ 16).clamp(max=vt.shape[-2] - 1), :]
        num = num * alpha + p @ vt
        l = l * (1.0 if mutant == "rescale_num_only" else alpha) + (p if mutant == "norm_from_rounded" else e).sum(-1, keepdim=True)
        mt[..., sl], P[..., sl] = mn, p
        m = mn
    if mutant == "p_global_max":                                          # oracle.attention(round_p=True) / enc_kernel_model.attention_model
        e = torch.exp(s - m)
        P, mt = rb(e), m.expand_as(s).clone()
        num, l = P @ v, e.sum(-1, keepdim=True)
    o = num / l
    out = o if not rounding else (trunc_bf16(o) if mutant == "trunc_out" else rb(o))
    n_tiles = (torch.arange(Tq) // KT + 1 if causal else torch.full((Tq,), n_t))
    return dict(out=out, o=o, s=s, mt=mt, et=torch.exp(s - mt), P=P, carry=torch.exp(mt - m), l=l, mfin=m, n_tiles=n_tiles, v=v)


def attention_beta(q, k, v, bias, causal, parts, any_order=False):
    """beta of the tile schedule's output, float64, term by term (the encoder's and the step kernels' derivations are
    sections 23 and 24).  Per key k of tile t, n = the query's tile count, everything in the FINAL scale (e_k = exp(s_k - m_final)):

      delta_k = 2^-23 (sum_d |q_d k_d| + |bias| + 2 |s_k - m_t| + |m_t - m_final| + 2 n + 4)    relative error of a device's e_k IN THE NORMALISER:
                the fp32 accumulation of the exact products and the bias addition (both for s_k and for the maximum), the subtraction and the
                product with log2(e) inside __expf (each rounds the exponent by 2^-24 |s_k - m_t|), v_exp_f32 at 1 ulp and the fixed ulps (4); every
                later tile multiplies by alpha = __expf(m_old - m_new): its exponent is rounded the same way, and the exponents along the path sum
                to m_t - m_final; one ulp of v_exp_f32 and the two roundings of sum * alpha + part per tile (2 n).
      flip      a key is flippable when exp(s_k - m_t) (1 +- d) rounds two ways, d = delta_k without the two carry terms (the rounding happens in
                tile t): a correct device may round P_k the other way, ulp_bf16(exp(s_k - m_t)) |v|, carried forward by exp(m_t - m_final).
      gamma_k = 2^-23 (|m_t - m_final| + n - 1 - t) + [m_t != m_final] (E(m_t) + E(m_final))    what the later tiles' alphas do to the NUMERATOR's
                contribution of key k: the exponent roundings again and one v_exp_f32 ulp per later tile (their multiplications are counted in
                c), and THE CARRIED MAXIMA'S OWN ERRORS.  E(j) = 3 2^-24 (sum_d |q_d k_jd| + |bias_j|) bounds a device's score j: two MFMA
                accumulations and the bias addition each round a partial sum no larger than that.  Within a tile such an error reaches P only
                through the bf16 rounding (the flips); across tiles the weight of an earlier tile's keys against a later one's is
                exp(m_t - m_final), a product of fp32 alphas that is never rounded to bf16, so the errors of the two scores that hold the
                maxima arrive whole (the maxima between them cancel: each enters one alpha as m_new and the next as m_old).  E(m_final) does
                NOT cancel between numerator and normaliser: the keys of the tile that holds the final maximum enter the numerator as
                P = R(exp(s - m_final)), pinned by the bf16 rounding (the maximum itself as exactly 1), not scaled by the device's error in
                m_final, while every earlier tile's share is; with two dominant keys a (earlier tile) and b (final maximum) the output is
                (w v_a + v_b) / (w + 1), w = exp(s_a - s_b), and an error in s_b moves w as much as one in s_a.  With the global
                maximum this path does not exist, which is why section 23's beta has no such term.  It was found on the device: three
                random cases of the sharp regime (q std 4) left the beta without it by up to 4 x, every one in a row whose two dominant
                keys lie in different tiles, |o| << |v|.
      c         the depth of the kernel's partition, 3 n + 4: per tile two MFMA accumulations and the product with alpha; the reciprocal, the
                product with it and the two lane merges of the sum.  any_order: n_keys + 2 n + 4, for an implementation that adds in another order.

      beta = (flip term + sum gamma_k P_k |v| + c 2^-24 sum P_k |v|) / sum(e) + |o| (sum delta_k e_k / sum(e) + c 2^-24 + 2^-23)"""
    q, k = q.double(), k.double()
    v = parts["v"]
    s, mt, et, P, carry, l, mfin = (parts[n] for n in ("s", "mt", "et", "P", "carry", "l", "mfin"))
    Tq, Tk = s.shape[-2], s.shape[-1]
    ab = q.abs() @ k.abs().transpose(-1, -2)
    if causal:
        idx = (torch.arange(Tq)[:, None] - torch.arange(Tk)[None, :]).clamp(0, bias.shape[1] - 1)
        ab = ab + bias.double().abs()[:, idx]
    live = torch.isfinite(s)
    z = torch.zeros_like(s)
    gap_t, gap_f = torch.where(live, (s - mt).abs(), z), (mt - mfin).abs()
    n = parts["n_tiles"].double()[:, None]
    tile = (torch.arange(Tk) // KT).double()[None, :]
    d_tile = 2.0 ** -23 * (ab + 2 * gap_t + 4)
    delta = d_tile + 2.0 ** -23 * (gap_f + 2 * n)
    gamma = 2.0 ** -23 * (gap_f + (n - 1 - tile).clamp(min=0))
    # the carried maxima: E of the score that holds the running maximum after each tile, and of the final one
    E = 3 * 2.0 ** -24 * ab
    run_m = torch.full(s.shape[:-1] + (1,), NEG0, dtype=s.dtype)
    run_E = torch.zeros_like(run_m)
    E_mt = torch.zeros_like(s)
    for t in range((Tk + KT - 1) // KT):
        sl = slice(t * KT, min((t + 1) * KT, Tk))
        tm, ti = s[..., sl].max(-1, keepdim=True)
        up = tm > run_m
        run_E = torch.where(up, E[..., sl].gather(-1, ti), run_E)
        run_m = torch.where(up, tm, run_m)
        E_mt[..., sl] = run_E
    gamma = gamma + torch.where(mt != mfin, E_mt + run_E, z)
    flip = live & (rb(et * (1 - d_tile)) != rb(et * (1 + d_tile)))
    e, Pf = et * carry, P * carry
    c = (Tk + 2 * n + 4 if any_order else 3 * n + 4)
    va = v.abs()
    beta = ((flip * ulp_bf16(et) * carry + gamma * Pf) @ va + c * 2.0 ** -24 * (Pf @ va)) / l \
        + parts["o"].abs() * ((delta * e).sum(-1, keepdim=True) / l + c * 2.0 ** -24 + 2.0 ** -23)
    return beta, flip


def attention_reference(c, mutant=None, dtype=torch.float64, rounding=True):
    """case -> (parts with out / o as (n_rows, L, H, 64), beta or None)"""
    idx = slab_of_row(c, mutant)
    qh, kh, vh = K.heads(c["q"]), K.heads(c["k"][idx]), K.heads(c["v"][idx])
    parts = attention_tiles(qh, kh, vh, c["bias"], c["causal"], dtype, mutant, rounding)
    beta = None
    if dtype == torch.float64 and mutant is None and rounding:
        beta = K.heads(attention_beta(qh, kh, vh, c["bias"], c["causal"], parts)[0])
    res = dict(parts)
    res["out"], res["o"] = K.heads(parts["out"]), K.heads(parts["o"])
    return res, beta


def attention_beta_any_order(c, parts_heads):
    idx = slab_of_row(c)
    return K.heads(attention_beta(K.heads(c["q"]), K.heads(c["k"][idx]), K.heads(c["v"][idx]), c["bias"], c["causal"], parts_heads, any_order=True)[0])


def _kv_slabs(n_slabs, first, n_keys, H, g, mean=0.0):
    """slabs below `first` hold NaN: nothing may read them"""
    k = torch.randn(n_slabs, n_keys, H, 64, generator=g).bfloat16()
    v = (torch.randn(n_slabs, n_keys, H, 64, generator=g) + mean).bfloat16()
    k[:first], v[:first] = float("nan"), float("nan")
    return k, v


# (name, causal, L, n_keys, n_rows, H, row0, rows_per_kv, layout, q std, bias std)
def attn_random_cases():
    """every one of the six regimes at every size of the score probe: causal L in {1, 2, 63, 64, 65, 127, 128, 129, 160, 1024} and cross n_keys in
    {1, 63, 64, 65, 128, 512} (96 cases); rows, heads, row0, rows_per_kv and the two layouts rotate through them"""
    out, i = [], 0

    def add(causal, L, nk, qs, bs):
        nonlocal i
        big = max(L, nk) >= 512
        n_rows, H = (1, 2) if big else ((2, 3)[i % 2], (1, 2)[(i // 2) % 2])
        rpk = 1 if causal else (1, 3, 13)[i % 3]
        row0 = (0, 2)[i % 2] if rpk == 1 else rpk - 1                     # a slab boundary inside the launch when n_rows > 1
        layout = ("fused", "headmajor")[(i + i // 3) % 2] if rpk == 1 else "headmajor"
        out.append((f"{'causal' if causal else 'cross'}_L{L}_k{nk}_q{qs:g}_b{bs:g}_R{n_rows}_H{H}_row{row0}_rpk{rpk}_{layout}", causal, L, nk, n_rows, H, row0,
                    rpk, layout, qs, bs))
        i += 1

    for L in (160, 1024):
        for qs, bs in K.ATTN_REGIMES:
            add(True, L, L, qs, bs)
    for nk in (64, 512):
        for qs, bs in K.ATTN_REGIMES:
            add(False, (40, 130)[nk == 512], nk, qs, bs)
    for L in (1, 2, 63, 64, 65, 127, 128, 129):
        for qs, bs in K.ATTN_REGIMES:
            add(True, L, L, qs, bs)
    for nk, L in ((1, 17), (63, 129), (65, 17), (128, 129)):
        for qs, bs in K.ATTN_REGIMES:
            add(False, L, nk, qs, bs)
    return out


def find_random_case(**want):
    """the first random case whose fields (causal, L, n_keys, n_rows, H, row0, rpk, layout, qs, bs) equal `want`; n_rows / H: at least"""
    names = ("name", "causal", "L", "n_keys", "n_rows", "H", "row0", "rpk", "layout", "qs", "bs")
    for case in attn_random_cases():
        f = dict(zip(names, case))
        if all(f[k] >= v if k in ("n_rows", "H") else f[k] == v for k, v in want.items()):
            return case[0]
    raise KeyError(want)


@functools.lru_cache(maxsize=None)
def attn_random_case(name):
    _, causal, L, nk, n_rows, H, row0, rpk, layout, qs, bs = next(x for x in attn_random_cases() if x[0] == name)
    g = torch.Generator().manual_seed(int(causal) + 2 * L + 2051 * nk + 7 * n_rows + 13 * H + 17 * row0 + 19 * rpk + int(100 * qs) + int(10 * bs))
    n_slabs = (row0 + n_rows - 1) // rpk + 1
    q = (torch.randn(n_rows, L, H, 64, generator=g) * qs).bfloat16()
    k, v = _kv_slabs(n_slabs, row0 // rpk, nk, H, g, mean=0.25 if qs == 0 else 0.0)
    stride = L + (0, 5)[L % 2]
    bias = (torch.randn(H, stride, generator=g) * bs).contiguous() if causal else None
    return dict(causal=causal, q=q, k=k, v=v, bias=bias, row0=row0, rows_per_kv=rpk, layout=layout)


@functools.lru_cache(maxsize=None)
def attn_random_reference(name):
    return attention_reference(attn_random_case(name))


def check_attention(c, got, ref=None):
    """got (n_rows, L, H, 64) bf16 -> the criterion's figures against the tile-schedule reference"""
    ref, beta = ref if ref is not None else attention_reference(c)
    return check_bf16(got, ref["o"], beta)


def v_code(n_slabs, n_keys, H):
    """integer codes of (key, dim, head, slab) below 251: exact in bf16.  INJECTIVE in (slab, key, head) for key < 1255, head < 251, slab < 6:
    the four groups of 16 dims hold (a mix of all three), key / 5, 37 head and 41 slab + key mod 5, each + d modulo 251, so no other row of
    the probe's V is bit-equal to the one a row must return (tests/test_seq_kernels_cpu.py asserts it at the probes' sizes)"""
    assert n_keys <= 1255 and H <= 251 and n_slabs <= 6
    b, t, h, d = torch.meshgrid(torch.arange(n_slabs), torch.arange(n_keys), torch.arange(H), torch.arange(64), indexing="ij")
    base = torch.stack([3 * t + 7 * h + 11 * b, t // 5, 37 * h, 41 * b + t % 5], -1).gather(-1, (d // 16)[..., None])[..., 0]
    return ((base + d) % 251).float().bfloat16()


# ----------------------------------------------------------------------------- bias probe
BIAS_PROBE_L, BIAS_PROBE_H = 1024, 64


@functools.lru_cache(maxsize=2)
def bias_probe_qkv(L=BIAS_PROBE_L, H=BIAS_PROBE_H):
    g = torch.Generator().manual_seed(5)
    return torch.zeros(1, L, H, 64).bfloat16(), torch.randn(1, L, H, 64, generator=g).bfloat16(), v_code(1, L, H)


def bias_probe_case(launch, L=BIAS_PROBE_L, H=BIAS_PROBE_H):
    """q = 0; head h's table is 0 at distance d_h = (H launch + h) mod L and -256 elsewhere: the row at position t >= d_h returns V[t - d_h] bit for
    bit (exp(-256) is 0 in fp32, and the alpha of the tile that brings the peak wipes what the tiles before it gathered); rows t < d_h are
    uniform over their t + 1 keys.  L / H launches make every distance the lone peak once."""
    q, k, v = bias_probe_qkv(L, H)
    peak = (H * launch + torch.arange(H)) % L
    bias = torch.full((H, L), -256.0)
    bias[torch.arange(H), peak] = 0.0
    key = torch.arange(L)[:, None] - peak[None, :]                        # (L, H)
    return dict(causal=True, q=q, k=k, v=v, bias=bias, row0=0, rows_per_kv=1, layout="fused"), torch.where(key >= 0, key, torch.full_like(key, -1))[None]


def uniform_prefix_rows(v, max_bias=256.0):
    """(o, beta) of causal rows whose unmasked scores are all EQUAL, v (1, L, H, 64) >= 0: o_t = mean(v[0 .. t]); every e is exp(0) = 1, no key is
    flippable, sum P |v| / sum e = o, and attention_beta's terms are o (delta + gamma + 2 c 2^-24 + 2^-23) with delta = 2^-23 (|bias| + 2 n + 4),
    gamma <= 2^-23 n, c = 3 n + 4"""
    L = v.shape[1]
    o = v.double().cumsum(1) / torch.arange(1, L + 1).double()[None, :, None, None]
    n = (torch.arange(L) // KT + 1).double()[None, :, None, None]
    return o, o * (2.0 ** -23 * (max_bias + 3 * n + 4) + 2 * (3 * n + 4) * 2.0 ** -24 + 2.0 ** -23)


def check_bias_probe(c, key, got, uniform=None):
    """-> record; exact rows bit for bit, the uniform rows on the criterion (`uniform`: uniform_prefix_rows(v), computed once for a sweep)"""
    hit = key >= 0
    b, t, h = torch.nonzero(hit, as_tuple=True)
    exact = bool(torch.equal(got[hit].view(torch.int16), c["v"][b, key[hit], h].view(torch.int16)))
    rec = dict(elements=0, stable_share=1.0, stable_wrong=0, unstable_differ=0, unstable_wrong=0, worst_err_over_allowance=0.0, ok=True)
    if bool((~hit).any()):
        uo, ub = uniform if uniform is not None else uniform_prefix_rows(c["v"])
        rec = check_bf16(got[~hit], uo[~hit], ub[~hit])
    return dict(rec, exact_rows=int(hit.sum()), exact=exact, ok=rec["ok"] and exact)


# ----------------------------------------------------------------------------- score probe
SCORE_CAUSAL_L = [1, 2, 63, 64, 65, 127, 128, 129, 160, 1024]
SCORE_CROSS_KEYS = [1, 63, 64, 65, 128, 512]
SCORE_RPK = [1, 3, 13]


def score_probe_case(causal, L, n_keys, n_rows, H, row0, rpk, layout):
    """K[key] = 16 e_{key mod 32} + 16 e_{32 + key / 32} (two hot coordinates from disjoint ranges, 1024 distinct keys), Q = the coordinates of the
    row's target: the target scores 512, a key sharing one coordinate 256, the rest 0; the bias is 0.  The target wins by 256 in every tile
    schedule: the row returns V[slab, target] bit for bit.  Targets: the newest key, key 0, and a key spread over every tile at or below the
    query's (cross: over all).  V = v_code."""
    n_slabs = (row0 + n_rows - 1) // rpk + 1
    r, t, h = torch.meshgrid(torch.arange(n_rows), torch.arange(L), torch.arange(H), indexing="ij")
    lim = t + 1 if causal else torch.full_like(t, n_keys)
    spread = (29 * t + 7 * h + 3 * r + 5) % lim
    pick = (t + h + r) % 3
    key = torch.where(pick == 0, lim - 1, torch.where(pick == 1, torch.zeros_like(t), spread))
    q = torch.zeros(n_rows, L, H, 64).scatter_(3, (key % 32)[..., None], 16.0).scatter_(3, (32 + key // 32)[..., None], 16.0)
    kk = torch.arange(n_keys)[None, :, None].expand(n_slabs, n_keys, H)
    k = torch.zeros(n_slabs, n_keys, H, 64).scatter_(3, (kk % 32)[..., None], 16.0).scatter_(3, (32 + kk // 32)[..., None], 16.0)
    k[:row0 // rpk] = float("nan")
    v = v_code(n_slabs, n_keys, H)
    bias = torch.zeros(H, L + 3) if causal else None
    return dict(causal=causal, q=q.bfloat16(), k=k.bfloat16(), v=v, bias=bias, row0=row0, rows_per_kv=rpk, layout=layout), key


def score_probe_cases():
    """(name, causal, L, n_keys, n_rows, H, row0, rpk, layout)"""
    out = []
    for i, L in enumerate(SCORE_CAUSAL_L):
        n_rows, row0 = (1, 0) if L == 1024 else (3, (0, 2)[i % 2])
        out.append((f"causal_L{L}", True, L, L, n_rows, 2, row0, 1, ("fused", "headmajor")[i % 2]))
    for i, nk in enumerate(SCORE_CROSS_KEYS):
        for j, rpk in enumerate(SCORE_RPK):
            L = (1, 17, 129, 140)[(i + j) % 4]
            row0 = 0 if rpk == 1 else rpk - 1                              # rows rpk - 1, rpk, ...: the slab changes after the first row
            out.append((f"cross_k{nk}_rpk{rpk}_L{L}", False, L, nk, 3, 2, row0, rpk, "fused" if rpk == 1 and (i % 2) else "headmajor"))
    return out


def check_score_probe(c, key, got):
    idx = slab_of_row(c)
    r, t, h = torch.meshgrid(torch.arange(got.shape[0]), torch.arange(got.shape[1]), torch.arange(got.shape[2]), indexing="ij")
    want = c["v"][idx[r], key, h]
    ok = bool(torch.equal(got.view(torch.int16), want.view(torch.int16)))
    return dict(elements=int(got.numel()), ok=ok, wrong_rows=int((got != want).any(-1).sum()))


# ----------------------------------------------------------------------------- layouts
def attention_layout(c):
    """The case's tensors placed as production places them, with NaN wherever nothing may read.  -> dict(q, k, v: (flat bf16 buffer, offset),
    strides, out_size, out_index (n_rows, L, H, 64) of flat positions in the output region).
      'fused'      one buffer [(row0 + n_rows)][max(L, n_keys)][3 inner], ld = 3 inner, kv_head = 64 (score_impl's self-attention; rows_per_kv = 1)
      'headmajor'  k / v [slab][H][n_keys][64] + pads, ldkv = 64, kv_head = n_keys 64 + 64 (score_impl's cross-attention); q rows of inner + 8,
                   out rows of inner + 24"""
    q, k, v = c["q"], c["k"], c["v"]
    n_rows, L, H, _ = q.shape
    n_slabs, nk = k.shape[0], k.shape[1]
    inner, row0 = H * 64, c["row0"]
    nan = float("nan")
    if c["layout"] == "fused":
        assert c["rows_per_kv"] == 1 and n_slabs == row0 + n_rows
        T = max(L, nk)
        buf = torch.full((n_slabs, T, 3, inner), nan).bfloat16()
        buf[row0:, :L, 0] = q.reshape(n_rows, L, inner)
        buf[:, :nk, 1], buf[:, :nk, 2] = k.reshape(n_slabs, nk, inner), v.reshape(n_slabs, nk, inner)
        seq = T * 3 * inner
        st = dict(ldq=3 * inner, ldkv=3 * inner, kv_head=64, q_seq=seq, kv_seq=seq)
        bufs = dict(q=(buf, row0 * seq), k=(buf, inner), v=(buf, 2 * inner))
    else:
        ldq = inner + 8
        qb = torch.full((n_rows, L, ldq), nan).bfloat16()
        qb[..., :inner] = q.reshape(n_rows, L, inner)
        kvh, kvs = nk * 64 + 64, H * (nk * 64 + 64) + 128
        kb, vb = torch.full((n_slabs, kvs), nan).bfloat16(), torch.full((n_slabs, kvs), nan).bfloat16()
        for h in range(H):
            kb[:, h * kvh:h * kvh + nk * 64] = k[:, :, h].reshape(n_slabs, nk * 64)
            vb[:, h * kvh:h * kvh + nk * 64] = v[:, :, h].reshape(n_slabs, nk * 64)
        st = dict(ldq=ldq, ldkv=64, kv_head=kvh, q_seq=L * ldq, kv_seq=kvs)
        bufs = dict(q=(qb, 0), k=(kb, 0), v=(vb, 0))
    ldo = inner + 24
    o_seq = L * ldo + 8
    r, t, e = torch.meshgrid(torch.arange(n_rows), torch.arange(L), torch.arange(inner), indexing="ij")
    st.update(ldo=ldo, o_seq=o_seq)
    return dict(bufs, strides=st, out_size=n_rows * o_seq, out_index=(r * o_seq + t * ldo + e).reshape(n_rows, L, H, 64))


# ============================================================================= lm head
LM_MUTANTS = ["lm_target_other_half", "lm_target_quarter_missing", "lm_merge_without_rescale", "lm_three_quarters", "lm_last_tile_dropped",
              "lm_j_le_len", "lm_row0_ignored", "lm_j_from_position_0"]


def lm_reference(c, mutant=None):
    """-> dict(scores (rows, n_steps) float64 with SENT where nothing is written, logits (rows, n_steps, V) likewise, score_bound, logit_bound, written
    (rows, n_steps) bool).  rows = row0 + M / L, indexed by the absolute row.

    Score bound, per written element, with b_v the any-order GEMM bound of logit v (K = 512), p = softmax(logits), lse = log sum exp:
      b_target + sum_v p_v b_v                                    the logits' own errors (d lse / d logit_v = p_v)
      + sum_v p_v 2^-23 (2 |logit_v - max| + 2)                   __expf of every term: the subtraction and the product with log2(e) round the
                                                                  exponent, twice over the path (against the running and then the final maximum:
                                                                  the two gaps add up to logit_v - max), v_exp_f32 at 1 ulp, twice
      + 2^-24 (V / 4 + 3) + 3 2^-24 (V / 16 + 1)                  the additions of a lane's sum (4 per tile) and the two merges; per tile the alpha's
                                                                  v_exp_f32 ulp (2 units) and the product with it, once more at the meeting
      + 2^-22 |log s| + 2^-149                                    logf at 2 ulp
      + 2^-24 (|lse| + |max| + |score|)                           max + logf(s), then target - that"""
    xn, W, V, L, P, n_steps, row0 = c["xn"], c["W"], c["V"], c["L"], c["P"], c["n_steps"], c["row0"]
    M = xn.shape[0]
    rows = row0 + M // L
    logit, b = gemm_reference_and_bound(xn, W)
    scores = torch.full((rows, n_steps), SENT, dtype=torch.float64)
    logits = torch.full((rows, n_steps, V), SENT, dtype=torch.float64)
    sb, lb = torch.zeros(rows, n_steps, dtype=torch.float64), torch.zeros(rows, n_steps, V, dtype=torch.float64)
    written = torch.zeros(rows, n_steps, dtype=torch.bool)
    mrow = torch.arange(M)
    lr, pos = mrow // L, mrow % L
    j = pos if mutant == "lm_j_from_position_0" else pos - P
    ok = (j >= 0) & (j < n_steps)
    arow = lr if mutant == "lm_row0_ignored" else row0 + lr
    tgt_rows = mrow ^ 16 if mutant == "lm_target_other_half" else mrow
    tgt_ok = tgt_rows < M
    tr = tgt_rows.clamp(max=M - 1)
    tgt = c["tokens"][arow[tr], j[tr].clamp(0, n_steps - 1)].long().clamp(0, V - 1)
    lg = logit[:, :V - 16] if mutant == "lm_last_tile_dropped" and V > 16 else logit
    quarter = (torch.arange(lg.shape[1]) % 16) // 4
    if mutant == "lm_three_quarters":
        lg = lg[:, quarter != 3]
    mx = lg.max(-1, keepdim=True).values
    if mutant == "lm_merge_without_rescale":                              # each quarter's sum left in its own scale
        s = sum(torch.exp(lg[:, quarter == qq] - lg[:, quarter == qq].max(-1, keepdim=True).values).sum(-1) for qq in range(4))
    else:
        s = torch.exp(lg - mx).sum(-1)
    lse = mx[:, 0] + torch.log(s)
    tl = logit[mrow, tgt]
    if mutant == "lm_target_quarter_missing":
        tl = torch.where((tgt % 16) // 4 == 3, torch.full_like(tl, float("-inf")), tl)
    if mutant == "lm_last_tile_dropped":
        tl = torch.where(tgt >= lg.shape[1], torch.full_like(tl, float("-inf")), tl)
    sc = tl - lse
    ln = c["lengths"][arow].long().clamp(0, n_steps) if c["lengths"] is not None else torch.full((M,), n_steps)
    sc = torch.where((j <= ln) if mutant == "lm_j_le_len" else (j < ln), sc, torch.zeros_like(sc))
    p = torch.exp(logit - mx - torch.log(s)[:, None])
    rho = (p * 2.0 ** -23 * (2 * (logit - mx).abs() + 2)).sum(-1) + 2.0 ** -24 * (V / 4 + 3) + 3 * 2.0 ** -24 * (V / 16 + 1)
    bound = b[mrow, tgt] + (p * b).sum(-1) + rho + 2.0 ** -22 * torch.log(s).abs() + 2.0 ** -149 + 2.0 ** -24 * (lse.abs() + mx[:, 0].abs() + sc.abs())
    bound = torch.where(j < ln, bound, torch.zeros_like(bound))
    sel = ok & tgt_ok
    scores[arow[sel], j[sel]], sb[arow[sel], j[sel]], written[arow[sel], j[sel]] = sc[sel], bound[sel], True
    logits[arow[sel], j[sel]], lb[arow[sel], j[sel]] = logit[sel], b[sel]
    return dict(scores=scores, logits=logits, score_bound=sb, logit_bound=lb, written=written)


def check_lm(c, got_scores, got_logits=None):
    """got_scores (rows, n_steps) f32 and got_logits (rows, n_steps, V) f32 or None, whole regions (SENT where untouched).  A NaN never passes."""
    ref = lm_reference(c)
    w = ref["written"]
    untouched = bool((got_scores[~w] == SENT).all()) and bool((got_scores[w] != SENT).all())
    live = w & (ref["score_bound"] > 0)                                   # the columns past a row's length have the bound 0: exactly 0.0
    past = bool((got_scores[w & ~live] == 0).all())
    rec = dict(elements=int(w.sum()), worst_err_over_beta=0.0, past_length_exact=past, ok=past and untouched)
    if bool(live.any()):
        f = check_f32(got_scores[live], ref["scores"][live], ref["score_bound"][live])
        rec.update(worst_err_over_beta=f["worst_err_over_beta"], ok=rec["ok"] and f["ok"])
    if got_logits is not None:
        f = check_f32(got_logits[w], ref["logits"][w], ref["logit_bound"][w])
        rec["worst_logit_err_over_beta"] = f["worst_err_over_beta"]
        rec["ok"] = rec["ok"] and f["ok"] and bool((got_logits[~w] == SENT).all())
    return rec


def lm_case(M, L, P, V, row0, with_lengths, seed=0):
    """plain random operands: logits of std ~ 1.4 x 22 / 16, the softmax neither one-hot nor uniform; targets with out-of-range ids; lengths
    below 0 and beyond n_steps"""
    g = torch.Generator().manual_seed(seed + 3 * M + 5 * L + 7 * V + 11 * row0)
    n_steps = L - P
    rows = row0 + M // L
    tokens = torch.randint(0, V, (rows, n_steps), generator=g, dtype=torch.int32)
    tokens[row0:, ::5] = torch.tensor([-3, V, V + 70000])[torch.arange(tokens[row0:, ::5].numel()) % 3].reshape(tokens[row0:, ::5].shape).int()
    lengths = torch.randint(-1, n_steps + 2, (rows,), generator=g, dtype=torch.int32) if with_lengths else None
    return dict(xn=torch.randn(M, 512, generator=g).bfloat16(), W=(torch.randn(V, 512, generator=g) / 16).bfloat16(), tokens=tokens, lengths=lengths,
                M=M, L=L, P=P, n_steps=n_steps, V=V, row0=row0)


# M -> (L, P): every M of the issue as rows x positions, with a prompt wherever L allows one
LM_EDGE_M = {1: (1, 0), 15: (5, 2), 16: (4, 1), 17: (17, 5), 32: (8, 0), 33: (11, 3), 127: (127, 40), 128: (16, 5), 129: (43, 0)}
LM_EDGE_V = [16, 32, 48, 1536]


def lm_edge_cases():
    """(name, M, L, P, V, row0, with_lengths): every M with V = 48 and every V with M = 33 and 129; row0, lengths and the prompt rotate"""
    out = []
    for i, (M, (L, P)) in enumerate(LM_EDGE_M.items()):
        out.append((f"M{M}_V48", M, L, P, 48, (0, 3)[i % 2], bool((i // 2) % 2)))
    for i, V in enumerate(LM_EDGE_V):
        for M in (33, 129):
            L, P = LM_EDGE_M[M]
            out.append((f"M{M}_V{V}", M, L, P, V, (2, 0)[i % 2], bool(i % 2) ^ (M == 33)))
    return out


def lm_winner_case(M=512, L=4, P=0, V=1536, row0=1):
    """xn one-hot rows (row m selects column (7 m + 3) mod 512), W[v][k] = (3 v + k) mod 251 but for the column's winner w(k) = (37 k + 5) mod V,
    which holds 512: the logits are W's column exactly, the winner leads by at least 262 (exp(-262) is 0 in fp32), the log-sum-exp is 512 and
    the score code[target] - 512 exactly, 0 at the winner.  Targets: flat row m aims at residue (m mod 16) + 16 (m / 128 mod 2) modulo 32, so
    that each (wave, 16-row half) meets every (tile parity, lane quarter, element) over the first two workgroups; the rows of the other two aim
    at their winners."""
    m = torch.arange(M)
    col = (7 * m + 3) % 512
    xn = torch.zeros(M, 512)
    xn[m, col] = 1.0
    kk = torch.arange(512)
    W = ((3 * torch.arange(V)[:, None] + kk[None, :]) % 251).float()
    win = (37 * kk + 5) % V
    W[win, kk] = 512.0
    tgt = (m % 16) + 16 * (m // 128 % 2) + 32 * ((5 * m) % (V // 32))
    tgt = torch.where(m >= M // 2, win[col], tgt)
    n_steps, rows = L - P, row0 + M // L
    tokens = torch.zeros(rows, n_steps, dtype=torch.int32)
    tokens[row0:] = tgt.reshape(M // L, L)[:, P:].int()
    want = torch.full((rows, n_steps), SENT)
    want[row0:] = (W[tgt, col] - 512.0).reshape(M // L, L)[:, P:]
    return dict(xn=xn.bfloat16(), W=W.bfloat16(), tokens=tokens, lengths=None, M=M, L=L, P=P, n_steps=n_steps, V=V, row0=row0), want, tgt


def check_lm_winner(c, want, got_scores):
    return dict(elements=int((want != SENT).sum()), ok=bool(torch.equal(got_scores.view(torch.int32), want.float().view(torch.int32))),
                zeros=int((want == 0).sum()))


def lm_uniform_case(M=20, L=5, P=1, V=1536, row0=0):
    c = lm_case(M, L, P, V, row0, False, seed=9)
    c["xn"] = torch.zeros_like(c["xn"])
    return c


def join(recs):
    """one record for several checks: sums and worsts"""
    out = dict(elements=sum(r["elements"] for r in recs), ok=all(r["ok"] for r in recs))
    for key, f in (("stable_share", min), ("worst_err_over_allowance", max), ("worst_err_over_beta", max), ("worst_logit_err_over_beta", max),
                   ("stable_wrong", sum), ("unstable_differ", sum), ("unstable_wrong", sum), ("unstable", sum), ("exact_rows", sum), ("wrong_rows", sum)):
        vals = [r[key] for r in recs if key in r]
        if vals:
            out[key] = f(vals)
    return out


assert math.isclose(KT * 2, QB)
