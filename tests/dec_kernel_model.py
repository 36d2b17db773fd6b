"""References, criteria and inputs for the per-kernel tests of the decoder step's separate-launch kernels (tests/test_decoder_kernels.py on the
GPU, tests/test_decoder_kernels_cpu.py for the model itself).  TEST INFRASTRUCTURE ONLY, CPU only.  The criterion (stable element => bit-exact,
otherwise within beta + 1 bf16 ulp; fp32 outputs by error / beta) is tests/enc_kernel_model.py's and is imported from there.

CONTRACTS, read off csrc/decode.hip and csrc/mc_cross_attn.hip (R(.) = round to nearest-even bf16; every sum fp32 on the device, float64 here):

  decode GEMMs (dec_gemm_kernel / dec_gemm_mid_kernel), rows [row0, row0 + R):
    norm operand   xn[r][k] = R(x[r][k] * rsqrt(sum_{t<32} ssq[t][r] / K + eps) * gain[k])                      (modes 0..3, K = 512)
    accumulation   acc[r][n] = sum_k xn[r][k] W[n][k]   (mode 4: a_bf16 in place of xn)                        fp32 over bf16 operands
    mode 1 / 2     out_bf16[r][n] = R(acc) / R(max(acc, 0))
    mode 3         out_f32[r][n] = acc
    mode 4         h[r][n] = h[r][n] + acc, or (h + (((p0 + p1) + ...) + p7)) + acc with `part` [R][8][512];
                   ssq[n / 16][r] = sum over the tile's 16 columns of h_new^2 (the partials the next norm reads)
    mode 0         columns [0, 64 H) -> out_bf16[r][.]; K and V thirds -> cache[((r H + h) L + pos) 64 + d], pos = row_pos[r] or step;
                   `table`: the packed row -> table[r N + n] and nothing else
    pend_y         x = f32(x_f32 + f32(y[2r] + y[2r + 1])), sum(x^2) taken from x itself; mode 0: h_out[r] = x (written by column tile 0)

  step attention (dec_attn_kernel, dec_attn_beam_kernel), one (row, head):
    o = R(sum_k softmax_k(q . k_k + bias[h][n_keys - 1 - k]) v_k), keys 0 .. n_keys - 1 of slab (r / rows_per_kv, h); fp32 throughout: no
    1/sqrt(d), p is NOT rounded.  self: n_keys = pos + 1; cross: n_keys_const, no bias.
    fused query    q = R(R(x scale gain) . wq[h]^T), x the residual row or f32(h + (((p0 + p1) + ...) + p7)) with sum(x^2) rebuilt from it
    folded O-proj  opart[r][h][c] = sum_d R(o)_d wo[c][64 h + d] in fp32, no `out`
    beam           key k lives in the slab of row (r - r % W) + min(anc[(n_keys - 1) & 1][r][k], W - 1)
  multi-channel cross-attention (mc_cross_attn_kernel): the fused-query contract, p carried into the MFMA as two bf16 terms p_hi + p_lo.

BOUNDS (each at its helper): gemm_beta, attention_beta, the candidate rule for a fused query (query_candidates, check_fused).  CAPS, conditions on the inputs
that the CPU module checks under the reference alone: stable share >= MIN_STABLE per case, left-out (row, head) pairs <= MAX_LEFT_OUT per case.
"""
from __future__ import annotations

import itertools

import torch

from enc_kernel_model import MIN_STABLE, check_bf16, check_f32, judge_bf16, rb, trunc_bf16, ulp_bf16  # noqa: F401 (MIN_STABLE: re-exported)

DG_QKV, DG_BF16, DG_RELU, DG_LOGITS, DG_RESID = range(5)
SSQ_TILES = 32
MAX_LEFT_OUT = 0.05
SENT = 12352.0                      # the sentinel of tests/test_encoder_kernels.py (exact in bf16 and fp32; no input or result holds it)
F64 = torch.float64


def merge(recs):
    """one record for several checks of one test: the worst of each figure (bf16 and fp32 checks may mix)"""
    out = dict(elements=sum(r["elements"] for r in recs), ok=all(r["ok"] for r in recs))
    b = [r for r in recs if "stable_share" in r]
    f = [r for r in recs if "worst_err_over_beta" in r]
    if b:
        out.update(worst_err_over_allowance=max(r["worst_err_over_allowance"] for r in b), stable_share=min(r["stable_share"] for r in b),
                   stable_wrong=sum(r["stable_wrong"] for r in b), unstable_differ=sum(r["unstable_differ"] for r in b),
                   unstable_wrong=sum(r["unstable_wrong"] for r in b))
    if f:
        out.update(worst_err_over_beta=max(r["worst_err_over_beta"] for r in f))
    if any("left_out_share" in r for r in recs):
        out.update(left_out_share=max(r.get("left_out_share", 0.0) for r in recs))
    return out


def exact(name, got, want):
    """a bit-for-bit check as a record"""
    same = got.shape == want.shape and bool((got.double() == want.double()).all())
    return dict(elements=int(want.numel()), ok=same, exact=name)


# ============================================================================= decode GEMMs
def ssq_partials(h):
    """what a producer of the residual stream leaves for the next norm: (32, R) fp32, tile t = sum of h^2 over columns [16 t, 16 t + 16)"""
    R, d = h.shape
    assert d == 16 * SSQ_TILES
    return h.double().pow(2).reshape(R, SSQ_TILES, 16).sum(-1).T.contiguous().float()


def norm_operand(x, gain, ms, eps, dtype=F64, mutant=None):
    """x (R, K) fp32 values, gain (K,), ms (R,) the mean square in `dtype` -> (xn, pre): the bf16-rounded operand and its value before the
    rounding.  Mutants: eps_outside, gain_next (the gain of column k + 1), unrounded_operand."""
    x, gain = x.to(dtype), gain.to(dtype)
    scale = 1.0 / (ms.sqrt() + eps) if mutant == "eps_outside" else torch.rsqrt(ms + eps)
    if mutant == "gain_next":
        gain = gain.roll(-1)
    pre = x * scale[:, None] * gain[None, :]
    return (pre if mutant == "unrounded_operand" else rb(pre)), pre


def norm_flippable(pre, K):
    """xn_k may round the other way on a correct device when [pre - b, pre + b] rounds two ways, b = (K / 64 + 8) 2^-24 |pre|: the bound of
    enc_kernel_model.rmsnorm_beta (the 32 partials are summed in a fixed tree of 5 additions where that kernel sums K / 64 squares and six
    butterfly steps; with pend_y the kernel sums 4 squares, four 16-lane steps and the eight waves: 15 roundings of the mean square, 7.5 of
    the scale; then the division by K, the addition of eps, v_rsq_f32 at 1 ulp and the two products -- under K / 64 + 8 = 16 either way)."""
    b = (K / 64 + 8) * 2.0 ** -24 * pre.abs()
    return rb(pre - b) != rb(pre + b)


def gemm_beta(xn, pre, W, flip=None):
    """beta of acc = xn . W^T for a bf16 or fp32 output:  K 2^-24 sum |xn||w|  (any fp32 summation order of K exact products: value_regimes.
    gemm_reference_and_bound)  +  sum over flippable k of ulp_bf16(xn_k) |w_k|  (a correct device may hold the neighbouring bf16 operand there)."""
    K = xn.shape[1]
    Wa = W.double().abs()
    beta = K * 2.0 ** -24 * (xn.double().abs() @ Wa.T) + K * 2.0 ** -149
    if flip is not None:
        beta = beta + (flip.double() * ulp_bf16(pre)) @ Wa.T
    return beta


def pend_sum(x, y, mutant=None):
    """x = f32(h + f32(y[2r] + y[2r + 1])): the kernel's two fp32 additions in its order (part of the contract: h_out holds these bits).
    Mutant pend_rows: y[r] + y[r + R]."""
    R = x.shape[0]
    y = y.float()
    y0, y1 = (y[:R], y[R:]) if mutant == "pend_rows" else (y[0::2], y[1::2])
    return x.float() + (y0 + y1)


def dec_gemm_model(mode, c, dtype=F64, mutant=None):
    """c: a case (dict of host tensors: W, and x / gain / ssq / eps / pend_y, or a / h / part) -> dict(acc, o, [xn, pre, x_eff, ssq_out]).
    `o` is the value before the output's final rounding (mode 2: NOT clamped; modes 3, 4: the fp32 result itself)."""
    W = c["W"].to(dtype)
    res = {}
    if mode == DG_RESID:
        a = c["a"].to(dtype)
        acc = a @ W.T
        base = c["h"].to(dtype)
        if c.get("part") is not None:
            p = c["part"].to(dtype)
            base = base + (p[:, :7] if mutant == "part_7" else p).sum(1)
        o = acc if mutant == "resid_overwrites" else base + acc
        R, N = o.shape
        sq = acc if mutant == "ssq_from_s" else o
        res.update(xn=a, pre=a, ssq_out=sq.pow(2).reshape(R, N // 16, 16).sum(-1).T.contiguous(), base=base)
    else:
        K = W.shape[1]
        x = c["x"]
        if c.get("pend_y") is not None:
            x = pend_sum(x, c["pend_y"], mutant)
            res["h_out"] = c["x"].float() if mutant == "h_out_no_pend" else x
            ms = x.to(dtype).pow(2).sum(-1) / K
        else:
            parts = c["ssq"].to(dtype)
            ms = (parts[:31] if mutant == "ssq_31" else parts).sum(0) / K
        xn, pre = norm_operand(x, c["gain"], ms, c["eps"], dtype, mutant)
        acc = xn @ W.T
        o = acc
        res.update(xn=xn, pre=pre)
    res.update(acc=acc, o=o)
    return res


def dec_gemm_reference(mode, c):
    """the float64 reference of a case with its beta (module docstring; mode 4 adds 2^-24 |result| for the residual addition and, with `part`,
    the seven additions of the partial sum -- 7 2^-24 sum_w |p_w| -- and the addition of that sum to h, 2^-24 |h + sum p|)"""
    ref = dec_gemm_model(mode, c)
    if mode == DG_RESID:
        beta = gemm_beta(ref["xn"], ref["pre"], c["W"]) + 2.0 ** -24 * ref["o"].abs()
        if c.get("part") is not None:
            beta = beta + 2.0 ** -24 * (7 * c["part"].double().abs().sum(1) + ref["base"].abs())
        ref["flip"] = None
    else:
        ref["flip"] = norm_flippable(ref["pre"], c["W"].shape[1])
        beta = gemm_beta(ref["xn"], ref["pre"], c["W"], ref["flip"])
    ref["beta"] = beta
    return ref


def qkv_place(o, H, L, pos, like, mutant=None):
    """mode 0's scatter of the packed rows o (R, 3 H 64) (already rounded) -> (q (R, H 64), kcache, vcache (R, H, L, 64) filled with SENT but for
    position pos[r]).  Mutants: append_plus_one, swap_kv."""
    R = o.shape[0]
    inner = H * 64
    q, k, v = o[:, :inner], o[:, inner:2 * inner].reshape(R, H, 64), o[:, 2 * inner:].reshape(R, H, 64)
    if mutant == "swap_kv":
        k, v = v, k
    if mutant == "append_plus_one":
        pos = (pos + 1) % L
    kc = torch.full((R, H, L, 64), SENT, dtype=like)
    vc = torch.full((R, H, L, 64), SENT, dtype=like)
    kc[torch.arange(R), :, pos] = k.to(like)
    vc[torch.arange(R), :, pos] = v.to(like)
    return q.to(like), kc, vc


def dec_gemm_simulate(mode, c, dtype=torch.float32, mutant=None):
    """what a device computing the model in `dtype` (the fp32 oracle's arithmetic by default) would leave, in the layout check_dec_gemm takes:
    the rows [row0, row0 + R) only.  Mutant no_relu: mode 2 without its clamp."""
    m = dec_gemm_model(mode, c, dtype, mutant)
    o = m["o"]
    if mode == DG_RESID:
        return dict(h=o.float(), ssq=m["ssq_out"].float())
    got = {}
    if "h_out" in m and mode == DG_QKV:
        got["h_out"] = m["h_out"]
    if mode == DG_LOGITS:
        got["out"] = o.float()
    elif mode == DG_QKV:
        packed = rb(o).bfloat16()
        if c.get("table"):
            got["table"] = packed
        else:
            got["q"], got["kc"], got["vc"] = qkv_place(packed, c["H"], c["L"], c["pos"], torch.bfloat16, mutant)
    else:
        got["out"] = rb(o if mode == DG_BF16 or mutant == "no_relu" else o.clamp(min=0)).bfloat16()
    return got


def check_dec_gemm(mode, c, ref, got):
    """the GPU test's whole check of one launch: `got` as dec_gemm_simulate lays it out -> one merged record"""
    o, beta = ref["o"], ref["beta"]
    recs = []
    if mode == DG_RESID:
        recs.append(check_f32(got["h"], o, beta))
        # the partials against the DEVICE's own h_new in double: 16 squares and 15 additions of positive terms, (16 + 2) 2^-24 relative
        own = got["h"].double().pow(2).reshape(o.shape[0], -1, 16).sum(-1).T
        recs.append(check_f32(got["ssq"], own, (16 + 2) * 2.0 ** -24 * own + 2.0 ** -140))
    elif mode == DG_LOGITS:
        recs.append(check_f32(got["out"], o, beta))
    elif mode == DG_QKV:
        H, L, R = c["H"], c["L"], o.shape[0]
        if c.get("table"):
            recs.append(check_bf16(got["table"], o, beta))
        else:
            inner = H * 64
            rows = torch.arange(R)
            recs.append(check_bf16(got["q"], o[:, :inner], beta[:, :inner]))
            for name, lo in (("kc", inner), ("vc", 2 * inner)):
                cache = got[name]
                recs.append(check_bf16(cache[rows, :, c["pos"]].reshape(R, inner), o[:, lo:lo + inner], beta[:, lo:lo + inner]))
                rest = torch.ones(R, H, L, dtype=torch.bool)
                rest[rows, :, c["pos"]] = False
                recs.append(exact(name + " elsewhere", cache[rest].float(), torch.full_like(cache[rest].float(), SENT)))
        if "h_out" in ref:
            recs.append(exact("h_out", got["h_out"], ref["h_out"]))
    else:
        recs.append(check_bf16(got["out"], o, beta, relu=mode == DG_RELU))
    return merge(recs)


def gemm_case(mode, R, N, K, seed=0, H=0, L=0, pos=None, part=False, pend=False, table=False, eps=1e-3):
    """Sign-coherent operands (enc_kernel_model.gemm_case): x = |randn| times a per-row power of two, a positive gain, row n of W = sign_n |randn|
    / K, so that acc = +- sum |xn||w| and the any-order bound is K 2^-24 RELATIVE.  eps = 1e-3 against mean squares from 2^-6 on: a misplaced
    eps moves the scale by 2 %.  The ssq partials are those of x itself.  Half the rows of W are negative (ReLU clamps half the columns)."""
    g = torch.Generator().manual_seed(seed + 1000 * mode + R + N + K)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    W = (torch.randn(N, K, generator=g).abs() * sign[:, None] / K).bfloat16()
    c = dict(W=W, eps=eps, H=H, L=L, table=table)
    if mode == DG_RESID:
        c["a"] = torch.randn(R, K, generator=g).abs().bfloat16()
        c["h"] = torch.randn(R, N, generator=g) * 0.25
        c["part"] = torch.randn(R, 8, N, generator=g) * 0.05 if part else None
        return c
    x = torch.randn(R, K, generator=g).abs() * torch.exp2(torch.randint(-3, 4, (R, 1), generator=g).float())
    c["gain"] = (0.5 + torch.rand(K, generator=g)) * torch.exp2(torch.randint(-1, 2, (K,), generator=g).float())
    if pend:
        y = torch.randn(2 * R, K, generator=g).abs() * 0.125
        c["pend_y"] = y
        c["x"] = x
    else:
        c["x"] = x
        c["ssq"] = ssq_partials(x)
    if mode == DG_QKV and not table:
        c["pos"] = pos if pos is not None else torch.randint(0, L, (R,), generator=g)
    return c


def permutation_case(mode, R, N, K):
    """exact: row i selects column (7 i + 3) mod K of W[n][k] = (3 n + k) mod 251.  mode 4: a one-hot a_bf16, h = 0.  NORM modes: x = c e_j
    with sum(x^2) = c^2 in its tile, eps = 0, gain 1: xn_j = R(c rsqrt(c^2 / 512)) = R(sqrt(512)) = 22.625, three bf16 ulps from a rounding
    boundary; the products 22.625 w are exact in fp32 (8 + 8 bits) and lie on the bf16 grid only for some w, so the want is R(22.625 w)."""
    sel = (torch.arange(R) * 7 + 3) % K
    Wp = (torch.arange(N)[:, None] * 3 + torch.arange(K)[None, :]).float().remainder(251).bfloat16()
    c = dict(W=Wp, eps=0.0, H=0, L=0, table=False)
    col = Wp.float()[:, sel].T.contiguous()
    if mode == DG_RESID:
        a = torch.zeros(R, K)
        a[torch.arange(R), sel] = 1.0
        c.update(a=a.bfloat16(), h=torch.zeros(R, N), part=None)
        return c, col
    cval = torch.exp2((torch.arange(R) % 5 - 2).float())
    x = torch.zeros(R, K)
    x[torch.arange(R), sel] = cval
    c.update(x=x, gain=torch.ones(K), ssq=ssq_partials(x))
    return c, 22.625 * col


# ============================================================================= step attention
# the kernels' partition: NW waves per (row, head), U sub-blocks of 8 NW keys per block
def attention_model(q, k, v, bias, n, dtype=F64, mutant=None, NW=8):
    """q (P, 64), k / v (P, Nmax, 64), bias (P, Nmax) or None, n (P,) key counts: keys >= n[p] do not exist (whatever k / v hold there, NaN
    included) -> dict(o (P, 64) before the output rounding, s, M, e, l).  Mutants (wrong kernels): scale (1 / sqrt(64)), round_p (the encoder's
    contract: bf16(e) in the numerator; the multi-channel kernel without its low term), drop_wave (the partial of the last wave -- keys with
    (key / 8) % NW == NW - 1 -- left out of the merge), merge_no_rescale (wave partials, each relative to its own maximum, added as they are)."""
    P, Nmax, _ = k.shape
    live = torch.arange(Nmax)[None, :] < n[:, None]
    if mutant == "drop_wave":
        dropped = live & ((torch.arange(Nmax)[None, :] // 8) % NW == NW - 1)
        live = torch.where((live & ~dropped).any(-1, keepdim=True), live & ~dropped, live)
    q = q.to(dtype)
    k = torch.where(live[..., None], k.to(dtype), torch.zeros((), dtype=dtype))
    v = torch.where(live[..., None], v.to(dtype), torch.zeros((), dtype=dtype))
    s = torch.einsum("pd,pkd->pk", q, k)
    if mutant == "scale":
        s = s / 8.0
    if bias is not None:
        s = s + torch.where(live, bias.to(dtype), torch.zeros((), dtype=dtype))
    s = torch.where(live, s, torch.full((), -float("inf"), dtype=dtype))
    M = s.max(-1, keepdim=True).values
    if mutant == "merge_no_rescale":
        wave = (torch.arange(Nmax) // 8) % NW
        Mw = torch.full_like(s, -float("inf"))
        for w in range(NW):
            mw = s[:, wave == w].max(-1, keepdim=True).values if bool((wave == w).any()) else M
            Mw[:, wave == w] = mw
        e = torch.exp(s - torch.where(torch.isfinite(Mw), Mw, M))
    else:
        e = torch.exp(s - M)
    e = torch.where(live, e, torch.zeros((), dtype=dtype))
    l = e.sum(-1, keepdim=True)
    p = rb(e) if mutant == "round_p" else e
    o = torch.einsum("pk,pkd->pd", p, v) / l
    return dict(o=o, s=s, M=M, e=e, l=l, live=live, k=k, v=v)


def attention_beta(q, parts, bias, n, NW, U, two_term_p=False, depth_c=True):
    """beta of o (P, 64) from the float64 parts.
    delta_k = 2^-23 (sum_d |q_d k_kd| + |bias_k| + 2 |s_k - M| + 2 n_stage + 4) bounds the relative error of key k's weight e_k as it reaches the
    final sums: the score (64 fp32 fmas and the bias addition), its own exponential (enc_kernel_model.attention_beta), and the n_stage rescale
    factors exp(m_old - m_new) it is multiplied by on the way -- one per block of the wave's stream (the running maximum), three lane merges,
    one wave merge.  Their exponents add up to M - s_k's complement along the path, so the exponent roundings are covered by ONE |s_k - M| term
    (hence 2 |s_k - M| with the key's own); each factor adds the ulp of v_exp_f32 and of the product: 2 n_stage.
    Accumulation: every accumulator (numerator per dim, normaliser) is a sum of positive-weighted terms of depth c = ceil(n_keys / (8 NW)) + 3
    + NW -- a lane's sequential fmas over its keys, three lane merges, the wave merge -- so c 2^-24 sum_k e_k |v_kd| for the numerator and
    c 2^-24 relative for the normaliser.  (The any-order c = n_keys is NOT used: at 1024 keys it alone is 6e-5 sum e|v| / sum e, which for
    a diffuse row with |o| ~ 0.1 is a tenth of a bf16 ulp and leaves 0.82-0.86 of the elements of the 1000-key rows stable; asserted under the
    reference alone in tests/test_decoder_kernels_cpu.py.  The depth is what the kernel's fixed partition gives and what the fp32 oracle's pairwise sums stay
    under as well.)  The normaliser's own accumulation term c 2^-24 |o| is added to the issue's formula: it is as real as the numerator's.
      beta_d = (sum_k delta_k e_k |v_kd| + c 2^-24 sum_k e_k |v_kd|) / sum e + |o_d| (sum_k delta_k e_k / sum e + c 2^-24 + 2^-23)
    two_term_p (multi-channel kernel): p = p_hi + p_lo with |e - p_hi| <= 2^-8 e and p_lo = bf16 of that remainder: 2^-16 e_k per key, and the
    MFMA accumulates T / 4 keys per wave in its own order: c = T / 4 + 4 there."""
    s, M, e, l, live, k, v = (parts[x] for x in ("s", "M", "e", "l", "live", "k", "v"))
    ab = torch.einsum("pd,pkd->pk", q.double().abs(), k.abs())
    if bias is not None:
        ab = ab + torch.where(live, bias.double().abs(), torch.zeros((), dtype=F64))
    nf = n.double()
    n_stage = torch.ceil(nf / (8 * NW * U)) + 4
    gap = torch.where(live, (s - M).abs(), torch.zeros((), dtype=F64))
    delta = 2.0 ** -23 * (ab + 2 * gap + 2 * n_stage[:, None] + 4)
    c = (torch.ceil(nf / (8 * NW)) + 3 + NW) if depth_c else nf
    if two_term_p:
        c = nf / 4 + 4
        delta = delta + 2.0 ** -16
    ev = torch.einsum("pk,pkd->pd", e, v.abs())
    dev = torch.einsum("pk,pkd->pd", delta * e, v.abs())
    return (dev + c[:, None] * 2.0 ** -24 * ev) / l + parts["o"].abs() * ((delta * e).sum(-1, keepdim=True) / l + c[:, None] * 2.0 ** -24 + 2.0 ** -23)


FORMS = {  # form -> (self, NW, U)
    "self8": (True, 8, 6), "self2": (True, 2, 6), "wo": (True, 8, 6), "beam8": (True, 8, 6), "beam2": (True, 2, 6),
    "cross8": (False, 8, 4), "cross2": (False, 2, 4), "fused": (False, 8, 4), "fused_ipart": (False, 8, 4), "mc": (False, 4, 4),
}


def gather_pairs(c, mutant=None):
    """A case -> per (row, head) pair p = (r - row0) H + h: k, v (P, Nmax, 64), bias (P, Nmax) or None, n (P,).  The case holds kc / vc
    (kv_rows, H, L, 64) as the device sees them, n_keys (R,) for rows row0.., rows_per_kv, and for self-attention bias (H, L); beam: anc (2,
    anc_rows, pitch) uint8 and W.  Mutants: bias_by_key, bias_off_by_one, bias_next_head, skip_newest, stale_key, rows_per_kv_ignored,
    other_parity."""
    is_self = FORMS[c["form"]][0]
    R, H, L, row0 = c["R"], c["H"], c["L"], c["row0"]
    n = c["n_keys"].clone()
    rows = row0 + torch.arange(R)
    Nmax = min(L, int(n.max()) + (1 if mutant == "stale_key" else 0))
    keys = torch.arange(Nmax)
    if "anc" in c:
        W = c["W"]
        buf = (n - 1) & 1
        if mutant == "other_parity":
            buf = buf ^ 1
        holder = c["anc"][buf, rows][:, :Nmax].long().clamp(max=W - 1)             # (R, Nmax)
        src = (rows - rows % W)[:, None] + holder                                   # the physical row of every key
        k = c["kc"][src, :, keys[None, :]].permute(0, 2, 1, 3)                      # (R, Nmax, H, 64) -> (R, H, Nmax, 64)
        v = c["vc"][src, :, keys[None, :]].permute(0, 2, 1, 3)
    else:
        rpk = c["rows_per_kv"]
        kv_row = rows if (is_self and rpk == 1) else rows // rpk
        if mutant == "rows_per_kv_ignored":
            kv_row = rows % c["kc"].shape[0]
        k, v = c["kc"][kv_row][:, :, :Nmax], c["vc"][kv_row][:, :, :Nmax]
    k, v = k.reshape(R * H, Nmax, 64), v.reshape(R * H, Nmax, 64)
    n = n.repeat_interleave(H)
    bias = None
    if is_self:
        tab = c["bias"].roll(-1, 0) if mutant == "bias_next_head" else c["bias"]    # (H, L)
        dist = n[:, None] - 1 - keys[None, :]
        if mutant == "bias_by_key":
            dist = keys[None, :].expand(R * H, -1)
        if mutant == "bias_off_by_one":
            dist = dist + 1
        idx = dist.clamp(0, L - 1)
        bias = tab.repeat(R, 1)[torch.arange(R * H)[:, None], idx]
    if mutant == "skip_newest":
        n = (n - 1).clamp(min=1)
    if mutant == "stale_key":
        n = (n + 1).clamp(max=L)
    return k, v, bias, n


def attention_reference(c, q=None, dtype=F64, mutant=None):
    """(parts, beta) of a case for query rows q (P, 64) (default: the case's own q (R, H, 64)); beta only for the float64 reference itself"""
    _, NW, U = FORMS[c["form"]]
    k, v, bias, n = gather_pairs(c, mutant)
    q = c["q"].reshape(-1, 64) if q is None else q
    parts = attention_model(q, k, v, bias, n, dtype, mutant, NW)
    if dtype != F64 or mutant:
        return parts, None
    return parts, attention_beta(q, parts, bias, n, NW, U, two_term_p=c["form"] == "mc")


def attention_simulate(c, dtype=torch.float32, mutant=None):
    """a device's `out` (R, H, 64) bf16 under the model in `dtype`; mutant trunc_out: the output truncated"""
    if "wq" in c:
        q = rb(fused_query(c, dtype, mutant)["q_pre"]).reshape(-1, 64)
    else:
        q = None
    parts, _ = attention_reference(c, q, dtype, mutant or "none")
    o = parts["o"]
    out = trunc_bf16(o) if mutant == "trunc_out" else rb(o)
    return out.bfloat16().reshape(c["R"], c["H"], 64)


def check_attention(c, ref, beta, got):
    """got (R, H, 64) bf16 against the reference of a plain (non-fused) case"""
    return check_bf16(got.reshape(-1, 64), ref["o"], beta)


# ----------------------------------------------------------------------------- fused query projection
def fused_query(c, dtype=F64, mutant=None):
    """q_pre (R, H, 64) = R(x scale gain) . wq[h]^T before its rounding, with beta_q and the flippable operand elements (float64 only).
    x: the residual rows, or f32(h + (((p0 + p1) + ...) + p7)) when the case holds ipart (R, 8, 512), with sum(x^2) from that x."""
    x = c["x"].float()
    if c.get("ipart") is not None:
        sp = c["ipart"][:, 0].float().clone()
        for w in range(1, 7 if mutant == "part_7" else 8):
            sp = sp + c["ipart"][:, w].float()
        x = x + sp
        ms = x.to(dtype).pow(2).sum(-1) / 512
    else:
        parts = c["ssq"].to(dtype)
        ms = (parts[:31] if mutant == "ssq_31" else parts).sum(0) / 512
    xn, pre = norm_operand(x, c["gain"], ms, c["eps"], dtype, mutant)
    wq = c["wq"].to(dtype)
    q_pre = (xn @ wq.T).reshape(x.shape[0], c["H"], 64)
    res = dict(q_pre=q_pre, xn=xn, pre=pre)
    if dtype == F64 and not mutant:
        flip = norm_flippable(pre, 512)
        res["beta_q"] = gemm_beta(xn, pre, c["wq"], flip).reshape(q_pre.shape)
    return res


MAX_ENUM = 3


def query_candidates(q_pre, beta_q):
    """(cands (8, P, 64), left_out (P,)).  An element of q is unstable when [q_pre - beta_q, q_pre + beta_q] rounds two ways; a pair with at
    most MAX_ENUM of them gets every combination of both roundings (8 slots; fewer unstable elements repeat combinations), a pair with more
    is left out."""
    P = q_pre.numel() // 64
    q_pre, beta_q = q_pre.reshape(P, 64), beta_q.reshape(P, 64)
    lo, hi = rb(q_pre - beta_q), rb(q_pre + beta_q)
    unstable = lo != hi
    cnt = unstable.sum(-1)
    left_out = cnt > MAX_ENUM
    rank = torch.cumsum(unstable.long(), -1) - 1                                    # index of an unstable element among its pair's
    cands = []
    for bits in itertools.product((0, 1), repeat=MAX_ENUM):
        b = torch.tensor(bits)[rank.clamp(0, MAX_ENUM - 1)]
        cands.append(torch.where(unstable & (b == 1), hi, torch.where(unstable, lo, rb(q_pre))))
    return torch.stack(cands), left_out, unstable


def fused_reference(c):
    """everything check_fused needs, from the reference alone: per candidate the attention parts' o and beta, the left-out pairs"""
    fq = fused_query(c)
    cands, left_out, unstable = query_candidates(fq["q_pre"], fq["beta_q"])
    os_, betas = [], []
    for q in cands:
        parts, beta = attention_reference(c, q)
        os_.append(parts["o"])
        betas.append(beta)
    return dict(o=torch.stack(os_), beta=torch.stack(betas), left_out=left_out, q_unstable_share=float(unstable.double().mean()), fq=fq)


def check_fused(fr, got):
    """The candidate rule: a (row, head) pair passes when the device's 64 outputs meet the criterion against ONE candidate query.  The figures
    are those of each pair's best candidate (fewest bad elements, then smallest worst error / allowance)."""
    P = fr["o"].shape[1]
    g = got.reshape(P, 64)
    best = None
    for o, beta in zip(fr["o"], fr["beta"]):
        stable, bs, bu, err, allow, ro = judge_bf16(g, o, beta)
        bad = (bs | bu).sum(-1)
        worst = torch.where(stable, torch.zeros((), dtype=F64), err / allow).max(-1).values
        cur = dict(bad=bad, worst=worst, stable=stable.double().mean(-1), bs=bs.sum(-1), bu=bu.sum(-1),
                   differ=(~stable & (g.double() != ro)).sum(-1))
        if best is None:
            best = cur
        else:
            take = (cur["bad"] < best["bad"]) | ((cur["bad"] == best["bad"]) & (cur["worst"] < best["worst"]))
            best = {k_: torch.where(take, cur[k_], best[k_]) for k_ in cur}
    keep = ~fr["left_out"]
    return dict(elements=int(keep.sum()) * 64, left_out_share=float(fr["left_out"].double().mean()),
                stable_share=float(best["stable"][keep].mean()) if bool(keep.any()) else 1.0,
                stable_wrong=int(best["bs"][keep].sum()), unstable_wrong=int(best["bu"][keep].sum()), unstable_differ=int(best["differ"][keep].sum()),
                worst_err_over_allowance=float(best["worst"][keep].max()) if bool(keep.any()) else 0.0, ok=not bool(best["bad"][keep].any()))


# ----------------------------------------------------------------------------- inputs
TAILS_8WAVE = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 319, 320, 321, 383, 384, 385, 447, 448, 449, 767, 768, 769, 1023, 1024]
TAILS_2WAVE = [1, 15, 16, 17, 95, 96, 97, 111, 112, 113, 191, 192, 193, 1024]
TAILS_STEP = [1, 65, 384, 385, 1024]            # again through `step` (lock-step), row0 != 0
CROSS_KEYS = [1, 17, 128, 250, 256, 257, 512, 1500]
FUSED_KEYS = [128, 256, 512]
MC_T = [128, 256, 512]
MC_CHANNELS = [2, 3, 13, 16]
NAN = float("nan")


def _fill_beyond(kc, vc, rows_n):
    """every cache position >= n_keys of a row holds NaN in K and V"""
    for r, n in enumerate(rows_n):
        kc[r, :, int(n):] = NAN
        vc[r, :, int(n):] = NAN


def self_case(form, n_keys, H=2, L=1024, row0=0, qs=0.5, bs=0.5, seed=0, W=4):
    """Random self-attention rows, one per entry of n_keys (row r of the launch decodes position n_keys[r] - 1).  q of std qs against k of
    std 1: scores of std 8 qs, neither one-hot nor uniform at qs = 0.5; v of std 1.  Cache rows [0, row0) hold NaN throughout.
    beam forms: R is padded to whole groups of W; holder bytes are random in [0, W + 2) (entries >= W are clamped by the kernel), both parity
    buffers differ, and K / V of position p are random in every row of the group."""
    n = torch.tensor(n_keys)
    beam = form.startswith("beam")
    if beam and len(n) % W:
        n = torch.cat([n, n[: W - len(n) % W]])
    R = len(n)
    g = torch.Generator().manual_seed(seed + 17 * R + H + int(100 * qs) + (7 if beam else 0))
    rows = row0 + R
    q = torch.full((rows, H, 64), NAN)
    q[row0:] = torch.randn(R, H, 64, generator=g) * qs
    kc = torch.randn(rows, H, L, 64, generator=g)
    vc = torch.randn(rows, H, L, 64, generator=g)
    c = dict(form=form, R=R, H=H, L=L, row0=row0, rows_per_kv=1, n_keys=n, bias=(torch.randn(H, L, generator=g) * bs).contiguous())
    if beam:
        pitch = L + 16
        c.update(W=W, anc=torch.randint(0, W + 2, (2, rows, pitch), generator=g, dtype=torch.uint8), anc_rows=rows, anc_pitch=pitch)
        grp = (torch.arange(R) // W) * W
        nmax = torch.stack([n[grp + j] for j in range(W)]).max(0).values        # a key below a group's largest count may be addressed
        kc[:row0], vc[:row0] = NAN, NAN
        _fill_beyond(kc[row0:], vc[row0:], nmax)
    else:
        kc[:row0], vc[:row0] = NAN, NAN
        _fill_beyond(kc[row0:], vc[row0:], n)
    c.update(q=q.bfloat16()[row0:], q_dev=q.bfloat16(), kc=kc.bfloat16(), vc=vc.bfloat16())
    return c


def cross_case(form, n_keys_const, R=5, H=2, rows_per_kv=1, row0=0, qs=0.5, seed=0, slab_extra=3):
    """Random cross-attention rows: slab_keys = n_keys_const + slab_extra, the positions beyond n_keys_const hold NaN"""
    g = torch.Generator().manual_seed(seed + 31 * n_keys_const + R + H + rows_per_kv)
    rows = row0 + R
    L = n_keys_const + slab_extra
    kv_rows = (rows - 1) // rows_per_kv + 1
    q = torch.full((rows, H, 64), NAN)
    q[row0:] = torch.randn(R, H, 64, generator=g) * qs
    kc = torch.randn(kv_rows, H, L, 64, generator=g)
    vc = torch.randn(kv_rows, H, L, 64, generator=g)
    kc[:, :, n_keys_const:], vc[:, :, n_keys_const:] = NAN, NAN
    return dict(form=form, R=R, H=H, L=L, row0=row0, rows_per_kv=rows_per_kv, n_keys=torch.full((R,), n_keys_const), q=q.bfloat16()[row0:],
                q_dev=q.bfloat16(), kc=kc.bfloat16(), vc=vc.bfloat16())


def fused_case(form, T, R=6, H=8, rows_per_kv=1, row0=0, seed=0, slab_extra=0):
    """The fused query projection on sign-coherent operands (module docstring of the issue: with plain randn operands 38 % of the q elements
    are unstable and every pair is left out): x = |randn| 2^e_r, gain > 0, row (h, o) of wq = sign |randn| 2^-6, so |q| ~ 0.5 sqrt(...) ~ a
    few tenths to a few units and the softmax over T keys of std-1 k is neither one-hot nor uniform.  form fused_ipart: x = h + sum of eight
    partial rows.  mc: R = n_seg n_channels, rows_per_kv = n_channels."""
    g = torch.Generator().manual_seed(seed + 13 * T + R + 3 * rows_per_kv + (5 if form == "mc" else 0))
    c = cross_case(form, T, R, H, rows_per_kv, row0, 0.0, seed, slab_extra)
    rows = row0 + R
    x = torch.full((rows, 512), NAN)
    x[row0:] = torch.randn(R, 512, generator=g).abs() * torch.exp2(torch.randint(-2, 3, (R, 1), generator=g).float())
    sign = torch.where(torch.rand(H * 64, generator=g) < 0.5, -1.0, 1.0)
    c["wq"] = (torch.randn(H * 64, 512, generator=g).abs() * sign[:, None] * 2.0 ** -9).bfloat16()
    c["gain"] = 0.5 + torch.rand(512, generator=g)
    c["eps"] = 1e-3
    if form == "mc":       # the two-term p costs 2^-16 sum p|v|: V of mean 1 keeps |o| near sum p|v| and 0.95 of the elements stable
        c["vc"] = (c["vc"].float() + 1.0).bfloat16()
    c["x_dev"] = x
    c["x"] = x[row0:]
    if form == "fused_ipart":
        ip = torch.full((rows, 8, 512), NAN)
        ip[row0:] = torch.randn(R, 8, 512, generator=g).abs() * 0.03
        c["ipart_dev"], c["ipart"] = ip, ip[row0:]
    else:
        ssq = torch.full((SSQ_TILES, rows), NAN)
        ssq[:, row0:] = ssq_partials(x[row0:])
        c["ssq_dev"], c["ssq"] = ssq, ssq[:, row0:]
    del c["q"], c["q_dev"]
    return c


# ----------------------------------------------------------------------------- exact probes
def hot_code(key):
    """two hot coordinates from disjoint ranges: key % 32 and 32 + key / 32 (keys below 1024)"""
    return key % 32, 32 + key // 32


def score_probe(form, n_keys, H=2, L=1024, row0=0, target=None, W=4, seed=0):
    """q[r, h] = 16 (e_a + e_b) with (a, b) = hot_code(target key), k[key] = 16 (e_a' + e_b'): the target scores 512, a key sharing one
    coordinate 256, the others 0, the bias is 0: the softmax is one-hot in fp32 (exp(-256) = 0) and the row returns v[target] bit for bit.
    v = (3 key + d + 7 h + 11 slab row) mod 251.  target (R, H) defaults to (37 r + 101 h + 5) mod n_keys[r]; 'newest': n_keys - 1.
    beam forms: the holder of key p in row r is (r + p + buffer) mod W for p < n (and W + 1, clamped to W - 1, at p = 1 of odd rows); K is the
    same in every row, V carries the row, so the returned codes name the holder."""
    c = self_case(form, n_keys, H, L, row0, 0.0, 0.0, seed, W)
    R, n = c["R"], c["n_keys"]
    rows = row0 + R
    r_, h_ = torch.meshgrid(torch.arange(R), torch.arange(H), indexing="ij")
    if target is None:
        target = (37 * r_ + 101 * h_ + 5) % n[:, None]
    elif isinstance(target, str):
        target = (n[:, None] - 1).expand(R, H)
    a, b = hot_code(target)
    q = torch.zeros(rows, H, 64)
    q[row0:] = torch.zeros(R, H, 64).scatter_(2, a[..., None], 16.0).scatter_(2, b[..., None], 16.0)
    keys = torch.arange(L)
    ka, kb = hot_code(keys)
    k1 = torch.zeros(L, 64)
    k1[keys, ka] = 16.0
    k1[keys, kb] = 16.0
    kc = k1[None, None].expand(rows, H, L, 64).clone()
    rr, hh, kk, dd = torch.meshgrid(torch.arange(rows), torch.arange(H), keys, torch.arange(64), indexing="ij")
    vc = ((3 * kk + dd + 7 * hh + 11 * rr) % 251).float()
    if "anc" in c:
        anc = torch.zeros(2, rows, c["anc_pitch"], dtype=torch.long)
        p = torch.arange(c["anc_pitch"])
        for buf in range(2):
            anc[buf] = (torch.arange(rows)[:, None] + p[None, :] + buf) % W
        anc[:, 1::2, 1] = W + 1
        c["anc"] = anc.to(torch.uint8)
        grp = (torch.arange(R) // W) * W
        nmax = torch.stack([n[grp + j] for j in range(W)]).max(0).values
    else:
        nmax = n
    kc[:row0], vc[:row0] = NAN, NAN
    _fill_beyond(kc[row0:], vc[row0:], nmax)
    c.update(q=q.bfloat16()[row0:], q_dev=q.bfloat16(), kc=kc.bfloat16(), vc=vc.bfloat16(), bias=torch.zeros(H, L), target=target)
    return c


def probe_want(c):
    """the V row every (row, head) of a score probe must return, gathered the way the contract addresses it (beam: through the table)"""
    k, v, _, n = gather_pairs(c)
    t = c["target"].reshape(-1)
    return v[torch.arange(v.shape[0]), t].reshape(c["R"], c["H"], 64)


BIAS_PROBE_N = [1024, 1023, 385, 9]
_BIAS_BASE = {}


def bias_probe_base(form, H=64, L=1024, W=4):
    """what every launch of a bias-probe sweep shares (built once per form): the score probe's K / V with q = 0, the V of every (row, head)
    gathered as the contract addresses it, and the mean of each pair's n keys (the output wherever no key lies at the peak's distance)"""
    if (form, H, L, W) not in _BIAS_BASE:
        c = score_probe(form, BIAS_PROBE_N, H, L, 0, None, W)
        q = torch.zeros_like(c["q_dev"])
        c.update(q=q, q_dev=q)
        _, v, _, n = gather_pairs(c)
        live = torch.arange(v.shape[1])[None, :] < n[:, None]
        vz = torch.where(live[..., None], v.double(), torch.zeros((), dtype=F64))
        c.update(gv=v, n_pair=n, mean_v=vz.sum(1) / n[:, None].double())
        _BIAS_BASE[(form, H, L, W)] = c
    return _BIAS_BASE[(form, H, L, W)]


def bias_probe(form, launch, H=64, L=1024, W=4):
    """q = 0, so every score is its bias; head h's table row is 0 at distance p_h = (H launch + h) mod L and -256 elsewhere.  Row r (n_keys =
    BIAS_PROBE_N[r]) with p_h < n returns v[n - 1 - p_h] exactly, the others the mean of their n keys' V.  ceil(L / H) launches make every
    distance the lone peak of the first row (n = L) once."""
    base = bias_probe_base(form, H, L, W)
    peak = (H * launch + torch.arange(H)) % L
    bias = torch.full((H, L), -256.0)
    bias[torch.arange(H), peak] = 0.0
    t = base["n_keys"][:, None] - 1 - peak[None, :]
    return dict(base, bias=bias, target=torch.where(t >= 0, t, torch.full_like(t, -1)), peak=peak)


def bias_probe_launches(H=64, L=1024):
    return -(-L // H)


def check_bias_probe(c, got):
    """rows with a key at the peak's distance return its V bit for bit; the others have all scores EQUAL (-256): every e is exp(0) = 1 exactly
    and o = mean of V, with attention_beta's terms for q = 0, |bias| = 256, no gap: delta = 2^-23 (256 + 2 n_stage + 4), depth c"""
    _, NW, U = FORMS[c["form"]]
    t = c["target"].reshape(-1)
    hit = t >= 0
    g = got.reshape(-1, 64)
    want = c["gv"][torch.arange(t.numel()), t.clamp(min=0)]
    recs = [exact("one-hot rows", g[hit].float(), want[hit].float())]
    if not bool(hit.all()):
        n = c["n_pair"][~hit].double()[:, None]
        o = c["mean_v"][~hit]                                      # V >= 0: mean |v| = o
        cdepth = torch.ceil(n / (8 * NW)) + 3 + NW
        delta = 2.0 ** -23 * (256 + 2 * (torch.ceil(n / (8 * NW * U)) + 4) + 4)
        recs.append(check_bf16(g[~hit], o, o * (2 * delta + 2 * cdepth * 2.0 ** -24 + 2.0 ** -23)))
    rec = merge(recs)
    rec["exact_row_share"] = float(hit.double().mean())
    return rec


def check_probe(c, got):
    """rows with a target equal its V bit for bit; the others (bias probe: no key at the peak's distance) meet the criterion of the reference"""
    t = c["target"]
    hit = t >= 0
    cc = dict(c, target=t.clamp(min=0))
    want = probe_want(cc)
    recs = [exact("one-hot rows", got[hit].float(), want[hit].float())]
    if not bool(hit.all()):
        parts, beta = attention_reference(c)
        miss = ~hit.reshape(-1)
        recs.append(check_bf16(got.reshape(-1, 64)[miss], parts["o"][miss], beta[miss]))
    rec = merge(recs)
    rec["exact_row_share"] = float(hit.double().mean())
    return rec


def wo_permutation(H=8):
    """wo [512][H 64] with wo[8 d + h][64 h + d] = 2^(h % 3 - 1) and zeros elsewhere: opart[r][h][8 d + h] = 2^(h % 3 - 1) R(o)_d exactly,
    every other column of the partial an exact +0"""
    wo = torch.zeros(512, H * 64)
    h, d = torch.meshgrid(torch.arange(H), torch.arange(64), indexing="ij")
    wo[8 * d + h, 64 * h + d] = torch.exp2((h % 3 - 1).float())
    return wo.bfloat16()


def out_from_opart(opart):
    """(R, 8, 512) fp32 partials under wo_permutation -> (out (R, 8, 64) bf16, all other columns are +0)"""
    R = opart.shape[0]
    h, d = torch.meshgrid(torch.arange(8), torch.arange(64), indexing="ij")
    val = opart[:, h, 8 * d + h] / torch.exp2((h % 3 - 1).float())
    rest = opart.clone()
    rest[:, h, 8 * d + h] = 0.0
    clean = bool((rest == 0).all()) and bool((val == val.bfloat16().float()).all())
    return val.bfloat16(), clean


def fused_probe(form, T=256, H=8, row0=0, n_channels=1):
    """The exact regime of the fused query: row r has x = c_r e_j (j = r mod 512, c_r a power of two), sum(x^2) = c_r^2 in tile j / 16, eps = 0,
    gain 2^(j % 3 - 1): xn_j = R(sqrt(512) g_j) = 22.625 g_j whatever the ulp of the root.  Column j of wq holds, in head h, 1 at the two rows
    of key(j, h)'s hot pair and zeros elsewhere, so q[h] = 22.625 g_j (e_a + e_b) exactly -- the products with the other columns are exact zeros --
    and against k = 16 (e_a' + e_b') the key scores 724 g_j, a key sharing one coordinate half of it: it wins by >= 181 and the row returns
    v[key] bit for bit (exp(-181) < 2^-149 / 2^-24 ... is 0 in fp32 against 1).  key(j, h) = (29 j + 7 h + 5) mod T with the hot pair (key % 32, 32 + (5 (key % 32) + key / 32) % 32), unique
    per key and covering all 64 head dims from T = 32 on: over j and h every (head row, k chunk, output of a wave) is the hot one -- the
    projection's whole index map, exactly."""
    R = 512 if n_channels == 1 else (512 // n_channels) * n_channels
    c = cross_case(form, T, R, H, n_channels, row0, 0.0, 0, 0)
    rows = row0 + R
    j = torch.arange(R) % 512
    x = torch.zeros(rows, 512)
    cval = torch.exp2((torch.arange(R) % 7 - 3).float())
    x[row0 + torch.arange(R), j] = cval
    gain = torch.exp2((torch.arange(512) % 3 - 1).float())
    hh, jj = torch.meshgrid(torch.arange(H), torch.arange(512), indexing="ij")
    key = (29 * jj + 7 * hh + 5) % T
    a, b = key % 32, 32 + (5 * (key % 32) + key // 32) % 32
    wq = torch.zeros(H, 64, 512)
    wq[hh, a, jj] = 1.0
    wq[hh, b, jj] = 1.0
    keys = torch.arange(T)
    kc = torch.zeros(c["kc"].shape[0], H, T, 64)
    hk, kk = torch.meshgrid(torch.arange(H), keys, indexing="ij")
    kc[:, hk, kk, kk % 32] = 16.0
    kc[:, hk, kk, 32 + (5 * (kk % 32) + kk // 32) % 32] = 16.0
    rr, h2, k2, dd = torch.meshgrid(torch.arange(kc.shape[0]), torch.arange(H), keys, torch.arange(64), indexing="ij")
    vc = ((3 * k2 + dd + 7 * h2 + 11 * rr) % 251).float()
    ssq = torch.zeros(SSQ_TILES, rows)
    ssq[:, row0:] = ssq_partials(x[row0:])
    c.update(kc=kc.bfloat16(), vc=vc.bfloat16(), wq=wq.reshape(H * 64, 512).bfloat16(), gain=gain, eps=0.0, x_dev=x, x=x[row0:], ssq_dev=ssq,
             ssq=ssq[:, row0:], target=key.T[j].contiguous())
    del c["q"], c["q_dev"]
    return c


# ============================================================================= the cases both modules run
def attention_cases():
    """name -> thunk of a random case (the GPU module runs every one; the CPU module checks the caps and the fp32 oracle on every one)"""
    out = {}
    out["self8_tails"] = lambda: self_case("self8", TAILS_8WAVE)
    out["self2_tails"] = lambda: self_case("self2", TAILS_2WAVE)
    out["wo_tails"] = lambda: self_case("wo", TAILS_8WAVE, H=8, seed=1)
    out["beam8_tails"] = lambda: self_case("beam8", TAILS_8WAVE, seed=2)
    out["beam2_tails"] = lambda: self_case("beam2", TAILS_2WAVE, seed=3)
    for n in TAILS_STEP:                          # lock-step: every row at the same position, read from `step`; row0 != 0
        out[f"self8_step_n{n}"] = (lambda n=n: self_case("self8", [n] * 3, row0=2, seed=4))
        out[f"self2_step_n{n}"] = (lambda n=n: self_case("self2", [n] * 3, row0=2, seed=5))
    out["self8_sharp"] = lambda: self_case("self8", [3, 200, 1024], qs=4.0, bs=20.0, seed=6)
    for i, n in enumerate(CROSS_KEYS):
        for form in ("cross8", "cross2"):
            rpk, row0 = (1, 3)[(i + (form == "cross2")) % 2], (0, 3)[i % 2]
            out[f"{form}_n{n}_rpk{rpk}_row{row0}"] = (lambda form=form, n=n, rpk=rpk, row0=row0: cross_case(form, n, 5, 2, rpk, row0))
    return out


def fused_cases():
    out = {}
    for i, T in enumerate(FUSED_KEYS):
        for form in ("fused", "fused_ipart"):
            rpk, row0 = (1, 3)[(i + (form == "fused")) % 2], (3, 6)[i % 2]
            out[f"{form}_T{T}_rpk{rpk}_row{row0}"] = (lambda form=form, T=T, rpk=rpk, row0=row0: fused_case(form, T, 6, 8, rpk, row0, slab_extra=0))
    for T in MC_T:
        for j, nc in enumerate(MC_CHANNELS):
            n_seg = (3, 1)[j % 2]
            row0 = (nc, 0)[j % 2] if T != 256 else (0, nc)[j % 2]
            out[f"mc_T{T}_c{nc}_seg{n_seg}_row{row0}"] = (lambda T=T, nc=nc, n_seg=n_seg, row0=row0: fused_case("mc", T, n_seg * nc, 8, nc, row0))
    return out


def gemm_cases():
    """name -> (mode, thunk of the case, launch arguments row0 / mid_rows / lockstep).  16-row-tile kernel: R in {1, 15, 16, 17, 33}, row0 in
    {0, 5}, N with and without a multiple of 8 column tiles, NT = 2 where N / 16 ceil(R / 16) > 320; mid-size tile kernel (mid_rows = 1):
    R in {1, 31, 32, 33, 64, 65, 100} in every mode it instantiates."""
    out = {}
    H, L = 2, 8
    small = [(1, 0), (15, 5), (16, 0), (17, 5), (33, 0)]
    for R, row0 in small:
        out[f"qkv_R{R}_row{row0}"] = (DG_QKV, (lambda R=R: gemm_case(DG_QKV, R, 3 * H * 64, 512, H=H, L=L)), dict(row0=row0))
        out[f"bf16_R{R}_row{row0}"] = (DG_BF16, (lambda R=R: gemm_case(DG_BF16, R, 128, 512)), dict(row0=row0))
        out[f"relu_R{R}_row{row0}"] = (DG_RELU, (lambda R=R: gemm_case(DG_RELU, R, 48, 512)), dict(row0=row0))
        out[f"logits_R{R}_row{row0}"] = (DG_LOGITS, (lambda R=R: gemm_case(DG_LOGITS, R, 80, 512)), dict(row0=row0))
    out["qkv_lockstep_pos0"] = (DG_QKV, lambda: gemm_case(DG_QKV, 5, 384, 512, H=H, L=L, pos=torch.zeros(5, dtype=torch.long)), dict(row0=3, lockstep=True))
    out["qkv_lockstep_pos1"] = (DG_QKV, lambda: gemm_case(DG_QKV, 5, 384, 512, H=H, L=L, pos=torch.ones(5, dtype=torch.long)), dict(row0=0, lockstep=True))
    out["qkv_lockstep_last"] = (DG_QKV, lambda: gemm_case(DG_QKV, 5, 384, 512, H=H, L=L, pos=torch.full((5,), L - 1)), dict(row0=3, lockstep=True))
    out["qkv_rows_pos_edges"] = (DG_QKV, lambda: gemm_case(DG_QKV, 6, 384, 512, H=H, L=L, pos=torch.tensor([0, 1, L - 1, L - 1, 0, 1])), dict(row0=5))
    out["qkv_nt2_R49"] = (DG_QKV, lambda: gemm_case(DG_QKV, 49, 1536, 512, H=8, L=4), dict(row0=0))
    out["bf16_nt2_R33"] = (DG_BF16, lambda: gemm_case(DG_BF16, 33, 2048, 512), dict(row0=5))
    out["relu_nt2_R33"] = (DG_RELU, lambda: gemm_case(DG_RELU, 33, 2048, 512), dict(row0=0))
    out["logits_nt2_R33"] = (DG_LOGITS, lambda: gemm_case(DG_LOGITS, 33, 2048, 512), dict(row0=5))
    for K in (512, 1024, 2048):
        for part in (False, True):
            out[f"resid_K{K}{'_part' if part else ''}"] = (DG_RESID, (lambda K=K, part=part: gemm_case(DG_RESID, 17, 512, K, part=part)), dict(row0=5))
    out["resid_R33"] = (DG_RESID, lambda: gemm_case(DG_RESID, 33, 512, 512), dict(row0=0))
    out["qkv_pend"] = (DG_QKV, lambda: gemm_case(DG_QKV, 17, 384, 512, H=H, L=L, pend=True), dict(row0=5))
    out["qkv_pend_nt2"] = (DG_QKV, lambda: gemm_case(DG_QKV, 49, 1536, 512, H=8, L=4, pend=True), dict(row0=0))
    out["logits_pend"] = (DG_LOGITS, lambda: gemm_case(DG_LOGITS, 17, 80, 512, pend=True), dict(row0=5))
    out["qkv_table"] = (DG_QKV, lambda: gemm_case(DG_QKV, 33, 384, 512, H=H, L=L, table=True), dict(row0=5))
    for R in (1, 31, 32, 33, 64, 65, 100):
        row0 = (0, 5)[R % 2]
        out[f"mid_qkv_R{R}"] = (DG_QKV, (lambda R=R: gemm_case(DG_QKV, R, 384, 512, H=H, L=L)), dict(row0=row0, mid_rows=1))
        out[f"mid_bf16_R{R}"] = (DG_BF16, (lambda R=R: gemm_case(DG_BF16, R, 128, 512)), dict(row0=row0, mid_rows=1))
        out[f"mid_relu_R{R}"] = (DG_RELU, (lambda R=R: gemm_case(DG_RELU, R, 64, 512)), dict(row0=row0, mid_rows=1))
        out[f"mid_logits_R{R}"] = (DG_LOGITS, (lambda R=R: gemm_case(DG_LOGITS, R, 192, 512)), dict(row0=row0, mid_rows=1))
        out[f"mid_resid_K512_R{R}"] = (DG_RESID, (lambda R=R: gemm_case(DG_RESID, R, 512, 512)), dict(row0=row0, mid_rows=1))
        out[f"mid_resid_K2048_R{R}"] = (DG_RESID, (lambda R=R: gemm_case(DG_RESID, R, 512, 2048)), dict(row0=row0, mid_rows=1))
    return out
