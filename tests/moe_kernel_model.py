"""References, criteria and inputs for the per-kernel tests of the mixture-of-experts decoder FFN (tests/test_moe_kernels.py on the GPU through
ymt3_test_moe_stage, tests/test_moe_kernels_cpu.py for the model itself).  TEST INFRASTRUCTURE ONLY, CPU only.  The criterion (stable element =>
bit-exact, otherwise within beta + 1 bf16 ulp; fp32 outputs by error / beta) is tests/enc_kernel_model.py's, the norm operand and the GEMM bound
are tests/dec_kernel_model.py's; both are imported, not restated.

CONTRACTS, read off csrc/moe.hip (R(.) = round to nearest-even bf16; every sum fp32 on the device, float64 here).  Rows r in [row0, row0 + R),
pairs p in [0, 2R) at index 2 row0 + p of every pair-indexed buffer:

  stage 0 router   xn[r][k] = R(h[r][k] * rsqrt(sum_{t<32} ssq[t][r] / 512 + eps) * gain[k])
                   l[e] = sum_k xn[r][k] router[e][k], e < E           (experts 0..7: eight sequential 64-term fmas and a 3-step lane tree;
                                                                         experts 8..15: 64 lanes of 8 fmas and a 6-step tree -- two ORDERS)
                   (e0, e1) = the two largest l, a tie to the lower expert id (strict > while scanning e upwards, in both slots); the rule is
                   exact for logits that are exact in fp32 in either order; a mathematical tie of ordinary values need not be one in fp32
                   t = exp(l[e1] - l[e0]); gate[2r] = 1 / (1 + t), gate[2r + 1] = t / (1 + t)
  stage 1 wi       hidden[p] = R(max(acc, 0)),  acc = xn[row0 + (p >> 1)] . wi[sel[p]]^T                     (K = 512, N = 2048)
  stage 2 wo       y[p] = f32(gate[p] * f32(acc)),  acc = hidden[2 row0 + p] . wo[sel[p]]^T                   (K = 2048, N = 512)
                   expert e's pairs are found by a scan of sel (512 pairs per pass), ascending, in chunks of <= 16; a pair whose sel is
                   outside [0, E) belongs to nobody and is not written
  fp8 (stages 1, 2) per activation row: mx = max(amax |x|, 1e-12), inv = f32(448 / mx), q = e4m3_rne(f32(x * inv)),
                   s = f32(f32(mx / 448) * wscale[e]);  out = f32(acc * s) with acc = sum_k q_k wq[e][n][k] (products of two e4m3 values are
                   exact in fp32).  THE DIVISION: yourmt3_amd/build.py passes neither a fast-math flag nor
                   -fno-hip-fp32-correctly-rounded-divide-sqrt, so 448.0f / mx is the correctly rounded IEEE quotient (the v_div_scale /
                   v_div_fmas / v_div_fixup sequence): q is a function of the inputs alone, EXACT in the reference, and there is no flip term.
  stage 3 combine  h[r] = f32(h[r] + f32(y[2r] + y[2r + 1]))  (this order is the contract: bit for bit);  ssq[0][r] = sum_k h_new^2,
                   ssq[1..31][r] = 0

BOUNDS, each at its helper: router_beta (logits), gate_bound, gemm_beta (dec_kernel_model), fp8_beta, the combine's sum.  CAPS checked under the
reference alone by the CPU module: stable share >= MIN_STABLE and undecided router rows <= MAX_LEFT_OUT per case.
Every check takes the device's WHOLE buffers (rows below row0 included), pre-filled with SENT: what the launch must not write must still hold it.
Mutants (wrong kernels, `mutant=` of the simulate functions) are listed at MUTANTS.
"""
from __future__ import annotations

import torch

from dec_kernel_model import MAX_LEFT_OUT, SENT, exact, gemm_beta, merge, norm_flippable, norm_operand, pend_sum, ssq_partials  # noqa: F401
from enc_kernel_model import MIN_STABLE, check_bf16, check_f32, judge_bf16, rb, ulp_bf16  # noqa: F401
from value_regimes import gemm_operands  # noqa: F401 (the `negative` kind: the sign-coherent operands of the expert GEMM value case)

F64, F32 = torch.float64, torch.float32
D_MODEL, D_FF = 512, 2048
NAN = float("nan")
E4M3 = torch.float8_e4m3fn


def _named(rec, name):
    rec = dict(rec)
    rec["check"] = name
    return rec


def join(recs):
    """dec_kernel_model.merge plus the names of the checks that failed"""
    out = merge(recs)
    out["failed"] = [r.get("check", r.get("exact", "?")) for r in recs if not r["ok"]]
    for k in ("undecided_share", "worst_gate_err_over_bound"):
        if any(k in r for r in recs):
            out[k] = max(r.get(k, 0.0) for r in recs)
    return out


def untouched(name, x):
    """everything in x still holds the sentinel"""
    return _named(dict(elements=int(x.numel()), ok=bool((x.double() == SENT).all())), name + " untouched")


# ============================================================================= router
def top2(l, mutant=None):
    """(R, E) logits -> (R, 2) ids, best first, ties to the lower id.  Mutants tie_higher, swap_23 (the third in the second slot)."""
    E = l.shape[1]
    if mutant == "tie_higher":
        order = E - 1 - torch.argsort(-l.flip(1), dim=1, stable=True)
    else:
        order = torch.argsort(-l, dim=1, stable=True)
    if mutant == "swap_23" and E > 2:
        return order[:, [0, 2]]
    return order[:, :2]


def router_model(c, dtype=F64, mutant=None, xn=None):
    """rows [row0, row0 + R) of a router case -> dict(xn, pre, l, sel (R, 2), gate (R, 2)).  xn: take these normed rows (the device's own) for
    the logits.  Mutants: eps_outside, unrounded_xn (the logits from the unrounded operand), ignore_8_15, tie_higher, swap_23, gates_swapped,
    softmax_all."""
    row0, R, E = c["row0"], c["R"], c["E"]
    rows = slice(row0, row0 + R)
    ms = c["ssq"][:, rows].to(dtype).sum(0) / D_MODEL
    xr, pre = norm_operand(c["h"][rows], c["gain"], ms, c["eps"], dtype, "eps_outside" if mutant == "eps_outside" else None)
    op = xr if xn is None else xn.to(dtype)
    if mutant == "unrounded_xn":
        op = pre
    l = op @ c["router"].to(dtype).T
    lsel = l.clone()
    if mutant == "ignore_8_15":
        lsel[:, 8:] = -float("inf")
    sel = top2(lsel, mutant)
    return dict(xn=xr, pre=pre, l=l, sel=sel, gate=gates_of(l, sel, mutant))


def gates_of(l, sel, mutant=None):
    l0, l1 = l.gather(1, sel[:, :1]), l.gather(1, sel[:, 1:])
    if mutant == "softmax_all":
        p = torch.softmax(l, -1)
        return torch.cat([p.gather(1, sel[:, :1]), p.gather(1, sel[:, 1:])], 1)
    t = torch.exp(l1 - l0)
    g = torch.cat([1 / (1 + t), t / (1 + t)], 1)
    return g.flip(1) if mutant == "gates_swapped" else g


def router_simulate(c, dtype=F32, mutant=None):
    """what a device computing the model in `dtype` leaves in its whole buffers: xn (rows, 512) bf16, sel (2 rows,) int32, gate (2 rows,) f32.
    Mutant row0_ignored: the launch works on rows [0, R)."""
    row0, R = c["row0"], c["R"]
    rows = row0 + R
    cc = dict(c, row0=0) if mutant == "row0_ignored" else c
    m = router_model(cc, dtype, mutant)
    at = cc["row0"]
    xn = torch.full((rows, D_MODEL), SENT, dtype=torch.bfloat16)
    sel = torch.full((2 * rows,), int(SENT), dtype=torch.int32)
    gate = torch.full((2 * rows,), SENT, dtype=F32)
    xn[at:at + R] = rb(m["xn"]).bfloat16()
    sel[2 * at:2 * (at + R)] = m["sel"].reshape(-1).int()
    gate[2 * at:2 * (at + R)] = m["gate"].reshape(-1).float()
    return dict(xn=xn, sel=sel, gate=gate)


def router_beta(xn, router):
    """beta_l (R, E) of a logit formed from GIVEN bf16 rows: K 2^-24 sum |xn||w| -- the products are exact in fp32 and any summation order of K
    of them (either of the kernel's two) rounds each partial sum, none above sum |xn||w|, by 2^-24 (value_regimes.gemm_reference_and_bound)"""
    return D_MODEL * 2.0 ** -24 * (xn.double().abs() @ router.double().abs().T) + D_MODEL * 2.0 ** -149


def gate_bound(l0, l1, g, beta):
    """bound of an fp32 gate against softmax(l0, l1) in float64, d = l1 - l0:
      beta / 2                    each logit is off by at most beta, d by 2 beta, and |dg/dd| = g0 g1 <= 1/4
      g0 g1 2^-23 (2 |d| + 4)     __expf, as enc_kernel_model.attention_beta takes it for softmax's p (the product with log2(e) rounds the
                                  exponent by 2^-24 |d| log2(e), the subtraction d itself by 2^-24 |d|, v_exp_f32 is good to 1 ulp; the constant
                                  covers the fixed ulps): a relative error of t, which moves either gate by g0 g1 times it
      3 2^-24 g                   the roundings of 1 + t, of the reciprocal and of the quotient (correctly rounded division: module docstring)"""
    d = (l1 - l0).abs()
    g0g1 = g[:, 0] * g[:, 1]
    return (beta / 2 + g0g1 * 2.0 ** -23 * (2 * d + 4))[:, None] + 3 * 2.0 ** -24 * g + 2.0 ** -149


def check_router(c, got, ref=None):
    """The GPU test's whole check of one router launch on the device's whole buffers.  Named checks: xn (criterion on the norm operand),
    sel decided (decided rows equal the reference, order included), sel allowed (the others: an ordering beta_l allows), undecided cap,
    gate bound, gate order / range / sum, and `untouched` for everything outside the launch's rows."""
    row0, R, E = c["row0"], c["R"], c["E"]
    rows = slice(row0, row0 + R)
    ref = ref or router_model(c)
    recs = [untouched("xn below row0", got["xn"][:row0]), untouched("sel below row0", got["sel"][:2 * row0]),
            untouched("gate below row0", got["gate"][:2 * row0])]
    xn = got["xn"][rows]
    b = (D_MODEL / 64 + 8) * 2.0 ** -24 * ref["pre"].abs()              # dec_kernel_model.norm_flippable's interval, as a beta
    assert bool(((rb(ref["pre"] - b) != rb(ref["pre"] + b)) == norm_flippable(ref["pre"], D_MODEL)).all())
    recs.append(_named(check_bf16(xn, ref["pre"], b), "xn"))
    sel = got["sel"][2 * row0:2 * (row0 + R)].reshape(R, 2).long()
    gate = got["gate"][2 * row0:2 * (row0 + R)].reshape(R, 2).double()
    inside = bool(((sel >= 0) & (sel < E)).all())
    recs.append(_named(dict(elements=2 * R, ok=inside), "sel in range"))
    if not inside or not bool(torch.isfinite(xn.float()).all()):
        return join(recs)
    own = router_model(c, xn=xn)                                       # float64 logits from the DEVICE's xn: no operand flip in the decision
    l = own["l"]
    beta = router_beta(xn, c["router"]).max(-1).values
    top = l.sort(-1, descending=True).values
    gap12 = top[:, 0] - top[:, 1]
    gap23 = top[:, 1] - top[:, 2] if E > 2 else torch.full_like(gap12, float("inf"))
    decided = (gap12 > 2 * beta) & (gap23 > 2 * beta)
    same = (sel == own["sel"]).all(-1)
    recs.append(_named(dict(elements=int(decided.sum()), ok=bool(same[decided].all())), "sel decided"))
    a, bb = sel[:, :1], sel[:, 1:]
    la, lb = l.gather(1, a)[:, 0], l.gather(1, bb)[:, 0]
    rest = l.scatter(1, a, -float("inf"))
    allowed = (a[:, 0] != bb[:, 0]) & (la >= l.max(-1).values - 2 * beta) & (lb >= rest.max(-1).values - 2 * beta)
    recs.append(_named(dict(elements=int((~decided).sum()), ok=bool(allowed[~decided].all())), "sel allowed"))
    und = float((~decided).double().mean())
    recs.append(_named(dict(elements=R, ok=und <= MAX_LEFT_OUT, undecided_share=und), "undecided cap"))
    g = gates_of(l, sel)
    bound = gate_bound(la, lb, g, beta)
    err = (gate - g).abs()
    recs.append(_named(dict(elements=2 * R, ok=bool((err <= bound).all()), worst_gate_err_over_bound=float((err / bound).max())), "gate bound"))
    # order: exact on a decided row (t <= 1 there whatever the rounding); an undecided row may hold l1 > l0 by its noise
    order_ok = (gate[:, 0] >= gate[:, 1]) | ~decided
    shape_ok = order_ok & (gate >= 0).all(-1) & (gate <= 1).all(-1) & ((gate[:, 0] + gate[:, 1] - 1).abs() <= 2.0 ** -23)
    recs.append(_named(dict(elements=2 * R, ok=bool(shape_ok.all())), "gate order / range / sum"))
    return join(recs)


def _pad_rows(x, row0, fill=NAN):
    return torch.cat([torch.full((row0,) + tuple(x.shape[1:]), fill, dtype=x.dtype), x], 0)


def router_case(E, R, row0, seed=0, eps=1e-3):
    """h = randn times a per-row power of two from 2^-4 (mean squares from 2^-8: a misplaced eps of 1e-3 moves the scale by a fifth there), a
    positive gain, ssq = the partials of h, NaN below row0 and in the slack of ssq (stride = row0 + R + 3); router rows randn / 8: logits of std
    about 3, so the gates are not saturated and the top-3 gaps (about 3 / E) lie far above 2 beta_l (about 0.01)."""
    for draw in range(16):
        g = torch.Generator().manual_seed(seed + 1000 * E + 10 * R + row0 + 100000 * draw)
        h = torch.randn(R, D_MODEL, generator=g) * torch.exp2(torch.randint(-4, 3, (R, 1), generator=g).float())
        gain = (0.5 + torch.rand(D_MODEL, generator=g)) * torch.exp2(torch.randint(-1, 2, (D_MODEL,), generator=g).float())
        stride = row0 + R + 3
        ssq = torch.full((32, stride), NAN)
        ssq[:, row0:row0 + R] = ssq_partials(h)
        c = dict(E=E, R=R, row0=row0, eps=eps, h=_pad_rows(h, row0), gain=gain, ssq=ssq, stride=stride,
                 router=(torch.randn(E, D_MODEL, generator=g) / 8).bfloat16())
        if router_margin(c) > 8.0:
            return c
    raise AssertionError("no draw with every row decided")


def router_margin(c):
    """min over the rows of (the smaller of the top-3 gaps) / beta_l under the reference alone.  The cap on undecided rows leaves no room for
    one at R <= 9, and beta_l is a fixed fraction of the logits' spread whatever the router's scale, so router_case redraws until every gap
    is 8 beta_l or more: four times what `decided` asks, which the device's own xn (a flipped operand moves a logit by ulp_bf16(xn) |w|, of
    the order of beta_l) cannot undo."""
    m = router_model(c)
    top = m["l"].sort(-1, descending=True).values
    gap = torch.minimum(top[:, 0] - top[:, 1], top[:, 1] - top[:, 2]) if c["E"] > 2 else top[:, 0] - top[:, 1]
    return float((gap / router_beta(m["xn"], c["router"]).max(-1).values).min())


ROUTER_E, ROUTER_R, ROUTER_ROW0 = [2, 3, 8, 9, 16], [1, 7, 8, 9], [0, 5]
TIE_PAIRS = [(0, 1), (3, 5), (7, 8), (8, 15)]


def router_probe(E, row0=0, identical=False):
    """Exact logits in either summation order: router row e is one-hot (1.0 at column e; `identical`: at column 0 for every e), h holds small
    integers and ssq[0][r] = 512 / 4 with eps = 0, gain = 1: the scale is rsqrt(1 / 4) = 2 (an ulp more or less of the root is absorbed by
    the bf16 rounding of integers below 256), xn = 2 h exactly and l[e] = 2 h[r][e] -- one exact product and zeros.  The rows:
      per tie pair (a, b) with b < E: a tie for FIRST  (l[a] = l[b] = 6, the others below, distinct) -> sel (a, b), gates (0.5, 0.5);
                                      a tie for SECOND (l[c] = 206 at an expert c outside the pair, then l[a] = l[b] = 6) -> sel (c, a), and the gap
                                      of 200 gives gates (1, 0) exactly (exp(-200) is 0 in fp32);
      E > 2: a three-way tie of the LAST three experts for first -> the two lowest of them;
      identical: every logit equal -> sel (0, 1), gates (0.5, 0.5).
    Returns (case, want_sel (R, 2), want_gate (R, 2), want_xn (R, 512))."""
    hs, sels, gts = [], [], []
    base = -(torch.arange(D_MODEL) % 100 + 1).float()                  # distinct negative logits for the experts not named
    if identical:
        hrow = base.clone()
        hrow[0] = 3.0
        hs, sels, gts = [hrow], [(0, 1)], [(0.5, 0.5)]
    else:
        for a, b in TIE_PAIRS:
            if b >= E:
                continue
            hrow = base.clone()
            hrow[a] = hrow[b] = 3.0
            hs.append(hrow); sels.append((a, b)); gts.append((0.5, 0.5))
            if E > 2:
                cexp = next(e for e in (E - 1, 0, 1, 2) if e not in (a, b))
                hrow = base.clone()
                hrow[a] = hrow[b] = 3.0
                hrow[cexp] = 103.0
                hs.append(hrow); sels.append((cexp, a)); gts.append((1.0, 0.0))
        if E > 2:
            hrow = base.clone()
            hrow[E - 3:E] = 3.0
            hs.append(hrow); sels.append((E - 3, E - 2)); gts.append((0.5, 0.5))
    h = torch.stack(hs)
    R = h.shape[0]
    router = torch.zeros(E, D_MODEL)
    router[torch.arange(E), 0 if identical else torch.arange(E)] = 1.0
    stride = row0 + R
    ssq = torch.full((32, stride), NAN)
    ssq[:, row0:] = 0.0
    ssq[0, row0:] = D_MODEL / 4.0
    c = dict(E=E, R=R, row0=row0, eps=0.0, h=_pad_rows(h, row0), gain=torch.ones(D_MODEL), ssq=ssq, stride=stride, router=router.bfloat16())
    return c, torch.tensor(sels), torch.tensor(gts, dtype=F64), 2 * h


def check_router_probe(c, want, got):
    row0, R = c["row0"], c["R"]
    ws, wg, wx = want
    return join([exact("probe xn", got["xn"][row0:row0 + R].float(), wx), exact("probe sel", got["sel"][2 * row0:2 * (row0 + R)].reshape(R, 2).long(), ws),
                 exact("probe gates", got["gate"][2 * row0:2 * (row0 + R)].reshape(R, 2), wg),
                 untouched("xn below row0", got["xn"][:row0]), untouched("sel below row0", got["sel"][:2 * row0])])


# ============================================================================= expert GEMMs
def e4m3_values(q8):
    return q8.view(E4M3).float()


def trunc_e4m3(x):
    """the WRONG conversion (mutant fp8_trunc): toward zero onto the e4m3 grid (4 significant bits, exponents from 2^-6, at most 448)"""
    x = x.double()
    _, ex = torch.frexp(x.abs())
    step = torch.ldexp(torch.ones_like(x), (ex - 1).clamp(min=-6) - 3)
    return (torch.sign(x) * torch.floor(x.abs() / step) * step).clamp(-448, 448).float()


def quant_rows(x, mutant=None):
    """the kernel's per-row quantisation with its own fp32 operations (module docstring) -> (q as fp32 values (n, K), row scale mx / 448 (n, 1)).
    Both quotients are TRUE fp32 divisions, as the kernel's are.  oracle.quant_rows_fp8 writes the same formulas, but torch evaluates
    `448 / amax` as f32(reciprocal(amax) * 448) and `amax / 448` as amax * f32(1 / 448): two roundings each, an ulp off the quotient for some
    maxima, which moves q by one e4m3 step where x * inv lies within that ulp of a rounding boundary (tests/test_moe_kernels_cpu.py bounds
    the difference: the scales within one fp32 ulp, q equal but for such elements).  Mutants: amax_slice (every K / 8 slice by its own maximum, the row scale
    of slice 0), fp8_trunc, no_clamp."""
    x = x.float()
    n, K = x.shape
    c448 = torch.full((1, 1), 448.0)                  # (a tensor that is no scalar: torch divides by a SCALAR through its reciprocal)
    if mutant == "amax_slice":
        xs = x.reshape(n, 8, K // 8)
        mx = xs.abs().amax(-1, keepdim=True).clamp_min(1e-12)
        q = (xs * (c448 / mx)).to(E4M3).float().reshape(n, K)
        return q, mx[:, 0] / c448.expand(n, 1)
    mx = x.abs().amax(-1, keepdim=True)
    if mutant != "no_clamp":
        mx = mx.clamp_min(1e-12)
    prod = x * (c448 / mx)
    q = trunc_e4m3(prod) if mutant == "fp8_trunc" else prod.to(E4M3).float()
    return q, mx / c448.expand(n, 1)


QUANT = quant_rows              # what expert_model quantises with (tests/test_moe_kernels_cpu.py puts the oracle's own function here for its chain)


def _expert_weights(c, e, dtype):
    return (e4m3_values(c["w_q8"][e]) if c["fp8"] else c["w"][e]).to(dtype)


def expert_rows(c, p, mutant=None):
    """the activation row of every pair p (relative to the launch) in the device's whole buffer"""
    row0 = c["row0"]
    if c["stage"] == 1:
        r = row0 + (p if mutant == "row_p" else p >> 1)
    else:
        r = (row0 if mutant == "hidden_row0" else 2 * row0) + p
    return r.clamp(max=c["a"].shape[0] - 1)


def expert_model(c, dtype=F64, mutant=None):
    """acc-level model of one expert GEMM launch, following the kernel's walk (expert by expert, pairs ascending, chunks of 16) so that the
    mutants of the walk can be written.  -> dict(o (2R, N): the value before the output's rounding (stage 1: NOT clamped), beta (float64 without
    a mutant), written (2R,) bool, extra: {absolute pair index: row} written beyond the contract by a mutant).
    Mutants: row_p, hidden_row0, gate_other, ragged_written, second_chunk_first, drop_beyond_512, amax_slice, no_wscale, wscale_e0, fp8_trunc,
    no_clamp, row0_ignored."""
    st, E, R, fp8 = c["stage"], c["E"], c["R"], c["fp8"]
    if mutant == "row0_ignored":
        c = dict(c, row0=0)
    row0 = c["row0"]
    N, K = (D_FF, D_MODEL) if st == 1 else (D_MODEL, D_FF)
    sel = c["sel"][2 * row0:2 * (row0 + R)].long()
    o = torch.zeros(2 * R, N, dtype=dtype)
    beta = torch.zeros(2 * R, N, dtype=F64)
    written = torch.zeros(2 * R, dtype=torch.bool)
    extra = {}
    for e in range(E):
        plist = (sel == e).nonzero().flatten()
        if mutant == "drop_beyond_512":
            plist = plist[plist < 512]
        if not plist.numel():
            continue
        W = _expert_weights(c, e, dtype)
        for c0 in range(0, plist.numel(), 16):
            chunk = plist[c0:c0 + 16]
            src = plist[:chunk.numel()] if (mutant == "second_chunk_first" and c0) else chunk
            A = c["a"][expert_rows(c, src, mutant)]
            if fp8:
                q, xs = quant_rows(A, mutant) if mutant in ("amax_slice", "fp8_trunc", "no_clamp") else QUANT(A.float())
                ws = c["w_s"][0 if mutant == "wscale_e0" else e]
                s = xs if mutant == "no_wscale" else (xs * ws)                      # fp32, the kernel's own product
                acc = q.to(dtype) @ W.T
                val = acc * s.to(dtype)
                if dtype == F64 and not mutant:
                    beta[chunk] = fp8_beta(q, W, s, val)
            else:
                val = A.to(dtype) @ W.T
                if dtype == F64 and not mutant:
                    beta[chunk] = gemm_beta(A, A, c["w"][e])
            if st == 2:
                gt = c["gate"][2 * row0 + (chunk ^ 1 if mutant == "gate_other" else chunk)].to(dtype)[:, None]
                if dtype == F64 and not mutant:
                    beta[chunk] = gt.abs() * beta[chunk] + 2.0 ** -24 * (gt * val).abs()     # the gate product: one more fp32 rounding
                val = gt * val
            o[chunk] = val
            written[chunk] = True
            if mutant == "ragged_written" and chunk.numel() < 16:                # the chunk's 16 rows stored: the padding goes to the pairs after the last
                for j in range(16 - chunk.numel()):
                    extra[2 * row0 + int(chunk[-1]) + 1 + j] = val[-1]
    return dict(o=o, beta=beta, written=written, extra=extra, row0=row0)


def mfma_fp8_alignment_loss(q, W):
    """What v_mfma_f32_16x16x32_fp8_fp8 drops BEFORE its fp32 accumulation (n, N).  The instruction forms the 8 products of one lane's 64-bit
    operands (k = 8 g .. 8 g + 7) in a fixed-point window aligned to the largest of the 8: bits more than 13 places below that product's
    leading bit are cut off (toward zero), and only then does the group's sum enter the fp32 chain.  Measured through the door with exact
    operands (next to 448 * 256 = 1.75 2^16, a product 3.0625 2^j in the same group of 8 arrives as its multiple of 2^3
    below -- nothing of it below 2^3 -- while the same product in another group of 8, another MFMA or another wave arrives whole).  Products
    of similar size lose nothing (8 significant bits fit the window until a product is 2^6 below its group's largest), so this term is zero
    for most groups and is what a row with one dominant element costs.  Per product the cut is |p| mod 2^(e_max - 13); their sum bounds the
    loss."""
    n, K = q.shape
    P = (q.float()[:, None, :] * W.float()[None, :, :]).abs().reshape(n, W.shape[0], K // 8, 8)          # exact in fp32 (4 + 4 bits)
    _, ex = torch.frexp(P.amax(-1, keepdim=True))
    unit = torch.ldexp(torch.ones_like(P[..., :1]), ex - 14)                                              # 2^(floor(log2 max) - 13)
    return torch.fmod(P, unit).double().sum((-1, -2))


def fp8_beta(q, W, s, val):
    """beta of f32(acc * s): the K products q w are exact in fp32 (4 + 4 significant bits), so any-order accumulation costs K 2^-24 sum |q||w|
    (times s); s and the product with it add two roundings, 2 2^-24 |value|; q itself is exact (correctly rounded division: module docstring).
    Plus what the fp8 MFMA cuts off inside a group of 8 products before it accumulates (mfma_fp8_alignment_loss), times s."""
    K = q.shape[1]
    acc_term = K * 2.0 ** -24 * (q.double().abs() @ W.double().abs().T) + mfma_fp8_alignment_loss(q, W)
    return acc_term * s.double() + 2 * 2.0 ** -24 * val.double().abs() + K * 2.0 ** -149


def expert_simulate(c, dtype=F32, mutant=None):
    """the device's whole output buffer (2 rows, N) under the model in `dtype`: bf16 (stage 1) or f32 (stage 2), SENT where nothing is written.
    Mutant no_relu."""
    m = expert_model(c, dtype, mutant)
    st, R = c["stage"], c["R"]
    N = D_FF if st == 1 else D_MODEL
    rows = c["row0"] + R
    out = torch.full((2 * rows, N), SENT, dtype=torch.bfloat16 if st == 1 else F32)
    o = m["o"] if (st == 2 or mutant == "no_relu") else m["o"].clamp(min=0)
    vals = rb(o).bfloat16() if st == 1 else o.float()
    idx = 2 * m["row0"] + m["written"].nonzero().flatten()
    out[idx] = vals[m["written"]]
    for p, v in m["extra"].items():
        if p < out.shape[0]:
            out[p] = (rb(v.clamp(min=0)).bfloat16() if st == 1 else v.float())
    return out


def check_expert(c, got, ref=None):
    """one expert GEMM launch on the device's whole output buffer: the criterion on the written pairs (stage 1: bf16 with relu; stage 2: fp32
    against beta), SENT below the launch's pairs and in every pair whose sel is outside [0, E)"""
    ref = ref or expert_model(c)
    row0, R, st = c["row0"], c["R"], c["stage"]
    mine = got[2 * row0:2 * (row0 + R)]
    w = ref["written"]
    recs = [untouched("pairs below row0", got[:2 * row0]), untouched("pairs of no expert", mine[~w])]
    if st == 1:
        recs.append(_named(check_bf16(mine[w], ref["o"][w], ref["beta"][w], relu=True), "hidden"))
    else:
        recs.append(_named(check_f32(mine[w], ref["o"][w], ref["beta"][w]), "y"))
    return join(recs)


def _sel_buffer(sel, row0, E):
    """sel of the launch's pairs behind 2 row0 pairs that name VALID experts (a launch that ignores row0 then does something)"""
    return torch.cat([torch.arange(2 * row0) % E, sel]).int()


def expert_case(stage, fp8, E, R, row0, seed=0, sel=None):
    """Sign-coherent operands (dec_kernel_model.gemm_case): activations |randn| times a per-row power of two (stage 2: what a relu leaves),
    row n of every expert's matrix = sign_n |randn| / K (fp8: that, times 64, rounded to e4m3, with the per-expert scale 2^-6 (1 + 0.37 e)),
    gates in (0, 1).  sel: random over the experts unless given.  NaN in every activation row and gate below row0."""
    g = torch.Generator().manual_seed(seed + 100 * stage + 10 * E + R + row0 + (7 if fp8 else 0))
    N, K = (D_FF, D_MODEL) if stage == 1 else (D_MODEL, D_FF)
    sign = torch.where(torch.rand(E, N, generator=g) < 0.5, -1.0, 1.0)
    Wf = torch.randn(E, N, K, generator=g).abs() * sign[..., None] / K
    n_act = R if stage == 1 else 2 * R
    a = torch.randn(n_act, K, generator=g).abs() * torch.exp2(torch.randint(-3, 4, (n_act, 1), generator=g).float())
    if sel is None:
        sel = torch.randint(0, E, (2 * R,), generator=g)
    c = dict(stage=stage, fp8=fp8, E=E, R=R, row0=row0, a=_pad_rows(a.bfloat16(), row0 if stage == 1 else 2 * row0), sel=_sel_buffer(sel, row0, E),
             gate=_pad_rows(0.05 + 0.9 * torch.rand(2 * R, generator=g), 2 * row0))
    if fp8:
        c["w_q8"] = (Wf * K * 0.5).to(E4M3).view(torch.uint8)
        c["w_s"] = (2.0 ** -6 * (1 + 0.37 * torch.arange(E))).float()
    else:
        c["w"] = Wf.bfloat16()
    return c


def fp8_edge_case(stage):
    """17 pairs of expert 0 (slot 0 of 17 rows; slot 1 goes to expert 1), so its second chunk holds ONE pair whose row maximum is 2^-20 of the
    first chunk's first row (a row maximum kept from the chunk before is caught); row 1 all zero (zeros, not NaN); row 2 with its maximum in the last K / 8 slice, 2^6 above the
    rest; row 3 with a negative maximum; rows 4 and 5 in one chunk with maxima 2^20 apart."""
    R = 17
    c = expert_case(stage, True, 2, R, 0, seed=5, sel=torch.arange(2 * R) % 2)
    K = c["a"].shape[1]
    a = c["a"].float()
    pr = (lambda r: r) if stage == 1 else (lambda r: 2 * r)           # the activation row of row r's slot-0 pair
    a[pr(0)] *= 2.0 ** 10
    a[pr(16)] *= 2.0 ** -10
    a[pr(1)] = 0.0
    a[pr(2), K - 5] = a[pr(2)].max() * 64
    a[pr(3), 77] = -a[pr(3)].max() * 4
    a[pr(4)] *= 2.0 ** 10
    a[pr(5)] *= 2.0 ** -10
    c["a"] = a.bfloat16()
    return c


def alignment_probe_case():
    """Stage 2, fp8, every scale 1 (row maximum 448, weight scale 1, gate 1): next to q w = 448 * 256 at k = 3 each row holds ONE more
    product v c_n -- v, c_n = (1 or 1.75) 2^i over the normal e4m3 range -- at k = 5 (the same group of 8 products), k = 20 (another lane's
    group of the same MFMA), k = 40 (the next MFMA of the wave) or k = 556 (another wave).  In float64 y = 114688 + v c_n; fp8_beta allows
    the cut of mfma_fp8_alignment_loss in the first position and nothing but fp32 rounding in the others."""
    K, N = D_FF, D_MODEL
    rows = []
    for k1 in (5, 20, 40, 556):
        for i in range(-6, 9):
            for mant in (1.0, 1.75):
                x = torch.zeros(K)
                x[3], x[k1] = 448.0, mant * 2.0 ** i
                rows.append(x)
    A = torch.stack(rows)
    cn = torch.tensor([(1.0 if (n // 15) % 2 == 0 else 1.75) * 2.0 ** (n % 15 - 6) for n in range(N)])
    W = torch.zeros(2, N, K)
    W[:, :, [5, 20, 40, 556]] = cn[None, :, None]
    W[:, :, 3] = 256.0
    P = A.shape[0]
    return dict(stage=2, fp8=True, E=2, R=P // 2, row0=0, a=A.bfloat16(), sel=torch.zeros(P, dtype=torch.int32), gate=torch.ones(P),
                w_q8=W.to(E4M3).view(torch.uint8), w_s=torch.ones(2))


def check_alignment_probe(c, got):
    """two products per output, so fp32 accumulation rounds once: the rows whose small product shares the big one's group of 8 may lie BELOW
    the float64 value by mfma_fp8_alignment_loss (and a rounding), the others within a rounding of it"""
    ref = expert_model(c)
    o = ref["o"]
    n = o.shape[0] // 4
    q, _ = quant_rows(c["a"].float())
    loss = mfma_fp8_alignment_loss(q[:n], e4m3_values(c["w_q8"][0]))
    rnd = 2 * 2.0 ** -24 * o.abs()
    d = o - got.double()
    same = _named(dict(elements=int(d[:n].numel()), ok=bool(((d[:n] >= -rnd[:n]) & (d[:n] <= loss + rnd[:n])).all()),
                       worst_err_over_beta=float((d[:n].abs() / (loss + rnd[:n])).max())), "cut within the window")
    return join([same, _named(check_f32(got[n:], o[n:], rnd[n:]), "other groups whole"), _named(check_expert(c, got, ref), "y")])


EXPERT_RANDOM = [  # (name, stage, fp8, E, R, row0): both stages and forms at E in {2, 3}; 8 once; 16 once in the stage-1 bf16 form
    (f"s{st}_{'fp8' if f else 'bf16'}_E{E}_R{R}_row{row0}", st, f, E, R, row0)
    for st in (1, 2) for f in (False, True) for (E, R, row0) in ((2, 1, 0), (3, 9, 3), (2, 40, 0), (3, 40, 3))
] + [("s2_bf16_E8_R9_row0", 2, False, 8, 9, 0), ("s1_fp8_E8_R9_row3", 1, True, 8, 9, 3), ("s1_bf16_E16_R9_row0", 1, False, 16, 9, 0)]


# ----------------------------------------------------------------------------- exact routing probes
def pattern_sel(name, E=3):
    """(R, row0, sel (2R,)) of a routing pattern; the expert under test is 1, the others share the rest"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def others(n):
        return torch.where(torch.rand(n, generator=g) < 0.5, 0, 2)

    def with_ones(R, at):
        s = others(2 * R)
        s[torch.as_tensor(at, dtype=torch.long)] = 1
        return s
    if name == "none":
        return 20, 0, others(40)
    if name.startswith("count"):
        n = int(name[5:])
        return 40, 0, with_ones(40, torch.randperm(80, generator=g)[:n])
    if name == "all_on_one":
        return 20, 0, torch.ones(40, dtype=torch.long)
    if name == "both_slots_same":
        s = others(40)
        s[1::2] = s[0::2]
        s[6:10] = 1
        return 20, 0, s
    if name == "only_second_pass":
        return 257, 0, with_ones(257, [512, 513])
    if name == "pass_boundary":
        return 300, 0, with_ones(300, [511, 512])
    if name == "six_passes":
        at = torch.cat([torch.arange(6) * 512 + j for j in (0, 63, 64, 300, 511)] + [torch.tensor([1, 2, 3])])
        return 1536, 0, with_ones(1536, at)
    if name == "row0_second_pass":
        return 257, 7, with_ones(257, [0, 17, 511, 512, 513])
    if name == "invalid_sel":
        s = with_ones(20, [3, 4, 20])
        s[5], s[11], s[12], s[39] = -1, E, -1, E
        return 20, 0, s
    raise KeyError(name)


PATTERNS = ["none", "count1", "count16", "count17", "count32", "count33", "all_on_one", "both_slots_same", "only_second_pass", "pass_boundary",
            "six_passes", "row0_second_pass", "invalid_sel"]
_PROBE_W = {}


def probe_weights(stage, fp8, E=3):
    """W[e][n][k] = code (3 n + k + 7 e) mod 251 as bf16 integers; fp8: the e4m3 value of byte (3 n + k + 7 e) mod 120 (finite, >= 0) with the
    power-of-two scales 2^(e % 3 - 1).  Built once per form."""
    key = (stage, fp8, E)
    if key not in _PROBE_W:
        N, K = (D_FF, D_MODEL) if stage == 1 else (D_MODEL, D_FF)
        code = 3 * torch.arange(N)[None, :, None] + torch.arange(K)[None, None, :] + 7 * torch.arange(E)[:, None, None]
        if fp8:
            q8 = (code % 120).to(torch.uint8)
            _PROBE_W[key] = dict(w_q8=q8, w_s=torch.exp2((torch.arange(E) % 3 - 1).float()), vals=e4m3_values(q8))
        else:
            w = (code % 251).float().bfloat16()
            _PROBE_W[key] = dict(w=w, vals=w.float())
    return _PROBE_W[key]


def pattern_probe(stage, fp8, name, E=3):
    """One-hot activation rows (1.0; fp8: 448, so inv = 1, q = 448 and the row scale is 1: every scale exact) against probe_weights: pair p
    returns column j of its expert's matrix -- times 448 wscale in fp8, times its power-of-two gate in stage 2 -- bit for bit (448 w has 7
    significant bits: exact in bf16 too).  j = (7 r + 3) mod 512 for row r (stage 1), (7 p + 3) mod 2048 for pair p (stage 2).
    -> (case, want (2R, N) with SENT at the pairs of no expert)."""
    R, row0, sel = pattern_sel(name, E)
    N, K = (D_FF, D_MODEL) if stage == 1 else (D_MODEL, D_FF)
    n_act = R if stage == 1 else 2 * R
    j = (7 * torch.arange(n_act) + 3) % K
    hot = 448.0 if fp8 else 1.0
    a = torch.zeros(n_act, K)
    a[torch.arange(n_act), j] = hot
    gate = torch.exp2(-(torch.arange(2 * R) % 4).float())
    pw = probe_weights(stage, fp8, E)
    c = dict(stage=stage, fp8=fp8, E=E, R=R, row0=row0, a=_pad_rows(a.bfloat16(), row0 if stage == 1 else 2 * row0), sel=_sel_buffer(sel, row0, E),
             gate=_pad_rows(gate, 2 * row0), **{k: v for k, v in pw.items() if k != "vals"})
    p = torch.arange(2 * R)
    ok = (sel >= 0) & (sel < E)
    e = sel.clamp(0, E - 1)
    jp = j[p >> 1] if stage == 1 else j
    want = pw["vals"][e, :, jp] * hot                                            # (2R, N) gather
    if fp8:
        want = want * pw["w_s"][e][:, None]
    if stage == 2:
        want = want * gate[:, None]
    want = torch.where(ok[:, None], want, torch.full((), SENT))
    return c, want


def check_pattern_probe(c, want, got):
    row0, R = c["row0"], c["R"]
    return join([exact("probe columns", got[2 * row0:2 * (row0 + R)].float(), want), untouched("pairs below row0", got[:2 * row0])])


# ============================================================================= combine
def combine_case(R, row0, seed=0, slack=3):
    g = torch.Generator().manual_seed(seed + 10 * R + row0)
    return dict(R=R, row0=row0, stride=row0 + R + slack, h=_pad_rows(torch.randn(R, D_MODEL, generator=g), row0),
                y=_pad_rows(torch.randn(2 * R, D_MODEL, generator=g) * 0.5, 2 * row0))


def combine_simulate(c, dtype=F32, mutant=None, ssq_before=SENT):
    """the device's whole h (rows, 512) and ssq (32, stride) after the launch; ssq pre-filled with `ssq_before`.  Mutants: combine_rows
    (y[r] + y[r + R]), ssq_stale (tiles 1..31 not written), row0_ignored."""
    R, row0 = c["R"], c["row0"]
    at = 0 if mutant == "row0_ignored" else row0
    h = c["h"].clone()
    ssq = torch.full((32, c["stride"]), ssq_before)
    new = pend_sum(c["h"][at:at + R], c["y"][2 * at:2 * (at + R)], "pend_rows" if mutant == "combine_rows" else None)
    h[at:at + R] = new
    if mutant != "ssq_stale":
        ssq[:, at:at + R] = 0.0
    ssq[0, at:at + R] = new.to(dtype).pow(2).sum(-1).float()
    return dict(h=h, ssq=ssq)


def check_combine(c, got):
    """h bit for bit (rows below row0 as they were: NaN); ssq[0] against the DEVICE's own h_new in double: per lane 8 squares and their
    additions (at most 9 roundings of a partial sum of positive terms), then the 6-step tree: (9 + 6 + 1) 2^-24 relative; tiles 1..31 exactly 0;
    the slack columns and the columns below row0 still SENT"""
    R, row0 = c["R"], c["row0"]
    rows = slice(row0, row0 + R)
    want = pend_sum(c["h"][rows], c["y"][2 * row0:2 * (row0 + R)])
    own = got["h"][rows].double().pow(2).sum(-1)
    outside = torch.ones(c["stride"], dtype=torch.bool)
    outside[rows] = False
    below = got["h"][:row0]
    return join([exact("h", got["h"][rows], want), _named(dict(elements=int(below.numel()), ok=bool(below.isnan().all())), "h below row0 as it was"),
                 _named(check_f32(got["ssq"][0, rows], own, 16 * 2.0 ** -24 * own + 2.0 ** -140), "ssq tile 0"),
                 exact("ssq tiles 1..31", got["ssq"][1:, rows], torch.zeros(31, R)), untouched("ssq outside the rows", got["ssq"][:, outside])])


COMBINE_R, COMBINE_ROW0 = [1, 8, 9], [0, 5]

# every wrong kernel the CPU module shows failing: mutant -> (family, what it is)
MUTANTS = {
    "tie_higher": "router", "swap_23": "router", "ignore_8_15": "router", "gates_swapped": "router", "softmax_all": "router", "unrounded_xn": "router",
    "eps_outside": "router", "row_p": "expert", "hidden_row0": "expert", "gate_other": "expert", "no_relu": "expert", "ragged_written": "expert",
    "second_chunk_first": "expert", "drop_beyond_512": "expert", "amax_slice": "expert", "no_wscale": "expert", "wscale_e0": "expert",
    "fp8_trunc": "expert", "no_clamp": "expert", "combine_rows": "combine", "ssq_stale": "combine", "row0_ignored": "all",
}
