"""The decoder step's separate-launch kernels one by one, through the test doors of include/ymt3.h (ymt3_test_dec_gemm / _dec_attention /
_mc_cross_attention), against float64 references of their contracts (tests/dec_kernel_model.py; tests/test_decoder_kernels_cpu.py shows that model
right and sharp, and that every random case here keeps its caps under the reference alone):

  exact probes   one-hot softmax rows return a row of V (integer codes) bit for bit; one-hot GEMM operands return a column of W
  criterion      tests/enc_kernel_model.py's: a stable element must equal the reference bit for bit, the others lie within beta + 1 bf16 ulp;
                 a fused query is judged against every candidate rounding of its unstable elements (dec_kernel_model.check_fused)
  guards         every output lies inside sentinels (Guarded): rows outside [row0, row0 + R), cache positions other than the row's, 64 elements
                 either side must come back untouched; input rows below row0 hold NaN, cache positions >= n_keys hold NaN
  state          a decode call after all the door calls gives the bits it gave before them (the last test of the module)
Every test records its figures under dec_kernel_* in the parity report.
"""
import pytest
import torch

import dec_kernel_model as D
from test_encoder_kernels import SENT, Guarded, m  # noqa: F401 (m: the encoder module's small handle, one per module)
from test_gpu_parity import _REPORT
from value_regimes import gemm_operands, gemm_reference_and_bound
from yourmt3_amd import _lib

pytestmark = pytest.mark.gpu
assert SENT == D.SENT
_BEFORE = {}


@pytest.fixture(scope="module", autouse=True)
def _decode_before_and_after(m):
    """the handle's own decode before any door call; test_decode_after_the_doors_gives_the_same_bits compares"""
    g = torch.Generator().manual_seed(11)
    enc = torch.randn(2, m.cfg.n_frames, m.cfg.d_model, generator=g).bfloat16()
    _BEFORE["enc"] = enc
    _BEFORE["out"] = [t.cpu() for t in m.decode(enc, 24, return_logits=True)]
    yield


def _record(name, rec):
    rec = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}
    _REPORT["dec_kernel_" + name] = rec
    print(name, rec)
    return rec


def _rows(x, row0, fill=float("nan")):
    """x (R, ...) -> (row0 + R, ...) with `fill` in the rows below row0"""
    pad = torch.full((row0,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
    return torch.cat([pad, x], 0)


def _mask(rows, row0, *rest):
    w = torch.zeros((rows,) + rest, dtype=torch.bool)
    w[row0:] = True
    return w


# ----------------------------------------------------------------------------- decode GEMMs
def _run_gemm(m, mode, c, row0=0, mid_rows=0, lockstep=False, state=None):
    """one launch of a dec_kernel_model GEMM case with its rows at [row0, row0 + R) -> `got` as dec_kernel_model.check_dec_gemm takes it.
    `state` (mode 4): the Guarded h and ssq of an earlier launch, to accumulate into."""
    dev = m.device
    W = c["W"].to(dev)
    N, K = W.shape
    kw = dict(W=W, N=N, K=K, row0=row0, eps=c["eps"], mid_rows=mid_rows)
    got = {}
    if mode == D.DG_RESID:
        R = c["a"].shape[0]
        rows, stride = row0 + R, row0 + R + 3
        if state is None:
            state = (Guarded(m, rows * N, torch.float32, _rows(c["h"], row0, SENT).flatten()), Guarded(m, 32 * stride, torch.float32))
        h, ssq = state
        part = None if c.get("part") is None else _rows(c["part"], row0).to(dev)
        m.test_dec_gemm(mode, R=R, a=_rows(c["a"], row0).to(dev), out_f32=h.view, ssq=ssq.view, ssq_stride=stride, part=part, **kw)
        ws = torch.zeros(32, stride, dtype=torch.bool)
        ws[:, row0:rows] = True
        got["h"] = h.read(_mask(rows, row0, N)).reshape(rows, N)[row0:]
        got["ssq"] = ssq.read(ws).reshape(32, stride)[:, row0:rows]
        got["state"] = state
        return got
    R = c["x"].shape[0]
    rows, stride = row0 + R, row0 + R + 3
    kw.update(R=R, x=_rows(c["x"], row0).to(dev), gain=c["gain"].to(dev))
    if c.get("pend_y") is not None:
        kw["pend_y"] = _rows(c["pend_y"], 2 * row0).to(dev)
        if mode == D.DG_QKV:
            h_out = Guarded(m, rows * K, torch.float32)
            kw["h_out"] = h_out.view
    else:
        ssq = torch.full((32, stride), float("nan"))
        ssq[:, row0:rows] = c["ssq"]
        kw.update(ssq=ssq.to(dev), ssq_stride=stride)
    if mode == D.DG_LOGITS:
        out = Guarded(m, rows * N, torch.float32)
        m.test_dec_gemm(mode, out_f32=out.view, **kw)
        got["out"] = out.read(_mask(rows, row0, N)).reshape(rows, N)[row0:]
    elif mode == D.DG_QKV:
        H, L = c["H"], c["L"]
        if c.get("table"):
            tab = Guarded(m, rows * N, torch.bfloat16)
            m.test_dec_gemm(mode, table=tab.view, H=H, L=L, **kw)
            got["table"] = tab.read(_mask(rows, row0, N)).reshape(rows, N)[row0:]
        else:
            q = Guarded(m, rows * H * 64, torch.bfloat16)
            kc, vc = Guarded(m, rows * H * L * 64, torch.bfloat16), Guarded(m, rows * H * L * 64, torch.bfloat16)
            pos = c["pos"]
            if lockstep:
                assert bool((pos == pos[0]).all())
                kw.update(step=int(pos[0]))
            else:
                kw.update(row_pos=_rows(pos.int(), row0, 10 ** 6).to(dev))
            m.test_dec_gemm(mode, out_bf16=q.view, kcache=kc.view, vcache=vc.view, H=H, L=L, **kw)
            wc = torch.zeros(rows, H, L, 64, dtype=torch.bool)
            wc[row0 + torch.arange(R), :, pos] = True
            got["q"] = q.read(_mask(rows, row0, H * 64)).reshape(rows, H * 64)[row0:]
            got["kc"] = kc.read(wc).reshape(rows, H, L, 64)[row0:]
            got["vc"] = vc.read(wc).reshape(rows, H, L, 64)[row0:]
        if "h_out" in kw:
            got["h_out"] = h_out.read(_mask(rows, row0, K)).reshape(rows, K)[row0:]
    else:
        out = Guarded(m, rows * N, torch.bfloat16)
        m.test_dec_gemm(mode, out_bf16=out.view, **kw)
        got["out"] = out.read(_mask(rows, row0, N)).reshape(rows, N)[row0:]
    return got


_GEMM = D.gemm_cases()


@pytest.mark.parametrize("name", list(_GEMM))
def test_dec_gemm_random_cases_meet_the_criterion(m, name):
    mode, make, la = _GEMM[name]
    c = make()
    ref = D.dec_gemm_reference(mode, c)
    got = _run_gemm(m, mode, c, **la)
    rec = _record("gemm_" + name, D.check_dec_gemm(mode, c, ref, got))
    assert rec["ok"] and rec.get("stable_share", 1.0) >= D.MIN_STABLE, rec


@pytest.mark.parametrize("mid_rows", [0, 1])
@pytest.mark.parametrize("mode", range(5))
def test_dec_gemm_permutation_probe_is_exact(m, mode, mid_rows):
    """one-hot rows against W[n][k] = (3 n + k) mod 251: the operand index maps of both kernels, bit for bit"""
    R, N = 37, (512 if mode == D.DG_RESID else 384)
    c, want = D.permutation_case(mode, R, N, 512)
    c.update(H=2, L=4, pos=torch.arange(R) % 4)
    got = _run_gemm(m, mode, c, row0=5, mid_rows=mid_rows)
    if mode == D.DG_QKV:
        rows = torch.arange(R)
        out = torch.cat([got["q"], got["kc"][rows, :, c["pos"]].reshape(R, 128), got["vc"][rows, :, c["pos"]].reshape(R, 128)], 1)
    else:
        out = got["out"] if "out" in got else got["h"]
    if mode == D.DG_RELU:
        want = want.clamp(min=0)
    want = want if mode in (D.DG_LOGITS, D.DG_RESID) else D.rb(want)
    rec = _record(f"gemm_permutation_mode{mode}_mid{mid_rows}", D.exact("columns of W", out.float(), want.float()))
    assert rec["ok"], rec
    if mode == D.DG_RESID:                      # sum(h^2) of a row that holds integers below 251: exact in fp32 in any order
        assert torch.equal(got["ssq"], D.ssq_partials(want))


@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_dec_gemm_resid_accumulates_and_its_partials_feed_the_next_norm(m, K):
    """DG_RESID twice in a row: h = (h0 + s) + s; the sum(h^2) partials of the second launch, fed with the device's own h to a NORM launch, give
    what the reference gives from the exact partials of that h"""
    c = D.gemm_case(D.DG_RESID, 17, 512, K, part=K == 1024)
    ref1 = D.dec_gemm_reference(D.DG_RESID, c)
    g1 = _run_gemm(m, D.DG_RESID, c, row0=5)
    r1 = D.check_dec_gemm(D.DG_RESID, c, ref1, g1)
    c2 = dict(c, h=g1["h"])
    ref2 = D.dec_gemm_reference(D.DG_RESID, c2)
    g2 = _run_gemm(m, D.DG_RESID, c2, row0=5, state=g1["state"])
    r2 = D.check_dec_gemm(D.DG_RESID, c2, ref2, g2)
    assert not torch.equal(g1["h"], g2["h"])
    n = D.gemm_case(D.DG_BF16, 17, 128, 512, seed=3)
    n.update(x=g2["h"], ssq=D.ssq_partials(g2["h"]))
    refn = D.dec_gemm_reference(D.DG_BF16, n)
    gn = _run_gemm(m, D.DG_BF16, dict(n, ssq=g2["ssq"]), row0=5)
    rn = D.check_dec_gemm(D.DG_BF16, n, refn, gn)
    rec = _record(f"gemm_resid_twice_K{K}", D.merge([r1, r2, rn]))
    assert rec["ok"], rec


@pytest.mark.parametrize("kind", ["cancel", "negative", "scale_up", "scale_down", "scale_mixed", "subnormal"])
@pytest.mark.parametrize("mid_rows", [0, 1])
def test_dec_gemm_value_regimes(m, kind, mid_rows):
    """DG_RESID's fp32 result on the operands of tests/value_regimes.py at the any-order bound (h = 0: the result is the product)"""
    A, W = gemm_operands(kind, 19, 512, 512)
    c = dict(a=A, W=W, h=torch.zeros(19, 512), part=None, eps=0.0)
    got = _run_gemm(m, D.DG_RESID, c, row0=0, mid_rows=mid_rows)
    ref, bound = gemm_reference_and_bound(A, W)
    rec = _record(f"gemm_values_{kind}_mid{mid_rows}", D.check_f32(got["h"], ref, bound))
    assert rec["ok"] and bool(torch.isfinite(got["h"]).all()), rec


@pytest.mark.parametrize("mid_rows", [0, 1])
def test_dec_gemm_nan_row_stays_in_its_row_and_a_repeat_gives_the_same_bits(m, mid_rows):
    c = D.gemm_case(D.DG_BF16, 37, 128, 512, seed=5)
    clean = _run_gemm(m, D.DG_BF16, c, row0=5, mid_rows=mid_rows)["out"]
    again = _run_gemm(m, D.DG_BF16, c, row0=5, mid_rows=mid_rows)["out"]
    assert torch.equal(clean.view(torch.int16), again.view(torch.int16))
    x = c["x"].clone()
    x[18, 77] = float("nan")
    got = _run_gemm(m, D.DG_BF16, dict(c, x=x), row0=5, mid_rows=mid_rows)["out"]
    keep = torch.arange(37) != 18
    assert bool(got[18].float().isnan().all()) and torch.equal(got[keep].view(torch.int16), clean[keep].view(torch.int16))


# ----------------------------------------------------------------------------- step attention
def _run_attn(m, c, lockstep=False, wo=None):
    """one launch of a dec_kernel_model attention case -> out (R, H, 64) bf16 on the host, or opart (R, 8, 512) f32 when `wo` is given"""
    dev = m.device
    form, R, H, L, row0 = c["form"], c["R"], c["H"], c["L"], c["row0"]
    rows = row0 + R
    is_self = D.FORMS[form][0]
    kw = dict(self_attn=is_self, k=c["kc"].to(dev).flatten(), v=c["vc"].to(dev).flatten(), R=R, H=H, slab_keys=L, row0=row0,
              rows_per_kv=c["rows_per_kv"], force_many=form in ("self2", "beam2", "cross2"))
    if form == "mc":
        nc = c["rows_per_kv"]
        assert row0 % nc == 0 and R % nc == 0
        skip = (row0 // nc) * H * L * 64
        out = Guarded(m, rows * H * 64, torch.bfloat16)
        m.test_mc_cross_attention(x=c["x_dev"].to(dev), gain=c["gain"].to(dev), ssq=c["ssq_dev"].to(dev), ssq_stride=rows, wq=c["wq"].to(dev),
                                  k=kw["k"][skip:], v=kw["v"][skip:], out=out.view, n_seg=R // nc, n_channels=nc, H=H, T=L, row0=row0, eps=c["eps"])
        return out.read(_mask(rows, row0, H * 64)).reshape(rows, H, 64)[row0:]
    if is_self:
        kw.update(q=c["q_dev"].to(dev).flatten(), bias=c["bias"].to(dev).contiguous())
        if lockstep:
            assert bool((c["n_keys"] == c["n_keys"][0]).all())
            kw.update(step=int(c["n_keys"][0]) - 1)
        else:
            kw.update(row_pos=_rows((c["n_keys"] - 1).int(), row0, 10 ** 6).to(dev))
        if "anc" in c:
            kw.update(anc=c["anc"].to(dev).flatten(), anc_rows=c["anc_rows"], anc_pitch=c["anc_pitch"], W=c["W"])
    else:
        kw.update(n_keys_const=int(c["n_keys"][0]))
        if "wq" in c:
            kw.update(wq=c["wq"].to(dev), x=c["x_dev"].to(dev), gain=c["gain"].to(dev), eps=c["eps"])
            if c.get("ipart") is not None:
                kw.update(ipart=c["ipart_dev"].to(dev))
            else:
                kw.update(ssq=c["ssq_dev"].to(dev), ssq_stride=rows)
        else:
            kw.update(q=c["q_dev"].to(dev).flatten())
    if wo is not None:
        op = Guarded(m, rows * 8 * 512, torch.float32)
        m.test_dec_attention(wo=wo.to(dev), opart=op.view, **kw)
        return op.read(_mask(rows, row0, 8 * 512)).reshape(rows, 8, 512)[row0:]
    out = Guarded(m, rows * H * 64, torch.bfloat16)
    m.test_dec_attention(out=out.view, **kw)
    return out.read(_mask(rows, row0, H * 64)).reshape(rows, H, 64)[row0:]


def _out(m, c, lockstep=False):
    """the (R, H, 64) output of any self- or cross-attention form; the wo form's through a permutation wo (exact: dec_kernel_model.wo_permutation)"""
    if c["form"] != "wo":
        return _run_attn(m, c, lockstep)
    val, clean = D.out_from_opart(_run_attn(m, c, lockstep, wo=D.wo_permutation()))
    assert clean, "the folded O-projection wrote something else than scaled bf16 outputs at its permutation's columns"
    return val


_ATTN = D.attention_cases()
_FUSED = D.fused_cases()
SELF_FORMS = ["self8", "self2", "wo", "beam8", "beam2"]


def _tails(form):
    return D.TAILS_2WAVE if form.endswith("2") else D.TAILS_8WAVE


@pytest.mark.parametrize("name", list(_ATTN))
def test_dec_attention_random_cases_meet_the_criterion(m, name):
    c = _ATTN[name]()
    parts, beta = D.attention_reference(c)
    got = _out(m, c, lockstep="_step_" in name)
    rec = _record("attn_" + name, D.check_attention(c, parts, beta, got))
    assert rec["ok"] and rec["stable_share"] >= D.MIN_STABLE, rec


@pytest.mark.parametrize("target", ["spread", "newest"])
@pytest.mark.parametrize("form", SELF_FORMS)
def test_self_attention_score_probe_is_exact_at_every_tail_length(m, form, target):
    """a one-hot q lets one key win by 256 at every tail length of the form's partition: the row is that key's V, bit for bit (beam: the V of
    the row the ancestry table names, both parity buffers, an entry >= W clamped)"""
    c = D.score_probe(form, _tails(form), H=8 if form == "wo" else 2, target=None if target == "spread" else "newest")
    rec = _record(f"attn_score_probe_{form}_{target}", D.check_probe(c, _out(m, c)))
    assert rec["ok"] and rec["exact_row_share"] == 1.0, rec


@pytest.mark.parametrize("form", ["self8", "self2", "beam8"])
def test_self_attention_score_probe_lockstep(m, form):
    recs = []
    for n in D.TAILS_STEP:
        c = D.score_probe(form, [n] * 4, row0=4, target="newest")
        recs.append(D.check_probe(c, _out(m, c, lockstep=True)))
    rec = _record(f"attn_score_probe_lockstep_{form}", D.merge(recs))
    assert rec["ok"], rec


@pytest.mark.parametrize("form", SELF_FORMS)
def test_self_attention_bias_probe_every_distance_is_the_lone_peak_once(m, form):
    """q = 0 and a table that is 0 at one distance per head, -256 elsewhere: over the launches every distance 0 .. L - 1 is the lone peak of a
    (row, head) with that many keys; rows with fewer keys return the mean of V"""
    H = 8 if form == "wo" else 64
    base = D.bias_probe_base(form, H)
    dev_c = dict(base, kc=base["kc"].to(m.device), vc=base["vc"].to(m.device), q_dev=base["q_dev"].to(m.device))
    recs, seen = [], set()
    for j in range(D.bias_probe_launches(H)):
        c = D.bias_probe(form, j, H)
        recs.append(D.check_bias_probe(c, _out(m, dict(dev_c, bias=c["bias"]))))
        seen |= set(c["peak"][c["target"][0] >= 0].tolist())
    rec = _record(f"attn_bias_probe_{form}", dict(D.merge(recs), launches=len(recs), exact_row_share=sum(r["exact_row_share"] for r in recs) / len(recs)))
    assert rec["ok"] and seen == set(range(1024)), rec


@pytest.mark.parametrize("name", list(_FUSED))
def test_fused_query_attention_random_cases_meet_the_candidate_rule(m, name):
    c = _FUSED[name]()
    fr = D.fused_reference(c)
    rec = _record("attn_" + name, D.check_fused(fr, _run_attn(m, c)))
    assert rec["ok"] and rec["stable_share"] >= D.MIN_STABLE and rec["left_out_share"] <= D.MAX_LEFT_OUT, rec


@pytest.mark.parametrize("name", [n for n in _FUSED if n.startswith("mc_") and ("_c3_" in n or "_c16_" in n)])
def test_multi_channel_inputs_through_the_fused_kernel_meet_the_same_reference(m, name):
    """dec_attn_kernel<false, true> on the multi-channel kernel's inputs (rows_per_kv = n_channels): the same contract, without the two-term p"""
    c = dict(_FUSED[name](), form="fused")
    rec = _record("attn_fused_on_" + name, D.check_fused(D.fused_reference(c), _run_attn(m, c)))
    assert rec["ok"], rec


@pytest.mark.parametrize("form,nc,T,row0", [("fused", 1, 256, 0), ("fused", 3, 128, 6), ("mc", 13, 256, 13), ("mc", 2, 512, 0), ("mc", 16, 128, 16)])
def test_fused_query_exact_probe(m, form, nc, T, row0):
    """x = c e_j rows: q is known exactly and one key wins by 181 or more; over the 512 rows and 8 heads every (head row, k chunk, output of a
    wave) of the projection is the hot one"""
    c = D.fused_probe(form, T, 8, row0, nc)
    got = _run_attn(m, c)
    _, v, _, _ = D.gather_pairs(c)
    want = v[torch.arange(v.shape[0]), c["target"].reshape(-1)].reshape(c["R"], 8, 64)
    rec = _record(f"attn_fused_probe_{form}_c{nc}_T{T}", D.exact("one-hot rows", got.float(), want.float()))
    assert rec["ok"], rec


def test_attention_values_nan_stays_in_its_pair_and_a_repeat_gives_the_same_bits(m):
    c = D.self_case("self8", [5, 300, 1024], seed=9)
    clean = _run_attn(m, c)
    assert torch.equal(_run_attn(m, c).view(torch.int16), clean.view(torch.int16))
    q = c["q_dev"].clone()
    q[1, 1, 17] = float("nan")
    got = _run_attn(m, dict(c, q_dev=q))
    bad = torch.zeros(3, 2, dtype=torch.bool)
    bad[1, 1] = True
    assert bool(got[bad].float().isnan().all()) and torch.equal(got[~bad].view(torch.int16), clean[~bad].view(torch.int16))


def test_folded_o_projection_partials_are_the_resid_kernels_wave_partials(m):
    """opart of the wo form against DG_RESID (K = 512) over the attention output o: h + (((p0 + p1) + ...) + p7) == h + o . wo^T, bit for bit --
    and DG_RESID with `part` adds the same sum"""
    c = D.self_case("wo", [1, 65, 385, 1024, 700], H=8, seed=12)
    g = torch.Generator().manual_seed(5)
    wo = (torch.randn(512, 512, generator=g) / 16).bfloat16()
    h0 = torch.randn(5, 512, generator=g)
    o = _run_attn(m, dict(c, form="self8")).reshape(5, 512)
    op = _run_attn(m, c, wo=wo)
    sp = op[:, 0].clone()
    for w in range(1, 8):
        sp = sp + op[:, w]
    want = h0 + sp
    got = _run_gemm(m, D.DG_RESID, dict(a=o, W=wo, h=h0, part=None, eps=0.0), row0=3)
    assert torch.equal(got["h"], want), float((got["h"] - want).abs().max())
    zero = dict(a=torch.zeros(5, 512).bfloat16(), W=wo, h=h0, part=op, eps=0.0)
    assert torch.equal(_run_gemm(m, D.DG_RESID, zero, row0=3)["h"], want)
    _record("attn_wo_partials_equal_resid", D.exact("h + sum opart", got["h"], want))


# ----------------------------------------------------------------------------- refusals
def _refused(call, **kw):
    with pytest.raises((ValueError, _lib.YMT3Error)):
        call(**kw)


def test_dec_gemm_door_refuses(m):
    """the C side's own refusals (YMT3_ERR_ARG), past the wrapper: a raw argument struct per case; the door stays usable"""
    dev = m.device
    W = torch.zeros(1536, 512, dtype=torch.bfloat16, device=dev)
    x = torch.zeros(8, 512, device=dev)
    gain, ssq = torch.ones(512, device=dev), torch.zeros(32, 8, device=dev)
    ob, of = torch.zeros(8, 1536, dtype=torch.bfloat16, device=dev), torch.zeros(8, 512, device=dev)
    kc = torch.zeros(8 * 8 * 4 * 64, dtype=torch.bfloat16, device=dev)
    p = lambda t: t.data_ptr()

    def raw(mode, **f):
        base = dict(x_f32=p(x), a_bf16=p(ob), gain=p(gain), W=p(W), out_bf16=p(ob), out_f32=p(of), kcache=p(kc), vcache=p(kc), ssq=p(ssq), row0=0, R=8,
                    N=512, K=512, H=0, L=0, ssq_stride=8, mid_rows=0, step=0, eps=1e-6)
        base.update(f)
        a = _lib.DecGemmArgs(**base)
        import ctypes
        return m._lib.ymt3_test_dec_gemm(m._handle, mode, ctypes.byref(a), m._stream())

    assert raw(1) == 0 and raw(4) == 0
    bad = [raw(1, W=None), raw(1, W=p(W) + 2), raw(5), raw(1, K=1024), raw(4, N=256), raw(4, K=768), raw(1, ssq_stride=7), raw(1, row0=1),
           raw(0, N=1536, H=8, L=4, step=4), raw(0, N=1536, H=8, L=4, step=-1), raw(0, N=1024, H=8, L=4), raw(1, pend_y=p(x)),
           raw(4, K=1024, mid_rows=1), raw(1, N=48, mid_rows=1), raw(0, N=1536, H=8, L=4, table=p(ob), mid_rows=1), raw(1, part=p(of)), raw(1, R=0)]
    assert all(rc != 0 for rc in bad), bad
    assert raw(0, N=1536, H=8, L=4, step=3) == 0 and raw(1) == 0
    torch.cuda.synchronize()


def test_dec_attention_door_refuses(m):
    import ctypes
    dev = m.device
    H, L, R = 8, 16, 4
    q = torch.zeros(R * H * 64, dtype=torch.bfloat16, device=dev)
    kv = torch.zeros(R * H * L * 64, dtype=torch.bfloat16, device=dev)
    bias = torch.zeros(H * L, device=dev)
    x, gain, ssq = torch.zeros(R * 512, device=dev), torch.ones(512, device=dev), torch.ones(32 * R, device=dev)
    wq = torch.zeros(H * 64 * 512, dtype=torch.bfloat16, device=dev)
    op = torch.zeros(R * 8 * 512, device=dev)
    anc = torch.zeros(2 * R * 32, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()

    def raw(**f):
        base = dict(q=p(q), k=p(kv), v=p(kv), out=p(q), bias=p(bias), self_attn=1, step=0, slab_keys=L, rows_per_kv=1, row0=0, R=R, H=H, bias_stride=L)
        base.update(f)
        a = _lib.DecAttnArgs(**base)
        return m._lib.ymt3_test_dec_attention(m._handle, ctypes.byref(a), m._stream())

    cross = dict(self_attn=0, bias=None, bias_stride=0, n_keys_const=L)
    fused = dict(cross, q=None, wq=p(wq), x_f32=p(x), gain=p(gain), ssq=p(ssq), ssq_stride=R, d=512)
    beam = dict(anc=p(anc), anc_rows=R, anc_pitch=32, W=4)
    assert raw() == 0 and raw(**cross) == 0 and raw(**fused) == 0 and raw(**beam) == 0
    bad = [raw(k=None), raw(q=p(q) + 2), raw(step=L), raw(step=-1), raw(bias_stride=L - 1), raw(H=0), raw(slab_keys=0), raw(rows_per_kv=0),
           raw(**dict(cross, n_keys_const=0)), raw(**dict(cross, n_keys_const=L + 1)), raw(**dict(cross, bias=p(bias))),
           raw(**dict(fused, d=256)), raw(**dict(fused, ssq_stride=R - 1)), raw(**dict(fused, force_many=1)),
           raw(**dict(fused, ssq=None, ipart=p(op), H=4)), raw(wo=p(wq), opart=p(op), out=None, H=4), raw(wo=p(wq), opart=None, out=None),
           raw(wo=p(wq), opart=p(op), out=None, force_many=1), raw(**dict(beam, W=3)), raw(**dict(beam, W=9)), raw(**dict(beam, anc_pitch=24)),
           raw(**dict(beam, anc_pitch=16)), raw(**dict(beam, anc_rows=R - 1)), raw(**dict(beam, wo=p(wq), opart=p(op), out=None)), raw(wq=p(wq))]
    assert all(rc != 0 for rc in bad), bad
    assert raw() == 0
    torch.cuda.synchronize()


def test_mc_cross_attention_door_refuses(m):
    import ctypes
    dev = m.device
    H, T, nc = 8, 128, 3
    x, gain, ssq = torch.zeros(nc * 512, device=dev), torch.ones(512, device=dev), torch.ones(32 * nc, device=dev)
    wq = torch.zeros(H * 64 * 512, dtype=torch.bfloat16, device=dev)
    kv = torch.zeros(H * T * 64, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(nc * H * 64, dtype=torch.bfloat16, device=dev)
    p = lambda t: t.data_ptr()

    def raw(**f):
        base = dict(x_f32=p(x), gain=p(gain), ssq=p(ssq), wq=p(wq), k=p(kv), v=p(kv), out=p(out), row0=0, n_seg=1, n_channels=nc, H=H, T=T,
                    ssq_stride=nc, d=512, eps=1e-6)
        base.update(f)
        a = _lib.McCrossArgs(**base)
        return m._lib.ymt3_test_mc_cross_attention(m._handle, ctypes.byref(a), m._stream())

    assert raw() == 0
    bad = [raw(x_f32=None), raw(out=p(out) + 2), raw(n_channels=1), raw(n_channels=17), raw(T=64), raw(T=1024), raw(T=192), raw(d=256),
           raw(ssq_stride=nc - 1), raw(n_seg=0), raw(H=0)]
    assert all(rc != 0 for rc in bad), bad
    assert raw() == 0
    torch.cuda.synchronize()


def test_wrappers_refuse_on_the_device_too(m):
    """the wrapper's value check of row_pos reads the tensor from the device"""
    dev = m.device
    c = D.self_case("self8", [3, 9], L=16)
    kw = dict(self_attn=True, k=c["kc"].to(dev).flatten(), v=c["vc"].to(dev).flatten(), R=2, H=2, slab_keys=16, q=c["q_dev"].to(dev).flatten(),
              bias=c["bias"].to(dev), out=torch.zeros(2 * 2 * 64, dtype=torch.bfloat16, device=dev))
    _refused(m.test_dec_attention, row_pos=torch.tensor([2, 16], dtype=torch.int32, device=dev), **kw)
    _refused(m.test_dec_attention, row_pos=torch.tensor([-1, 3], dtype=torch.int32, device=dev), **kw)
    m.test_dec_attention(row_pos=torch.tensor([2, 15], dtype=torch.int32, device=dev), **kw)


# ----------------------------------------------------------------------------- the handle's own state (LAST test of the module)
def test_decode_after_the_doors_gives_the_same_bits(m):
    after = [t.cpu() for t in m.decode(_BEFORE["enc"], 24, return_logits=True)]
    assert len(after) == len(_BEFORE["out"])
    for a, b in zip(after, _BEFORE["out"]):
        assert torch.equal(a, b)
