"""The token-selection kernels one by one, through the test doors of include/ymt3.h (ymt3_test_token_step: argmax_embed_kernel and its
companions of csrc/decode.hip; ymt3_test_beam_step: the kernels of csrc/beam.hip with one beam per group), against the float64 reference of their contract (tests/select_kernel_model.py;
tests/test_select_kernels_cpu.py shows that reference right and every named case sharp against its mutants):

  exact      ids, flags, positions, automaton states, loop state, ticket and counter lines; h (one fp32 add); copied logits and gathered
             q / k / v bit for bit
  bounds     ssq[0] within (d + 2) 2^-24 sum(v^2) of the float64 sum, ssq[1..31] exactly 0.0; scores within 1e-4 + 1e-5 |ref| of the float64
             log-softmax, the prescribed specials (NaN, -inf, 0.0) as such; uniform rows make the score bound sharp (-log n)
  guards     every buffer the kernels write lies between sentinels and holds sentinels wherever the launch must not write: rows outside
             [row0, row0 + R), other columns of tokens / scores / logits, other cache positions, the counter lines' neighbours
  beam       every select judged alone from the device's own state before it, the whole state after it compared; host-made logits whose every
             deciding comparison is an exact tie or has a float64 margin >= 2e-4 (asserted per step): zero undecided steps
  state      a decode, a beam decode and a streaming decode after all door calls give the bits they gave before (the last test)
Every test records its figures under select_kernel_* in the parity report.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import select_kernel_model as S
from test_encoder_kernels import SENT, Guarded, m  # noqa: F401 (m: the encoder module's small handle, one per module)
from test_gpu_parity import _REPORT
from yourmt3_amd import _lib

pytestmark = pytest.mark.gpu
assert SENT == S.SENT
_BEFORE = {}
_CASES = S.greedy_cases()


def _handle_calls(m):
    g = torch.Generator().manual_seed(12)
    enc = torch.randn(2, m.cfg.n_frames, m.cfg.d_model, generator=g).bfloat16()
    audio = torch.randn(3, m.cfg.segment_samples, generator=g) * 0.1
    out = [t.cpu() for t in m.decode(enc, 12, return_logits=True, return_scores=True)]
    out += [t.cpu() for t in m.decode(enc[:1], 8, num_beams=2, return_scores=True)]
    out.append(m.inference_stream(audio, 8, slots=2, interval=4).cpu())
    return out


@pytest.fixture(scope="module", autouse=True)
def _handle_before_and_after(m):
    """the handle's own decodes before any door call; test_handle_calls_after_the_doors_give_the_same_bits compares"""
    _BEFORE["out"] = _handle_calls(m)
    yield


def _record(name, rec):
    rec = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}
    _REPORT["select_kernel_" + name] = rec
    print(name, rec)
    return rec


# ----------------------------------------------------------------------------- buffers
def _t(a):
    """numpy -> torch on the host; uint16 arrays are bf16 bits, uint32 arrays travel as int32"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32))
    return torch.from_numpy(a)


def _dev(m, a):
    return None if a is None else _t(a).to(m.device).flatten()


class Out:
    """a Guarded buffer holding `before` (numpy, or a size: all sentinels); read() checks the guard bands and gives the region as numpy"""

    def __init__(self, m, before, dtype=None):
        if isinstance(before, (int, np.integer)):
            self.g = Guarded(m, int(before), dtype)
            self.shape = (int(before),)
        else:
            t = _t(before)
            self.g = Guarded(m, t.numel(), t.dtype, t.flatten())
            self.shape = before.shape
        self.view = self.g.view

    def read(self):
        host = self.g.read(torch.ones(self.view.numel(), dtype=torch.bool))
        if host.dtype == torch.bfloat16:
            return host.view(torch.int16).numpy().view(np.uint16).reshape(self.shape)
        return host.numpy().reshape(self.shape)


def _launch(m, c, keep_shared=False):
    """one launch of op 1 on a select_kernel_model case -> every buffer after it, as select_kernel_model.compare takes them"""
    rows, V, ns = c.rows, c.V, c.n_steps
    o = dict(h=Out(m, rows * S.D, torch.float32), ssq=Out(m, 32 * c.stride, torch.float32), finished=Out(m, c.finished),
             tokens=Out(m, c.n_out, torch.int32), state_out=Out(m, 4, torch.int32))
    kw = dict(R=c.R, row0=c.row0, V=V, n_steps=ns, n_prompt=c.n_prompt, step=c.step, step0=c.step0, eos_id=c.eos_id, pad_id=c.pad_id,
              n_channels=c.n_channels, logits=_dev(m, c.logits), embed=_dev(m, c.embed), chan_embed=_dev(m, c.chan), ssq_stride=c.stride,
              forced=_dev(m, c.forced), prompt=_dev(m, c.prompt), keep_shared=keep_shared)
    o["scores"] = Out(m, c.n_out, torch.float32)
    if c.want_scores:
        kw["scores_out"] = o["scores"].view
    if c.want_logits:
        o["logits_out"] = Out(m, c.n_out * V, torch.float32)
        kw["logits_out"] = o["logits_out"].view
    if c.allowed is not None:
        o["row_state"] = Out(m, c.state)
        kw.update(c_allowed=_dev(m, S.allowed_words(c.allowed)), c_next=_dev(m, c.next), c_n_states=c.allowed.shape[0], row_state=o["row_state"].view)
    if c.slot:
        o["row_pos"] = Out(m, c.row_pos)
        kw.update(row_pos=o["row_pos"].view, row_out=_dev(m, c.row_out), row_prompt=_dev(m, c.row_prompt))
    if c.ticket:
        o["ticket"] = Out(m, np.zeros((c.R // 32 + 1) * 32, np.int32))
        kw["ticket"] = o["ticket"].view
    if c.zero_lines:
        o["zero_sync"] = Out(m, c.zero_lines * 32 + 32, torch.int32)
        kw.update(zero_sync=o["zero_sync"].view, zero_lines=c.zero_lines)
    if c.qkv0 is not None:
        n = rows * 8 * c.L * 64
        o.update(q0=Out(m, rows * S.D, torch.bfloat16), kc=Out(m, n, torch.bfloat16), vc=Out(m, n, torch.bfloat16))
        kw.update(qkv0=_dev(m, c.qkv0), q0=o["q0"].view, kcache0=o["kc"].view, vcache0=o["vc"].view, L=c.L)
    m.test_token_step(1, h=o["h"].view, ssq=o["ssq"].view, finished=o["finished"].view, tokens_out=o["tokens"].view, state_out=o["state_out"].view, **kw)
    got = {k: v.read() for k, v in o.items()}
    got["h"] = got["h"].reshape(rows, S.D)
    got["ssq"] = got["ssq"].reshape(32, c.stride)
    if c.want_logits:
        got["logits_out"] = got["logits_out"].reshape(c.n_out, V)
    if c.qkv0 is not None:
        got["q0"] = got["q0"].reshape(rows, S.D)
        for k in ("kc", "vc"):                        # the reference's flat cache has room for one position past the end: the guard band here
            got[k] = np.concatenate([got[k], np.full(64, S.SENT_BF16, np.uint16)])
    return SimpleNamespace(**got)


@pytest.mark.parametrize("name", list(_CASES))
def test_argmax_embed_case_equals_the_reference(m, name):
    c, _ = _CASES[name]
    ref = S.token_step_ref(c)
    got = _launch(m, c)
    bad, fig = S.compare(c, ref, got)
    _record(name, dict(rows=c.R, V=c.V, differs=",".join(bad), **fig))
    assert not bad, bad


# ----------------------------------------------------------------------------- the init kernels and the tails
def _init_buffers(m, rows, stride, n_cache=0):
    o = dict(h=Out(m, rows * S.D, torch.float32), ssq=Out(m, 32 * stride, torch.float32), finished=Out(m, rows, torch.int32),
             row_state=Out(m, rows, torch.int32), state_out=Out(m, 4, torch.int32))
    if n_cache:
        o.update(q0=Out(m, rows * S.D, torch.bfloat16), kc=Out(m, n_cache, torch.bfloat16), vc=Out(m, n_cache, torch.bfloat16))
    return o


def _check_embed(got_h, got_ssq, h, ssq0, lo, hi):
    """rows [lo, hi) of h bit-equal and of ssq within the bound; everything else untouched -> the worst ssq error over its bound"""
    want = np.full(got_h.shape, np.float32(SENT))
    want[lo:hi] = h
    assert np.array_equal(want.view(np.uint32), got_h.view(np.uint32))
    bound = (S.D + 2) * 2.0 ** -24 * ssq0
    err = np.abs(got_ssq[0, lo:hi].astype(np.float64) - ssq0)
    assert (err <= bound).all() and (got_ssq[1:, lo:hi] == 0.0).all()
    rest = np.ones(got_ssq.shape, bool)
    rest[:, lo:hi] = False
    assert (got_ssq[rest] == SENT).all()
    return float((err / bound).max())


@pytest.mark.parametrize("chan", [0, 3])
def test_decode_init_then_steps_chain_on_the_door_block(m, chan):
    """op 0 writes the block; two op 1 launches with keep_shared run on it: the prompt, the pointers, the automaton and step0 the init kernel
    wrote are what the steps read (state_out after each call), and the pad feed of the init kernel is exact"""
    V, R, ns, P, step0, pad = 48, 5, 3, 1, 0, 4
    rng = np.random.default_rng(50 + chan)
    x = rng.uniform(-2, 2, (R, V)).astype(np.float32)
    al = rng.random((4, V)) < 0.5
    al[:, 0] = True
    nxt = rng.integers(0, 4, (4, V)).astype(np.int32)
    start = np.array([2, -7, 99, 0, 3], np.int32)                  # out of range: clamped into [0, 4)
    c = S.make_case(x, seed=50, eos_id=-1, pad_id=pad, n_steps=ns, n_prompt=P, step=step0, prompt=[[V + 5], [1], [2], [-3], [7]], allowed=al, nxt=nxt,
                    state=np.clip(start, 0, 3), chan=chan, want_scores=True)
    stride = R + 3
    o = _init_buffers(m, R, stride)
    tokens, scores = Out(m, R * ns, torch.int32), Out(m, R * ns, torch.float32)
    kw = dict(R=R, V=V, n_steps=ns, n_prompt=P, pad_id=pad, n_channels=c.n_channels, embed=_dev(m, c.embed), chan_embed=_dev(m, c.chan), ssq_stride=stride,
              h=o["h"].view, ssq=o["ssq"].view, finished=o["finished"].view, row_state=o["row_state"].view, state_out=o["state_out"].view,
              tokens_out=tokens.view, scores_out=scores.view, prompt=_dev(m, c.prompt), c_allowed=_dev(m, S.allowed_words(al)), c_next=_dev(m, nxt),
              c_n_states=4)
    m.test_token_step(0, step0=step0, c_start=_dev(m, start), **kw)
    h, ssq0 = S.embed_ref(c.embed, c.chan, np.full(R, pad), np.arange(R), c.n_channels)
    worst = _check_embed(o["h"].read().reshape(R, S.D), o["ssq"].read().reshape(32, stride), h, ssq0, 0, R)
    assert np.array_equal(o["finished"].read(), np.zeros(R, np.int32))
    assert np.array_equal(o["row_state"].read(), np.clip(start, 0, 3))
    assert np.array_equal(o["state_out"].read(), [step0, 0, R, ns])
    assert (tokens.read() == SENT).all() and (scores.read() == SENT).all()
    # position 0 feeds the prompt; position 1 emits column 0 under the automaton, from the clamped start states
    logits = _dev(m, c.logits)
    m.test_token_step(1, logits=logits, keep_shared=True, **kw)
    assert np.array_equal(o["state_out"].read(), [1, 0, R, ns])
    assert (tokens.read() == SENT).all() and np.array_equal(o["row_state"].read(), np.clip(start, 0, 3))
    feed = np.array([S.clamp(p, V) for p in c.prompt[:, 0]])
    h, ssq0 = S.embed_ref(c.embed, c.chan, feed, np.arange(R), c.n_channels)
    worst = max(worst, _check_embed(o["h"].read().reshape(R, S.D), o["ssq"].read().reshape(32, stride), h, ssq0, 0, R))
    m.test_token_step(1, logits=logits, keep_shared=True, **kw)
    c.step = 1
    ref = S.token_step_ref(c)
    assert np.array_equal(o["state_out"].read(), [2, 0, R, ns])
    assert np.array_equal(tokens.read(), ref.tokens) and np.array_equal(o["row_state"].read(), ref.row_state)
    ok, ratio = S.compare_scores(ref.scores, scores.read())
    assert ok
    _record(f"init_chain_chan{chan}", dict(rows=R, V=V, differs="", ssq_err_over_bound=worst, score_err_over_bound=ratio))


@pytest.mark.parametrize("step0", [0, 5])
def test_decode_init_gathers_the_pad_row_at_step0(m, step0):
    V, R, L, pad = 48, 3, 6, 9
    c = S.make_case(np.zeros((R, V), np.float32), seed=60, qkv0=True, L=L)
    o = _init_buffers(m, R, R, R * 8 * L * 64)
    m.test_token_step(0, R=R, V=V, n_steps=L, step0=step0, pad_id=pad, embed=_dev(m, c.embed), ssq_stride=R, h=o["h"].view, ssq=o["ssq"].view,
                      finished=o["finished"].view, state_out=o["state_out"].view, qkv0=_dev(m, c.qkv0), q0=o["q0"].view, kcache0=o["kc"].view,
                      vcache0=o["vc"].view, L=L)
    t = c.qkv0[pad]
    kc = np.full((R, 8, L, 64), S.SENT_BF16, np.uint16)
    vc = kc.copy()
    kc[:, :, step0] = t[S.D:2 * S.D].reshape(8, 64)
    vc[:, :, step0] = t[2 * S.D:].reshape(8, 64)
    assert np.array_equal(o["q0"].read().reshape(R, S.D), np.tile(t[:S.D], (R, 1)))
    assert np.array_equal(o["kc"].read().reshape(kc.shape), kc) and np.array_equal(o["vc"].read().reshape(vc.shape), vc)
    assert np.array_equal(o["state_out"].read(), [step0, 0, R, L]) and (o["row_state"].read() == SENT).all()
    _record(f"init_gather_step0_{step0}", dict(rows=R, V=V, differs="", exact=True))


def test_slot_start_retire_and_pad_tail(m):
    """slot_start over the 3 channel rows of one segment at row0 = 3 (clamped start states by channel, offsets by channel); then slot_retire
    and pad_tail from every `from` in {0, 1, n_steps - 1, n_steps}: only the tail cells change"""
    V, K, row0, ns, P, pad = 48, 3, 3, 5, 2, 6
    rows, stride = row0 + K, row0 + K + 2
    c = S.make_case(np.zeros((K, V), np.float32), seed=70, chan=K)
    o = _init_buffers(m, rows, stride)
    row_pos, row_out, row_prompt = Out(m, rows, torch.int32), Out(m, rows, torch.int64), Out(m, rows, torch.int64)
    start = np.array([5, -1, 1], np.int32)
    m.test_token_step(2, R=K, row0=row0, V=V, n_steps=ns, n_prompt=P, pad_id=pad, n_channels=K, embed=_dev(m, c.embed), chan_embed=_dev(m, c.chan),
                      ssq_stride=stride, h=o["h"].view, ssq=o["ssq"].view, finished=o["finished"].view, row_state=o["row_state"].view,
                      row_pos=row_pos.view, row_out=row_out.view, row_prompt=row_prompt.view, c_start=_dev(m, start), c_n_states=3, first_out=40,
                      first_prompt=7)
    h, ssq0 = S.embed_ref(c.embed, c.chan, np.full(K, pad), np.arange(row0, rows), K)
    worst = _check_embed(o["h"].read().reshape(rows, S.D), o["ssq"].read().reshape(32, stride), h, ssq0, row0, rows)
    sent = np.full(row0, np.int32(SENT))
    assert np.array_equal(o["finished"].read(), np.concatenate([sent, np.zeros(K, np.int32)]))
    assert np.array_equal(o["row_state"].read(), np.concatenate([sent, [2, 0, 1]]))
    assert np.array_equal(row_pos.read(), np.concatenate([sent, np.zeros(K, np.int32)]))
    assert np.array_equal(row_out.read(), np.concatenate([sent, 40 + ns * np.arange(K)]))
    assert np.array_equal(row_prompt.read(), np.concatenate([sent, 7 + P * np.arange(K)]))
    _record("slot_start", dict(ssq_err_over_bound=worst))
    # tails.  slot_retire: row r of [row0, row0 + R) pads emitted columns [row_pos + 1 - n_prompt, n_steps) at row_out[r]
    froms = [0, 1, ns - 1, ns]
    R = len(froms)
    pos = np.array([f - 1 + P for f in froms], np.int32)           # from = pos + 1 - P; the first row also shows the clamp at 0 (pos = P - 1)
    pos[0] = 0                                                     # a row still inside its prompt: the whole row is padded
    out_at = np.array([3 * ns, 0, 2 * ns, 1 * ns], np.int64)
    for with_scores in (True, False):
        tokens, scores = Out(m, (row0 + R) * ns + 2, torch.int32), Out(m, (row0 + R) * ns + 2, torch.float32)
        m.test_token_step(3, R=R, row0=row0, n_steps=ns, n_prompt=P, pad_id=pad, V=V, tokens_out=tokens.view, scores_out=scores.view if with_scores else None,
                          row_pos=_dev(m, np.concatenate([np.zeros(row0, np.int32), pos])), row_out=_dev(m, np.concatenate([np.zeros(row0, np.int64), out_at])))
        want_t = np.full(tokens.shape, np.int32(SENT))
        for f, at in zip(froms, out_at):
            want_t[at + f:at + ns] = pad
        want_s = np.where(want_t == pad, 0.0, SENT).astype(np.float32) if with_scores else np.full(tokens.shape, np.float32(SENT))
        assert np.array_equal(tokens.read(), want_t) and np.array_equal(scores.read(), want_s)
    for f in froms:
        tokens, scores = Out(m, (row0 + 2) * ns, torch.int32), Out(m, (row0 + 2) * ns, torch.float32)
        m.test_token_step(4, R=2, row0=row0, n_steps=ns, pad_id=pad, from_=f, tokens_out=tokens.view, scores_out=scores.view)
        want_t = np.full((row0 + 2, ns), np.int32(SENT))
        want_t[row0:, f:] = pad
        assert np.array_equal(tokens.read().reshape(want_t.shape), want_t)
        assert np.array_equal(scores.read().reshape(want_t.shape), np.where(want_t == pad, 0.0, SENT).astype(np.float32))


def test_qkv0_embed_over_a_slice(m):
    V, v0, n = 272, 200, 72
    c = S.make_case(np.zeros((1, V), np.float32), seed=80)
    o = _init_buffers(m, n, n + 1)
    m.test_token_step(5, R=n, V=V, n_steps=1, v0=v0, embed=_dev(m, c.embed), ssq_stride=n + 1, h=o["h"].view, ssq=o["ssq"].view)
    h, ssq0 = S.embed_ref(c.embed, None, np.arange(v0, v0 + n), np.arange(n), 1)
    worst = _check_embed(o["h"].read().reshape(n, S.D), o["ssq"].read().reshape(32, n + 1), h, ssq0, 0, n)
    _record("qkv0_embed_slice", dict(rows=n, ssq_err_over_bound=worst))


# ----------------------------------------------------------------------------- refusals
def _refused(f, *a, **kw):
    with pytest.raises((ValueError, _lib.YMT3Error)):
        f(*a, **kw)


def test_token_step_door_refuses(m):
    """the C side's own refusals (YMT3_ERR_ARG), past the wrapper: a raw argument struct per requirement; the door stays usable"""
    dev = m.device
    V, R, L, ns = 48, 4, 6, 3
    f32 = lambda n: torch.zeros(n, device=dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    bf = lambda n: torch.zeros(n, dtype=torch.bfloat16, device=dev)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)
    logits, h, ssq, embed, chan = f32(R * V), f32(R * 512), f32(32 * R), bf(V * 512), bf(2 * 512)
    fin, state, tok, sc, lo, forced, prompt = i32(R), i32(R), i32(R * ns), f32(R * ns), f32(R * ns * V), i32(R * ns), i32(R * 2)
    ticket, zs, so = i32(64), i32(5 * 32), i32(4)
    al, nx, start = torch.full((2 * 2,), -1, dtype=torch.int32, device=dev), i32(2 * V), i32(R)
    tab, q0, kc = bf(V * 1536), bf(R * 512), bf(R * 8 * L * 64)
    rpos, rout, rpr = i32(R), i64(R), i64(R)
    p = lambda t: t.data_ptr()

    def raw(op, **f):
        base = dict(logits=p(logits), h=p(h), embed=p(embed), finished=p(fin), ssq=p(ssq), tokens_out=p(tok), ssq_stride=R, row0=0, R=R, V=V, d=512,
                    n_channels=1, eos_id=-1, pad_id=0, n_steps=ns)
        base.update(f)
        a = _lib.TokenStepArgs(**base)
        return m._lib.ymt3_test_token_step(m._handle, op, ctypes.byref(a), m._stream())

    con = dict(c_allowed=p(al), c_next=p(nx), row_state=p(state), c_words=2, c_n_states=2)
    gat = dict(qkv0=p(tab), q0=p(q0), kcache0=p(kc), vcache0=p(kc), H=8, L=L)
    slot = dict(row_pos=p(rpos), row_out=p(rout), row_prompt=p(rpr))
    good = [raw(0), raw(1), raw(1, **con), raw(1, **gat), raw(1, **slot), raw(2, **slot), raw(3, **slot), raw(4, from_=1), raw(5),
            raw(1, ticket=p(ticket), zero_sync=p(zs), zero_lines=5, state_out=p(so)), raw(0, c_start=p(start), **con)]
    assert all(rc == 0 for rc in good), good
    assert raw(1, step=1, keep_shared=1, **con) == 0              # the block holds the previous call's automaton at position 0 + 1
    bad = [raw(6), raw(-1), raw(1, R=0), raw(1, R=0x10000), raw(1, row0=-1), raw(1, row0=0x10000), raw(1, n_steps=0), raw(1, n_prompt=-1), raw(1, state_out=p(so) + 4),
           raw(1, h=None), raw(1, embed=p(embed) + 2), raw(1, ssq=None), raw(1, V=0), raw(1, d=0), raw(1, n_channels=0), raw(1, pad_id=V), raw(1, pad_id=-1),
           raw(1, eos_id=V), raw(1, chan_embed=p(chan) + 2), raw(1, finished=None), raw(0, row0=1, ssq_stride=R + 1), raw(1, ssq_stride=R - 1),
           raw(2, n_channels=R + 1, **slot), raw(1, **dict(gat, q0=None)), raw(1, **dict(gat, H=4)), raw(1, **dict(gat, L=0)),
           raw(1, chan_embed=p(chan), **gat), raw(1, n_channels=2, **gat), raw(1, row_state=p(state) + 4), raw(1, **dict(con, c_next=None)),
           raw(1, **dict(con, row_state=None)), raw(1, **dict(con, c_n_states=0)), raw(1, **dict(con, c_words=1)), raw(1, c_next=p(nx)),
           raw(1, c_start=p(start), **con), raw(0, c_start=p(start), c_n_states=2), raw(0, c_start=p(start), row_state=p(state)),
           raw(0, **slot), raw(4, **slot), raw(5, **slot), raw(2), raw(3), raw(1, row_out=p(rout)), raw(1, row_prompt=p(rpr)),
           raw(1, tokens_out=p(tok) + 4), raw(1, forced=p(forced) + 4), raw(1, logits_out=p(lo) + 4), raw(1, scores_out=p(sc) + 4), raw(1, prompt=p(prompt) + 4),
           raw(1, n_prompt=1), raw(0, n_prompt=1), raw(0, step0=-1), raw(0, step0=L, **gat), raw(0, forced=p(forced), tokens_out=None),
           raw(1, logits=None), raw(1, tokens_out=None), raw(1, ticket=p(ticket) + 4), raw(1, zero_sync=p(zs), zero_lines=0), raw(1, zero_lines=2),
           raw(1, keep_shared=1, n_steps=ns + 1), raw(1, keep_shared=1, R=R - 1, **con), raw(1, keep_shared=1, row0=1, R=R - 1, **con), raw(1, keep_shared=1, n_prompt=1, prompt=p(prompt)), raw(1, keep_shared=1),
           raw(1, forced=p(forced), **slot), raw(1, logits_out=p(lo), **slot), raw(1, n_prompt=1, prompt=p(prompt), **dict(slot, row_prompt=None)),
           raw(1, step=-1), raw(1, step0=1, step=0), raw(1, step=ns), raw(1, step=L, n_steps=L + 2, **gat),
           raw(2, **dict(slot, row_prompt=None)), raw(2, first_out=-1, **slot), raw(3, tokens_out=None, **slot), raw(4, tokens_out=None),
           raw(4, from_=-1), raw(4, from_=ns + 1), raw(5, row0=1, ssq_stride=R + 1), raw(5, chan_embed=p(chan)), raw(5, v0=-1), raw(5, v0=V - R + 1)]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert raw(1) == 0 and raw(0) == 0
    torch.cuda.synchronize()


def test_token_step_wrapper_refuses_values_on_the_device(m):
    """the wrapper's checks of what the kernels follow: positions, offsets, states, the next-state table"""
    c, _ = _CASES["slot_rows"]
    dev = m.device
    kw = dict(R=c.R, V=c.V, n_steps=c.n_steps, n_prompt=c.n_prompt, eos_id=c.eos_id, pad_id=c.pad_id, logits=_dev(m, c.logits), embed=_dev(m, c.embed),
              ssq_stride=c.stride, h=torch.zeros(c.rows * 512, device=dev), ssq=torch.zeros(32 * c.stride, device=dev), finished=_dev(m, c.finished),
              tokens_out=torch.zeros(c.n_out, dtype=torch.int32, device=dev), prompt=_dev(m, c.prompt), c_allowed=_dev(m, S.allowed_words(c.allowed)),
              c_next=_dev(m, c.next), c_n_states=2, row_state=_dev(m, c.state), row_pos=_dev(m, c.row_pos), row_out=_dev(m, c.row_out),
              row_prompt=_dev(m, c.row_prompt))
    def but(**f):
        return dict(kw, **{k: (_dev(m, v) if isinstance(v, np.ndarray) else v) for k, v in f.items()})
    bump = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(a.dtype)
    _refused(m.test_token_step, 1, **but(row_pos=bump(c.row_pos, 0, -1)))
    _refused(m.test_token_step, 1, **but(row_pos=bump(c.row_pos, 1, c.n_prompt + c.n_steps)))
    _refused(m.test_token_step, 1, **but(row_out=bump(c.row_out, 2, c.n_out - c.n_steps + 1)))
    _refused(m.test_token_step, 1, **but(row_prompt=bump(c.row_prompt, 0, 15)))
    _refused(m.test_token_step, 1, **but(row_state=bump(c.state, 3, 2)))
    _refused(m.test_token_step, 1, **but(c_next=bump(c.next.flatten(), 5, 2)))
    _refused(m.test_token_step, 1, **but(tokens_out=torch.zeros(c.n_steps - 1, dtype=torch.int32, device=dev)))
    m.test_token_step(1, **kw)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- beam select, W = 1: the greedy pick through the beam kernels
class _BeamState:
    """every buffer of a beam door call for G groups of W beams; the ancestry bytes start at 0xAB (uint8 holds no SENT)"""

    def __init__(self, m, G, W, V, ns, N, embed, P=0):
        R = G * W
        self.R, self.W, self.V, self.ns, self.N, self.pitch, self.fed = R, W, V, ns, N, 16, ns + P + 2
        self.o = dict(h=Out(m, R * S.D, torch.float32), ssq=Out(m, 32 * (R + 1), torch.float32), tokens=Out(m, G * N * ns, torch.int32),
                      seq=Out(m, G * N, torch.float32), tok=Out(m, G * N * ns, torch.float32), state_out=Out(m, 4, torch.int32),
                      fed_tok=Out(m, R * self.fed, torch.int32), fed_lp=Out(m, R * self.fed, torch.float32))
        for k, dt in (("finished", torch.int32), ("run", torch.float32), ("fin_score", torch.float32), ("fin_len", torch.int32),
                      ("fin_store", torch.int32), ("fin_tok", torch.int32), ("fin_lp", torch.float32)):
            self.o[k] = Out(m, R, dt)
        self.o["n_fin"] = Out(m, G, torch.int32)
        self.anc = torch.full((2 * R * self.pitch,), 0xAB, dtype=torch.uint8, device=m.device)
        self.slot_anc = torch.full((R * self.pitch,), 0xAB, dtype=torch.uint8, device=m.device)
        o = self.o
        self.kw = dict(R=R, W=W, V=V, n_steps=ns, N=N, anc_rows=R, anc_pitch=self.pitch, fed_pitch=self.fed, embed=embed, ssq_stride=R + 1, h=o["h"].view,
                       ssq=o["ssq"].view, finished=o["finished"].view, anc=self.anc, slot_anc=self.slot_anc, fed_tok=o["fed_tok"].view,
                       fed_lp=o["fed_lp"].view, run=o["run"].view, fin_score=o["fin_score"].view, fin_len=o["fin_len"].view,
                       fin_store=o["fin_store"].view, fin_tok=o["fin_tok"].view, fin_lp=o["fin_lp"].view, n_fin=o["n_fin"].view,
                       tokens_out=o["tokens"].view, seq_out=o["seq"].view, tok_out=o["tok"].view, state_out=o["state_out"].view, alpha=0.0)

    def read(self, k):
        return self.o[k].read()


@pytest.mark.parametrize("V", [16, 272, 1536])
def test_beam_w1_chain_equals_the_greedy_door_bit_for_bit(m, V):
    """init -> three selects on host-made logits -> finalize with one beam per group, every call after the first on the blocks the previous one
    left: ids, h, ssq and scores of every step equal op 1 of the greedy door on the same logits bit for bit (the claim of beam_embed_row's and
    the select kernel's comments), the run is the fp32 sum of the scores, and the third step (the length limit) fills the slot"""
    G, ns, pad = 5, 3, 1
    rng = np.random.default_rng(V + 90)
    steps = [rng.uniform(-3, 3, (G, V)).astype(np.float32) for _ in range(ns)]
    for x in steps:                                               # a clear winner per row: the running sum rounds no two candidates together
        x[np.arange(G), rng.integers(0, V, G)] = 4.5
    steps[1][2, [3, V - 1]] = 7.0                                 # an exact tie: the lower index
    cases = [S.make_case(x, seed=V, pad_id=pad, n_steps=ns, step=j) for j, x in enumerate(steps)]
    b = _BeamState(m, G, 1, V, ns, 1, _dev(m, cases[0].embed))
    m.test_beam_step(0, pad_id=pad, **b.kw)
    assert np.array_equal(b.read("state_out"), [0, 0, G, ns]) and np.array_equal(b.read("run"), np.zeros(G, np.float32))
    assert np.array_equal(b.read("n_fin"), np.zeros(G, np.int32)) and np.array_equal(b.read("fin_store"), np.zeros(G, np.int32))
    h, ssq0 = S.embed_ref(cases[0].embed, None, np.full(G, pad), np.arange(G), 1)
    _check_embed(b.read("h").reshape(G, S.D), b.read("ssq").reshape(32, G + 1), h, ssq0, 0, G)
    run = np.zeros(G, np.float32)
    toks, lps = [], []
    for j, c in enumerate(cases):
        g = _launch(m, c)
        m.test_beam_step(1, pad_id=pad, logits=_dev(m, c.logits), keep_shared=True, **b.kw)
        tok, lp = g.tokens.reshape(G, ns)[:, j], g.scores.reshape(G, ns)[:, j]
        assert np.array_equal(tok, S.token_step_ref(c).tokens.reshape(G, ns)[:, j])
        fed_tok, fed_lp = b.read("fed_tok").reshape(G, b.fed), b.read("fed_lp").reshape(G, b.fed)
        assert np.array_equal(fed_tok[:, j + 1], tok) and np.array_equal(fed_lp[:, j + 1].view(np.uint32), lp.view(np.uint32))
        assert (fed_tok[:, j + 2:] == SENT).all() and (fed_tok[:, 0] == SENT).all()
        assert np.array_equal(b.read("h").view(np.uint32), g.h.view(np.uint32).flatten())
        assert np.array_equal(b.read("ssq").reshape(32, G + 1)[:, :G].view(np.uint32), g.ssq[:, :G].view(np.uint32))
        run = run + lp                                             # fp32: run[w] + lp
        last = j == ns - 1
        assert np.array_equal(b.read("run").view(np.uint32), (run + np.float32(-1e9) if last else run).astype(np.float32).view(np.uint32))
        assert np.array_equal(b.read("state_out"), [j + 1, 0, 0 if last else G, ns])
        assert np.array_equal(b.read("n_fin"), np.full(G, int(last), np.int32)) and np.array_equal(b.read("finished"), np.full(G, int(last), np.int32))
        anc = b.anc.cpu().numpy().reshape(2, G, b.pitch)
        words = (j + 1) // 4 + 1
        assert (anc[(j + 1) & 1, :, :j + 2] == 0).all() and (anc[(j + 1) & 1, :, 4 * words:] == 0xAB).all()
        toks.append(tok)
        lps.append(lp)
    assert np.array_equal(b.read("fin_score").view(np.uint32), run.view(np.uint32)) and np.array_equal(b.read("fin_len"), np.full(G, ns, np.int32))
    assert np.array_equal(b.read("fin_tok"), toks[-1]) and np.array_equal(b.read("fin_lp").view(np.uint32), lps[-1].view(np.uint32))
    assert (b.slot_anc.cpu().numpy().reshape(G, b.pitch)[:, :ns] == 0).all()
    m.test_beam_step(2, pad_id=pad, keep_shared=True, **b.kw)
    assert np.array_equal(b.read("tokens").reshape(G, ns), np.stack(toks, 1))
    assert np.array_equal(b.read("tok").reshape(G, ns).view(np.uint32), np.stack(lps, 1).view(np.uint32))
    assert np.array_equal(b.read("seq").view(np.uint32), run.view(np.uint32))
    _record(f"beam_w1_chain_V{V}", dict(groups=G, steps=ns, bit_equal=True))


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("V", [16, 272])
def test_beam_step0_expands_beam_0_only(m, W, V):
    """init -> the first select, two groups: the W new beams are the W best tokens of beam 0 in order (beam_oracle.host_select on float64
    log-probabilities; every comparison has a margin of 0.01 or 1e9), each with parent 0: ancestry entry 0 is the parent's, entry 1 the row's
    own index, the rest of the word the parent's bytes, nothing beyond it"""
    from beam_oracle import host_select
    G, ns, pad = 2, 4, 1
    x, _, acc = S.beam_step0_case(G, W, V)
    c = S.make_case(x, seed=W, pad_id=pad, n_steps=ns)
    b = _BeamState(m, G, W, V, ns, 1, _dev(m, c.embed))
    m.test_beam_step(0, pad_id=pad, **b.kw)
    assert np.array_equal(b.read("run"), np.tile(np.array([0.0] + [-1e9] * (W - 1), np.float32), G))
    assert np.array_equal(b.read("fin_store"), np.tile(np.arange(W, dtype=np.int32), G))
    m.test_beam_step(1, pad_id=pad, logits=_dev(m, x), keep_shared=True, **b.kw)
    R = G * W
    want = [host_select(acc[g], W, -1, False, [], 1, 0.0)["beams"] for g in range(G)]
    tok = np.array([t for g in range(G) for _, t, _ in want[g]], np.int32)
    run = np.array([r for g in range(G) for _, _, r in want[g]])
    fed_tok, fed_lp = b.read("fed_tok").reshape(R, b.fed), b.read("fed_lp").reshape(R, b.fed)
    assert np.array_equal(fed_tok[:, 1], tok) and (fed_tok[:, 2:] == SENT).all() and (fed_tok[:, 0] == SENT).all()
    ok1, w1 = S.compare_scores(run, b.read("run"))
    ok2, w2 = S.compare_scores(run, fed_lp[:, 1])
    assert ok1 and ok2
    h, ssq0 = S.embed_ref(c.embed, None, tok, np.arange(R), 1)
    _check_embed(b.read("h").reshape(R, S.D), b.read("ssq").reshape(32, R + 1), h, ssq0, 0, R)
    anc = b.anc.cpu().numpy().reshape(2, R, b.pitch)
    own = np.tile(np.arange(W, dtype=np.uint8), G)
    assert (anc[1, :, 0] == 0).all() and np.array_equal(anc[1, :, 1], own) and (anc[1, :, 2:] == 0xAB).all()
    assert np.array_equal(anc[0, :, 0], own) and (anc[0, :, 1:] == 0xAB).all()
    assert np.array_equal(b.read("state_out"), [1, 0, R, ns]) and (b.read("n_fin") == 0).all() and (b.read("finished") == 0).all()
    assert (b.slot_anc.cpu() == 0xAB).all()
    _record(f"beam_step0_W{W}_V{V}", dict(score_err_over_bound=max(w1, w2)))


_SEQ = S.beam_sequences()


def _beam_read(b, step, constrained, slot=False):
    """the device's beam state as select_kernel_model.beam_step_ref takes it"""
    R = b.R
    s = SimpleNamespace(step=step, anc=b.anc.cpu().numpy().reshape(2, R, b.pitch), slot_anc=b.slot_anc.cpu().numpy().reshape(R, b.pitch),
                        fed_tok=b.read("fed_tok").reshape(R, b.fed), fed_lp=b.read("fed_lp").reshape(R, b.fed),
                        row_state=b.read("row_state") if constrained else None, state_out=b.read("state_out"))
    for k in ("run", "finished", "fin_score", "fin_len", "fin_store", "fin_tok", "fin_lp", "n_fin") + (("row_pos", "row_out", "row_prompt") if slot else ()):
        setattr(s, k, b.read(k))
    return s


@pytest.mark.parametrize("name", list(_SEQ))
def test_beam_sequence_every_step_equals_the_reference(m, name):
    """init -> one select per position on host-made logits -> finalize, all on the door's own blocks (keep_shared).  Every step is judged alone:
    the reference starts from the device's own state before the step, every comparison it makes is an exact tie or has a margin >= 2e-4
    (asserted), and the WHOLE state after the step is compared: run, fed_*, fin_*, n_fin, finished, both ancestry buffers, slot_anc,
    row_state, h, ssq, state_out.  The result kernel's tokens are the histories followed on the host, its scores the device's own bits."""
    p, steps, N, _, _ = _SEQ[name]
    G, W, V, R = p.G, p.W, p.V, p.G * p.W
    con = p.allowed is not None
    b = _BeamState(m, G, W, V, p.ns, N, _dev(m, p.embed), P=p.P)
    kw = dict(b.kw, n_prompt=p.P, prompt=_dev(m, p.prompt.astype(np.int32)) if p.P else None, eos_id=p.eos, pad_id=p.pad, alpha=p.alpha,
              n_channels=p.n_channels, chan_embed=_dev(m, p.chan))
    if con:
        b.o["row_state"] = Out(m, R, torch.int32)
        kw.update(c_allowed=_dev(m, S.allowed_words(p.allowed)), c_next=_dev(m, p.next), c_n_states=len(p.allowed), row_state=b.o["row_state"].view)
    m.test_beam_step(0, **kw)
    s = _beam_read(b, 0, con)
    want = S.beam_init_state(p)
    want.state_out = np.array([0, 0, R, p.ns], np.int32)
    bad, _ = S.beam_compare(SimpleNamespace(**{k: (v.astype(np.float64) if k in S.BEAM_F else v) for k, v in vars(want).items()}), s)
    assert not bad, bad
    hist = [[([], []) for _ in range(W)] for _ in range(G)]               # (tokens, log-probabilities) of every running beam
    hyp = {}                                                              # (group, snapshot row) -> the same of a finished hypothesis, less its last lp
    worst = worst_ssq = 0.0
    for t, x in enumerate(steps):
        ref, ev = S.beam_step_ref(s, x, p)
        assert ev["undecided"] == 0, (t, ev)
        m.test_beam_step(1, logits=_dev(m, x), keep_shared=True, **kw)
        got = _beam_read(b, t + 1, con)
        bad, w = S.beam_compare(ref, got)
        assert not bad, (t, bad)
        worst = max(worst, w)
        want_h = ref.h.reshape(R, S.D)
        worst_ssq = max(worst_ssq, _check_embed(b.read("h").reshape(R, S.D), b.read("ssq").reshape(32, R + 1), want_h, ref.ssq0, 0, R))
        if t >= p.P:
            for g in range(G):
                if s.n_fin[g] >= W:
                    continue
                old = hist[g]
                for gg, st, par, tok in ref.entered:
                    if gg == g:
                        hyp[(g, st)] = (old[par][0] + [tok], list(old[par][1]))
                hist[g] = [(old[ref.parent[g * W + i]][0] + [int(ref.feed[g * W + i])], old[ref.parent[g * W + i]][1] + [got.fed_lp[g * W + i, t + 1]])
                           for i in range(W)]
        s = got
    assert (s.n_fin == W).all()
    m.test_beam_step(2, keep_shared=True, **kw)
    tokens, tok_lp, seq = b.read("tokens").reshape(G, N, p.ns), b.read("tok").reshape(G, N, p.ns), b.read("seq").reshape(G, N)
    for g in range(G):
        for n in range(N):
            o = g * W + n
            toks, lps = hyp[(g, int(s.fin_store[o]))]
            ln = int(s.fin_len[o])
            assert len(toks) == ln and toks[-1] == s.fin_tok[o]
            assert np.array_equal(tokens[g, n], toks + [p.pad] * (p.ns - ln))
            want_lp = np.array(lps + [s.fin_lp[o]] + [0.0] * (p.ns - ln), np.float32)
            assert np.array_equal(tok_lp[g, n].view(np.uint32), want_lp.view(np.uint32))
            assert seq[g, n].view(np.uint32) == s.fin_score[o].view(np.uint32)
    _record("beam_seq_" + name, dict(groups=G, W=W, V=V, positions=len(steps), differs="", score_err_over_bound=worst, ssq_err_over_bound=worst_ssq))


def test_beam_slot_mode_groups_at_their_own_positions(m):
    """beam_slot_start, slot-mode selects and beam_slot_finalize: three slots started one launch apart, so every launch sees groups at different
    positions, empty or done ones stopped beside live ones.  Each launch is judged alone from the device's own state, the whole state compared;
    a stopped group changes nothing but its pad feed; the results land at the groups' queue indices and nowhere else."""
    p, n_queue, actions = S.beam_slot_case()
    G, W, V, R, N = p.G, p.W, p.V, p.G * p.W, 2
    b = _BeamState(m, G, W, V, p.ns, N, _dev(m, p.embed), P=p.P)
    b.o.update(finished=Out(m, np.ones(R, np.int32)), row_pos=Out(m, R, torch.int32), row_out=Out(m, R, torch.int64), row_prompt=Out(m, R, torch.int64),
               tokens=Out(m, n_queue * N * p.ns, torch.int32), seq=Out(m, n_queue * N, torch.float32), tok=Out(m, n_queue * N * p.ns, torch.float32))
    o = b.o
    kw = dict(b.kw, n_prompt=p.P, prompt=_dev(m, p.prompt.astype(np.int32)), eos_id=p.eos, pad_id=p.pad, alpha=p.alpha, N=N, n_queue=n_queue,
              finished=o["finished"].view, row_pos=o["row_pos"].view, row_out=o["row_out"].view, row_prompt=o["row_prompt"].view,
              tokens_out=o["tokens"].view, seq_out=o["seq"].view, tok_out=o["tok"].view)
    s = _beam_read(b, 0, False, slot=True)
    hist = [[([], []) for _ in range(W)] for _ in range(G)]
    hyp, worst, queue_of = {}, 0.0, {}
    pad_h, _ = S.embed_ref(p.embed, None, np.full(W, p.pad), np.arange(W), 1)
    for a in actions:
        if a[0] == "start":
            m.test_beam_step(3, row0=a[1], first_group=a[2], **kw)
            ref = S.beam_slot_start_ref(s, p, a[1], a[2])
            got = _beam_read(b, 0, False, slot=True)
            ref.state_out = got.state_out
            for k in S.BEAM_F:
                setattr(ref, k, getattr(ref, k).astype(np.float64))
            bad, _ = S.beam_compare(ref, got)
            assert not bad, (a[:3], bad)
            assert np.array_equal(b.read("h").reshape(R, S.D)[a[1]:a[1] + W].view(np.uint32), pad_h.view(np.uint32))
            hist[a[1] // W] = [([], []) for _ in range(W)]
            queue_of[a[1] // W] = a[2]
            s = got
            continue
        s.state_out = np.array([0, 0, R, p.ns], np.int32)
        ref, ev = S.beam_step_ref(s, a[1], p)
        assert ev["undecided"] == 0
        m.test_beam_step(1, logits=_dev(m, a[1]), **kw)
        got = _beam_read(b, 0, False, slot=True)
        bad, w = S.beam_compare(ref, got)
        assert not bad, bad
        worst = max(worst, w)
        _check_embed(b.read("h").reshape(R, S.D), b.read("ssq").reshape(32, R + 1), ref.h.reshape(R, S.D), ref.ssq0, 0, R)
        for g in range(G):
            t = int(s.row_pos[g * W])
            if s.finished[g * W] or t < p.P:
                continue
            old = hist[g]
            for gg, st, par, tok in ref.entered:
                if gg == g:
                    hyp[(g, st)] = (old[par][0] + [tok], list(old[par][1]))
            hist[g] = [(old[ref.parent[g * W + i]][0] + [int(ref.feed[g * W + i])], old[ref.parent[g * W + i]][1] + [got.fed_lp[g * W + i, t + 1]]) for i in range(W)]
        s = got
    assert (s.n_fin == W).all() and (s.finished == 1).all()
    want_t = np.full((n_queue, N, p.ns), np.int32(SENT))
    want_lp = np.full((n_queue, N, p.ns), np.float32(SENT))
    want_seq = np.full((n_queue, N), np.float32(SENT))
    for g in range(G):
        m.test_beam_step(4, row0=g * W, **kw)
        for n in range(N):
            r = g * W + n
            toks, lps = hyp[(g, int(s.fin_store[r]))]
            ln = int(s.fin_len[r])
            assert len(toks) == ln
            want_t[queue_of[g], n] = toks + [p.pad] * (p.ns - ln)
            want_lp[queue_of[g], n] = np.array(lps + [s.fin_lp[r]] + [0.0] * (p.ns - ln), np.float32)
            want_seq[queue_of[g], n] = s.fin_score[r]
    assert np.array_equal(b.read("tokens").reshape(want_t.shape), want_t)
    assert np.array_equal(b.read("tok").reshape(want_lp.shape).view(np.uint32), want_lp.view(np.uint32))
    assert np.array_equal(b.read("seq").reshape(want_seq.shape).view(np.uint32), want_seq.view(np.uint32))
    _record("beam_slot_mode", dict(groups=G, W=W, V=V, launches=len(actions), differs="", score_err_over_bound=worst))


def test_beam_step_door_refuses(m):
    b = _BeamState(m, 2, 2, 48, 3, 1, torch.zeros(48 * 512, dtype=torch.bfloat16, device=m.device))
    logits = torch.zeros(4 * 48, device=m.device)
    m.test_beam_step(0, **b.kw)
    m.test_beam_step(1, logits=logits, keep_shared=True, **b.kw)
    for bad in (dict(W=3), dict(W=9, R=9, anc_rows=9), dict(anc_rows=3), dict(anc_pitch=24), dict(n_steps=15), dict(fed_pitch=3), dict(pad_id=48),
                dict(eos_id=48), dict(ssq_stride=3), dict(alpha=-1.0), dict(N=3), dict(N=0), dict(step=3), dict(step=-1), dict(n_prompt=1),
                dict(keep_shared=True, n_steps=2), dict(logits=None), dict(tokens_out=None)):
        kw = dict(b.kw, logits=logits)
        kw.update(bad)
        _refused(m.test_beam_step, 1, **kw)
    _refused(m.test_beam_step, 3, **b.kw)
    _refused(m.test_beam_step, 4, **b.kw)
    p = lambda t: t.data_ptr()
    k = b.kw

    def raw(op, **f):
        base = dict(logits=p(logits), h=p(k["h"]), embed=p(k["embed"]), finished=p(k["finished"]), ssq=p(k["ssq"]), anc=p(b.anc), slot_anc=p(b.slot_anc),
                    fed_tok=p(k["fed_tok"]), fed_lp=p(k["fed_lp"]), run=p(k["run"]), fin_score=p(k["fin_score"]), fin_len=p(k["fin_len"]),
                    fin_store=p(k["fin_store"]), fin_tok=p(k["fin_tok"]), fin_lp=p(k["fin_lp"]), n_fin=p(k["n_fin"]), tokens_out=p(k["tokens_out"]),
                    ssq_stride=5, R=4, V=48, d=512, n_channels=1, eos_id=-1, pad_id=0, W=2, anc_rows=4, anc_pitch=16, fed_pitch=5, n_steps=3, N=1, alpha=1.0)
        base.update(f)
        a = _lib.BeamStepArgs(**base)
        return m._lib.ymt3_test_beam_step(m._handle, op, ctypes.byref(a), m._stream())

    assert raw(0) == 0 and raw(1) == 0 and raw(2) == 0
    bad = [raw(5), raw(1, h=None), raw(1, anc=p(b.anc) + 4), raw(1, W=0), raw(1, R=3), raw(1, anc_rows=2), raw(1, V=0), raw(1, ssq_stride=3),
           raw(1, pad_id=-1), raw(1, eos_id=48), raw(1, n_steps=0), raw(1, n_prompt=1), raw(1, anc_pitch=8), raw(1, fed_pitch=3), raw(1, c_next=p(logits)),
           raw(1, c_allowed=p(logits), c_next=p(logits), c_words=2, c_n_states=1), raw(1, c_start=p(logits)), raw(0, row_pos=p(logits)),
           raw(3), raw(4), raw(1, row_out=p(logits)), raw(1, tokens_out=None), raw(1, alpha=-1.0), raw(1, logits=None), raw(1, step=3),
           raw(1, keep_shared=1, n_steps=2), raw(1, keep_shared=1, R=2), raw(2, N=3), raw(2, N=0)]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert raw(0) == 0 and raw(1, keep_shared=1) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the handle's own state (LAST test of the module)
def test_handle_calls_after_the_doors_give_the_same_bits(m):
    after = _handle_calls(m)
    assert len(after) == len(_BEFORE["out"])
    for a, b in zip(after, _BEFORE["out"]):
        assert torch.equal(a, b) or (a.is_floating_point() and torch.equal(a.view(torch.int32), b.view(torch.int32)))
