"""float64 / NumPy reference of the token-selection stage as include/ymt3.h states it (greedy pick: the decode, scores and constraint
sections plus the rules under ymt3_test_token_step; beam select: the beam-search section through beam_oracle.host_select), the case builders of
tests/test_select_kernels.py and the mutants tests/test_select_kernels_cpu.py shows those cases to reject.  Not a restatement of the kernels'
instruction order: ids come from comparisons over the whole row, scores from a float64 log-softmax.

A greedy CASE is one launch of op 1: every buffer the launch reads, `before` the launch (rows below row0 and every cell the launch must not
touch hold SENT).  token_step_ref(case) gives every buffer `after` it.  compare() judges two such dicts by the criteria of the test module:
integers, copies and h exactly, ssq[0] within (d + 2) 2^-24 sum(v^2), scores within 1e-4 + 1e-5 |ref| with the prescribed specials as such.
"""
import itertools
from types import SimpleNamespace

import numpy as np

SENT = 12352.0                     # tests/test_encoder_kernels.SENT: exact in bf16, fp32 and int32
SENT_BF16 = 0x4641                 # its bf16 bits
D = 512
NO_INDEX = 0x7fffffff
MUTANTS = ("tie_high", "skip_partial_stride", "mask_word_off_by_one", "scan_start_zero", "lse_unmasked", "dropped_term", "no_pad_after_eos",
           "automaton_not_frozen", "last_group_32", "kv_at_L", "forced_unclamped", "nan_wins")
BEAM_MUTANTS = ("beam_tie_high", "anc_at_t", "snapshot_not_reused", "beam_lse_unmasked", "fill_not_zero", "hit_outside_w_enters", "all_beams_step0")


def bf16_bits(x):
    """float array -> bf16 bits (uint16), round to nearest even"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_f32(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def clamp(i, V):
    return min(max(int(i), 0), V - 1)


# ----------------------------------------------------------------------------- the rules
def pick(row, allowed=None, mut=()):
    """the emitted index of one logits row: the first maximum over the allowed, non-NaN logits that compare greater than -3.4e38, otherwise the
    lowest allowed index, clamped into [0, V) (a state that allows nothing: V - 1)"""
    V = row.size
    ok = np.ones(V, bool) if allowed is None else allowed.copy()
    if "mask_word_off_by_one" in mut and allowed is not None:
        ok = np.concatenate([allowed[32:], np.zeros(32, bool)])[:V]
    if "skip_partial_stride" in mut and V % 256:
        ok[V - V % 256:] = False
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return 0 if "scan_start_zero" in mut else V - 1
    v = row[idx].astype(np.float64)
    if "nan_wins" in mut and np.isnan(v).any():
        return int(idx[np.flatnonzero(np.isnan(v))[0]])
    comp = ~np.isnan(v) & (v > np.float64(np.float32(-3.4e38)))
    if not comp.any():
        return 0 if ("scan_start_zero" in mut and allowed is not None) else int(idx[0])
    best = v[comp].max()
    hits = idx[comp][v[comp] == best]
    return int(hits[-1] if "tie_high" in mut else hits[0])


def score(row, ident, allowed=None, mut=()):
    """log_softmax over the allowed set at `ident` in float64; NaN for a row with a NaN or without a finite allowed logit, -inf for an id the
    state does not allow"""
    if allowed is not None and not allowed[ident]:
        return -np.inf
    ok = np.ones(row.size, bool) if allowed is None or "lse_unmasked" in mut else allowed
    v = row[ok].astype(np.float64)
    if "dropped_term" in mut:
        v = v[:-1]
    if v.size == 0 or np.isnan(v).any() or not (v > -np.inf).any() or np.isposinf(v).any():
        return np.nan
    mx = v.max()
    return float(row[ident]) - mx - np.log(np.exp(v - mx).sum())


def embed_ref(embed_bits, chan_bits, feed, rows, n_channels):
    """h = f32(bf16 e) + f32(bf16 c) (one fp32 add) and the float64 sum of its squares, for the given rows"""
    e = bf16_f32(embed_bits[feed])
    h = e + bf16_f32(chan_bits[np.asarray(rows) % n_channels]) if chan_bits is not None else e.copy()
    return h.astype(np.float32), (h.astype(np.float64) ** 2).sum(-1)


# ----------------------------------------------------------------------------- greedy cases
def make_case(logits, *, row0=0, seed=0, eos_id=-1, pad_id=0, n_steps=4, n_prompt=0, step=0, step0=0, finished=None, forced=None, prompt=None,
              want_logits=False, want_scores=True, allowed=None, nxt=None, state=None, chan=0, ticket=False, zero_lines=0, qkv0=False, L=0,
              row_pos=None, row_out=None, row_prompt=None, n_out=0):
    """logits (R, V) -> a case.  Per-row inputs are given for the R launched rows; the buffers get row0 SENT rows in front.  chan: channel rows
    (0: no channel table).  Slot mode when row_pos is given (row_out: offsets into a tokens / scores buffer of n_out cells)."""
    rng = np.random.default_rng(1000 + seed)
    logits = np.asarray(logits, np.float32)
    R, V = logits.shape
    rows = row0 + R
    front = lambda a, fill: np.concatenate([np.full((row0,) + a.shape[1:], fill, a.dtype), a], 0)
    c = SimpleNamespace(R=R, V=V, row0=row0, rows=rows, eos_id=eos_id, pad_id=pad_id, n_steps=n_steps, n_prompt=n_prompt, step=step, step0=step0,
                        want_logits=want_logits, want_scores=want_scores, n_channels=max(chan, 1), ticket=ticket, zero_lines=zero_lines, L=L,
                        slot=row_pos is not None, stride=rows + 3)
    c.logits = front(logits, np.float32(np.nan))
    c.embed = bf16_bits(rng.integers(-64, 65, (V, D)) / 32.0)                       # bf16-exact values
    c.chan = bf16_bits(rng.integers(-64, 65, (chan, D)) / 64.0) if chan else None
    c.finished = front(np.zeros(R, np.int32) if finished is None else np.asarray(finished, np.int32), np.int32(SENT))
    c.forced = None if forced is None else front(np.asarray(forced, np.int32).reshape(R, n_steps), np.int32(0))
    c.allowed = None if allowed is None else np.asarray(allowed, bool)
    c.next = None if nxt is None else np.asarray(nxt, np.int32)
    c.state = None if allowed is None else front(np.zeros(R, np.int32) if state is None else np.asarray(state, np.int32), np.int32(SENT))
    c.qkv0 = bf16_bits(rng.integers(-96, 97, (V, 3 * D)) / 16.0) if qkv0 else None
    if c.slot:
        c.row_pos = front(np.asarray(row_pos, np.int32), np.int32(SENT))
        c.row_out = front(np.asarray(row_out, np.int64), np.int64(0))
        c.row_prompt = front(np.zeros(R, np.int64) if row_prompt is None else np.asarray(row_prompt, np.int64), np.int64(0))
        c.prompt = None if prompt is None else np.asarray(prompt, np.int32).reshape(-1)
        c.n_out = n_out
    else:
        c.prompt = None if prompt is None else front(np.asarray(prompt, np.int32).reshape(R, n_prompt), np.int32(0))
        c.n_out = rows * n_steps
    return c


def allowed_words(allowed):
    """(S, V) bool -> (S, ceil(V / 32)) uint32 mask words, bits at or beyond V set (they must be ignored)"""
    S, V = allowed.shape
    words = (V + 31) // 32
    bits = np.ones((S, words * 32), bool)
    bits[:, :V] = allowed
    return (bits.reshape(S, words, 32) * (np.uint64(1) << np.arange(32, dtype=np.uint64))).sum(-1).astype(np.uint32)


def token_step_ref(c, mut=()):
    """every buffer of the launch after it (float64 where the criterion is a bound): tokens, scores, logits_out, finished, row_pos, row_state, h,
    ssq0 (the float64 sums; ssq[1..31] are checked as zeros by compare), q0, kc, vc (flat bf16 bits), ticket, zero_sync, state_out"""
    R, V, rows, r0, ns, P = c.R, c.V, c.rows, c.row0, c.n_steps, c.n_prompt
    out = SimpleNamespace()
    out.tokens = np.full(c.n_out, np.int32(SENT))
    out.scores = np.full(c.n_out, SENT, np.float64)
    out.logits_out = np.full((c.n_out, V), np.float32(SENT)) if c.want_logits else None
    out.finished = c.finished.copy()
    out.row_pos = c.row_pos.copy() if c.slot else None
    out.row_state = c.state.copy() if c.state is not None else None
    feed = np.zeros(R, np.int64)
    kv_pos = np.full(R, c.step + 1, np.int64)
    col = c.step - c.step0 - P
    for i in range(R):
        r = r0 + i
        row = c.logits[r]
        was = bool(c.finished[r])
        st = int(c.state[r]) if c.state is not None else 0
        al = c.allowed[st] if c.allowed is not None else None
        al_s = al
        if al is not None and "mask_word_off_by_one" in mut:
            al_s = np.concatenate([al[32:], np.zeros(32, bool)])[:V]
        if c.slot:
            pos0, out0 = int(c.row_pos[r]), int(c.row_out[r])
            kv_pos[i] = pos0
            feed[i] = c.pad_id
            if was:
                continue
            if pos0 < P:
                out.row_pos[r] = kv_pos[i] = pos0 + 1
                feed[i] = clamp(c.prompt[int(c.row_prompt[r]) + pos0], V)
                continue
            p = pos0 - P
            tok = pick(row, al, mut)
            out.tokens[out0 + p] = tok
            if (c.eos_id >= 0 and tok == c.eos_id) or p + 1 >= ns:
                out.finished[r] = 1
            else:
                out.row_pos[r] = kv_pos[i] = pos0 + 1
            feed[i] = tok
            if c.want_scores:
                out.scores[out0 + p] = score(row, tok, al_s, mut)
            if al is not None:
                out.row_state[r] = c.next[st, tok]
            continue
        if col < 0:
            feed[i] = clamp(c.prompt[r, c.step - c.step0], V)
            continue
        tok = pick(row, al, mut)
        if c.eos_id >= 0:
            if was and "no_pad_after_eos" not in mut:
                tok = c.pad_id
            elif not was and tok == c.eos_id:
                out.finished[r] = 1
        cell = r * ns + col
        out.tokens[cell] = tok
        f = int(c.forced[r, col]) if c.forced is not None else tok
        f = f % V if "forced_unclamped" in mut else clamp(f, V)
        feed[i] = f
        after_eos = c.eos_id >= 0 and was
        if c.want_scores:
            out.scores[cell] = 0.0 if (c.forced is None and after_eos) else score(row, f, al_s, mut)
        if al is not None and (not after_eos or "automaton_not_frozen" in mut):
            out.row_state[r] = c.next[st, f]
        if c.want_logits:
            out.logits_out[cell] = row
    out.feed = feed
    h, ssq0 = embed_ref(c.embed, c.chan, feed, np.arange(r0, rows), c.n_channels)
    out.h = np.full((rows, D), np.float32(SENT))
    out.h[r0:] = h
    out.ssq0 = ssq0
    if c.qkv0 is not None:
        H, L = 8, c.L
        out.q0 = np.full((rows, D), SENT_BF16, np.uint16)
        out.kc = np.full(rows * H * L * 64 + 64, SENT_BF16, np.uint16)          # flat, with room for a write one position past the last slab
        out.vc = out.kc.copy()
        for i in range(R):
            r, t = r0 + i, c.qkv0[feed[i]]
            out.q0[r] = t[:D]
            if kv_pos[i] < L or "kv_at_L" in mut:
                for hh in range(H):
                    at = ((r * H + hh) * L + int(kv_pos[i])) * 64
                    out.kc[at:at + 64] = t[D + hh * 64:D + hh * 64 + 64]
                    out.vc[at:at + 64] = t[2 * D + hh * 64:2 * D + hh * 64 + 64]
    # the last arriver: the step advances, the counters are left at zero, the unfinished rows are counted when EOS accounting is on
    stuck = "last_group_32" in mut and c.ticket and R > 64 and R % 32
    n_unf = int((out.finished[r0:] == 0).sum()) if c.eos_id >= 0 and not stuck else R
    out.state_out = np.array([c.step if stuck else c.step + 1, 0, n_unf, ns], np.int32) if not c.slot else \
        np.array([0 if stuck else 1, 0, n_unf, ns], np.int32)
    out.ticket = np.zeros((R // 32 + 1) * 32, np.int32) if c.ticket else None
    if stuck:
        out.ticket[(R // 32) * 32] = R % 32
    if c.zero_lines:
        out.zero_sync = np.full(c.zero_lines * 32 + 32, np.int32(SENT))             # one line more than is zeroed
        out.zero_sync[:c.zero_lines * 32:32] = 0
    else:
        out.zero_sync = None
    return out


SCORE_ABS, SCORE_REL = 1e-4, 1e-5       # tests/test_token_scores.py


def _same_special(ref, got):
    """prescribed specials as such: NaN where NaN, the same infinity, SENT (untouched) where untouched, exactly 0.0 where 0.0"""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    special = np.isnan(ref) | np.isinf(ref) | (ref == SENT) | (ref == 0.0)
    ok = np.where(np.isnan(ref), np.isnan(got), ref == got)
    return special, bool(ok[special].all()) and bool(np.isfinite(got[~special]).all() and (got[~special] != SENT).all())


def compare_scores(ref, got):
    special, ok = _same_special(ref, got)
    ref, got = np.asarray(ref, np.float64)[~special], np.asarray(got, np.float64)[~special]
    if not ok:
        return False, float("inf")
    if ref.size == 0:
        return True, 0.0
    ratio = np.abs(got - ref) / (SCORE_ABS + SCORE_REL * np.abs(ref))
    return bool((ratio <= 1.0).all()), float(ratio.max())


def compare(c, ref, got):
    """-> (list of the quantities that differ, figures).  `got`: a namespace like token_step_ref's, with ssq (32, stride) instead of ssq0."""
    bad, fig = [], {}
    for k in ("tokens", "finished", "row_pos", "row_state", "state_out", "ticket", "zero_sync", "logits_out", "q0", "kc", "vc"):
        a, b = getattr(ref, k, None), getattr(got, k, None)
        if a is None:
            continue
        if k == "logits_out":                           # copies: bit-equal (NaN payloads included)
            same = np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
        else:
            same = np.array_equal(a, b)
        if not same:
            bad.append(k)
    if not np.array_equal(ref.h.view(np.uint32), np.asarray(got.h, np.float32).view(np.uint32)):
        bad.append("h")
    if hasattr(got, "ssq"):
        ssq = np.asarray(got.ssq, np.float64)
        bound = (D + 2) * 2.0 ** -24 * ref.ssq0
        err = np.abs(ssq[0, c.row0:c.rows] - ref.ssq0)
        fig["ssq_err_over_bound"] = float((err / np.maximum(bound, 1e-300)).max())
        untouched = np.ones(ssq.shape, bool)
        untouched[:, c.row0:c.rows] = False
        if not ((err <= bound).all() and (ssq[1:, c.row0:c.rows] == 0.0).all() and (ssq[untouched] == SENT).all()):
            bad.append("ssq")
    else:
        if not np.array_equal(ref.ssq0, got.ssq0):
            bad.append("ssq")
    if c.want_scores:
        ok, worst = compare_scores(ref.scores, got.scores)
        fig["score_err_over_bound"] = worst
        if not ok:
            bad.append("scores")
    elif not (np.asarray(got.scores) == SENT).all():
        bad.append("scores")
    return bad, fig


# ----------------------------------------------------------------------------- the named greedy cases
PLACE_V = (16, 48, 240, 256, 272, 1040, 1536)
MAX_ROWS = 97


def place_set(V):
    return sorted({i for i in (0, 15, 16, 63, 64, 255, 256, V - 17, V - 16, V - 1) if 0 <= i < V})


def placement_rows(V):
    """-> (logits (n, V), labels): a single maximum at each index of the set, an exact tie for each pair, the pair with NaN at its lower index; all
    three again with every other logit at -inf; an all-NaN row and an all--inf row.  The background is random in (-1, 1), the maximum 4.0."""
    rng = np.random.default_rng(V)
    S = place_set(V)
    rows, labels = [], []
    for rest_inf in (False, True):
        def base():
            return np.full(V, -np.inf, np.float32) if rest_inf else rng.uniform(-1, 1, V).astype(np.float32)
        for a in S:
            x = base(); x[a] = 4.0
            rows.append(x); labels.append(("single", rest_inf, a))
        for a, b in itertools.combinations(S, 2):
            x = base(); x[a] = x[b] = 4.0
            rows.append(x); labels.append(("tie", rest_inf, a, b))
            x = base(); x[a] = np.nan; x[b] = 4.0
            rows.append(x); labels.append(("nan_low", rest_inf, a, b))
    rows.append(np.full(V, np.nan, np.float32)); labels.append(("all_nan",))
    rows.append(np.full(V, -np.inf, np.float32)); labels.append(("all_ninf",))
    return np.stack(rows), labels


def placement_cases(V):
    """the placement rows of one V in launches of at most 97 rows (lock-step, scores on, logits copy on in the first launch)"""
    x, _ = placement_rows(V)
    return [make_case(x[i:i + MAX_ROWS], seed=V + i, n_steps=3, step=1, want_logits=i == 0, ticket=True) for i in range(0, len(x), MAX_ROWS)]


def uniform_case(V, allowed_n=None):
    """every (allowed) logit equal: the score is -log n, and a dropped or doubled term moves it by >= 1 / n"""
    vals = np.array([0.0, 3.5, -7.25, 100.0], np.float32)
    x = np.repeat(vals[:, None], V, 1)
    if allowed_n is None:
        return make_case(x, seed=V, n_steps=2)
    al = np.zeros((1, V), bool)
    al[0, np.random.default_rng(V).choice(V, allowed_n, replace=False)] = True
    x = np.where(al[0], x, np.float32(9.0))                   # the disallowed logits are larger: an unmasked sum is far off
    return make_case(x, seed=V, n_steps=2, allowed=al, nxt=np.zeros((1, V), np.int32))


def constraint_case():
    """V = 1040 (the last mask word holds 16 tokens): one state per situation, one row per state plus a forced / frozen pair"""
    V = 1040
    rng = np.random.default_rng(7)
    names = ["only_last", "last_word_only", "sparse_strides", "nothing", "all_nan_members", "every_other", "lower_half"]
    al = np.zeros((len(names), V), bool)
    al[0, V - 1] = True
    al[1, 1024:] = True
    al[2, [5, 261, 517, 700, 1039]] = True                   # most threads' strides hold no allowed token
    al[4, [40, 300, 1030]] = True
    al[5, ::2] = True
    al[6, :520] = True
    x = rng.uniform(-2, 2, (len(names), V)).astype(np.float32)
    x[1, 3] = 9.0                                             # the row maximum is not allowed
    x[2, 6] = 9.0
    x[2, [5, 261, 517, 700, 1039]] = [1.0, 1.0, -1.0, 1.0, 0.5]      # a tie among the allowed: 5 wins
    x[4, [40, 300, 1030]] = np.nan
    x[5, 1] = 9.0
    x[5, [1038, 2]] = 3.0
    x[6, 900] = 9.0
    nxt = rng.integers(0, len(names), (len(names), V)).astype(np.int32)
    return make_case(x, seed=7, n_steps=2, allowed=al, nxt=nxt, state=np.arange(len(names)), want_logits=True), names


def modes_case(step, forced, eos_id, row0, want_logits, want_scores, constrained=False):
    """a lock-step launch of 6 rows at emitted column step - 2 (two prompt positions): live rows, a row that emits EOS now, rows finished
    before, with caller ids outside [0, V)"""
    V, R, ns, P = 272, 6, 3, 2
    rng = np.random.default_rng(step * 8 + row0)
    x = rng.uniform(-2, 2, (R, V)).astype(np.float32)
    eos = 7
    x[1, eos] = 5.0                                           # emits id 7: EOS when eos_id == 7
    x[4, eos] = 5.0
    fin = [0, 0, 1, 1, 0, 0]
    f = None
    if forced:
        f = rng.integers(0, V, (R, ns))
        f[0, :] = -5
        f[3, :] = V + 100
        f[5, :] = 2 ** 31 - 1
    prompt = np.array([[3, -9], [V, 5], [0, 1], [2 ** 30, 2], [4, 4], [-1, V - 1]])
    kw = {}
    if constrained:
        al = rng.random((3, V)) < 0.5
        al[:, eos] = True
        al[:, 0] = True
        kw = dict(allowed=al, nxt=rng.integers(0, 3, (3, V)), state=[0, 1, 2, 0, 1, 2])
    return make_case(x, row0=row0, seed=step, eos_id=eos_id, pad_id=0, n_steps=ns, n_prompt=P, step=step, finished=fin, forced=f, prompt=prompt,
                     want_logits=want_logits, want_scores=want_scores, chan=3, **kw)


def ticket_case(R, eos_id=9):
    """R rows with EOS accounting: finished rows in the first and the last group of 32, one row finishing now"""
    V = 48
    rng = np.random.default_rng(R)
    x = rng.uniform(-2, 2, (R, V)).astype(np.float32)
    fin = np.zeros(R, np.int32)
    fin[[0, R - 1]] = 1
    if R > 2:
        fin[R // 2] = 1
        x[1, 9] = 6.0                                         # finishes in this launch
    return make_case(x, seed=R, eos_id=eos_id, pad_id=1, n_steps=2, step=1, finished=fin, ticket=True, zero_lines=5)


def slot_case(qkv0=False, L=8):
    """slot mode, 8 rows at their own positions: prompt positions, emitted positions, EOS now, the n_steps-th token now, stopped rows"""
    V, ns, P = 272, 4, 2
    rng = np.random.default_rng(31 + qkv0)
    x = rng.uniform(-2, 2, (8, V)).astype(np.float32)
    eos = 11
    x[3, eos] = 6.0
    pos = [0, 1, 2, 3, P + ns - 1, 4, 2, 5]                   # row 4: its last token; row 6, 7: stopped
    fin = [0, 0, 0, 0, 0, 0, 1, 1]
    if qkv0:
        ns = L - P + 1                                        # one position more than the cache holds, so that a live row can reach pos == L
        pos[4], pos[5] = L - 1, L - 2                         # row 4 moves on to L (the q third only), row 5 to L - 1; row 0 to 1
    row_out = [5 * ns, 0, 3 * ns, 1 * ns, 6 * ns, 2 * ns, 4 * ns, 7 * ns]
    prompt = np.array([V + 3, 2, -1, 5, 6, 7, 8, 9, 1, 1, 2, 2, 3, 3, 4, 4], np.int32)
    row_prompt = [0, 2, 4, 6, 8, 10, 12, 14]
    al = rng.random((2, V)) < 0.6
    al[:, eos] = True
    return make_case(x, seed=31, eos_id=eos, pad_id=2, n_steps=ns, n_prompt=P, finished=fin, prompt=prompt, allowed=al,
                     nxt=rng.integers(0, 2, (2, V)), state=[0, 1, 0, 1, 0, 1, 0, 1], row_pos=pos, row_out=row_out, row_prompt=row_prompt,
                     n_out=8 * ns + 3, qkv0=qkv0, L=L if qkv0 else 0)


def gather_case(pos, L=6):
    """lock-step table gather at cache position pos = step + 1 (pos == L: the q third only)"""
    V = 48
    x = np.random.default_rng(pos).uniform(-2, 2, (3, V)).astype(np.float32)
    return make_case(x, row0=2, seed=pos, n_steps=L, step=pos - 1, qkv0=True, L=L)


def greedy_cases():
    """name -> (case, the mutants it must reject)"""
    out = {}
    for V in PLACE_V:
        for i, c in enumerate(placement_cases(V)):
            out[f"place_V{V}_{i}"] = (c, ["tie_high", "nan_wins"] + (["skip_partial_stride"] if V % 256 else []))
    for V in (16, 272, 1040, 1536):
        out[f"uniform_V{V}"] = (uniform_case(V), ["dropped_term"])
    out["uniform_allowed_V1040"] = (uniform_case(1040, 37), ["dropped_term", "lse_unmasked"])
    c, _ = constraint_case()
    out["constraints_V1040"] = (c, ["mask_word_off_by_one", "scan_start_zero", "lse_unmasked"])
    for step in (0, 1, 2, 4):
        for forced in (False, True):
            for eos_id in (-1, 7):
                row0 = 5 if (step + forced + (eos_id >= 0)) % 2 else 0
                kills = []
                if step >= 2 and eos_id >= 0 and not forced:
                    kills.append("no_pad_after_eos")
                if step >= 2 and forced:
                    kills.append("forced_unclamped")
                out[f"modes_step{step}_forced{int(forced)}_eos{eos_id}"] = (modes_case(step, forced, eos_id, row0, forced, not forced or step == 2), kills)
    out["modes_constrained_after_eos"] = (modes_case(3, True, 7, 5, False, True, constrained=True), ["automaton_not_frozen"])
    out["modes_constrained_free"] = (modes_case(2, False, 7, 0, True, True, constrained=True), ["lse_unmasked"])
    for R in (1, 64, 65, 96, 97):
        out[f"ticket_R{R}"] = (ticket_case(R), ["last_group_32"] if R in (65, 97) else [])
    out["ticket_R97_no_eos"] = (ticket_case(97, eos_id=-1), ["last_group_32"])
    out["slot_rows"] = (slot_case(), ["lse_unmasked"])
    out["slot_rows_gather"] = (slot_case(qkv0=True), ["kv_at_L"])
    for pos in (1, 5, 6):
        out[f"gather_pos{pos}"] = (gather_case(pos), ["kv_at_L"] if pos == 6 else [])
    return out


# ----------------------------------------------------------------------------- beam select: the first emitted step
MARGIN = 2e-4                      # tests/test_beam.py: a comparison the reference decides by less is undecided


def beam_step0_case(G, W, V, seed=0):
    """logits (G * W, V) for the first emitted step: the logits of every group's beam 0 are a permutation of a 0.01 grid (every comparison among
    its candidates has a margin of 0.01 in log-probability), the other beams' rows are random and 1e9 below.  -> (logits, run (G, W) float64,
    acc (G, W, V) float64)"""
    rng = np.random.default_rng(500 + seed + W * 7 + V)
    x = rng.uniform(-2, 2, (G * W, V)).astype(np.float32)
    for g in range(G):
        x[g * W] = (rng.permutation(V) * 0.01).astype(np.float32)
    run = np.full((G, W), -1.0e9)
    run[:, 0] = 0.0
    v = x.astype(np.float64).reshape(G, W, V)
    lp = v - v.max(-1, keepdims=True) - np.log(np.exp(v - v.max(-1, keepdims=True)).sum(-1, keepdims=True))
    return x, run, run[:, :, None] + lp


def undecided(acc, W):
    """deciding comparisons of one group's select that the reference decides by less than MARGIN without an exact tie: the gaps between
    neighbours among its 2W + 1 best candidates"""
    top = np.sort(acc.reshape(-1))[::-1][:2 * W + 1]
    gaps = -np.diff(top)
    return int(((gaps < MARGIN) & (gaps != 0)).sum())


# ----------------------------------------------------------------------------- beam select: one step on a given state
BEAM_MUTANTS = ("beam_tie_high", "anc_at_t", "snapshot_not_reused", "hit_outside_w_enters", "beam_lse_unmasked")
NEG = -1.0e9


def beam_acc(run, logits, allowed=None, mut=()):
    """(W,) runs and (W, V) logits of one group -> (lp, acc) float64 (W, V) as beam_oracle.host_select takes acc: -inf = no candidate (a NaN logit
    of a live row, a token the beam's state does not allow), NaN = ranks at -1e9 (a row with a NaN in its sum, or without a comparable logit)"""
    W, V = logits.shape
    lp = np.full((W, V), np.nan)
    acc = np.full((W, V), -np.inf)
    for w in range(W):
        al = np.ones(V, bool) if allowed is None else allowed[w]
        v = logits[w].astype(np.float64)
        comp = al & ~np.isnan(v) & (v > np.float64(np.float32(-3.4e38)))
        if not comp.any():                                 # a dead row: every allowed token at -1e9 with NaN scores
            acc[w, al] = np.nan
            continue
        mx = v[comp].max()
        members = v if "beam_lse_unmasked" in mut else v[al]
        lse = np.log(np.exp(members - mx).sum()) if not np.isnan(members).any() else np.nan
        lp[w] = v - mx - lse
        a = np.float64(run[w]) + lp[w]
        cand = al & ~np.isnan(v) & ~(a == -np.inf)
        acc[w, cand] = a[cand]
    return lp, acc


def beam_step_ref(s, logits, p, mut=()):
    """the state after one lock-step select, from the state before it (`s`: numpy copies of the device buffers; float64 where a bound applies).
    p: G, W, V, ns, P, eos, pad, alpha, allowed (S, V) / next or None, prompt (G, P) or None, embed, chan, n_channels.  -> (state, events)"""
    from beam_oracle import host_select
    G, W, V = p.G, p.W, p.V
    slot = getattr(s, "row_pos", None) is not None          # slot mode: every group at its own position, a flagged group stopped
    o = SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(s).items()})
    for k in ("run", "fed_lp", "fin_score", "fin_lp"):
        setattr(o, k, getattr(o, k).astype(np.float64))
    ev = dict(undecided=0, hit_in_w=0, hit_outside_w=0, displaced=0, store_reused=0, filled=0, done_idle=0, tie_across=0, dead=0, at_limit=0)
    o.entered = []                                         # (group, snapshot row, parent, token) of every hypothesis that entered a slot
    feed = np.full(G * W, p.pad, np.int64)
    parent = np.tile(np.arange(W), G)
    pos = np.zeros(G, np.int64)
    moved = np.zeros(G, bool)                               # groups whose ancestry rows the step writes (all but the stopped ones)
    for g in range(G):
        rb = g * W
        rows = slice(rb, rb + W)
        t = pos[g] = int(s.row_pos[rb]) if slot else int(s.step)
        col = t - p.P
        cur = s.anc[t & 1]
        if slot and s.finished[rb]:
            continue
        moved[g] = True
        if col < 0:
            feed[rows] = clamp(p.prompt.reshape(-1)[int(s.row_prompt[rb]) + t] if slot else p.prompt[g, t], V)
        elif s.n_fin[g] >= W:
            ev["done_idle"] += 1
        else:
            al = None if p.allowed is None else p.allowed[s.row_state[rows]]
            lp, acc = beam_acc(s.run[rows], logits[rows], al, mut)
            ev["dead"] += int(np.isnan(acc).any())
            fin = [dict(score=float(s.fin_score[rb + i]), len=int(s.fin_len[rb + i]), store=int(s.fin_store[rb + i]), tok=int(s.fin_tok[rb + i]),
                        lp=float(s.fin_lp[rb + i])) for i in range(int(s.n_fin[g]))]
            at_limit = col + 1 >= p.ns
            ev["at_limit"] += int(at_limit)
            acc_sel = acc + np.arange(W * V).reshape(W, V) * 1e-12 if "beam_tie_high" in mut else acc      # equal scores to the HIGHER flat index
            sel = host_select(acc_sel, W, p.eos, at_limit, fin, col + 1, p.alpha)
            cand = sel["cand"]
            top = np.sort(np.where(np.isnan(acc), NEG, acc).reshape(-1))[::-1][:2 * W + 1]
            top = top[top > -np.inf]
            gaps = -np.diff(top)
            ev["undecided"] += int(((gaps < MARGIN) & (gaps != 0)).sum())
            flat = [f for f, a in cand if a > -np.inf]
            keys = [a for f, a in cand if a > -np.inf]
            ev["tie_across"] += int(any(keys[i] == keys[i + 1] and flat[i] // V != flat[i + 1] // V for i in range(len(keys) - 1)))
            ev["filled"] += int(len(flat) < 2 * W)
            if not at_limit:
                ev["hit_in_w"] += int(any(sel["hit"][:W]))
                ev["hit_outside_w"] += int(any(sel["hit"][W:]))
            if "hit_outside_w_enters" in mut and s.n_fin[g] < W:
                items = [dict(x) for x in fin] + [dict(score=a / float(col + 1) ** p.alpha, parent=f // V, token=f % V, acc=a, new=c)
                                                   for c, (f, a) in enumerate(cand) if sel["hit"][c]]
                key = [NEG if np.isnan(x["score"]) else x["score"] for x in items]
                sel["fin"] = [items[i] for i in sorted(range(len(items)), key=lambda i: (-key[i], i))[:W]]
            for i, (pw, tok, r) in enumerate(sel["beams"]):
                fill = r == -np.inf                             # (a real candidate's score is never -inf)
                o.run[rb + i] = r
                o.fed_tok[rb + i, t + 1] = tok
                o.fed_lp[rb + i, t + 1] = -np.inf if fill else lp[pw, tok]
                if p.allowed is not None:
                    o.row_state[rb + i] = p.next[s.row_state[rb + pw], tok]
                feed[rb + i], parent[rb + i] = tok, pw
            new = sel["fin"]
            sc = [x["score"] for x in new if "new" not in x]
            if s.n_fin[g] < W:                             # slot order: every comparison that involves an entering score (old against old is exact)
                old = [NEG if np.isnan(x["score"]) else x["score"] for x in fin]
                ent = [NEG if np.isnan(a) else a / float(col + 1) ** p.alpha for c, (f, a) in enumerate(cand[:W]) if sel["hit"][c]]
                for i, e in enumerate(ent):
                    d = np.abs(np.array(old + ent[:i] + ent[i + 1:], np.float64) - e) if np.isfinite(e) else np.zeros(0)
                    ev["undecided"] += int(((d < MARGIN) & (d != 0)).sum())
            ev["displaced"] += int(len(sc) < len(fin))
            used = {x["store"] for x in (fin if "snapshot_not_reused" in mut else new) if "new" not in x}
            freed = {x["store"] for x in fin} - {x["store"] for x in new if "new" not in x}
            for i, x in enumerate(new):
                if "new" in x:
                    st = 0
                    while st < W - 1 and st in used:
                        st += 1
                    used.add(st)
                    ev["store_reused"] += int(st in freed)
                    x.update(len=col + 1, store=st, tok=x["token"], lp=-np.inf if x["acc"] == -np.inf else lp[x["parent"], x["token"]])
                    o.entered.append((g, st, x["parent"], x["token"]))
                    nw = t >> 2
                    o.slot_anc[rb + st, :4 * nw + 4] = cur[rb + x["parent"], :4 * nw + 4]
                o.fin_score[rb + i], o.fin_len[rb + i], o.fin_store[rb + i], o.fin_tok[rb + i], o.fin_lp[rb + i] = x["score"], x["len"], x["store"], x["tok"], x["lp"]
            o.n_fin[g] = len(new)
            if len(new) >= W:
                o.finished[rows] = 1
    for r in range(G * W):
        g, t = r // W, int(pos[r // W])
        if not moved[g]:
            continue
        nw = ((t + 1) >> 2) + 1
        o.anc[(t + 1) & 1, r, :4 * nw] = s.anc[t & 1, r - r % W + parent[r], :4 * nw]
        o.anc[(t + 1) & 1, r, t if "anc_at_t" in mut else t + 1] = r % W
        if slot and o.n_fin[g] < W:                        # a group the step made done stays where it is
            o.row_pos[r] = t + 1
    o.feed, o.parent = feed, parent
    o.h, o.ssq0 = embed_ref(p.embed, p.chan, feed, np.arange(G * W) // W, p.n_channels)
    if slot:                                               # the block's loop state is not touched in slot mode
        o.state_out = s.state_out.copy()
    else:
        o.step = int(s.step) + 1
        o.state_out = np.array([o.step, 0, W * int((o.n_fin < W).sum()), p.ns], np.int32)
    return o, ev


def beam_init_state(p, start=None):
    """the state beam_init leaves (buffers it does not write hold SENT, ancestry bytes 0xAB)"""
    R = p.G * p.W
    s = SimpleNamespace(step=0, run=np.where(np.arange(R) % p.W == 0, 0.0, NEG).astype(np.float32), finished=np.zeros(R, np.int32),
                        fin_score=np.full(R, NEG, np.float32), fin_len=np.zeros(R, np.int32), fin_store=(np.arange(R) % p.W).astype(np.int32),
                        fin_tok=np.full(R, p.pad, np.int32), fin_lp=np.zeros(R, np.float32), n_fin=np.zeros(p.G, np.int32),
                        fed_tok=np.full((R, p.fed), np.int32(SENT)), fed_lp=np.full((R, p.fed), np.float32(SENT)),
                        anc=np.full((2, R, p.pitch), 0xAB, np.uint8), slot_anc=np.full((R, p.pitch), 0xAB, np.uint8),
                        row_state=None if p.allowed is None else np.repeat(np.clip(np.zeros(p.G, np.int64) if start is None else start, 0, len(p.allowed) - 1), p.W).astype(np.int32))
    s.anc[0, :, 0] = np.arange(R) % p.W
    return s


BEAM_INT = ("finished", "fin_len", "fin_store", "fin_tok", "n_fin", "fed_tok", "anc", "slot_anc", "row_state", "state_out", "row_pos", "row_out", "row_prompt")
BEAM_F = ("run", "fed_lp", "fin_score", "fin_lp")


def beam_compare(ref, got):
    """-> (names that differ, worst score error over its bound).  Slots at or beyond n_fin are not looked at beyond being untouched by the caller."""
    bad, worst = [], 0.0
    for k in BEAM_INT:
        a, b = getattr(ref, k, None), getattr(got, k, None)
        if a is not None and not np.array_equal(a, b):
            bad.append(k)
    for k in BEAM_F:
        ok, w = compare_scores(getattr(ref, k), getattr(got, k))
        worst = max(worst, w if ok else 0.0)
        if not ok:
            bad.append(k)
    if hasattr(got, "h") and not np.array_equal(ref.h.view(np.uint32), np.asarray(got.h, np.float32).reshape(ref.h.shape).view(np.uint32)):
        bad.append("h")
    return bad, worst


def beam_params(G, W, V, ns, *, eos=-1, pad=1, alpha=1.0, P=0, prompt=None, allowed=None, nxt=None, seed=0, chan=0):
    rng = np.random.default_rng(4000 + seed)
    return SimpleNamespace(G=G, W=W, V=V, ns=ns, P=P, eos=eos, pad=pad, alpha=alpha, prompt=prompt, allowed=allowed, next=nxt, pitch=16, fed=ns + P + 2,
                           embed=bf16_bits(rng.integers(-64, 65, (V, D)) / 32.0), chan=bf16_bits(rng.integers(-64, 65, (chan, D)) / 64.0) if chan else None,
                           n_channels=max(chan, 1))


def _grid_rows(rng, n, V, W, eos=-1, p_eos=0.0):
    """n rows, each a permutation of an exact 2^-4 (2^-6 beyond V = 272) grid whose lowest entry is moved off the grid, to 0.1 .. 0.7 of the top term (so that the rows' log-sum-exps, and with them the
    phases of the beams' score lattices, differ); EOS swapped into one of the top 2W + 2 ranks with probability p_eos"""
    x = np.stack([rng.permutation(V) for _ in range(n)]).astype(np.float32) * np.float32(2.0 ** -4 if V <= 272 else 2.0 ** -6)
    for r in range(n):
        x[r, np.argmin(x[r])] = x[r].max() + np.float32(np.log(rng.uniform(0.1, 0.7)))     # 0.1 .. 0.7 of the top term: log-sum-exp moves by up to a grid step or more
        if eos >= 0 and rng.random() < p_eos:
            k = np.argsort(-x[r])[rng.integers(0, min(V, 2 * W + 2))]
            x[r, eos], x[r, k] = x[r, k], x[r, eos]
    return x


def _build(p, n_pos, seed, p_eos=0.0, tweak=None):
    """logits per position, drawn again until the reference decides every comparison of the position by MARGIN or by an exact tie"""
    rng = np.random.default_rng(7000 + seed)
    s, steps = beam_init_state(p), []
    for t in range(n_pos):
        for _ in range(400):
            x = _grid_rows(rng, p.G * p.W, p.V, p.W, p.eos, p_eos)
            if tweak:
                x = tweak(t, x)
            o, ev = beam_step_ref(s, x, p)
            if ev["undecided"] == 0:
                break
        else:
            raise RuntimeError("no decided draw")
        steps.append(x)
        s = _as_device(o)
    return steps


def _as_device(o):
    s = SimpleNamespace(**vars(o))
    for k in BEAM_F:
        setattr(s, k, getattr(o, k).astype(np.float32))
    return s


_SEQ = {}


def beam_sequences():
    """name -> (params, logits per position [(G * W, V)], finalize N, the events the sequence must show, the mutants it must reject)"""
    if _SEQ:
        return _SEQ
    for name, (W, V, ns, eos, alpha, N, seed, p_eos, want) in {
        "W2_V16_eos": (2, 16, 4, 3, 2.0, 1, 3, 0.3, ("hit_in_w", "at_limit")),
        "W4_V272_eos_displace": (4, 272, 7, 5, 1.0, 2, 1, 0.45, ("hit_in_w", "hit_outside_w", "displaced", "store_reused")),
        "W8_V1536_eos": (8, 1536, 6, 7, 0.0, 8, 2, 0.3, ("hit_in_w", "hit_outside_w")),
        "W1_V272": (1, 272, 6, 5, 1.0, 1, 4, 0.1, ("at_limit",)),
        "W4_V16_no_eos": (4, 16, 6, -1, 1.0, 3, 5, 0.0, ("at_limit",)),
    }.items():
        p = beam_params(2, W, V, ns, eos=eos, alpha=alpha, seed=seed)
        kills = ["anc_at_t"] + (["snapshot_not_reused"] if "store_reused" in want else []) + (["hit_outside_w_enters"] if "hit_outside_w" in want else [])
        _SEQ[name] = (p, _build(p, ns, seed, p_eos), N, want, kills)
    # exact ties across beams: two tokens tied at the top of beam 0 at step 0 give beams 0 and 1 the same run; at step 1 their rows are bit-identical
    p = beam_params(1, 2, 48, 4, seed=11)

    def ties(t, x):
        if t == 0:
            x[0, [9, 30]] = np.float32(1.0)
        if t == 1:
            x[1] = x[0]
        return x
    _SEQ["W2_V48_ties_across_beams"] = (p, _build(p, 4, 11, tweak=ties), 2, ("tie_across",), ["anc_at_t", "beam_tie_high"])
    # a prompt, an automaton that runs the group out of candidates (state 1 allows one token, state 2 nothing)
    V, W = 16, 4
    al = np.ones((3, V), bool)
    al[1] = False
    al[1, 6] = True
    al[2] = False
    nxt = np.zeros((3, V), np.int32)
    nxt[0, :] = 1                                            # after the first token every beam allows one token: 4 candidates < 2W
    nxt[1, :] = 2                                            # then nothing: 0 candidates < W, every place is flat index 0 at -inf
    p = beam_params(2, W, V, 5, P=2, prompt=np.array([[3, V + 4], [-2, 5]]), allowed=al, nxt=nxt, seed=12, chan=2)
    _SEQ["W4_V16_prompt_exhausted"] = (p, _build(p, 7, 12, tweak=lambda t, x: np.where(al[1], x, np.float32(9.0)) if t == 3 else x), 1, ("filled",),
                                       ["anc_at_t", "beam_lse_unmasked"])
    p = beam_params(1, 2, 48, 4, seed=13)

    def dead(t, x):
        if t == 1:
            x[1, 5] = np.nan                                 # beam 1's row holds a NaN: its candidates stand at -1e9
        if t == 2:
            x[0, :] = np.nan                                 # no comparable logit in beam 0's row
        return x
    _SEQ["W2_V48_dead_rows"] = (p, _build(p, 4, 13, tweak=dead), 2, ("dead",), ["anc_at_t"])
    return _SEQ


def beam_simulate(p, steps, mut=()):
    """the whole sequence under the reference alone -> (states after every position, summed events, the hypotheses' token lists per slot)"""
    s = beam_init_state(p)
    states, total = [], {}
    for x in steps:
        o, ev = beam_step_ref(s, x, p, mut)
        for k, v in ev.items():
            total[k] = total.get(k, 0) + v
        states.append(o)
        s = _as_device(o)
    return states, total


def beam_slot_start_ref(s, p, row0, first_group):
    """the state after beam_slot_start over the n_channels * W rows from row0 (queue indices first_group + channel); the rest untouched"""
    o = SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(s).items()})
    W = p.W
    for r in range(row0, row0 + p.n_channels * W):
        w, ch = r % W, (r - row0) // W
        o.finished[r], o.run[r], o.fin_score[r], o.fin_len[r], o.fin_store[r], o.fin_tok[r], o.fin_lp[r] = 0, 0.0 if w == 0 else NEG, NEG, 0, w, p.pad, 0.0
        o.n_fin[r // W] = 0
        o.anc[0, r, 0] = w
        o.row_pos[r], o.row_out[r], o.row_prompt[r] = 0, first_group + ch, (first_group + ch) * p.P
    return o


def beam_slot_case():
    """slot mode: three slots of one group each (W = 2, one prompt position, 3 emitted tokens) started one launch apart, so the groups stand at
    different positions in every launch and the earlier ones are done (stopped) while the last still runs; empty slots are flagged stopped.
    -> (params, n_queue, actions): ("start", row0, first_group) or ("step", logits), drawn until the reference decides every comparison"""
    if "slot" in _SEQ_SLOT:
        return _SEQ_SLOT["slot"]
    G, W, V, ns, P, n_queue = 3, 2, 48, 3, 1, 6
    p = beam_params(G, W, V, ns, eos=4, pad=1, alpha=1.0, P=P, prompt=np.array([[k % V] for k in (7, V + 1, 9, 3, -4, 11)]), seed=21)
    rng = np.random.default_rng(7400)
    s = beam_slot_empty_state(p)
    actions = []
    queue = [(0, 5), (2, 0), (4, 3)]
    for launch in range(P + ns + len(queue) - 1):
        if launch < len(queue):
            actions.append(("start",) + queue[launch])
            s = beam_slot_start_ref(s, p, *queue[launch])
        for _ in range(400):
            x = _grid_rows(rng, G * W, V, W, p.eos, 0.25)
            o, ev = beam_step_ref(s, x, p)
            if ev["undecided"] == 0:
                break
        else:
            raise RuntimeError("no decided draw")
        actions.append(("step", x))
        s = _as_device(o)
    _SEQ_SLOT["slot"] = (p, n_queue, actions)
    return _SEQ_SLOT["slot"]


_SEQ_SLOT = {}


def beam_slot_empty_state(p):
    """before any slot is started: every row flagged stopped, everything else unwritten (SENT; ancestry 0xAB)"""
    R = p.G * p.W
    i32, f32 = lambda: np.full(R, np.int32(SENT)), lambda: np.full(R, np.float32(SENT))
    return SimpleNamespace(step=0, run=f32(), finished=np.ones(R, np.int32), fin_score=f32(), fin_len=i32(), fin_store=i32(), fin_tok=i32(), fin_lp=f32(),
                           n_fin=np.full(p.G, np.int32(SENT)), fed_tok=np.full((R, p.fed), np.int32(SENT)), fed_lp=np.full((R, p.fed), np.float32(SENT)),
                           anc=np.full((2, R, p.pitch), 0xAB, np.uint8), slot_anc=np.full((R, p.pitch), 0xAB, np.uint8), row_state=None,
                           row_pos=i32(), row_out=np.full(R, np.int64(SENT)), row_prompt=np.full(R, np.int64(SENT)),
                           state_out=np.array([0, 0, R, p.ns], np.int32))
