// Beam search on the device (include/ymt3.h, beam search): the selection kernel that takes argmax_embed_kernel's place in a beam
// call's step, its init and its result kernels, and their per-slot forms for continuous batching (ymt3_transcribe_stream_beam: slot mode
// of the selection kernel, beam_slot_start_kernel, the result kernel over one slot's groups).  The ancestry-addressed self-attention lives
// with the other attention kernels (decode.hip: attn_body<..., BEAM>).
//
// Rows: r = (segment * n_channels + channel) * W + beam; group g = r / W.  One workgroup per group:
//   1. per running beam the row maximum and log-sum-exp of its logits exactly as argmax_embed_kernel's score pass takes them (same
//      __expf, same per-thread / wave / 4-wave summation order, masked by the beam's automaton state), so lp = (v - max) - log(sum)
//      is the number scores_dev holds in a greedy call;
//   2. the 2W largest run[w] + lp[w][v] over the group's W * V candidates, descending, ties towards the lower flat index w * V + v:
//      every thread owns the candidates v = tid (mod 256) of all beams and offers the best one it has not given yet; a round is one
//      (value, lowest index) reduction over the workgroup, and only the round's winner looks for its next candidate;
//   3. HF `_beam_search` steps 3-7 (early_stopping = True) by thread 0: EOS / length-limit hits, the next W running beams, the
//      finished slots (merge, best W, stable), done;
//   4. all threads: the new beams' ancestry rows (parent's row + own index at the next position, into the other buffer), ancestry
//      snapshots of the hypotheses that entered a slot, the W fed tokens' embeddings, the step advance by the last workgroup.
// NaN logits are no candidates; a candidate whose score is NaN (a beam whose row has a NaN in its sum) ranks at -1e9 and keeps its NaN as
// value; a row without any comparable logit (all NaN, all -inf) offers every allowed token at -1e9 with NaN scores, lowest index first; when a group runs out of candidates (an automaton state that allows fewer than 2W / W tokens) the remaining
// places go to flat index 0 at -inf.  Every index written or followed is clamped.
#include "common.h"
#include "kernels.h"

namespace {

constexpr float BEAM_NEG = -1.0e9f;
constexpr int NO_INDEX = 0x7fffffff;

// embed_row of decode.hip (same sums in the same order: a beam call with W = 1 leaves the bits a greedy call leaves)
__device__ __forceinline__ void beam_embed_row(const BeamArgs& a, int r, const bf16_t* e, const bf16_t* c, float* scratch4) {
    const int tid = threadIdx.x;
    float q = 0.f;
    for (int i = tid; i < a.d; i += 256) {
        const float v = bf2f(e[i]) + (c ? bf2f(c[i]) : 0.f);
        a.h[(size_t)r * a.d + i] = v;
        q += v * v;
    }
    q = wave_sum(q);
    __syncthreads();
    if ((tid & 63) == 0) scratch4[tid >> 6] = q;
    __syncthreads();
    if (tid < SSQ_TILES) a.ssq[(size_t)tid * a.ssq_stride + r] = tid == 0 ? (scratch4[0] + scratch4[1]) + (scratch4[2] + scratch4[3]) : 0.f;
}

// (ka, ia) ranks before (kb, ib): larger value, then lower index
__device__ __forceinline__ bool ranks_before(float ka, int ia, float kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// SLOT (continuous batching, ymt3_transcribe_stream_beam): every group decodes at its own position a.row_pos[rb] (its W rows share it),
// reads its prompt through a.row_prompt and records its trace under its queue index a.row_out[rb].  A stopped group (finished flag set:
// done, or an empty slot) keeps its state and its position and only feeds PAD; a live one advances the positions of its own rows unless
// the step made it done, and the workgroups do not meet at the end.  Steps 1-4 are the same instructions on the same values: a group's results depend on no other slot.
template <bool SLOT>
__global__ __launch_bounds__(256) void beam_select_kernel(BeamArgs a) {
    __shared__ float sv[4], s_sum[4];
    __shared__ int si[4];
    __shared__ float s_max[BEAM_MAX], s_lse[BEAM_MAX], s_run[BEAM_MAX];
    __shared__ int s_state[BEAM_MAX];
    __shared__ float c_acc[2 * BEAM_MAX], c_lp[2 * BEAM_MAX];
    __shared__ int c_idx[2 * BEAM_MAX];
    __shared__ int s_parent[BEAM_MAX], s_feed[BEAM_MAX];
    __shared__ int s_snap_store[BEAM_MAX], s_snap_parent[BEAM_MAX], s_n_snap, s_done;
    // thread 0's work arrays of step 3 (in LDS: they are indexed at run time, and as private arrays they lived in scratch memory, a memory
    // round trip per access on a serial path)
    __shared__ bool hit[2 * BEAM_MAX], used[2 * BEAM_MAX], taken[2 * BEAM_MAX];
    __shared__ float kmod[2 * BEAM_MAX], m_score[2 * BEAM_MAX], m_key[2 * BEAM_MAX], n_score[BEAM_MAX], n_lp[BEAM_MAX];
    __shared__ int cw[2 * BEAM_MAX], ctok[2 * BEAM_MAX], m_src[2 * BEAM_MAX], order[BEAM_MAX], n_len[BEAM_MAX], n_store[BEAM_MAX], n_tok[BEAM_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.W, V = a.V, g = blockIdx.x, rb = g * W;
    DecodeShared* sh = a.shared;
    const BeamShared* bs = a.beam;
    const bool stopped = SLOT && a.finished[rb] != 0;
    const int step0 = SLOT ? 0 : sh->step0, tg = SLOT ? (int)a.row_out[rb] : g;      // tg: the group's index in the debug trace
    const int t = SLOT ? min(max(a.row_pos[rb], 0), min(a.fed_pitch, a.anc_pitch) - 2) : sh->step, n_steps = sh->n_steps, n_prompt = sh->n_prompt, col = t - step0 - n_prompt;
    const uint32_t* const c_allowed = sh->c_allowed;
    const int c_words = sh->c_words;
    const int n_fin0 = a.n_fin[g];
    const bool live = !stopped && col >= 0 && n_fin0 < W;         // an emitted step of a group that is not done: the search moves
    if (a.stamp && tid == 0) a.stamp[2 * blockIdx.x] = wall_clock64();
    if (tid < W) {
        s_run[tid] = a.run[rb + tid];
        s_state[tid] = c_allowed ? a.row_state[rb + tid] : 0;
        s_parent[tid] = tid;
        s_feed[tid] = a.pad_id;
    }
    if (tid == 0) { s_n_snap = 0; s_done = 0; }
    __syncthreads();

    if (stopped) {
        // slot mode, a done group or an empty slot: PAD is fed, nothing else moves
    } else if (col < 0) {
        // a prompt position: all W rows of the group are fed the group's prompt id; no token, no beam state
        if (tid < W) {
            const int p = sh->prompt[(SLOT ? (size_t)a.row_prompt[rb] : (size_t)g * n_prompt) + (t - step0)];
            s_feed[tid] = p < 0 ? 0 : (p >= V ? V - 1 : p);
        }
    } else if (live) {
        // ---- 1. row maximum and log-sum-exp of every running beam (argmax_embed_kernel's score pass)
        for (int w = 0; w < W; ++w) {
            const float* row = a.logits + (size_t)(rb + w) * V;
            const uint32_t* mrow = c_allowed ? c_allowed + (size_t)s_state[w] * c_words : nullptr;
            float bv = -3.4e38f;
            for (int i = tid; i < V; i += 256) {
                const float v = row[i];
                if ((!mrow || ((mrow[i >> 5] >> (i & 31)) & 1u)) && v > bv) bv = v;
            }
            bv = wave_max(bv);
            if (lane == 0) sv[wave] = bv;
            __syncthreads();
            const float row_max = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
            float q = 0.f;
            if (mrow) {
                for (int i = tid; i < V; i += 256)
                    if ((mrow[i >> 5] >> (i & 31)) & 1u) q += __expf(row[i] - row_max);
            } else {
                for (int i = tid; i < V; i += 256) q += __expf(row[i] - row_max);
            }
            q = wave_sum(q);
            if (lane == 0) s_sum[wave] = q;
            __syncthreads();
            if (tid == 0) {
                s_max[w] = row_max;
                s_lse[w] = __logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
            }
            __syncthreads();
        }
        // ---- 2. the 2W best candidates, one per round
        // A thread's candidates are ranked by `key` (the score, -1e9 for a NaN one); NaN marks "no candidate": a NaN logit, a disallowed
        // token, or a score of -inf (a -inf logit in a row with a finite maximum), so that a group that runs out of candidates fills the
        // remaining places with flat index 0 at -inf, as the header says.  The winner of a round rescans its W * V / 256 candidates from
        // the logits (in cache by then).  (A copy of the keys in dynamic LDS, W * V floats where they fit, was measured at 74 us per
        // step against 87 us for this form at W = 4 -- profiles/beam_step_ab.txt -- and left out: it needs this path as its fall-back for
        // large vocabularies anyway, and the kernel's time is mostly elsewhere; it belongs to the rework of this kernel.)
        float last_k = __builtin_inff();              // the candidate this thread gave last: it offers only what ranks behind it
        int last_f = -1;
        float my_k = 0.f;
        int my_f = NO_INDEX;
        auto score_at = [&](int w, int i, float& lp, float& acc) -> float {      // -> key, NaN: no candidate
            const float* row = a.logits + (size_t)(rb + w) * V;
            const uint32_t* mrow = c_allowed ? c_allowed + (size_t)s_state[w] * c_words : nullptr;
            const float mx = s_max[w];
            const bool dead = !(mx > -3.4e38f);                     // no comparable logit in the row: its candidates stand at NEG, scores NaN
            const float v = row[i];
            lp = dead ? __builtin_nanf("") : (v - mx) - s_lse[w];
            acc = s_run[w] + lp;
            if ((v != v && !dead) || (mrow && !((mrow[i >> 5] >> (i & 31)) & 1u)) || acc == -__builtin_inff()) return __builtin_nanf("");
            return acc != acc ? BEAM_NEG : acc;
        };
        auto rescan = [&]() {
            my_k = -__builtin_inff(); my_f = NO_INDEX;
            for (int w = 0; w < W; ++w) {
                for (int i = tid; i < V; i += 256) {
                    float lp, acc;
                    const float key = score_at(w, i, lp, acc);
                    if (key != key) continue;
                    const int f = w * V + i;
                    if (ranks_before(last_k, last_f, key, f) && ranks_before(key, f, my_k, my_f)) { my_k = key; my_f = f; }
                }
            }
        };
        rescan();
        for (int c = 0; c < 2 * W; ++c) {
            float bk = my_k;
            int bf = my_f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ok = __shfl_xor(bk, o, 64);
                const int of = __shfl_xor(bf, o, 64);
                if (ranks_before(ok, of, bk, bf)) { bk = ok; bf = of; }
            }
            if (lane == 0) { sv[wave] = bk; si[wave] = bf; }
            __syncthreads();
            bk = sv[0]; bf = si[0];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (ranks_before(sv[w], si[w], bk, bf)) { bk = sv[w]; bf = si[w]; }
            if (bf == NO_INDEX) {                     // nothing left in the group
                if (tid == 0) { c_acc[c] = -__builtin_inff(); c_lp[c] = -__builtin_inff(); c_idx[c] = 0; }
            } else if (bf == my_f) {                  // (flat indices are unique: exactly one thread)
                float lp, acc;
                (void)score_at(my_f / V, my_f % V, lp, acc);
                c_acc[c] = acc; c_lp[c] = lp; c_idx[c] = my_f;
                last_k = my_k; last_f = my_f;
                rescan();
            }
            __syncthreads();
        }
        // ---- 3. hits, the next running beams, the finished slots (thread 0; 2W <= 16 candidates)
        if (tid == 0) {
            const int len = col + 1;
            const bool at_limit = len >= n_steps;
            for (int c = 0; c < 2 * W; ++c) {
                const int f = min(max(c_idx[c], 0), W * V - 1);
                cw[c] = f / V; ctok[c] = f % V;
                hit[c] = at_limit || (a.eos_id >= 0 && ctok[c] == a.eos_id);
                const float key = c_acc[c] != c_acc[c] ? BEAM_NEG : c_acc[c];
                kmod[c] = hit[c] ? key + BEAM_NEG : key;
            }
            // the next running beams: the best W by the hit-penalised score, in order (first among equals)
            for (int c = 0; c < 2 * W; ++c) used[c] = false;
            int32_t* tr = bs->trace && col < bs->trace_steps && tg >= 0 && tg < bs->trace_groups ? bs->trace + ((size_t)col * bs->trace_groups + tg) * W * 2 : nullptr;
            float* trr = bs->trace_run && col < bs->trace_steps && tg >= 0 && tg < bs->trace_groups ? bs->trace_run + ((size_t)col * bs->trace_groups + tg) * W : nullptr;
            for (int i = 0; i < W; ++i) {
                int b = -1;
                for (int c = 0; c < 2 * W; ++c)
                    if (!used[c] && (b < 0 || kmod[c] > kmod[b])) b = c;
                used[b] = true;
                const float run_new = hit[b] ? c_acc[b] + BEAM_NEG : c_acc[b];
                s_parent[i] = cw[b];
                s_feed[i] = ctok[b];
                a.run[rb + i] = run_new;
                a.fed_tok[(size_t)(rb + i) * a.fed_pitch + t + 1] = ctok[b];
                a.fed_lp[(size_t)(rb + i) * a.fed_pitch + t + 1] = c_lp[b];
                if (c_allowed) a.row_state[rb + i] = sh->c_next[(size_t)s_state[cw[b]] * V + ctok[b]];
                if (tr) { tr[2 * i] = cw[b]; tr[2 * i + 1] = ctok[b]; }
                if (trr) trr[i] = run_new;
            }
            // the finished slots: old ones first, then the hit candidates among the first W, in candidate order; best W, stable
            const float lenp = powf((float)len, bs->alpha);
            int n_items = 0;                           // (m_src < W: old slot; >= W: candidate m_src - W)
            for (int i = 0; i < n_fin0; ++i) {
                m_score[n_items] = a.fin_score[rb + i];
                m_key[n_items] = m_score[n_items] != m_score[n_items] ? BEAM_NEG : m_score[n_items];
                m_src[n_items++] = i;
            }
            for (int c = 0; c < W; ++c) {
                if (!hit[c]) continue;
                m_score[n_items] = c_acc[c] / lenp;
                m_key[n_items] = m_score[n_items] != m_score[n_items] ? BEAM_NEG : m_score[n_items];
                m_src[n_items++] = W + c;
            }
            const int n_keep = min(n_items, W);
            for (int i = 0; i < n_items; ++i) taken[i] = false;
            unsigned stores_used = 0;
            for (int i = 0; i < n_keep; ++i) {
                int b = -1;
                for (int j = 0; j < n_items; ++j)
                    if (!taken[j] && (b < 0 || m_key[j] > m_key[b])) b = j;
                taken[b] = true;
                order[i] = b;
                if (m_src[b] < W) stores_used |= 1u << (a.fin_store[rb + m_src[b]] & (BEAM_MAX - 1));
            }
            // read the surviving old slots before any is overwritten
            int n_snap = 0;
            for (int i = 0; i < n_keep; ++i) {
                const int b = order[i];
                n_score[i] = m_score[b];
                if (m_src[b] < W) {
                    const int o = rb + m_src[b];
                    n_len[i] = a.fin_len[o]; n_store[i] = a.fin_store[o]; n_tok[i] = a.fin_tok[o]; n_lp[i] = a.fin_lp[o];
                } else {
                    const int c = m_src[b] - W;
                    int st = 0;
                    while (st < W - 1 && ((stores_used >> st) & 1u)) ++st;      // a free snapshot row of the group (W rows, at most W kept)
                    stores_used |= 1u << st;
                    n_len[i] = len; n_store[i] = st; n_tok[i] = ctok[c]; n_lp[i] = c_lp[c];
                    s_snap_store[n_snap] = st; s_snap_parent[n_snap] = cw[c]; ++n_snap;
                }
            }
            for (int i = 0; i < n_keep; ++i) {
                const int o = rb + i;
                a.fin_score[o] = n_score[i]; a.fin_len[o] = n_len[i]; a.fin_store[o] = n_store[i]; a.fin_tok[o] = n_tok[i]; a.fin_lp[o] = n_lp[i];
            }
            a.n_fin[g] = n_keep;
            s_n_snap = n_snap;
            if (n_keep >= W) {
                for (int i = 0; i < W; ++i) a.finished[rb + i] = 1;
                s_done = 1;
            }
        }
    } else if (!SLOT && tid < W && bs->trace && col < bs->trace_steps && g < bs->trace_groups) {
        // a done group: its rows idle on PAD, every row its own parent (slot mode: a done group is stopped and records nothing)
        int32_t* tr = bs->trace + (((size_t)col * bs->trace_groups + g) * W + tid) * 2;
        tr[0] = tid; tr[1] = a.pad_id;
        if (bs->trace_run) bs->trace_run[((size_t)col * bs->trace_groups + g) * W + tid] = s_run[tid];
    }
    __syncthreads();

    // ---- 4. ancestry rows of the next position, snapshots, embeddings
    if (!stopped) {
        const uint8_t* cur = a.anc + ((size_t)(t & 1) * a.anc_rows + rb) * a.anc_pitch;
        uint8_t* nxt = a.anc + ((size_t)((t + 1) & 1) * a.anc_rows + rb) * a.anc_pitch;
        const int last_word = (t + 1) >> 2, n_words = last_word + 1;           // positions 0 .. t + 1 (anc_pitch > max_decode_len, a multiple of 16)
        for (int i = 0; i < W; ++i) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(cur + (size_t)min(max(s_parent[i], 0), W - 1) * a.anc_pitch);
            uint32_t* dst = reinterpret_cast<uint32_t*>(nxt + (size_t)i * a.anc_pitch);
            for (int j = tid; j < n_words; j += 256) {
                uint32_t v = src[j];
                if (j == last_word) {
                    const int sh8 = ((t + 1) & 3) * 8;
                    v = (v & ~(0xffu << sh8)) | ((uint32_t)i << sh8);
                }
                dst[j] = v;
            }
        }
        const int n_snap = s_n_snap;
        for (int k = 0; k < n_snap; ++k) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(cur + (size_t)min(max(s_snap_parent[k], 0), W - 1) * a.anc_pitch);
            uint32_t* dst = reinterpret_cast<uint32_t*>(a.slot_anc + (size_t)(rb + min(max(s_snap_store[k], 0), W - 1)) * a.anc_pitch);
            for (int j = tid; j <= (t >> 2); j += 256) dst[j] = src[j];
        }
    }
    if (live && bs->trace_logits && col < bs->trace_steps && tg >= 0 && tg < bs->trace_groups) {
        float* dst = bs->trace_logits + ((size_t)col * bs->trace_groups + tg) * W * V;
        const float* src = a.logits + (size_t)rb * V;
        for (int i = tid; i < W * V; i += 256) dst[i] = src[i];
    }
    for (int i = 0; i < W; ++i) {
        const int r = rb + i;
        const int feed = min(max(s_feed[i], 0), V - 1);
        const bf16_t* e = a.embed + (size_t)feed * a.d;
        const bf16_t* c = a.chan_embed ? a.chan_embed + (size_t)(g % a.n_channels) * a.d : nullptr;
        beam_embed_row(a, r, e, c, sv);
    }
    // the last workgroup to finish advances the position; every workgroup has read `t` by then
    // (slot mode: a live group advances its own rows; nothing is shared between groups)
    __syncthreads();
    if constexpr (SLOT) {
        // (a group that has just become done stays where it is, like a greedy row after its EOS: the step that filled its slots may have
        // been the last position of its cache slabs, and the rows go on running until the host retires them)
        if (!stopped && !s_done && tid < W) a.row_pos[rb + tid] = t + 1;
    } else if (tid == 0) {
        __threadfence();
        if (atomicAdd(&sh->done_count, 1) == (int)gridDim.x - 1) {
            sh->done_count = 0;
            sh->step = t + 1;
            int n = 0;
            for (int i = 0; i < (int)gridDim.x; ++i) n += a.n_fin[i] >= W ? 0 : W;
            sh->n_unfinished = n;
        }
    }
    if (a.stamp && (tid & 63) == 0) atomicMax(a.stamp + 2 * blockIdx.x + 1, (unsigned long long)wall_clock64());
}

__global__ __launch_bounds__(256) void beam_init_kernel(BeamArgs a, int n_steps, const int32_t* prompt, int n_prompt, ConstraintView cv, BeamShared params) {
    const int r = blockIdx.x, tid = threadIdx.x, W = a.W, g = r / W, w = r % W;
    const bf16_t* e = a.embed + (size_t)a.pad_id * a.d;
    const bf16_t* c = a.chan_embed ? a.chan_embed + (size_t)(g % a.n_channels) * a.d : nullptr;
    __shared__ float sv[4];
    beam_embed_row(a, r, e, c, sv);
    if (tid == 0) {
        a.finished[r] = 0;
        a.run[r] = w == 0 ? 0.f : BEAM_NEG;            // step 0 expands beam 0 only
        a.fin_score[r] = BEAM_NEG; a.fin_len[r] = 0; a.fin_store[r] = w; a.fin_tok[r] = a.pad_id; a.fin_lp[r] = 0.f;
        if (w == 0) a.n_fin[g] = 0;
        if (a.row_state) a.row_state[r] = cv.start ? min(max(cv.start[g], 0), cv.n_states - 1) : 0;
        a.anc[(size_t)r * a.anc_pitch] = (uint8_t)w;   // buffer 0: position 0 is the row's own
    }
    if (r == 0 && tid == 0) {
        DecodeShared* sh = a.shared;
        sh->step = 0; sh->step0 = 0; sh->done_count = 0; sh->n_unfinished = a.R; sh->n_steps = n_steps;
        sh->tokens_out = nullptr; sh->forced = nullptr; sh->logits_out = nullptr; sh->scores_out = nullptr;
        sh->prompt = prompt; sh->n_prompt = n_prompt;
        sh->c_allowed = cv.allowed; sh->c_next = cv.next; sh->c_words = cv.words;
        *a.beam = params;
    }
}

// slot mode: (re)start the n_channels * W rows from row0 on the segment whose first group has queue index first_group; cv.start: that
// segment's [n_channels] start states (or null).  What beam_init_kernel does for every row of a call, for one slot, plus the slot's own
// position and indices.
__global__ __launch_bounds__(256) void beam_slot_start_kernel(BeamArgs a, int row0, long long first_group, int n_prompt, ConstraintView cv) {
    const int r = row0 + blockIdx.x, tid = threadIdx.x, W = a.W, g = r / W, w = r % W, ch = (int)(blockIdx.x / W);
    const bf16_t* e = a.embed + (size_t)a.pad_id * a.d;
    const bf16_t* c = a.chan_embed ? a.chan_embed + (size_t)(g % a.n_channels) * a.d : nullptr;
    __shared__ float sv[4];
    beam_embed_row(a, r, e, c, sv);
    if (tid == 0) {
        a.finished[r] = 0;
        a.run[r] = w == 0 ? 0.f : BEAM_NEG;
        a.fin_score[r] = BEAM_NEG; a.fin_len[r] = 0; a.fin_store[r] = w; a.fin_tok[r] = a.pad_id; a.fin_lp[r] = 0.f;
        if (w == 0) a.n_fin[g] = 0;
        if (a.row_state) a.row_state[r] = cv.start ? min(max(cv.start[ch], 0), cv.n_states - 1) : 0;
        a.anc[(size_t)r * a.anc_pitch] = (uint8_t)w;   // buffer 0: position 0 is the row's own
        a.row_pos[r] = 0;
        a.row_out[r] = first_group + ch;
        a.row_prompt[r] = (first_group + ch) * n_prompt;
    }
}

// one workgroup per returned hypothesis (group, n): its tokens up to and including the one that finished it, then PAD
// (slot mode, a.row_out set: the groups from g0 on, written at their queue index)
__global__ __launch_bounds__(256) void beam_finalize_kernel(BeamArgs a, int N, int g0) {
    const BeamShared* bs = a.beam;
    const DecodeShared* sh = a.shared;
    const int W = a.W, g = g0 + blockIdx.x / N, n = blockIdx.x % N, rb = g * W, n_steps = sh->n_steps, P = sh->n_prompt;
    const size_t out = a.row_out ? (size_t)a.row_out[rb] * N + n : (size_t)blockIdx.x;
    const bool filled = n < a.n_fin[g];
    const int o = rb + min(n, W - 1);
    const int len = filled ? min(max(a.fin_len[o], 1), n_steps) : 0;
    const uint8_t* snap = a.slot_anc + (size_t)(rb + min(max(a.fin_store[o], 0), W - 1)) * a.anc_pitch;
    int32_t* tok = bs->tokens_out + out * n_steps;
    float* ts = bs->tok_out ? bs->tok_out + out * n_steps : nullptr;
    for (int j = threadIdx.x; j < n_steps; j += 256) {
        int id = a.pad_id;
        float lp = 0.f;
        if (j == len - 1) { id = a.fin_tok[o]; lp = a.fin_lp[o]; }
        else if (j < len - 1) {
            const int p = P + j + 1;                    // emitted token j was fed at position P + j + 1 into the row that holds it
            const size_t at = (size_t)(rb + min((int)snap[p], W - 1)) * a.fed_pitch + p;
            id = a.fed_tok[at]; lp = a.fed_lp[at];
        }
        tok[j] = id;
        if (ts) ts[j] = lp;
    }
    if (threadIdx.x == 0 && bs->seq_out) bs->seq_out[out] = filled ? a.fin_score[o] : BEAM_NEG;
}

bool beam_args_ok(const BeamArgs& a) {
    return a.W >= 1 && a.W <= BEAM_MAX && a.R > 0 && a.R % a.W == 0 && a.R <= a.anc_rows && a.anc && a.anc_pitch % 16 == 0 && a.fed_tok && a.fed_lp &&
           a.run && a.fin_score && a.fin_len && a.fin_store && a.fin_tok && a.fin_lp && a.n_fin && a.slot_anc && a.beam && a.shared &&
           a.n_channels >= 1 && a.V >= 1;
}

}  // namespace

int launch_beam_select(const BeamArgs& a, hipStream_t stream) {
    if (!beam_args_ok(a) || !a.logits) return -1;
    if (a.row_pos) {
        if (!a.row_out || !a.row_prompt || !a.finished) return -1;
        beam_select_kernel<true><<<a.R / a.W, 256, 0, stream>>>(a);
    } else {
        beam_select_kernel<false><<<a.R / a.W, 256, 0, stream>>>(a);
    }
    return 0;
}

int launch_beam_init(const BeamArgs& a, int n_steps, const int32_t* prompt, int n_prompt, const ConstraintView& cv, const BeamShared& params,
                     hipStream_t stream) {
    if (!beam_args_ok(a)) return -1;
    if (n_prompt < 0 || (n_prompt > 0 && !prompt) || n_prompt + n_steps >= a.anc_pitch || n_prompt + n_steps >= a.fed_pitch) return -1;
    if (cv.allowed && (!cv.next || !a.row_state || cv.n_states < 1 || cv.words * 32 < a.V)) return -1;
    if (!params.tokens_out) return -1;
    beam_init_kernel<<<a.R, 256, 0, stream>>>(a, n_steps, prompt, n_prompt, cv, params);
    return 0;
}

int launch_beam_finalize(const BeamArgs& a, int N, hipStream_t stream) {
    if (!beam_args_ok(a) || N < 1 || N > a.W || a.row_out) return -1;
    beam_finalize_kernel<<<a.R / a.W * N, 256, 0, stream>>>(a, N, 0);
    return 0;
}

int launch_beam_slot_start(const BeamArgs& a, int row0, long long first_group, int n_prompt, const ConstraintView& cv, hipStream_t stream) {
    const int rows = a.n_channels * a.W;
    if (!beam_args_ok(a) || !a.row_pos || !a.row_out || !a.row_prompt || !a.finished || row0 < 0 || row0 % rows || row0 + rows > a.R || first_group < 0 ||
        n_prompt < 0)
        return -1;
    if (cv.start && (!a.row_state || cv.n_states < 1)) return -1;
    beam_slot_start_kernel<<<rows, 256, 0, stream>>>(a, row0, first_group, n_prompt, cv);
    return 0;
}

int launch_beam_slot_finalize(const BeamArgs& a, int row0, int N, hipStream_t stream) {
    const int rows = a.n_channels * a.W;
    if (!beam_args_ok(a) || N < 1 || N > a.W || !a.row_out || row0 < 0 || row0 % rows || row0 + rows > a.R) return -1;
    beam_finalize_kernel<<<a.n_channels * N, 256, 0, stream>>>(a, N, row0 / a.W);
    return 0;
}
