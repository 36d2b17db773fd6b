// Full-sequence (teacher-forced) decoder pass: with the ids GIVEN, every position of every decoder row is computed at once and the
// decoder becomes an encoder-shaped MFMA workload (include/ymt3.h, sequence scoring).  Projections and FFN are launch_gemm /
// launch_rmsnorm over rows x positions; this file holds what those cannot do:
//
//   seq_embed_kernel          the fed id of every (row, position) -- pad, prompt, tokens -- and its f32 residual row
//   dec_seq_attn_kernel<1>    causal self-attention over up to max_decode_len keys, by-distance bias
//   dec_seq_attn_kernel<0>    cross-attention, many queries per row over the segment's T keys
//   seq_lm_head_score_kernel  logits in MFMA column tiles with an online log-sum-exp per row: writes logit[target] - lse, and
//                             the logits only when asked for (64 x 1024 x 1536 f32 logits are 400 MB)
//
// The attention kernel has the shape of enc_attn_kernel: S^T = K Q^T with v_mfma_f32_16x16x32_bf16 (each lane owns ONE query column
// and 4 consecutive keys per accumulator: softmax statistics are lane-local plus two shuffles), the exponentials rounded to bf16
// are the B operand of O^T = V^T P^T, and V^T fragments come from the row-major LDS image through ds_read_b64_tr_b16.  1024 keys x 64
// of K and V are 256 KB, more than the LDS, so keys stream through LDS in tiles of 64 (double buffered: the next tile's global loads
// are in flight under the current tile's math, one barrier per tile) with f32 running max and sum.
//
// Numerics contract (DESIGN.md sections 2 and 30): THE TILE SCHEDULE.  e = exp(s - running max AFTER the current 64-key tile) rounded to bf16
// for P.V, the normaliser sums the unrounded f32 e, a rescale by exp(old max - new max) multiplies the f32 accumulators and the f32 sum
// alike, output rounded to bf16 (tests/seq_kernel_model.py::attention_tiles states it in float64).  Up to 64 keys that is the encoder
// kernel's contract, oracle/ymt3_oracle.py::attention(round_p=True), bit for bit; beyond, the oracle rounds exp(s - GLOBAL max), another
// grid for P wherever a later tile raises the maximum: the same model in another correct arithmetic, compared within tolerances only.
// Not the step kernels' all-f32 softmax.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int DKV = 64;
constexpr int ROWB = 144;    // LDS row pitch in bytes (128 + 16 pad), as enc_attn.hip
constexpr int QB = 128;      // queries per workgroup: 8 waves x 16
constexpr int KT = 64;       // keys per LDS tile
constexpr int NB = QB + KT;  // bias window of a (query block, key tile) pair: QB + KT - 1 distances

__global__ __launch_bounds__(256) void seq_embed_kernel(SeqEmbedArgs a) {
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per (row, position)
    const int lane = threadIdx.x & 63;
    if (m >= (long long)a.n_rows * a.L) return;
    const int lr = (int)(m / a.L), pos = (int)(m % a.L), r = a.row0 + lr;
    int id;
    if (pos == 0) id = a.pad_id;
    else if (pos <= a.n_prompt) id = a.prompt[(size_t)r * a.n_prompt + pos - 1];
    else id = a.tokens[(size_t)r * a.n_steps + pos - a.n_prompt - 1];
    id = min(max(id, 0), a.V - 1);                                          // clamped where it is fed, as the forced path does
    float e[8], c[8];
    unpack8(*reinterpret_cast<const uint4*>(a.embed + (size_t)id * 512 + lane * 8), e);
    if (a.chan_embed) {
        unpack8(*reinterpret_cast<const uint4*>(a.chan_embed + (size_t)(r % a.n_channels) * 512 + lane * 8), c);
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] += c[i];
    }
    float4* dst = reinterpret_cast<float4*>(a.h + (size_t)m * 512 + lane * 8);
    dst[0] = make_float4(e[0], e[1], e[2], e[3]);
    dst[1] = make_float4(e[4], e[5], e[6], e[7]);
}

// grid (query blocks, heads, decoder rows).  Every lane stays active to the end (ds_read_b64_tr_b16 needs a full EXEC mask):
// queries beyond L are computed on clamped addresses and not stored; key rows beyond n_keys are ZERO in LDS, never stale memory
// (a masked probability is exactly 0, and 0 x stale NaN would not be).
template <bool CAUSAL>
__global__ __launch_bounds__(512) void dec_seq_attn_kernel(SeqAttnDecArgs a) {
    __shared__ __attribute__((aligned(16))) char sK[2][KT * ROWB];
    __shared__ __attribute__((aligned(16))) char sV[2][KT * ROWB];
    __shared__ float sB[2][NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int qb = blockIdx.x, h = blockIdx.y, r = blockIdx.z;
    const int q0 = qb * QB + wave * 16, q = q0 + li;                          // this lane's query position
    const size_t kvb = (size_t)((a.row0 + r) / a.rows_per_kv) * a.kv_seq + (size_t)h * a.kv_head;
    const bf16_t* kp = a.k + kvb;
    const bf16_t* vp = a.v + kvb;
    const float* bp = CAUSAL ? a.bias + (size_t)h * a.bias_stride : nullptr;
    const int last_q = min(qb * QB + QB - 1, a.L - 1);
    const int n_kt = CAUSAL ? last_q / KT + 1 : (a.n_keys + KT - 1) / KT;     // causal: tiles wholly beyond the query block are skipped

    bf16x8 qf[2];
    {
        const bf16_t* qr = a.q + (size_t)r * a.q_seq + (size_t)min(q, a.L - 1) * a.ldq + h * DKV;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(qr + ks * 32 + g * 8));
    }
    // staging: thread -> (key row tid >> 3, 16-byte chunk tid & 7) of the K and the V tile, threads 0 .. NB-2 one bias entry each
    const int srow = tid >> 3, sch = tid & 7;
    uint4 kc, vc;
    float bc = 0.f;
    auto fetch = [&](int kt) {
        const int key = kt * KT + srow;
        kc = make_uint4(0u, 0u, 0u, 0u);
        vc = kc;
        if (key < a.n_keys) {
            kc = *reinterpret_cast<const uint4*>(kp + (size_t)key * a.ldkv + sch * 8);
            vc = *reinterpret_cast<const uint4*>(vp + (size_t)key * a.ldkv + sch * 8);
        }
        if (CAUSAL && tid < NB - 1) {
            const int dist = qb * QB - (kt * KT + KT - 1) + tid;              // entry tid of the window: query - key
            bc = bp[min(max(dist, 0), a.bias_stride - 1)];
        }
    };
    auto stage = [&](int buf) {
        *reinterpret_cast<uint4*>(sK[buf] + srow * ROWB + sch * 16) = kc;
        *reinterpret_cast<uint4*>(sV[buf] + srow * ROWB + sch * 16) = vc;
        if (CAUSAL && tid < NB - 1) sB[buf][tid] = bc;
    };
    fetch(0);
    stage(0);
    __syncthreads();

    float mx = -3.0e38f, sum = 0.f;                                           // running max (the query's), this lane's share of the running sum
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    for (int kt = 0; kt < n_kt; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < n_kt) fetch(kt + 1);
        if (!CAUSAL || kt * KT <= q0 + 15) {                                  // wave-uniform: a tile wholly beyond this wave's queries
            const char* tK = sK[buf];
            const char* tV = sV[buf];
            // S^T tiles: lane -> query q, keys kt*64 + t*16 + 4g + r
            f32x4 s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 kf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(tK + (t * 16 + li) * ROWB + (ks * 4 + g) * 16));
                    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[t], 0, 0, 0);
                }
            }
            float tmax = -3.0e38f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int kl = t * 16 + 4 * g + rr, key = kt * KT + kl;
                    float v = s[t][rr];
                    if (CAUSAL) v = key <= q ? v + sB[buf][wave * 16 + li - kl + KT - 1] : -INFINITY;   // the diagonal tile, per element
                    else v = key < a.n_keys ? v : -INFINITY;
                    s[t][rr] = v;
                    tmax = fmaxf(tmax, v);
                }
            tmax = fmaxf(tmax, lane_xor16(tmax));
            tmax = fmaxf(tmax, lane_xor32(tmax));
            const float mn = fmaxf(mx, tmax);
            const float alpha = __expf(mx - mn);
            mx = mn;
            float part = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float e = __expf(s[t][rr] - mn);
                    s[t][rr] = e;
                    part += e;
                }
            sum = sum * alpha + part;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
            // O^T[d][q] += sum_key V^T[d][key] P^T[key][q]; k-step = key sub-tiles (2kp, 2kp+1)
#pragma unroll
            for (int kp2 = 0; kp2 < 2; ++kp2) {
                bf16x8 pf;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    pf[rr] = (__bf16)s[2 * kp2][rr];
                    pf[4 + rr] = (__bf16)s[2 * kp2 + 1][rr];
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int r0 = (2 * kp2) * 16 + 4 * g + (li >> 2);
                    const int col = dt * 16 + 4 * (li & 3);
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tV + r0 * ROWB + col * 2));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tV + (r0 + 16) * ROWB + col * 2));
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
                }
            }
        }
        if (kt + 1 < n_kt) stage(buf ^ 1);       // every wave left that buffer at the barrier that closed the previous tile
        __syncthreads();
    }
    sum += lane_xor16(sum);
    sum += lane_xor32(sum);
    const float inv = 1.0f / sum;
    if (q < a.L) {
        bf16_t* orow = a.out + (size_t)r * a.o_seq + (size_t)q * a.ldo + h * DKV;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const uint2 pk = make_uint2(pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv), pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv));
            *reinterpret_cast<uint2*>(orow + dt * 16 + 4 * g) = pk;
        }
    }
}

// logits^T tiles = lm_head tile (16 tokens x 512) . xn^T, the token tile as the MFMA A operand: a lane holds 4 consecutive tokens of
// ONE row, so the running max / sum of the row's log-sum-exp are lane-local over the lane's quarter of every tile and meet the other
// three quarters once, at the end.  A workgroup = 4 waves x 32 rows with their normed rows (bf16 [32][512]) held in registers for the
// whole vocabulary; token tiles go through LDS, double buffered.  d_model = 512.
constexpr int LM_VT = 16, LM_PITCH = 1024 + 16;
__global__ __launch_bounds__(256) void seq_lm_head_score_kernel(SeqLmHeadArgs a) {
    __shared__ __attribute__((aligned(16))) char sW[2][LM_VT * LM_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int m_base = blockIdx.x * 128 + wave * 32;
    bf16x8 xf0[16], xf1[16];
    int tgt0, tgt1;
    long long at0, at1;                  // (row, emitted column) flat index, or -1: a prompt position or a row beyond M
    auto load_rows = [&](int rs, bf16x8 (&xf)[16], int& tgt, long long& at) {
        const int m = m_base + rs * 16 + li, mc = min(m, a.M - 1);
        const bf16_t* xr = a.xn + (size_t)mc * 512;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) xf[ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(xr + ks * 32 + g * 8));
        const int lr = mc / a.L, j = mc % a.L - a.n_prompt;
        at = (m < a.M && j >= 0) ? (long long)(a.row0 + lr) * a.n_steps + j : -1;
        tgt = at >= 0 ? min(max(a.tokens[at], 0), a.V - 1) : -1;
    };
    load_rows(0, xf0, tgt0, at0);
    load_rows(1, xf1, tgt1, at1);
    const int n_vt = a.V / LM_VT;
    uint4 wc0, wc1, wc2, wc3;
    const int frow = tid >> 6, fch = tid & 63;           // staging: thread -> token rows frow + 4i, 16-byte chunk fch
    auto fetch = [&](int vt) {
        const bf16_t* src = a.W + (size_t)(vt * LM_VT + frow) * 512 + fch * 8;
        wc0 = *reinterpret_cast<const uint4*>(src);
        wc1 = *reinterpret_cast<const uint4*>(src + 4 * 512);
        wc2 = *reinterpret_cast<const uint4*>(src + 8 * 512);
        wc3 = *reinterpret_cast<const uint4*>(src + 12 * 512);
    };
    auto stage = [&](int buf) {
        char* dst = sW[buf] + frow * LM_PITCH + fch * 16;
        *reinterpret_cast<uint4*>(dst) = wc0;
        *reinterpret_cast<uint4*>(dst + 4 * LM_PITCH) = wc1;
        *reinterpret_cast<uint4*>(dst + 8 * LM_PITCH) = wc2;
        *reinterpret_cast<uint4*>(dst + 12 * LM_PITCH) = wc3;
    };
    fetch(0);
    stage(0);
    __syncthreads();
    float mx0 = -3.0e38f, mx1 = -3.0e38f, sm0 = 0.f, sm1 = 0.f, tl0 = -INFINITY, tl1 = -INFINITY;
    // one tile's 4 logits of a row into its running statistics (and to memory, if asked for)
    auto update = [&](const f32x4& acc, int v0, int tgt, long long at, float& mx, float& sm, float& tl) {
        if (a.logits && at >= 0) *reinterpret_cast<float4*>(a.logits + (size_t)at * a.V + v0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        const float mn = fmaxf(mx, fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])));
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            part += __expf(acc[i] - mn);
            if (v0 + i == tgt) tl = acc[i];
        }
        sm = sm * __expf(mx - mn) + part;
        mx = mn;
    };
    for (int vt = 0; vt < n_vt; ++vt) {
        const int buf = vt & 1;
        if (vt + 1 < n_vt) fetch(vt + 1);
        f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const bf16x8 wf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(sW[buf] + li * LM_PITCH + (ks * 4 + g) * 16));
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf0[ks], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf1[ks], acc1, 0, 0, 0);
        }
        const int v0 = vt * LM_VT + 4 * g;                                    // acc[i]: token v0 + i of row m_base + rs*16 + li
        update(acc0, v0, tgt0, at0, mx0, sm0, tl0);
        update(acc1, v0, tgt1, at1, mx1, sm1, tl1);
        if (vt + 1 < n_vt) stage(buf ^ 1);
        __syncthreads();
    }
    // the four lanes of a row (its four quarters of every tile) meet; one of them holds the target's logit, the others -inf
    auto finish = [&](long long at, float mx, float sm, float tl) {
        float mall = fmaxf(mx, lane_xor16(mx));
        mall = fmaxf(mall, lane_xor32(mall));
        float s = sm * __expf(mx - mall);
        s += lane_xor16(s);
        s += lane_xor32(s);
        float t = fmaxf(tl, lane_xor16(tl));
        t = fmaxf(t, lane_xor32(t));
        if (g == 0 && at >= 0) {
            const long long row = at / a.n_steps;
            const int j = (int)(at % a.n_steps);
            const int len = a.lengths ? min(max(a.lengths[row], 0), a.n_steps) : a.n_steps;
            a.scores[at] = j < len ? t - (mall + logf(s)) : 0.f;             // NaN logits, or all -inf (s = 0, t = -inf): NaN
        }
    };
    finish(at0, mx0, sm0, tl0);
    finish(at1, mx1, sm1, tl1);
}

}  // namespace

int launch_seq_embed(const SeqEmbedArgs& a, hipStream_t stream) {
    if (a.n_rows <= 0 || a.L <= 0) return 0;
    if (a.d != 512 || a.V <= 0 || (a.n_prompt > 0 && !a.prompt)) return -1;
    const long long M = (long long)a.n_rows * a.L;
    seq_embed_kernel<<<(unsigned)((M + 3) / 4), 256, 0, stream>>>(a);
    return 0;
}

int launch_dec_seq_attention(bool causal, const SeqAttnDecArgs& a, hipStream_t stream) {
    if (a.n_rows <= 0 || a.L <= 0) return 0;
    if (a.n_keys <= 0 || a.rows_per_kv <= 0 || a.H <= 0 || a.H > 65535 || a.n_rows > 65535) return -1;
    if ((a.ldq | a.ldkv | a.ldo) % 8 || (a.q_seq | a.kv_seq | a.o_seq | (long long)a.kv_head) % 8) return -1;     // 16-byte rows
    if (causal && (!a.bias || a.bias_stride <= 0 || a.n_keys != a.L)) return -1;
    const dim3 grid((a.L + QB - 1) / QB, a.H, a.n_rows);
    if (causal) dec_seq_attn_kernel<true><<<grid, 512, 0, stream>>>(a);
    else dec_seq_attn_kernel<false><<<grid, 512, 0, stream>>>(a);
    return 0;
}

int launch_seq_lm_head_score(const SeqLmHeadArgs& a, hipStream_t stream) {
    if (a.M <= 0) return 0;
    if (a.d != 512 || a.V <= 0 || a.V % LM_VT || a.L <= 0 || a.n_steps <= 0 || !a.tokens || !a.scores) return -1;
    seq_lm_head_score_kernel<<<(a.M + 127) / 128, 256, 0, stream>>>(a);
    return 0;
}
