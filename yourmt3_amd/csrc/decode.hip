// Autoregressive decoder step kernels (a7, a8, a10 of SURVEY.md section 8).
//
// Every kernel reads the decode position from DecodeShared in device memory, so ONE captured
// hipGraph of a step can be replayed for every position with no host round trip (SURVEY section 3.4:
// the per-step `.max()==0` host sync of TP: generation/utils.py:2936-2937 becomes device state).
//
//  dec_gemm_kernel      skinny GEMM, R = segments x channels rows (up to 511) against a [N][K] bf16
//                       weight: one workgroup per 16 rows x 16 output columns, eight waves split K, each
//                       wave pulls its K-slice of both operands with whole-line coalesced loads (all in
//                       flight at once), parks them in a wave-private LDS strip and reads MFMA fragments
//                       back; partial tiles are summed through LDS in a fixed order (bitwise reproducible;
//                       no float atomics).  NORM modes apply the T5 RMS norm (TP: modeling_t5.py:50-72)
//                       with the row's sum(h^2) carried between kernels as partials; the epilogues fuse
//                       KV-cache append (TP: cache_utils.py:144-145), ReLU, residual add + sum(h^2) partials.
//  dec_gemm_mid_kernel  the same GEMMs on BM x 64 tiles with a K loop, from 512 rows on (the 13-channel decoder).
//  dec_attn_kernel      one (row, head) per workgroup; K/V slabs streamed HBM -> registers with 16-byte
//                       coalesced loads, 8-12 in flight per lane; online softmax per 8-lane group (DPP sums),
//                       merged by shuffles and one LDS pass.  Self-attention adds the unidirectional relative
//                       position bias by distance (TP: modeling_t5.py:264-279) and, up to 96 rows, ends with its
//                       head's share of the output projection (OP); cross-attention has no bias and
//                       computes its own query projection (FUSEQ) while its K/V loads are in flight.
//  argmax_embed_kernel  fp32 argmax (first index wins ties, TP: utils.py:2925), EOS -> PAD fill
//                       (:2928-2929), token store, next-token embedding gather into the residual
//                       stream, and the step counter advance by the last workgroup to finish.  The first
//                       n_prompt steps of a call (a task prompt, HF `decoder_input_ids` after the start id)
//                       feed the caller's ids instead and emit nothing.  With a scores buffer it also writes
//                       log_softmax(logits)[fed id] per emitted token: a second pass over the row for sum(exp(v - max)).
//                       Under a token automaton (include/ymt3.h, constraints) both passes skip the tokens the row's state does
//                       not allow, and thread 0 moves the row's state along the fed id.
//
// Oracle: oracle/ymt3_oracle.py::decoder_step / greedy_decode.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int DKV = 64;
constexpr int WO_LDS_BYTES = 8 * 64 * 128;     // folded O-projection: the head's 64 k of all 512 wo rows
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Measurement only (YMT3_STAMP=1 at ymt3_create; the pointer is null otherwise): constant-rate wall clock (100 MHz) at the
// first instruction of a workgroup and at the end of its last wave, read back by ymt3_debug_step_stamps to split a decode
// step into launch gaps, dispatch ramps and kernel bodies.
#ifndef YMT3_STAMP_PHASE
#define YMT3_STAMP_PHASE 0           // 1 / 2: timing-only builds that move dec_gemm_kernel's entry stamp to a later phase (tools, not product)
#endif
#define STAMP_IN(a) do { if ((a).stamp && threadIdx.x == 0) (a).stamp[2 * blockIdx.x] = wall_clock64(); } while (0)
// attention pair only: stage marks behind the [grid][2] stamps of the kernel's slot (1024 words for its 512 workgroups), 8 per workgroup
#define PAIR_MARK(a, k, v) do { if ((a).stamp && threadIdx.x == 0) (a).stamp[1024 + 8 * blockIdx.x + (k)] = (v); } while (0)
#define STAMP_OUT(a) do { if ((a).stamp && (threadIdx.x & 63) == 0) atomicMax((a).stamp + 2 * blockIdx.x + 1, (unsigned long long)wall_clock64()); } while (0)

// ------------------------------------------------------------------------------------------------
// 512 threads = 8 waves; one workgroup = a 16 rows x 16 columns output tile over the full K, each wave
// owning K/8 of the reduction.  Small tiles keep every workgroup's operand traffic small (the per-CU load
// path is what bounds these kernels, not HBM); workgroups that share a weight tile are placed on one XCD
// (same blockIdx % 8) so its re-reads hit that XCD's L2.
//
// Operand path: every wave pulls ITS K-slice of the 16 activation rows and 16 weight rows
// with fully coalesced 16-byte loads (8..32 consecutive lanes per row = whole 128-byte lines), all
// issued up front (one memory round trip), parks them in a wave-private LDS strip, and reads them
// back in MFMA fragment order with ds_read_b128.  Fragment-shaped global loads (16 rows x 64 B per
// instruction) measured 3-4x slower for the same bytes (profiles/r01_notes.md).  No workgroup barrier
// is needed for the strip: only the owning wave touches it and LDS executes a wave's ops in order.
// (A 64-row-tile variant with direct fragment loads was measured 13-15 % slower at 256 and 832 rows and removed.)
//
// The RMS norm needs sum(x^2) over the FULL row, which no single wave sees: it is carried between
// kernels as per-row partial sums `ssq[tile][row]` written by whoever last wrote the residual stream
// (the 32 column tiles of the RESID epilogue, or the embedding gather) and summed in a fixed order.
// NT = 16-column tiles per workgroup (1 or 2): two halve the workgroup count of the wide projections (QKV, FFN-in, lm_head)
// to about one per CU -- at two per CU the second one's operands queue behind the first's and the kernel's last exit came
// 1.1 us after its first (profiles/r01_step_stamps.txt) -- and the activation strip is read once for both.
// PEND (NORM modes, MoE decoder): the residual stream still lacks the previous layer's expert outputs -- x = h + (y[2r] + y[2r+1]),
// the sum the MoE combine launch used to store.  The kernel forms x while loading, takes sum(x^2) itself (16-lane row sums, then
// the eight waves in order), and the workgroups of column tile 0 write x to a.h_out, the OTHER residual buffer (the rest of the
// layer reads that one; writing in place would race with the other column tiles still reading h): one launch less per MoE layer.
template <int MODE, int K, int NT, bool PEND = false>
__global__ __launch_bounds__(512) void dec_gemm_kernel(const bf16_t* __restrict__ pW, const void* __restrict__ pX, const float* __restrict__ pGain,
                                                       float* pSsq, float* pOut, int row0, int R, int N, int ssq_stride, DecGemmArgs a) {
    // The operand pointers and the tile geometry are LEADING SCALAR kernel arguments (14 dwords): built with
    // -mllvm -amdgpu-kernarg-preload-count=16 they arrive in SGPRs with the dispatch instead of through a scalar load at the head
    // of the kernel's critical path (every global load's address depends on them).  `a` carries the rest, read when needed.
    constexpr bool NORM = (MODE != DG_RESID);
    constexpr int KW = K / 8;            // K slice per wave
    constexpr int KS = KW / 32;          // MFMA k-steps per wave
    constexpr int ROWS = 16, COLS = 16 * NT;
    constexpr int PITCH = KW * 2 + 16;   // bytes per strip row (bf16 slice + 16 B pad against bank conflicts)
    constexpr int STRIP = 16 * PITCH;    // one operand strip (16 rows) of one wave
    static_assert(MODE != DG_RESID || NT == 1, "the RESID epilogue writes one sum(h^2) partial per 16-column tile");
    static_assert(!PEND || NORM, "a pending combine is folded into the norm prologue");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem);                    // [8][ROWS][COLS]
    float* sscale = red + 8 * ROWS * COLS;                          // [ROWS]
    float* wpart = sscale + ROWS;                                   // PEND: [8 waves][ROWS] sum(x^2) of each wave's K-slice
    char* strips = smem + (8 * ROWS * COLS + ROWS + (PEND ? 8 * ROWS : 0)) * 4;   // [8 waves][A strip | NT W strips]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    // block -> (n tile, m tile): blocks with equal blockIdx % 8 (one XCD under round-robin placement;
    // speed only) walk the m tiles of one n tile back to back
    const int n_mt = (R + ROWS - 1) / ROWS, n_nt = N / COLS;
    int nt_idx, mt_idx;
    if ((n_nt & 7) == 0) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        mt_idx = slot % n_mt;
        nt_idx = (slot / n_mt) * 8 + xcd;
    } else {
        mt_idx = blockIdx.x % n_mt;
        nt_idx = blockIdx.x / n_mt;
    }
    const int n0 = nt_idx * COLS, m0 = row0 + mt_idx * ROWS, m_end = row0 + R;

    // epilogue ownership: thread -> (row mr, 2 columns nq)
    const bool epi = tid < ROWS * 8 * NT;
    const int mr = tid / (8 * NT), nq = (tid % (8 * NT)) * 2;
    const int m = m0 + mr, n = n0 + nq;
    const bool live = epi && m < m_end;
    float2 hold = make_float2(0.f, 0.f);
    float2 hp[8];                                // DG_RESID with a.part: the eight per-head partials of the folded O-projection
    if constexpr (MODE == DG_RESID) {
        if (live) hold = *reinterpret_cast<const float2*>(pOut + (size_t)m * N + n);   // prefetch the RMW operand
        if (a.part && live) {
#pragma unroll
            for (int w = 0; w < 8; ++w) hp[w] = *reinterpret_cast<const float2*>(a.part + ((size_t)m * 8 + w) * N + n);
        }
    }
    int step = 0;                                // cache position of the KV append: requested now, not as a round trip in the epilogue
    if constexpr (MODE == DG_NORM_QKV_CACHE) step = a.row_pos ? a.row_pos[m < m_end ? m : m_end - 1] : a.shared->step;

    f32x4 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    {
        char* sA = strips + wave * (1 + NT) * STRIP;
        char* sW = sA + STRIP;
        // weight slice: LPRW lanes cover one row's KW bf16
        constexpr int LPRW = KW * 2 / 16, RPIW = 64 / LPRW, NIA = 16 / RPIW, NIW = NIA * NT;
        u32x4 wv[NIW];
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int row = i * RPIW + lane / LPRW, ch = lane % LPRW;
            wv[i] = *reinterpret_cast<const u32x4*>(pW + (size_t)(n0 + row) * K + wave * KW + ch * 8);
        }
        if constexpr (NORM) {
            constexpr int LPRX = KW * 4 / 16, RPIX = 64 / LPRX, NIX = 16 / RPIX;   // fp32 rows
            f32x4 xv[NIX];
#pragma unroll
            for (int i = 0; i < NIX; ++i) {
                int mm = m0 + i * RPIX + lane / LPRX;
                mm = mm < m_end ? mm : m_end - 1;
                xv[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(pX) + (size_t)mm * K + wave * KW + (lane % LPRX) * 4);
            }
            const f32x4 gv = *reinterpret_cast<const f32x4*>(pGain + wave * KW + (lane % LPRX) * 4);
            f32x4 y0v[PEND ? NIX : 1], y1v[PEND ? NIX : 1];
            float ss = 0.f;
            if constexpr (PEND) {
#pragma unroll
                for (int i = 0; i < NIX; ++i) {
                    int mm = m0 + i * RPIX + lane / LPRX;
                    mm = mm < m_end ? mm : m_end - 1;
                    const float* yr = a.pend_y + (size_t)(2 * mm) * K + wave * KW + (lane % LPRX) * 4;
                    y0v[i] = *reinterpret_cast<const f32x4*>(yr);
                    y1v[i] = *reinterpret_cast<const f32x4*>(yr + K);
                }
            } else if (tid < ROWS * 8) {                             // 8 threads per row, 4 of the 32 partials each
                const int mm = m0 + (tid >> 3) < m_end ? m0 + (tid >> 3) : m_end - 1;
#pragma unroll
                for (int j = 0; j < 4; ++j) ss += pSsq[(size_t)((tid & 7) * 4 + j) * ssq_stride + mm];
            }
            __builtin_amdgcn_sched_barrier(0);   // every operand load is in flight before anything waits
            STAMP_IN(a);                         // (reads a.stamp from the kernarg segment: after the loads, not in front of them)
            if constexpr (PEND) {
#pragma unroll
                for (int i = 0; i < NIX; ++i) {
                    const int row = i * RPIX + lane / LPRX;
#pragma unroll
                    for (int e = 0; e < 4; ++e) xv[i][e] += y0v[i][e] + y1v[i][e];          // h + (y0 + y1), as the combine kernel summed
                    float q = (xv[i][0] * xv[i][0] + xv[i][1] * xv[i][1]) + (xv[i][2] * xv[i][2] + xv[i][3] * xv[i][3]);
                    q = add_xor8(sum8(q));                           // the LPRX = 16 lanes that hold this row's K-slice (lanes ^1, ^2, ^4, ^8)
                    if ((lane % LPRX) == 0) wpart[wave * ROWS + row] = q;
                    if constexpr (MODE == DG_NORM_QKV_CACHE) {       // (lm_head is the last reader of the stream: nothing to publish)
                        if (nt_idx == 0 && m0 + row < m_end)         // column tile 0 publishes the completed residual row
                            *reinterpret_cast<f32x4*>(a.h_out + (size_t)(m0 + row) * K + wave * KW + (lane % LPRX) * 4) = xv[i];
                    }
                }
            } else {
                ss = sum8(ss);
                if (tid < ROWS * 8 && (tid & 7) == 0) sscale[tid >> 3] = rsqrtf(ss / (float)K + a.eps);
            }
#pragma unroll
            for (int i = 0; i < NIW; ++i)
                *reinterpret_cast<u32x4*>(sW + (i * RPIW + lane / LPRW) * PITCH + (lane % LPRW) * 16) = wv[i];
            __syncthreads();
            if constexpr (PEND) {
                if (tid < ROWS) {
                    float t = wpart[tid];
#pragma unroll
                    for (int w = 1; w < 8; ++w) t += wpart[w * ROWS + tid];
                    sscale[tid] = rsqrtf(t / (float)K + a.eps);
                }
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < NIX; ++i) {
                const int row = i * RPIX + lane / LPRX;
                const float sc = sscale[row];
                *reinterpret_cast<uint2*>(sA + row * PITCH + (lane % LPRX) * 8) =
                    make_uint2(pack_bf16x2(xv[i][0] * sc * gv[0], xv[i][1] * sc * gv[1]),
                               pack_bf16x2(xv[i][2] * sc * gv[2], xv[i][3] * sc * gv[3]));
            }
        } else {
            u32x4 av[NIA];
#pragma unroll
            for (int i = 0; i < NIA; ++i) {
                int mm = m0 + i * RPIW + lane / LPRW;
                mm = mm < m_end ? mm : m_end - 1;
                av[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(pX) + (size_t)mm * K + wave * KW + (lane % LPRW) * 8);
            }
            __builtin_amdgcn_sched_barrier(0);   // every operand load is in flight before anything waits
            STAMP_IN(a);
#pragma unroll
            for (int i = 0; i < NIW; ++i) {
                const int off = (i * RPIW + lane / LPRW) * PITCH + (lane % LPRW) * 16;
                *reinterpret_cast<u32x4*>(sW + off) = wv[i];
                if (i < NIA) *reinterpret_cast<u32x4*>(sA + off) = av[i];
            }
        }
        // fragment order read-back (wave-private strips: in-order LDS, no barrier)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int off = li * PITCH + (ks * 32 + g * 8) * 2;
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(sA + off);
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(sW + c * STRIP + off);
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[c], 0, 0, 0);
            }
        }
    }

#if YMT3_STAMP_PHASE == 1
    STAMP_IN(a);             // timing-only build: "entry" = operands have arrived and the MFMAs are done
#endif
    // fixed-order cross-wave reduction: red[wave][row][n (COLS)]
#pragma unroll
    for (int c = 0; c < NT; ++c)
        *reinterpret_cast<float4*>(red + ((wave * ROWS + li) * COLS + c * 16 + g * 4)) =
            make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    __syncthreads();
#if YMT3_STAMP_PHASE == 2
    STAMP_IN(a);             // timing-only build: "entry" = partial tiles reduced across waves, epilogue next
#endif
    float2 s = make_float2(0.f, 0.f);
    if (epi) {
        s = *reinterpret_cast<const float2*>(red + (mr * COLS + nq));
#pragma unroll
        for (int w = 1; w < 8; ++w) {
            const float2 t = *reinterpret_cast<const float2*>(red + ((w * ROWS + mr) * COLS + nq));
            s.x += t.x; s.y += t.y;
        }
    }

    if constexpr (MODE == DG_RESID) {
        float2 o = make_float2(0.f, 0.f);
        if (live) {
            if (a.part) {                         // h + (p0 + ... + p7): what the separate O-projection launch left in h
                float2 sp = hp[0];
#pragma unroll
                for (int w = 1; w < 8; ++w) { sp.x += hp[w].x; sp.y += hp[w].y; }
                hold.x += sp.x; hold.y += sp.y;
            }
            o = make_float2(hold.x + s.x, hold.y + s.y);
            *reinterpret_cast<float2*>(pOut + (size_t)m * N + n) = o;
        }
        // this tile's share of sum(h^2) for the next norm
        float q = o.x * o.x + o.y * o.y;
        q = sum8(q);
        if (live && (tid & 7) == 0) pSsq[(size_t)nt_idx * ssq_stride + m] = q;
    } else if constexpr (MODE == DG_NORM_LOGITS) {
        if (live) *reinterpret_cast<float2*>(pOut + (size_t)m * N + n) = s;
    } else if (live) {
        if constexpr (MODE == DG_NORM_BF16_RELU) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); }
        const uint32_t pk = pack_bf16x2(s.x, s.y);
        if constexpr (MODE == DG_NORM_QKV_CACHE) {
            const int inner = a.H * DKV;
            if (a.table) {                       // the layer-0 table build (ymt3_create): the packed row as it is, row = token id
                *reinterpret_cast<uint32_t*>(a.table + (size_t)m * N + n) = pk;
            } else if (n < inner) {
                *reinterpret_cast<uint32_t*>(a.out_bf16 + (size_t)m * inner + n) = pk;
            } else {
                const int nn = n - inner, kv = nn / inner, hh = (nn % inner) >> 6, dd = nn & 63;
                bf16_t* cache = kv ? a.vcache : a.kcache;
                *reinterpret_cast<uint32_t*>(cache + (((size_t)m * a.H + hh) * a.L + step) * DKV + dd) = pk;
            }
        } else {
            *reinterpret_cast<uint32_t*>(a.out_bf16 + (size_t)m * N + n) = pk;
        }
    }
    STAMP_OUT(a);
}

// ------------------------------------------------------------------------------------------------
// Mid-size tile form of the same GEMMs for MANY rows (R >= 256: the 13-channel decoder's 832 rows, batches of 256+).
// The 16-row kernel above launches (R / 16) x (N / 16..32) workgroups of 143 KB LDS each -- 3328 for the FFN-in projection at
// 832 rows, thirteen rounds over the chip -- and re-reads the weights once per 16 rows.  Here one 256-thread workgroup owns a
// BM x 64 output tile (BM = 64, or 32 where N = 512 would leave the chip half empty), walks K in 64-wide steps through two LDS
// stages (operands staged through registers one step ahead; the RMS norm -- row scale from the carried sum(h^2) partials,
// gain per k -- is applied while the fp32 rows are converted), wave w owning output columns [16w, 16w + 16) of every 16-row
// block.  Same epilogues as above (KV-cache append, ReLU, residual add + sum(h^2) partials per 16-column tile, logits).
// K is accumulated in ONE MFMA chain per output (no 8-way split), so results differ from the 16-row kernel in the last
// bits: the launcher switches on R alone, and rows stay independent of their batch inside either regime.
template <int MODE, int K, int BM, int PF, int NTH>
__global__ __launch_bounds__(NTH) void dec_gemm_mid_kernel(const bf16_t* __restrict__ pW, const void* __restrict__ pX, const float* __restrict__ pGain,
                                                           float* pSsq, float* pOut, int row0, int R, int N, int ssq_stride, DecGemmArgs a) {
    constexpr bool NORM = (MODE != DG_RESID);
    constexpr int BN = 64, BK = 64, MT = BM / 16, PITCH = BK * 2 + 16, NKT = K / BK;
    // NTH = 512: two waves per SIMD, each with half of the row tiles of its 16 columns (wave & 3: columns, wave >> 2: row tiles) -- with one wave per
    // SIMD every LDS read, MFMA and barrier of a K-step was exposed (K = 2048 at 832 rows: 8.5 -> ... us, profiles/r03_notes.md)
    constexpr int RG = NTH / 256, MTW = MT / RG;
    static_assert(NTH == 256 || NTH == 512, "");
    static_assert(MT % RG == 0, "row tiles split between the two wave groups");
    constexpr int A_STAGE = BM * PITCH, W_STAGE = BN * PITCH;
    __shared__ __attribute__((aligned(16))) char sA[2][A_STAGE];
    __shared__ __attribute__((aligned(16))) char sW[2][W_STAGE];
    __shared__ float sscale[BM];
    __shared__ __attribute__((aligned(16))) float sgain[NORM ? K : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int wc = wave & 3, rg = wave >> 2;
    const int n_mt = (R + BM - 1) / BM, n_nt = N / BN;
    int nt_idx, mt_idx;
    if ((n_nt & 7) == 0) {                       // blocks with equal blockIdx % 8 (one XCD; speed only) walk the row tiles of one column tile
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        mt_idx = slot % n_mt;
        nt_idx = (slot / n_mt) * 8 + xcd;
    } else {
        mt_idx = blockIdx.x % n_mt;
        nt_idx = blockIdx.x / n_mt;
    }
    const int n0 = nt_idx * BN, m0 = row0 + mt_idx * BM, m_end = row0 + R;

    // staging registers, a ring of PF K-steps: W tile 64 x 128 B = 2 x 16 B per thread; A tile BM x 128 B (bf16) or BM x 256 B (fp32).
    // One step ahead left every step exposed to a full L2 / HBM round trip (22.6 us for K = 2048 at 832 rows, profiles/r02_notes.md)
    constexpr int NWV = 512 / NTH, NAB = (BM * 8 + NTH - 1) / NTH, NAF = BM * 16 / NTH;
    static_assert(BM * 16 % NTH == 0, "");
    static_assert(NKT % PF == 0, "the K loop is unrolled by the prefetch depth");
    u32x4 wvr[PF][NWV];
    u32x4 abr[PF][NORM ? 1 : NAB];
    f32x4 afr[PF][NORM ? NAF : 1];
    auto load_regs = [&](int kt, u32x4 (&wv)[NWV], u32x4 (&ab)[NORM ? 1 : NAB], f32x4 (&af)[NORM ? NAF : 1]) {
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int idx = tid + i * NTH, row = idx >> 3, ch = idx & 7;
            wv[i] = *reinterpret_cast<const u32x4*>(pW + (size_t)(n0 + row) * K + kt * BK + ch * 8);
        }
        if constexpr (NORM) {
#pragma unroll
            for (int i = 0; i < NAF; ++i) {
                const int idx = tid + i * NTH, row = idx >> 4, ch = idx & 15;
                int mm = m0 + row;
                mm = mm < m_end ? mm : m_end - 1;
                af[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(pX) + (size_t)mm * K + kt * BK + ch * 4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NAB; ++i) {
                const int idx = tid + i * NTH, row = idx >> 3, ch = idx & 7;
                int mm = m0 + row;
                mm = mm < m_end ? mm : m_end - 1;
                if (BM * 8 % NTH == 0 || idx < BM * 8)  // (BM = 32 with 512 threads: half of them carry a chunk)
                    ab[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(pX) + (size_t)mm * K + kt * BK + ch * 8);
            }
        }
    };
    auto store_lds = [&](int kt, int buf, const u32x4 (&wv)[NWV], const u32x4 (&ab)[NORM ? 1 : NAB], const f32x4 (&af)[NORM ? NAF : 1]) {
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int idx = tid + i * NTH, row = idx >> 3, ch = idx & 7;
            *reinterpret_cast<u32x4*>(sW[buf] + row * PITCH + ch * 16) = wv[i];
        }
        if constexpr (NORM) {
#pragma unroll
            for (int i = 0; i < NAF; ++i) {
                const int idx = tid + i * NTH, row = idx >> 4, ch = idx & 15;
                const float sc = sscale[row];
                const f32x4 gv = *reinterpret_cast<const f32x4*>(sgain + kt * BK + ch * 4);
                *reinterpret_cast<uint2*>(sA[buf] + row * PITCH + ch * 8) =
                    make_uint2(pack_bf16x2(af[i][0] * sc * gv[0], af[i][1] * sc * gv[1]), pack_bf16x2(af[i][2] * sc * gv[2], af[i][3] * sc * gv[3]));
            }
        } else {
#pragma unroll
            for (int i = 0; i < NAB; ++i) {
                const int idx = tid + i * NTH, row = idx >> 3, ch = idx & 7;
                if (BM * 8 % NTH == 0 || idx < BM * 8) *reinterpret_cast<u32x4*>(sA[buf] + row * PITCH + ch * 16) = ab[i];
            }
        }
    };

    // requested in the order of first use (vector loads return in order): the norm's inputs -- the sum(h^2) partials of this thread's row, the gain
    // vector -- then the operand ring
    float ss = 0.f;
    f32x4 gv = {0.f, 0.f, 0.f, 0.f};
    if constexpr (NORM) {
        static_assert(K / 4 <= NTH, "one float4 of the gain vector per thread");
        if (tid < K / 4) gv = *reinterpret_cast<const f32x4*>(pGain + tid * 4);
        if (tid < BM * 4) {
            const int row = tid >> 2;
            const int mm = m0 + row < m_end ? m0 + row : m_end - 1;
#pragma unroll
            for (int j = 0; j < SSQ_TILES / 4; ++j) ss += pSsq[(size_t)((tid & 3) * (SSQ_TILES / 4) + j) * ssq_stride + mm];
        }
    }
#pragma unroll
    for (int p = 0; p < PF; ++p) load_regs(p, wvr[p], abr[p], afr[p]);
    int step = 0;
    if constexpr (MODE == DG_NORM_QKV_CACHE) step = a.row_pos ? 0 : a.shared->step;       // per-row positions are read in the epilogue
    if constexpr (NORM) {
        // row scales from the carried partials (4 threads per row, 8 partials each, then the 4-lane sum) and the gain vector
        if (tid < K / 4) *reinterpret_cast<f32x4*>(sgain + tid * 4) = gv;
        if (tid < BM * 4) {
            ss = add_xor2(add_xor1(ss));
            if ((tid & 3) == 0) sscale[tid >> 2] = rsqrtf(ss / (float)K + a.eps);
        }
        __syncthreads();
    }
    // DG_RESID: the residual values this lane will add to are requested now, behind the operand ring, not in the epilogue (a dependent round trip there)
    float4 resid[MODE == DG_RESID ? MTW : 1];
    if constexpr (MODE == DG_RESID) {
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
            const int m = m0 + (rg * MTW + mt) * 16 + li;
            resid[mt] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < m_end) resid[mt] = *reinterpret_cast<const float4*>(pOut + (size_t)m * N + n0 + wc * 16 + g * 4);
        }
    }
    STAMP_IN(a);
    store_lds(0, 0, wvr[0], abr[0], afr[0]);
    __syncthreads();

    f32x4 acc[MTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kt0 = 0; kt0 < NKT; kt0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {             // ring slot j holds step kt0 + j; after its LDS store it is refilled with step kt + PF
            const int kt = kt0 + j, buf = kt & 1;
            if (kt + PF < NKT) load_regs(kt + PF, wvr[j], abr[j], afr[j]);     // slot j went to LDS one step ago (or before the loop)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(sW[buf] + (wc * 16 + li) * PITCH + (ks * 32 + g * 8) * 2);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) {
                    const bf16x8 xf = *reinterpret_cast<const bf16x8*>(sA[buf] + ((rg * MTW + mt) * 16 + li) * PITCH + (ks * 32 + g * 8) * 2);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[mt], 0, 0, 0);
                }
            }
            if (kt + 1 < NKT) {
                constexpr int PFm = PF - 1;
                const int jn = (j + 1) & PFm;
                // the other LDS stage: its last readers passed the barrier at the end of step kt - 1
                store_lds(kt + 1, buf ^ 1, wvr[jn], abr[jn], afr[jn]);          // (j is a constant after unrolling)
                __syncthreads();
            }
        }
    }

    // epilogue: lane (li, g) of wave w holds row m0 + mt*16 + li, columns n0 + 16w + 4g .. +3
    const int n = n0 + wc * 16 + g * 4;
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
        const int m = m0 + (rg * MTW + mt) * 16 + li;
        const bool live = m < m_end;
        f32x4 s = acc[mt];
        if constexpr (MODE == DG_RESID) {
            float q = 0.f;
            if (live) {
                float4* dst = reinterpret_cast<float4*>(pOut + (size_t)m * N + n);
                float4 o = resid[mt];
                o.x += s[0]; o.y += s[1]; o.z += s[2]; o.w += s[3];
                *dst = o;
                q = (o.x * o.x + o.y * o.y) + (o.z * o.z + o.w * o.w);
            }
            q += lane_xor16(q);                   // the four lanes (g) that hold this row's 16 columns of the tile
            q += lane_xor32(q);
            if (live && g == 0) pSsq[(size_t)(n0 / 16 + wc) * ssq_stride + m] = q;
        } else if constexpr (MODE == DG_NORM_LOGITS) {
            if (live) *reinterpret_cast<float4*>(pOut + (size_t)m * N + n) = make_float4(s[0], s[1], s[2], s[3]);
        } else if (live) {
            if constexpr (MODE == DG_NORM_BF16_RELU) { s[0] = fmaxf(s[0], 0.f); s[1] = fmaxf(s[1], 0.f); s[2] = fmaxf(s[2], 0.f); s[3] = fmaxf(s[3], 0.f); }
            const uint2 pk = make_uint2(pack_bf16x2(s[0], s[1]), pack_bf16x2(s[2], s[3]));
            if constexpr (MODE == DG_NORM_QKV_CACHE) {
                const int inner = a.H * DKV;
                if (n < inner) {
                    *reinterpret_cast<uint2*>(a.out_bf16 + (size_t)m * inner + n) = pk;
                } else {
                    const int nn = n - inner, kv = nn / inner, hh = (nn % inner) >> 6, dd = nn & 63;
                    const int pos = a.row_pos ? a.row_pos[m] : step;
                    bf16_t* cache = kv ? a.vcache : a.kcache;
                    *reinterpret_cast<uint2*>(cache + (((size_t)m * a.H + hh) * a.L + pos) * DKV + dd) = pk;
                }
            } else {
                *reinterpret_cast<uint2*>(a.out_bf16 + (size_t)m * N + n) = pk;
            }
        }
    }
    STAMP_OUT(a);
}

// ------------------------------------------------------------------------------------------------
// (sum8: the sum over the 8 lanes that share one key -- lane & 7 = 16-byte chunk of the 128-byte row -- by DPP moves: common.h)

// FUSEQ (cross-attention only): the query projection of the block,  q = R( R(rmsnorm(h_r) * gain) . Wq[head]^T ),  is
// computed inside this kernel instead of by a separate skinny GEMM launch.  Its operands (64 weight rows of this
// head, the residual row, the sum(h^2) partials) are independent of the K/V stream, so they are issued first and
// the whole projection runs while the K/V loads are in flight: one kernel boundary (~5 us in situ) less per layer.
// NW = waves per (row, head): 8 for up to ~2k workgroups (16 waves per CU keep > 12 MB in flight chip-wide); 2 when there
// are many more (row, head) pairs than CUs (multi-channel / large batches), where 512-thread workgroups with a few keys
// each only add dispatch rounds.
// (Two rows per workgroup sharing the head's projection weights -- half the weight reads from L2 -- was measured twice and is
// slower: with 512 threads, 10.2 vs 8.7 us, eight waves per CU keep too little of the K/V stream in flight
// (profiles/r01_step_stamps.txt); with 1024 threads, one workgroup per CU puts both rows' projections and streams in lockstep behind
// the same barriers, +1.4 us per cross-attention launch, and the folded self-attention gains nothing end to end (profiles/r02_two_rows*.txt).)
// OP (O-projection partials; 8 waves only).  SELF: the kernel ends with its head's share of the output projection,
// opart[r][h][:] = R(o) . wo[:, 64h..64h+64)^T -- the same two chained MFMAs over the same 64 k as wave h of the DG_RESID kernel, so
// the values are that kernel's split-K partials bit for bit; the 64 weight rows x 128 B of every wave come in by LDS DMA issued
// before the K/V stream (L2 hits, no registers) and sit in LDS until the tail.  FUSEQ cross-attention: the residual row is
// h + (p0 + ... + p7), summed in wave order as DG_RESID's reduction does, and sum(x^2) is rebuilt with DG_RESID's tree
// (pairs, then the 16-column tiles) followed by the 32-tile wave sum the ssq consumers use: one launch less per layer, same bits.
// PAIR (dec_attn_pair_kernel below: a layer's self- and cross-attention as one launch): 1 = the self-attention half -- its
// O-projection partials leave at agent scope, the caller signals the row; 2 = the cross-attention half -- it requests everything that
// does not depend on the self-attention (its head's wq, the residual row, its K/V block), THEN waits for the row's eight heads and
// reads their partials at agent scope.
struct PairSync {
    unsigned* rows;             // [R][2] lines of CHAIN_LINE words: arrivals, departures (the eighth to leave zeroes both)
    unsigned* abort_word;       // the handle's sticky abort word (shared with the GEMM chain)
    unsigned* host_abort;
};
// Returns (thread 0) the number of heads that had left the row before this one, or ~0u after an abort: the departure count is REQUESTED here, behind
// the barrier, and looked at only at the end of the kernel (pair_leave) -- as a fetch-add whose result thread 0 waited for in front of the barrier it
// put a memory round trip (~0.7 us) on every workgroup's way out of the hand-off.
__device__ __forceinline__ unsigned pair_wait(const PairSync& ps, int r) {
    bool ok = true;
    if (threadIdx.x == 0) {
        unsigned* arr = ps.rows + (size_t)(2 * r) * CHAIN_LINE;
        unsigned long long t0 = 0;
        unsigned polls = 0;
        while (__hip_atomic_load(arr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 8u) {
            if ((++polls & 63u) == 0u) {
                const unsigned long long now = wall_clock64();
                if (t0 == 0) t0 = now;
                if (__hip_atomic_load(ps.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || now - t0 > 100000000ull) {      // 1 s
                    __hip_atomic_store(ps.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (ps.host_abort) __hip_atomic_store(ps.host_abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    ok = false;
                    break;
                }
            }
        }
    }
    __syncthreads();
    unsigned before = ~0u;
    if (threadIdx.x == 0 && ok) before = __hip_atomic_fetch_add(ps.rows + (size_t)(2 * r + 1) * CHAIN_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return before;
}
// the last of the row's eight heads to have left leaves both counters at zero for the next launch
__device__ __forceinline__ void pair_leave(const PairSync& ps, int r, unsigned before) {
    if (threadIdx.x == 0 && before == 7u) {
        unsigned* arr = ps.rows + (size_t)(2 * r) * CHAIN_LINE;
        __hip_atomic_store(arr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(arr + CHAIN_LINE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// BEAM (beam search, self-attention without the folded O-projection only): the history of the beam living in row r is spread over the
// slabs of its group's W rows -- K/V of a position stays where the row that computed it appended it -- and ba.anc says, one byte per
// position, which row of the group holds it.  The row's table is staged in LDS at entry (one 16-byte load per lane, requested together
// with q; n_keys bytes against the 256 * n_keys of K/V the workgroup streams), so a key's slab base costs an LDS read in front of its
// two loads and never a global round trip in front of a K/V block.  Each 8-lane key group already addresses one key per load, so
// only the address changes, not the shape of the stream.  Every table entry is clamped into the group where it is used.
template <bool SELF, bool FUSEQ, int NW, bool OP, int PAIR, bool BEAM = false>
__device__ __forceinline__ void attn_body(const bf16_t* __restrict__ pK, const bf16_t* __restrict__ pV, const bf16_t* __restrict__ pQ,
                                          const float* __restrict__ pF, const void* __restrict__ p4, const void* __restrict__ p5,
                                          unsigned geom0, unsigned geom1, const DecAttnArgs& a, const PairSync& ps, const BeamAttn& ba = BeamAttn{}) {
    static_assert(!BEAM || (SELF && !FUSEQ && !OP && PAIR == 0), "the ancestry table addresses the self-attention cache of the separate launches");
    // Leading scalar arguments (14 dwords; kernarg preload, see dec_gemm_kernel) -- everything the first loads' addresses depend
    // on: K / V slab bases, pQ = q (wq when FUSEQ), pF = the position-bias table (SELF) or the residual stream (FUSEQ),
    // p4 / p5 = loop state and per-row positions (SELF) or norm gain and sum(h^2) partials / O-projection partials (FUSEQ),
    // geom0 = row0 | rows_per_kv << 16 | H << 24, geom1 = slab_keys | n_keys_const << 20.
    unsigned long long t_entry = 0;
    if constexpr (PAIR == 1) t_entry = wall_clock64();          // measurement: stored with the entry stamp, behind the first loads
    // Laggard first: a workgroup's waves run the whole self-attention half, up to the row's signal, at raised priority, so that on a CU whose
    // two workgroups are in different halves the one still on its way to the hand-off -- the one seven other heads may be waiting for -- issues
    // ahead of the one already in its cross-attention half.  Back to 0 right behind the arrival (below), in front of the projection loads
    // and pair_wait.  A scalar instruction, no lane guard.  230.0 -> 222.3 ms per batch; raised only from "self stream consumed" on:
    // 225.8 ms (profiles/pair_request_order_ab.txt).
    if constexpr (PAIR == 1) __builtin_amdgcn_s_setprio(1);
    const int row0 = geom0 & 0xffff, rows_per_kv = (geom0 >> 16) & 0xff, H = geom0 >> 24;
    const int slab_keys = geom1 & 0xfffff, n_keys_const = geom1 >> 20;
    const DecodeShared* pShared = static_cast<const DecodeShared*>(p4);
    const int* pRowPos = static_cast<const int*>(p5);
    const float* pGain = static_cast<const float*>(p4);
    const float* pPart = static_cast<const float*>(p5);
    static_assert(!OP || NW == 8, "the folded O-projection maps wave w to output columns [64w, 64w + 64)");
    __shared__ float sm[NW], sl[NW], sacc[NW][DKV];
    __shared__ __attribute__((aligned(16))) float xs[FUSEQ ? 512 : 4];
    __shared__ __attribute__((aligned(16))) bf16_t qs[DKV];
    __shared__ float s_scale;
    __shared__ float s_tile[OP && FUSEQ ? SSQ_TILES : 1];
    extern __shared__ __attribute__((aligned(1024))) char wo_lds[];      // OP && SELF: [8 waves][64 rows][128 B], chunks XOR-swizzled by row
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = lane & 7, kg = lane >> 3;
    const int r = row0 + blockIdx.x / H, h = blockIdx.x % H;      // (a row's eight heads on one XCD instead -- block -> row 8 * (b / 64) + b % 8 -- measured 1 % slower)
    const int n_keys = SELF ? (pRowPos ? pRowPos[r] : pShared->step) + 1 : n_keys_const;
    const int kv_row = BEAM ? r - r % ba.W : r / rows_per_kv;               // BEAM: the group's first row; a key adds its holder's row pitch
    const size_t slab = ((size_t)kv_row * H + h) * slab_keys * DKV;
    const size_t row_pitch = (size_t)H * slab_keys * DKV;
    const unsigned char* anc_s = reinterpret_cast<const unsigned char*>(wo_lds);       // BEAM: [n_keys] staged table (the dynamic LDS block)
    const bf16_t* kb = pK + slab + sub * 8;
    const bf16_t* vb = pV + slab + sub * 8;
    const float* bias = SELF ? pF + (size_t)h * slab_keys : nullptr;      // the bias table's row pitch is the cache length (launcher checks)
    // OP && SELF: this wave's 64 rows of wo (output columns 64w..64w+63), the head's 64 k each: 8 DMAs of 8 rows x 128 B.  LDS slot
    // (row, pos) holds source chunk pos ^ (row & 7): the swizzle sits on the source address, the DMA writes linearly.
    // Issued BEHIND the wave's first K/V block (below): at entry, 512 workgroups' 64 KB pulls backed the vector-memory queues up and a
    // wave's first K/V request left up to 5.9 us after entry (profiles/r02_attn_pair_marks.txt); requested when the stream has been consumed
    // instead, they land under the merge and lengthen the tail by more than the head gains (259.5 against 253.9 ms per batch, same file).
    auto issue_wo = [&]() {
        if constexpr (OP && SELF) {
            const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)wo_lds + (unsigned)wave * 8192u;
            const bf16_t* src = a.wo + ((size_t)(wave * 64 + (lane >> 3)) * H + h) * DKV + ((lane & 7) ^ (lane >> 3)) * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) glds16(src + (size_t)i * 8 * H * DKV, lds0 + (unsigned)i * 1024u);
        }
    };

    // q stays packed (4 x bf16x2); halves are widened to fp32 at use
    u32x4 qp;
    u32x4 wq_v[FUSEQ ? 8 : 1];
    float x_v = 0.f, g_v = 0.f, ss = 0.f;
    float pv[OP && FUSEQ ? 8 : 1];
    unsigned left_before = ~0u;                 // PAIR == 2: pair_wait's departure count (thread 0)
    auto load_proj = [&]() {
        // operands of the fused projection: wave w owns outputs 8w..8w+7, lane l the k-chunk 8l..8l+7
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
            wq_v[jj] = *reinterpret_cast<const u32x4*>(pQ + ((size_t)h * DKV + wave * 8 + jj) * 512 + lane * 8);
        x_v = pF[(size_t)r * 512 + tid];
        g_v = pGain[tid];
    };
    if constexpr (FUSEQ) {
        if constexpr (PAIR != 2) load_proj();
        if constexpr (OP) {
            if constexpr (PAIR != 2) {
#pragma unroll
                for (int w = 0; w < 8; ++w) pv[w] = pPart[((size_t)r * H + w) * 512 + tid];
            }
        } else {
            if (tid < SSQ_TILES) ss = pPart[(size_t)tid * a.ssq_stride + r];
        }
    } else {
        qp = *reinterpret_cast<const u32x4*>(pQ + ((size_t)r * H + h) * DKV + sub * 8);
    }
    if constexpr (BEAM) {
        // the buffer of the position being decoded (n_keys - 1); rows are anc_pitch (a multiple of 16, > max_decode_len) bytes apart
        const uint8_t* tab = ba.anc + ((size_t)((n_keys - 1) & 1) * ba.anc_rows + r) * ba.anc_pitch;
        for (int i = tid * 16; i < n_keys; i += 64 * NW * 16)
            *reinterpret_cast<u32x4*>(wo_lds + i) = *reinterpret_cast<const u32x4*>(tab + i);
        __syncthreads();
    }

    float m = -1.0e30f, l = 0.f, acc[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = 0.f;
    if constexpr (PAIR != 2) STAMP_IN(a);      // (reads a.stamp from the kernarg segment: behind the first loads, not in front of them)
    if constexpr (PAIR == 1) PAIR_MARK(a, 0, t_entry);

    // The self-attention cache (up to 805 MB) is read exactly once per step: non-temporal loads keep it
    // from evicting the weights (42 MB) and the cross-attention K/V (201 MB at 64 segments), both
    // re-read every step, out of the 256 MB Infinity Cache.  Up to 12 x 16-byte loads in flight per lane.
    constexpr int U = SELF ? 6 : 4;            // self: 12 loads in flight per lane (8 would spill at 128 VGPRs); cross: 8 x 8 x 4 = 256 frames in one shot
    // Every load of a block -- K, V and the position-bias values -- is issued in STRAIGHT-LINE code, keys beyond n_keys
    // clamped to the wave's first key and masked in the math: with the loads behind `if (u < nblk)` branches hipcc's
    // wait-count pass merges the paths and waits for the oldest load with the count of the path that issued the fewest
    // (vmcnt(1): the whole block), and each bias value became its own load + vmcnt(0) round trip in the score loop.
    // A partly filled block (FULL == false) comes in two forms.  nv_tag = 0: all U sub-blocks are loaded and run, each masked by key.
    // nv_tag = NV in 1..U (the self-attention stream's last block, see `tail` below): only the NV sub-blocks that hold a key of this wave --
    // the wave's first key of sub-block u is valid for u < NV and for no other u, so sub-blocks below NV - 1 are whole and only the
    // last one keeps its per-lane mask.  A sub-block left out contributed p = 0 to l and to every accumulator and had no part in the
    // maximum: the same bits (but for the sign of an accumulator that is exactly -0), and still one straight-line path per NV.
    auto load_block = [&](u32x4 (&ku)[U], u32x4 (&vu)[U], bool (&ok)[U], float (&bv)[U], int kw, auto full_tag, auto nv_tag) {
        constexpr bool FULL = decltype(full_tag)::value;         // FULL: all U blocks valid, no masks
        constexpr int NVT = decltype(nv_tag)::value, NV = NVT ? NVT : U;
        static_assert(NVT >= 0 && NVT <= U && !(FULL && NVT), "sub-block count of a partly filled block");
        const int k0 = kw + kg;
        int holder[BEAM ? U : 1];                                // BEAM: the block's table entries, read together in front of its loads
        if constexpr (BEAM) {
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int key = k0 + 8 * NW * u;
                holder[u] = anc_s[FULL || key < n_keys ? key : kw];
            }
        }
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int key = k0 + 8 * NW * u;
            ok[u] = FULL || (NVT && u < NV - 1) || key < n_keys;
            const int kc = ok[u] ? key : kw;
            if constexpr (BEAM) {
                const size_t at = (size_t)min(holder[u], ba.W - 1) * row_pitch + (size_t)kc * DKV;
                ku[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + at));
                vu[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + at));
            } else if constexpr (SELF) {
                ku[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + (size_t)kc * DKV));
                vu[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + (size_t)kc * DKV));
            } else {
                ku[u] = *reinterpret_cast<const u32x4*>(kb + (size_t)kc * DKV);
                vu[u] = *reinterpret_cast<const u32x4*>(vb + (size_t)kc * DKV);
            }
        }
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            if constexpr (SELF) bv[u] = bias[ok[u] ? n_keys - 1 - (k0 + 8 * NW * u) : 0];
            else bv[u] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);                       // every load of the block is in flight before any math waits
    };
    auto compute_block = [&](u32x4 (&ku)[U], u32x4 (&vu)[U], bool (&ok)[U], float (&bv)[U], auto full_tag, auto nv_tag) {
        constexpr int NV = decltype(nv_tag)::value ? decltype(nv_tag)::value : U;
        float sc[U];
        float mn = m;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            {
                float s = 0.f;
                // plain fp32 FMAs on the unpacked halves: v_dot2c_f32_bf16 chains gave O(1) wrong scores on
                // gfx950 / ROCm 7.2 in this kernel (bisected on hardware), so the packed dot is not used
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s = fmaf(__uint_as_float(qp[j] << 16), __uint_as_float(ku[u][j] << 16), s);
                    s = fmaf(__uint_as_float(qp[j] & 0xffff0000u), __uint_as_float(ku[u][j] & 0xffff0000u), s);
                }
                s = sum8(s);
                if constexpr (SELF) s += bv[u];
                sc[u] = s;
                if (ok[u]) mn = fmaxf(mn, s);
            }
        }
        const float rescale = __expf(m - mn);
        l *= rescale;
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[d] *= rescale;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            {
                const float p = ok[u] ? __expf(sc[u] - mn) : 0.f;
                l += p;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[2 * j] = fmaf(p, __uint_as_float(vu[u][j] << 16), acc[2 * j]);
                    acc[2 * j + 1] = fmaf(p, __uint_as_float(vu[u][j] & 0xffff0000u), acc[2 * j + 1]);
                }
            }
        }
        m = mn;
    };
    u32x4 fku[FUSEQ ? U : 1], fvu[FUSEQ ? U : 1];             // FUSEQ: the first K/V block lives across the projection
    bool fok[FUSEQ ? U : 1];
    float fbv[FUSEQ ? U : 1];
    if constexpr (!FUSEQ) {
        constexpr std::integral_constant<int, 0> every_sub{};
        auto block = [&](int kw, auto full_tag) {                // staging registers scoped to one block
            u32x4 ku[U], vu[U];
            bool ok[U];
            float bv[U];
            load_block(ku, vu, ok, bv, kw, full_tag, every_sub);
            compute_block(ku, vu, ok, bv, full_tag, every_sub);
        };
        int kw = wave * 8;
#if defined(YMT3_PARENT_B)                      // A/B builds of one tree (build.py: flags / lib; selected with YMT3_LIB): the masked form everywhere
        constexpr bool TAIL_NV = false;
#else
        constexpr bool TAIL_NV = SELF && !BEAM;      // (the beam kernels keep the masked form: their table reads sit in front of every sub-block's loads)
#endif
        if constexpr (!TAIL_NV) {
            if constexpr (OP && SELF) {
                // the first block's K/V requests, then the wo DMAs, then its math (the inline-asm DMAs are invisible to hipcc's wait counts: its waits
                // for the block's loads, which are older, do not wait for them until the block's last load is needed)
                if (kw < n_keys) {
                    u32x4 ku[U], vu[U];
                    bool ok[U];
                    float bv[U];
                    if (n_keys - kw >= 8 * NW * U) {
                        load_block(ku, vu, ok, bv, kw, std::true_type{}, every_sub);
                        issue_wo();
                        compute_block(ku, vu, ok, bv, std::true_type{}, every_sub);
                    } else {
                        load_block(ku, vu, ok, bv, kw, std::false_type{}, every_sub);
                        issue_wo();
                        compute_block(ku, vu, ok, bv, std::false_type{}, every_sub);
                    }
                    kw += 8 * NW * U;
                } else {
                    issue_wo();
                }
            }
            for (; kw < n_keys; kw += 8 * NW * U) {      // wave-uniform trip count: waves with no key skip everything
                if (n_keys - kw >= 8 * NW * U) block(kw, std::true_type{});
                else block(kw, std::false_type{});
            }
        } else {
            // Whole blocks, then ONE partly filled block that costs what its keys cost: nv = the sub-blocks in which this wave still has a
            // key (wave-uniform, 1..U), one straight-line instantiation each.  OP: the wo DMAs go behind the wave's first block of K/V
            // requests, whichever form that block takes (see above), or out at once for a wave without keys.
            bool wo_pending = OP && SELF;
            if constexpr (OP && SELF) {
                if (n_keys - kw >= 8 * NW * U) {
                    u32x4 ku[U], vu[U];
                    bool ok[U];
                    float bv[U];
                    load_block(ku, vu, ok, bv, kw, std::true_type{}, every_sub);
                    issue_wo();
                    compute_block(ku, vu, ok, bv, std::true_type{}, every_sub);
                    kw += 8 * NW * U;
                    wo_pending = false;
                }
            }
            for (; n_keys - kw >= 8 * NW * U; kw += 8 * NW * U) block(kw, std::true_type{});
            if (kw < n_keys) {
                auto tail = [&](auto nv_tag) {
                    u32x4 ku[U], vu[U];
                    bool ok[U];
                    float bv[U];
                    load_block(ku, vu, ok, bv, kw, std::false_type{}, nv_tag);
                    if constexpr (OP && SELF) { if (wo_pending) issue_wo(); }
                    compute_block(ku, vu, ok, bv, std::false_type{}, nv_tag);
                };
                static_assert(U == 6 || !TAIL_NV, "one case per sub-block count");
                switch ((n_keys - kw + 8 * NW - 1) / (8 * NW)) {
                    case 1: tail(std::integral_constant<int, 1>{}); break;
                    case 2: tail(std::integral_constant<int, 2>{}); break;
                    case 3: tail(std::integral_constant<int, 3>{}); break;
                    case 4: tail(std::integral_constant<int, 4>{}); break;
                    case 5: tail(std::integral_constant<int, 5>{}); break;
                    default: tail(std::integral_constant<int, U < 6 ? U : 6>{}); break;
                }
            } else if constexpr (OP && SELF) {
                if (wo_pending) issue_wo();
            }
        }
    } else {
        // every wave's projection operands are requested before ANY wave's K/V: the CU returns vector-memory data in request
        // order, so weight lines (L2 hits) queued behind another wave's K/V lines (HBM) reached the projection only after
        // most of the stream had arrived, and the projection ran exposed at the end (+2.7 us, profiles/r01_step_stamps.txt)
        if constexpr (PAIR == 2) {
            // The self-attention half's partial stores are acknowledged (vmcnt(0)), the row is signalled, and only THEN are the projection's own
            // operands requested (10 loads per lane: 8 wq, x, gain).  Round 2 issued them first and signalled behind `s_waitcnt vmcnt(10)` (the
            // stores are older; vector-memory operations retire in issue order) so that the acknowledgement ran under the requests -- but a load
            // instruction waits for room in the CU's vector-memory queue, which the other workgroups' K/V streams keep full, and that wait sat
            // in front of the signal: 245.5 -> 241.6 ms per batch with the order turned round (same box, two builds interleaved,
            // profiles/r03_notes.md).  The K/V block is requested after the hand-off.  Requested before it, a poll (and the partials) came
            // back behind it, in issue
            // order, i.e. only once the whole block had arrived (254.5 ms per batch against 253.9); requested by the self-attention half
            // as soon as its own stream was consumed, it slowed the other workgroups' self-attention streams by more than it gained
            // (263 ms; profiles/r02_attn_pair_marks.txt).  (The pair kernel keeps hipcc from moving memory operations across the
            // boundary between the halves.)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_fetch_add(ps.rows + (size_t)(2 * r) * CHAIN_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            PAIR_MARK(a, 3, wall_clock64());     // row signalled
            __builtin_amdgcn_s_setprio(0);       // (raised at the entry of the self-attention half)
            load_proj();
            __builtin_amdgcn_sched_barrier(0);
            left_before = pair_wait(ps, r);
            PAIR_MARK(a, 4, wall_clock64());     // the row's eight heads have arrived
#pragma unroll
            for (int w = 0; w < 8; ++w) pv[w] = __hip_atomic_load(pPart + ((size_t)r * H + w) * 512 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            __builtin_amdgcn_s_barrier();
        }
    }
    if constexpr (FUSEQ) {
        // first (for T <= 256: only) K/V block goes in flight now; its math waits for the projection below.  STRAIGHT-LINE
        // code, keys beyond n_keys clamped to key 0 of the slab: behind a branch hipcc merges the two paths' load counts and
        // waits for the projection operands with the count of the path that issued no K/V loads -- i.e. for (almost) the
        // whole K/V stream, which put the projection after the stream instead of under it
        const int k0 = wave * 8 + kg;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int key = k0 + 8 * NW * u;
            fok[u] = key < n_keys;
            fbv[u] = 0.f;
            const int kc = fok[u] ? key : 0;
            fku[u] = *reinterpret_cast<const u32x4*>(kb + (size_t)kc * DKV);
            fvu[u] = *reinterpret_cast<const u32x4*>(vb + (size_t)kc * DKV);
        }
    }
    if constexpr (FUSEQ) {
        if constexpr (OP) {
            // x = h + (p0 + p1 + ... + p7), then DG_RESID's sum(x^2) tree: (x_even^2 + x_odd^2), the 8 pairs of a 16-column
            // tile by xor 1, 2, 4 -- mul_sep / add_sep: the epilogue this mirrors multiplies (v_pk_mul) and adds, never an fma
            float sp = pv[0];
#pragma unroll
            for (int w = 1; w < 8; ++w) sp += pv[w];
            x_v += sp;
            float q2 = mul_sep(x_v, x_v);
            q2 = add_sep(q2, DPP_F(q2, 0xB1));        // lane ^ 1
            q2 = add_sep(q2, DPP_F(q2, 0x4E));        // lane ^ 2
            q2 = add_sep(q2, DPP_F(q2, 0x141));       // row_half_mirror: a lane of the other quad, which holds what lane ^ 4 holds
            q2 = add_sep(q2, DPP_F(q2, 0x128));       // row_ror:8 = lane ^ 8 within the row of 16
            if ((tid & 15) == 0) s_tile[tid >> 4] = q2;
            __syncthreads();
            ss = lane < SSQ_TILES ? s_tile[lane] : 0.f;              // every wave sums the 32 tiles itself: no broadcast of the scale, one barrier less
        }
        // norm scale (fixed-order tree over the 32 partials), normed row -> LDS as bf16-rounded floats
        ss = wave_sum(ss);
        float scale;
        if constexpr (OP) {
            scale = rsqrtf(ss / 512.f + a.eps);
        } else {                                                     // the carried partials were loaded by the first 32 threads only
            if (tid == 0) s_scale = rsqrtf(ss / 512.f + a.eps);
            __syncthreads();
            scale = s_scale;
        }
        xs[tid] = bf2f(f2bf(x_v * scale * g_v));
        __syncthreads();
        float xn[8];
        *reinterpret_cast<float4*>(xn) = *reinterpret_cast<const float4*>(xs + lane * 8);
        *reinterpret_cast<float4*>(xn + 4) = *reinterpret_cast<const float4*>(xs + lane * 8 + 4);
        float dd[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d = fmaf(xn[2 * j], __uint_as_float(wq_v[jj][j] << 16), d);
                d = fmaf(xn[2 * j + 1], __uint_as_float(wq_v[jj][j] & 0xffff0000u), d);
            }
            d = sum8(d);
            d += DPP_F(d, 0x128);                                 // row_ror:8 -> lane ^ 8 within the row of 16
            dd[jj] = d;
        }
        // Every lane of a 16-lane row now holds its row's sum r0..r3.  The wave total is (r0 + r1) + (r2 + r3) -- what two butterfly steps
        // (lane ^ 16, lane ^ 32) gave every lane, through the LDS crossbar, sixteen dependent round trips for the eight outputs (0.8 us on
        // the critical path).  Row broadcasts (DPP) add the same pairs with the operands swapped -- IEEE addition commutes, same bits --
        // and leave the total in row 3.
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) dd[jj] += DPP_ROWS(dd[jj], 0x142, 0xA);       // row_bcast:15 -> rows 1 and 3: r1 + r0, r3 + r2
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) dd[jj] += DPP_ROWS(dd[jj], 0x143, 0xC);       // row_bcast:31 -> row 3: (r3 + r2) + (r1 + r0)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
            if (lane == 56 + jj) qs[wave * 8 + jj] = f2bf(dd[jj]);
        __syncthreads();
        qp = *reinterpret_cast<const u32x4*>(qs + sub * 8);
        // the block loaded above, then the remaining ones
        for (int kw = wave * 8; kw < n_keys; kw += 8 * NW * U) {
            if (kw != wave * 8) load_block(fku, fvu, fok, fbv, kw, std::false_type{}, std::integral_constant<int, 0>{});
            compute_block(fku, fvu, fok, fbv, std::false_type{}, std::integral_constant<int, 0>{});
        }
    }
    if constexpr (PAIR == 1) PAIR_MARK(a, 1, wall_clock64());     // self-attention stream consumed
    if constexpr (PAIR == 2) PAIR_MARK(a, 5, wall_clock64());     // cross-attention block consumed
    // merge the 8 key groups of the wave (lanes with equal `sub`)
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
        const float mo = lane_xor(m, off), lo = lane_xor(l, off);      // (register moves, not the LDS crossbar: common.h)
        const float mn = fmaxf(m, mo);
        const float sa = __expf(m - mn), sb = __expf(mo - mn);
        l = l * sa + lo * sb;
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[d] = acc[d] * sa + lane_xor(acc[d], off) * sb;
        m = mn;
    }
    if (kg == 0) {
#pragma unroll
        for (int d = 0; d < 8; ++d) sacc[wave][sub * 8 + d] = acc[d];
        if (sub == 0) { sm[wave] = m; sl[wave] = l; }
    }
    __syncthreads();
    if (tid < DKV) {
        float M = sm[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) M = fmaxf(M, sm[w]);
        float L = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float e = __expf(sm[w] - M);
            L += sl[w] * e;
            o += sacc[w][tid] * e;
        }
        if constexpr (OP && SELF) qs[tid] = f2bf(o / L);        // the projection's operand; nobody reads a.out in this mode
        else a.out[((size_t)r * H + h) * DKV + tid] = f2bf(o / L);
    }
    if constexpr (OP && SELF) {
        __syncthreads();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's own wo rows have landed (nobody else reads them)
        const int li = lane & 15, g = lane >> 4;
        const char* strip = wo_lds + wave * 8192;
        f32x4 pa[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) pa[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            // activation operand: row 0 of the 16-row tile is (r, h)'s output, rows 1..15 are zero (their results are not stored)
            bf16x8 af = *reinterpret_cast<const bf16x8*>(qs + ks * 32 + g * 8);
            if (li != 0) af = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int row = c * 16 + li;
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(strip + row * 128 + (((ks * 4 + g) ^ (row & 7)) * 16));
                pa[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, pa[c], 0, 0, 0);
            }
        }
        if (li == 0) {
            float* dst = a.opart + ((size_t)r * H + h) * 512 + wave * 64 + g * 4;
            if constexpr (PAIR == 1) {           // read by the row's other heads, on other XCDs, later in this launch: agent scope (aux 16 = sc1)
                const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.opart, 0, 0x7fffffff, 0x00020000);
                const int off = (((r * H + h) * 512) + wave * 64 + g * 4) * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pa[c]), ro, off + c * 64, 0, 16);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) *reinterpret_cast<float4*>(dst + c * 16) = make_float4(pa[c][0], pa[c][1], pa[c][2], pa[c][3]);
            }
        }
    }
    if constexpr (FUSEQ) {
        if (a.chain_sync && blockIdx.x == 0 && tid < CHAIN_COUNTERS) a.chain_sync[tid * CHAIN_LINE] = 0u;      // the next launch's arrival counters (dec_chain.hip)
    }
    if constexpr (PAIR == 1) PAIR_MARK(a, 2, wall_clock64());     // O-projection partial stored
    if constexpr (PAIR == 2) pair_leave(ps, r, left_before);
    if constexpr (PAIR != 1) STAMP_OUT(a);
}

template <bool SELF, bool FUSEQ, int NW, bool OP = false>
__global__ __launch_bounds__(64 * NW, 4) void dec_attn_kernel(const bf16_t* __restrict__ pK, const bf16_t* __restrict__ pV, const bf16_t* __restrict__ pQ,
                                                              const float* __restrict__ pF, const void* __restrict__ p4, const void* __restrict__ p5,
                                                              unsigned geom0, unsigned geom1, DecAttnArgs a) {   // 4 waves / SIMD -> <= 128 VGPRs
    attn_body<SELF, FUSEQ, NW, OP, 0>(pK, pV, pQ, pF, p4, p5, geom0, geom1, a, PairSync{});
}

// beam search: self-attention through the ancestry table (8 waves, or 2 per (row, head) for many rows)
template <int NW>
__global__ __launch_bounds__(64 * NW, 4) void dec_attn_beam_kernel(const bf16_t* __restrict__ pK, const bf16_t* __restrict__ pV, const bf16_t* __restrict__ pQ,
                                                                   const float* __restrict__ pF, const void* __restrict__ p4, const void* __restrict__ p5,
                                                                   unsigned geom0, unsigned geom1, DecAttnArgs a, BeamAttn ba) {
    attn_body<true, false, NW, false, 0, true>(pK, pV, pQ, pF, p4, p5, geom0, geom1, a, PairSync{}, ba);
}

// A layer's self-attention and cross-attention as ONE launch (up to 64 rows: 512 workgroups, two per CU, all resident).  Workgroup
// (row, head) streams its self-attention slab and leaves its O-projection partial (the folded form above), signals the row, requests
// its cross-attention operands, waits for the row's eight heads and goes on as the fused cross-attention.  What that saves is the
// launch gap and the cross-attention's start-up: its K/V stream is requested ~1 us after the self-attention's last bytes instead of
// after a kernel boundary and a dispatch ramp.  Same arithmetic as the two launches, bit for bit.
__global__ __launch_bounds__(512, 4) void dec_attn_pair_kernel(const bf16_t* __restrict__ pK, const bf16_t* __restrict__ pV, const bf16_t* __restrict__ pQ,
                                                               const float* __restrict__ pF, const void* __restrict__ p4, const void* __restrict__ p5,
                                                               unsigned geom0, unsigned geom1, DecAttnArgs a, DecAttnArgs b, unsigned gb0, unsigned gb1,
                                                               PairSync ps) {
    attn_body<true, false, 8, true, 1>(pK, pV, pQ, pF, p4, p5, geom0, geom1, a, ps);
    // the second half counts its loads against the first half's stores (see PAIR == 2): nothing may cross this line
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    attn_body<false, true, 8, true, 2>(b.k, b.v, b.wq, b.x_f32, b.gain, b.ipart, gb0, gb1, b, ps);
}

// ------------------------------------------------------------------------------------------------
// h[r] = embed row (+ channel row); sum(h^2) goes to ssq tile 0 of the row, tiles 1.. are zeroed
__device__ __forceinline__ void embed_row(const ArgmaxArgs& a, int r, const bf16_t* e, const bf16_t* c, float* scratch4) {
    const int tid = threadIdx.x;
    float q = 0.f;
    for (int i = tid; i < a.d; i += 256) {
        const float v = bf2f(e[i]) + (c ? bf2f(c[i]) : 0.f);
        a.h[(size_t)r * a.d + i] = v;
        q += v * v;
    }
    q = wave_sum(q);
    __syncthreads();                       // scratch4 may still be read by the caller's previous phase
    if ((tid & 63) == 0) scratch4[tid >> 6] = q;
    __syncthreads();
    if (tid < SSQ_TILES) a.ssq[(size_t)tid * a.ssq_stride + r] = tid == 0 ? (scratch4[0] + scratch4[1]) + (scratch4[2] + scratch4[3]) : 0.f;
}

// Layer 0's QKV projection as a gather (ArgmaxArgs::qkv0): thread i < 192 carries 16 bytes (8 columns) of the fed id's table row.
// Everything but the fed id and the position is known at entry, so a thread's share of both addresses is formed there (under the logits
// loads in the argmax kernel) and kept in VGPRs: the table's five scalar arguments held in SGPRs to the end of the kernel cost
// argmax_embed_kernel its 8th wave per SIMD (106 SGPRs), as the constraint's mask row once did.
struct Qkv0Lane {
    const bf16_t* src;          // qkv0 + this thread's 8 columns, or null: no table / no chunk for this thread
    bf16_t* dst;                // columns [0, 512): q of row r; then k and v of head (n % 512) / 64 at cache position 0 (dec_gemm_kernel's epilogue)
    int pos_stride, L;          // elements per cache position (0 for q), cache length
};
__device__ __forceinline__ Qkv0Lane qkv0_lane(const ArgmaxArgs& a, int r) {
    Qkv0Lane q{nullptr, nullptr, 0, 0};
    if (a.qkv0 && threadIdx.x < QKV0_COLS / 8) {
        constexpr int inner = QKV0_COLS / 3, H = inner / DKV;
        const int n = threadIdx.x * 8, nn = n - inner;
        q.src = a.qkv0 + n;
        q.L = a.L;
        if (n < inner) {
            q.dst = a.q0 + (size_t)r * inner + n;
        } else {
            q.dst = (nn / inner ? a.vcache0 : a.kcache0) + ((size_t)r * H + ((nn % inner) >> 6)) * a.L * DKV + (nn & 63);
            q.pos_stride = DKV;
        }
    }
    asm volatile("" : "+v"(q.src), "+v"(q.dst), "+v"(q.pos_stride), "+v"(q.L));
    return q;
}
// the load is requested in front of embed_row's loads (one round trip for both); the store follows them
__device__ __forceinline__ u32x4 qkv0_load(const Qkv0Lane& q, int feed) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (q.src) v = *reinterpret_cast<const u32x4*>(q.src + (size_t)feed * QKV0_COLS);
    return v;
}
// nothing goes to position L, past the (row, head) slab: the last position of a full-length decode has no next step, and the launch never ran after it
__device__ __forceinline__ void qkv0_store(const Qkv0Lane& q, int pos, const u32x4& v) {
    if (q.src && (pos < q.L || q.pos_stride == 0)) *reinterpret_cast<u32x4*>(q.dst + (size_t)pos * q.pos_stride) = v;
}

__global__ __launch_bounds__(256) void argmax_embed_kernel(const float* __restrict__ pLogits, DecodeShared* pShared, int* pFinished, int* pRowPos,
                                                           const long long* __restrict__ pRowOut, const bf16_t* __restrict__ pEmbed, int row0, int V,
                                                           ArgmaxArgs a) {
    // leading scalar arguments: kernarg preload (see dec_gemm_kernel)
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int s_feed;
    __shared__ int s_pos;                  // slot mode: the row's position after this step (where layer 0's k / v of the fed id go)
    __shared__ float s_sum[4];             // the score pass's wave partials (sv is embed_row's scratch by then)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = row0 + blockIdx.x;
    DecodeShared* sh = pShared;
    // col: emitted index within this call; the first n_prompt steps (col < 0) feed prompt ids and emit nothing
    const int t = sh->step, n_steps = sh->n_steps, n_prompt = sh->n_prompt, col = t - sh->step0 - n_prompt;
    const float* row = pLogits + (size_t)r * V;
    // everything thread 0 needs after the argmax is requested now (workgroup-uniform addresses), under the logits loads,
    // instead of as a chain of round trips behind them
    int32_t* const tokens_out = sh->tokens_out;
    const int32_t* const forced = sh->forced;
    float* const logits_out = sh->logits_out;
    const int32_t* const prompt = sh->prompt;
    // (unconditionally, with the other pointers: with scores and constraints off these loads are the only change to the kernel;
    // the rest of a constraint is read where it is used, under it)
    float* const scores_out = sh->scores_out;
    const uint32_t* const c_allowed = sh->c_allowed;
    const int was_finished = pFinished[r];
    const int forced_tok = forced && col >= 0 ? forced[(size_t)r * n_steps + col] : 0;
    // (a prompt id is read by thread 0 behind the argmax, at prompt positions only.  Requested here, its conditional load split
    // this block, the kernel-argument loads moved behind it and every step's argmax waited for pFinished first: the whole
    // decode ran ~1 ms per 1024-step batch slower)
    const int pos0 = pRowPos ? pRowPos[r] : 0;
    const long long out0 = pRowPos ? pRowOut[r] : 0;
    const Qkv0Lane ql = qkv0_lane(a, r);

    STAMP_IN(a);
    // A row in which no logit compares greater than -3.4e38 (all NaN, all -inf) emits the lowest index, as a tie does: every
    // thread starts from index 0, and NaN logits take no part anywhere (include/ymt3.h, non-finite values).
    float bv = -3.4e38f;
    int bi = 0;
    for (int i = tid; i < V; i += 256) {
        const float v = row[i];
        if (v > bv) { bv = v; bi = i; }       // ascending i: the first maximum is kept
    }
    // Constrained: the scan again (the row is in cache by now) over the tokens the row's state allows.  Behind the plain scan,
    // which thus waits on no load of the constraint's pointers: the unconstrained kernel issues its logits loads as before.
    int state = 0;
    const uint32_t* mrow = nullptr;
    if (c_allowed) {
        state = a.row_state[r];              // (workgroup-uniform; seeded by decode_init / slot_start)
        asm volatile("" : "+v"(state));      // kept in a VGPR: in SGPRs the mask row's address cost the kernel its 8th wave per SIMD
        mrow = c_allowed + (size_t)state * sh->c_words;
        bv = -3.4e38f;
        bi = 0x7fffffff;
        for (int i = tid; i < V; i += 256) {
            const float v = row[i];
            if ((mrow[i >> 5] >> (i & 31)) & 1u) {                                   // disallowed tokens take no part
                if (v > bv) { bv = v; bi = i; }
                else bi = min(bi, i);          // (ascending i: only the start value moves) no comparable logit: the lowest allowed index
            }
        }
    }
    // wave-wide (max value, lowest index): the selection is commutative and associative, so any reduction order gives the same pair.
    // Rotations inside the 16-lane rows, then row broadcasts (all DPP; twelve dependent ds_bpermute round trips before): row 3 ends up
    // with the wave's pair.
#define ARGMAX_TAKE(ctrl, rows, cond)                                                                                      \
    do {                                                                                                                  \
        const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, bv), (ctrl), (rows), 0xF, false)); \
        const int oi = __builtin_amdgcn_update_dpp(0, bi, (ctrl), (rows), 0xF, false);                                    \
        if ((cond) && (ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }                                           \
    } while (0)
    ARGMAX_TAKE(0x128, 0xF, true);            // row_ror:8
    ARGMAX_TAKE(0x124, 0xF, true);            // row_ror:4
    ARGMAX_TAKE(0x122, 0xF, true);            // row_ror:2
    ARGMAX_TAKE(0x121, 0xF, true);            // row_ror:1: every lane holds its row's pair
    ARGMAX_TAKE(0x142, 0xA, (lane & 16) != 0);    // row_bcast:15 -> rows 1 and 3
    ARGMAX_TAKE(0x143, 0xC, lane >= 32);          // row_bcast:31 -> (rows 2 and) 3
#undef ARGMAX_TAKE
    if (lane == 63) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    // score pass: the row maximum is the argmax value, over the allowed tokens under a constraint (every thread takes it now:
    // embed_row reuses sv below)
    const float row_max = scores_out ? fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])) : 0.f;
    long long score_at = -1;               // thread 0: where this step's score goes (-1: nowhere) ...
    int score_id = -1;                     // ... and the id it scores (-1: 0.0, an unforced row after its EOS)
    if (tid == 0) { bv = sv[0]; bi = si[0]; }      // (the wave's pair sits in its last row)
    if (tid == 0 && pRowPos) {
        // slot mode: this row's own position; a stopped row writes nothing and stays where it is (its slot is refilled
        // by the host), a live one stops after EOS or its n_steps-th token
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
        bi = min(bi, V - 1);               // (only a state that allows nothing leaves the start value) no index reaches memory unclamped
        int feed = a.pad_id, pos1 = pos0;
        if (!was_finished && pos0 < n_prompt) {           // a prompt position: feed the prompt id, emit nothing
            pRowPos[r] = pos1 = pos0 + 1;
            feed = prompt[a.row_prompt[r] + pos0];
        } else if (!was_finished) {
            const int p = pos0 - n_prompt;
            tokens_out[out0 + p] = bi;
            if ((a.eos_id >= 0 && bi == a.eos_id) || p + 1 >= n_steps) pFinished[r] = 1;
            else pRowPos[r] = pos1 = pos0 + 1;
            feed = bi;
            score_at = out0 + p;
            score_id = bi;
            if (mrow) a.row_state[r] = sh->c_next[(size_t)state * V + bi];
        }
        s_feed = feed < 0 ? 0 : (feed >= V ? V - 1 : feed);
        s_pos = pos1;
    } else if (tid == 0 && col < 0) {
        // a prompt position: feed the prompt id; no token, no logits, no EOS flag
        const int p = prompt[(size_t)r * n_prompt + (t - sh->step0)];
        s_feed = p < 0 ? 0 : (p >= V ? V - 1 : p);
    } else if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
        int tok = min(bi, V - 1);
        if (a.eos_id >= 0) {
            if (was_finished) tok = a.pad_id;
            else if (tok == a.eos_id) pFinished[r] = 1;
        }
        tokens_out[(size_t)r * n_steps + col] = tok;
        int feed = forced ? forced_tok : tok;
        feed = feed < 0 ? 0 : (feed >= V ? V - 1 : feed);         // caller-supplied ids must not index outside the table
        s_feed = feed;
        score_at = (long long)r * n_steps + col;
        score_id = !forced && a.eos_id >= 0 && was_finished ? -1 : feed;
        if (mrow && !(a.eos_id >= 0 && was_finished)) a.row_state[r] = sh->c_next[(size_t)state * V + feed];   // frozen after EOS
    }
    __syncthreads();
    const int feed = s_feed;
    const int kv_pos = pRowPos ? s_pos : t + 1;        // the position the next step decodes: a stopped row stays where it is
    const u32x4 qkv0 = qkv0_load(ql, feed);
    const bf16_t* e = pEmbed + (size_t)feed * a.d;
    const bf16_t* c = a.chan_embed ? a.chan_embed + (size_t)(r % a.n_channels) * a.d : nullptr;
    embed_row(a, r, e, c, sv);
    qkv0_store(ql, kv_pos, qkv0);
    if (logits_out && !pRowPos && col >= 0) {
        float* dst = logits_out + ((size_t)r * n_steps + col) * V;
        for (int i = tid; i < V; i += 256) dst[i] = row[i];
    }
    if (scores_out) {
        // log-sum-exp of the row the argmax read (still in cache): per-thread partials, the wave butterfly, the 4 waves below
        float q = 0.f;
        if (mrow) {
            for (int i = tid; i < V; i += 256)
                if ((mrow[i >> 5] >> (i & 31)) & 1u) q += __expf(row[i] - row_max);         // disallowed: exp(-inf) = 0
        } else {
            for (int i = tid; i < V; i += 256) q += __expf(row[i] - row_max);
        }
        q = wave_sum(q);
        if (lane == 0) s_sum[wave] = q;
    }
    // the per-step kernel's arrival counters (dec_step.hip), left at zero for the next step's launch
    if (a.zero_sync)
        for (int i = blockIdx.x * 256 + tid; i < a.zero_lines; i += gridDim.x * 256) a.zero_sync[(size_t)i * CHAIN_LINE] = 0u;
    // the last workgroup to finish advances the position; every workgroup has read `t` by then
    __syncthreads();
    if (tid == 0) {
        if (scores_out && score_at >= 0)           // (the barrier above also published s_sum)
            scores_out[score_at] = score_id < 0 ? 0.f
                                 : mrow && !((mrow[score_id >> 5] >> (score_id & 31)) & 1u) ? -__builtin_inff()   // a forced disallowed id
                                 : (row[score_id] - row_max) - __logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
        if (a.eos_id >= 0) __threadfence();      // only the flags the last arriver counts below need to be visible to it
        // Who is last?  One atomic per workgroup on ONE word serialises at the memory side (~12 ns each: 10 us of the 13-channel decoder's
        // 832 workgroups); beyond 64 workgroups groups of 32 count on lines of their own and only each group's last one takes the shared ticket.
        bool last;
        if (a.ticket && gridDim.x > 64) {
            const int grp = blockIdx.x >> 5, n_grp = ((int)gridDim.x + 31) >> 5, in_grp = min(32, (int)gridDim.x - 32 * grp);
            last = false;
            if (atomicAdd(a.ticket + (size_t)grp * CHAIN_LINE, 1u) == (unsigned)(in_grp - 1)) {
                a.ticket[(size_t)grp * CHAIN_LINE] = 0u;
                if (a.eos_id >= 0) __threadfence();
                last = atomicAdd(&sh->done_count, 1) == n_grp - 1;
            }
        } else {
            last = atomicAdd(&sh->done_count, 1) == (int)gridDim.x - 1;
        }
        if (last) {
            sh->done_count = 0;
            sh->step = t + 1;
            if (a.eos_id >= 0) {             // the fence above makes every row's flag visible to this last arriver
                int n = 0;
                for (int i = 0; i < (int)gridDim.x; ++i) n += pFinished[row0 + i] ? 0 : 1;
                sh->n_unfinished = n;
            }
        }
    }
    STAMP_OUT(a);
}

__global__ __launch_bounds__(256) void decode_init_kernel(ArgmaxArgs a, int n_chains, int n_steps, int step0, int32_t* tokens_out,
                                                          const int32_t* forced, float* logits_out, const int32_t* prompt, int n_prompt,
                                                          float* scores_out, ConstraintView cv) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const bf16_t* e = a.embed + (size_t)a.pad_id * a.d;
    const bf16_t* c = a.chan_embed ? a.chan_embed + (size_t)(r % a.n_channels) * a.d : nullptr;
    __shared__ float sv[4];
    const Qkv0Lane ql = qkv0_lane(a, r);
    const u32x4 qkv0 = qkv0_load(ql, a.pad_id);
    embed_row(a, r, e, c, sv);
    qkv0_store(ql, step0, qkv0);
    if (tid == 0) {
        a.finished[r] = 0;
        // the start state, clamped into range like a fed id
        if (a.row_state) a.row_state[r] = cv.start ? min(max(cv.start[r], 0), cv.n_states - 1) : 0;
    }
    if (r == 0 && tid < n_chains) {          // a.shared is the array of per-chain loop states
        DecodeShared* sh = a.shared + tid;
        sh->step = step0;
        sh->step0 = step0;
        sh->done_count = 0;
        sh->n_unfinished = a.R;
        sh->n_steps = n_steps;
        sh->tokens_out = tokens_out;
        sh->forced = forced;
        sh->logits_out = logits_out;
        sh->prompt = prompt;
        sh->n_prompt = n_prompt;
        sh->scores_out = scores_out;
        sh->c_allowed = cv.allowed;
        sh->c_next = cv.next;
        sh->c_words = cv.words;
    }
}

__global__ __launch_bounds__(256) void slot_start_kernel(ArgmaxArgs a, int row0, long long first_out, int n_steps, long long* row_out,
                                                         long long first_prompt, int n_prompt, long long* row_prompt, ConstraintView cv) {
    const int r = row0 + blockIdx.x, tid = threadIdx.x;
    const bf16_t* e = a.embed + (size_t)a.pad_id * a.d;
    const bf16_t* c = a.chan_embed ? a.chan_embed + (size_t)(r % a.n_channels) * a.d : nullptr;
    __shared__ float sv[4];
    const Qkv0Lane ql = qkv0_lane(a, r);
    const u32x4 qkv0 = qkv0_load(ql, a.pad_id);
    embed_row(a, r, e, c, sv);
    qkv0_store(ql, 0, qkv0);
    if (tid == 0) {
        a.finished[r] = 0;
        a.row_pos[r] = 0;
        row_out[r] = first_out + (long long)blockIdx.x * n_steps;
        row_prompt[r] = first_prompt + (long long)blockIdx.x * n_prompt;
        if (a.row_state) a.row_state[r] = cv.start ? min(max(cv.start[blockIdx.x], 0), cv.n_states - 1) : 0;
    }
}

// the layer-0 table build (ymt3_create): row blockIdx.x of the scratch stream = embed[v0 + blockIdx.x], through embed_row as every decode row
__global__ __launch_bounds__(256) void qkv0_embed_kernel(ArgmaxArgs a, int v0) {
    __shared__ float sv[4];
    embed_row(a, blockIdx.x, a.embed + (size_t)(v0 + blockIdx.x) * a.d, nullptr, sv);
}

__global__ void slot_retire_kernel(ArgmaxArgs a, int row0, int n_steps, int n_prompt, int32_t* tokens_out, float* scores_out) {
    const int r = row0 + blockIdx.x;
    const long long o = a.row_out[r];
    for (int i = max(a.row_pos[r] + 1 - n_prompt, 0) + threadIdx.x; i < n_steps; i += blockDim.x) {
        tokens_out[o + i] = a.pad_id;
        if (scores_out) scores_out[o + i] = 0.f;
    }
}

__global__ void pad_tail_kernel(int32_t* tokens_out, float* scores_out, int row0, int n_steps, int from, int pad_id) {
    const size_t o = (size_t)(row0 + blockIdx.x) * n_steps;
    for (int i = from + threadIdx.x; i < n_steps; i += blockDim.x) {
        tokens_out[o + i] = pad_id;
        if (scores_out) scores_out[o + i] = 0.f;
    }
}

template <int MODE, int K, int NT, bool PEND = false>
constexpr size_t dg_lds_bytes() {
    return (size_t)(8 * 16 * 16 * NT + 16 + (PEND ? 8 * 16 : 0)) * 4 + (size_t)8 * (1 + NT) * 16 * (K / 8 * 2 + 16);
}

template <int MODE, int K, int NT = 1, bool PEND = false>
int launch_dg(const DecGemmArgs& a, hipStream_t stream) {
    if (a.W == nullptr)     // attribute-only call from init_decode_kernels(): > 64 KB of dynamic LDS needs opting in
        return hipFuncSetAttribute(reinterpret_cast<const void*>(dec_gemm_kernel<MODE, K, NT, PEND>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)dg_lds_bytes<MODE, K, NT, PEND>()) == hipSuccess ? 0 : -2;
    if (MODE == DG_RESID && a.N != 16 * SSQ_TILES) return -3;   // the norm consumers sum exactly SSQ_TILES partials
    if (PEND && (!a.pend_y || (MODE == DG_NORM_QKV_CACHE && !a.h_out))) return -4;
    dec_gemm_kernel<MODE, K, NT, PEND><<<(a.N / (16 * NT)) * ((a.R + 15) / 16), 512, dg_lds_bytes<MODE, K, NT, PEND>(), stream>>>(
        a.W, MODE == DG_RESID ? static_cast<const void*>(a.a_bf16) : static_cast<const void*>(a.x_f32), a.gain, a.ssq, a.out_f32, a.row0, a.R, a.N,
        a.ssq_stride, a);
    return 0;
}

// wide projections: 32 columns per workgroup once 16-column tiles would put more than one workgroup on a CU
template <int MODE, bool PEND = false>
int launch_dg_wide(const DecGemmArgs& a, hipStream_t stream) {
    static const bool narrow = getenv("YMT3_DEC_GEMM_NARROW") != nullptr;      // A/B timing only
    const int wgs16 = (a.N / 16) * ((a.R + 15) / 16);
    if (!narrow && a.N % 32 == 0 && wgs16 > 320) return launch_dg<MODE, 512, 2, PEND>(a, stream);
    return launch_dg<MODE, 512, 1, PEND>(a, stream);
}

}  // namespace

int init_decode_kernels() {
    DecGemmArgs z{};
    int rc = 0;
    rc |= launch_dg<DG_RESID, 512>(z, nullptr);
    rc |= launch_dg<DG_RESID, 1024>(z, nullptr);
    rc |= launch_dg<DG_RESID, 2048>(z, nullptr);
    rc |= launch_dg<DG_NORM_QKV_CACHE, 512>(z, nullptr);
    rc |= launch_dg<DG_NORM_BF16, 512>(z, nullptr);
    rc |= launch_dg<DG_NORM_BF16_RELU, 512>(z, nullptr);
    rc |= launch_dg<DG_NORM_LOGITS, 512>(z, nullptr);
    rc |= launch_dg<DG_NORM_QKV_CACHE, 512, 2>(z, nullptr);
    rc |= launch_dg<DG_NORM_BF16, 512, 2>(z, nullptr);
    rc |= launch_dg<DG_NORM_BF16_RELU, 512, 2>(z, nullptr);
    rc |= launch_dg<DG_NORM_LOGITS, 512, 2>(z, nullptr);
    rc |= launch_dg<DG_NORM_QKV_CACHE, 512, 1, true>(z, nullptr);
    rc |= launch_dg<DG_NORM_QKV_CACHE, 512, 2, true>(z, nullptr);
    rc |= launch_dg<DG_NORM_LOGITS, 512, 1, true>(z, nullptr);
    rc |= launch_dg<DG_NORM_LOGITS, 512, 2, true>(z, nullptr);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(dec_attn_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, WO_LDS_BYTES) != hipSuccess) rc |= -2;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(dec_attn_kernel<true, false, 8, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            WO_LDS_BYTES) != hipSuccess) rc |= -2;
    return rc;
}

template <int MODE, int K, int BM>
int launch_dg_mid(const DecGemmArgs& a, hipStream_t stream) {
    if (MODE == DG_RESID && a.N != 16 * SSQ_TILES) return -3;
    constexpr int PF = 4;     // K-steps of operands in flight per thread (8 = all of K = 512 and 2 were measured: profiles/r03_notes.md)
    constexpr int NTH = 256;  // (512 -- two waves per SIMD, half the row tiles each -- was measured: K = 512 forms 0.5 us slower, K = 2048 twice as slow: profiles/r03_notes.md)
    dec_gemm_mid_kernel<MODE, K, BM, PF, NTH><<<(a.N / 64) * ((a.R + BM - 1) / BM), NTH, 0, stream>>>(
        a.W, MODE == DG_RESID ? static_cast<const void*>(a.a_bf16) : static_cast<const void*>(a.x_f32), a.gain, a.ssq, a.out_f32, a.row0, a.R, a.N,
        a.ssq_stride, a);
    return 0;
}

// many rows: the mid-size tile kernel from DEC_GEMM_MID_ROWS rows on (kernels.h; a handle created under YMT3_DEC_GEMM_MID_ROWS=n passes its own
// threshold in DecGemmArgs::mid_rows, 0 = never: A/B timing, and the late-position parity test of the many-row kernels at a few rows)
static int launch_dec_gemm_mid(int mode, const DecGemmArgs& a, hipStream_t stream) {
    if (a.N % 64 || a.part) return -1;
    switch (mode) {
        case DG_RESID:
            if (a.K == 512) return launch_dg_mid<DG_RESID, 512, 32>(a, stream);
            if (a.K == 2048) return launch_dg_mid<DG_RESID, 2048, 32>(a, stream);
            return -1;
        // (32-row tiles for the wide projections too: 154.6 vs 156.4 ms per configs[3] batch -- no difference; 64 stays)
        case DG_NORM_QKV_CACHE: return a.K == 512 ? launch_dg_mid<DG_NORM_QKV_CACHE, 512, 64>(a, stream) : -1;
        case DG_NORM_BF16: return a.K == 512 ? launch_dg_mid<DG_NORM_BF16, 512, 32>(a, stream) : -1;
        case DG_NORM_BF16_RELU: return a.K == 512 ? launch_dg_mid<DG_NORM_BF16_RELU, 512, 64>(a, stream) : -1;
        case DG_NORM_LOGITS: return a.K == 512 ? launch_dg_mid<DG_NORM_LOGITS, 512, 64>(a, stream) : -1;
        default: return -1;
    }
}

int launch_dec_gemm(int mode, const DecGemmArgs& a, hipStream_t stream) {
    if (a.R <= 0) return 0;
    if (a.N % 16) return -1;
    const int mid_rows = a.mid_rows >= 0 ? a.mid_rows : DEC_GEMM_MID_ROWS;
    if (a.table && (mode != DG_NORM_QKV_CACHE || a.pend_y || (mid_rows > 0 && a.R >= mid_rows))) return -1;     // the 16-row-tile kernel only
    if (mid_rows > 0 && a.R >= mid_rows && a.N % 64 == 0 && !a.part && !a.pend_y && (a.K == 512 || (a.K == 2048 && mode == DG_RESID)))
        return launch_dec_gemm_mid(mode, a, stream);
    if (mode == DG_RESID) {
        if (a.K == 512) return launch_dg<DG_RESID, 512>(a, stream);
        if (a.K == 2048) return launch_dg<DG_RESID, 2048>(a, stream);
        if (a.K == 1024) return launch_dg<DG_RESID, 1024>(a, stream);
        return -1;
    }
    if (a.K != 512) return -1;
    if (a.pend_y) {           // a pending MoE combine: only the two kernels that can follow an MoE FFN take it
        if (mode == DG_NORM_QKV_CACHE) return launch_dg_wide<DG_NORM_QKV_CACHE, true>(a, stream);
        if (mode == DG_NORM_LOGITS) return launch_dg_wide<DG_NORM_LOGITS, true>(a, stream);
        return -1;
    }
    switch (mode) {
        case DG_NORM_QKV_CACHE: return launch_dg_wide<DG_NORM_QKV_CACHE>(a, stream);
        case DG_NORM_BF16: return launch_dg_wide<DG_NORM_BF16>(a, stream);
        case DG_NORM_BF16_RELU: return launch_dg_wide<DG_NORM_BF16_RELU>(a, stream);
        case DG_NORM_LOGITS: return launch_dg_wide<DG_NORM_LOGITS>(a, stream);
        default: return -1;
    }
}

int launch_dec_attention(bool self_attn, const DecAttnArgs& a, hipStream_t stream) {
    if (a.R <= 0) return 0;
    const bool many = a.force_many || a.R * a.H > 2048;
    if (a.chain_sync && (self_attn || !a.wq)) return -1;                              // only the fused cross-attention zeroes the chain counters
    if ((a.wo || a.ipart) && (many || a.H != 8 || (a.wo && !a.opart) || (a.ipart && !a.wq))) return -1;   // folded O-projection: 8 heads, 8-wave kernels
    if (a.row0 < 0 || a.row0 > 0xffff || a.rows_per_kv < 1 || a.rows_per_kv > 0xff || a.H < 1 || a.H > 0xff || a.slab_keys < 1 || a.slab_keys > 0xfffff ||
        a.n_keys_const < 0 || a.n_keys_const > 0xfff || (self_attn && a.bias_stride != a.slab_keys))
        return -1;                                                                     // the packed geometry words
    const unsigned g0 = (unsigned)a.row0 | (unsigned)a.rows_per_kv << 16 | (unsigned)a.H << 24, g1 = (unsigned)a.slab_keys | (unsigned)a.n_keys_const << 20;
    const int grid = a.R * a.H;
#define ATTN(S, F, W, O, THREADS, LDS, PQ, PF, P4, P5) dec_attn_kernel<S, F, W, O><<<grid, THREADS, LDS, stream>>>(a.k, a.v, PQ, PF, P4, P5, g0, g1, a)
    if (self_attn) {
        if (a.wo) ATTN(true, false, 8, true, 512, WO_LDS_BYTES, a.q, a.bias, a.shared, a.row_pos);
        else if (many) ATTN(true, false, 2, false, 128, 0, a.q, a.bias, a.shared, a.row_pos);
        else ATTN(true, false, 8, false, 512, 0, a.q, a.bias, a.shared, a.row_pos);
    } else if (a.wq) {
        // the fused projection maps one thread per d_model element
        if (a.ipart) ATTN(false, true, 8, true, 512, 0, a.wq, a.x_f32, a.gain, a.ipart);
        else ATTN(false, true, 8, false, 512, 0, a.wq, a.x_f32, a.gain, a.ssq);
    } else {
        if (many) ATTN(false, false, 2, false, 128, 0, a.q, nullptr, nullptr, nullptr);
        else ATTN(false, false, 8, false, 512, 0, a.q, nullptr, nullptr, nullptr);
    }
#undef ATTN
    return 0;
}

// beam search: no folded O-projection; the staged table is the kernel's dynamic LDS block.  a.row_pos (slot mode, ymt3_transcribe_stream_beam)
// goes where the plain self-attention takes it: attn_body reads a row's key count as row_pos[r] + 1 behind the same workgroup-uniform test
// of the pointer, and the BEAM path picks the ancestry buffer by the parity of THAT position, so a row at its own position stages its own
// table -- the lock-step and the slot-mode call run the same two instantiations.
int launch_dec_attention_beam(const DecAttnArgs& a, const BeamAttn& ba, hipStream_t stream) {
    if (a.R <= 0) return 0;
    if (!ba.anc || ba.W < 1 || ba.W > BEAM_MAX || a.R % ba.W || a.row0 % ba.W || ba.anc_pitch % 16 || ba.anc_pitch <= a.slab_keys || ba.anc_pitch > 48 * 1024 ||
        a.row0 + a.R > ba.anc_rows || a.wo || a.ipart || a.wq || a.chain_sync || a.rows_per_kv != 1)
        return -1;
    if (a.row0 < 0 || a.row0 > 0xffff || a.H < 1 || a.H > 0xff || a.slab_keys < 1 || a.slab_keys > 0xfffff || a.bias_stride != a.slab_keys) return -1;
    const bool many = a.force_many || a.R * a.H > 2048;
    const unsigned g0 = (unsigned)a.row0 | 1u << 16 | (unsigned)a.H << 24, g1 = (unsigned)a.slab_keys;
    const int grid = a.R * a.H;
    if (many) dec_attn_beam_kernel<2><<<grid, 128, ba.anc_pitch, stream>>>(a.k, a.v, a.q, a.bias, a.shared, a.row_pos, g0, g1, a, ba);
    else dec_attn_beam_kernel<8><<<grid, 512, ba.anc_pitch, stream>>>(a.k, a.v, a.q, a.bias, a.shared, a.row_pos, g0, g1, a, ba);
    return 0;
}

// the attention pair's 8 x R <= 512 workgroups must all be resident at once: two per CU at its LDS / register footprint
bool dec_attention_pair_fits(int n_cus) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dec_attn_pair_kernel, 512, WO_LDS_BYTES) != hipSuccess) return false;
    return (long long)n * n_cus >= 512;
}

// self-attention (folded O-projection) + fused cross-attention of one layer as one launch; < 0: not this kernel's shape
int launch_dec_attention_pair(const DecAttnArgs& a, const DecAttnArgs& b, unsigned* pair_rows, unsigned* abort_word, unsigned* host_abort,
                              hipStream_t stream) {
    if (a.R <= 0) return 0;
    if (a.R > 16 * CHAIN_TILES_MAX || a.R != b.R || a.row0 != b.row0 || a.H != 8 || b.H != 8 || !a.wo || !a.opart || !b.wq || b.ipart != a.opart || !pair_rows || !abort_word ||
        a.rows_per_kv != 1 || b.rows_per_kv < 1 || b.rows_per_kv > 0xff || a.row0 < 0 || a.row0 > 0xffff || a.slab_keys < 1 || a.slab_keys > 0xfffff ||
        b.slab_keys < 1 || b.slab_keys > 0xfffff || b.n_keys_const < 1 || b.n_keys_const > 0xfff || a.bias_stride != a.slab_keys)
        return -1;
    const unsigned g0 = (unsigned)a.row0 | 1u << 16 | 8u << 24, g1 = (unsigned)a.slab_keys;
    const unsigned h0 = (unsigned)b.row0 | (unsigned)b.rows_per_kv << 16 | 8u << 24, h1 = (unsigned)b.slab_keys | (unsigned)b.n_keys_const << 20;
    dec_attn_pair_kernel<<<a.R * 8, 512, WO_LDS_BYTES, stream>>>(a.k, a.v, a.q, a.bias, a.shared, a.row_pos, g0, g1, a, b, h0, h1,
                                                                 PairSync{pair_rows, abort_word, host_abort});
    return 0;
}

// the layer-0 table: one channel, rows of QKV0_COLS columns (8 heads of 64), every destination set
static bool qkv0_args_ok(const ArgmaxArgs& a) {
    return !a.qkv0 || (a.q0 && a.kcache0 && a.vcache0 && a.H * DKV * 3 == QKV0_COLS && a.L > 0 && !a.chan_embed && a.n_channels == 1);
}

int launch_argmax_embed(const ArgmaxArgs& a, hipStream_t stream) {
    if (a.R <= 0) return 0;
    if (!qkv0_args_ok(a)) return -1;
    argmax_embed_kernel<<<a.R, 256, 0, stream>>>(a.logits, a.shared, a.finished, a.row_pos, a.row_out, a.embed, a.row0, a.V, a);
    return 0;
}

int launch_decode_init(const ArgmaxArgs& a, int n_chains, int n_steps, int step0, int32_t* tokens_out, const int32_t* forced,
                       float* logits_out, const int32_t* prompt, int n_prompt, float* scores_out, const ConstraintView& cv,
                       hipStream_t stream) {
    if (a.R <= 0) return 0;
    if (n_prompt < 0 || (n_prompt > 0 && !prompt)) return -1;
    if (cv.allowed && (!cv.next || !a.row_state || cv.n_states < 1 || cv.words * 32 < a.V)) return -1;
    if (!qkv0_args_ok(a) || (a.qkv0 && (step0 < 0 || step0 >= a.L))) return -1;
    decode_init_kernel<<<a.R, 256, 0, stream>>>(a, n_chains, n_steps, step0, tokens_out, forced, logits_out, prompt, n_prompt, scores_out, cv);
    return 0;
}

int launch_slot_start(const ArgmaxArgs& a, int row0, long long first_out, int n_steps, long long* row_out, long long first_prompt,
                      int n_prompt, long long* row_prompt, const ConstraintView& cv, hipStream_t stream) {
    if (!a.row_pos || !row_out || !row_prompt || a.n_channels <= 0) return -1;
    if (cv.start && cv.n_states < 1) return -1;
    if (!qkv0_args_ok(a)) return -1;
    slot_start_kernel<<<a.n_channels, 256, 0, stream>>>(a, row0, first_out, n_steps, row_out, first_prompt, n_prompt, row_prompt, cv);
    return 0;
}

int launch_slot_retire(const ArgmaxArgs& a, int row0, int n_rows, int n_steps, int n_prompt, int32_t* tokens_out, float* scores_out,
                       hipStream_t stream) {
    if (!a.row_pos || !a.row_out || n_rows <= 0) return -1;
    slot_retire_kernel<<<n_rows, 256, 0, stream>>>(a, row0, n_steps, n_prompt, tokens_out, scores_out);
    return 0;
}

int launch_pad_tail(int32_t* tokens_out, float* scores_out, int row0, int R, int n_steps, int from, int pad_id, hipStream_t stream) {
    if (R <= 0 || from >= n_steps) return 0;
    pad_tail_kernel<<<R, 256, 0, stream>>>(tokens_out, scores_out, row0, n_steps, from, pad_id);
    return 0;
}

int launch_qkv0_embed(const ArgmaxArgs& a, int v0, int n, hipStream_t stream) {
    if (n <= 0 || v0 < 0 || v0 + n > a.V || !a.h || !a.ssq || !a.embed || a.ssq_stride < n) return -1;
    qkv0_embed_kernel<<<n, 256, 0, stream>>>(a, v0);
    return 0;
}
