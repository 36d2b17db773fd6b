// Device alignment: banded dynamic time warping of a reference note set onto an estimate over frame-wise pitch sets, and the warp of note
// times along the path (include/ymt3.h, alignment).  The specification is the host path, dtw_align and warp_notes of
// yourmt3_amd/metrics.py; tests/align_model.py states the rules as plain loops.  Everything is an integer, or an f64 expression with
// contraction off: every output equals the host's.
//
// Features: feat[side][frame][2], two 16-byte words per frame (the instrument-agnostic pitch set, then the drum row's), each side packed at
// its own frame count.  The rasteriser classifies a record and clips its frames by the rule roll.hip and metrics.hip use (note_rule.h).
//
// The dynamic programme runs on (r, c): c is the LONGER side (the lanes' axis), r the other; for n_ref_frames > n_est_frames that is the
// transposed problem, and only the tie order between the two non-diagonal steps and the step codes (always those of the untransposed
// cell: 0 diagonal, 1 (i-1, j), 2 (i, j-1)) know about it.  The band |r * (C-1) - c * (R-1)| <= band * max(C-1, 1) is the rule's, which is
// symmetric.
// (a) align_clear_kernel: zeroes the feature words in use and result[4]; sets the edge arrays, the corners and the total to INF.
// (b) align_raster_kernel: one wave per record and side, as in roll.hip.
// (c) align_tile_kernel: one wave per tile of ALIGN_TILE_ROWS x 64 cells, one launch per tile anti-diagonal, the tiles of a launch being
//     independent.  Lane l owns column c0 + l and keeps its 256 bits in eight registers; at step s it computes cell (r0 + s - l, c0 + l):
//     D(r, c-1) comes from lane l-1 by one cross-lane move, D(r-1, c-1) is what came the step before, D(r-1, c) is the lane's own last
//     value.  The tile's rows are staged in LDS at 32 bytes per frame.  A tile reads bottom[c] (the last row above), right[r] (the last
//     column to its left) and its corner, and overwrites them with its own last row, last column and last cell; a tile wholly outside the
//     band is not run and leaves INF (the in-band tiles of a tile row, column or diagonal are contiguous: the band is convex).
//     Steps: 2 bits per cell, steps[c][(r >> 4) - (rlo(c) >> 4)] holding 16 consecutive rows of column c, rlo(c) being the column's first
//     in-band row: a lane writes whole dwords, and only dwords that hold an in-band cell.
// (d) align_backtrack_kernel, one workgroup: walks the path tile by tile with the tile's step dwords staged in LDS, writing it in reverse
//     into scratch; then all lanes copy it out forward, set warp[i] to the j of the first path cell of row i, and write result.
// (e) warp_notes_kernel: one lane per record, W(t) of the rules on onset and offset.
// No kernel waits on another workgroup and nothing spins.  All launch counts follow from the shapes: nothing is read back.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "note_rule.h"

namespace {

constexpr int ALIGN_THREADS = 256;
constexpr int CLEAR_BLOCKS = 1024;
constexpr int TR = ALIGN_TILE_ROWS, TC = ALIGN_TILE_COLS;
constexpr int GROUPS = TR / 16;                                          // step dwords of a tile column
static_assert(TC == WAVE && TR % 16 == 0, "one lane per tile column; a step dword holds 16 rows");

// the dynamic programme's view of a call
struct Dp {
    long long R, C, PC, QR, BM;           // rows, columns (C >= R), C - 1, R - 1, band * max(PC, 1)
    int transposed;                       // r is the estimate's frame, c the reference's
    int ntr, ntc;                         // tiles per side
    long long step_words;                 // dwords per column of steps
    const uint4 *feat_r, *feat_c;
    int *bottom, *right, *corner, *total;
    unsigned* steps;
};

__host__ __device__ inline bool tile_in_band(const Dp& d, long long tr, long long tc) {
    const long long r0 = tr * TR, c0 = tc * TC;
    const long long r1 = (r0 + TR < d.R ? r0 + TR : d.R) - 1, c1 = (c0 + TC < d.C ? c0 + TC : d.C) - 1;
    return r1 * d.PC - c0 * d.QR >= -d.BM && r0 * d.PC - c1 * d.QR <= d.BM;
}

// the 16-row group of column c's first in-band row
__device__ __forceinline__ long long first_group(const Dp& d, long long c) {
    const long long num = c * d.QR - d.BM;
    return (num <= 0 || d.PC == 0) ? 0 : ((num + d.PC - 1) / d.PC) >> 4;
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_clear_kernel(AlignArgs a, Dp d) {
    const long long stride = (long long)gridDim.x * ALIGN_THREADS, t0 = (long long)blockIdx.x * ALIGN_THREADS + threadIdx.x;
    for (int s = 0; s < 2; ++s) {
        uint4* f = a.feat + (long long)s * a.max_frames * 2;
        for (long long i = t0; i < a.n_frames[s] * 2; i += stride) f[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    for (long long i = t0; i < (long long)d.ntc * TC; i += stride) d.bottom[i] = ALIGN_INF;
    for (long long i = t0; i < (long long)d.ntr * TR; i += stride) d.right[i] = ALIGN_INF;
    for (long long i = t0; i < d.ntr + d.ntc - 1; i += stride) d.corner[i] = ALIGN_INF;
    if (t0 == 0) *d.total = ALIGN_INF;
    if (t0 < 4) a.result[t0] = 0;
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_raster_kernel(AlignArgs a) {
    const int side = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * (ALIGN_THREADS / WAVE) + (threadIdx.x >> 6);
    if (i >= note_live_count(a.n[side], a.count[side])) return;
    const DetokNote r = a.notes[side][i];
    const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
    if (!c.counted) {
        if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[2 + side]), 1ull);
        return;
    }
    long long f_lo, f_hi;
    if (!note_frame_span(r, c.drum, a.frames_per_second, a.n_frames[side], &f_lo, &f_hi)) return;
    const unsigned bit = 1u << (r.pitch & 31);
    unsigned* w = reinterpret_cast<unsigned*>(a.feat + (long long)side * a.max_frames * 2) + (c.drum ? 4 : 0) + (r.pitch >> 5);
    for (long long f = f_lo + lane; f < f_hi; f += WAVE) atomicOr(&w[f * 8], bit);
}

__device__ __forceinline__ int popc4(uint4 a, uint4 b) { return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w); }

__global__ __launch_bounds__(WAVE) void align_tile_kernel(Dp d, int antidiagonal, int tr_first) {
    const int tr = tr_first + blockIdx.x, tc = antidiagonal - tr;
    if (tr < 0 || tr >= d.ntr || tc < 0 || tc >= d.ntc || !tile_in_band(d, tr, tc)) return;
    __shared__ uint4 rows[TR][2];
    __shared__ int left_edge[TR + 1];                                   // D(r0 - 1 + k, c0 - 1): the corner, then right[r0 ...]
    const int lane = threadIdx.x;
    const long long r0 = (long long)tr * TR, c0 = (long long)tc * TC, c = c0 + lane;
    const int diag_id = tc - tr + d.ntr - 1;
    for (int k = lane; k < TR; k += WAVE) {
        const long long r = r0 + k;
        const bool in = r < d.R;
        rows[k][0] = in ? d.feat_r[r * 2] : make_uint4(0u, 0u, 0u, 0u);
        rows[k][1] = in ? d.feat_r[r * 2 + 1] : make_uint4(0u, 0u, 0u, 0u);
        left_edge[k + 1] = d.right[r];
    }
    if (lane == 0) left_edge[0] = d.corner[diag_id];
    __syncthreads();
    const bool col = c < d.C;
    const uint4 e0 = col ? d.feat_c[c * 2] : make_uint4(0u, 0u, 0u, 0u), e1 = col ? d.feat_c[c * 2 + 1] : make_uint4(0u, 0u, 0u, 0u);
    const long long group0 = (r0 >> 4) - (col ? first_group(d, c) : 0);
    unsigned* my_steps = d.steps + (col ? c : 0) * d.step_words;
    int cur = d.bottom[c];                                               // D(r0 - 1, c); the arrays are padded to whole tiles
    int recv = __shfl_up(cur, 1, WAVE);                                  // D(r0 - 1, c - 1)
    if (lane == 0) recv = left_edge[0];
    long long f = (r0 - lane) * d.PC - c * d.QR;                         // r * PC - c * QR of the cell of step 0, then + PC per step
    unsigned acc = 0;
    bool any = false;
    for (int s = 0; s < TR + WAVE - 1; ++s) {
        const int diag = recv;
        recv = __shfl_up(cur, 1, WAVE);                                  // lane l-1's cell of the step before: D(r, c - 1)
        const int k = s - lane;
        if (k >= 0 && k < TR) {
            if (lane == 0) recv = left_edge[k + 1];
            const long long r = r0 + k;
            const bool in = col && r < d.R && f >= -d.BM && f <= d.BM;
            int v = ALIGN_INF;
            unsigned code = 0;
            if (in) {
                const int up = cur, left = recv;
                int best = min(diag, min(up, left));
                const int first = d.transposed ? left : up;              // (i-1, j) of the untransposed cell
                code = diag == best ? 0u : (first == best ? 1u : 2u);
                if (r == 0 && c == 0) best = 0;
                v = min(best + popc4(rows[k][0], e0) + popc4(rows[k][1], e1), ALIGN_INF);
                if (r == d.R - 1 && c == d.C - 1) *d.total = v;
            }
            cur = v;
            acc |= code << (2 * (k & 15));
            any |= in;
            if ((k & 15) == 15) {
                const long long g = group0 + (k >> 4);
                if (any && g >= 0 && g < d.step_words) my_steps[g] = acc;
                acc = 0;
                any = false;
            }
            if (lane == WAVE - 1) d.right[r] = v;
        }
        f += d.PC;
    }
    d.bottom[c] = cur;
    if (lane == WAVE - 1) d.corner[diag_id] = cur;
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_backtrack_kernel(AlignArgs a, Dp d) {
    __shared__ unsigned tile[TC][GROUPS + 1];
    __shared__ long long pos[2];                                         // the path's current cell (i, j)
    __shared__ long long len;
    __shared__ int state;                                                // 0 walking, 1 arrived at (0, 0), 2 lost
    const int tid = threadIdx.x;
    const long long na = a.n_frames[0], nb = a.n_frames[1], cap = na + nb - 1;
    const int total = *d.total;
    if (tid == 0) {
        pos[0] = na - 1; pos[1] = nb - 1; len = 0;
        state = total >= ALIGN_INF ? 2 : 0;
    }
    __syncthreads();
    while (state == 0) {
        const long long r = d.transposed ? pos[1] : pos[0], c = d.transposed ? pos[0] : pos[1];
        const long long r0 = r / TR * TR, c0 = c / TC * TC;
        __syncthreads();                                                 // everyone has read pos and state
        for (int x = tid; x < TC * GROUPS; x += ALIGN_THREADS) {
            const int l = x / GROUPS, g = x % GROUPS;
            const long long cc = c0 + l;
            unsigned w = 0;
            if (cc < d.C) {
                const long long idx = (r0 >> 4) + g - first_group(d, cc);
                if (idx >= 0 && idx < d.step_words) w = d.steps[cc * d.step_words + idx];
            }
            tile[l][g] = w;
        }
        __syncthreads();
        if (tid == 0) {
            long long i = pos[0], j = pos[1], n = len;
            int st = 0;
            while (true) {
                const long long rr = d.transposed ? j : i, cc = d.transposed ? i : j;
                if (rr < r0 || cc < c0) break;                           // the walk only goes up and left
                if (n >= cap) { st = 2; break; }
                a.rpath[n++] = make_int2((int)i, (int)j);
                if (i == 0 && j == 0) { st = 1; break; }
                const int k = (int)(rr - r0);
                const unsigned code = (tile[cc - c0][k >> 4] >> (2 * (k & 15))) & 3u;
                i -= code != 2u;
                j -= code != 1u;
                if (i < 0 || j < 0) { st = 2; break; }
            }
            pos[0] = i; pos[1] = j; len = n; state = st;
        }
        __syncthreads();
    }
    const long long n = state == 1 ? len : 0;
    if (state != 1)
        for (long long i = tid; i < na; i += ALIGN_THREADS) a.warp[i] = -1;
    for (long long k = tid; k < n; k += ALIGN_THREADS) {
        const int2 cell = a.rpath[n - 1 - k];
        if (a.path) reinterpret_cast<int2*>(a.path)[k] = cell;
        if (k == 0 || a.rpath[n - k].x != cell.x) a.warp[cell.x] = cell.y;
    }
    if (tid == 0) {
        a.result[0] = state == 1 ? total : ALIGN_INF;
        a.result[1] = n;
    }
}

__device__ __forceinline__ double warp_time(double t, const int32_t* warp, double q, double fps) {
#pragma clang fp contract(off)
    const double x = t * fps;
    if (x != x) return x;
    double k = floor(x);
    k = k > 0.0 ? k : 0.0;
    k = k < q ? k : q;
    double f = x - k;
    f = f > 0.0 ? f : 0.0;
    f = f < 1.0 ? f : 1.0;
    const long long ki = (long long)k, kn = ki + 1 < (long long)q ? ki + 1 : (long long)q;
    const double w0 = (double)warp[ki], w1 = (double)warp[kn];
    return (w0 + f * (w1 - w0)) / fps;
}

__global__ __launch_bounds__(ALIGN_THREADS) void warp_notes_kernel(WarpNotesArgs a) {
    const long long i = (long long)blockIdx.x * ALIGN_THREADS + threadIdx.x;
    if (i >= note_live_count(a.n, a.count)) return;
    DetokNote r = a.notes[i];
    const double q = (double)(a.n_ref_frames - 1);
    r.onset = warp_time(r.onset, a.warp, q, a.frames_per_second);
    r.offset = warp_time(r.offset, a.warp, q, a.frames_per_second);
    a.out[i] = r;
}

}  // namespace

int launch_align(const AlignArgs& a, hipStream_t stream) {
    if (a.n_programs < 1 || a.n_programs > ROLL_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -1;
    if (a.max_frames < 1 || a.max_frames > ALIGN_MAX_FRAMES || a.band_frames < 1 || a.band_frames > a.max_frames) return -2;
    for (int s = 0; s < 2; ++s) {
        if (a.n_frames[s] < 1 || a.n_frames[s] > a.max_frames) return -3;
        if (a.n[s] < 0 || a.n[s] > ROLL_MAX_NOTES || (a.n[s] && !a.notes[s])) return -4;
    }
    if (!a.feat || !a.edges || !a.steps || !a.rpath || !a.warp || !a.result || !(a.frames_per_second > 0.0)) return -5;
    Dp d{};
    d.transposed = a.n_frames[0] > a.n_frames[1];
    d.R = a.n_frames[d.transposed ? 1 : 0];
    d.C = a.n_frames[d.transposed ? 0 : 1];
    d.PC = d.C - 1; d.QR = d.R - 1;
    d.BM = a.band_frames * std::max(d.PC, 1LL);
    d.ntr = (int)((d.R + TR - 1) / TR); d.ntc = (int)((d.C + TC - 1) / TC);
    d.step_words = align_step_words(a.band_frames);
    d.feat_r = a.feat + (d.transposed ? a.max_frames * 2 : 0);
    d.feat_c = a.feat + (d.transposed ? 0 : a.max_frames * 2);
    d.bottom = a.edges;
    d.right = d.bottom + align_padded(a.max_frames, TC);
    d.corner = d.right + align_padded(a.max_frames, TR);
    d.total = d.corner + align_corners(a.max_frames);
    d.steps = a.steps;
    const long long work = std::max({a.n_frames[0] * 2, a.n_frames[1] * 2, (long long)d.ntc * TC});
    align_clear_kernel<<<(unsigned)std::max(1LL, std::min<long long>((work + ALIGN_THREADS - 1) / ALIGN_THREADS, CLEAR_BLOCKS)), ALIGN_THREADS, 0, stream>>>(a, d);
    const long long n = std::max(a.n[0], a.n[1]);
    if (n) {
        const int per = ALIGN_THREADS / WAVE;
        align_raster_kernel<<<dim3((unsigned)((n + per - 1) / per), 2), ALIGN_THREADS, 0, stream>>>(a);
    }
    for (int ad = 0; ad < d.ntr + d.ntc - 1; ++ad) {
        int first = std::max(0, ad - d.ntc + 1), last = std::min(ad, d.ntr - 1);
        while (first <= last && !tile_in_band(d, first, ad - first)) ++first;
        while (last >= first && !tile_in_band(d, last, ad - last)) --last;
        if (first <= last) align_tile_kernel<<<(unsigned)(last - first + 1), WAVE, 0, stream>>>(d, ad, first);
    }
    align_backtrack_kernel<<<1, ALIGN_THREADS, 0, stream>>>(a, d);
    return 0;
}

int launch_warp_notes(const WarpNotesArgs& a, hipStream_t stream) {
    if (a.n < 0 || a.n > ROLL_MAX_NOTES || a.n_ref_frames < 1 || a.n_ref_frames > ALIGN_MAX_FRAMES || !(a.frames_per_second > 0.0)) return -1;
    if (a.n == 0) return 0;
    if (!a.notes || !a.out || !a.warp) return -2;
    warp_notes_kernel<<<(unsigned)((a.n + ALIGN_THREADS - 1) / ALIGN_THREADS), ALIGN_THREADS, 0, stream>>>(a);
    return 0;
}
