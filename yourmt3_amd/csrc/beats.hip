// Beat tracking over note records: onset envelope, windowed autocorrelation tempogram, a tempo path over the windows, a dynamic-programming
// beat tracker, and every note's position in beats (include/ymt3.h, beat tracking).  The specification is the host path, track_beats and
// beat_positions of yourmt3_amd/beats.py; tests/beat_model.py states the rules as plain loops.  Everything is an integer, or an f64
// expression with contraction off: every output equals the host's.
// (a) beat_clear_kernel zeroes e[0, n_frames) and result[4]; beat_envelope_kernel, one lane per record, classifies it by the rule metrics.hip,
//     roll.hip and align.hip use (note_rule.h) and adds 1 to e[F(onset)] (an integer atomicAdd: exact in any order), or to `skipped`;
//     beat_smooth_kernel caps e and writes s = e[f-1] + 2 e[f] + e[f+1].
// (b) beat_tempogram_kernel, one workgroup per window: the window's s[lo, hi + lag_max) is staged once in LDS as 16-bit values (zeros beyond
//     the frames, which is the rule's f + L < n_frames), the waves split the lags, the lanes the frames, a __shfl_xor butterfly finishes
//     each sum.  A fits int32: s <= 4 * 255 and a window has at most 2048 frames.
// (c) beat_tempo_path_kernel, one workgroup, one lane per lag, serial over the windows: the previous row of V lies in LDS, double
//     buffered, so a window costs one barrier; the next window's row of T is requested before the current one is finished; back-pointers
//     go to global scratch and lane 0 follows them back (written and read by one workgroup, ordered by __syncthreads).
// (d) beat_dp_kernel, one workgroup, the serial spine: frame f looks back no nearer than ceil(t / 2) >= G = ceil(lag_min / 2) frames, so G
//     consecutive frames are independent.  The workgroup steps through the file G frames at a time, one wave per frame of the block (a
//     wave takes several when G > 16); the wave's lanes split the predecessors and a butterfly that carries (value, p) takes the maximum,
//     the larger p winning a tie at every exchange, which is the rule's "largest p".  C lives in an LDS ring of BEAT_RING int64 (a block
//     writes frames [f0, f0 + G) and reads [f0 - 2 lag_max, f0): 2 lag_max + G entries suffice), back[] in global scratch; one barrier
//     per block.  Each wave keeps a running (max, first f); lane 0 joins them, follows back[] into a reversed scratch, and all lanes copy
//     the beats out forward, as align_backtrack_kernel does.
// (e) beat_positions_kernel, one lane per record: a binary search over the beats, then the f64 expression.
// No kernel waits on another workgroup and nothing spins.  All launch counts follow from the shapes: nothing is read back.
#include <climits>

#include "common.h"
#include "kernels.h"
#include "note_rule.h"

namespace {

constexpr int BEAT_THREADS = 256;
constexpr int BEAT_PATH_THREADS = 512;                                 // one lane per lag
constexpr int BEAT_DP_WAVES = 16;
static_assert(BEAT_PATH_THREADS >= BEAT_MAX_LAG - BEAT_MIN_LAG + 1, "one lane per lag");
static_assert(BEAT_RING >= 2 * BEAT_MAX_LAG + (BEAT_MAX_LAG + 1) / 2 && (BEAT_RING & (BEAT_RING - 1)) == 0, "the ring holds a block's reach");

__global__ __launch_bounds__(BEAT_THREADS) void beat_clear_kernel(BeatArgs a) {
    const long long stride = (long long)gridDim.x * BEAT_THREADS, t0 = (long long)blockIdx.x * BEAT_THREADS + threadIdx.x;
    for (long long f = t0; f < a.n_frames; f += stride) a.env[f] = 0u;
    if (t0 < 4) a.result[t0] = 0;
}

__global__ __launch_bounds__(BEAT_THREADS) void beat_envelope_kernel(BeatArgs a) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * BEAT_THREADS + threadIdx.x;
    if (i >= note_live_count(a.n, a.count)) return;
    const DetokNote r = a.notes[i];
    if (!note_classify(r, a.n_programs, a.drum_program).counted) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[3]), 1ull);
        return;
    }
    const double f = rint(r.onset * a.frames_per_second);
    if (f >= 0.0 && f < (double)a.n_frames) atomicAdd(&a.env[(long long)f], 1u);
}

__global__ __launch_bounds__(BEAT_THREADS) void beat_smooth_kernel(BeatArgs a) {
    const long long f = (long long)blockIdx.x * BEAT_THREADS + threadIdx.x;
    if (f >= a.n_frames) return;
    const unsigned cap = (unsigned)a.onset_cap;
    const unsigned l = f > 0 ? min(a.env[f - 1], cap) : 0u, m = min(a.env[f], cap), r = f + 1 < a.n_frames ? min(a.env[f + 1], cap) : 0u;
    a.smooth[f] = (unsigned short)(l + 2u * m + r);
}

__global__ __launch_bounds__(BEAT_THREADS) void beat_tempogram_kernel(BeatArgs a) {
    __shared__ unsigned short sh[BEAT_MAX_WINDOW + BEAT_MAX_LAG];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const long long w = blockIdx.x, c = w * a.hop + a.hop / 2;
    const long long lo = max(0LL, c - a.window / 2), hi = min(a.n_frames, c + a.window / 2);
    const int len = (int)(hi - lo), nL = a.lag_max - a.lag_min + 1;
    for (int i = tid; i < len + a.lag_max; i += BEAT_THREADS) sh[i] = lo + i < a.n_frames ? a.smooth[lo + i] : (unsigned short)0;
    __syncthreads();
    for (int L = a.lag_min + wave; L <= a.lag_max; L += BEAT_THREADS / WAVE) {
        int acc = 0;
        for (int f = lane; f < len; f += WAVE) acc += (int)sh[f] * (int)sh[f + L];
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) acc += __shfl_xor(acc, x, WAVE);
        if (lane == 0) a.tgram[w * nL + (L - a.lag_min)] = (long long)acc * (long long)a.prior[L - a.lag_min];
    }
}

__global__ __launch_bounds__(BEAT_PATH_THREADS) void beat_tempo_path_kernel(BeatArgs a) {
    __shared__ long long V[2][BEAT_PATH_THREADS];
    const int l = threadIdx.x, nL = a.lag_max - a.lag_min + 1, D = min(a.lag_step, nL);
    const long long nW = beat_windows(a.n_frames, a.hop);
    const bool active = l < nL;
    if (active) V[0][l] = a.tgram[l];
    long long t_next = active && nW > 1 ? a.tgram[nL + l] : 0;
    __syncthreads();
    int cur = 0;
    for (long long w = 1; w < nW; ++w) {
        const long long t_cur = t_next;
        if (active && w + 1 < nW) t_next = a.tgram[(w + 1) * nL + l];
        if (active) {
            long long best = V[cur][l];
            int arg = l;
            for (int k = 1; k <= D; ++k) {                                // the nearest first, the smaller before the larger: only a strictly larger value takes over
                if (l - k >= 0 && V[cur][l - k] > best) { best = V[cur][l - k]; arg = l - k; }
                if (l + k < nL && V[cur][l + k] > best) { best = V[cur][l + k]; arg = l + k; }
            }
            V[cur ^ 1][l] = t_cur + best;
            a.lag_back[w * nL + l] = (unsigned short)arg;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (l == 0) {
        long long top = V[cur][0];
        int arg = 0;
        for (int j = 1; j < nL; ++j)
            if (V[cur][j] > top) { top = V[cur][j]; arg = j; }
        for (long long w = nW - 1; w >= 0; --w) {
            a.lags[w] = arg + a.lag_min;
            if (a.tempo) a.tempo[w] = arg + a.lag_min;
            if (w) arg = a.lag_back[w * nL + arg];
        }
        a.result[2] = top;
    }
}

__global__ __launch_bounds__(BEAT_DP_WAVES* WAVE) void beat_dp_kernel(BeatArgs a, int G, int n_waves) {
    __shared__ long long ring[BEAT_RING];
    __shared__ long long top_c[BEAT_DP_WAVES];
    __shared__ int top_f[BEAT_DP_WAVES];
    __shared__ long long n_found;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int n = (int)a.n_frames, row = 2 * a.lag_max + 1;
    const int last_window = (int)beat_windows(a.n_frames, a.hop) - 1;
    long long best_c = 0;
    int best_f = -1;
    for (int f0 = 0; f0 < n; f0 += G) {
        for (int k = wave; k < G; k += n_waves) {
            const int f = f0 + k;
            if (f >= n) break;
            const int t = a.lags[min(f / a.hop, last_window)];
            const int lo = max(0, f - 2 * t), hi = f - (t + 1) / 2;
            const long long mine = 1024LL * a.smooth[f];
            const int32_t* pen = a.pen + (long long)(t - a.lag_min) * row;
            long long v = LLONG_MIN;
            int vp = -1;
            for (int p = lo + lane; p <= hi; p += WAVE) {
                const long long c = ring[p & (BEAT_RING - 1)] - pen[f - p];
                if (c >= v) { v = c; vp = p; }                             // p ascends within a lane: the larger p keeps a tie
            }
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) {
                const long long ov = __shfl_xor(v, x, WAVE);
                const int op = __shfl_xor(vp, x, WAVE);
                if (ov > v || (ov == v && op > vp)) { v = ov; vp = op; }
            }
            const bool linked = v > 0;                                     // (a lane without a predecessor holds LLONG_MIN)
            const long long c = mine + (linked ? v : 0);
            if (lane == 0) {
                ring[f & (BEAT_RING - 1)] = c;
                a.back[f] = linked ? vp : -1;
            }
            if (c > best_c) { best_c = c; best_f = f; }                    // f ascends within a wave: the first f keeps a tie
        }
        __syncthreads();
    }
    if (lane == 0 && wave < BEAT_DP_WAVES) { top_c[wave] = best_c; top_f[wave] = best_f; }
    __syncthreads();
    if (tid == 0) {
        long long c = 0;
        int f = -1;
        for (int k = 0; k < n_waves; ++k)
            if (top_c[k] > c || (top_c[k] == c && c > 0 && top_f[k] < f)) { c = top_c[k]; f = top_f[k]; }
        const long long cap = min(a.max_beats, beat_max_beats(a.n_frames, a.lag_min));
        long long found = 0;
        while (f >= 0 && found < cap) {
            a.rbeats[found++] = f;
            f = a.back[f];
        }
        n_found = found;
        a.result[0] = found;
        a.result[1] = c;
    }
    __syncthreads();
    const long long found = n_found;
    for (long long k = tid; k < found; k += blockDim.x) a.beats[k] = a.rbeats[found - 1 - k];
}

// the tick of time t: -1 for NaN; grid steps of `step` ticks, clamped in f64 before the conversion
__device__ __forceinline__ int beat_tick(double t, const int32_t* beats, int K, int n0, double fps, int grid, int step) {
#pragma clang fp contract(off)
    if (t != t) return -1;
    double v;
    if (K < 2) {
        v = rint(t * (double)(2 * BEAT_TICKS_PER_BEAT));
        v = v > 0.0 ? v : 0.0;
        v = v < (double)(1 << 29) ? v : (double)(1 << 29);
        return (int)v;
    }
    const double x = t * fps;
    int lo = 0, hi = K - 1;                                                // the largest i with beats[i] <= x, 0 if there is none
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((double)beats[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    const int i = min(lo, K - 2);
    const double b = (double)beats[i], d = (double)(beats[i + 1] - beats[i]);
    const double pos = (double)(n0 + i) + (x - b) / d;
    v = rint(pos * (double)grid);
    v = v > 0.0 ? v : 0.0;
    v = v < (double)(1 << 20) ? v : (double)(1 << 20);
    return (int)v * step;
}

__global__ __launch_bounds__(BEAT_THREADS) void beat_positions_kernel(BeatPositionArgs a) {
    const long long i = (long long)blockIdx.x * BEAT_THREADS + threadIdx.x;
    if (i >= a.n) return;
    int2 out = make_int2(-1, -1);
    if (i < note_live_count(a.n, a.count)) {
        const DetokNote r = a.notes[i];
        const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
        if (c.counted) {
            const long long found = a.result[0];
            const int K = (int)(found < 0 ? 0 : (found < a.max_beats ? found : a.max_beats));
            const int grid = a.divisions ? a.divisions : BEAT_TICKS_PER_BEAT, step = K >= 2 ? BEAT_TICKS_PER_BEAT / grid : 1;
            int n0 = 0;
            if (K >= 2) {
                const int d = a.beats[1] - a.beats[0];
                n0 = (a.beats[0] + d - 1) / d;
            }
            out.x = beat_tick(r.onset, a.beats, K, n0, a.frames_per_second, grid, step);
            out.y = beat_tick(r.offset, a.beats, K, n0, a.frames_per_second, grid, step);
            if (!c.drum) out.y = max(out.y, out.x + step);
        }
    }
    reinterpret_cast<int2*>(a.ticks)[i] = out;
}

}  // namespace

int launch_track_beats(const BeatArgs& a, hipStream_t stream) {
    if (a.n_programs < 1 || a.n_programs > BEAT_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -1;
    if (a.lag_min < BEAT_MIN_LAG || a.lag_min > a.lag_max || a.lag_max > BEAT_MAX_LAG || a.window < 2 * a.lag_max || a.window > BEAT_MAX_WINDOW) return -2;
    if (a.hop < 1 || a.hop > a.window || a.lag_step < 0 || a.onset_cap < 1 || a.onset_cap > 255 || !(a.frames_per_second > 0.0)) return -3;
    if (a.n_frames < 1 || a.n_frames > BEAT_MAX_FRAMES || a.n < 0 || a.n > BEAT_MAX_NOTES || (a.n && !a.notes)) return -4;
    if (!a.prior || !a.pen || !a.env || !a.smooth || !a.tgram || !a.lag_back || !a.lags || !a.back || !a.rbeats || !a.beats || !a.result) return -5;
    if (a.max_beats < beat_max_beats(a.n_frames, a.lag_min)) return -6;
    const unsigned frame_blocks = (unsigned)((a.n_frames + BEAT_THREADS - 1) / BEAT_THREADS);
    beat_clear_kernel<<<frame_blocks, BEAT_THREADS, 0, stream>>>(a);
    if (a.n) beat_envelope_kernel<<<(unsigned)((a.n + BEAT_THREADS - 1) / BEAT_THREADS), BEAT_THREADS, 0, stream>>>(a);
    beat_smooth_kernel<<<frame_blocks, BEAT_THREADS, 0, stream>>>(a);
    beat_tempogram_kernel<<<(unsigned)beat_windows(a.n_frames, a.hop), BEAT_THREADS, 0, stream>>>(a);
    beat_tempo_path_kernel<<<1, BEAT_PATH_THREADS, 0, stream>>>(a);
    const int G = (a.lag_min + 1) / 2, n_waves = G < BEAT_DP_WAVES ? G : BEAT_DP_WAVES;
    beat_dp_kernel<<<1, n_waves * WAVE, 0, stream>>>(a, G, n_waves);
    return 0;
}

int launch_beat_positions(const BeatPositionArgs& a, hipStream_t stream) {
    if (a.n_programs < 1 || a.n_programs > BEAT_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -1;
    if (a.divisions < 0 || (a.divisions && BEAT_TICKS_PER_BEAT % a.divisions) || !(a.frames_per_second > 0.0)) return -2;
    if (a.n < 0 || a.n > BEAT_MAX_NOTES || a.max_beats < 1) return -3;
    if (a.n == 0) return 0;
    if (!a.notes || !a.ticks || !a.beats || !a.result) return -4;
    beat_positions_kernel<<<(unsigned)((a.n + BEAT_THREADS - 1) / BEAT_THREADS), BEAT_THREADS, 0, stream>>>(a);
    return 0;
}
