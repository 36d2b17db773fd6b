// Bars and key over note records and tracked beats: per-beat accents and pitch-class content, a salience per beat, a Viterbi over
// (metre, place in the bar), and one key per file (include/ymt3.h, bars and key).  The specification is the host path, track_bars of
// yourmt3_amd/bars.py; tests/bar_model.py states the rules as plain loops.  Everything is an integer (times stay f64 until they are known
// to lie inside the slots or the frames): every output equals the host's.
// The number of beats K is read from the beat tracker's result on the device, so every launch is sized by the object's max_beats or by
// the number of records, and nothing is read back.
// (a) bar_clear_kernel zeroes a[0, K), c[0, K)[12], the accumulators and result[8].
// (b) bar_features_kernel, one lane per record: classifies it by the rule every note consumer uses (note_rule.h), finds its slot by a
//     binary search over the slots' lower edges (computed on the fly from the beats), adds its accent to a[slot] and, for a pitched
//     record, walks the slots its span overlaps and adds the shared frames to c[slot][pitch class] and their sum to tot[pitch class].
//     Integer atomicAdd: exact in any order.
// (c) bar_salience_kernel, one lane per beat: the cap, the two normalised chroma rows, h and d; a shuffle butterfly and one LDS round
//     give the block's sum of d, one atomicAdd per block the file's.
// (d) bar_key_kernel, one wave: lane j < 24 takes the dot product of (mode, tonic) j; two butterflies give the best and the second best.
// (e) bar_path_kernel, one wave, the serial spine: one lane per state (at most 20), V in a register.  d[] is fetched 64 beats at a time
//     by the lanes and broadcast with __shfl; a step takes the predecessor's V from the lane below and every metre's last state by
//     __shfl; those are uniform, so every lane works out all downbeat choices (3 bits per metre) and lane j of the chunk keeps beat j's
//     word: one coalesced store per chunk.  Lane 0 follows the choices back and writes metre[].  Written and read by one workgroup,
//     ordered by __syncthreads.
// No kernel waits on another workgroup and nothing spins.
#include <climits>

#include "common.h"
#include "kernels.h"
#include "beat_slots.h"
#include "note_rule.h"

namespace {

constexpr int BAR_THREADS = 256;
constexpr int BAR_CLEAR_BLOCKS = 256;

__device__ const int BAR_KEY_TABLE[2][12] = {{671, -293, -1, -270, 210, 142, -225, 400, -256, 42, -279, -141},
                                             {671, -263, -48, 428, -284, -46, -299, 266, 69, -261, -94, -138}};

__global__ __launch_bounds__(BAR_THREADS) void bar_clear_kernel(BarArgs a) {
    const long long stride = (long long)gridDim.x * BAR_THREADS, t0 = (long long)blockIdx.x * BAR_THREADS + threadIdx.x;
    const long long K = beat_count(a.beat_result, a.max_beats);
    for (long long i = t0; i < K * 12; i += stride) a.chroma[i] = 0u;
    for (long long i = t0; i < K; i += stride) a.accent[i] = 0u;
    if (t0 < BAR_ACC_WORDS) a.acc[t0] = 0ull;
    if (t0 < 8) a.result[t0] = 0;
}

__global__ __launch_bounds__(BAR_THREADS) void bar_features_kernel(BarArgs a) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * BAR_THREADS + threadIdx.x;
    if (i >= note_live_count(a.n, a.count)) return;
    const DetokNote r = a.notes[i];
    const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
    if (!c.counted) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[6]), 1ull);
        return;
    }
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2) return;
    const BeatSlots sl = {a.beats, K, a.near_div};
    const long long e0 = slot_edge(sl, 0), eK = slot_edge(sl, K);
    const double f0 = rint(r.onset * a.frames_per_second);
    if (f0 >= (double)e0 && f0 < (double)eK) {                             // finite, and inside the slots
        const long long F = (long long)f0;
        const int s = slot_of(sl, F);
        const int D = slot_delta(sl, s);
        if (F <= (long long)sl.b[s] + D / sl.nd) {
            unsigned w = 1u;
            if (c.drum && r.pitch >= a.kick_lo && r.pitch <= a.kick_hi) w += (unsigned)a.w_kick;
            if (!c.drum && rint(r.offset * a.frames_per_second) - f0 >= (double)D) w += (unsigned)a.w_long;
            atomicAdd(&a.accent[s], w);
        }
    }
    long long lo, hi;
    if (c.drum || !note_frame_span(r, false, a.frames_per_second, a.n_frames, &lo, &hi)) return;
    if (hi <= e0 || lo >= eK) return;
    const int pc = r.pitch % 12;
    unsigned long long total = 0ull;
    slot_walk(sl, lo, hi, [&](int s, long long share, long long) {
        atomicAdd(&a.chroma[(long long)s * 12 + pc], (unsigned)share);
        total += (unsigned long long)share;
    });
    if (total) atomicAdd(&a.acc[pc], total);
}

__global__ __launch_bounds__(BAR_THREADS) void bar_salience_kernel(BarArgs a) {
    __shared__ long long part[BAR_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const long long s = (long long)blockIdx.x * BAR_THREADS + tid;
    const int K = beat_count(a.beat_result, a.max_beats);
    long long d = 0;
    if (K >= 2 && s < K) {
        const unsigned acc = min(a.accent[s], (unsigned)a.accent_cap);
        long long h = 0;
        if (s > 0) {
            unsigned long long cur[12], prev[12], sc = 0ull, sp = 0ull;
#pragma unroll
            for (int pc = 0; pc < 12; ++pc) {
                cur[pc] = a.chroma[s * 12 + pc];
                prev[pc] = a.chroma[(s - 1) * 12 + pc];
                sc += cur[pc];
                sp += prev[pc];
            }
            if (sc && sp) {
#pragma unroll
                for (int pc = 0; pc < 12; ++pc) {
                    const long long x = (long long)(cur[pc] * 1024ull / sc) - (long long)(prev[pc] * 1024ull / sp);
                    h += x < 0 ? -x : x;
                }
            }
        }
        d = (long long)a.w_accent * acc + h;
        a.salience[s] = (int32_t)d;
    }
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) d += __shfl_xor(d, x, WAVE);
    if (lane == 0) part[wave] = d;
    __syncthreads();
    if (tid == 0) {
        long long sum = 0;
        for (int w = 0; w < BAR_THREADS / WAVE; ++w) sum += part[w];
        if (sum) atomicAdd(&a.acc[12], (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(WAVE) void bar_key_kernel(BarArgs a) {
    const int lane = threadIdx.x;
    long long tot[12], all = 0;
#pragma unroll
    for (int pc = 0; pc < 12; ++pc) {
        tot[pc] = (long long)a.acc[pc];
        all += tot[pc];
    }
    long long S = LLONG_MIN;
    if (lane < 24) {
        const int mode = lane / 12, t = lane % 12;
        S = 0;
#pragma unroll
        for (int pc = 0; pc < 12; ++pc) S += tot[pc] * BAR_KEY_TABLE[mode][(pc - t + 12) % 12];
    }
    long long best = S;
    int key = lane;
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {                                      // major before minor, then the smaller tonic: the smaller lane keeps a tie
        const long long ov = __shfl_xor(best, x, WAVE);
        const int ok = __shfl_xor(key, x, WAVE);
        if (ov > best || (ov == best && ok < key)) { best = ov; key = ok; }
    }
    long long second = lane == key ? LLONG_MIN : S;
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const long long ov = __shfl_xor(second, x, WAVE);
        second = ov > second ? ov : second;
    }
    if (lane == 0) {
        a.result[3] = all ? key : -1;
        a.result[4] = all ? best : 0;
        a.result[5] = all ? second : 0;
    }
}

__global__ __launch_bounds__(WAVE) void bar_path_kernel(BarArgs a) {
    const int lane = threadIdx.x;
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2) return;                                                     // result[0 .. 2] stay 0
    const int nM = a.n_metres;
    int m[BAR_MAX_METRES], first[BAR_MAX_METRES], last[BAR_MAX_METRES];
    int nS = 0, my_q = -1, my_k = 0, my_m = 1;
#pragma unroll
    for (int q = 0; q < BAR_MAX_METRES; ++q) {
        m[q] = q < nM ? a.metres[q] : 1;
        first[q] = nS;
        last[q] = nS + m[q] - 1;
        if (q < nM) {
            if (lane >= nS && lane < nS + m[q]) { my_q = q; my_k = lane - nS; my_m = m[q]; }
            nS += m[q];
        }
    }
    const bool active = my_q >= 0, down = active && my_k == 0;
    const long long gain = !active ? 0 : (down ? (long long)(60 / my_m) * (my_m - 1) : -(long long)(60 / my_m));
    const long long mean_d = (long long)(a.acc[12] / (unsigned long long)K);
    const long long P = (long long)a.switch_cost * 60 * mean_d;
    long long V = 0;
    for (int i0 = 0; i0 < K; i0 += WAVE) {
        const int chunk = i0 + lane < K ? a.salience[i0 + lane] : 0;
        const int nj = min(WAVE, K - i0);
        unsigned mine = 0u;
        for (int j = 0; j < nj; ++j) {
            const long long d = __shfl(chunk, j, WAVE);
            if (i0 + j == 0) {
                V = gain * d;
                continue;
            }
            const long long below = __shfl(V, lane > 0 ? lane - 1 : 0, WAVE);
            long long ends[BAR_MAX_METRES];
#pragma unroll
            for (int q = 0; q < BAR_MAX_METRES; ++q) ends[q] = __shfl(V, last[q], WAVE);
            unsigned packed = 0u;
            long long nv = below;
#pragma unroll
            for (int q = 0; q < BAR_MAX_METRES; ++q) {
                if (q < nM) {
                    long long best = ends[q];
                    int arg = q;
#pragma unroll
                    for (int q2 = 0; q2 < BAR_MAX_METRES; ++q2)            // only a strictly larger value takes over: staying, then the earliest m'
                        if (q2 < nM && q2 != q && ends[q2] - P > best) { best = ends[q2] - P; arg = q2; }
                    packed |= (unsigned)arg << (3 * q);
                    if (down && q == my_q) nv = best;
                }
            }
            V = active ? nv + gain * d : 0;
            if (lane == j) mine = packed;
        }
        if (i0 + lane < K) a.choice[i0 + lane] = (unsigned short)mine;
    }
    __syncthreads();
    long long top = active ? V : LLONG_MIN;
    int end = lane;
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {                                      // the first state in state order keeps a tie
        const long long ov = __shfl_xor(top, x, WAVE);
        const int oe = __shfl_xor(end, x, WAVE);
        if (ov > top || (ov == top && oe < end)) { top = ov; end = oe; }
    }
    if (lane == 0) {
        int q = 0, k = 0;
#pragma unroll
        for (int x = 0; x < BAR_MAX_METRES; ++x)
            if (x < nM && end >= first[x] && end <= last[x]) { q = x; k = end - first[x]; }
        long long downs = 0;
        for (int i = K - 1; i >= 0; --i) {
            int mq = m[0];
#pragma unroll
            for (int x = 1; x < BAR_MAX_METRES; ++x) mq = x == q ? m[x] : mq;
            a.metre[i] = 256 * mq + k;
            if (k) {
                --k;
            } else {
                ++downs;
                const int c = (a.choice[i] >> (3 * q)) & 7;
                q = c < nM ? c : 0;
                k = m[0] - 1;
#pragma unroll
                for (int x = 1; x < BAR_MAX_METRES; ++x) k = x == q ? m[x] - 1 : k;
            }
        }
        a.result[0] = downs;
        a.result[1] = top;
        a.result[2] = mean_d;
    }
}

}  // namespace

int launch_track_bars(const BarArgs& a, hipStream_t stream) {
    if (int e = slot_check_programs(a)) return e;
    if (a.n_metres < 1 || a.n_metres > BAR_MAX_METRES) return -2;
    int states = 0;
    for (int q = 0; q < a.n_metres; ++q) {
        if (a.metres[q] < BAR_MIN_METRE || a.metres[q] > BAR_MAX_METRE) return -2;
        states += a.metres[q];
    }
    if (states > WAVE) return -2;
    if (a.accent_cap < 1 || a.accent_cap > 255 || a.w_long < 0 || a.w_kick < 0 || a.w_accent < 0 || a.switch_cost < 0) return -3;
    if (int e = slot_check_call(a)) return e;
    if (!a.accent || !a.salience || !a.choice || !a.acc || !a.metre) return -6;
    const unsigned beat_blocks = (unsigned)((a.max_beats + BAR_THREADS - 1) / BAR_THREADS);
    bar_clear_kernel<<<beat_blocks < (unsigned)BAR_CLEAR_BLOCKS ? beat_blocks : (unsigned)BAR_CLEAR_BLOCKS, BAR_THREADS, 0, stream>>>(a);
    if (a.n) bar_features_kernel<<<(unsigned)((a.n + BAR_THREADS - 1) / BAR_THREADS), BAR_THREADS, 0, stream>>>(a);
    bar_salience_kernel<<<beat_blocks, BAR_THREADS, 0, stream>>>(a);
    bar_key_kernel<<<1, WAVE, 0, stream>>>(a);
    bar_path_kernel<<<1, WAVE, 0, stream>>>(a);
    return 0;
}
