// Device tokeniser: notes -> token ids (include/ymt3.h, device tokeniser), the inverse of detok.hip.  The specification is the host
// path, TaskManager.notes_to_tokens (yourmt3_amd/task_manager.py); tests/tok_model.py states this file's algorithm in plain Python.
// Integer work plus one f64 subtract, multiply and rint per event time; nothing here rounds differently from the host.
//
// (a) tok_items_kernel, one lane per note record.  A binary search of the f64 start times finds the onset's segment, the step is
//     rint((onset - start) * steps_per_second) in f64 with contraction off.  The note yields an onset item, at most one offset item
//     and one tie item per later segment that starts before its offset.  An item is one 64-bit word whose integer order is the
//     host's order of a row (tie section first, then NoteEvent's order: step, is_drum, program, velocity, pitch); equal words are equal
//     items, so the order of the appends does not matter.  Items are appended to the owning (segment, channel) row's L slots through
//     a per-row counter.  A tie is appended only by the lane that sets its bit in a per-segment (program, pitch) bitmap first: a tie
//     section lists a key once, and with that every item in a row yields at least one token -- a row with more than L items has
//     overflowed, so L slots per row always suffice.
// (b) tok_rows_kernel, one wave per row.  A bitonic sort of the row's words in LDS, then encode_segment as scans over the sorted events:
//     lane l owns ceil(E / 64) consecutive events; the previous event's step and velocity are its left neighbour's, the last pitched
//     program before the lane is a "last writer" ballot, a first pass counts the lane's tokens (shifts = ceil(dstep / max_shift_steps), a
//     velocity token where the effective velocity changes, a program token where the last pitched program differs), a prefix sum gives the
//     write position, a second pass writes.  Then EOS and PAD.  A row that needs more than L tokens reports that count and keeps the
//     first L of them.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int ITEM_THREADS = 256;
constexpr unsigned long long BODY = 1ull << 49;          // clear: a tie item (sorts first)
constexpr int STEP_MAX = 2147483646;                     // steps saturate here (a segment of 248 days)

__device__ __forceinline__ unsigned long long pack_item(bool body, int step, int drum, int prog, int vel, int pitch) {
    return (body ? BODY : 0ull) | ((unsigned long long)(unsigned)step << 17) | ((unsigned long long)drum << 16) | ((unsigned long long)prog << 8) |
           ((unsigned long long)vel << 7) | (unsigned long long)pitch;
}
__device__ __forceinline__ int item_step(unsigned long long x) { return (int)((x >> 17) & 0x7fffffffull); }
__device__ __forceinline__ int item_drum(unsigned long long x) { return (int)((x >> 16) & 1ull); }
__device__ __forceinline__ int item_prog(unsigned long long x) { return (int)((x >> 8) & 0xffull); }
__device__ __forceinline__ int item_vel(unsigned long long x) { return (int)((x >> 7) & 1ull); }
__device__ __forceinline__ int item_pitch(unsigned long long x) { return (int)(x & 0x7full); }

// the host's int(round((t - t0) * steps_per_second)): that subtract and that multiply in f64, half to even; negative and NaN give 0
__device__ __forceinline__ int to_step(double t, double t0, int steps_per_second) {
#pragma clang fp contract(off)
    const double d = (t - t0) * (double)steps_per_second;
    const double r = rint(d);
    return r >= (double)STEP_MAX ? STEP_MAX : (r > 0.0 ? (int)r : 0);
}

// bisect_right(start, t) - 1: the last segment that starts at or before t (-1: none)
__device__ __forceinline__ int segment_of(const double* start, int n, double t) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t < start[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

__device__ __forceinline__ void append(const TokArgs& a, int seg, int ch, unsigned long long w) {
    const long long row = (long long)seg * a.n_chan + ch;
    const int pos = atomicAdd(&a.row_count[row], 1);
    if (pos >= 0 && pos < a.L) a.items[row * a.L + pos] = w;
}

__global__ __launch_bounds__(ITEM_THREADS) void tok_items_kernel(TokArgs a) {
    const long long i = (long long)blockIdx.x * ITEM_THREADS + threadIdx.x;
    if (i >= a.n_notes) return;
    const DetokNote r = a.notes[i];
    const bool drum = r.is_drum != 0;
    const int prog = drum ? a.drum_program : r.program, pitch = r.pitch;
    if (!(r.onset >= a.start[0] && r.onset < a.end_sec)) return;       // (a NaN onset too)
    if (prog < 0 || prog >= a.n_programs || pitch < 0 || pitch >= TOK_PITCHES) return;
    if (!drum && r.offset != r.offset) return;
    const int ch = a.program_channel[prog];
    const int s = segment_of(a.start, a.n_seg, r.onset);               // >= 0: start[0] <= onset
    const int step = to_step(r.onset, a.start[s], a.steps_per_second);
    append(a, s, ch, pack_item(true, step, drum, prog, 1, pitch));
    if (drum) return;
    const int key = prog * TOK_PITCHES + pitch;
    for (int s2 = s + 1; s2 < a.n_seg && a.start[s2] < r.offset; ++s2) {
        const unsigned bit = 1u << (key & 31);
        const unsigned old = atomicOr(&a.tie_seen[(long long)s2 * (a.n_programs * (TOK_PITCHES / 32)) + (key >> 5)], bit);
        if (!(old & bit)) append(a, s2, ch, pack_item(false, 0, 0, prog, 0, pitch));
    }
    if (r.offset >= a.end_sec) return;                                  // the detokeniser closes the note at end_sec
    int so = segment_of(a.start, a.n_seg, r.offset), ostep;
    if (so <= s) {                                                      // in (or before) the onset's segment: never at or before the onset
        so = s;
        ostep = to_step(r.offset, a.start[s], a.steps_per_second);
        if (ostep <= step) ostep = step + 1;
    } else {
        if (r.offset == a.start[so]) return;                            // the missing tie closes the note at that boundary
        ostep = to_step(r.offset, a.start[so], a.steps_per_second);
    }
    append(a, so, ch, pack_item(true, ostep, 0, prog, 0, pitch));
}

// One lane's events S[c0, c1) from its entry state -> number of tokens (an event's shifts count as at most L + 1, which already
// overflows the row).  EMIT: writes them from column `pos` on, columns below L only.
template <bool EMIT>
__device__ __forceinline__ int walk_events(const TokArgs& a, const unsigned long long* S, int c0, int c1, int prev_step, int prev_vel, int cur_prog,
                                           int32_t* out, int pos) {
    int n = 0;
    const int L = a.L, ms = a.max_shift_steps;
    auto put = [&](int id) {
        if (EMIT && pos + n < L) out[pos + n] = id;
        ++n;
    };
    for (int c = c0; c < c1; ++c) {
        const unsigned long long x = S[c];
        const int step = item_step(x), drum = item_drum(x), prog = item_prog(x), vel = drum ? 1 : item_vel(x), pitch = item_pitch(x);
        int d = step - prev_step;                                       // >= 0: the events are sorted
        if (d > 0) {
            const int ns = min((d - 1) / ms + 1, L + 1);
            if (EMIT)
                for (int k = 0; k < ns && pos + n + k < L; ++k, d -= ms) out[pos + n + k] = a.shift_base + min(d, ms) - 1;
            n += ns;
        }
        prev_step = step;
        if (vel != prev_vel) {
            put(a.velocity_base + vel);
            prev_vel = vel;
        }
        if (drum) {
            put(a.drum_base + pitch);
            continue;
        }
        if (prog != cur_prog) {
            put(a.program_base + prog);
            cur_prog = prog;
        }
        put(a.pitch_base + pitch);
    }
    return n;
}

__global__ __launch_bounds__(WAVE) void tok_rows_kernel(TokArgs a) {
    extern __shared__ unsigned long long S[];                           // [next power of two >= the row's items]
    const int row = blockIdx.x, lane = threadIdx.x, L = a.L;
    int32_t* out = a.tokens + (long long)row * L;
    const int count = a.row_count[row];
    if (count > L || count < 0) {                                       // more items than slots: every item is at least one token
        for (int i = lane; i < L; i += WAVE) out[i] = a.pad_id;
        if (lane == 0) a.lengths[row] = count < 0 ? 0x7fffffff : count + 2;
        return;
    }
    int N = 1;
    while (N < count) N <<= 1;
    const unsigned long long* src = a.items + (long long)row * L;
    for (int i = lane; i < N; i += WAVE) S[i] = i < count ? src[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (N >> 1); t += WAVE) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));    // bit j clear; the partner is i + j
                const unsigned long long x = S[i], y = S[i + j];
                if ((x > y) == ((i & k) == 0)) {
                    S[i] = y;
                    S[i + j] = x;
                }
            }
            __syncthreads();
        }
    // the tie section: the items without BODY sort first
    int T = 0;
    for (int i = lane; i < count; i += WAVE) T += !(S[i] & BODY);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) T += __shfl_xor(T, o, WAVE);
    for (int i = lane; i < T; i += WAVE) {
        const unsigned long long x = S[i];
        if (2 * i < L) out[2 * i] = a.program_base + item_prog(x);
        if (2 * i + 1 < L) out[2 * i + 1] = a.pitch_base + item_pitch(x);
    }
    if (lane == 0 && 2 * T < L) out[2 * T] = a.tie_base;
    // the events: lane l owns `per` consecutive ones
    const int E = count - T, per = (E + WAVE - 1) / WAVE;
    const int c0 = T + min(lane * per, E), c1 = T + min(lane * per + per, E);
    int lprog = -1;                                                     // the lane's last pitched program
    for (int c = c0; c < c1; ++c)
        if (!item_drum(S[c])) lprog = item_prog(S[c]);
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long pm = __ballot(lprog >= 0) & below;
    const int psrc = __shfl(lprog, pm ? 63 - __clzll((long long)pm) : 0, WAVE);
    const int prog0 = pm ? psrc : -1;                                   // -1: no pitched event yet, the first one emits its program
    int step0 = 0, vel0 = -1;                                           // the first event always emits its velocity
    if (c0 > T && c0 < c1) {
        const unsigned long long p = S[c0 - 1];
        step0 = item_step(p);
        vel0 = item_drum(p) ? 1 : item_vel(p);
    }
    const int n = walk_events<false>(a, S, c0, c1, step0, vel0, prog0, nullptr, 0);
    int incl = n;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int u = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += u;
    }
    const int body = __shfl(incl, WAVE - 1, WAVE);
    const int total = 2 * T + 1 + body + 1;                             // ties, TIE, events, EOS
    if (n) walk_events<true>(a, S, c0, c1, step0, vel0, prog0, out, 2 * T + 1 + incl - n);
    if (lane == 0) a.lengths[row] = total;
    if (total <= L) {
        if (lane == 0) out[total - 1] = a.eos_id;
        for (int i = total + lane; i < L; i += WAVE) out[i] = a.pad_id;
    }
}

}  // namespace

int launch_tok(const TokArgs& a, hipStream_t stream) {
    if (a.n_seg <= 0) return 0;
    if (a.n_chan <= 0 || a.L <= 0 || a.L > TOK_MAX_STEPS || a.n_seg > TOK_MAX_SEGMENTS) return -1;
    if (a.n_programs <= 0 || a.n_programs > TOK_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -2;
    if (a.n_notes < 0 || a.n_notes > TOK_MAX_NOTES || (long long)a.n_seg * a.n_chan > 0x7fffffffLL) return -3;
    if (a.max_shift_steps < 1 || a.steps_per_second < 1) return -4;
    const int rows = a.n_seg * a.n_chan;
    if (hipMemsetAsync(a.row_count, 0, (size_t)rows * sizeof(int), stream) != hipSuccess) return -5;
    if (hipMemsetAsync(a.tie_seen, 0, (size_t)a.n_seg * a.n_programs * (TOK_PITCHES / 8), stream) != hipSuccess) return -5;
    if (a.n_notes > 0)
        tok_items_kernel<<<(unsigned)((a.n_notes + ITEM_THREADS - 1) / ITEM_THREADS), ITEM_THREADS, 0, stream>>>(a);
    int N = 1;
    while (N < a.L) N <<= 1;
    tok_rows_kernel<<<rows, WAVE, (size_t)N * sizeof(unsigned long long), stream>>>(a);
    return 0;
}
