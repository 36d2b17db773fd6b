// Device detokeniser: token ids -> notes (include/ymt3.h, device detokeniser).  The specification is the host path,
// NoteEventTokenizer.decode_segment + note_events_to_notes (yourmt3_amd/task_manager.py); tests/detok_model.py states this file's
// algorithm in plain Python.  Integer work plus one f64 divide and add per event time; nothing here rounds differently from the host.
//
// (a) detok_rows_kernel, one wave per (channel, segment) row of L columns.  decode_segment is a scan: `step` is the prefix sum of
//     the shift values, velocity and program are "last writer" (initially 1 and 0), in_tie ends at the first TIE or SHIFT, and the
//     row ends at the first PAD / EOS.  Lane l owns the ceil(L / 64) consecutive columns from l * ceil(L / 64): a lane-local pass
//     gives its aggregates, wave operations (__shfl_up for the sum, ballots for the flags and the last writers) give every lane
//     its entry state, a second pass counts what the lane yields and the invalid tokens, a prefix count ranks the lanes, a third
//     pass writes the items.  A row owns L item slots (it cannot yield more), so items land in column order without an atomic.
// (b) detok_notes_kernel, one workgroup per channel.  The merge state of note_events_to_notes is per (program, pitch) key and keys
//     do not interact: a counting sort over the n_programs * 128 keys (32-bit LDS counters) buckets the channel's items, scattered
//     segment by segment so that a bucket is in segment order; one lane per key then orders its bucket (an insertion pass that
//     only ever moves items inside one segment's group) and walks it with the host's rules.
// (c) detok_notes_carry_kernel, the incremental form of (b): the same bucketing, and per-key walks that start from the state an
//     earlier call left (the sounding note of a pitched key, the held hits of a drum pitch) and store it back.
#include "common.h"
#include "kernels.h"

namespace {

enum { CLS_INVALID = 0, CLS_STOP, CLS_SKIP, CLS_SHIFT, CLS_PITCH, CLS_VELOCITY, CLS_TIE, CLS_PROGRAM, CLS_DRUM };

constexpr int NOTES_THREADS = 1024;
constexpr unsigned long long NOT_TIE = 1ull << 43;

__device__ __forceinline__ unsigned long long pack_item(int seg, bool tie, int step, int vel, int col) {
    return ((unsigned long long)seg << 44) | (tie ? 0ull : NOT_TIE) | ((unsigned long long)step << 16) | ((unsigned long long)vel << 15) |
           (unsigned long long)col;
}
__device__ __forceinline__ int item_seg(unsigned long long x) { return (int)(x >> 44); }
__device__ __forceinline__ int item_step(unsigned long long x) { return (int)((x >> 16) & 0x7ffffffull); }
__device__ __forceinline__ int item_vel(unsigned long long x) { return (int)((x >> 15) & 1ull); }
__device__ __forceinline__ int item_col(unsigned long long x) { return (int)(x & 0x7fffull); }

// the host's `start_sec + step / steps_per_second`: that division and that add in f64, nothing contracted or reciprocal
__device__ __forceinline__ double event_time(const DetokArgs& a, int seg, int step) {
#pragma clang fp contract(off)
    const double d = (double)step / (double)a.steps_per_second;
    return a.start[seg] + d;
}

// One lane's columns [c0, c1) from its entry state.  EMIT = false: -> number of items, `bad` counts the invalid tokens;
// EMIT = true: writes them from slot `out` on.
template <bool EMIT>
__device__ __forceinline__ int walk_columns(const uint16_t* ent, int c0, int c1, int step, int vel, int prog, bool in_tie, int drum_program,
                                            int seg, unsigned long long* items, uint16_t* keys, long long out, int& bad) {
    int n = 0;
    for (int c = c0; c < c1; ++c) {
        const int e = ent[c], cls = e >> 12, v = e & 0xfff;
        if (cls == CLS_STOP) break;
        int key = -1, ivel = 1;
        bool tie = false;
        switch (cls) {
        case CLS_INVALID: ++bad; break;
        case CLS_SHIFT: in_tie = false; step += v; break;
        case CLS_VELOCITY: vel = v; break;
        case CLS_TIE: in_tie = false; break;
        case CLS_PROGRAM: prog = v; break;
        case CLS_PITCH:
            if (prog == drum_program) {                 // a drum hit: no ties, no offsets
                if (in_tie) ++bad;
                else if (vel) key = prog * DETOK_PITCHES + v;
            } else {
                key = prog * DETOK_PITCHES + v;
                tie = in_tie;
                ivel = vel ? 1 : 0;
            }
            break;
        case CLS_DRUM:
            if (in_tie) ++bad;
            else key = drum_program * DETOK_PITCHES + v;
            break;
        default: break;                                 // CLS_SKIP
        }
        if (key >= 0) {
            if (EMIT) {
                items[out + n] = pack_item(seg, tie, tie ? 0 : step, tie ? 0 : ivel, c);
                keys[out + n] = (uint16_t)key;
            }
            ++n;
        }
    }
    return n;
}

__global__ __launch_bounds__(WAVE) void detok_rows_kernel(DetokArgs a) {
    extern __shared__ uint16_t ent[];                   // [L] the row's table entries
    const int row = blockIdx.x, ch = row / a.n_seg, seg = row % a.n_seg, lane = threadIdx.x;
    const int32_t* tok = a.tokens + (long long)seg * a.seg_stride + (long long)ch * a.chan_stride;
    for (int i = lane; i < a.L; i += WAVE) {
        const int t = tok[i];
        ent[i] = (t >= 0 && t < a.vocab) ? a.table[t] : (uint16_t)0;      // an id outside the vocabulary is invalid
    }
    __syncthreads();
    const int per = (a.L + WAVE - 1) / WAVE;
    const int c0 = min(lane * per, a.L), c1 = min(c0 + per, a.L);
    // lane-local aggregates, up to the lane's first stop token
    int sum = 0, lvel = -1, lprog = -1;
    bool opened = false, stop = false;
    for (int c = c0; c < c1; ++c) {
        const int e = ent[c], cls = e >> 12, v = e & 0xfff;
        if (cls == CLS_STOP) { stop = true; break; }
        if (cls == CLS_SHIFT) { sum += v; opened = true; }
        else if (cls == CLS_TIE) opened = true;
        else if (cls == CLS_VELOCITY) lvel = v;
        else if (cls == CLS_PROGRAM) lprog = v;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool dead = (__ballot(stop) & below) != 0ull;               // a lower lane ended the row (the lanes below the first stop are all live)
    int incl = sum;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int u = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += u;
    }
    const int step0 = incl - sum;
    const bool in_tie0 = (__ballot(opened) & below) == 0ull;
    const unsigned long long vm = __ballot(lvel >= 0) & below, pm = __ballot(lprog >= 0) & below;
    const int vsrc = __shfl(lvel, vm ? 63 - __clzll((long long)vm) : 0, WAVE), psrc = __shfl(lprog, pm ? 63 - __clzll((long long)pm) : 0, WAVE);
    const int vel0 = vm ? vsrc : 1, prog0 = pm ? psrc : 0;
    int bad = 0;
    const int n = dead ? 0 : walk_columns<false>(ent, c0, c1, step0, vel0, prog0, in_tie0, a.drum_program, seg, nullptr, nullptr, 0, bad);
    int rank = n, nbad = bad;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int u = __shfl_up(rank, o, WAVE);
        if (lane >= o) rank += u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, WAVE);
    if (lane == WAVE - 1) a.row_count[row] = rank;                      // rank <= L: a column yields at most one item
    if (lane == 0 && nbad) atomicAdd(&a.counts[1], nbad);
    if (n) walk_columns<true>(ent, c0, c1, step0, vel0, prog0, in_tie0, a.drum_program, seg, a.items, a.keys, (long long)row * a.L + (rank - n), bad);
}

__device__ __forceinline__ void emit_note(const DetokArgs& a, double on, double off, int prog, int pitch, int drum, float score) {
    const int i = atomicAdd(&a.counts[0], 1);
    if (i < a.capacity) a.notes[i] = DetokNote{on, off, prog, pitch, drum, score};
}

__device__ __forceinline__ float item_score(const DetokArgs& a, int ch, unsigned long long x) {
    if (!a.scores) return __uint_as_float(0x7fc00000u);
    return a.scores[(long long)item_seg(x) * a.seg_stride + (long long)ch * a.chan_stride + item_col(x)];
}

// pitched key: the host's active / tie / re-trigger / offset rules over the bucket S[b, e), ordered by the packed item
__device__ void walk_pitched(const DetokArgs& a, int ch, int prog, int pitch, const unsigned long long* S, long long b, long long e) {
    bool active = false;
    double on = 0.0;
    float score = 0.f;
    int q = 0;                                                          // the last segment that confirmed the note
    for (long long i = b; i < e; ++i) {
        const unsigned long long x = S[i];
        const int s = item_seg(x);
        const bool tie = !(x & NOT_TIE);
        if (active && s > q) {
            if (tie && s == q + 1) { q = s; continue; }
            const double end = a.start[q + 1];                          // no tie in segment q + 1: the note ends at its start
            if (end > on) emit_note(a, on, end, prog, pitch, 0, score);
            active = false;
        }
        if (tie) continue;
        const double t = event_time(a, s, item_step(x));
        if (item_vel(x)) {
            if (active && t > on) emit_note(a, on, t, prog, pitch, 0, score);
            active = true; on = t; score = item_score(a, ch, x); q = s;
        } else if (active) {
            if (t > on) emit_note(a, on, t, prog, pitch, 0, score);
            active = false;
        }
    }
    if (active) {
        const double end = q != a.n_seg - 1 ? a.start[q + 1] : a.end_sec;
        if (end > on) emit_note(a, on, end, prog, pitch, 0, score);
    }
}

// drum key: one note per distinct time; the bucket is re-ordered by (time, processing order) so that equal times are neighbours (a
// shift may run past the next segment's start: segment-and-step order is not time order).  The first hit's score stands unless a later
// one compares greater -- a NaN neither replaces nor is replaced.
__device__ void walk_drum(const DetokArgs& a, int ch, int prog, int pitch, unsigned long long* S, long long b, long long e) {
    double tprev = event_time(a, item_seg(S[b]), item_step(S[b]));
    for (long long i = b + 1; i < e; ++i) {
        const unsigned long long x = S[i];
        const double t = event_time(a, item_seg(x), item_step(x));
        if (t >= tprev) { tprev = t; continue; }                        // (equal times keep their processing order: x is the later item)
        long long j = i;
        while (j > b) {
            const unsigned long long y = S[j - 1];
            if (!(event_time(a, item_seg(y), item_step(y)) > t)) break;
            S[j] = y;
            --j;
        }
        S[j] = x;
    }
    long long i = b;
    while (i < e) {
        const unsigned long long x = S[i];
        const double t = event_time(a, item_seg(x), item_step(x));
        float score = item_score(a, ch, x);
        for (++i; i < e; ++i) {
            const unsigned long long y = S[i];
            if (event_time(a, item_seg(y), item_step(y)) != t) break;
            const float sc = item_score(a, ch, y);
            if (sc > score) score = sc;
        }
        double off;
        {
#pragma clang fp contract(off)
            off = t + 0.01;                                             // DRUM_NOTE_SEC
        }
        emit_note(a, t, off, prog, pitch, 1, score);
    }
}

// Bucket one channel's items by key (the counting sort of (b)): on return S is the channel's bucketed copy, the bucket of key k is
// S[koff[k], hist[k]) with its segments in order.  Every thread of the workgroup calls it.
__device__ __forceinline__ void bucket_channel(const DetokArgs& a, int ch, unsigned* hist, unsigned*& koff, unsigned long long*& S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_keys = a.n_programs * DETOK_PITCHES;
    unsigned* wsum = hist + n_keys;
    const long long cbase = (long long)ch * a.n_seg * a.L;              // the channel's slots in items / keys / sorted
    const int* rc = a.row_count + (long long)ch * a.n_seg;
    for (int k = tid; k < n_keys; k += NOTES_THREADS) hist[k] = 0u;
    __syncthreads();
    for (int s = wave; s < a.n_seg; s += NOTES_THREADS / WAVE) {
        const int cnt = rc[s];
        const uint16_t* kp = a.keys + cbase + (long long)s * a.L;
        for (int i = lane; i < cnt; i += WAVE) atomicAdd(&hist[kp[i]], 1u);
    }
    __syncthreads();
    // exclusive scan of the counters: every thread owns `per` consecutive keys
    const int per = (n_keys + NOTES_THREADS - 1) / NOTES_THREADS;
    const int k0 = min(tid * per, n_keys), k1 = min(k0 + per, n_keys);
    unsigned mine = 0u;
    for (int k = k0; k < k1; ++k) mine += hist[k];
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned u = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += u;
    }
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    unsigned off = incl - mine;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    koff = a.key_off + (long long)ch * n_keys;
    for (int k = k0; k < k1; ++k) {
        const unsigned c = hist[k];
        hist[k] = off;
        koff[k] = off;
        off += c;
    }
    __syncthreads();
    // scatter, one segment at a time: a bucket then holds its segments in order (within a segment the order is the atomics')
    S = a.sorted + cbase;
    for (int s = 0; s < a.n_seg; ++s) {
        const int cnt = rc[s];
        const long long rbase = cbase + (long long)s * a.L;
        for (int i = tid; i < cnt; i += NOTES_THREADS) {
            const unsigned pos = atomicAdd(&hist[a.keys[rbase + i]], 1u);
            S[pos] = a.items[rbase + i];
        }
        __syncthreads();
    }
}

// order a bucket by the packed item (an insertion pass that only ever moves items inside one segment's group)
__device__ __forceinline__ void order_bucket(unsigned long long* S, long long b, long long e) {
    unsigned long long prev = S[b];
    for (long long i = b + 1; i < e; ++i) {
        const unsigned long long x = S[i];
        if (x >= prev) { prev = x; continue; }
        long long j = i;
        while (j > b && S[j - 1] > x) { S[j] = S[j - 1]; --j; }
        S[j] = x;
    }
}

__global__ __launch_bounds__(NOTES_THREADS) void detok_notes_kernel(DetokArgs a) {
    extern __shared__ unsigned hist[];                                  // [n_keys] counters, then [16] wave sums
    const int ch = blockIdx.x, tid = threadIdx.x;
    const int n_keys = a.n_programs * DETOK_PITCHES;
    unsigned* koff;
    unsigned long long* S;
    bucket_channel(a, ch, hist, koff, S);
    // one lane per key: order the bucket, then merge.  hist[k] is now the bucket's end.
    for (int k = tid; k < n_keys; k += NOTES_THREADS) {
        const long long b = koff[k], e = hist[k];
        if (b == e) continue;
        order_bucket(S, b, e);
        const int prog = k / DETOK_PITCHES, pitch = k % DETOK_PITCHES;
        if (prog == a.drum_program) walk_drum(a, ch, prog, pitch, S, b, e);
        else walk_pitched(a, ch, prog, pitch, S, b, e);
    }
}

// ---------------------------------------------------------------- incremental form (include/ymt3.h, incremental detokeniser)
// The per-key walks of (b) with their state carried between calls (tests/live_model.py states them in plain Python).  Segment indices
// are those of the push: the last segment of the previous push is segment -1.

// pitched key: walk_pitched starting from the carried note and storing back what still sounds after the push's last segment
__device__ void walk_pitched_carry(const DetokArgs& a, const DetokCarryArgs& c, int ch, int k, const unsigned long long* S, long long b, long long e) {
    const int prog = k / DETOK_PITCHES, pitch = k % DETOK_PITCHES;
    DetokSounding& st = c.sounding[(long long)ch * a.n_programs * DETOK_PITCHES + k];
    bool active = st.valid != 0;
    double on = st.onset;
    float score = st.score;
    if (a.n_seg > 0) {
        int q = -1;                                                     // the last segment that confirmed the note
        for (long long i = b; i < e; ++i) {
            const unsigned long long x = S[i];
            const int s = item_seg(x);
            const bool tie = !(x & NOT_TIE);
            if (active && s > q) {
                if (tie && s == q + 1) { q = s; continue; }
                const double end = a.start[q + 1];                      // no tie in segment q + 1: the note ends at its start
                if (end > on) emit_note(a, on, end, prog, pitch, 0, score);
                active = false;
            }
            if (tie) continue;
            const double t = event_time(a, s, item_step(x));
            if (item_vel(x)) {
                if (active && t > on) emit_note(a, on, t, prog, pitch, 0, score);
                active = true; on = t; score = item_score(a, ch, x); q = s;
            } else if (active) {
                if (t > on) emit_note(a, on, t, prog, pitch, 0, score);
                active = false;
            }
        }
        if (active && q != a.n_seg - 1) {                               // a later segment of this push did not tie it
            const double end = a.start[q + 1];
            if (end > on) emit_note(a, on, end, prog, pitch, 0, score);
            active = false;
        }
    }
    if (active && c.finish) {
        if (a.end_sec > on) emit_note(a, on, a.end_sec, prog, pitch, 0, score);
        active = false;
    }
    st.onset = on; st.score = score; st.valid = active ? 1 : 0;
}

// drum key: the held hits (distinct times, ascending; earlier in processing order than anything new) merged with the push's bucket.
// Hits below the horizon leave; the others are held again, at most max_held of them: the earliest surplus ones leave too and count as
// forced.  Pass 0 counts, pass 1 emits and stores.
__device__ void walk_drum_carry(const DetokArgs& a, const DetokCarryArgs& c, int ch, int prog, int pitch, unsigned long long* S, long long b, long long e) {
    if (e > b) {
        double tprev = event_time(a, item_seg(S[b]), item_step(S[b]));
        for (long long i = b + 1; i < e; ++i) {
            const unsigned long long x = S[i];
            const double t = event_time(a, item_seg(x), item_step(x));
            if (t >= tprev) { tprev = t; continue; }
            long long j = i;
            while (j > b) {
                const unsigned long long y = S[j - 1];
                if (!(event_time(a, item_seg(y), item_step(y)) > t)) break;
                S[j] = y;
                --j;
            }
            S[j] = x;
        }
    }
    const long long slot = (long long)ch * DETOK_PITCHES + pitch;
    const DetokHeld* Hin = c.held_in + slot * c.max_held;
    DetokHeld* Hout = c.held_out + slot * c.max_held;
    const int nh = min(max(c.held_count_in[slot], 0), c.max_held);
    int total = 0, below = 0, n_emit = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int i = 0, idx = 0;
        long long j = b;
        while (i < nh || j < e) {
            const double tj = j < e ? event_time(a, item_seg(S[j]), item_step(S[j])) : 0.0;
            const bool take_held = i < nh && (j >= e || Hin[i].time <= tj);
            const bool take_new = j < e && (!take_held || tj == Hin[i].time);
            const double t = take_held ? Hin[i].time : tj;
            float score = 0.f;
            if (pass) score = take_held ? Hin[i].score : item_score(a, ch, S[j]);
            if (take_held) ++i;
            if (take_new) {
                if (pass && take_held) { const float sc = item_score(a, ch, S[j]); if (sc > score) score = sc; }
                for (++j; j < e; ++j) {
                    const unsigned long long y = S[j];
                    if (event_time(a, item_seg(y), item_step(y)) != t) break;
                    if (pass) { const float sc = item_score(a, ch, y); if (sc > score) score = sc; }
                }
            }
            if (!pass) {
                ++total;
                if (t < c.horizon) ++below;
            } else if (idx < n_emit) {
                double off;
                {
#pragma clang fp contract(off)
                    off = t + 0.01;                                     // DRUM_NOTE_SEC
                }
                emit_note(a, t, off, prog, pitch, 1, score);
            } else {
                Hout[idx - n_emit] = DetokHeld{t, score, 0};
            }
            ++idx;
        }
        if (!pass) {
            const int forced = max(0, total - below - c.max_held);
            n_emit = below + forced;
            if (forced) atomicAdd(&a.counts[2], forced);
        }
    }
    c.held_count_out[slot] = total - n_emit;
}

__global__ __launch_bounds__(NOTES_THREADS) void detok_notes_carry_kernel(DetokArgs a, DetokCarryArgs c) {
    extern __shared__ unsigned hist[];                                  // [n_keys] counters, then [16] wave sums
    const int ch = blockIdx.x, tid = threadIdx.x;
    const int n_keys = a.n_programs * DETOK_PITCHES;
    unsigned* koff = nullptr;
    unsigned long long* S = nullptr;
    if (a.n_seg > 0) bucket_channel(a, ch, hist, koff, S);             // (uniform over the grid)
    for (int k = tid; k < n_keys; k += NOTES_THREADS) {
        const long long b = a.n_seg > 0 ? koff[k] : 0, e = a.n_seg > 0 ? hist[k] : 0;
        if (e > b) order_bucket(S, b, e);
        const int prog = k / DETOK_PITCHES, pitch = k % DETOK_PITCHES;
        if (prog == a.drum_program) walk_drum_carry(a, c, ch, prog, pitch, S, b, e);
        else walk_pitched_carry(a, c, ch, k, S, b, e);
    }
}

constexpr size_t NOTES_LDS_MAX = (size_t)DETOK_MAX_PROGRAMS * DETOK_PITCHES * sizeof(unsigned) + (NOTES_THREADS / WAVE) * sizeof(unsigned);

}  // namespace

int init_detok_kernels() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(detok_notes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NOTES_LDS_MAX) !=
               hipSuccess ||
           hipFuncSetAttribute(reinterpret_cast<const void*>(detok_notes_carry_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)NOTES_LDS_MAX) != hipSuccess;
}

int launch_detok_carry(const DetokArgs& a, const DetokCarryArgs& c, hipStream_t stream) {
    if (a.n_seg < 0 || a.n_chan <= 0) return 0;
    if (a.n_seg > 0 && (a.L <= 0 || a.L > DETOK_MAX_STEPS || a.n_seg > DETOK_MAX_SEGMENTS)) return -1;
    if (a.n_programs <= 0 || a.n_programs > DETOK_MAX_PROGRAMS || a.drum_program >= a.n_programs || c.max_held < 1) return -2;
    if ((long long)a.n_seg * a.n_chan > 0x7fffffffLL || (long long)a.n_seg * a.L > 0xffffffffLL) return -3;
    const size_t lds = (size_t)a.n_programs * DETOK_PITCHES * sizeof(unsigned) + (NOTES_THREADS / WAVE) * sizeof(unsigned);
    if (a.n_seg > 0) detok_rows_kernel<<<a.n_seg * a.n_chan, WAVE, (size_t)a.L * sizeof(uint16_t), stream>>>(a);
    detok_notes_carry_kernel<<<a.n_chan, NOTES_THREADS, lds, stream>>>(a, c);
    return 0;
}

int launch_detok(const DetokArgs& a, hipStream_t stream) {
    if (a.n_seg <= 0 || a.n_chan <= 0) return 0;
    if (a.L <= 0 || a.L > DETOK_MAX_STEPS || a.n_seg > DETOK_MAX_SEGMENTS) return -1;
    if (a.n_programs <= 0 || a.n_programs > DETOK_MAX_PROGRAMS || a.drum_program >= a.n_programs) return -2;
    if ((long long)a.n_seg * a.n_chan > 0x7fffffffLL || (long long)a.n_seg * a.L > 0xffffffffLL) return -3;
    const size_t lds = (size_t)a.n_programs * DETOK_PITCHES * sizeof(unsigned) + (NOTES_THREADS / WAVE) * sizeof(unsigned);
    detok_rows_kernel<<<a.n_seg * a.n_chan, WAVE, (size_t)a.L * sizeof(uint16_t), stream>>>(a);
    detok_notes_kernel<<<a.n_chan, NOTES_THREADS, lds, stream>>>(a);
    return 0;
}
