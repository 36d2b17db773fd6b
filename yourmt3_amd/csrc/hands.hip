// Hands over note records: every piano note's hand from a split point that moves with the music (include/ymt3.h, hands).  The
// specification is the host path, split_hands of yourmt3_amd/hands.py; tests/hand_model.py states the rules as plain loops.  Everything
// is an integer (times stay f64 until they are known to lie inside the frames): every output equals the host's.
// The number of slices T stays on the device: every launch is sized by the number of records or is one workgroup, and nothing is read
// back.  Scratch: 20 bytes per slot of the object's ceil(max_frames / slice_frames) (the 128-bit pitch set and the slot -> slice map)
// and 153 bytes per slice of its min(max_notes, slots) (the compacted set, the slot, the 129 back-pointers in 132 bytes, the split).
// (a) hand_clear_kernel zeroes the call's slots' sets, result[8] and the accumulators.
// (b) hand_mark_kernel, one lane per record: the record rule (note_rule.h), the program range, the span's first frame; an atomicOr of the
//     pitch bit into the slot's set; the skipped and the selected records counted.
// (c) hand_compact_kernel, one workgroup: an exclusive scan of the occupied flags, 1024 slots a round (a ballot per wave, the waves'
//     counts through LDS); writes Q_t, P_t densely, the slot -> t map and T.
// (d) hand_path_kernel, the hot one: one workgroup of nine waves, four lanes per state, each taking a quarter of the s'.  A step reads
//     its slice's set (requested one step ahead) and forms e_t(s) and class_t(s) from the bits.  The costs of the step before lie in LDS
//     as keys (C << 8 | s'), so that one unsigned minimum finds the smallest minimiser, three times: plain, with w_switch added where
//     class_{t-1}(s') = 2 (read by the states of class 0) and where it is 0 (read by those of class 2): the inner loop is an LDS read
//     of four keys and per key a distance, a multiply-add and a minimum.  A quarter's 32 keys are 36 words after the last quarter's and
//     the arrays 152 words apart, so the twelve 16-byte slots that a wave's lanes can ask for in one read lie on distinct banks.  Costs
//     are 32 bits relative to the minimum of the step before (each wave leaves its minimum beside the keys) under a 64-bit base: within
//     the parameter ranges a step's costs lie within 2^20 of each other, a key stays below 2^30.  The two LDS images alternate: one
//     barrier per step.  Back-pointers go out as one byte per (t, s).
// (e) hand_trace_kernel, one workgroup: 256 rows of back-pointers at a time into LDS, one lane follows them, all write s_t.
// (f) hand_finish_kernel, one lane per record and per slice: hand[i], the left and right counts; split[t] and the hand-overs on the path.
// No kernel waits on another workgroup and nothing spins.
#include "common.h"
#include "kernels.h"
#include "note_rule.h"

namespace {

constexpr int HAND_THREADS = 256;
constexpr int HAND_CLEAR_BLOCKS = 256;
constexpr int HAND_SCAN_THREADS = 1024;                                     // slots per round of the compaction scan
constexpr int HAND_PARTS = 4;                                               // lanes per state in the path kernel
constexpr int HAND_PATH_THREADS = 576;                                      // nine waves: 129 states x 4 lanes = 516 of them at work
constexpr int HAND_PART_WORDS = 36;                                         // a quarter's 32 keys and four words of padding
constexpr int HAND_LAST_AT = 4 * HAND_PART_WORDS;                           // where the key of s' = 128 lies
constexpr int HAND_ROW = 152;                                               // words per key array: 152 mod 64 = 24
constexpr unsigned HAND_PAD = 0x3fffffffu;                                  // above every key, and no sum with a distance term overflows
constexpr int HAND_TRACE_ROWS = 256;

struct HandSet { unsigned long long lo, hi; };                              // pitches 0 .. 63, 64 .. 127

__device__ __forceinline__ HandSet hand_set(const uint4 v) { return HandSet{v.x | (unsigned long long)v.y << 32, v.z | (unsigned long long)v.w << 32}; }
__device__ __forceinline__ bool hand_some(const HandSet p) { return (p.lo | p.hi) != 0ull; }
// of a set that is not empty
__device__ __forceinline__ int hand_min(const HandSet p) { return p.lo ? __ffsll((long long)p.lo) - 1 : 63 + __ffsll((long long)p.hi); }
__device__ __forceinline__ int hand_max(const HandSet p) { return p.hi ? 127 - __clzll((long long)p.hi) : 63 - __clzll((long long)p.lo); }
// the pitches below s, s in [0, 128]
__device__ __forceinline__ HandSet hand_below(const HandSet p, int s) {
    if (s >= 128) return p;
    if (s >= 64) return HandSet{p.lo, p.hi & ((1ull << (s - 64)) - 1ull)};
    return HandSet{p.lo & ((1ull << s) - 1ull), 0ull};
}
__device__ __forceinline__ int hand_class(const HandSet p, int s) { return s <= hand_min(p) ? 0 : s > hand_max(p) ? 2 : 1; }

// e_t(s) and class_t(s) of a slice's set
__device__ __forceinline__ int hand_emission(const HandArgs& a, const HandSet p, int s, int* cls) {
    const HandSet left = hand_below(p, s), right = HandSet{p.lo & ~left.lo, p.hi & ~left.hi};
    const bool some_l = hand_some(left), some_r = hand_some(right);
    int e = 0, max_l = 0, min_r = 0;
    if (some_l) {
        max_l = hand_max(left);
        e += a.w_span * max(0, max_l - hand_min(left) - a.span);
    }
    if (some_r) {
        min_r = hand_min(right);
        e += a.w_span * max(0, hand_max(right) - min_r - a.span);
    }
    if (some_l && some_r) e += a.w_cut * max(0, a.cut_min - (min_r - max_l)) + a.w_centre * (abs(2 * s - (max_l + min_r + 1)) >> 1);
    *cls = !some_l ? 0 : !some_r ? 2 : 1;
    return e + a.w_mid * max(0, abs(s - a.middle) - a.mid_free);
}

// the slot of a record that is selected; -1: it is not (counted: whether the note rule counts it)
__device__ __forceinline__ long long hand_slot(const HandArgs& a, const DetokNote r, bool* counted) {
    const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
    *counted = c.counted;
    if (!c.counted || c.drum || c.prog < a.program_lo || c.prog > a.program_hi) return -1;
    long long lo, hi;
    if (!note_frame_span(r, false, a.frames_per_second, a.n_frames, &lo, &hi)) return -1;
    return lo / a.slice_frames;                                            // lo < n_frames: below n_slots
}

__global__ __launch_bounds__(HAND_THREADS) void hand_clear_kernel(HandArgs a) {
    const long long stride = (long long)gridDim.x * HAND_THREADS, t0 = (long long)blockIdx.x * HAND_THREADS + threadIdx.x;
    for (long long i = t0; i < a.n_slots; i += stride) a.sets[i] = make_uint4(0u, 0u, 0u, 0u);
    if (t0 < 8) a.result[t0] = 0;
    if (t0 < HAND_ACC_WORDS) a.acc[t0] = 0ull;
}

__global__ __launch_bounds__(HAND_THREADS) void hand_mark_kernel(HandArgs a) {
    const long long i = (long long)blockIdx.x * HAND_THREADS + threadIdx.x;
    if (i >= note_live_count(a.n, a.count)) return;
    const DetokNote r = a.notes[i];
    bool counted;
    const long long slot = hand_slot(a, r, &counted);
    if (!counted) atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[5]), 1ull);
    if (slot < 0) return;
    atomicOr(reinterpret_cast<unsigned*>(a.sets + slot) + (r.pitch >> 5), 1u << (r.pitch & 31));
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[1]), 1ull);
}

__global__ __launch_bounds__(HAND_SCAN_THREADS) void hand_compact_kernel(HandArgs a) {
    constexpr int WAVES = HAND_SCAN_THREADS / WAVE;
    __shared__ int counts[WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    long long T = 0;
    for (long long first = 0; first < a.n_slots; first += HAND_SCAN_THREADS) {
        const long long slot = first + tid;
        const uint4 v = slot < a.n_slots ? a.sets[slot] : make_uint4(0u, 0u, 0u, 0u);
        const bool occupied = (v.x | v.y | v.z | v.w) != 0u;
        const unsigned long long ballot = __ballot(occupied);
        if (lane == 0) counts[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < WAVES; ++w) {
            before += w < wave ? counts[w] : 0;
            total += counts[w];
        }
        const long long t = T + before + __popcll(ballot & ((1ull << lane) - 1ull));
        if (occupied && t < a.max_slices) {                                 // (a slice has a record of its own and a slot of its own: T <= max_slices)
            a.cset[t] = v;
            a.slot_of[t] = (int32_t)slot;
            a.slice_of[slot] = (int32_t)t;
        }
        T += total;
        __syncthreads();
    }
    if (tid == 0) {
        T = min(T, a.max_slices);
        a.acc[0] = (unsigned long long)T;
        a.result[0] = T;
    }
}

// the smallest key + step |s - s'| over this lane's quarter of the s' and s' = 128
__device__ __forceinline__ unsigned hand_best(const unsigned* from, int part, int s, unsigned step) {
    const uint4* q = reinterpret_cast<const uint4*>(from + HAND_PART_WORDS * part);
    unsigned best = from[HAND_LAST_AT] + step * (unsigned)(128 - s);
    int d = s - 32 * part;                                                  // s - s'
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint4 k = q[j];
        best = min(best, k.x + step * (unsigned)abs(d));
        best = min(best, k.y + step * (unsigned)abs(d - 1));
        best = min(best, k.z + step * (unsigned)abs(d - 2));
        best = min(best, k.w + step * (unsigned)abs(d - 3));
        d -= 4;
    }
    best = min(best, (unsigned)__shfl_xor((int)best, 1, WAVE));             // the four lanes of a state
    return min(best, (unsigned)__shfl_xor((int)best, 2, WAVE));
}

__global__ __launch_bounds__(HAND_PATH_THREADS) void hand_path_kernel(HandArgs a) {
    constexpr int WAVES = HAND_PATH_THREADS / WAVE;
    // [image][0 plain, 1 + w_switch where the writer's class is 2, 2 + w_switch where it is 0][the keys]
    __shared__ __attribute__((aligned(16))) unsigned keys[2][3][HAND_ROW];
    __shared__ unsigned wave_min[2][16];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int T = (int)a.acc[0];
    if (T <= 0) return;
    const bool live = tid < HAND_STATES * HAND_PARTS;
    const int s = live ? tid >> 2 : HAND_STATES - 1, part = tid & (HAND_PARTS - 1);
    const int at = s + 4 * (s >> 5);                                        // where the key of state s lies in its array
    for (int x = tid; x < 2 * 3 * HAND_ROW; x += HAND_PATH_THREADS) (&keys[0][0][0])[x] = HAND_PAD;
    if (tid < 32) (&wave_min[0][0])[tid] = 0xffffffffu;
    __syncthreads();
    const unsigned w8 = (unsigned)a.w_move << 8, pen8 = (unsigned)a.w_switch << 8;
    unsigned long long base = 0ull;
    uint4 set = a.cset[0], next_set = set;
    int slot = a.slot_of[0], next_slot = slot, prev_slot = slot;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        if (t + 1 < T) {                                                    // the next slice, asked for before this step's work
            next_set = a.cset[t + 1];
            next_slot = a.slot_of[t + 1];
        }
        int cls;
        unsigned c = (unsigned)hand_emission(a, hand_set(set), s, &cls);
        if (t > 0) {
            const bool rest = slot - prev_slot >= a.rest_slots;
            const unsigned best = hand_best(keys[cur ^ 1][rest || cls == 1 ? 0 : cls == 0 ? 1 : 2], part, s, rest ? 0u : w8);
            unsigned m = wave_min[cur ^ 1][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) m = min(m, wave_min[cur ^ 1][w]);
            base += m;
            c += (best >> 8) - m;
            if (live && part == 3) a.back[(long long)t * HAND_BACK_ROW + s] = (unsigned char)(best & 255u);
        }
        const unsigned key = c << 8 | (unsigned)s;
        if (live && part < 3) keys[cur][part][at] = key + ((part == 1 && cls == 2) || (part == 2 && cls == 0) ? pen8 : 0u);
        unsigned low = live ? c : 0xffffffffu;
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) low = min(low, (unsigned)__shfl_xor((int)low, x, WAVE));
        if (lane == 0) wave_min[cur][wave] = low;
        __syncthreads();
        prev_slot = slot;
        set = next_set;
        slot = next_slot;
    }
    const unsigned best = hand_best(keys[(T - 1) & 1][0], part, s, 0u);      // the smallest minimiser of C_{T-1}; every state finds the same
    if (tid == 0) {
        a.acc[1] = best & 255u;
        a.cut[T - 1] = (unsigned char)(best & 255u);
        a.result[4] = (long long)(base + (best >> 8));
    }
}

__global__ __launch_bounds__(HAND_THREADS) void hand_trace_kernel(HandArgs a) {
    __shared__ unsigned rows[HAND_TRACE_ROWS * (HAND_BACK_ROW / 4)];
    __shared__ unsigned char found[HAND_TRACE_ROWS];
    const int tid = threadIdx.x;
    const int T = (int)a.acc[0];
    if (T <= 0) return;
    int cur = (int)a.acc[1];                                                // s_{T-1}; lane 0 follows the path
    for (int hi = T - 1; hi >= 1; hi -= HAND_TRACE_ROWS) {                  // the rows [lo, hi] give s_{lo-1} .. s_{hi-1}
        const int lo = max(1, hi - HAND_TRACE_ROWS + 1), n = hi - lo + 1;
        const unsigned* src = reinterpret_cast<const unsigned*>(a.back + (long long)lo * HAND_BACK_ROW);
        for (int x = tid; x < n * (HAND_BACK_ROW / 4); x += HAND_THREADS) rows[x] = src[x];
        __syncthreads();
        if (tid == 0) {
            const unsigned char* row = reinterpret_cast<const unsigned char*>(rows);
            for (int t = hi; t >= lo; --t) {
                cur = row[(t - lo) * HAND_BACK_ROW + cur];
                found[t - lo] = (unsigned char)cur;
            }
        }
        __syncthreads();
        for (int x = tid; x < n; x += HAND_THREADS) a.cut[lo - 1 + x] = found[x];
    }
}

__global__ __launch_bounds__(HAND_THREADS) void hand_finish_kernel(HandArgs a) {
    const long long i = (long long)blockIdx.x * HAND_THREADS + threadIdx.x;
    const long long T = (long long)a.acc[0];
    if (i < T) {
        const int s = a.cut[i], slot = a.slot_of[i];
        if (a.split) a.split[i] = 256 * slot + s;
        if (i >= 1 && slot - a.slot_of[i - 1] < a.rest_slots) {
            const int before = hand_class(hand_set(a.cset[i - 1]), a.cut[i - 1]), now = hand_class(hand_set(a.cset[i]), s);
            if (before + now == 2 && before != 1) atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[6]), 1ull);
        }
    }
    if (i >= note_live_count(a.n, a.count)) return;
    const DetokNote r = a.notes[i];
    bool counted;
    const long long slot = hand_slot(a, r, &counted);
    if (slot < 0) {
        a.hand[i] = 255;
        return;
    }
    const int right = r.pitch >= (int)a.cut[a.slice_of[slot]] ? 1 : 0;
    a.hand[i] = (uint8_t)right;
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[2 + right]), 1ull);
}

}  // namespace

int launch_split_hands(const HandArgs& a, hipStream_t stream) {
    if (a.n_programs < 1 || a.n_programs > BAR_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -1;
    if (a.slice_frames < 1 || a.slice_frames > HAND_MAX_SLICE_FRAMES || a.program_lo < 0 || a.program_lo > a.program_hi || a.program_hi >= a.n_programs) return -2;
    const int weights[] = {a.w_span, a.w_cut, a.w_centre, a.w_mid, a.w_move, a.w_switch};
    for (const int w : weights)
        if (w < 0 || w > HAND_MAX_WEIGHT) return -3;                       // the 32-bit keys of the path kernel rest on these bounds
    if (a.span < 1 || a.span > 127 || a.cut_min < 0 || a.cut_min > 127 || a.middle < 0 || a.middle > 128 || a.mid_free < 0 || a.mid_free > 128 ||
        a.rest_slots < 1 || a.rest_slots > HAND_MAX_REST || !(a.frames_per_second > 0.0))
        return -3;
    if (a.n_frames < 1 || a.n_frames > BAR_MAX_FRAMES || a.n < 0 || a.n > BAR_MAX_NOTES || (a.n && (!a.notes || !a.hand))) return -4;
    if (a.n_slots != hand_slots(a.n_frames, a.slice_frames) || a.max_slices < 1 || a.max_slices < (a.n < a.n_slots ? a.n : a.n_slots)) return -5;
    if (!a.sets || !a.slice_of || !a.cset || !a.slot_of || !a.back || !a.cut || !a.acc || !a.result) return -6;
    const unsigned slot_blocks = (unsigned)((a.n_slots + HAND_THREADS - 1) / HAND_THREADS);
    hand_clear_kernel<<<slot_blocks < (unsigned)HAND_CLEAR_BLOCKS ? slot_blocks : (unsigned)HAND_CLEAR_BLOCKS, HAND_THREADS, 0, stream>>>(a);
    if (!a.n) return 0;                                                    // no record: no slice
    const unsigned note_blocks = (unsigned)((a.n + HAND_THREADS - 1) / HAND_THREADS);
    hand_mark_kernel<<<note_blocks, HAND_THREADS, 0, stream>>>(a);
    hand_compact_kernel<<<1, HAND_SCAN_THREADS, 0, stream>>>(a);
    hand_path_kernel<<<1, HAND_PATH_THREADS, 0, stream>>>(a);
    hand_trace_kernel<<<1, HAND_THREADS, 0, stream>>>(a);
    hand_finish_kernel<<<note_blocks, HAND_THREADS, 0, stream>>>(a);
    return 0;
}
