// Chords over note records and tracked beats: per-beat pitch-class content and bass, template emissions, and a smoothing path over
// (quality, root) and N (include/ymt3.h, chords).  The specification is the host path, track_chords of yourmt3_amd/chords.py;
// tests/chord_model.py states the rules as plain loops.  Everything is an integer (times stay f64 until they are known to lie inside the
// frames): every output equals the host's.
// The number of beats K is read from the beat tracker's result on the device, so every launch is sized by the object's max_beats or by
// the number of records, and nothing is read back.
// (a) chord_clear_kernel zeroes c[0, K)[12] and result[8] and sets bass[0, K) to 255.
// (b) chord_features_kernel, one lane per record: classifies it by the rule every note consumer uses (note_rule.h), finds the first slot
//     its span overlaps by a binary search over the slots' lower edges (beat_slots.h, computed on the fly from the beats), walks the
//     slots it overlaps, adds the shared frames to c[slot][pitch class] and, where the share is long enough, takes bass[slot] down to its
//     pitch.  Integer atomicAdd and atomicMin: exact in any order.
// (c) chord_path_kernel, one workgroup of four waves.  Wave 0 is the serial spine: the states two per lane (s = lane, lane + 64), V in
//     registers.  A beat takes one wave arg-max over keys (V << 7 | 127 - s: the larger V, then the smaller state), a compare and an add;
//     the stay bits come from two ballots, and lane j of a chunk keeps beat j's back-pointer words: one coalesced 16-byte store per lane
//     and chunk.  Waves 1 to 3 meanwhile produce the emissions of the NEXT 64 beats into the other of two LDS buffers (one lane per beat:
//     the 64-bit normalisation and a third of the templates each, rows 99 words apart, so neither side has bank conflicts): the serial
//     chain carries no division and no template gather.  One __syncthreads per chunk orders the two buffers.  Then wave 0 follows the
//     back-pointers back, a chunk's words loaded coalesced and read with __shfl, and writes chord[] coalesced.
// No kernel waits on another workgroup and nothing spins.
#include "common.h"
#include "kernels.h"
#include "beat_slots.h"
#include "note_rule.h"

namespace {

constexpr int CHORD_THREADS = 256;
constexpr int CHORD_CLEAR_BLOCKS = 256;
constexpr int CHORD_ROW = 99;                                              // LDS words per beat: S <= 97 emissions, [97] the downbeat flag; odd
constexpr int CHORD_FLAG = 97;
constexpr unsigned CHORD_NO_BASS = 255u, CHORD_NONE = 255u;

__global__ __launch_bounds__(CHORD_THREADS) void chord_clear_kernel(ChordArgs a) {
    const long long stride = (long long)gridDim.x * CHORD_THREADS, t0 = (long long)blockIdx.x * CHORD_THREADS + threadIdx.x;
    const long long K = beat_count(a.beat_result, a.max_beats);
    for (long long i = t0; i < K * 12; i += stride) a.chroma[i] = 0u;
    for (long long i = t0; i < K; i += stride) a.bass[i] = CHORD_NO_BASS;
    if (t0 < 8) a.result[t0] = 0;
}

__global__ __launch_bounds__(CHORD_THREADS) void chord_features_kernel(ChordArgs a) {
    const long long i = (long long)blockIdx.x * CHORD_THREADS + threadIdx.x;
    if (i >= note_live_count(a.n, a.count)) return;
    const DetokNote r = a.notes[i];
    const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
    if (!c.counted) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.result[3]), 1ull);
        return;
    }
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2 || c.drum) return;
    long long lo, hi;
    if (!note_frame_span(r, false, a.frames_per_second, a.n_frames, &lo, &hi)) return;
    const BeatSlots sl = {a.beats, K, a.near_div};
    if (hi <= slot_edge(sl, 0) || lo >= slot_edge(sl, K)) return;
    const int pc = r.pitch % 12;
    slot_walk(sl, lo, hi, [&](int s, long long share, long long length) {
        atomicAdd(&a.chroma[(long long)s * 12 + pc], (unsigned)share);
        if ((long long)a.bass_div * share >= length) atomicMin(&a.bass[s], (unsigned)r.pitch);
    });
}

// where the states of the fixed table's quality q start in this object's state order; -1 if it is not among them
__device__ __forceinline__ int chord_base(const ChordArgs& a, int q) {
    int base = -1;
#pragma unroll
    for (int k = 0; k < CHORD_QUALITIES; ++k)
        if (k < a.n_qualities && a.qualities[k] == q) base = 12 * k;
    return base;
}

// the twelve roots of one quality: intervals {0, A, B} or {0, A, B, C} (C < 0: a triad), weight W
template <int A, int B, int C, int W>
__device__ __forceinline__ void chord_emit(const unsigned (&n)[12], int* out, int bass_pc, int bonus) {
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        unsigned s = n[r] + n[(r + A) % 12] + n[(r + B) % 12];
        if (C >= 0) s += n[(r + (C >= 0 ? C : 0)) % 12];
        out[r] = W * (int)s + (r == bass_pc ? bonus : 0);
    }
}

// the emissions of the 64 beats of `chunk` into buf, lane = the beat; part in [0, 3): which third of the templates this wave writes
__device__ __forceinline__ void chord_emissions(const ChordArgs& a, int K, int chunk, int* buf, int lane, int part) {
    const long long i = (long long)chunk * WAVE + lane;
    if (i >= K) return;
    const uint4* cp = reinterpret_cast<const uint4*>(a.chroma + i * 12);
    const uint4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
    const unsigned c[12] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w};
    unsigned long long sum = 0ull;
#pragma unroll
    for (int pc = 0; pc < 12; ++pc) sum += c[pc];
    if (!sum) sum = 1ull;
    unsigned n[12];
#pragma unroll
    for (int pc = 0; pc < 12; ++pc) n[pc] = (unsigned)((unsigned long long)c[pc] * 1024ull / sum);
    const unsigned bass = a.bass[i];
    const int bass_pc = bass < 128u ? (int)(bass % 12u) : -1;
    const int bonus = 1024 * a.w_bass;
    int* row = buf + lane * CHORD_ROW;
    int base;
    if (part == 0) {
        if ((base = chord_base(a, 0)) >= 0) chord_emit<4, 7, -1, 591>(n, row + base, bass_pc, bonus);       // maj
        if ((base = chord_base(a, 3)) >= 0) chord_emit<4, 8, -1, 591>(n, row + base, bass_pc, bonus);       // aug
        if ((base = chord_base(a, 6)) >= 0) chord_emit<4, 7, 11, 512>(n, row + base, bass_pc, bonus);       // maj7
    } else if (part == 1) {
        if ((base = chord_base(a, 1)) >= 0) chord_emit<3, 7, -1, 591>(n, row + base, bass_pc, bonus);       // min
        if ((base = chord_base(a, 4)) >= 0) chord_emit<5, 7, -1, 591>(n, row + base, bass_pc, bonus);       // sus4
        if ((base = chord_base(a, 7)) >= 0) chord_emit<3, 7, 10, 512>(n, row + base, bass_pc, bonus);       // min7
    } else {
        if ((base = chord_base(a, 2)) >= 0) chord_emit<3, 6, -1, 591>(n, row + base, bass_pc, bonus);       // dim
        if ((base = chord_base(a, 5)) >= 0) chord_emit<4, 7, 10, 512>(n, row + base, bass_pc, bonus);       // 7
        row[12 * a.n_qualities] = 1024 * a.w_none;                                                          // N
        row[CHORD_FLAG] = a.metre && (a.metre[i] & 255) == 0 ? 1 : 0;
    }
}

// the wave's maximum of the keys; every lane gets it
__device__ __forceinline__ unsigned long long chord_wave_max(unsigned long long key) {
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const unsigned long long o = __shfl_xor(key, x, WAVE);
        key = o > key ? o : key;
    }
    return key;
}

__device__ __forceinline__ unsigned long long chord_key(bool active, long long v, int state) {
    return active ? ((unsigned long long)v << 7) | (unsigned)(127 - state) : 0ull;     // V >= 0; an inactive slot loses to every state
}

__global__ __launch_bounds__(CHORD_THREADS) void chord_path_kernel(ChordArgs a) {
    __shared__ int em[2][WAVE * CHORD_ROW];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2) return;                                                     // result[0 .. 2] stay 0
    const int S = 12 * a.n_qualities + 1;
    const int n_chunks = (K + WAVE - 1) / WAVE;
    const long long p_change = 1024LL * a.change_cost, p_down = 1024LL * a.change_cost_down;
    const bool act0 = lane < S, act1 = lane + WAVE < S;
    long long V0 = 0, V1 = 0;
    if (wave > 0) chord_emissions(a, K, 0, em[0], lane, wave - 1);
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
        if (wave == 0) {
            const int* buf = em[c & 1];
            const int i0 = c * WAVE, nj = min(WAVE, K - i0);
            uint4 mine = make_uint4(~0u, ~0u, ~0u, 1u);                    // beat 0 has no predecessor: every state stays
            for (int j = 0; j < nj; ++j) {
                const int* row = buf + j * CHORD_ROW;
                const long long e0 = act0 ? row[lane] : 0, e1 = act1 ? row[WAVE + lane] : 0;
                if (i0 + j == 0) {
                    V0 = e0;
                    V1 = e1;
                    continue;
                }
                const long long P = row[CHORD_FLAG] ? p_down : p_change;
                const unsigned long long k0 = chord_key(act0, V0, lane), k1 = chord_key(act1, V1, lane + WAVE);
                const unsigned long long key = chord_wave_max(k0 > k1 ? k0 : k1);
                const unsigned best = 127u - (unsigned)(key & 127ull);     // j*: the first state with V maximal
                const long long jump = (long long)(key >> 7) - P;
                const bool s0 = V0 >= jump, s1 = V1 >= jump;
                const unsigned long long m0 = __ballot(s0), m1 = __ballot(s1 && act1);
                V0 = (s0 ? V0 : jump) + e0;
                V1 = (s1 ? V1 : jump) + e1;
                if (lane == j) mine = make_uint4((unsigned)m0, (unsigned)(m0 >> 32), (unsigned)m1, ((unsigned)(m1 >> 32) & 1u) | best << 1);
            }
            if (i0 + lane < K) reinterpret_cast<uint4*>(a.back)[i0 + lane] = mine;
        } else if (c + 1 < n_chunks) {
            chord_emissions(a, K, c + 1, em[(c + 1) & 1], lane, wave - 1);
        }
        __syncthreads();
    }
    if (wave != 0) return;
    // the end: the first state with V[K-1] maximal; then back, every lane with the same (uniform) state
    const unsigned long long k0 = chord_key(act0, V0, lane), k1 = chord_key(act1, V1, lane + WAVE);
    const unsigned long long key = chord_wave_max(k0 > k1 ? k0 : k1);
    int s = 127 - (int)(key & 127ull);
    long long runs = 1, none = 0;
    for (int c = n_chunks - 1; c >= 0; --c) {
        const int i0 = c * WAVE, nj = min(WAVE, K - i0);
        const uint4 m = lane < nj ? reinterpret_cast<const uint4*>(a.back)[i0 + lane] : make_uint4(0u, 0u, 0u, 0u);
        int my = 0;
        for (int j = nj - 1; j >= 0; --j) {
            if (lane == j) my = s;
            none += s == S - 1;
            if (i0 + j == 0) break;
            const unsigned w = s < 32 ? m.x : (s < 64 ? m.y : (s < 96 ? m.z : m.w));
            const int v = __shfl((int)(((w >> (s & 31)) & 1u) | (m.w >> 1) << 1), j, WAVE);      // beat i0 + j's: stay bit of s, then j*
            const int from = (v & 1) ? s : v >> 1;
            runs += from != s;                                             // distinct states carry distinct labels
            s = from;
        }
        if (lane < nj) {
            unsigned label = CHORD_NONE;
            if (my < S - 1) {
                int q = 0;
#pragma unroll
                for (int k = 0; k < CHORD_QUALITIES; ++k) q = k == my / 12 ? a.qualities[k] : q;
                label = (unsigned)(12 * q + my % 12);
            }
            a.chord[i0 + lane] = (int32_t)(256u * a.bass[i0 + lane] + label);
        }
    }
    if (lane == 0) {
        a.result[0] = runs;
        a.result[1] = (long long)(key >> 7);
        a.result[2] = none;
    }
}

}  // namespace

int launch_track_chords(const ChordArgs& a, hipStream_t stream) {
    if (int e = slot_check_programs(a)) return e;
    if (a.n_qualities < 1 || a.n_qualities > CHORD_QUALITIES) return -2;
    for (int k = 0; k < a.n_qualities; ++k)
        if (a.qualities[k] < 0 || a.qualities[k] >= CHORD_QUALITIES) return -2;
    if (a.bass_div < 1 || a.w_bass < 0 || a.w_bass > 1024 || a.w_none < 0 || a.w_none > 1024 || a.change_cost < 0 || a.change_cost_down < 0) return -3;
    if (int e = slot_check_call(a)) return e;
    if (!a.bass || !a.back || !a.chord) return -6;
    const unsigned beat_blocks = (unsigned)((a.max_beats + CHORD_THREADS - 1) / CHORD_THREADS);
    chord_clear_kernel<<<beat_blocks < (unsigned)CHORD_CLEAR_BLOCKS ? beat_blocks : (unsigned)CHORD_CLEAR_BLOCKS, CHORD_THREADS, 0, stream>>>(a);
    if (a.n) chord_features_kernel<<<(unsigned)((a.n + CHORD_THREADS - 1) / CHORD_THREADS), CHORD_THREADS, 0, stream>>>(a);
    chord_path_kernel<<<1, CHORD_THREADS, 0, stream>>>(a);
    return 0;
}
