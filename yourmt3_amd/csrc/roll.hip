// Device piano roll and frame metrics: note records -> a 0/1 roll per (row, frame, pitch), and the integers of frame-level F1 of an
// estimate against a reference (include/ymt3.h, piano roll and frame metrics).  The specification is the host path, piano_roll and
// frame_metrics of yourmt3_amd/metrics.py; tests/roll_model.py states the rules in plain Python.  Integer work plus, per record, two f64
// multiplies, two rint and one add with contraction off, and the clipping in f64 before any conversion: nothing here rounds differently
// from the host, and every output is an integer or a 0/1 byte.
//
// Working layout: frame-major bit sets.  bits[side][row][frame] is one 16-byte word of 128 pitch bits (dword pitch / 32, bit pitch % 32),
// so a frame's polyphony is popc of four dwords, tp is popc(ref & est), and one 16-byte load per side gives a (row, frame).  The rows of
// a call are packed at the call's n_frames, so the frames in use are one contiguous range of words.  The object's scratch holds
// 2 x (n_programs + 1) x max_frames words: about 126 MB per side for 131 rows x 10 minutes at 100 frames per second.
// (a) roll_clear_kernel: zeroes the words in use (n_frames of every row and side of the call) and, for the metrics, counts_dev.
// (b) roll_raster_kernel, one wave per record and side: every lane classifies the record and computes the clipped frame
//     interval (note_rule.h); the lanes stride over its frames and set the pitch bit with atomicOr on the dword, in the record's
//     aware row and, if it is pitched, in the agnostic row.  A skipped record adds one to skipped[side].
// (c) roll_reduce_kernel (metrics), one lane per (row, frame) and REDUCE_FRAMES frames per lane: nr, ne, tp and the three error terms;
//     the wave sums the six values with shuffles and lane 0 adds those that are not zero to the row's six 64-bit integers.  Integer
//     sums commute: the result does not depend on the order.
// (d) roll_expand_kernel (roll): eight lanes per (row, frame), each turns 16 pitch bits into 16 bytes and stores them as one 16-byte
//     word: a wave writes 1 KB of consecutive bytes.
// No kernel waits on another workgroup and nothing spins.
#include "common.h"
#include "kernels.h"
#include "note_rule.h"

namespace {

constexpr int ROLL_THREADS = 256;
constexpr int CLEAR_BLOCKS = 2048;        // grid-stride: 8 workgroups per CU
constexpr int REDUCE_FRAMES = 4;          // frames per lane of the reduction: a workgroup covers 1024 frames of one row

__global__ __launch_bounds__(ROLL_THREADS) void roll_clear_kernel(RollArgs a) {
    const long long words = (long long)a.n_sides * a.row_n * a.n_frames;
    const long long stride = (long long)gridDim.x * ROLL_THREADS;
    for (long long i = (long long)blockIdx.x * ROLL_THREADS + threadIdx.x; i < words; i += stride) a.bits[i] = make_uint4(0u, 0u, 0u, 0u);
    if (a.counts && blockIdx.x == 0)
        for (int i = threadIdx.x; i < (a.n_programs + 1) * 6 + 2; i += ROLL_THREADS) a.counts[i] = 0;
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_raster_kernel(RollArgs a) {
    const int side = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * (ROLL_THREADS / WAVE) + (threadIdx.x >> 6);
    if (i >= note_live_count(a.n[side], a.count[side])) return;
    const DetokNote r = a.notes[side][i];
    const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
    if (!c.counted) {
        if (a.counts && lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts[(a.n_programs + 1) * 6 + side]), 1ull);
        return;
    }
    long long f_lo, f_hi;
    if (!note_frame_span(r, c.drum, a.frames_per_second, a.n_frames, &f_lo, &f_hi)) return;
    const int dword = r.pitch >> 5;
    const unsigned bit = 1u << (r.pitch & 31);
    unsigned* words = reinterpret_cast<unsigned*>(a.bits);
    const int rows[2] = {c.prog, c.drum ? -1 : a.n_programs};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int row = rows[k] - a.row0;
        if (rows[k] < 0 || row < 0 || row >= a.row_n) continue;         // (a roll call may keep a range of the rows only)
        unsigned* w = words + (((long long)side * a.row_n + row) * a.n_frames) * 4 + dword;
        for (long long f = f_lo + lane; f < f_hi; f += WAVE) atomicOr(&w[f * 4], bit);
    }
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_reduce_kernel(RollArgs a) {
    const int row = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const uint4* R = a.bits + (long long)row * a.n_frames;
    const uint4* E = a.bits + ((long long)a.row_n + row) * a.n_frames;
    int v[6] = {0, 0, 0, 0, 0, 0};                                      // a lane's sums: at most REDUCE_FRAMES * 128 each
    const long long f0 = (long long)blockIdx.x * (ROLL_THREADS * REDUCE_FRAMES) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < REDUCE_FRAMES; ++k) {
        const long long f = f0 + (long long)k * ROLL_THREADS;
        if (f >= a.n_frames) break;
        const uint4 r = R[f], e = E[f];
        const int nr = __popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w);
        const int ne = __popc(e.x) + __popc(e.y) + __popc(e.z) + __popc(e.w);
        const int tp = __popc(r.x & e.x) + __popc(r.y & e.y) + __popc(r.z & e.z) + __popc(r.w & e.w);
        v[0] += tp;
        v[1] += nr;
        v[2] += ne;
        v[3] += min(nr, ne) - tp;
        v[4] += max(0, nr - ne);
        v[5] += max(0, ne - nr);
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) v[c] += __shfl_xor(v[c], x, WAVE);
        if (lane == 0 && v[c]) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts[row * 6 + c]), (unsigned long long)v[c]);
    }
}

// 4 bits -> 4 bytes of 0 / 1, the lowest bit in the lowest byte
__device__ __forceinline__ unsigned spread4(unsigned n) { return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21); }

__global__ __launch_bounds__(ROLL_THREADS) void roll_expand_kernel(RollArgs a) {
    const long long t = (long long)blockIdx.x * ROLL_THREADS + threadIdx.x;         // 16 pitches of one (row, frame)
    const long long cell = t >> 3;
    if (cell >= (long long)a.row_n * a.n_frames) return;
    const int part = (int)(t & 7);
    const unsigned word = reinterpret_cast<const unsigned*>(a.bits)[cell * 4 + (part >> 1)];
    const unsigned h = (word >> ((part & 1) * 16)) & 0xffffu;
    reinterpret_cast<uint4*>(a.roll)[t] = make_uint4(spread4(h), spread4(h >> 4), spread4(h >> 8), spread4(h >> 12));
}

int check(const RollArgs& a) {
    if (a.n_programs < 1 || a.n_programs > ROLL_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -1;
    if (a.max_frames < 1 || a.max_frames > ROLL_MAX_FRAMES || a.n_frames < 0 || a.n_frames > a.max_frames) return -2;
    if (a.n_sides < 1 || a.n_sides > 2 || a.row0 < 0 || a.row_n < 1 || a.row0 + a.row_n > a.n_programs + 1) return -3;
    for (int s = 0; s < a.n_sides; ++s)
        if (a.n[s] < 0 || a.n[s] > ROLL_MAX_NOTES || (a.n[s] && !a.notes[s])) return -4;
    if (!a.bits || !(a.frames_per_second > 0.0)) return -5;
    return 0;
}

void clear_and_rasterise(const RollArgs& a, hipStream_t stream) {
    const long long words = (long long)a.n_sides * a.row_n * a.n_frames;
    const long long blocks = (words + ROLL_THREADS - 1) / ROLL_THREADS;
    roll_clear_kernel<<<(unsigned)std::max(1LL, std::min<long long>(blocks, CLEAR_BLOCKS)), ROLL_THREADS, 0, stream>>>(a);
    long long n = 0;
    for (int s = 0; s < a.n_sides; ++s) n = std::max(n, a.n[s]);
    if (n == 0) return;
    const int per = ROLL_THREADS / WAVE;
    roll_raster_kernel<<<dim3((unsigned)((n + per - 1) / per), a.n_sides), ROLL_THREADS, 0, stream>>>(a);
}

}  // namespace

int launch_frame_metrics(const RollArgs& a, hipStream_t stream) {
    if (const int rc = check(a)) return rc;
    if (!a.counts || a.n_sides != 2 || a.row0 != 0 || a.row_n != a.n_programs + 1) return -6;
    clear_and_rasterise(a, stream);
    if (a.n_frames == 0) return 0;
    const long long per_block = (long long)ROLL_THREADS * REDUCE_FRAMES;
    roll_reduce_kernel<<<dim3((unsigned)((a.n_frames + per_block - 1) / per_block), a.row_n), ROLL_THREADS, 0, stream>>>(a);
    return 0;
}

int launch_piano_roll(const RollArgs& a, hipStream_t stream) {
    if (const int rc = check(a)) return rc;
    if (a.counts || a.n_sides != 1 || !a.roll) return -6;
    if (a.n_frames == 0) return 0;
    clear_and_rasterise(a, stream);
    const long long threads = (long long)a.row_n * a.n_frames * 8;
    roll_expand_kernel<<<(unsigned)((threads + ROLL_THREADS - 1) / ROLL_THREADS), ROLL_THREADS, 0, stream>>>(a);
    return 0;
}
