// The one rule for the beats' slots, shared by bars.hip and chords.hip: how many beats there are, where slot i begins and ends, which
// slot a frame lies in, and how a span of frames is shared out among the slots it overlaps.  The host specification is slot_edges and
// share_spans of yourmt3_amd/bars.py: every piece here computes what they compute, to the last bit.  The helpers take the small struct
// by value (profiles/note_side_refactor_ab.txt: with reference parameters the same compiler produced visibly worse code).
#pragma once
#include "kernels.h"

// K: the beat tracker's count, read on the device and clamped to what the object's scratch holds
__device__ __forceinline__ int beat_count(const long long* beat_result, long long max_beats) {
    const long long k = beat_result[0];
    return (int)(k < 0 ? 0 : (k < max_beats ? k : max_beats));
}

// b[0 .. K) frames, strictly ascending, K >= 2; nd = near_div
struct BeatSlots { const int32_t* b; int K, nd; };

// D[i], i in [0, K)
__device__ __forceinline__ int slot_delta(const BeatSlots s, int i) { return i < s.K - 1 ? s.b[i + 1] - s.b[i] : s.b[s.K - 1] - s.b[s.K - 2]; }

// the slots' edges, i in [0, K]: lo[i] for i < K, hi[K-1] for i = K
__device__ __forceinline__ long long slot_edge(const BeatSlots s, int i) {
    const int32_t* b = s.b;
    if (i == 0) return (long long)b[0] - (b[1] - b[0]) / s.nd;
    if (i < s.K) return (long long)b[i] - (b[i] - b[i - 1]) / s.nd;
    const int d = b[s.K - 1] - b[s.K - 2];
    return (long long)b[s.K - 1] + d - d / s.nd;
}

// the largest i in [0, K-1] with edge(i) <= f (0 if there is none)
__device__ __forceinline__ int slot_of(const BeatSlots s, long long f) {
    int lo = 0, hi = s.K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (slot_edge(s, mid) <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// body(slot, share, the slot's length) for every slot that shares frames with [lo, hi), ascending.  Right for any span; the two
// kernels leave before it when the span lies outside all slots (with that test in here, the bars' kernel came out a branch longer).
template <class Body>
__device__ __forceinline__ void slot_walk(const BeatSlots s, long long lo, long long hi, Body body) {
    for (int i = slot_of(s, lo); i < s.K; ++i) {
        const long long es = slot_edge(s, i), en = slot_edge(s, i + 1);
        if (es >= hi) break;
        const long long share = min(hi, en) - max(lo, es);
        if (share > 0) body(i, share, en - es);
    }
}

// what launch_track_bars and launch_track_chords refuse alike, in the order of their codes; each keeps its own -2, parameters and buffers
template <class Args> inline int slot_check_programs(const Args& a) {
    return a.n_programs < 1 || a.n_programs > BAR_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs ? -1 : 0;
}
template <class Args> inline int slot_check_call(const Args& a) {
    if (a.near_div < 2 || !(a.frames_per_second > 0.0)) return -3;
    if (a.n_frames < 1 || a.n_frames > BAR_MAX_FRAMES || a.n < 0 || a.n > BAR_MAX_NOTES || (a.n && !a.notes)) return -4;
    if (a.max_beats < 1 || a.max_beats > BAR_MAX_BEATS) return -5;
    if (!a.beats || !a.beat_result || !a.chroma || !a.result) return -6;
    return 0;
}
