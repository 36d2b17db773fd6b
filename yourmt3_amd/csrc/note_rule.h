// The one rule for which note record counts and which frames it covers, shared by metrics.hip, roll.hip and align.hip.  The host
// specification is classify and _cells of yourmt3_amd/metrics.py: every piece here computes what they compute, to the last bit.
#pragma once
#include "kernels.h"

// records the side has: min(n, max(*count, 0)) under a device count, n without one
__device__ __forceinline__ long long note_live_count(long long n, const int32_t* count) {
    if (!count) return n;
    const long long c = max(*count, 0);
    return min(n, c);
}

// prog: the record's row, drum_program for a drum whatever `program` says; a record that is not counted is skipped by every consumer
struct NoteClass { int prog; bool drum, counted; };
__device__ __forceinline__ NoteClass note_classify(const DetokNote r, int n_programs, int drum_program) {
    NoteClass c;
    c.prog = r.is_drum != 0 ? drum_program : r.program;
    c.drum = c.prog == drum_program;
    c.counted = r.onset == r.onset && r.pitch >= 0 && r.pitch < NOTE_PITCHES && c.prog >= 0 && c.prog < n_programs &&
                (c.drum || r.offset == r.offset);                          // NaN by self-comparison; a drum needs no offset
    return c;
}

// [F(on), max(F(off), F(on) + 1)) clipped to [0, n_frames) in f64: +-inf and huge times never reach an integer conversion.
// false: the span is empty; else 0 <= *f_lo < *f_hi <= n_frames.
__device__ __forceinline__ bool note_frame_span(const DetokNote r, bool drum, double frames_per_second, long long n_frames, long long* f_lo,
                                                long long* f_hi) {
#pragma clang fp contract(off)
    const double f0 = rint(r.onset * frames_per_second);
    double f1 = f0 + 1.0;
    if (!drum) {
        const double fo = rint(r.offset * frames_per_second);
        f1 = fo > f1 ? fo : f1;
    }
    const double lo = f0 > 0.0 ? f0 : 0.0, hi = f1 < (double)n_frames ? f1 : (double)n_frames;
    if (!(lo < hi)) return false;
    *f_lo = (long long)lo;
    *f_hi = (long long)hi;
    return true;
}
