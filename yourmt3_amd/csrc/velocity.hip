// Note velocities from the audio: the level of the signal under each note's onset, mapped to a MIDI velocity (include/ymt3.h, note
// velocities).  The specification is the host path, note_velocities of yourmt3_amd/velocity.py, in f64; the sums here are f32 and in
// another order, so energies agree within the tolerance DESIGN section 21 measures, and counts, the measured / unmeasured split and
// the bytes of unmeasured records agree exactly.
// (a) velocity_measure_kernel, one wave per record, four records per workgroup: the lanes stride the window, so every audio read is a
//     coalesced row of 256 bytes and overlapping notes meet in L2.  A lane keeps the f32 power and, per harmonic, the real and imaginary
//     sums of its W / 64 samples; the trig argument is the exact integer phase word (step * k) mod 2^32, read as a signed fraction of
//     pi, never an f32 product of frequency and time.  A butterfly of __shfl_xor finishes the sums in a fixed order, so a record's
//     energy does not depend on the launch.  Lane 0 writes E, raises its class's peak with atomicMax on the bits of the non-negative
//     finite f32 (that order is the numbers' order) and bumps one of the two counters.
// (b) velocity_map_kernel, one lane per record, ordered after (a) by the stream: E and the class's peak -> the velocity, in f64, one
//     byte per record.  Without an energy buffer from the caller there is nowhere to keep E for 2^29 records, so
//     velocity_remeasure_kernel takes (b)'s place: one wave per record measures again (the same function, the same bits) and maps.
// No kernel waits on another workgroup and nothing spins.
#include "common.h"
#include "kernels.h"
#include "note_rule.h"

namespace {

constexpr int VEL_THREADS = 256;
constexpr int VEL_PER_BLOCK = VEL_THREADS / WAVE;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) v += __shfl_xor(v, x, WAVE);
    return v;
}

__device__ __forceinline__ bool record_is_drum(const DetokNote& r, int drum_program) { return r.is_drum != 0 || r.program == drum_program; }

// The energy of record r, the same value in every lane of the wave; NaN: the record is not measured.
__device__ __forceinline__ float measure(const VelocityArgs& a, const DetokNote& r, int lane) {
    const float nan = __uint_as_float(0x7fc00000u);
    const bool drum = record_is_drum(r, a.drum_program);
    if (!(fabs(r.onset) < INFINITY) || r.pitch < 0 || r.pitch >= NOTE_PITCHES) return nan;
    const uint32_t* steps = a.steps + r.pitch * VELOCITY_MAX_HARMONICS;
    if (!drum && steps[0] == 0) return nan;                                 // the fundamental's step is there iff f(pitch) < sr / 2
    double n0;
    {
#pragma clang fp contract(off)
        n0 = rint(r.onset * a.sample_rate);
    }
    // clamped in f64 before the conversion: [lo, lo + W) either meets [0, n_audio) or reads nothing
    const double lo_d = fmin(fmax(n0, -(double)a.W), (double)a.n_audio);
    const long long lo = (long long)lo_d;
    uint32_t st[VELOCITY_MAX_HARMONICS];
#pragma unroll
    for (int h = 0; h < VELOCITY_MAX_HARMONICS; ++h) st[h] = (!drum && h < a.H) ? steps[h] : 0u;
    float pw = 0.f, re[VELOCITY_MAX_HARMONICS], im[VELOCITY_MAX_HARMONICS];
#pragma unroll
    for (int h = 0; h < VELOCITY_MAX_HARMONICS; ++h) re[h] = im[h] = 0.f;
    for (int k = lane; k < a.W; k += WAVE) {
        const long long idx = lo + k;
        const float x = (idx >= 0 && idx < a.n_audio) ? a.audio[idx] : 0.f;
        const float v = a.window[k] * x;
        pw += v * v;
#pragma unroll
        for (int h = 0; h < VELOCITY_MAX_HARMONICS; ++h) {
            if (st[h] == 0u) continue;                                      // (uniform over the wave)
            const int phi = (int)(st[h] * (uint32_t)k);                     // the phase word, as a signed fraction of pi
            float s, c;
            sincospif((float)phi * 4.656612873077393e-10f, &s, &c);        // 2^-31
            re[h] += v * c;
            im[h] -= v * s;
        }
    }
    float e;
    if (drum) {
        e = wave_sum(pw) * a.p_scale;
    } else {
        float sum = 0.f;
#pragma unroll
        for (int h = 0; h < VELOCITY_MAX_HARMONICS; ++h) {
            if (st[h] == 0u) continue;
            const float R = wave_sum(re[h]), I = wave_sum(im[h]);
            sum += R * R + I * I;
        }
        e = sum * a.e_scale;
    }
    return fabsf(e) < INFINITY ? e : nan;
}

// E (not NaN) and the energy of peak_velocity -> the velocity, in f64
__device__ __forceinline__ uint8_t map_velocity(const VelocityArgs& a, float e, bool drum) {
#pragma clang fp contract(off)
    double ref = a.ref_energy;
    if (!(ref == ref)) ref = (double)a.peaks[drum ? 1 : 0];
    const double le = 10.0 * log10(fmax((double)e, 1e-12)), lr = 10.0 * log10(fmax(ref, 1e-12));
    const double u = (double)a.peak_velocity + a.velocity_per_db * (le - lr);
    return (uint8_t)fmin(fmax(rint(u), (double)a.min_velocity), 127.0);
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_measure_kernel(VelocityArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * VEL_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= a.n) return;
    if (i >= note_live_count(a.n, a.count)) {
        if (a.energy && lane == 0) a.energy[i] = __uint_as_float(0x7fc00000u);
        return;
    }
    const DetokNote r = a.notes[i];
    const float e = measure(a, r, lane);
    if (lane != 0) return;
    if (a.energy) a.energy[i] = e;
    if (e == e) {
        atomicAdd(&a.counts[0], 1);
        atomicMax(reinterpret_cast<unsigned*>(&a.peaks[record_is_drum(r, a.drum_program) ? 1 : 0]), __float_as_uint(e));
    } else {
        atomicAdd(&a.counts[1], 1);
    }
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_map_kernel(VelocityArgs a) {
    const long long i = (long long)blockIdx.x * VEL_THREADS + threadIdx.x;
    if (i >= a.n) return;
    if (i >= note_live_count(a.n, a.count)) { a.velocity[i] = 0; return; }
    const float e = a.energy[i];
    if (!(e == e)) { a.velocity[i] = (uint8_t)a.default_velocity; return; }
    a.velocity[i] = map_velocity(a, e, record_is_drum(a.notes[i], a.drum_program));
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_remeasure_kernel(VelocityArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * VEL_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= a.n) return;
    if (i >= note_live_count(a.n, a.count)) {
        if (lane == 0) a.velocity[i] = 0;
        return;
    }
    const DetokNote r = a.notes[i];
    const float e = measure(a, r, lane);
    if (lane != 0) return;
    a.velocity[i] = e == e ? map_velocity(a, e, record_is_drum(r, a.drum_program)) : (uint8_t)a.default_velocity;
}

}  // namespace

int launch_note_velocities(const VelocityArgs& a, hipStream_t stream) {
    if (a.n < 1 || a.n > VELOCITY_MAX_NOTES || !a.notes || !a.velocity || !a.peaks || !a.counts) return -1;
    if (a.n_audio < 0 || (a.n_audio && !a.audio)) return -2;
    if (a.W < VELOCITY_MIN_WINDOW || a.W > VELOCITY_MAX_WINDOW || a.H < 1 || a.H > VELOCITY_MAX_HARMONICS || !a.window || !a.steps) return -3;
    const unsigned waves = (unsigned)((a.n + VEL_PER_BLOCK - 1) / VEL_PER_BLOCK);
    velocity_measure_kernel<<<waves, VEL_THREADS, 0, stream>>>(a);
    if (a.energy) velocity_map_kernel<<<(unsigned)((a.n + VEL_THREADS - 1) / VEL_THREADS), VEL_THREADS, 0, stream>>>(a);
    else velocity_remeasure_kernel<<<waves, VEL_THREADS, 0, stream>>>(a);
    return 0;
}
