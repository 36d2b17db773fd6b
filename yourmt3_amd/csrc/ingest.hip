// Audio ingest, the step before the hot path: interleaved PCM (int16 or fp32, any
// channel count, any rate) -> mono mix -> polyphase FIR resample to the model rate -> zero-padded fixed-length
// segments, written straight into the (n_seg, segment_samples) layout ymt3_logmel reads.
//
//   y[n] = sum_j P[phase(n)][j] * x[k0(n) - j],   q = (n + r) * down,  phase = q % up,  k0 = q / up
//
// (the upfirdn form of TP: scipy/signal/_signaltools.py resample_poly; the taps P and the alignment r are derived on
// the host in runtime.hip).  One workgroup produces 256 consecutive output samples: the input span they need is
// mono-mixed once into LDS with coalesced reads of the interleaved frames (HBM sees every PCM byte once per
// workgroup span, ~1.1x overall), each thread then walks its own phase row of the tap table (16-byte loads, L2
// resident: <= 40 KB per rate pair).  HBM-bound streaming work; fp32 throughout.
// Oracle: oracle/ingest_oracle.py::ingest.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int OUT_PER_WG = 256;

// The two pieces of arithmetic the one-shot kernel and the streaming kernels share.  They are the ONLY place a frame is mixed and
// a tap row is summed: the streaming outputs equal the one-shot ones bit for bit because both run these instructions -- the same
// products, in the same order, contracted the same way.
template <bool S16>
__device__ __forceinline__ float mono_frame(const void* pcm, long long k, int n_channels, float inv_c) {
    if (S16) {
        const short* p = static_cast<const short*>(pcm) + k * n_channels;
        float s = 0.f;
        for (int c = 0; c < n_channels; ++c) s += (float)p[c] * (1.0f / 32768.0f);
        return s * inv_c;
    } else {
        const float* p = static_cast<const float*>(pcm) + k * n_channels;
        float s = 0.f;
        for (int c = 0; c < n_channels; ++c) s += p[c];
        return s * inv_c;
    }
}

// sum_j P[phase][j] * xw[base - j], j ascending; `base` is the window index of x[k0]
__device__ __forceinline__ float tap_sum(const float* taps, int Jp, int phase, int base, const float* xw) {
    float y = 0.f;
    const float4* row = reinterpret_cast<const float4*>(taps + (size_t)phase * Jp);
    for (int j4 = 0; j4 < Jp / 4; ++j4) {
        const float4 t = row[j4];
        const int i = base - 4 * j4;
        // taps beyond J are zero and the window below k_lo is never read: clamp the index, keep the product
        y += t.x * xw[max(i, 0)];
        y += t.y * xw[max(i - 1, 0)];
        y += t.z * xw[max(i - 2, 0)];
        y += t.w * xw[max(i - 3, 0)];
    }
    return y;
}

template <bool S16>
__global__ __launch_bounds__(OUT_PER_WG) void ingest_kernel(IngestArgs a) {
    extern __shared__ float xw[];                                   // mono input window of this workgroup
    const int tid = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * OUT_PER_WG;
    if (n0 >= a.n_out) {                                            // pure padding tail
        const long long n = n0 + tid;
        if (n < a.n_total) a.out[n] = 0.f;
        return;
    }
    long long n_last = n0 + OUT_PER_WG - 1;
    if (n_last >= a.n_out) n_last = a.n_out - 1;
    const long long k_hi = ((n_last + a.r) * a.down) / a.up;        // newest input frame any output here needs
    const long long k_lo = ((n0 + a.r) * a.down) / a.up - (a.J - 1);
    const int W = (int)(k_hi - k_lo + 1);                           // <= a.window (checked on the host)
    const float inv_c = 1.0f / (float)a.n_channels;
    for (int i = tid; i < W; i += OUT_PER_WG) {
        const long long k = k_lo + i;
        float v = 0.f;
        if (k >= 0 && k < a.n_in) {
            v = mono_frame<S16>(a.pcm, k, a.n_channels, inv_c);
        }
        xw[i] = v;
    }
    __syncthreads();
    const long long n = n0 + tid;
    if (n >= a.n_total) return;
    float y = 0.f;
    if (n < a.n_out) {
        const long long q = (n + a.r) * a.down;
        const int phase = (int)(q % a.up);
        const int base = (int)(q / a.up - k_lo);                    // xw index of x[k0]
        y = tap_sum(a.taps, a.Jp, phase, base, xw);
    }
    a.out[n] = y;
}

// ---------------------------------------------------------------- streaming form (include/ymt3.h, streaming ingest)
// Every arriving frame is mixed to mono once, into a ring that keeps frame k at hist[k & mask]; the ring holds at least J - 1 +
// max_chunk_frames frames, so a push's new frames never land on a frame its own outputs still read.
template <bool S16>
__global__ __launch_bounds__(OUT_PER_WG) void ingest_mix_kernel(IngestStreamArgs a) {
    const long long i = (long long)blockIdx.x * OUT_PER_WG + threadIdx.x;
    if (i >= a.n_new) return;
    a.hist[(a.n_in - a.n_new + i) & a.hist_mask] = mono_frame<S16>(a.pcm, i, a.n_channels, 1.0f / (float)a.n_channels);
}

// Outputs [g0, n_total), 256 per workgroup.  n < n_done: already computed by an earlier push, copied from the partial segment it
// was kept in; n_done <= n < n_end: resampled from the ring (frames outside [0, n_in) are zero, as in the one-shot kernel); beyond:
// the padding of the last segment.  Samples below n_row_end go to the caller's rows, the others start the next partial segment.
__global__ __launch_bounds__(OUT_PER_WG) void ingest_stream_kernel(IngestStreamArgs a) {
    extern __shared__ float xw[];
    const int tid = threadIdx.x;
    const long long n0 = a.g0 + (long long)blockIdx.x * OUT_PER_WG;
    const long long nc0 = n0 > a.n_done ? n0 : a.n_done;            // first output this workgroup computes
    long long n_last = n0 + OUT_PER_WG - 1;
    if (n_last >= a.n_end) n_last = a.n_end - 1;
    long long k_lo = 0;
    if (nc0 <= n_last) {
        const long long k_hi = ((n_last + a.r) * a.down) / a.up;
        k_lo = ((nc0 + a.r) * a.down) / a.up - (a.J - 1);
        const int W = (int)(k_hi - k_lo + 1);                       // <= a.window: at most 256 consecutive outputs
        for (int i = tid; i < W; i += OUT_PER_WG) {
            const long long k = k_lo + i;
            xw[i] = (k >= 0 && k < a.n_in) ? a.hist[k & a.hist_mask] : 0.f;
        }
    }
    __syncthreads();
    const long long n = n0 + tid;
    if (n >= a.n_total) return;
    float y = 0.f;
    if (n < a.n_done) {
        y = a.part_old[n - a.n_row0];
    } else if (n < a.n_end) {
        const long long q = (n + a.r) * a.down;
        y = tap_sum(a.taps, a.Jp, (int)(q % a.up), (int)(q / a.up - k_lo), xw);
    }
    if (n < a.n_row_end) a.out[n - a.n_row0] = y;
    else a.part_new[n - a.n_row_end] = y;
}

}  // namespace

int launch_ingest_stream(const IngestStreamArgs& a, hipStream_t stream) {
    if (a.up <= 0 || a.down <= 0 || a.J <= 0 || a.Jp % 4 || a.Jp < a.J || a.n_channels <= 0 || a.window <= 0) return -1;
    const size_t lds = (size_t)a.window * sizeof(float);
    if (lds > 64 * 1024) return -2;
    if (a.n_new > 0) {
        const long long blocks = (a.n_new + OUT_PER_WG - 1) / OUT_PER_WG;
        if (blocks > 0x7fffffffLL) return -3;
        if (a.s16) ingest_mix_kernel<true><<<(int)blocks, OUT_PER_WG, 0, stream>>>(a);
        else ingest_mix_kernel<false><<<(int)blocks, OUT_PER_WG, 0, stream>>>(a);
    }
    if (a.n_total > a.g0) {
        const long long blocks = (a.n_total - a.g0 + OUT_PER_WG - 1) / OUT_PER_WG;
        if (blocks > 0x7fffffffLL) return -3;
        ingest_stream_kernel<<<(int)blocks, OUT_PER_WG, lds, stream>>>(a);
    }
    return 0;
}

int launch_ingest(const IngestArgs& a, hipStream_t stream) {
    if (a.n_total <= 0) return 0;
    if (a.up <= 0 || a.down <= 0 || a.J <= 0 || a.Jp % 4 || a.Jp < a.J || a.n_channels <= 0 || a.window <= 0) return -1;
    const size_t lds = (size_t)a.window * sizeof(float);
    if (lds > 64 * 1024) return -2;
    const long long blocks = (a.n_total + OUT_PER_WG - 1) / OUT_PER_WG;
    if (blocks > 0x7fffffffLL) return -3;
    if (a.s16) ingest_kernel<true><<<(int)blocks, OUT_PER_WG, lds, stream>>>(a);
    else ingest_kernel<false><<<(int)blocks, OUT_PER_WG, lds, stream>>>(a);
    return 0;
}
