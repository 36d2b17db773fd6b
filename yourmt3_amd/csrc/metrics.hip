// Device note metrics: two sets of note records -> the integers of onset / onset+offset / drum F1 (include/ymt3.h, note metrics).  The
// specification is the host path, note_metrics of yourmt3_amd/metrics.py; tests/metrics_model.py states this file's algorithm in plain
// Python.  Integer work plus, per compared pair, one f64 subtract, multiply, rint and divide with contraction off: nothing here rounds
// differently from the host.
//
// A counted record enters the bucket of its instrument-aware key, program * 128 + pitch, and, if pitched, of its agnostic key,
// n_programs * 128 + pitch: (n_programs + 1) * 128 keys per side, most of them empty.
// (a) metrics_notes_kernel<false>, one lane per record and side: validity (note_rule.h), the two keys, a per-key histogram; skipped records are counted.
// (b) metrics_scan_kernel, one workgroup per side: exclusive scan of the histogram into bucket offsets, and n_ref / n_est of every row
//     (the sum of the row's 128 counters) stored into the result.
// (c) metrics_notes_kernel<true>: the same lanes scatter their (onset, offset) into the buckets through a per-key cursor.
// (d) metrics_keys_kernel, one wave per key that has notes on both sides.  A key whose working set fits KEY_LDS_BYTES is copied into LDS,
//     a larger one works in the object's global scratch through the same pointers.  Both buckets are sorted by onset (a bitonic network
//     whose comparators all point upwards, so that slots beyond the bucket act as +inf and are never touched).  Sorted, the estimates a
//     reference can hit by onset are one interval [lo, hi), found by two binary searches, and both ends grow with the reference's onset.
//       - onset metric: every reference in order takes the earliest free estimate of its interval: a maximum matching, by that monotony;
//       - onset+offset metric: Kuhn's augmenting paths over the interval's candidates, depth first with an explicit stack, the 64 lanes
//         testing 64 candidates at a time.  Visited marks are the search's root index; a search visits an estimate at most once and a
//         frame's cursor only advances, so the kernel ends on any input.  Nothing waits on another workgroup.
//       - a drum key never looks at offsets: its onset matching counts for both metrics.
//     One atomic per key and metric adds TP to the key's row.
// Worst case: the searches are cubic in the notes of ONE key that lie within one onset window of each other; the sort is n log^2 n.
#include "common.h"
#include "kernels.h"
#include "note_rule.h"

namespace {

constexpr int NOTE_THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr int KEY_LDS_BYTES = 24576;      // 32 bytes per reference + 24 per estimate of a key: 6 workgroups per CU
constexpr int REF_BYTES = 32, EST_BYTES = 24;

__device__ __forceinline__ int n_keys(const MetricsArgs& a) { return (a.n_programs + 1) * METRICS_PITCHES; }

// d(a, b) <= tol with d = rint(|a - b| * 1e4) / 1e4: that subtract, multiply, round-half-even and divide in f64.  A NaN distance misses.
__device__ __forceinline__ bool within(double x, double y, double tol) {
#pragma clang fp contract(off)
    const double s = fabs(x - y) * 1e4;
    const double d = rint(s) / 1e4;
    return d <= tol;
}

// max(offset_min_tol, offset_ratio * (off - on)), not rounded; a NaN product (inf - inf) gives the minimum
__device__ __forceinline__ double offset_tol(const MetricsArgs& a, double on, double off) {
#pragma clang fp contract(off)
    const double dur = off - on;
    const double t = a.offset_ratio * dur;
    return t > a.offset_min_tol ? t : a.offset_min_tol;
}

template <bool SCATTER>
__global__ __launch_bounds__(NOTE_THREADS) void metrics_notes_kernel(MetricsArgs a) {
    const int side = blockIdx.y;
    const long long i = (long long)blockIdx.x * NOTE_THREADS + threadIdx.x;
    if (i >= note_live_count(side ? a.n_est : a.n_ref, side ? a.est_count : a.ref_count)) return;
    const DetokNote r = (side ? a.est : a.ref)[i];
    const NoteClass c = note_classify(r, a.n_programs, a.drum_program);
    if (!c.counted) {
        if (!SCATTER) atomicAdd(&a.counts[(a.n_programs + 1) * 6 + side], 1);
        return;
    }
    const int NK = n_keys(a);
    const int aware = c.prog * METRICS_PITCHES + r.pitch, agnostic = a.n_programs * METRICS_PITCHES + r.pitch;
    if (!SCATTER) {
        unsigned* h = a.hist + (long long)side * NK;
        atomicAdd(&h[aware], 1u);
        if (!c.drum) atomicAdd(&h[agnostic], 1u);
    } else {
        unsigned* cur = a.cursor + (long long)side * NK;
        double2* T = side ? a.t_est : a.t_ref;
        const long long cap = 2 * (side ? a.max_est : a.max_ref);
        const unsigned p0 = atomicAdd(&cur[aware], 1u);
        if (p0 < cap) T[p0] = make_double2(r.onset, r.offset);
        if (!c.drum) {
            const unsigned p1 = atomicAdd(&cur[agnostic], 1u);
            if (p1 < cap) T[p1] = make_double2(r.onset, r.offset);
        }
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void metrics_scan_kernel(MetricsArgs a) {
    __shared__ unsigned wsum[SCAN_THREADS / WAVE];
    const int side = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NK = n_keys(a);
    const unsigned* hist = a.hist + (long long)side * NK;
    unsigned* off = a.off + (long long)side * (NK + 1);
    unsigned* cur = a.cursor + (long long)side * NK;
    // every thread owns `per` consecutive keys
    const int per = (NK + SCAN_THREADS - 1) / SCAN_THREADS;
    const int k0 = min(tid * per, NK), k1 = min(k0 + per, NK);
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
    unsigned o = incl - mine;
    for (int w = 0; w < wave; ++w) o += wsum[w];
    for (int k = k0; k < k1; ++k) {
        off[k] = o;
        cur[k] = o;
        o += hist[k];
    }
    if (tid == SCAN_THREADS - 1) off[NK] = o;                           // (its k1 is NK: the total)
    // n_ref / n_est of every row, both metrics: the sum of the row's 128 counters
    for (int row = wave; row <= a.n_programs; row += SCAN_THREADS / WAVE) {
        unsigned s = hist[row * METRICS_PITCHES + lane] + hist[row * METRICS_PITCHES + WAVE + lane];
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) s += __shfl_xor(s, x, WAVE);
        if (lane == 0) {
            a.counts[(row * 2 + 0) * 3 + 1 + side] = (int32_t)s;
            a.counts[(row * 2 + 1) * 3 + 1 + side] = (int32_t)s;
        }
    }
}

// ascending by onset, any n: a bitonic network whose comparators all put the smaller onset at the lower index, so that the slots from n
// to the next power of two behave as +inf without existing (a comparator that reaches one has nothing to do)
__device__ void sort_by_onset(double2* T, int n, int lane) {
    if (n < 2) return;
    int N = 2;
    while (N < n) N <<= 1;
    auto cswap = [&](int lo, int hi) {
        if (hi >= n) return;
        const double2 x = T[lo], y = T[hi];
        if (x.x > y.x) {
            T[lo] = y;
            T[hi] = x;
        }
    };
    for (int k = 2, s = 0; k <= N; k <<= 1, ++s) {                      // s = log2(k / 2)
        for (int t = lane; t < (N >> 1); t += WAVE) {                   // block of k: slot w against its mirror image
            const int base = (t >> s) << (s + 1), w = t & ((k >> 1) - 1);
            cswap(base + w, base + k - 1 - w);
        }
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int t = lane; t < (N >> 1); t += WAVE) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear; the partner is lo + j
                cswap(lo, lo + j);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(WAVE) void metrics_keys_kernel(MetricsArgs a) {
    extern __shared__ double2 lds[];
    const int key = blockIdx.x, lane = threadIdx.x;
    const int NK = n_keys(a);
    const unsigned rb = a.off[key], re = a.off[key + 1], eb = a.off[NK + 1 + key], ee = a.off[NK + 1 + key + 1];
    if (re > 2 * a.max_ref || ee > 2 * a.max_est || re <= rb || ee <= eb) return;      // (an empty side: TP = 0)
    const int nr = (int)(re - rb), ne = (int)(ee - eb);
    double2 *R = a.t_ref + rb, *E = a.t_est + eb;
    int2 *win = a.win + rb, *stk = a.stack + rb;
    int *match = a.match + eb, *visit = a.visit + eb;
    if ((long long)nr * REF_BYTES + (long long)ne * EST_BYTES <= KEY_LDS_BYTES) {
        double2* r2 = lds;
        double2* e2 = r2 + nr;
        for (int i = lane; i < nr; i += WAVE) r2[i] = R[i];
        for (int j = lane; j < ne; j += WAVE) e2[j] = E[j];
        R = r2;
        E = e2;
        win = reinterpret_cast<int2*>(e2 + ne);
        stk = win + nr;
        match = reinterpret_cast<int*>(stk + nr);
        visit = match + ne;
    }
    __syncthreads();
    sort_by_onset(R, nr, lane);
    sort_by_onset(E, ne, lane);
    // the interval of estimates a reference can hit by onset: those before it are too early, those from its end on too late
    const double otol = a.onset_tol;
    for (int i = lane; i < nr; i += WAVE) {
        const double on = R[i].x;
        int l = 0, h = ne;
        while (l < h) {
            const int m = (l + h) >> 1;
            const double e = E[m].x;
            if (e < on && !within(on, e, otol)) l = m + 1;
            else h = m;
        }
        const int lo = l;
        h = ne;
        while (l < h) {
            const int m = (l + h) >> 1;
            const double e = E[m].x;
            if (e > on && !within(on, e, otol)) h = m;
            else l = m + 1;
        }
        win[i] = make_int2(lo, l);
    }
    for (int j = lane; j < ne; j += WAVE) {
        match[j] = -1;
        visit[j] = -1;
    }
    __syncthreads();
    // onset metric: earliest free estimate of the interval (every lane walks the same path)
    int tp_on = 0;
    for (int i = 0, j = 0; i < nr; ++i) {
        const int2 w = win[i];
        if (w.x > j) j = w.x;
        if (j < w.y && within(R[i].x, E[j].x, otol)) {
            ++tp_on;
            ++j;
        }
    }
    const int row = key / METRICS_PITCHES;                              // the agnostic keys are row n_programs
    int tp_off = tp_on;
    if (row != a.drum_program) {
        tp_off = 0;
        for (int root = 0; root < nr && tp_off < tp_on; ++root) {       // (an onset+offset matching is an onset matching: never more than tp_on)
            int sp = 0, u = root, c = win[root].x;
            for (;;) {
                const double2 r = R[u];
                const int hi = win[u].y;
                const double tol = offset_tol(a, r.x, r.y);
                int found = -1;
                for (int base = c; base < hi; base += WAVE) {
                    const int j = base + lane;
                    bool ok = false;
                    if (j < hi && visit[j] != root) {
                        const double2 e = E[j];
                        ok = within(r.x, e.x, otol) && within(r.y, e.y, tol);
                    }
                    const unsigned long long mask = __ballot(ok);
                    if (mask) {
                        found = base + __ffsll((long long)mask) - 1;
                        break;
                    }
                }
                if (found < 0) {                                        // this reference is exhausted: back to the one that led here
                    if (sp == 0) break;
                    --sp;
                    const int2 f = stk[sp];
                    u = __builtin_amdgcn_readfirstlane(f.x);
                    c = __builtin_amdgcn_readfirstlane(f.y);
                    continue;
                }
                const int w = __builtin_amdgcn_readfirstlane(match[found]);
                __syncthreads();                                        // every lane has read match[found] and the marks
                if (lane == 0) {
                    visit[found] = root;
                    stk[sp] = make_int2(u, found + 1);
                }
                __syncthreads();
                if (w < 0) {                                            // a free estimate: every frame takes the estimate it stopped at
                    for (int k = lane; k <= sp; k += WAVE) {
                        const int2 f = stk[k];
                        match[f.y - 1] = f.x;
                    }
                    __syncthreads();
                    ++tp_off;
                    break;
                }
                if (sp + 1 >= nr) break;                                // (unreachable: the references on a path are distinct)
                ++sp;
                u = w;
                c = win[w].x;
            }
        }
    }
    if (lane == 0) {
        if (tp_on) atomicAdd(&a.counts[(row * 2 + 0) * 3], tp_on);
        if (tp_off) atomicAdd(&a.counts[(row * 2 + 1) * 3], tp_off);
    }
}

}  // namespace

int launch_metrics(const MetricsArgs& a, hipStream_t stream) {
    if (a.n_programs < 1 || a.n_programs > METRICS_MAX_PROGRAMS || a.drum_program < 0 || a.drum_program >= a.n_programs) return -1;
    if (a.max_ref < 1 || a.max_ref > METRICS_MAX_NOTES || a.max_est < 1 || a.max_est > METRICS_MAX_NOTES) return -2;
    if (a.n_ref < 0 || a.n_ref > a.max_ref || a.n_est < 0 || a.n_est > a.max_est) return -3;
    const int NK = (a.n_programs + 1) * METRICS_PITCHES;
    if (hipMemsetAsync(a.counts, 0, ((size_t)(a.n_programs + 1) * 6 + 2) * sizeof(int32_t), stream) != hipSuccess) return -5;
    const long long n = a.n_ref > a.n_est ? a.n_ref : a.n_est;
    if (n == 0) return 0;
    if (hipMemsetAsync(a.hist, 0, (size_t)2 * NK * sizeof(unsigned), stream) != hipSuccess) return -5;
    const dim3 grid((unsigned)((n + NOTE_THREADS - 1) / NOTE_THREADS), 2);
    metrics_notes_kernel<false><<<grid, NOTE_THREADS, 0, stream>>>(a);
    metrics_scan_kernel<<<2, SCAN_THREADS, 0, stream>>>(a);
    if (a.n_ref == 0 || a.n_est == 0) return 0;                         // nothing can match: the rows' note counts are the result
    metrics_notes_kernel<true><<<grid, NOTE_THREADS, 0, stream>>>(a);
    metrics_keys_kernel<<<NK, WAVE, KEY_LDS_BYTES, stream>>>(a);
    return 0;
}
