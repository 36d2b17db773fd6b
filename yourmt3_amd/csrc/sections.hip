// Sections over note records and tracked beats: per-beat pitch-class content with context, a checkerboard novelty over the beats'
// self-similarity, boundaries at its peaks and a letter per section from the sections' diagonals (include/ymt3.h, sections).  The
// specification is the host path, track_sections of yourmt3_amd/sections.py; tests/section_model.py states the rules as plain loops.
// Everything is an integer (times stay f64 until they are known to lie inside the frames): every output equals the host's.
// The number of beats K and the number of sections stay on the device: every launch is sized by the object's max_beats, by the number
// of records or by max_sections, and nothing is read back.  Scratch is linear in max_beats plus 64 x 64 bytes: no K x K matrix in memory.
// (a) section_clear_kernel zeroes c[0, K)[12], result[8] and the accumulators.
// (b) section_features_kernel, one lane per record: chords.hip's features without the bass (note_rule.h, beat_slots.h).
// (c) section_context_kernel, one lane per beat: the 64-bit normalisation of the w rows it sums, f as twelve 16-bit words and the flag.
// (d) section_novelty_kernel, the hot one: one workgroup per tile of 64 beats.  The f rows of [i0 - L, i0 + 64 + L) go into LDS once, rows
//     7 words apart (odd: lanes on consecutive rows hit distinct banks).  Then every S(r, r + d), 0 <= d < 2L, of those rows is formed
//     ONCE into LDS, 16 bits each (S <= 32768), rows 2L + 2 halfwords apart: a wave writes and reads consecutive halfwords of a row,
//     and with L + 1 words between rows the rows a 32-lane group touches lie on distinct banks.  A beat's novelty is one wave's sum:
//     with g = (t[L_i-1] .. t[0], -t[0] .. -t[L_i-1]) over the rows [i - L_i, i + L_i) the four tapered quadrants are g S g, and S is
//     symmetric, so the wave sums g[r] g[r+d] S(r, r+d) over the upper triangle (twice off the diagonal) and reduces by __shfl_xor.
//     Integer sums: exact in any order.  Lane 0 stores nov[i] and raises the candidates' maximum by a 64-bit atomicMax (biased by 2^62).
// (e) section_peaks_kernel, one lane per candidate: the three peak conditions, the +-m comparison read from nov.
// (f) section_select_kernel, one workgroup: with more than M - 1 peaks the (M - 1)-th largest key (nov << 21 | 2^21 - 1 - i) is found by
//     rank counting among the peaks' keys in LDS (up to 4096 of them; beyond that by M - 1 rounds of a block-wide maximum below the
//     previous one), and the section starts are written in time order by a prefix count.
// (g) section_pairs_kernel, one workgroup per pair (s, t), t <= s: the diagonal's sum of D from f, its mean and the length test into a
//     64 x 64 table; t = s finds whether section s is silent.  Pairs beyond the section count leave at once.
// (h) section_label_kernel, one lane per beat: every workgroup's first wave makes the serial pass over at most 64 sections from the
//     table (a ballot per section), then every lane finds its section by a binary search and writes section[i].
// No kernel waits on another workgroup and nothing spins.
#include "common.h"
#include "kernels.h"
#include "beat_slots.h"
#include "note_rule.h"

namespace {

constexpr int SECTION_THREADS = 256;
constexpr int SECTION_CLEAR_BLOCKS = 256;
constexpr int SECTION_TILE = 64;                                            // beats per workgroup of the novelty kernel
constexpr int SECTION_ROWS = SECTION_TILE + 2 * SECTION_MAX_KERNEL;         // 192 rows of f at most
constexpr int SECTION_F_ROW = 14;                                           // LDS halfwords per row of f: 7 words, the last one padding
constexpr int SECTION_S_ROW = 2 * SECTION_MAX_KERNEL + 2;                   // LDS halfwords per row of S at L = 64
constexpr int SECTION_SELECT_THREADS = 1024;
constexpr int SECTION_SELECT_KEYS = 4096;                                   // peak keys that the select kernel ranks in LDS (32 KiB)
constexpr int SECTION_COUNT_AT = SECTION_MAX_SECTIONS + 1;                  // where starts[] keeps the number of sections
constexpr unsigned long long SECTION_BIAS = 1ull << 62;                     // |nov| < 2^41: nov + bias is positive, 0 means no candidate
constexpr unsigned SECTION_SILENT = 255u;

__device__ __forceinline__ bool section_candidate(const SectionArgs& a, int i) { return i >= 1 && (!a.metre || (a.metre[i] & 255) == 0); }

// the key (nov, -i) of a peak: nov in (0, 2^41), i < 2^21
__device__ __forceinline__ unsigned long long section_key(long long nov, int i) { return ((unsigned long long)nov << 21) | (unsigned)((1 << 21) - 1 - i); }

// sum over the twelve pitch classes of |x - y|, the rows as six words of two 16-bit values
__device__ __forceinline__ unsigned section_row_distance(const unsigned (&x)[6], const unsigned (&y)[6]) {
    unsigned d = 0u;
#pragma unroll
    for (int j = 0; j < 6; ++j) d = __builtin_amdgcn_sad_u16(x[j], y[j], d);
    return d;
}

__global__ __launch_bounds__(SECTION_THREADS) void section_clear_kernel(SectionArgs a) {
    const long long stride = (long long)gridDim.x * SECTION_THREADS, t0 = (long long)blockIdx.x * SECTION_THREADS + threadIdx.x;
    const long long K = beat_count(a.beat_result, a.max_beats);
    for (long long i = t0; i < K * 12; i += stride) a.chroma[i] = 0u;
    if (t0 < 8) a.result[t0] = 0;
    if (t0 < SECTION_ACC_WORDS) a.acc[t0] = 0ull;
    if (t0 == 0) a.starts[SECTION_COUNT_AT] = 0;
}

__global__ __launch_bounds__(SECTION_THREADS) void section_features_kernel(SectionArgs a) {
    const long long i = (long long)blockIdx.x * SECTION_THREADS + threadIdx.x;
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
    slot_walk(sl, lo, hi, [&](int s, long long share, long long) { atomicAdd(&a.chroma[(long long)s * 12 + pc], (unsigned)share); });
}

__global__ __launch_bounds__(SECTION_THREADS) void section_context_kernel(SectionArgs a) {
    const long long i = (long long)blockIdx.x * SECTION_THREADS + threadIdx.x;
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2 || i >= K) return;
    unsigned f[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    unsigned empty = 0u;
    for (int d = 0; d < a.context; ++d) {
        const long long j = min(i + d, (long long)K - 1);
        const uint4* cp = reinterpret_cast<const uint4*>(a.chroma + j * 12);
        const uint4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
        const unsigned c[12] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w};
        unsigned long long sum = 0ull;
#pragma unroll
        for (int pc = 0; pc < 12; ++pc) sum += c[pc];
        if (d == 0) empty = sum == 0ull;
        if (!sum) sum = 1ull;
#pragma unroll
        for (int pc = 0; pc < 12; ++pc) f[pc] += (unsigned)((unsigned long long)c[pc] * 1024ull / sum);
    }
    uint4* out = reinterpret_cast<uint4*>(a.f + i * SECTION_F_WORDS);
    out[0] = make_uint4(f[0] | f[1] << 16, f[2] | f[3] << 16, f[4] | f[5] << 16, f[6] | f[7] << 16);
    out[1] = make_uint4(f[8] | f[9] << 16, f[10] | f[11] << 16, empty, 0u);
}

__global__ __launch_bounds__(SECTION_THREADS) void section_novelty_kernel(SectionArgs a) {
    __shared__ unsigned fs[SECTION_ROWS * SECTION_F_ROW / 2];
    __shared__ unsigned short ss[SECTION_ROWS * SECTION_S_ROW];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int K = beat_count(a.beat_result, a.max_beats);
    const long long first = (long long)blockIdx.x * SECTION_TILE;
    if (K < 2 || first >= K) return;
    const int i0 = (int)first, L = a.kernel_beats, band = 2 * L, s_row = band + 2;
    const int row0 = max(i0 - L, 0), rows = min(i0 + SECTION_TILE + L, K) - row0;          // rows <= SECTION_ROWS
    const unsigned* fg = reinterpret_cast<const unsigned*>(a.f);
    for (int x = tid; x < rows * 6; x += SECTION_THREADS) {
        const int r = x / 6, j = x - 6 * r;
        fs[r * (SECTION_F_ROW / 2) + j] = fg[(long long)(row0 + r) * (SECTION_F_WORDS / 2) + j];
    }
    __syncthreads();
    const int full = 2048 * a.context;
    for (int x = tid; x < rows * band; x += SECTION_THREADS) {
        const int r = x / band, d = x - band * r;
        if (r + d >= rows) continue;
        unsigned p[6], q[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            p[j] = fs[r * (SECTION_F_ROW / 2) + j];
            q[j] = fs[(r + d) * (SECTION_F_ROW / 2) + j];
        }
        ss[r * s_row + d] = (unsigned short)(full - (int)section_row_distance(p, q));
    }
    __syncthreads();
    for (int bi = wave; bi < SECTION_TILE; bi += SECTION_THREADS / WAVE) {
        const int i = i0 + bi;
        if (i >= K) break;
        const int Li = min(L, min(i, K - i)), n = 2 * Li, base = i - Li - row0;                // rows [base, base + n) of the tile's
        long long sum = 0;
        if (n) {
            const int step_r = WAVE / n, step_d = WAVE - step_r * n;
            int r = lane / n, d = lane - r * n;
            while (r < n) {
                if (r + d < n) {
                    const int c = r + d;
                    const int g0 = r < Li ? L - (Li - 1 - r) : -(L - (r - Li)), g1 = c < Li ? L - (Li - 1 - c) : -(L - (c - Li));
                    const int term = g0 * g1 * (int)ss[(base + r) * s_row + d];
                    sum += d ? 2 * term : term;
                }
                d += step_d;
                r += step_r;
                if (d >= n) {
                    d -= n;
                    ++r;
                }
            }
        }
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x, WAVE);
        if (lane == 0) {
            a.nov[i] = sum;
            if (a.novelty) a.novelty[i] = sum;
            if (section_candidate(a, i)) atomicMax(&a.acc[0], (unsigned long long)sum + SECTION_BIAS);
        }
    }
}

__global__ __launch_bounds__(SECTION_THREADS) void section_peaks_kernel(SectionArgs a) {
    const long long at = (long long)blockIdx.x * SECTION_THREADS + threadIdx.x;
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2 || at >= K) return;
    const int i = (int)at;
    bool peak = false;
    if (section_candidate(a, i)) {
        const long long v = a.nov[i], top = (long long)(a.acc[0] - SECTION_BIAS);            // i is a candidate: acc[0] is not 0
        if (v > 0 && (long long)a.peak_div * v >= top) {
            peak = true;
            const int j1 = min(K - 1, i + a.min_len);
            for (int j = max(1, i - a.min_len); j <= j1 && peak; ++j) {
                if (j == i || !section_candidate(a, j)) continue;
                const long long u = a.nov[j];
                if (u > v || (u == v && j < i)) peak = false;
            }
        }
    }
    a.peak[i] = peak ? 1 : 0;
    if (peak) atomicAdd(&a.acc[1], 1ull);
}

// the block's maximum; every thread gets it (red: one word per wave)
__device__ __forceinline__ unsigned long long section_block_max(unsigned long long v, unsigned long long* red, int lane, int wave, int n_waves) {
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const unsigned long long o = __shfl_xor(v, x, WAVE);
        v = o > v ? o : v;
    }
    if (lane == 0) red[wave] = v;
    __syncthreads();
    for (int w = 0; w < n_waves; ++w) v = red[w] > v ? red[w] : v;
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(SECTION_SELECT_THREADS) void section_select_kernel(SectionArgs a) {
    constexpr int WAVES = SECTION_SELECT_THREADS / WAVE;
    __shared__ unsigned long long keys[SECTION_SELECT_KEYS];
    __shared__ unsigned long long red[WAVES];
    __shared__ int counts[WAVES];
    __shared__ int n_keys;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int K = beat_count(a.beat_result, a.max_beats);
    if (K < 2) return;
    const long long n_peaks = (long long)a.acc[1];
    const int keep = a.max_sections - 1;
    unsigned long long least = 0ull;                                        // the smallest key that is kept
    if (n_peaks > keep && keep == 0) {
        least = ~0ull;
    } else if (n_peaks > keep && n_peaks <= SECTION_SELECT_KEYS) {          // rank counting among the peaks, their keys in LDS in any order
        if (tid == 0) {
            n_keys = 0;
            red[0] = ~0ull;
        }
        __syncthreads();
        for (int i = tid; i < K; i += SECTION_SELECT_THREADS) {
            if (!a.peak[i]) continue;
            const int at = atomicAdd(&n_keys, 1);
            if (at < SECTION_SELECT_KEYS) keys[at] = section_key(a.nov[i], i);
        }
        __syncthreads();
        const int n = min(n_keys, SECTION_SELECT_KEYS);
        for (int j = tid; j < n; j += SECTION_SELECT_THREADS) {
            const unsigned long long mine = keys[j];
            int larger = 0;
            for (int k = 0; k < n; ++k) larger += keys[k] > mine;           // every lane reads the same word: a broadcast
            if (larger == keep - 1) red[0] = mine;                         // the keys are distinct: one writer
        }
        __syncthreads();
        least = red[0];
        __syncthreads();
    } else if (n_peaks > keep) {                                            // more peaks than LDS holds: keep rounds of a maximum below the last
        least = ~0ull;
        for (int round = 0; round < keep; ++round) {
            unsigned long long best = 0ull;
            for (int i = tid; i < K; i += SECTION_SELECT_THREADS) {
                if (!a.peak[i]) continue;
                const unsigned long long key = section_key(a.nov[i], i);
                if (key < least && key > best) best = key;
            }
            least = section_block_max(best, red, lane, wave, WAVES);
        }
    }
    int n_sections = 1;
    for (int i0 = 0; i0 < K; i0 += SECTION_SELECT_THREADS) {
        const int i = i0 + tid;
        const bool kept = i < K && a.peak[i] && section_key(a.nov[i], i) >= least;
        const unsigned long long ballot = __ballot(kept);
        if (lane == 0) counts[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < WAVES; ++w) {
            before += w < wave ? counts[w] : 0;
            total += counts[w];
        }
        const int at = n_sections + before + __popcll(ballot & ((1ull << lane) - 1ull));
        if (kept && at < SECTION_MAX_SECTIONS) a.starts[at] = i;           // at most max_sections - 1 are kept: at <= 63
        n_sections += total;
        __syncthreads();
    }
    if (tid == 0) {
        a.starts[0] = 0;
        a.starts[n_sections] = K;
        a.starts[SECTION_COUNT_AT] = n_sections;
        a.result[0] = n_sections;
        a.result[2] = a.acc[0] ? (long long)(a.acc[0] - SECTION_BIAS) : 0;
        a.result[4] = n_peaks;
    }
}

__global__ __launch_bounds__(SECTION_THREADS) void section_pairs_kernel(SectionArgs a) {
    __shared__ unsigned long long red[SECTION_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int n_sections = a.starts[SECTION_COUNT_AT];                      // 0 with K < 2
    int s = 0, t = (int)blockIdx.x;
    while (t > s) t -= ++s;                                                 // row s holds the pairs (s, 0 .. s)
    if (s >= n_sections) return;
    const int as = a.starts[s], ls = a.starts[s + 1] - as;
    unsigned long long sum = 0ull;
    int m = ls;
    if (t == s) {                                                           // the number of beats that are not empty
        for (int k = tid; k < ls; k += SECTION_THREADS) sum += a.f[(long long)(as + k) * SECTION_F_WORDS + 12] == 0;
    } else {
        const int at = a.starts[t], lt = a.starts[t + 1] - at;
        m = min(ls, lt);
        for (int k = tid; k < m; k += SECTION_THREADS) {
            const unsigned* x = reinterpret_cast<const unsigned*>(a.f + (long long)(as + k) * SECTION_F_WORDS);
            const unsigned* y = reinterpret_cast<const unsigned*>(a.f + (long long)(at + k) * SECTION_F_WORDS);
            const unsigned p[6] = {x[0], x[1], x[2], x[3], x[4], x[5]}, q[6] = {y[0], y[1], y[2], y[3], y[4], y[5]};
            sum += section_row_distance(p, q);
        }
    }
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x, WAVE);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid != 0) return;
    sum = red[0] + red[1] + red[2] + red[3];
    if (t == s) {
        a.same[s * SECTION_MAX_SECTIONS + s] = sum == 0ull;
    } else {
        const int longer = max(ls, a.starts[t + 1] - a.starts[t]);
        a.same[s * SECTION_MAX_SECTIONS + t] = (long long)a.len_num * m >= longer && sum / (unsigned long long)m <= (unsigned long long)a.same_dist;
    }
}

__global__ __launch_bounds__(SECTION_THREADS) void section_label_kernel(SectionArgs a) {
    __shared__ int starts[SECTION_MAX_SECTIONS + 1];
    __shared__ unsigned labels[SECTION_MAX_SECTIONS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int K = beat_count(a.beat_result, a.max_beats);
    const long long first = (long long)blockIdx.x * SECTION_THREADS;
    if (K < 2 || first >= K) return;
    const int n_sections = a.starts[SECTION_COUNT_AT];                      // 1 .. max_sections
    if (tid <= n_sections) starts[tid] = a.starts[tid];
    if (tid < WAVE) {
        const bool silent = lane < n_sections && a.same[lane * SECTION_MAX_SECTIONS + lane] != 0;
        unsigned label = 0u;
        int letters = 0, n_silent = 0;
        for (int s = 0; s < n_sections; ++s) {
            const bool s_silent = a.same[s * SECTION_MAX_SECTIONS + s] != 0;
            const unsigned long long like = __ballot(lane < s && !silent && a.same[s * SECTION_MAX_SECTIONS + lane] != 0);
            const unsigned earliest = (unsigned)__shfl((int)label, like ? __ffsll((long long)like) - 1 : 0, WAVE);
            unsigned mine;
            if (s_silent) {
                mine = SECTION_SILENT;
                ++n_silent;
            } else if (like) {
                mine = earliest;
            } else {
                mine = (unsigned)letters++;
            }
            if (lane == s) label = mine;
        }
        labels[lane] = label;
        if (blockIdx.x == 0 && lane == 0) {
            a.result[1] = letters;
            a.result[5] = n_silent;
        }
    }
    __syncthreads();
    const long long at = first + tid;
    if (at >= K) return;
    const int i = (int)at;
    int lo = 0, hi = n_sections - 1;                                        // the largest s with starts[s] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    a.section[i] = (int32_t)((starts[lo] == i ? 65536u : 0u) + 256u * (unsigned)lo + labels[lo]);
}

}  // namespace

int launch_track_sections(const SectionArgs& a, hipStream_t stream) {
    if (int e = slot_check_programs(a)) return e;
    if (a.context < 1 || a.context > SECTION_MAX_CONTEXT || a.kernel_beats < 2 || a.kernel_beats > SECTION_MAX_KERNEL || a.min_len < 1 ||
        a.min_len > SECTION_MAX_MIN_LEN || a.max_sections < 1 || a.max_sections > SECTION_MAX_SECTIONS)
        return -2;
    if (a.peak_div < 1 || a.peak_div > 1024 || a.same_dist < 0 || a.same_dist > 32768 || a.len_num < 1 || a.len_num > 16) return -3;
    if (int e = slot_check_call(a)) return e;
    if (!a.f || !a.nov || !a.peak || !a.acc || !a.starts || !a.same || !a.section) return -6;
    const unsigned beat_blocks = (unsigned)((a.max_beats + SECTION_THREADS - 1) / SECTION_THREADS);
    const unsigned pairs = (unsigned)(a.max_sections * (a.max_sections + 1) / 2);
    section_clear_kernel<<<beat_blocks < (unsigned)SECTION_CLEAR_BLOCKS ? beat_blocks : (unsigned)SECTION_CLEAR_BLOCKS, SECTION_THREADS, 0, stream>>>(a);
    if (a.n) section_features_kernel<<<(unsigned)((a.n + SECTION_THREADS - 1) / SECTION_THREADS), SECTION_THREADS, 0, stream>>>(a);
    section_context_kernel<<<beat_blocks, SECTION_THREADS, 0, stream>>>(a);
    section_novelty_kernel<<<(unsigned)((a.max_beats + SECTION_TILE - 1) / SECTION_TILE), SECTION_THREADS, 0, stream>>>(a);
    section_peaks_kernel<<<beat_blocks, SECTION_THREADS, 0, stream>>>(a);
    section_select_kernel<<<1, SECTION_SELECT_THREADS, 0, stream>>>(a);
    section_pairs_kernel<<<pairs, SECTION_THREADS, 0, stream>>>(a);
    section_label_kernel<<<beat_blocks, SECTION_THREADS, 0, stream>>>(a);
    return 0;
}
