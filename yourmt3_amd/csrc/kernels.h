// Launcher declarations shared between the kernel translation units and the host code (runtime.hip, note_objects.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

// ---------------------------------------------------------------- front-end (frontend.hip)
struct FrontendTables {
    const float* window;      // [n_fft] periodic Hann
    const float2* tw;         // [n_fft/2]   exp(-2 pi i m / (n_fft/2))
    const float2* untw;       // [n_fft/2+1] exp(-2 pi i k / n_fft)
    const int* mel_start;     // [n_mels] first bin of each triangle
    const int* mel_len;       // [n_mels] bins in each triangle
    const int* mel_off;       // [n_mels] offset into mel_w
    const float* mel_w;       // concatenated triangle weights
    int n_fft, hop, n_mels, n_samples, n_frames, n_mel_w;
    float log_floor;
};
int launch_logmel(const FrontendTables& t, const float* audio, float* mel, int B, hipStream_t stream);

// ---------------------------------------------------------------- audio ingest (ingest.hip)
struct IngestArgs {
    const void* pcm;          // [n_in][n_channels] interleaved int16 or fp32
    const float* taps;        // [up][Jp] polyphase rows of the low-pass, zero padded beyond J
    float* out;               // [n_total] = (n_seg, segment_samples), zero beyond n_out
    long long n_in, n_out, n_total, r;   // r: output alignment offset (n_pre_remove of resample_poly)
    int up, down, J, Jp, n_channels, s16, window;   // window: LDS floats per workgroup
};
int launch_ingest(const IngestArgs& a, hipStream_t stream);
// streaming form: one push (or the finish) of a ymt3_ingest_stream.  Output sample n of the whole stream is addressed by its number.
struct IngestStreamArgs {
    const void* pcm;          // [n_new][n_channels] the frames of this push
    float* hist;              // [hist_mask + 1] mono ring: frame k at k & hist_mask
    const float* taps;        // as IngestArgs
    float* out;               // the caller's rows: sample n at out[n - n_row0] for n < n_row_end
    const float* part_old;    // partial segment kept by earlier pushes: sample n at part_old[n - n_row0] for n < n_done
    float* part_new;          // partial segment this call leaves: sample n at part_new[n - n_row_end] for n >= n_row_end
    long long hist_mask, n_new, n_in;      // n_in: frames arrived, these n_new included
    long long g0, n_done, n_end, n_total;  // the launch covers [g0, n_total): copy below n_done, compute below n_end, then zero
    long long n_row0, n_row_end, r;
    int up, down, J, Jp, n_channels, s16, window;
};
int launch_ingest_stream(const IngestStreamArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- device detokeniser (detok.hip; include/ymt3.h, device detokeniser)
constexpr int DETOK_PITCHES = 128;        // pitch / drum values per program: a merge key is program * 128 + pitch
constexpr int DETOK_MAX_PROGRAMS = 256;   // 256 * 128 32-bit counters = 128 KB of the 160 KB of LDS
constexpr int DETOK_MAX_STEPS = 32768;    // an item's column has 15 bits, its step 27 (32768 * 4095 < 2^27), its segment 20
constexpr int DETOK_MAX_SEGMENTS = 1 << 20;
constexpr int NOTE_PITCHES = 128;         // the pitch range of a counted record (note_rule.h)
struct DetokNote {                        // the 32-byte record of include/ymt3.h
    double onset, offset;
    int32_t program, pitch, is_drum;
    float score;
};
struct DetokArgs {
    const uint16_t* table;                // [vocab] class << 12 | value
    int vocab, steps_per_second, drum_program, n_programs;
    const int32_t* tokens;                // element (s, ch, col) at s * seg_stride + ch * chan_stride + col
    const float* scores;                  // the same layout, or null
    long long seg_stride, chan_stride;
    int n_seg, n_chan, L;
    const double* start;                  // [n_seg] strictly increasing
    double end_sec;
    unsigned long long* items;            // [n_chan][n_seg][L] row (ch, s) owns L slots: segment:20 | not-tie:1 | step:27 | velocity:1 | column:15
    uint16_t* keys;                       // the same slots: program * 128 + pitch
    int* row_count;                       // [n_chan][n_seg] items of the row
    unsigned long long* sorted;           // [n_chan][n_seg * L] a channel's items bucketed by key
    unsigned* key_off;                    // [n_chan][n_programs * 128] first slot of every key's bucket
    DetokNote* notes;
    long long capacity;
    int32_t* counts;                      // [2] n_notes, n_invalid (zero at launch)
};
int init_detok_kernels();
int launch_detok(const DetokArgs& a, hipStream_t stream);
// incremental form (ymt3_detokenize_push / ymt3_detokenize_finish): the state a ymt3_detok_state carries between calls
struct DetokSounding { double onset; float score; int32_t valid; };     // per (channel, key): the note still sounding after the last pushed segment
struct DetokHeld { double time; float score; int32_t pad; };            // a drum hit not yet below the horizon
struct DetokCarryArgs {
    DetokSounding* sounding;              // [n_chan][n_programs * 128]
    const DetokHeld* held_in;             // [n_chan][128][max_held] ascending times, the first held_count_in valid
    DetokHeld* held_out;                  // the other copy: what this call leaves
    const int* held_count_in;             // [n_chan][128]
    int* held_count_out;
    int max_held, finish;                 // finish: close every sounding note at end_sec
    double horizon;                       // hits with time < horizon leave the state
};
// DetokArgs as for launch_detok (n_seg may be 0: nothing is decoded, the state alone is walked); counts is [3], n_forced last
int launch_detok_carry(const DetokArgs& a, const DetokCarryArgs& c, hipStream_t stream);

// ---------------------------------------------------------------- device tokeniser (tok.hip; include/ymt3.h, device tokeniser)
constexpr int TOK_PITCHES = 128;          // pitch values per program: a tie key is program * 128 + pitch
constexpr int TOK_MAX_PROGRAMS = 256;     // an item word gives the program 8 bits
constexpr int TOK_MAX_STEPS = 4096;       // a row's items are sorted in LDS: 4096 * 8 B = 32 KB
constexpr int TOK_MAX_SEGMENTS = 1 << 20;
constexpr long long TOK_MAX_NOTES = 1LL << 29;   // a row's 32-bit counter takes at most two appends per note plus the ties
struct TokArgs {
    int shift_base, pitch_base, velocity_base, tie_base, program_base, drum_base;     // ymt3_tok_params
    int max_shift_steps, steps_per_second, drum_program, eos_id, pad_id;
    int n_programs;
    const uint8_t* program_channel;       // [n_programs], every entry < n_chan
    const DetokNote* notes;               // [n_notes] the detokeniser's record; `score` is not read
    long long n_notes;
    const double* start;                  // [n_seg] strictly increasing
    double end_sec;
    int n_seg, n_chan, L;
    unsigned long long* items;            // [n_seg][n_chan][L] the rows' item words, in append order
    int* row_count;                       // [n_seg][n_chan] items appended to the row (may exceed L); zeroed by launch_tok
    unsigned* tie_seen;                   // [n_seg][n_programs * 4] one bit per (program, pitch) tied into the segment; zeroed by launch_tok
    int32_t* tokens;                      // [n_seg][n_chan][L]
    int32_t* lengths;                     // [n_seg][n_chan] tokens the row needs, EOS included (> L: overflow)
};
int launch_tok(const TokArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- device note metrics (metrics.hip; include/ymt3.h, note metrics)
constexpr int METRICS_PITCHES = NOTE_PITCHES;      // a key is row * 128 + pitch; row n_programs holds the instrument-agnostic keys
constexpr int METRICS_MAX_PROGRAMS = 256;
constexpr long long METRICS_MAX_NOTES = 1LL << 24; // per side; a counted note fills at most two bucket slots
struct MetricsArgs {
    double onset_tol, offset_min_tol, offset_ratio;
    int n_programs, drum_program;
    const DetokNote* ref;                 // [n_ref] the detokeniser's record; `score` is not read
    const DetokNote* est;                 // [n_est]
    long long n_ref, n_est;               // the launches' sizes
    const int32_t* ref_count;             // device counts (or null): the side has min(n, max(*count, 0)) records
    const int32_t* est_count;
    long long max_ref, max_est;           // what the scratch below was sized for
    unsigned* hist;                       // [2][n_keys] records per key and side; zeroed by launch_metrics
    unsigned* off;                        // [2][n_keys + 1] first bucket slot of every key, then the total
    unsigned* cursor;                     // [2][n_keys] next free slot of every bucket
    double2* t_ref;                       // [2 * max_ref] (onset, offset) bucketed by key
    double2* t_est;                       // [2 * max_est]
    int2* win;                            // [2 * max_ref] per reference slot: the interval of estimates it can hit by onset
    int2* stack;                          // [2 * max_ref] the search's frames: (reference, next candidate)
    int* match;                           // [2 * max_est] per estimate slot: the reference it is matched to, or -1
    int* visit;                           // [2 * max_est] the root of the last search that visited it
    int32_t* counts;                      // [(n_programs + 1) * 6 + 2]; zeroed by launch_metrics
};
int launch_metrics(const MetricsArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- device piano roll and frame metrics (roll.hip; include/ymt3.h, piano roll)
constexpr int ROLL_PITCHES = NOTE_PITCHES;         // one 16-byte word of pitch bits per (side, row, frame)
constexpr int ROLL_MAX_PROGRAMS = 256;
constexpr long long ROLL_MAX_FRAMES = 1LL << 24;
constexpr long long ROLL_MAX_NOTES = 1LL << 29;    // per side
struct RollArgs {
    double frames_per_second;
    int n_programs, drum_program;
    int n_sides;                          // 2: reference and estimate (frame metrics); 1: the notes of a roll
    const DetokNote* notes[2];            // [n[side]] the detokeniser's record; `score` is not read
    long long n[2];                       // the launches' sizes
    const int32_t* count[2];              // device counts (or null): the side has min(n, max(*count, 0)) records
    long long n_frames, max_frames;       // frames of this call; what the scratch below was sized for
    int row0, row_n;                      // the rows the call works on: all n_programs + 1 (metrics), or the roll's row range
    uint4* bits;                          // [n_sides][row_n][n_frames] 128 pitch bits each, inside 2 * (n_programs + 1) * max_frames words; zeroed by the launch
    long long* counts;                    // metrics: [(n_programs + 1) * 6 + 2], zeroed by the launch; null for a roll
    uint8_t* roll;                        // roll: [row_n][n_frames][128] bytes of 0 / 1, every byte written; null for the metrics
};
int launch_frame_metrics(const RollArgs& a, hipStream_t stream);
int launch_piano_roll(const RollArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- device alignment: banded DTW over pitch sets (align.hip; include/ymt3.h, alignment)
constexpr int ALIGN_INF = 1 << 30;
constexpr long long ALIGN_MAX_FRAMES = 1LL << 20;
constexpr int ALIGN_TILE_ROWS = 256, ALIGN_TILE_COLS = 64;               // a tile of the dynamic programme: one wave, one lane per column
// scratch sizing, shared by ymt3_aligner_create and the launches (band = min(band_frames, max_frames): a wider band changes no cell)
inline long long align_step_words(long long band) { return band / 8 + 2; }                       // dwords per column: 2 bits x (2 * band + 1) rows, 16-row groups
inline long long align_padded(long long frames, int tile) { return (frames + tile - 1) / tile * tile; }
inline long long align_corners(long long max_frames) { return align_padded(max_frames, ALIGN_TILE_ROWS) / ALIGN_TILE_ROWS + align_padded(max_frames, ALIGN_TILE_COLS) / ALIGN_TILE_COLS; }
inline long long align_edge_ints(long long max_frames) {                                          // bottom, right, corners, total
    return align_padded(max_frames, ALIGN_TILE_COLS) + align_padded(max_frames, ALIGN_TILE_ROWS) + align_corners(max_frames) + 1;
}
struct AlignArgs {
    double frames_per_second;
    int n_programs, drum_program;
    long long band_frames;                // min(the object's band_frames, max_frames)
    const DetokNote* notes[2];            // reference, estimate: [n[side]]
    long long n[2];
    const int32_t* count[2];              // device counts (or null): the side has min(n, max(*count, 0)) records
    long long n_frames[2], max_frames;    // each in [1, max_frames]
    uint4* feat;                          // [2][max_frames][2] 128 pitch bits each: the agnostic word, then the drum word
    int* edges;                           // [align_edge_ints(max_frames)]
    unsigned* steps;                      // [max_frames][align_step_words(band_frames)]
    int2* rpath;                          // [2 * max_frames - 1] the path, last cell first
    int32_t* warp;                        // [n_frames[0]]
    int32_t* path;                        // [(n_frames[0] + n_frames[1] - 1) * 2] or null
    long long* result;                    // [4]: total, path_len, skipped ref, skipped est
};
int launch_align(const AlignArgs& a, hipStream_t stream);
struct WarpNotesArgs {
    double frames_per_second;
    const DetokNote* notes;               // [n]
    DetokNote* out;                       // [n]; may be `notes`
    long long n;
    const int32_t* count;                 // device count (or null)
    const int32_t* warp;                  // [n_ref_frames]
    long long n_ref_frames;
};
int launch_warp_notes(const WarpNotesArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- note velocities from the audio (velocity.hip; include/ymt3.h, note velocities)
constexpr int VELOCITY_MIN_WINDOW = 64, VELOCITY_MAX_WINDOW = 4096;
constexpr int VELOCITY_MAX_HARMONICS = 8;
constexpr long long VELOCITY_MAX_NOTES = 1LL << 29;
struct VelocityArgs {
    const float* audio;                   // [n_audio] mono at the object's sample rate; samples outside read as 0
    long long n_audio;
    const DetokNote* notes;               // [n] the detokeniser's record; offset and score are not read
    long long n;
    const int32_t* count;                 // device count (or null): min(n, max(*count, 0)) records are live
    const float* window;                  // [W]
    const uint32_t* steps;                // [128][VELOCITY_MAX_HARMONICS] phase steps, 0 = absent
    int W, H, drum_program;
    double sample_rate;
    float e_scale, p_scale;               // 4 / (sum w)^2 and 2 / sum w^2
    double velocity_per_db, ref_energy;   // ref_energy: 10^(peak_db / 10), or NaN for the class's peak
    int peak_velocity, min_velocity, default_velocity;
    uint8_t* velocity;                    // [n] every byte written; 0 at or beyond the count
    float* energy;                        // [n] or null: E, NaN where unmeasured or beyond the count
    float* peaks;                         // [2] pitched, drums; zeroed by the caller before the launch
    int32_t* counts;                      // [2] measured, unmeasured; zeroed by the caller before the launch
};
int launch_note_velocities(const VelocityArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- beat tracking over note records (beats.hip; include/ymt3.h, beat tracking)
constexpr long long BEAT_MAX_FRAMES = 1LL << 20;
constexpr long long BEAT_MAX_NOTES = 1LL << 29;
constexpr int BEAT_MIN_LAG = 4, BEAT_MAX_LAG = 512, BEAT_MAX_WINDOW = 2048, BEAT_MAX_PROGRAMS = 256;
constexpr int BEAT_TICKS_PER_BEAT = 480;
constexpr int BEAT_RING = 2048;                                        // the power of two >= 2 * BEAT_MAX_LAG + BEAT_MAX_LAG / 2
__host__ __device__ inline long long beat_windows(long long n_frames, int hop) { const long long w = (n_frames + hop - 1) / hop; return w > 1 ? w : 1; }
__host__ __device__ inline long long beat_max_beats(long long n_frames, int lag_min) { return n_frames / ((lag_min + 1) / 2) + 1; }
struct BeatArgs {
    double frames_per_second;
    int n_programs, drum_program;
    int lag_min, lag_max, window, hop, lag_step, onset_cap;
    const DetokNote* notes;               // [n] the detokeniser's record; offset is read only by the counting rule
    long long n;
    const int32_t* count;                 // device count (or null): min(n, max(*count, 0)) records are live
    long long n_frames;                   // in [1, the object's max_frames]
    const int32_t* prior;                 // [nL], nL = lag_max - lag_min + 1
    const int32_t* pen;                   // [nL][2 * lag_max + 1]: row t - lag_min, column d
    unsigned* env;                        // [max_frames] onsets per frame
    unsigned short* smooth;               // [max_frames] s
    long long* tgram;                     // [nW][nL] T
    unsigned short* lag_back;             // [nW][nL] the tempo path's back-pointers, as lag indices
    int32_t* lags;                        // [nW] the tempo path, read by the beat kernel
    int32_t* back;                        // [max_frames]
    int32_t* rbeats;                      // [beat_max_beats(max_frames)] the chain, last beat first
    int32_t* beats;                       // [max_beats]: the first n_beats are written
    long long max_beats;
    int32_t* tempo;                       // [nW] or null
    long long* result;                    // [4]: n_beats, max C, max V, skipped
};
int launch_track_beats(const BeatArgs& a, hipStream_t stream);
struct BeatPositionArgs {
    double frames_per_second;
    int n_programs, drum_program, divisions;
    const int32_t* beats;                 // [result[0]] ascending
    const long long* result;              // track_beats' result: [0] is read
    long long max_beats;                  // what [0] is clamped to: beat_max_beats(the object's max_frames)
    const DetokNote* notes;               // [n]
    long long n;
    const int32_t* count;                 // device count (or null)
    int32_t* ticks;                       // [n][2] every entry written; -1 at or beyond the count
};
int launch_beat_positions(const BeatPositionArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- bars and key over note records and beats (bars.hip; include/ymt3.h, bars and key)
constexpr long long BAR_MAX_FRAMES = 1LL << 20;
constexpr long long BAR_MAX_BEATS = (1LL << 20) + 1, BAR_MAX_NOTES = 1LL << 20;
constexpr int BAR_MAX_METRES = 5, BAR_MIN_METRE = 2, BAR_MAX_METRE = 6, BAR_MAX_PROGRAMS = 256;
constexpr int BAR_ACC_WORDS = 16;                                       // tot[12], the sum of d, three spare
struct BarArgs {
    double frames_per_second;
    int n_programs, drum_program;
    int n_metres, metres[BAR_MAX_METRES];
    int near_div, accent_cap, w_long, w_kick, kick_lo, kick_hi, w_accent, switch_cost;
    const int32_t* beats;                 // [K] frames, strictly ascending
    const long long* beat_result;         // track_beats' result: [0] is K, clamped to [0, max_beats]
    long long max_beats;                  // the object's: what the scratch below holds
    const DetokNote* notes;               // [n]
    long long n;
    const int32_t* count;                 // device count (or null): min(n, max(*count, 0)) records are live
    long long n_frames;
    unsigned* accent;                     // [max_beats] a
    unsigned* chroma;                     // [max_beats][12] c
    int32_t* salience;                    // [max_beats] d
    unsigned short* choice;               // [max_beats] the downbeat states' back-pointers, 3 bits per metre
    unsigned long long* acc;              // [BAR_ACC_WORDS]
    int32_t* metre;                       // [>= max_beats]: the first K are written
    long long* result;                    // [8]: n_downbeats, max V, mean_d, key, best S, second S, skipped, 0
};
int launch_track_bars(const BarArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- chords over note records and beats (chords.hip; include/ymt3.h, chords)
constexpr int CHORD_QUALITIES = 8;                                      // the fixed table: maj, min, dim, aug, sus4, 7, maj7, min7
constexpr int CHORD_MAX_STATES = 12 * CHORD_QUALITIES + 1;              // (q, r), then N
constexpr int CHORD_BACK_WORDS = 4;                                     // per beat: a stay bit per state, then j* (7 bits)
struct ChordArgs {
    double frames_per_second;
    int n_programs, drum_program;
    int n_qualities, qualities[CHORD_QUALITIES];                         // indices into the fixed table, in state order
    int near_div, bass_div, w_bass, w_none, change_cost, change_cost_down;
    const int32_t* beats;                 // [K] frames, strictly ascending
    const long long* beat_result;         // track_beats' result: [0] is K, clamped to [0, max_beats]
    long long max_beats;                  // the object's: what the scratch below holds
    const int32_t* metre;                 // [K] 256 m + k of every beat, or null
    const DetokNote* notes;               // [n]
    long long n;
    const int32_t* count;                 // device count (or null): min(n, max(*count, 0)) records are live
    long long n_frames;
    unsigned* chroma;                     // [max_beats][12] c
    unsigned* bass;                       // [max_beats] the lowest long pitch, 255 with none
    unsigned* back;                       // [max_beats][CHORD_BACK_WORDS] the back-pointers
    int32_t* chord;                       // [>= max_beats]: the first K are written
    long long* result;                    // [8]: runs, max V, N beats, skipped, 0, 0, 0, 0
};
int launch_track_chords(const ChordArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- sections over note records and beats (sections.hip; include/ymt3.h, sections)
constexpr int SECTION_MAX_SECTIONS = 64, SECTION_MAX_KERNEL = 64, SECTION_MAX_CONTEXT = 16, SECTION_MAX_MIN_LEN = 256;
constexpr int SECTION_F_WORDS = 16;                                     // per beat: f[12] as 16-bit words, [12] the empty flag, three spare
constexpr int SECTION_ACC_WORDS = 4;                                    // the biased top, the number of peaks, two spare
struct SectionArgs {
    double frames_per_second;
    int n_programs, drum_program;
    int near_div, context, kernel_beats, min_len, peak_div, same_dist, len_num, max_sections;
    const int32_t* beats;                 // [K] frames, strictly ascending
    const long long* beat_result;         // track_beats' result: [0] is K, clamped to [0, max_beats]
    long long max_beats;                  // the object's: what the scratch below holds
    const int32_t* metre;                 // [K] 256 m + k of every beat, or null
    const DetokNote* notes;               // [n]
    long long n;
    const int32_t* count;                 // device count (or null): min(n, max(*count, 0)) records are live
    long long n_frames;
    unsigned* chroma;                     // [max_beats][12] c
    unsigned short* f;                    // [max_beats][SECTION_F_WORDS]
    long long* nov;                       // [max_beats]
    unsigned char* peak;                  // [max_beats] 1: a peak
    unsigned long long* acc;              // [SECTION_ACC_WORDS]
    int32_t* starts;                      // [SECTION_MAX_SECTIONS + 2]: a_0 .. a_n, then the number of sections at [SECTION_MAX_SECTIONS + 1]
    unsigned char* same;                  // [SECTION_MAX_SECTIONS][SECTION_MAX_SECTIONS]: [s][t], t < s: the same; [s][s]: s is silent
    int32_t* section;                     // [>= max_beats]: the first K are written
    long long* novelty;                   // [>= max_beats] or null: the first K are written
    long long* result;                    // [8]: sections, letters, top, skipped, peaks, silent sections, 0, 0
};
int launch_track_sections(const SectionArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- hands over note records (hands.hip; include/ymt3.h, hands)
constexpr int HAND_STATES = 129;                                        // the split points 0 .. 128
constexpr int HAND_BACK_ROW = 132;                                      // bytes per slice of back-pointers: one per state, padded to words
constexpr int HAND_ACC_WORDS = 4;                                       // T, s_{T-1}, two spare
constexpr int HAND_MAX_SLICE_FRAMES = 64, HAND_MAX_WEIGHT = 1024;
constexpr long long HAND_MAX_REST = 1LL << 20;
__host__ __device__ inline long long hand_slots(long long n_frames, int slice_frames) { return (n_frames + slice_frames - 1) / slice_frames; }
struct HandArgs {
    double frames_per_second;
    int n_programs, drum_program;
    int slice_frames, program_lo, program_hi, span, w_span, cut_min, w_cut, w_centre, middle, mid_free, w_mid, w_move, w_switch, rest_slots;
    const DetokNote* notes;               // [n]
    long long n;
    const int32_t* count;                 // device count (or null): min(n, max(*count, 0)) records are live
    long long n_frames;
    long long n_slots;                    // hand_slots(n_frames, slice_frames): at most the object's slots
    long long max_slices;                 // the object's: min(max_notes, hand_slots(max_frames)) slices fit the scratch below
    uint4* sets;                          // [the object's slots] 128 pitch bits per slot
    int32_t* slice_of;                    // [the object's slots] slot -> t, written for the occupied slots
    uint4* cset;                          // [max_slices] P_t
    int32_t* slot_of;                     // [max_slices] Q_t
    unsigned char* back;                  // [max_slices][HAND_BACK_ROW] back_t(s)
    unsigned char* cut;                   // [max_slices] s_t
    unsigned long long* acc;              // [HAND_ACC_WORDS]
    uint8_t* hand;                        // [n]: the live ones are written
    int32_t* split;                       // [>= min(n, n_slots)] or null: the first T are written
    long long* result;                    // [8]: slices, selected, left, right, total, skipped, hand-overs, 0
};
int launch_split_hands(const HandArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- dense GEMM (gemm.hip)
// C[M][N] (+)= A[M][K] (bf16, row stride lda) * W[N][K]^T (bf16, row stride ldw), fp32 accumulate.
enum GemmEpilogue {
    EPI_F32 = 0,          // out f32 [M][ldc] = acc (+ bias[n])
    EPI_BF16 = 1,         // out bf16 [M][ldc] = R(acc)
    EPI_BF16_RELU = 2,    // out bf16 [M][ldc] = R(max(acc, 0))
    EPI_RESID = 3,        // out f32 [M][ldc] += acc
    EPI_KV_HEADMAJOR = 4, // out bf16 [n / (H*64)][m / T][h][m % T][64]  (cross-attention K/V slabs)
};
struct GemmArgs {
    const bf16_t* A; const bf16_t* W; void* out; const float* bias;
    int M, N, K, lda, ldw, ldc;
    int T, H, n_seg;      // EPI_KV_HEADMAJOR only: frames per segment, heads, segments
};
int launch_gemm(int epilogue, const GemmArgs& a, hipStream_t stream);
int init_gemm_kernels();

// ---------------------------------------------------------------- norm / casts (norm.hip)
// out bf16 [M][d] = R(x * rsqrt(mean(x^2) + eps) * gain)
int launch_rmsnorm(const float* x, const float* gain, bf16_t* out, int M, int d, float eps, hipStream_t stream);
int launch_f32_to_bf16(const float* x, bf16_t* out, size_t n, hipStream_t stream);
// out f32 [B][n] = src bf16 [n] repeated for every b (the latent array as the initial residual stream)
int launch_broadcast_bf16(const bf16_t* src, float* out, int B, size_t n, hipStream_t stream);

// ---------------------------------------------------------------- encoder attention (enc_attn.hip)
// qkv bf16 [B*T][3*H*64] -> out bf16 [B*T][H*64]; bias_off f32 [H][2T-1] indexed by key - query + T-1
int init_enc_attn_kernels();
// general form: queries and keys/values from separate buffers (latent cross-attention, a9)
int launch_enc_attention_qkv(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, const float* bias_off,
                             bf16_t* out, int B, int T, int H, hipStream_t stream);
int launch_enc_attention(const bf16_t* qkv, const float* bias_off, bf16_t* out, int B, int T, int H, hipStream_t stream);

// Batched small-sequence attention for the Perceiver-TF encoder (a9): n_seq independent sequences, heads of 64, Tq queries
// over Tk keys per sequence.  Sequence s starts at element (s / inner_n) * outer + (s % inner_n) * inner of each buffer and
// its consecutive positions are `step` elements apart -- so the same kernel serves sequences that are contiguous runs of rows
// (spectral cross-attention and latent self-attention: one sequence per (segment, frame)) and sequences strided through
// them (temporal self-attention: one sequence per (segment, latent), positions = frames).
struct SeqAttnArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* out;
    const float* bias_off;        // [H][2*Tk-1] by key - query + Tk - 1 (needs Tq == Tk), or null: no bias
    int n_seq, H, Tq, Tk, inner_n;
    long long q_outer, q_inner, q_step, kv_outer, kv_inner, kv_step, o_outer, o_inner, o_step;
};
int launch_seq_attention(const SeqAttnArgs& a, hipStream_t stream);
// spectral tokens of the Perceiver-TF encoder: out bf16 [n_rows][d] = R(rmsnorm(mel[row] * w + pos[row % F]) * gain)
int launch_spec_embed(const float* mel, const float* w, const bf16_t* pos, const float* gain, bf16_t* out, long long n_rows, int F, int d,
                      float eps, hipStream_t stream);

// ---------------------------------------------------------------- decoder step (decode.hip)
struct DecodeShared {           // device-resident loop state, read by every decode kernel
    int step;                   // position being decoded (tokens already in the cache)
    int done_count;             // ticket counter of the argmax kernel
    int n_steps;                // row stride of tokens_out / forced / logits_out / scores_out
    int step0;                  // first position of this call (0 except under the debug hook ymt3_debug_decode_start)
    int n_unfinished;           // rows of this chain that have not emitted EOS yet (maintained when eos_id >= 0)
    int n_prompt;               // P: the first P steps of the call feed prompt ids and emit nothing (0: none)
    int32_t* tokens_out;        // [R][n_steps]
    const int32_t* forced;      // [R][n_steps] or null
    float* logits_out;          // [R][n_steps][V] or null
    const int32_t* prompt;      // [R][n_prompt] (lock-step) or indexed through row_prompt (slot mode); null when n_prompt = 0
    float* scores_out;          // [R][n_steps] log_softmax(logits)[fed id] per emitted token (indexed as tokens_out), or null
    // token automaton (include/ymt3.h, constraints), or null: every emitted token is the first maximum over the tokens
    // allowed[row_state[r]], and the fed id f moves the row to next[row_state[r]][f]
    const uint32_t* c_allowed;  // [n_states][c_words] one bit per token
    const int32_t* c_next;      // [n_states][V]
    int c_words;                // ceil(V / 32)
};

// the automaton of a call as the kernels see it (all null / 0: none)
struct ConstraintView {
    const uint32_t* allowed;    // [n_states][words]
    const int32_t* next;        // [n_states][V]
    int words, n_states;
    const int32_t* start;       // per-row start states (lock-step: [R]; slot mode: the admitted segment's [n_channels]) or null: state 0
};

constexpr int SSQ_TILES = 32;    // sum(h^2) partials per row = d_model / 16 column tiles of the RESID epilogue

struct DecGemmArgs {
    const float* x_f32;         // NORM variants: residual stream [R][K] fp32
    const float* gain;          // NORM variants: [K]
    const bf16_t* a_bf16;       // plain variants: [R][K] bf16
    const bf16_t* W;            // [N][K] bf16
    int row0, R, N, K;          // rows [row0, row0 + R) of every row-indexed buffer
    float eps;
    // outputs (by mode)
    bf16_t* out_bf16;           // [R][N] (MODE_BF16, MODE_BF16_RELU, q part of MODE_QKV_CACHE)
    float* out_f32;             // [R][N] (MODE_RESID: +=, MODE_LOGITS: =)
    bf16_t* kcache;             // MODE_QKV_CACHE: [R][H][L][64]
    bf16_t* vcache;
    int H, L;                   // cache geometry
    const DecodeShared* shared; // MODE_QKV_CACHE reads shared->step
    const int* row_pos;         // slot mode (ymt3_transcribe_stream): per-row positions replace shared->step; else null
    unsigned long long* stamp;  // measurement (YMT3_STAMP=1): [grid][2] wall-clock entry / exit per workgroup; else null
    float* ssq;                 // [SSQ_TILES][ssq_stride] per-row partial sums of h^2 (read by NORM, written by RESID)
    int ssq_stride;
    // MODE_RESID only, or null: per-head O-projection partials [R][H][N] left by the self-attention kernel; the residual
    // operand becomes h + (p0 + p1 + ... + p7) -- the sum the separate O-projection launch would have stored in h
    const float* part;
    // NORM modes after an MoE FFN whose combine launch was folded away, or null: y [2R][K] gate-scaled expert outputs by pair;
    // the residual row is x_f32 + (y[2r] + y[2r+1]) and the workgroups of column tile 0 store it to h_out (QKV mode)
    const float* pend_y;
    float* h_out;
    int mid_rows;               // row count from which the mid-size tile kernel is taken; < 0: DEC_GEMM_MID_ROWS; 0: never (handle-level: YMT3_DEC_GEMM_MID_ROWS at create)
    // MODE_QKV_CACHE, 16-row-tile kernel only, or null: all N packed columns of row m go to table[m * N + n] instead of out_bf16 and the caches
    // (ymt3_create builds the layer-0 QKV table with it, rows = token ids: see ArgmaxArgs::qkv0)
    bf16_t* table;
};
constexpr int DEC_GEMM_MID_ROWS = 512;
// The four skinny GEMMs between a layer's cross-attention and the next layer's self-attention as one launch (dec_chain.hip):
// cross O-projection -> FFN-in -> FFN-out -> next QKV projection (or lm_head); dense FFN, d_model = 512, d_ff = 2048, R <= 64.
struct ChainArgs {
    const bf16_t *w0, *w1, *w2, *w3;   // wo_c [512][512], wi [d_ff][512], wo2 [512][d_ff], next wqkv [3*512][512] or lm_head [V][512]
    const bf16_t* attn;         // [R][512] cross-attention output
    const float* part;          // folded self-attention O-projection partials [R][8][512], or null (DecGemmArgs::part)
    float* h;                   // [R][512] residual stream (read, += twice)
    float* ssq; int ssq_stride; // sum(h^2) partials, as DecGemmArgs
    const float *gain1, *gain3; // ln3 of this layer; ln1 of the next layer or ln_f
    bf16_t* dff;                // [R][d_ff] FFN hidden (scratch)
    int d_ff;
    int mode3, N3;              // DG_NORM_QKV_CACHE (N3 = 3*512) or DG_NORM_LOGITS (N3 = vocab)
    bf16_t* out_q; bf16_t* kcache; bf16_t* vcache;   // stage 3, QKV mode (next layer's cache slabs)
    float* logits;              // stage 3, lm_head mode
    int H, L;
    const DecodeShared* shared; const int* row_pos;
    int row0, R;
    float eps;
    unsigned* sync;             // CHAIN_SYNC_WORDS: arrival counters [3 boundaries][CHAIN_TILES_MAX row tiles][8 replicas], one 128-byte line each (zeroed by the
                                // preceding cross-attention launch), then the sticky abort word on a line of its own
    unsigned* host_abort;       // pinned host word, set with the abort (the host refuses further calls)
    unsigned long long* stamp;
    unsigned* sync_abort;       // dec_step.hip only: the sticky abort word (the chain launch finds it at sync + CHAIN_ABORT_WORD)
    int nsub;                   // measurement only: counters per boundary (1 / 2 / 4) in bits 0-3, 4-7, 8-11; 0 = the built-in choice
};
constexpr int CHAIN_LINE = 32;                                  // 32-bit words per 128-byte line
constexpr int CHAIN_TILES_MAX = 16;                             // row tiles of 16 rows a chain launch can hold (256 rows)
constexpr int CHAIN_COUNTERS = 3 * CHAIN_TILES_MAX * 8;
constexpr int CHAIN_ABORT_WORD = CHAIN_COUNTERS * CHAIN_LINE;
constexpr int CHAIN_SYNC_WORDS = (CHAIN_COUNTERS + 1) * CHAIN_LINE;
int init_chain_kernels();
bool dec_chain_fits(int n_cus);                 // occupancy x CUs covers the chain's grid (all its workgroups wait for each other)
bool dec_attention_pair_fits(int n_cus);        // the same for the attention pair at 64 rows
int launch_dec_chain(const ChainArgs& c, hipStream_t stream);       // 0 launched, < 0: not this kernel's shape
// tokens = INT32_MIN (and scores, if not null, = NaN) if the chain aborted
int launch_chain_poison(const unsigned* sync, int32_t* tokens, float* scores, long long n, hipStream_t stream);

// One decode step's layers as ONE launch (dec_step.hip): per layer the attention pair and the GEMM chain, handed over inside the kernel.
struct StepLayer {
    const bf16_t *wo, *wq_c, *wo_c, *wi, *wo2, *w3;    // w3: the next layer's wqkv, or lm_head after the last layer
    const float *ln2, *ln3, *gain3;                      // gain3: the next layer's ln1, or ln_f
    const bf16_t *kself, *vself;                         // this layer's self-attention cache [R][H][L][64]
    const bf16_t *kcross, *vcross;                       // its cross-attention K/V [B][H][T][64]
    bf16_t *knext, *vnext;                               // the next layer's cache (the QKV stage appends to it)
    int N3, last;                                        // 3 * 512, or the vocabulary after the last layer
};
struct StepArgs {
    // (dec_step_kernel reads this struct straight from its kernel-argument segment, per layer: common fields first, layers last)
    int n_layers, R, T, L, ssq_stride;
    float eps;
    int tiles_free, pad_;                                // 1: a row tile waits only for itself (four independent pipelines); 0: the tiles move in step
    bf16_t* q; bf16_t* attn; float* opart; float* h; float* ssq; bf16_t* dff; float* logits;
    const float* bias;                                   // [H][L] self-attention bias by distance
    const DecodeShared* shared; const int* row_pos;
    unsigned* sync;                                      // [(n_layers + 1)][STEP_SYNC_LINES_PER_LAYER] counter lines, zero at entry (the argmax kernel zeroes them)
    unsigned* pair_rows;                                 // [R][2] self-resetting row counters (as the attention pair's)
    unsigned* abort_word; unsigned* host_abort;
    unsigned long long* stamp;                           // measurement (YMT3_STAMP=1) or null: [grid][2] entry / exit clocks, then 16 marks per workgroup from word 1024
    StepLayer layer[8];
};
// per layer: the chain's counter lines, then attn_done [4 row tiles][8 replicas], then qkv_done [4 row tiles][8 heads]
constexpr int STEP_SYNC_LINES_PER_LAYER = CHAIN_COUNTERS + 32 + 32;
constexpr int STEP_SYNC_LINES = 9 * STEP_SYNC_LINES_PER_LAYER;
int init_step_kernel();
bool dec_step_fits(int n_cus);
int launch_dec_step(const StepArgs& s, hipStream_t stream);

enum DecGemmMode { DG_NORM_QKV_CACHE = 0, DG_NORM_BF16 = 1, DG_NORM_BF16_RELU = 2, DG_NORM_LOGITS = 3, DG_RESID = 4 };
int init_decode_kernels();
int launch_dec_gemm(int mode, const DecGemmArgs& a, hipStream_t stream);

struct DecAttnArgs {
    const bf16_t* q;            // [R][H*64]
    const bf16_t* k;            // slab base; slab (kv_row, h) at ((kv_row*H + h) * slab_keys) * 64
    const bf16_t* v;
    bf16_t* out;                // [R][H*64]
    const float* bias;          // [H][L] by distance (self) or null (cross)
    const DecodeShared* shared; // self: n_keys = shared->step + 1
    const int* row_pos;         // slot mode: n_keys = row_pos[r] + 1; else null
    unsigned long long* stamp;  // measurement: as DecGemmArgs::stamp
    int n_keys_const;           // cross: fixed key count
    int slab_keys;              // keys allocated per (row, head) slab (L for self, T for cross)
    int rows_per_kv;            // 1 for self; n_channels for cross (row r reads segment r / n_channels)
    int row0, R, H, bias_stride;
    // fused query projection (cross-attention; wq == nullptr -> q is read from `q`): q = R(R(norm(x_r)*gain) . wq[head]^T)
    const bf16_t* wq;           // [H*64][512]
    const float* x_f32;         // [R][512] residual stream
    const float* gain;          // [512]
    const float* ssq; int ssq_stride;
    float eps;
    // O-projection folded into the self-attention kernel (wo != nullptr; self, 8 waves per (row, head)): the kernel ends with
    // its head's share of the projection, opart[r][h][0..512) = R(o_h) . wo[:, 64h..64h+64)^T, exactly the wave-h split-K partial
    // of the DG_RESID kernel; the fused cross-attention (ipart != nullptr) and the cross O-projection's residual read
    // (DecGemmArgs::part) sum the eight partials in wave order instead of reading an updated h
    const bf16_t* wo;           // [512][H*64]
    float* opart;               // [R][H][512]
    const float* ipart;         // [R][H][512]
    unsigned* chain_sync;       // fused cross-attention, or null: the arrival counters of the GEMM chain launched next (dec_chain.hip), zeroed here
    int force_many;             // test knob (YMT3_SELF_ATTN_2WAVE=1 at create): take the 2-waves-per-(row, head) form whatever the row count
};
int launch_dec_attention(bool self_attn, const DecAttnArgs& a, hipStream_t stream);
// one layer's self-attention (folded O-projection) and fused cross-attention as one launch (decode.hip: dec_attn_pair_kernel);
// pair_rows = [R][2] zeroed 128-byte counter lines the kernel leaves zeroed; 0 launched, < 0 not this kernel's shape
int launch_dec_attention_pair(const DecAttnArgs& self_args, const DecAttnArgs& cross_args, unsigned* pair_rows, unsigned* abort_word,
                              unsigned* host_abort, hipStream_t stream);

// multi-channel cross-attention with the query projection fused, one workgroup per (segment, head) (mc_cross_attn.hip)
struct McCrossArgs {
    const float* x_f32;         // [R][512] residual stream, row = row0 + seg*n_channels + channel
    const float* gain;          // [512]
    const float* ssq; int ssq_stride;
    const bf16_t* wq;           // [H*64][512]
    const bf16_t* k;            // [n_seg][H][T][64]
    const bf16_t* v;
    bf16_t* out;                // [R][H*64]
    int row0, n_seg, n_channels, H, T;
    float eps;
};
int init_mc_cross_kernels();
int launch_mc_cross_attention(const McCrossArgs& a, hipStream_t stream);

struct ArgmaxArgs {
    const float* logits;        // [R][V]
    float* h;                   // [R][d] residual stream to refill with the next embedding
    const bf16_t* embed;        // [V][d]
    const bf16_t* chan_embed;   // [K][d] or null
    DecodeShared* shared;
    int* finished;              // [R]
    float* ssq;                 // [SSQ_TILES][ssq_stride]
    int ssq_stride;
    int row0, R, V, d, n_channels, eos_id, pad_id;
    // slot mode (ymt3_transcribe_stream; all null otherwise): every row decodes at its own position row_pos[r], feeds
    // prompt[row_prompt[r] + p] at positions p < n_prompt and writes the token of position p >= n_prompt to
    // tokens_out[row_out[r] + p - n_prompt]; a row stops (finished = 1, position frozen) after EOS or n_steps emitted tokens
    int* row_pos;               // [R]
    const long long* row_out;   // [R]
    unsigned long long* stamp;  // measurement: as DecGemmArgs::stamp
    unsigned* ticket;           // or null: [rows / 32 + 1] sub-counters, one 128-byte line each (zero between launches): a two-level ticket for many rows
    unsigned* zero_sync;        // or null: counter lines (CHAIN_LINE words each) to leave zeroed for the next step's dec_step_kernel
    int zero_lines;
    const long long* row_prompt;   // slot mode, or null: [R] offset of the row's prompt (see row_pos)
    int* row_state;             // [R] automaton state of every row (read only under a constraint, see DecodeShared::c_allowed)
    // Layer 0's QKV projection as a gather, or null: qkv0[V][3 * H * 64] = what dec_gemm_kernel<DG_NORM_QKV_CACHE> writes for a row fed token
    // v (one channel: the residual stream entering layer 0 is embed[v] and nothing else).  The kernel that feeds a row also copies the fed
    // id's table row: the q third to q0[r], the k / v thirds to layer 0's caches at the position the next step decodes (nothing at
    // position L: the last position of a full-length decode has no next step) -- and the step launches no layer-0 projection.
    const bf16_t* qkv0;
    bf16_t* q0;                 // [R][H * 64]
    bf16_t* kcache0;            // layer 0: [R][H][L][64]
    bf16_t* vcache0;
    int H, L;
};
constexpr int QKV0_COLS = 3 * 512;      // a table row: 192 chunks of 16 bytes, one per thread of the feeding kernels
int launch_argmax_embed(const ArgmaxArgs& a, hipStream_t stream);
// the layer-0 table build: h[i] = embed[v0 + i] with its sum(h^2) tiles, i in [0, n), through embed_row (a.h / a.ssq: scratch of n rows)
int launch_qkv0_embed(const ArgmaxArgs& a, int v0, int n, hipStream_t stream);
// tokens_out[r][from .. n_steps) = pad (scores_out, if not null: 0.0) for rows [row0, row0 + R): the tail of a decode that stopped
// early (`from`: emitted index)
int launch_pad_tail(int32_t* tokens_out, float* scores_out, int row0, int R, int n_steps, int from, int pad_id, hipStream_t stream);
// slot mode: (re)start rows [row0, row0 + n_channels) on a new segment: h = embed[pad] (+ channel), position 0,
// finished = 0, row_out = first_out + channel * n_steps, row_prompt = first_prompt + channel * n_prompt,
// row_state = cv.start[channel] clamped into [0, cv.n_states) (0 without start states)
int launch_slot_start(const ArgmaxArgs& a, int row0, long long first_out, int n_steps, long long* row_out, long long first_prompt,
                      int n_prompt, long long* row_prompt, const ConstraintView& cv, hipStream_t stream);
// slot mode: PAD the unwritten tail [row_pos + 1 - n_prompt, n_steps) of rows [row0, row0 + n_rows) (scores_out, if not null: 0.0)
int launch_slot_retire(const ArgmaxArgs& a, int row0, int n_rows, int n_steps, int n_prompt, int32_t* tokens_out, float* scores_out,
                       hipStream_t stream);
// all rows: h[r] = embed[pad] (+ chan_embed), finished = 0, row_state = cv.start[r] clamped into [0, cv.n_states) (0 without start
// states); a.shared[0..n_chains) reset (prompt / n_prompt / the automaton: every chain's)
int launch_decode_init(const ArgmaxArgs& a, int n_chains, int n_steps, int step0, int32_t* tokens_out, const int32_t* forced,
                       float* logits_out, const int32_t* prompt, int n_prompt, float* scores_out, const ConstraintView& cv,
                       hipStream_t stream);

// ---------------------------------------------------------------- beam search (beam.hip; self-attention: decode.hip)
// Rows of a beam call: r = (segment * n_channels + channel) * W + beam; a group = the W rows of one (segment, channel).  K/V of a position
// stays in the slab of the physical row that computed it; anc[buf][r][p] (one byte: the row's index within its group) says which row of the
// group holds position p of the history of the beam now living in row r.  Two buffers alternate by the parity of the position being decoded
// (the selection kernel of step t reads buffer t & 1 and writes buffer (t + 1) & 1, entries 0 .. t + 1).
constexpr int BEAM_MAX = 8;
struct BeamAttn {               // what the ancestry-addressed self-attention needs on top of DecAttnArgs
    const uint8_t* anc;         // [2][anc_rows][anc_pitch]
    int anc_rows, anc_pitch, W;
};
int launch_dec_attention_beam(const DecAttnArgs& a, const BeamAttn& ba, hipStream_t stream);

struct BeamShared {             // device-resident per-call parameters of the beam kernels: no captured graph depends on a call's arguments
    float alpha;                // length penalty
    int32_t* tokens_out;        // [G][N][n_steps]
    float* seq_out;             // [G][N] or null (N = num_return: the grid of the result kernel)
    float* tok_out;             // [G][N][n_steps] or null
    // debug hook ymt3_debug_beam_trace (null otherwise)
    int32_t* trace;             // [trace_steps][trace_groups][W][2] = (parent, token) of every new running beam
    float* trace_run;           // [trace_steps][trace_groups][W] its cumulative log-probability
    float* trace_logits;        // [trace_steps][trace_groups][W][V] raw logits of the running beams the step selected from, or null
    int trace_steps, trace_groups;
};
struct BeamArgs {
    const float* logits;        // [R][V]
    float* h;                   // [R][d] residual stream to refill with the fed tokens' embeddings
    const bf16_t* embed; const bf16_t* chan_embed;
    DecodeShared* shared; BeamShared* beam;
    int* finished;              // [R]: 1 for every row of a done group
    float* ssq; int ssq_stride;
    int R, V, d, n_channels, eos_id, pad_id, W;
    int* row_state;             // [R] automaton state of every running beam
    uint8_t* anc; int anc_rows, anc_pitch;
    int32_t* fed_tok; float* fed_lp; int fed_pitch;    // [R][fed_pitch]: the token fed into physical row r at position p, and its log-probability
    float* run;                 // [R] cumulative log-probability of every running beam
    float* fin_score; int* fin_len; int* fin_store; int32_t* fin_tok; float* fin_lp;   // [R] = [G][W] finished slots, best first
    int* n_fin;                 // [G] filled slots
    uint8_t* slot_anc;          // [R][anc_pitch]: ancestry snapshots of the finished hypotheses, indexed by fin_store
    unsigned long long* stamp;
    // slot mode (ymt3_transcribe_stream_beam; all null otherwise): a group decodes at its own position row_pos[r] (the same for its W rows),
    // feeds prompt[row_prompt[r] + p] at positions p < n_prompt, and row_out[r] is its index in the queue, (segment * n_channels + channel):
    // where its results and its debug trace go.  A group whose `finished` flag is set is stopped: its state and position stay as they are.
    int* row_pos;               // [R]
    long long* row_out;         // [R]
    long long* row_prompt;      // [R]
};
int launch_beam_select(const BeamArgs& a, hipStream_t stream);
// all rows: h[r] = embed[pad] (+ channel), run = 0 / -1e9, slots empty, anc[step0 & 1][r][0] = own index, automaton start state of the
// row's group; loop state and beam parameters reset
int launch_beam_init(const BeamArgs& a, int n_steps, const int32_t* prompt, int n_prompt, const ConstraintView& cv, const BeamShared& params,
                     hipStream_t stream);
// tokens_out / seq_out / tok_out from the finished slots
int launch_beam_finalize(const BeamArgs& a, int N, hipStream_t stream);
// slot mode: (re)start rows [row0, row0 + n_channels * W) on the segment whose groups have queue indices first_group ..: h = embed[pad]
// (+ channel), run = 0 / -1e9, slots empty, anc[0][r][0] = own index, position 0, finished = 0, the automaton state from cv.start[channel]
// clamped (the segment's start states; 0 without), row_out / row_prompt of the group
int launch_beam_slot_start(const BeamArgs& a, int row0, long long first_group, int n_prompt, const ConstraintView& cv, hipStream_t stream);
// slot mode: the results of the n_channels groups from row row0 on, written at their queue indices
int launch_beam_slot_finalize(const BeamArgs& a, int row0, int N, hipStream_t stream);

// ---------------------------------------------------------------- full-sequence decoder pass (dec_seq.hip)
// Teacher-forced scoring (include/ymt3.h, sequence scoring): every position of every decoder row at once.  A chunk holds n_rows whole
// decoder rows of L = n_prompt + n_steps positions; activation row m = local row * L + position; row0 = the chunk's first decoder row.
struct SeqEmbedArgs {
    float* h;                   // [n_rows * L][d] f32 residual rows: embed[fed id] (+ chan_embed[row % n_channels])
    const bf16_t* embed;        // [V][d]
    const bf16_t* chan_embed;   // [n_channels][d] or null
    const int32_t* prompt;      // [R][n_prompt] or null (n_prompt = 0)
    const int32_t* tokens;      // [R][n_steps]; position 0 feeds pad_id, 1 .. P the prompt, P + j + 1 tokens[j] (clamped into [0, V))
    int row0, n_rows, L, n_prompt, n_steps, V, d, n_channels, pad_id;
};
int launch_seq_embed(const SeqEmbedArgs& a, hipStream_t stream);
// softmax(Q K^T (+ bias, causal)) V per (decoder row, head); query row (r, t) at q + r * q_seq + t * ldq + h * 64, key / value row (b, t) at
// k|v + b * kv_seq + h * kv_head + t * ldkv with b = (row0 + r) / rows_per_kv, output row at out + r * o_seq + t * ldo + h * 64.
// causal: n_keys = L, key <= query only, bias[h][query - key] added ([H][bias_stride] by distance); else all n_keys keys, no bias.
struct SeqAttnDecArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* out;
    const float* bias;
    long long q_seq, kv_seq, o_seq;
    int ldq, ldkv, ldo, kv_head;
    int row0, n_rows, L, n_keys, rows_per_kv, H, bias_stride;
};
int launch_dec_seq_attention(bool causal, const SeqAttnDecArgs& a, hipStream_t stream);
// logits = xn . W^T in column tiles with an online log-sum-exp: scores[row][j] = logit[tokens[row][j]] - lse for the emitted column
// j = position - n_prompt >= 0 (0.0 for j >= lengths[row]; prompt positions write nothing); logits[row][j][V] only when not null
struct SeqLmHeadArgs {
    const bf16_t* xn;           // [M][d] final-normed rows
    const bf16_t* W;            // [V][d] lm_head
    const int32_t* tokens;      // [R][n_steps] targets (clamped into [0, V))
    const int32_t* lengths;     // [R] or null: n_steps
    float* scores;              // [R][n_steps]
    float* logits;              // [R][n_steps][V] or null
    int M, L, n_prompt, n_steps, V, d, row0;
};
int launch_seq_lm_head_score(const SeqLmHeadArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- MoE decoder FFN (moe.hip)
struct MoeArgs {
    float* h;                   // [R][d_model] fp32 residual stream (read by router, updated by combine)
    const float* gain;          // [d_model]
    float* ssq; int ssq_stride; // carried sum(h^2) partials
    const bf16_t* router;       // [E][d_model]
    const bf16_t* wi;           // [E][d_ff][d_model]
    const bf16_t* wo;           // [E][d_model][d_ff]
    const uint8_t* wi_q8; const uint8_t* wo_q8;   // fp8 (OCP e4m3) forms, same shapes
    const float* wi_s; const float* wo_s;         // [E] dequantisation scales
    int fp8;
    bf16_t* xn;                 // [R][d_model] normed rows (bf16)
    int* sel; float* gate;      // [R][2] chosen experts and their gates; pair p = 2 * row + slot
    bf16_t* hidden;             // [2R][d_ff] by pair
    float* y;                   // [2R][d_model] gate-scaled expert outputs by pair
    int row0, R, E, top_k, d_model, d_ff;
    float eps;
    // debug hook ymt3_debug_moe_trace (null otherwise): the router also records its choices, [step][layer][row][2] int32, so a test can
    // teacher-force the ORACLE's routing with them and check every choice was a legitimate near-tie instead of excluding such steps
    int32_t* sel_trace; const DecodeShared* shared; int layer, n_layers, trace_rows, trace_steps;
};
int init_moe_kernels();
int launch_moe_stage(int stage, const MoeArgs& a, hipStream_t stream);

// The MoE layer's five skinny launches -- cross O-projection, router, expert FFN-in, expert FFN-out, the next QKV projection (or lm_head) with the
// combine folded in -- as ONE launch (moe_chain.hip); up to 64 rows, one channel, 8 experts, top-2; bf16 or fp8 expert weights.
struct MoeChainArgs {
    const bf16_t* wo_c; const void* wi; const void* wo; const bf16_t* w3;     // [512][512]; experts [8][2048][512] / [8][512][2048] (bf16 or e4m3); next wqkv / lm_head
    const bf16_t* attn; float* h; const float* part; float* ssq; int ssq_stride;   // as ChainArgs
    const float* gain_r; const bf16_t* router; bf16_t* xn; int* sel; float* gate;  // router: ln3, [8][512]; scratch [R][512], [2R], [2R]
    const float* wi_s; const float* wo_s;                                         // fp8: per-expert dequantisation scales
    bf16_t* hidden; float* y;                                                     // [2R][2048], [2R][512] by pair
    const float* gain3; int mode3, N3;                                            // stage 4: the next layer's ln1 or ln_f; DG_NORM_QKV_CACHE / DG_NORM_LOGITS
    float* h_out;                                                                 // QKV mode: the other residual buffer (column tile 0 stores h + y0 + y1 there)
    bf16_t* out_q; bf16_t* kcache; bf16_t* vcache; float* logits; int H, L;
    const DecodeShared* shared; const int* row_pos;
    int R, E, fp8;
    float eps;
    unsigned* sync; unsigned* host_abort;                                         // the chain's counter block (zeroed by the preceding cross-attention launch) + abort word
    unsigned long long* stamp;
    int32_t* sel_trace; int layer, n_layers, trace_rows, trace_steps;             // debug hook ymt3_debug_moe_trace, as MoeArgs
};
int init_moe_chain_kernels();
bool moe_chain_fits(int n_cus, bool fp8);
int launch_moe_chain(const MoeChainArgs& c, hipStream_t stream);       // 0 launched, < 0: not this kernel's shape
