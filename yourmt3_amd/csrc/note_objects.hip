// The note-side objects of the C ABI (include/ymt3.h): detokeniser and its incremental state, tokeniser, note metrics, piano roll / frame
// metrics, aligner, note velocities, beat tracker, bar tracker, chord tracker, section tracker, hand splitter.  Host logic only: argument checks, scratch, and the launches of detok.hip, tok.hip, metrics.hip, roll.hip,
// align.hip, velocity.hip, beats.hip, bars.hip, chords.hip, sections.hip and hands.hip.  Of the handle they need the device and the configuration (runtime.h).  What they have in common is written once, at the top: the
// create prologue, the owner check, the program and record-array checks, and the scratch list that both *_create and *_destroy walk.
#include <algorithm>
#include <cmath>
#include <vector>

#include "kernels.h"
#include "runtime.h"

// ---------------------------------------------------------------- shared checks
// name: the argument every create but the state's needs besides the handle (NULL: none)
static int create_prologue(void** out, ymt3_handle h, const void* arg, const char* name) {
    if (!out) FAIL(YMT3_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (name && !arg) FAIL(YMT3_ERR_ARG, "%s is NULL", name);
    return YMT3_OK;
}

template <class T> static int check_owner(ymt3_handle h, const T* o, const char* noun) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!o) FAIL(YMT3_ERR_ARG, "null %s", noun);
    if (o->owner != h) FAIL(YMT3_ERR_ARG, "the %s belongs to another handle", noun);
    return YMT3_OK;
}

// why: what the object's limit comes from, ending in ", " (or empty)
static int check_programs(int n_programs, int drum_program, int max_programs, const char* why) {
    if (n_programs < 1) FAIL(YMT3_ERR_ARG, "n_programs=%d must be >= 1", n_programs);
    if (n_programs > max_programs) FAIL(YMT3_ERR_UNSUPPORTED, "n_programs=%d: %sat most %d programs", n_programs, why, max_programs);
    if (drum_program < 0 || drum_program >= n_programs) FAIL(YMT3_ERR_ARG, "drum_program=%d outside [0, n_programs=%d)", drum_program, n_programs);
    return YMT3_OK;
}

// A record array of a call: its count is in [0, max] (max_name: the object's limit of that name, or NULL for a constant of the kernels) ...
static int check_count(const char* n_name, long long n, long long max, const char* max_name) {
    if (n < 0 || n > max) FAIL(YMT3_ERR_ARG, "%s=%lld outside [0, %s%s%lld]", n_name, n, max_name ? max_name : "", max_name ? "=" : "", max);
    return YMT3_OK;
}
// ... and where it has records (always: without them too) its pointer is there and aligned for the records' doubles
static int check_record_ptr(const char* ptr_name, const void* p, long long n, bool always = false) {
    if (n && !p) FAIL(YMT3_ERR_ARG, "%s is NULL", ptr_name);
    if ((n || always) && reinterpret_cast<uintptr_t>(p) % 8) FAIL(YMT3_ERR_ARG, "%s is not aligned to 8 bytes", ptr_name);
    return YMT3_OK;
}

// ---------------------------------------------------------------- scratch
// One device allocation of an object (src: host data to upload, or NULL; zero: zero-filled at create).  Every object type has a slots() that
// lists its allocations: *_create allocates and fills them in that order, *_destroy frees them.
struct Slot { void** p; size_t bytes; const void* src; bool zero; };
template <class T> static Slot slot(T** p, size_t bytes, const void* src = nullptr, bool zero = false) { return Slot{reinterpret_cast<void**>(p), bytes, src, zero}; }

template <class T> static void destroy_object(T* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    for (const Slot& s : slots(o))
        if (*s.p) (void)hipFree(*s.p);
    delete o;
}

// the tail of every create: on failure nothing is leaked, no object is returned and HIP's sticky error is cleared (unnamed: bytes of the
// list that the message's total leaves out)
template <class T> static int allocate_object(T* o, const std::vector<Slot>& list, const char* what, T** out, size_t unnamed = 0) {
    size_t total = 0;
    bool ok = true;
    for (const Slot& s : list) {
        total += s.bytes;
        ok = ok && hipMalloc(s.p, s.bytes) == hipSuccess && (!s.src || hipMemcpy(*s.p, s.src, s.bytes, hipMemcpyHostToDevice) == hipSuccess) &&
             (!s.zero || hipMemset(*s.p, 0, s.bytes) == hipSuccess);
    }
    if (ok) { *out = o; return YMT3_OK; }
    (void)hipGetLastError();
    destroy_object(o);
    FAIL(YMT3_ERR_HIP, "%s (%zu bytes) could not be allocated", what, total - unnamed);
}

// ---------------------------------------------------------------- device detokeniser (include/ymt3.h)
struct ymt3_detok_s {
    ymt3_handle owner;
    int device, n_chan, vocab, steps_per_second, drum_program, n_programs, max_segments, max_steps;
    uint16_t* table = nullptr;              // [vocab]
    unsigned long long* items = nullptr;    // [n_channels * max_segments * max_steps]
    unsigned long long* sorted = nullptr;   // the same
    uint16_t* keys = nullptr;               // the same
    int* row_count = nullptr;               // [n_channels * max_segments]
    unsigned* key_off = nullptr;            // [n_channels][n_programs * 128]
};

static std::vector<Slot> slots(ymt3_detok d, const uint16_t* table_host = nullptr) {
    const size_t rows = (size_t)d->max_segments * d->n_chan, n = rows * d->max_steps;
    return {slot(&d->table, (size_t)d->vocab * 2, table_host), slot(&d->items, n * 8), slot(&d->sorted, n * 8), slot(&d->keys, n * 2),
            slot(&d->row_count, rows * sizeof(int)), slot(&d->key_off, (size_t)d->n_chan * d->n_programs * DETOK_PITCHES * sizeof(unsigned))};
}
extern "C" void ymt3_detok_destroy(ymt3_detok d) { destroy_object(d); }

extern "C" int ymt3_detok_create(ymt3_handle h, const uint16_t* token_table_host, int vocab, int steps_per_second, int drum_program,
                                 int max_segments, int max_steps, ymt3_detok* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, token_table_host, "token_table_host")) return rc;
    const ymt3_config& cfg = handle_config(h);
    if (vocab != cfg.vocab) FAIL(YMT3_ERR_ARG, "detokeniser vocab=%d != the model's vocab=%d", vocab, cfg.vocab);
    if (steps_per_second < 1) FAIL(YMT3_ERR_ARG, "steps_per_second=%d must be >= 1", steps_per_second);
    if (drum_program < 0 || drum_program > 4095) FAIL(YMT3_ERR_ARG, "drum_program=%d outside [0, 4095]", drum_program);
    if (max_segments < 1 || max_segments > DETOK_MAX_SEGMENTS) FAIL(YMT3_ERR_ARG, "max_segments=%d outside [1, %d]", max_segments, DETOK_MAX_SEGMENTS);
    if (max_steps < 1 || max_steps > cfg.max_decode_len || max_steps > DETOK_MAX_STEPS)
        FAIL(YMT3_ERR_ARG, "max_steps=%d outside [1, max_decode_len=%d]", max_steps, std::min(cfg.max_decode_len, DETOK_MAX_STEPS));
    int n_programs = drum_program + 1;
    for (int i = 0; i < vocab; ++i) {
        const int cls = token_table_host[i] >> 12, v = token_table_host[i] & 0xfff;
        if (cls > 8) FAIL(YMT3_ERR_ARG, "token_table_host[%d] has class %d (0..8 are defined)", i, cls);
        if ((cls == 4 || cls == 8) && v >= DETOK_PITCHES) FAIL(YMT3_ERR_ARG, "token_table_host[%d]: pitch %d outside [0, %d)", i, v, DETOK_PITCHES);
        if (cls == 5 && v > 1) FAIL(YMT3_ERR_ARG, "token_table_host[%d]: velocity %d is neither 0 (offsets) nor 1 (onsets)", i, v);
        if (cls == 7) n_programs = std::max(n_programs, v + 1);
    }
    if (n_programs > DETOK_MAX_PROGRAMS)
        FAIL(YMT3_ERR_UNSUPPORTED, "programs up to %d: the merge keeps one LDS counter per (program, pitch), at most %d programs", n_programs - 1, DETOK_MAX_PROGRAMS);
    HIP_TRY(hipSetDevice(handle_device(h)));
    if (init_detok_kernels()) FAIL(YMT3_ERR_HIP, "hipFuncSetAttribute(max dynamic LDS) failed");
    ymt3_detok d = new ymt3_detok_s{h, handle_device(h), cfg.n_channels, vocab, steps_per_second, drum_program, n_programs, max_segments, max_steps};
    return allocate_object(d, slots(d, token_table_host), "detokeniser scratch", out, (size_t)vocab * 2);     // (the message never counted the table)
}

// what ymt3_detokenize and the incremental calls tell the kernels about the tokens and the output
static DetokArgs detok_args(ymt3_detok d, const int32_t* tokens_dev, const float* scores_dev, int n_segments, int L, long long seg_stride, long long chan_stride,
                            const double* start_sec_dev, double end_sec, void* notes_dev, long long capacity, int32_t* counts_dev) {
    DetokArgs a{};
    a.table = d->table; a.vocab = d->vocab; a.steps_per_second = d->steps_per_second; a.drum_program = d->drum_program; a.n_programs = d->n_programs;
    a.tokens = tokens_dev; a.scores = scores_dev; a.seg_stride = seg_stride; a.chan_stride = chan_stride;
    a.n_seg = n_segments; a.n_chan = d->n_chan; a.L = L;
    a.start = start_sec_dev; a.end_sec = end_sec;
    a.items = d->items; a.keys = d->keys; a.row_count = d->row_count; a.sorted = d->sorted; a.key_off = d->key_off;
    a.notes = static_cast<DetokNote*>(notes_dev); a.capacity = capacity; a.counts = counts_dev;
    return a;
}

extern "C" int ymt3_detokenize(ymt3_handle h, ymt3_detok d, const int32_t* tokens_dev, const float* scores_dev, int n_segments, int n_steps,
                               long long seg_stride, long long chan_stride, const double* start_sec_dev, double end_sec, void* notes_dev,
                               long long capacity, int32_t* counts_dev, void* stream) {
    if (const int rc = check_owner(h, d, "detokeniser")) return rc;
    if (n_segments < 0 || n_segments > d->max_segments) FAIL(YMT3_ERR_ARG, "n_segments=%d outside [0, max_segments=%d]", n_segments, d->max_segments);
    if (n_steps < 1 || n_steps > d->max_steps) FAIL(YMT3_ERR_ARG, "n_steps=%d outside [1, max_steps=%d]", n_steps, d->max_steps);
    if (!counts_dev) FAIL(YMT3_ERR_ARG, "counts_dev is NULL");
    if (n_segments && !tokens_dev) FAIL(YMT3_ERR_ARG, "tokens_dev is NULL");
    if (n_segments && !start_sec_dev) FAIL(YMT3_ERR_ARG, "start_sec_dev is NULL");
    if (n_segments && !notes_dev) FAIL(YMT3_ERR_ARG, "notes_dev is NULL");
    const long long bound = (long long)n_segments * d->n_chan * n_steps;
    if (capacity < bound) FAIL(YMT3_ERR_ARG, "capacity=%lld below n_segments * n_channels * n_steps = %lld records", capacity, bound);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts_dev, 0, 2 * sizeof(int32_t), s));
    if (!n_segments) return YMT3_OK;
    const DetokArgs a = detok_args(d, tokens_dev, scores_dev, n_segments, n_steps, seg_stride, chan_stride, start_sec_dev, end_sec, notes_dev, capacity, counts_dev);
    LAUNCH(launch_detok(a, s));
    return YMT3_OK;
}

// ---------------------------------------------------------------- incremental detokeniser (include/ymt3.h)
struct ymt3_detok_state_s {
    ymt3_handle owner;
    ymt3_detok detok;                       // the detokeniser it was created for (compared by address only)
    int device, n_chan, n_programs, max_held;
    DetokSounding* sounding = nullptr;      // [n_chan][n_programs * 128]
    DetokHeld* held[2] = {nullptr, nullptr};   // [n_chan][128][max_held], read from [cur], written to [cur ^ 1]
    int* held_count[2] = {nullptr, nullptr};   // [n_chan][128]
    int cur = 0;
    double horizon = -INFINITY;             // of the last push
    bool finished = false;
};

static size_t detok_state_sounding_bytes(const ymt3_detok_state_s* st) { return (size_t)st->n_chan * st->n_programs * DETOK_PITCHES * sizeof(DetokSounding); }
static size_t detok_state_count_bytes(const ymt3_detok_state_s* st) { return (size_t)st->n_chan * DETOK_PITCHES * sizeof(int); }
static std::vector<Slot> slots(ymt3_detok_state st) {
    const size_t hb = (size_t)st->n_chan * DETOK_PITCHES * st->max_held * sizeof(DetokHeld), cb = detok_state_count_bytes(st);
    return {slot(&st->sounding, detok_state_sounding_bytes(st), nullptr, true), slot(&st->held[0], hb), slot(&st->held[1], hb),
            slot(&st->held_count[0], cb, nullptr, true), slot(&st->held_count[1], cb, nullptr, true)};
}
extern "C" void ymt3_detok_state_destroy(ymt3_detok_state st) { destroy_object(st); }

extern "C" long long ymt3_detok_state_carry(ymt3_detok_state st) {
    return st ? (long long)st->n_chan * DETOK_PITCHES * ((long long)st->n_programs - 1 + st->max_held) : 0;
}

extern "C" int ymt3_detok_state_create(ymt3_handle h, ymt3_detok d, int max_held, ymt3_detok_state* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, nullptr, nullptr)) return rc;
    if (const int rc = check_owner(h, d, "detokeniser")) return rc;
    if (max_held < 1 || max_held > 4096) FAIL(YMT3_ERR_ARG, "max_held=%d outside [1, 4096]", max_held);
    HIP_TRY(hipSetDevice(d->device));
    ymt3_detok_state st = new ymt3_detok_state_s{h, d, d->device, d->n_chan, d->n_programs, max_held};
    return allocate_object(st, slots(st), "detokeniser state", out);
}

extern "C" int ymt3_detok_state_reset(ymt3_handle h, ymt3_detok_state st, void* stream) {
    if (const int rc = check_owner(h, st, "detokeniser state")) return rc;
    HIP_TRY(hipSetDevice(st->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(st->sounding, 0, detok_state_sounding_bytes(st), s));
    HIP_TRY(hipMemsetAsync(st->held_count[st->cur], 0, detok_state_count_bytes(st), s));
    st->horizon = -INFINITY;
    st->finished = false;
    return YMT3_OK;
}

// the shared tail of push and finish: n_segments = 0 walks the state alone
static int detok_carry(ymt3_handle h, ymt3_detok d, ymt3_detok_state st, const int32_t* tokens_dev, const float* scores_dev, int n_segments,
                       int n_steps, long long seg_stride, long long chan_stride, const double* start_sec_dev, double horizon, double end_sec,
                       int finish, void* notes_dev, long long capacity, int32_t* counts_dev, void* stream) {
    if (h && d && !st) FAIL(YMT3_ERR_ARG, "null detokeniser state");
    if (const int rc = check_owner(h, d, "detokeniser")) return rc;
    if (st->owner != h || st->detok != d) FAIL(YMT3_ERR_ARG, "the detokeniser state was created for another detokeniser");
    if (st->finished) FAIL(YMT3_ERR_ARG, "the state has been finished: reset it first");
    if (n_segments < 0 || n_segments > d->max_segments) FAIL(YMT3_ERR_ARG, "n_segments=%d outside [0, max_segments=%d]", n_segments, d->max_segments);
    if (n_segments && (n_steps < 1 || n_steps > d->max_steps)) FAIL(YMT3_ERR_ARG, "n_steps=%d outside [1, max_steps=%d]", n_steps, d->max_steps);
    if (!counts_dev) FAIL(YMT3_ERR_ARG, "counts_dev is NULL");
    if (!notes_dev) FAIL(YMT3_ERR_ARG, "notes_dev is NULL");
    if (n_segments && !tokens_dev) FAIL(YMT3_ERR_ARG, "tokens_dev is NULL");
    if (n_segments && !start_sec_dev) FAIL(YMT3_ERR_ARG, "start_sec_dev is NULL");
    if (!finish && !(horizon >= st->horizon && horizon > -INFINITY))
        FAIL(YMT3_ERR_ARG, "horizon_sec=%g is -inf, NaN or below the previous push's horizon %g", horizon, st->horizon);
    const long long bound = (long long)n_segments * d->n_chan * (n_segments ? n_steps : 0) + ymt3_detok_state_carry(st);
    if (capacity < bound)
        FAIL(YMT3_ERR_ARG, "capacity=%lld below n_segments * n_channels * n_steps + ymt3_detok_state_carry = %lld records", capacity, bound);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts_dev, 0, 3 * sizeof(int32_t), s));
    const DetokArgs a = detok_args(d, tokens_dev, scores_dev, n_segments, n_segments ? n_steps : 1, seg_stride, chan_stride, start_sec_dev, end_sec,
                                   notes_dev, capacity, counts_dev);
    DetokCarryArgs c{};
    c.sounding = st->sounding; c.held_in = st->held[st->cur]; c.held_out = st->held[st->cur ^ 1];
    c.held_count_in = st->held_count[st->cur]; c.held_count_out = st->held_count[st->cur ^ 1];
    c.max_held = st->max_held; c.finish = finish; c.horizon = horizon;
    LAUNCH(launch_detok_carry(a, c, s));
    HIP_TRY(hipGetLastError());
    st->cur ^= 1;
    if (finish) st->finished = true;
    else st->horizon = horizon;
    return YMT3_OK;
}

extern "C" int ymt3_detokenize_push(ymt3_handle h, ymt3_detok d, ymt3_detok_state st, const int32_t* tokens_dev, const float* scores_dev,
                                    int n_segments, int n_steps, long long seg_stride, long long chan_stride, const double* start_sec_dev,
                                    double horizon_sec, void* notes_dev, long long capacity, int32_t* counts_dev, void* stream) {
    return detok_carry(h, d, st, tokens_dev, scores_dev, n_segments, n_steps, seg_stride, chan_stride, start_sec_dev, horizon_sec, 0.0, 0,
                       notes_dev, capacity, counts_dev, stream);
}

extern "C" int ymt3_detokenize_finish(ymt3_handle h, ymt3_detok d, ymt3_detok_state st, double end_sec, void* notes_dev, long long capacity,
                                      int32_t* counts_dev, void* stream) {
    return detok_carry(h, d, st, nullptr, nullptr, 0, 0, 0, 0, nullptr, INFINITY, end_sec, 1, notes_dev, capacity, counts_dev, stream);
}

// ---------------------------------------------------------------- device tokeniser (include/ymt3.h)
struct ymt3_tok_s {
    ymt3_handle owner;
    int device, n_chan;
    ymt3_tok_params p;
    int n_programs, max_segments, max_steps;
    uint8_t* program_channel = nullptr;     // [n_programs]
    unsigned long long* items = nullptr;    // [max_segments * n_channels * max_steps]
    int* row_count = nullptr;               // [max_segments * n_channels]
    unsigned* tie_seen = nullptr;           // [max_segments][n_programs * 4]
};

static std::vector<Slot> slots(ymt3_tok t, const uint8_t* program_channel_host = nullptr) {
    const size_t rows = (size_t)t->max_segments * t->n_chan;
    return {slot(&t->program_channel, (size_t)t->n_programs, program_channel_host), slot(&t->items, rows * t->max_steps * 8),
            slot(&t->row_count, rows * sizeof(int)), slot(&t->tie_seen, (size_t)t->max_segments * t->n_programs * (TOK_PITCHES / 8))};
}
extern "C" void ymt3_tok_destroy(ymt3_tok t) { destroy_object(t); }

extern "C" int ymt3_tok_create(ymt3_handle h, const ymt3_tok_params* params, const uint8_t* program_channel_host, int n_programs, int max_segments,
                               int max_steps, ymt3_tok* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    if (!program_channel_host) FAIL(YMT3_ERR_ARG, "program_channel_host is NULL");
    const ymt3_tok_params& p = *params;
    const ymt3_config& cfg = handle_config(h);
    if (const int rc = check_programs(n_programs, 0, TOK_MAX_PROGRAMS, "an item gives the program 8 bits, ")) return rc;     // n_programs only (0 is always a valid drum)
    if (p.steps_per_second < 1) FAIL(YMT3_ERR_ARG, "steps_per_second=%d must be >= 1", p.steps_per_second);
    if (p.max_shift_steps < 1) FAIL(YMT3_ERR_ARG, "max_shift_steps=%d must be >= 1", p.max_shift_steps);
    if (const int rc = check_programs(n_programs, p.drum_program, TOK_MAX_PROGRAMS, "")) return rc;     // n_programs passed above: this tests drum_program, where it always was
    const struct { const char* name; int base, size; } ranges[] = {
        {"shift_base", p.shift_base, p.max_shift_steps}, {"pitch_base", p.pitch_base, TOK_PITCHES}, {"velocity_base", p.velocity_base, 2},
        {"tie_base", p.tie_base, 1}, {"program_base", p.program_base, n_programs}, {"drum_base", p.drum_base, TOK_PITCHES},
        {"eos_id", p.eos_id, 1}, {"pad_id", p.pad_id, 1}};
    for (const auto& r : ranges)
        if (r.base < 0 || (long long)r.base + r.size > cfg.vocab) FAIL(YMT3_ERR_ARG, "%s=%d: its %d ids do not fit the model's vocab=%d", r.name, r.base, r.size, cfg.vocab);
    for (int i = 0; i < n_programs; ++i)
        if (program_channel_host[i] >= cfg.n_channels) FAIL(YMT3_ERR_ARG, "program_channel_host[%d]=%d outside [0, n_channels=%d)", i, (int)program_channel_host[i], cfg.n_channels);
    if (max_segments < 1 || max_segments > TOK_MAX_SEGMENTS) FAIL(YMT3_ERR_ARG, "max_segments=%d outside [1, %d]", max_segments, TOK_MAX_SEGMENTS);
    if (max_steps < 1 || max_steps > cfg.max_decode_len || max_steps > TOK_MAX_STEPS)
        FAIL(YMT3_ERR_ARG, "max_steps=%d outside [1, max_decode_len=%d]", max_steps, std::min(cfg.max_decode_len, TOK_MAX_STEPS));
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_tok t = new ymt3_tok_s{h, handle_device(h), cfg.n_channels, p, n_programs, max_segments, max_steps};
    return allocate_object(t, slots(t, program_channel_host), "tokeniser scratch", out);
}

extern "C" int ymt3_tokenize(ymt3_handle h, ymt3_tok t, const void* notes_dev, long long n_notes, const double* start_sec_dev, int n_segments,
                             double end_sec, int n_steps, int32_t* tokens_dev, int32_t* lengths_dev, void* stream) {
    if (const int rc = check_owner(h, t, "tokeniser")) return rc;
    if (n_segments < 0 || n_segments > t->max_segments) FAIL(YMT3_ERR_ARG, "n_segments=%d outside [0, max_segments=%d]", n_segments, t->max_segments);
    if (n_steps < 1 || n_steps > t->max_steps) FAIL(YMT3_ERR_ARG, "n_steps=%d outside [1, max_steps=%d]", n_steps, t->max_steps);
    if (const int rc = check_count("n_notes", n_notes, TOK_MAX_NOTES, nullptr)) return rc;
    if (!n_segments) return YMT3_OK;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes, true)) return rc;
    if (!start_sec_dev) FAIL(YMT3_ERR_ARG, "start_sec_dev is NULL");
    if (!tokens_dev) FAIL(YMT3_ERR_ARG, "tokens_dev is NULL");
    if (!lengths_dev) FAIL(YMT3_ERR_ARG, "lengths_dev is NULL");
    HIP_TRY(hipSetDevice(t->device));
    const ymt3_tok_params& p = t->p;
    TokArgs a{};
    a.shift_base = p.shift_base; a.pitch_base = p.pitch_base; a.velocity_base = p.velocity_base; a.tie_base = p.tie_base;
    a.program_base = p.program_base; a.drum_base = p.drum_base; a.max_shift_steps = p.max_shift_steps; a.steps_per_second = p.steps_per_second;
    a.drum_program = p.drum_program; a.eos_id = p.eos_id; a.pad_id = p.pad_id;
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n_notes = n_notes;
    a.start = start_sec_dev; a.end_sec = end_sec; a.n_seg = n_segments; a.n_chan = t->n_chan; a.L = n_steps;
    a.items = t->items; a.row_count = t->row_count; a.tie_seen = t->tie_seen;
    a.n_programs = t->n_programs; a.program_channel = t->program_channel; a.tokens = tokens_dev; a.lengths = lengths_dev;
    LAUNCH(launch_tok(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- device note metrics (include/ymt3.h)
struct ymt3_metrics_s {
    ymt3_handle owner;
    int device;
    ymt3_metrics_params p;
    long long max_ref, max_est;
    unsigned* hist = nullptr;               // [2][n_keys], then off [2][n_keys + 1] and cursor [2][n_keys]: one allocation
    double2* t_ref = nullptr;               // [2 * max_ref]
    double2* t_est = nullptr;               // [2 * max_est]
    int2* win = nullptr;                    // [2 * max_ref], then stack [2 * max_ref]: one allocation
    int* match = nullptr;                   // [2 * max_est], then visit [2 * max_est]: one allocation
};

static std::vector<Slot> slots(ymt3_metrics m) {
    const size_t nk = (size_t)(m->p.n_programs + 1) * METRICS_PITCHES;
    const size_t rs = 2 * (size_t)m->max_ref, es = 2 * (size_t)m->max_est;       // bucket slots: a counted note fills at most two
    return {slot(&m->hist, (2 * nk + 2 * (nk + 1) + 2 * nk) * sizeof(unsigned)), slot(&m->t_ref, rs * sizeof(double2)), slot(&m->t_est, es * sizeof(double2)),
            slot(&m->win, 2 * rs * sizeof(int2)), slot(&m->match, 2 * es * sizeof(int))};
}
extern "C" void ymt3_metrics_destroy(ymt3_metrics m) { destroy_object(m); }

extern "C" int ymt3_metrics_create(ymt3_handle h, const ymt3_metrics_params* params, long long max_ref, long long max_est, ymt3_metrics* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_metrics_params& p = *params;
    if (!std::isfinite(p.onset_tol) || p.onset_tol < 0) FAIL(YMT3_ERR_ARG, "onset_tol=%g must be finite and >= 0", p.onset_tol);
    if (!std::isfinite(p.offset_min_tol) || p.offset_min_tol < 0) FAIL(YMT3_ERR_ARG, "offset_min_tol=%g must be finite and >= 0", p.offset_min_tol);
    if (!std::isfinite(p.offset_ratio) || p.offset_ratio < 0) FAIL(YMT3_ERR_ARG, "offset_ratio=%g must be finite and >= 0", p.offset_ratio);
    if (const int rc = check_programs(p.n_programs, p.drum_program, METRICS_MAX_PROGRAMS, "")) return rc;
    if (max_ref < 1 || max_ref > METRICS_MAX_NOTES) FAIL(YMT3_ERR_ARG, "max_ref=%lld outside [1, %lld]", max_ref, METRICS_MAX_NOTES);
    if (max_est < 1 || max_est > METRICS_MAX_NOTES) FAIL(YMT3_ERR_ARG, "max_est=%lld outside [1, %lld]", max_est, METRICS_MAX_NOTES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_metrics m = new ymt3_metrics_s{h, handle_device(h), p, max_ref, max_est};
    return allocate_object(m, slots(m), "note metrics scratch", out);
}

extern "C" int ymt3_note_metrics(ymt3_handle h, ymt3_metrics m, const void* ref_notes_dev, long long n_ref, const int32_t* ref_count_dev,
                                 const void* est_notes_dev, long long n_est, const int32_t* est_count_dev, int32_t* counts_dev, void* stream) {
    if (const int rc = check_owner(h, m, "metrics object")) return rc;
    if (const int rc = check_count("n_ref", n_ref, m->max_ref, "max_ref")) return rc;
    if (const int rc = check_count("n_est", n_est, m->max_est, "max_est")) return rc;
    if (!counts_dev) FAIL(YMT3_ERR_ARG, "counts_dev is NULL");
    if (const int rc = check_record_ptr("ref_notes_dev", ref_notes_dev, n_ref)) return rc;
    if (const int rc = check_record_ptr("est_notes_dev", est_notes_dev, n_est)) return rc;
    HIP_TRY(hipSetDevice(m->device));
    const size_t nk = (size_t)(m->p.n_programs + 1) * METRICS_PITCHES;
    MetricsArgs a{};
    a.onset_tol = m->p.onset_tol; a.offset_min_tol = m->p.offset_min_tol; a.offset_ratio = m->p.offset_ratio;
    a.ref = static_cast<const DetokNote*>(ref_notes_dev); a.est = static_cast<const DetokNote*>(est_notes_dev);
    a.n_ref = n_ref; a.n_est = n_est; a.ref_count = n_ref ? ref_count_dev : nullptr; a.est_count = n_est ? est_count_dev : nullptr;
    a.max_ref = m->max_ref; a.max_est = m->max_est; a.t_ref = m->t_ref; a.t_est = m->t_est;
    a.hist = m->hist; a.off = m->hist + 2 * nk; a.cursor = a.off + 2 * (nk + 1);
    a.n_programs = m->p.n_programs; a.drum_program = m->p.drum_program; a.win = m->win; a.stack = m->win + 2 * (size_t)m->max_ref;
    a.match = m->match; a.visit = m->match + 2 * (size_t)m->max_est; a.counts = counts_dev;
    LAUNCH(launch_metrics(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- device piano roll and frame metrics (include/ymt3.h)
struct ymt3_roll_s {
    ymt3_handle owner;
    int device;
    ymt3_roll_params p;
    long long max_frames;
    uint4* bits = nullptr;                  // [2][n_programs + 1][max_frames] 128 pitch bits each
};

static std::vector<Slot> slots(ymt3_roll r) { return {slot(&r->bits, (size_t)2 * (r->p.n_programs + 1) * (size_t)r->max_frames * sizeof(uint4))}; }
extern "C" void ymt3_roll_destroy(ymt3_roll r) { destroy_object(r); }

extern "C" int ymt3_roll_create(ymt3_handle h, const ymt3_roll_params* params, long long max_frames, ymt3_roll* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_roll_params& p = *params;
    if (!std::isfinite(p.frames_per_second) || p.frames_per_second <= 0) FAIL(YMT3_ERR_ARG, "frames_per_second=%g must be finite and > 0", p.frames_per_second);
    if (const int rc = check_programs(p.n_programs, p.drum_program, ROLL_MAX_PROGRAMS, "")) return rc;
    if (max_frames < 1 || max_frames > ROLL_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "max_frames=%lld outside [1, %lld]", max_frames, ROLL_MAX_FRAMES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_roll r = new ymt3_roll_s{h, handle_device(h), p, max_frames};
    return allocate_object(r, slots(r), "piano roll scratch", out);
}

// the checks the two roll calls share, and the arguments they share
static int roll_args(ymt3_handle h, ymt3_roll r, long long n_frames, RollArgs* a) {
    if (const int rc = check_owner(h, r, "roll object")) return rc;
    if (n_frames < 0 || n_frames > r->max_frames) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [0, max_frames=%lld]", n_frames, r->max_frames);
    *a = RollArgs{};
    a->frames_per_second = r->p.frames_per_second; a->n_programs = r->p.n_programs; a->drum_program = r->p.drum_program;
    a->n_frames = n_frames; a->max_frames = r->max_frames; a->bits = r->bits;
    return YMT3_OK;
}

// one side of a roll or alignment call (RollArgs and AlignArgs name these three fields alike)
template <class Args>
static int set_side(Args* a, int side, const char* n_name, const char* ptr_name, const void* notes_dev, long long n, const int32_t* count_dev) {
    if (const int rc = check_count(n_name, n, ROLL_MAX_NOTES, nullptr)) return rc;
    if (const int rc = check_record_ptr(ptr_name, notes_dev, n)) return rc;
    a->notes[side] = static_cast<const DetokNote*>(notes_dev); a->n[side] = n; a->count[side] = n ? count_dev : nullptr;
    return YMT3_OK;
}

extern "C" int ymt3_piano_roll(ymt3_handle h, ymt3_roll r, const void* notes_dev, long long n_notes, const int32_t* count_dev, long long n_frames,
                               int first_row, int n_rows, uint8_t* roll_dev, void* stream) {
    RollArgs a;
    if (const int rc = roll_args(h, r, n_frames, &a)) return rc;
    if (const int rc = set_side(&a, 0, "n_notes", "notes_dev", notes_dev, n_notes, count_dev)) return rc;
    if (first_row < 0 || n_rows < 1 || (long long)first_row + n_rows > r->p.n_programs + 1)
        FAIL(YMT3_ERR_ARG, "rows [first_row=%d, first_row + n_rows=%lld) outside [0, n_programs + 1=%d]", first_row, (long long)first_row + n_rows, r->p.n_programs + 1);
    if (!roll_dev) FAIL(YMT3_ERR_ARG, "roll_dev is NULL");
    if (reinterpret_cast<uintptr_t>(roll_dev) % 16) FAIL(YMT3_ERR_ARG, "roll_dev is not aligned to 16 bytes");
    HIP_TRY(hipSetDevice(r->device));
    a.n_sides = 1; a.row0 = first_row; a.row_n = n_rows; a.roll = roll_dev;
    LAUNCH(launch_piano_roll(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

extern "C" int ymt3_frame_metrics(ymt3_handle h, ymt3_roll r, const void* ref_notes_dev, long long n_ref, const int32_t* ref_count_dev,
                                  const void* est_notes_dev, long long n_est, const int32_t* est_count_dev, long long n_frames, long long* counts_dev,
                                  void* stream) {
    RollArgs a;
    if (const int rc = roll_args(h, r, n_frames, &a)) return rc;
    if (const int rc = set_side(&a, 0, "n_ref", "ref_notes_dev", ref_notes_dev, n_ref, ref_count_dev)) return rc;
    if (const int rc = set_side(&a, 1, "n_est", "est_notes_dev", est_notes_dev, n_est, est_count_dev)) return rc;
    if (!counts_dev) FAIL(YMT3_ERR_ARG, "counts_dev is NULL");
    if (reinterpret_cast<uintptr_t>(counts_dev) % 8) FAIL(YMT3_ERR_ARG, "counts_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(r->device));
    a.n_sides = 2; a.row0 = 0; a.row_n = r->p.n_programs + 1; a.counts = counts_dev;
    LAUNCH(launch_frame_metrics(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- device alignment (include/ymt3.h)
struct ymt3_aligner_s {
    ymt3_handle owner;
    int device;
    ymt3_align_params p;
    long long max_frames, band;             // band = min(p.band_frames, max_frames)
    uint4* feat = nullptr;                  // [2][max_frames][2]
    int* edges = nullptr;                   // [align_edge_ints(max_frames)]
    unsigned* steps = nullptr;              // [max_frames][align_step_words(band)]
    int2* rpath = nullptr;                  // [2 * max_frames - 1]
};

static std::vector<Slot> slots(ymt3_aligner a) {
    return {slot(&a->feat, (size_t)2 * a->max_frames * 2 * sizeof(uint4)), slot(&a->edges, (size_t)align_edge_ints(a->max_frames) * sizeof(int)),
            slot(&a->steps, (size_t)a->max_frames * align_step_words(a->band) * sizeof(unsigned)), slot(&a->rpath, (size_t)(2 * a->max_frames - 1) * sizeof(int2))};
}
extern "C" void ymt3_aligner_destroy(ymt3_aligner a) { destroy_object(a); }

extern "C" int ymt3_aligner_create(ymt3_handle h, const ymt3_align_params* params, long long max_frames, ymt3_aligner* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_align_params& p = *params;
    if (!std::isfinite(p.frames_per_second) || p.frames_per_second <= 0) FAIL(YMT3_ERR_ARG, "frames_per_second=%g must be finite and > 0", p.frames_per_second);
    if (const int rc = check_programs(p.n_programs, p.drum_program, ROLL_MAX_PROGRAMS, "")) return rc;
    if (p.band_frames < 1) FAIL(YMT3_ERR_ARG, "band_frames=%d must be >= 1", p.band_frames);
    if (max_frames < 1 || max_frames > ALIGN_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "max_frames=%lld outside [1, %lld]", max_frames, ALIGN_MAX_FRAMES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_aligner a = new ymt3_aligner_s{h, handle_device(h), p, max_frames, std::min<long long>(p.band_frames, max_frames)};
    return allocate_object(a, slots(a), "alignment scratch", out);
}

extern "C" int ymt3_align_notes(ymt3_handle h, ymt3_aligner al, const void* ref_notes_dev, long long n_ref, const int32_t* ref_count_dev,
                                long long n_ref_frames, const void* est_notes_dev, long long n_est, const int32_t* est_count_dev,
                                long long n_est_frames, int32_t* warp_dev, int32_t* path_dev, long long* result_dev, void* stream) {
    if (const int rc = check_owner(h, al, "aligner object")) return rc;
    AlignArgs a{};
    a.frames_per_second = al->p.frames_per_second; a.n_programs = al->p.n_programs; a.drum_program = al->p.drum_program;
    a.band_frames = al->band; a.max_frames = al->max_frames; a.n_frames[0] = n_ref_frames; a.n_frames[1] = n_est_frames;
    if (n_ref_frames < 1 || n_ref_frames > a.max_frames) FAIL(YMT3_ERR_ARG, "n_ref_frames=%lld outside [1, max_frames=%lld]", n_ref_frames, a.max_frames);
    if (const int rc = set_side(&a, 0, "n_ref", "ref_notes_dev", ref_notes_dev, n_ref, ref_count_dev)) return rc;
    if (n_est_frames < 1 || n_est_frames > a.max_frames) FAIL(YMT3_ERR_ARG, "n_est_frames=%lld outside [1, max_frames=%lld]", n_est_frames, a.max_frames);
    if (const int rc = set_side(&a, 1, "n_est", "est_notes_dev", est_notes_dev, n_est, est_count_dev)) return rc;
    if (!warp_dev) FAIL(YMT3_ERR_ARG, "warp_dev is NULL");
    if (reinterpret_cast<uintptr_t>(warp_dev) % 4) FAIL(YMT3_ERR_ARG, "warp_dev is not aligned to 4 bytes");
    if (reinterpret_cast<uintptr_t>(path_dev) % 8) FAIL(YMT3_ERR_ARG, "path_dev is not aligned to 8 bytes");
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(al->device));
    a.feat = al->feat; a.edges = al->edges; a.steps = al->steps; a.rpath = al->rpath; a.warp = warp_dev; a.path = path_dev; a.result = result_dev;
    LAUNCH(launch_align(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

extern "C" int ymt3_warp_notes(ymt3_handle h, ymt3_aligner al, const void* notes_dev, long long n_notes, const int32_t* count_dev,
                               const int32_t* warp_dev, long long n_ref_frames, void* notes_out_dev, void* stream) {
    if (const int rc = check_owner(h, al, "aligner object")) return rc;
    if (n_ref_frames < 1 || n_ref_frames > al->max_frames) FAIL(YMT3_ERR_ARG, "n_ref_frames=%lld outside [1, max_frames=%lld]", n_ref_frames, al->max_frames);
    if (const int rc = check_count("n_notes", n_notes, ROLL_MAX_NOTES, nullptr)) return rc;
    if (!warp_dev) FAIL(YMT3_ERR_ARG, "warp_dev is NULL");
    if (reinterpret_cast<uintptr_t>(warp_dev) % 4) FAIL(YMT3_ERR_ARG, "warp_dev is not aligned to 4 bytes");
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (const int rc = check_record_ptr("notes_out_dev", notes_out_dev, n_notes)) return rc;
    HIP_TRY(hipSetDevice(al->device));
    WarpNotesArgs a{al->p.frames_per_second, static_cast<const DetokNote*>(notes_dev), static_cast<DetokNote*>(notes_out_dev), n_notes,
                    n_notes ? count_dev : nullptr, warp_dev, n_ref_frames};
    LAUNCH(launch_warp_notes(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- note velocities from the audio (include/ymt3.h)
struct ymt3_velocity_s {
    ymt3_handle owner;
    int device;
    ymt3_velocity_params p;
    double ref_energy;                      // 10^(peak_db / 10), or NaN: the class's peak
    float e_scale, p_scale;                 // 4 / (sum w)^2, 2 / sum w^2
    float* window = nullptr;                // [window_samples]
    uint32_t* steps = nullptr;              // [128][VELOCITY_MAX_HARMONICS]
};

static std::vector<Slot> slots(ymt3_velocity v, const float* window_host = nullptr, const uint32_t* steps_host = nullptr) {
    return {slot(&v->window, (size_t)v->p.window_samples * sizeof(float), window_host),
            slot(&v->steps, (size_t)NOTE_PITCHES * VELOCITY_MAX_HARMONICS * sizeof(uint32_t), steps_host)};
}
extern "C" void ymt3_velocity_destroy(ymt3_velocity v) { destroy_object(v); }

extern "C" int ymt3_velocity_create(ymt3_handle h, const ymt3_velocity_params* params, ymt3_velocity* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_velocity_params& p = *params;
    const ymt3_config& cfg = handle_config(h);
    if (p.sample_rate != cfg.sample_rate) FAIL(YMT3_ERR_ARG, "sample_rate=%d != the model's sample_rate=%d", p.sample_rate, cfg.sample_rate);
    if (p.window_samples < VELOCITY_MIN_WINDOW || p.window_samples > VELOCITY_MAX_WINDOW)
        FAIL(YMT3_ERR_ARG, "window_samples=%d outside [%d, %d]", p.window_samples, VELOCITY_MIN_WINDOW, VELOCITY_MAX_WINDOW);
    if (p.n_harmonics < 1 || p.n_harmonics > VELOCITY_MAX_HARMONICS) FAIL(YMT3_ERR_ARG, "n_harmonics=%d outside [1, %d]", p.n_harmonics, VELOCITY_MAX_HARMONICS);
    if (!std::isfinite(p.velocity_per_db) || p.velocity_per_db <= 0) FAIL(YMT3_ERR_ARG, "velocity_per_db=%g must be finite and > 0", p.velocity_per_db);
    if (p.peak_velocity < 1 || p.peak_velocity > 127) FAIL(YMT3_ERR_ARG, "peak_velocity=%d outside [1, 127]", p.peak_velocity);
    if (p.min_velocity < 1 || p.min_velocity > p.peak_velocity) FAIL(YMT3_ERR_ARG, "min_velocity=%d outside [1, peak_velocity=%d]", p.min_velocity, p.peak_velocity);
    if (p.default_velocity < 1 || p.default_velocity > 127) FAIL(YMT3_ERR_ARG, "default_velocity=%d outside [1, 127]", p.default_velocity);
    if (std::isinf(p.peak_db)) FAIL(YMT3_ERR_ARG, "peak_db=%g must be finite, or NaN for the loudest measured note", p.peak_db);
    if (p.drum_program < 0) FAIL(YMT3_ERR_ARG, "drum_program=%d must be >= 0", p.drum_program);
    // the two tables, in f64 as velocity_tables of yourmt3_amd/velocity.py builds them: the same libm calls, the sums in index order
    const int W = p.window_samples;
    const double sr = (double)p.sample_rate;
    std::vector<float> window(W);
    double sw = 0.0, sw2 = 0.0;
    for (int k = 0; k < W; ++k) {
        window[k] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (k + 0.5) / W));
        sw += (double)window[k];
        sw2 += (double)window[k] * (double)window[k];
    }
    std::vector<uint32_t> steps((size_t)NOTE_PITCHES * VELOCITY_MAX_HARMONICS, 0u);
    for (int pitch = 0; pitch < NOTE_PITCHES; ++pitch) {
        const double f = 440.0 * std::pow(2.0, (pitch - 69) / 12.0);
        for (int k = 1; k <= p.n_harmonics; ++k)
            if (k * f < sr / 2.0) steps[(size_t)pitch * VELOCITY_MAX_HARMONICS + k - 1] = (uint32_t)std::rint(k * f / sr * 4294967296.0);
    }
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_velocity v = new ymt3_velocity_s{h, handle_device(h), p, std::isnan(p.peak_db) ? (double)NAN : std::pow(10.0, p.peak_db / 10.0),
                                          (float)(4.0 / (sw * sw)), (float)(2.0 / sw2)};
    return allocate_object(v, slots(v, window.data(), steps.data()), "note velocity tables", out);
}

extern "C" int ymt3_note_velocities(ymt3_handle h, ymt3_velocity v, const float* audio_dev, long long n_audio, const void* notes_dev, long long n_notes,
                                    const int32_t* count_dev, uint8_t* velocity_dev, float* energy_dev, float* peaks_dev, int32_t* counts_dev, void* stream) {
    if (const int rc = check_owner(h, v, "note velocity object")) return rc;
    if (n_audio < 0) FAIL(YMT3_ERR_ARG, "n_audio=%lld must be >= 0", n_audio);
    if (n_audio && !audio_dev) FAIL(YMT3_ERR_ARG, "audio_dev is NULL");
    if (reinterpret_cast<uintptr_t>(audio_dev) % 4) FAIL(YMT3_ERR_ARG, "audio_dev is not aligned to 4 bytes");
    if (const int rc = check_count("n_notes", n_notes, VELOCITY_MAX_NOTES, nullptr)) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (n_notes && !velocity_dev) FAIL(YMT3_ERR_ARG, "velocity_dev is NULL");
    if (reinterpret_cast<uintptr_t>(energy_dev) % 4) FAIL(YMT3_ERR_ARG, "energy_dev is not aligned to 4 bytes");
    if (!peaks_dev) FAIL(YMT3_ERR_ARG, "peaks_dev is NULL");
    if (reinterpret_cast<uintptr_t>(peaks_dev) % 4) FAIL(YMT3_ERR_ARG, "peaks_dev is not aligned to 4 bytes");
    if (!counts_dev) FAIL(YMT3_ERR_ARG, "counts_dev is NULL");
    if (reinterpret_cast<uintptr_t>(counts_dev) % 4) FAIL(YMT3_ERR_ARG, "counts_dev is not aligned to 4 bytes");
    HIP_TRY(hipSetDevice(v->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(peaks_dev, 0, 2 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, 2 * sizeof(int32_t), s));
    if (!n_notes) return YMT3_OK;
    VelocityArgs a{};
    a.audio = audio_dev; a.n_audio = n_audio; a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = count_dev;
    a.window = v->window; a.steps = v->steps; a.W = v->p.window_samples; a.H = v->p.n_harmonics; a.drum_program = v->p.drum_program;
    a.sample_rate = (double)v->p.sample_rate; a.e_scale = v->e_scale; a.p_scale = v->p_scale;
    a.velocity_per_db = v->p.velocity_per_db; a.ref_energy = v->ref_energy;
    a.peak_velocity = v->p.peak_velocity; a.min_velocity = v->p.min_velocity; a.default_velocity = v->p.default_velocity;
    a.velocity = velocity_dev; a.energy = energy_dev; a.peaks = peaks_dev; a.counts = counts_dev;
    LAUNCH(launch_note_velocities(a, s));
    return YMT3_OK;
}

// ---------------------------------------------------------------- beat tracking over note records (include/ymt3.h)
struct ymt3_beats_s {
    ymt3_handle owner;
    int device;
    ymt3_beat_params p;
    long long max_frames;
    int lag_min, lag_max;
    int32_t* prior = nullptr;               // [nL]
    int32_t* pen = nullptr;                 // [nL][2 * lag_max + 1]
    unsigned* env = nullptr;                // [max_frames]
    unsigned short* smooth = nullptr;       // [max_frames]
    long long* tgram = nullptr;             // [beat_windows(max_frames)][nL]
    unsigned short* lag_back = nullptr;     // the same
    int32_t* lags = nullptr;                // [beat_windows(max_frames)]
    int32_t* back = nullptr;                // [max_frames]
    int32_t* rbeats = nullptr;              // [beat_max_beats(max_frames)]
};

static std::vector<Slot> slots(ymt3_beats b, const int32_t* prior_host = nullptr, const int32_t* pen_host = nullptr) {
    const size_t nL = (size_t)(b->lag_max - b->lag_min + 1), F = (size_t)b->max_frames, nW = (size_t)beat_windows(b->max_frames, b->p.hop_frames);
    return {slot(&b->prior, nL * sizeof(int32_t), prior_host), slot(&b->pen, nL * (2 * (size_t)b->lag_max + 1) * sizeof(int32_t), pen_host),
            slot(&b->env, F * sizeof(unsigned)), slot(&b->smooth, F * sizeof(unsigned short)), slot(&b->tgram, nW * nL * sizeof(long long)),
            slot(&b->lag_back, nW * nL * sizeof(unsigned short)), slot(&b->lags, nW * sizeof(int32_t)), slot(&b->back, F * sizeof(int32_t)),
            slot(&b->rbeats, (size_t)beat_max_beats(b->max_frames, b->lag_min) * sizeof(int32_t))};
}
extern "C" void ymt3_beats_destroy(ymt3_beats b) { destroy_object(b); }

extern "C" int ymt3_beats_create(ymt3_handle h, const ymt3_beat_params* params, long long max_frames, ymt3_beats* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_beat_params& p = *params;
    const struct { const char* name; double v; } positive[] = {{"frames_per_second", p.frames_per_second}, {"bpm_min", p.bpm_min}, {"bpm_max", p.bpm_max},
                                                               {"bpm_prior", p.bpm_prior}, {"prior_octaves", p.prior_octaves}, {"tightness", p.tightness}};
    for (const auto& q : positive)
        if (!std::isfinite(q.v) || q.v <= 0) FAIL(YMT3_ERR_ARG, "%s=%g must be finite and > 0", q.name, q.v);
    if (p.bpm_min > p.bpm_max) FAIL(YMT3_ERR_ARG, "bpm_min=%g above bpm_max=%g", p.bpm_min, p.bpm_max);
    if (p.tightness > 10000) FAIL(YMT3_ERR_ARG, "tightness=%g above 10000", p.tightness);
    const double lo = std::ceil(60.0 * p.frames_per_second / p.bpm_max), hi = std::floor(60.0 * p.frames_per_second / p.bpm_min);
    if (!(lo >= BEAT_MIN_LAG && lo <= hi && hi <= BEAT_MAX_LAG))
        FAIL(YMT3_ERR_ARG, "lag_min=%g, lag_max=%g (60 frames_per_second / bpm_max, / bpm_min) must satisfy %d <= lag_min <= lag_max <= %d", lo, hi, BEAT_MIN_LAG, BEAT_MAX_LAG);
    const int lag_min = (int)lo, lag_max = (int)hi;
    if (p.window_frames < 2 * lag_max || p.window_frames > BEAT_MAX_WINDOW)
        FAIL(YMT3_ERR_ARG, "window_frames=%d outside [2 * lag_max=%d, %d]", p.window_frames, 2 * lag_max, BEAT_MAX_WINDOW);
    if (p.hop_frames < 1 || p.hop_frames > p.window_frames) FAIL(YMT3_ERR_ARG, "hop_frames=%d outside [1, window_frames=%d]", p.hop_frames, p.window_frames);
    if (p.lag_step_max < 0 || p.lag_step_max > BEAT_MAX_LAG) FAIL(YMT3_ERR_ARG, "lag_step_max=%d outside [0, %d]", p.lag_step_max, BEAT_MAX_LAG);
    if (p.onset_cap < 1 || p.onset_cap > 255) FAIL(YMT3_ERR_ARG, "onset_cap=%d outside [1, 255]", p.onset_cap);
    if (const int rc = check_programs(p.n_programs, p.drum_program, BEAT_MAX_PROGRAMS, "")) return rc;
    if (max_frames < 1 || max_frames > BEAT_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "max_frames=%lld outside [1, %lld]", max_frames, BEAT_MAX_FRAMES);
    // the tempo path adds one T per window: nW * Wn * (4 cap)^2 * 65535 bounds every sum; in integers, as the
    // specification checks it: the first three factors stay below 2^52
    const unsigned long long s_max = 4ull * p.onset_cap, terms = (unsigned long long)beat_windows(max_frames, p.hop_frames) * p.window_frames * s_max * s_max;
    if (terms > (1ull << 62) / 65535ull)
        FAIL(YMT3_ERR_ARG, "max_frames=%lld with hop_frames=%d: the tempo path's sums could pass 2^62", max_frames, p.hop_frames);
    // the two tables, in f64 as beat_tables of yourmt3_amd/beats.py builds them: the same libm calls, element by element
    const int nL = lag_max - lag_min + 1, row = 2 * lag_max + 1;
    const double l0 = 60.0 * p.frames_per_second / p.bpm_prior;
    std::vector<int32_t> prior(nL), pen((size_t)nL * row, 0);
    for (int lag = lag_min; lag <= lag_max; ++lag) {
        const double z = std::log2(lag / l0) / p.prior_octaves;
        prior[lag - lag_min] = (int32_t)std::rint(65535.0 * std::exp(-0.5 * (z * z)));
        for (int d = (lag + 1) / 2; d <= 2 * lag; ++d) {
            const double g = std::log((double)d / lag);
            pen[(size_t)(lag - lag_min) * row + d] = (int32_t)std::rint(p.tightness * 1024.0 * (g * g));
        }
    }
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_beats b = new ymt3_beats_s{h, handle_device(h), p, max_frames, lag_min, lag_max};
    return allocate_object(b, slots(b, prior.data(), pen.data()), "beat tracker scratch", out);
}

extern "C" int ymt3_track_beats(ymt3_handle h, ymt3_beats b, const void* notes_dev, long long n_notes, const int32_t* count_dev, long long n_frames,
                                int32_t* beats_dev, long long max_beats, int32_t* tempo_dev, long long* result_dev, void* stream) {
    if (const int rc = check_owner(h, b, "beat tracker")) return rc;
    if (n_frames < 1 || n_frames > b->max_frames) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [1, max_frames=%lld]", n_frames, b->max_frames);
    if (const int rc = check_count("n_notes", n_notes, BEAT_MAX_NOTES, nullptr)) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (!beats_dev) FAIL(YMT3_ERR_ARG, "beats_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beats_dev) % 4) FAIL(YMT3_ERR_ARG, "beats_dev is not aligned to 4 bytes");
    const long long need = beat_max_beats(n_frames, b->lag_min);
    if (max_beats < need) FAIL(YMT3_ERR_ARG, "max_beats=%lld below n_frames / ceil(lag_min / 2) + 1 = %lld", max_beats, need);
    if (reinterpret_cast<uintptr_t>(tempo_dev) % 4) FAIL(YMT3_ERR_ARG, "tempo_dev is not aligned to 4 bytes");
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(b->device));
    BeatArgs a{};
    a.frames_per_second = b->p.frames_per_second; a.n_programs = b->p.n_programs; a.drum_program = b->p.drum_program;
    a.lag_min = b->lag_min; a.lag_max = b->lag_max; a.window = b->p.window_frames; a.hop = b->p.hop_frames; a.lag_step = b->p.lag_step_max;
    a.onset_cap = b->p.onset_cap;
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = n_notes ? count_dev : nullptr; a.n_frames = n_frames;
    a.prior = b->prior; a.pen = b->pen; a.env = b->env; a.smooth = b->smooth; a.tgram = b->tgram; a.lag_back = b->lag_back; a.lags = b->lags;
    a.back = b->back; a.rbeats = b->rbeats; a.beats = beats_dev; a.max_beats = max_beats; a.tempo = tempo_dev; a.result = result_dev;
    LAUNCH(launch_track_beats(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

extern "C" int ymt3_beat_positions(ymt3_handle h, ymt3_beats b, const int32_t* beats_dev, const long long* result_dev, const void* notes_dev,
                                   long long n_notes, const int32_t* count_dev, int divisions, int32_t* ticks_dev, void* stream) {
    if (const int rc = check_owner(h, b, "beat tracker")) return rc;
    if (divisions < 0 || (divisions && BEAT_TICKS_PER_BEAT % divisions)) FAIL(YMT3_ERR_ARG, "divisions=%d must be 0 or a divisor of %d", divisions, BEAT_TICKS_PER_BEAT);
    if (const int rc = check_count("n_notes", n_notes, BEAT_MAX_NOTES, nullptr)) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (!beats_dev) FAIL(YMT3_ERR_ARG, "beats_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beats_dev) % 4) FAIL(YMT3_ERR_ARG, "beats_dev is not aligned to 4 bytes");
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    if (n_notes && !ticks_dev) FAIL(YMT3_ERR_ARG, "ticks_dev is NULL");
    if (reinterpret_cast<uintptr_t>(ticks_dev) % 8) FAIL(YMT3_ERR_ARG, "ticks_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(b->device));
    BeatPositionArgs a{};
    a.frames_per_second = b->p.frames_per_second; a.n_programs = b->p.n_programs; a.drum_program = b->p.drum_program; a.divisions = divisions;
    a.beats = beats_dev; a.result = result_dev; a.max_beats = beat_max_beats(b->max_frames, b->lag_min);
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = n_notes ? count_dev : nullptr; a.ticks = ticks_dev;
    LAUNCH(launch_beat_positions(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- bars and key over note records and beats (include/ymt3.h)
struct ymt3_bars_s {
    ymt3_handle owner;
    int device;
    ymt3_bar_params p;
    long long max_beats, max_notes;
    unsigned* accent = nullptr;             // [max_beats]
    unsigned* chroma = nullptr;             // [max_beats][12]
    int32_t* salience = nullptr;            // [max_beats]
    unsigned short* choice = nullptr;       // [max_beats]
    unsigned long long* acc = nullptr;      // [BAR_ACC_WORDS]
};

static std::vector<Slot> slots(ymt3_bars b) {
    const size_t B = (size_t)b->max_beats;
    return {slot(&b->accent, B * sizeof(unsigned)), slot(&b->chroma, B * 12 * sizeof(unsigned)), slot(&b->salience, B * sizeof(int32_t)),
            slot(&b->choice, B * sizeof(unsigned short)), slot(&b->acc, BAR_ACC_WORDS * sizeof(unsigned long long))};
}
extern "C" void ymt3_bars_destroy(ymt3_bars b) { destroy_object(b); }

extern "C" int ymt3_bars_create(ymt3_handle h, const ymt3_bar_params* params, long long max_beats, long long max_notes, ymt3_bars* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_bar_params& p = *params;
    if (!std::isfinite(p.frames_per_second) || p.frames_per_second <= 0) FAIL(YMT3_ERR_ARG, "frames_per_second=%g must be finite and > 0", p.frames_per_second);
    if (p.n_metres < 1 || p.n_metres > BAR_MAX_METRES) FAIL(YMT3_ERR_ARG, "n_metres=%d outside [1, %d]", p.n_metres, BAR_MAX_METRES);
    for (int q = 0; q < p.n_metres; ++q) {
        if (p.metres[q] < BAR_MIN_METRE || p.metres[q] > BAR_MAX_METRE)
            FAIL(YMT3_ERR_ARG, "metres[%d]=%d outside [%d, %d]", q, p.metres[q], BAR_MIN_METRE, BAR_MAX_METRE);
        for (int r = 0; r < q; ++r)
            if (p.metres[r] == p.metres[q]) FAIL(YMT3_ERR_ARG, "metres[%d]=%d is given twice", q, p.metres[q]);
    }
    const struct { const char* name; int v, lo, hi; } ranged[] = {{"near_div", p.near_div, 2, 64}, {"accent_cap", p.accent_cap, 1, 255}, {"w_long", p.w_long, 0, 15},
                                                                  {"w_kick", p.w_kick, 0, 15}, {"w_accent", p.w_accent, 0, 1024}, {"switch_cost", p.switch_cost, 0, 4096}};
    for (const auto& q : ranged)
        if (q.v < q.lo || q.v > q.hi) FAIL(YMT3_ERR_ARG, "%s=%d outside [%d, %d]", q.name, q.v, q.lo, q.hi);
    if (p.kick_lo < 0 || p.kick_lo > p.kick_hi || p.kick_hi > 127)
        FAIL(YMT3_ERR_ARG, "kick_lo=%d, kick_hi=%d must satisfy 0 <= kick_lo <= kick_hi <= 127", p.kick_lo, p.kick_hi);
    if (const int rc = check_programs(p.n_programs, p.drum_program, BAR_MAX_PROGRAMS, "")) return rc;
    if (max_beats < 1 || max_beats > BAR_MAX_BEATS) FAIL(YMT3_ERR_ARG, "max_beats=%lld outside [1, %lld]", max_beats, BAR_MAX_BEATS);
    if (max_notes < 1 || max_notes > BAR_MAX_NOTES) FAIL(YMT3_ERR_ARG, "max_notes=%lld outside [1, %lld]", max_notes, BAR_MAX_NOTES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_bars b = new ymt3_bars_s{h, handle_device(h), p, max_beats, max_notes};
    return allocate_object(b, slots(b), "bar tracker scratch", out);
}

extern "C" int ymt3_track_bars(ymt3_handle h, ymt3_bars b, const int32_t* beats_dev, const long long* beat_result_dev, const void* notes_dev,
                               long long n_notes, const int32_t* count_dev, long long n_frames, int32_t* metre_dev, long long max_beats,
                               long long* result_dev, void* stream) {
    if (const int rc = check_owner(h, b, "bar tracker")) return rc;
    if (!beats_dev) FAIL(YMT3_ERR_ARG, "beats_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beats_dev) % 4) FAIL(YMT3_ERR_ARG, "beats_dev is not aligned to 4 bytes");
    if (!beat_result_dev) FAIL(YMT3_ERR_ARG, "beat_result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beat_result_dev) % 8) FAIL(YMT3_ERR_ARG, "beat_result_dev is not aligned to 8 bytes");
    if (const int rc = check_count("n_notes", n_notes, b->max_notes, "max_notes")) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (n_frames < 1 || n_frames > BAR_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [1, %lld]", n_frames, BAR_MAX_FRAMES);
    if (!metre_dev) FAIL(YMT3_ERR_ARG, "metre_dev is NULL");
    if (reinterpret_cast<uintptr_t>(metre_dev) % 4) FAIL(YMT3_ERR_ARG, "metre_dev is not aligned to 4 bytes");
    if (max_beats < b->max_beats) FAIL(YMT3_ERR_ARG, "max_beats=%lld below the bar tracker's max_beats=%lld", max_beats, b->max_beats);
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(b->device));
    BarArgs a{};
    a.frames_per_second = b->p.frames_per_second; a.n_programs = b->p.n_programs; a.drum_program = b->p.drum_program;
    a.n_metres = b->p.n_metres;
    for (int q = 0; q < BAR_MAX_METRES; ++q) a.metres[q] = q < b->p.n_metres ? b->p.metres[q] : 0;
    a.near_div = b->p.near_div; a.accent_cap = b->p.accent_cap; a.w_long = b->p.w_long; a.w_kick = b->p.w_kick; a.kick_lo = b->p.kick_lo;
    a.kick_hi = b->p.kick_hi; a.w_accent = b->p.w_accent; a.switch_cost = b->p.switch_cost;
    a.beats = beats_dev; a.beat_result = beat_result_dev; a.max_beats = b->max_beats;
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = n_notes ? count_dev : nullptr; a.n_frames = n_frames;
    a.accent = b->accent; a.chroma = b->chroma; a.salience = b->salience; a.choice = b->choice; a.acc = b->acc;
    a.metre = metre_dev; a.result = result_dev;
    LAUNCH(launch_track_bars(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- chords over note records and beats (include/ymt3.h)
struct ymt3_chords_s {
    ymt3_handle owner;
    int device;
    ymt3_chord_params p;
    long long max_beats, max_notes;
    unsigned* chroma = nullptr;             // [max_beats][12]
    unsigned* bass = nullptr;               // [max_beats]
    unsigned* back = nullptr;               // [max_beats][CHORD_BACK_WORDS]
};

static std::vector<Slot> slots(ymt3_chords c) {
    const size_t B = (size_t)c->max_beats;
    return {slot(&c->chroma, B * 12 * sizeof(unsigned)), slot(&c->bass, B * sizeof(unsigned)), slot(&c->back, B * CHORD_BACK_WORDS * sizeof(unsigned))};
}
extern "C" void ymt3_chords_destroy(ymt3_chords c) { destroy_object(c); }

extern "C" int ymt3_chords_create(ymt3_handle h, const ymt3_chord_params* params, long long max_beats, long long max_notes, ymt3_chords* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_chord_params& p = *params;
    if (!std::isfinite(p.frames_per_second) || p.frames_per_second <= 0) FAIL(YMT3_ERR_ARG, "frames_per_second=%g must be finite and > 0", p.frames_per_second);
    if (p.n_qualities < 1 || p.n_qualities > CHORD_QUALITIES) FAIL(YMT3_ERR_ARG, "n_qualities=%d outside [1, %d]", p.n_qualities, CHORD_QUALITIES);
    for (int q = 0; q < p.n_qualities; ++q) {
        if (p.qualities[q] < 0 || p.qualities[q] >= CHORD_QUALITIES) FAIL(YMT3_ERR_ARG, "qualities[%d]=%d outside [0, %d)", q, p.qualities[q], CHORD_QUALITIES);
        for (int r = 0; r < q; ++r)
            if (p.qualities[r] == p.qualities[q]) FAIL(YMT3_ERR_ARG, "qualities[%d]=%d is given twice", q, p.qualities[q]);
    }
    const struct { const char* name; int v, lo, hi; } ranged[] = {{"near_div", p.near_div, 2, 64}, {"bass_div", p.bass_div, 1, 64}, {"w_bass", p.w_bass, 0, 1024},
                                                                  {"w_none", p.w_none, 0, 1024}, {"change_cost", p.change_cost, 0, 4096},
                                                                  {"change_cost_down", p.change_cost_down, 0, 4096}};
    for (const auto& q : ranged)
        if (q.v < q.lo || q.v > q.hi) FAIL(YMT3_ERR_ARG, "%s=%d outside [%d, %d]", q.name, q.v, q.lo, q.hi);
    if (const int rc = check_programs(p.n_programs, p.drum_program, BAR_MAX_PROGRAMS, "")) return rc;
    if (max_beats < 1 || max_beats > BAR_MAX_BEATS) FAIL(YMT3_ERR_ARG, "max_beats=%lld outside [1, %lld]", max_beats, BAR_MAX_BEATS);
    if (max_notes < 1 || max_notes > BAR_MAX_NOTES) FAIL(YMT3_ERR_ARG, "max_notes=%lld outside [1, %lld]", max_notes, BAR_MAX_NOTES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_chords c = new ymt3_chords_s{h, handle_device(h), p, max_beats, max_notes};
    return allocate_object(c, slots(c), "chord tracker scratch", out);
}

extern "C" int ymt3_track_chords(ymt3_handle h, ymt3_chords c, const int32_t* beats_dev, const long long* beat_result_dev, const int32_t* metre_dev,
                                 const void* notes_dev, long long n_notes, const int32_t* count_dev, long long n_frames, int32_t* chord_dev,
                                 long long chord_cap, long long* result_dev, void* stream) {
    if (const int rc = check_owner(h, c, "chord tracker")) return rc;
    if (!beats_dev) FAIL(YMT3_ERR_ARG, "beats_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beats_dev) % 4) FAIL(YMT3_ERR_ARG, "beats_dev is not aligned to 4 bytes");
    if (!beat_result_dev) FAIL(YMT3_ERR_ARG, "beat_result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beat_result_dev) % 8) FAIL(YMT3_ERR_ARG, "beat_result_dev is not aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(metre_dev) % 4) FAIL(YMT3_ERR_ARG, "metre_dev is not aligned to 4 bytes");
    if (const int rc = check_count("n_notes", n_notes, c->max_notes, "max_notes")) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (n_frames < 1 || n_frames > BAR_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [1, %lld]", n_frames, BAR_MAX_FRAMES);
    if (!chord_dev) FAIL(YMT3_ERR_ARG, "chord_dev is NULL");
    if (reinterpret_cast<uintptr_t>(chord_dev) % 4) FAIL(YMT3_ERR_ARG, "chord_dev is not aligned to 4 bytes");
    if (chord_cap < c->max_beats) FAIL(YMT3_ERR_ARG, "chord_cap=%lld below the chord tracker's max_beats=%lld", chord_cap, c->max_beats);
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(c->device));
    ChordArgs a{};
    a.frames_per_second = c->p.frames_per_second; a.n_programs = c->p.n_programs; a.drum_program = c->p.drum_program;
    a.n_qualities = c->p.n_qualities;
    for (int q = 0; q < CHORD_QUALITIES; ++q) a.qualities[q] = q < c->p.n_qualities ? c->p.qualities[q] : -1;
    a.near_div = c->p.near_div; a.bass_div = c->p.bass_div; a.w_bass = c->p.w_bass; a.w_none = c->p.w_none; a.change_cost = c->p.change_cost;
    a.change_cost_down = c->p.change_cost_down;
    a.beats = beats_dev; a.beat_result = beat_result_dev; a.max_beats = c->max_beats; a.metre = metre_dev;
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = n_notes ? count_dev : nullptr; a.n_frames = n_frames;
    a.chroma = c->chroma; a.bass = c->bass; a.back = c->back;
    a.chord = chord_dev; a.result = result_dev;
    LAUNCH(launch_track_chords(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- sections over note records and beats (include/ymt3.h)
struct ymt3_sections_s {
    ymt3_handle owner;
    int device;
    ymt3_section_params p;
    long long max_beats, max_notes;
    unsigned* chroma = nullptr;             // [max_beats][12]
    unsigned short* f = nullptr;            // [max_beats][SECTION_F_WORDS]
    long long* nov = nullptr;               // [max_beats]
    unsigned char* peak = nullptr;          // [max_beats]
    unsigned long long* acc = nullptr;      // [SECTION_ACC_WORDS]
    int32_t* starts = nullptr;              // [SECTION_MAX_SECTIONS + 2]
    unsigned char* same = nullptr;          // [SECTION_MAX_SECTIONS][SECTION_MAX_SECTIONS]
};

static std::vector<Slot> slots(ymt3_sections c) {
    const size_t B = (size_t)c->max_beats;
    return {slot(&c->chroma, B * 12 * sizeof(unsigned)), slot(&c->f, B * SECTION_F_WORDS * sizeof(unsigned short)), slot(&c->nov, B * sizeof(long long)),
            slot(&c->peak, B), slot(&c->acc, SECTION_ACC_WORDS * sizeof(unsigned long long)),
            slot(&c->starts, (SECTION_MAX_SECTIONS + 2) * sizeof(int32_t), nullptr, true),
            slot(&c->same, (size_t)SECTION_MAX_SECTIONS * SECTION_MAX_SECTIONS, nullptr, true)};
}
extern "C" void ymt3_sections_destroy(ymt3_sections c) { destroy_object(c); }

extern "C" int ymt3_sections_create(ymt3_handle h, const ymt3_section_params* params, long long max_beats, long long max_notes, ymt3_sections* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_section_params& p = *params;
    if (!std::isfinite(p.frames_per_second) || p.frames_per_second <= 0) FAIL(YMT3_ERR_ARG, "frames_per_second=%g must be finite and > 0", p.frames_per_second);
    const struct { const char* name; int v, lo, hi; } ranged[] = {{"near_div", p.near_div, 2, 64}, {"context", p.context, 1, SECTION_MAX_CONTEXT},
                                                                  {"kernel_beats", p.kernel_beats, 2, SECTION_MAX_KERNEL},
                                                                  {"min_len", p.min_len, 1, SECTION_MAX_MIN_LEN}, {"peak_div", p.peak_div, 1, 1024},
                                                                  {"same_dist", p.same_dist, 0, 32768}, {"len_num", p.len_num, 1, 16},
                                                                  {"max_sections", p.max_sections, 1, SECTION_MAX_SECTIONS}};
    for (const auto& q : ranged)
        if (q.v < q.lo || q.v > q.hi) FAIL(YMT3_ERR_ARG, "%s=%d outside [%d, %d]", q.name, q.v, q.lo, q.hi);
    if (const int rc = check_programs(p.n_programs, p.drum_program, BAR_MAX_PROGRAMS, "")) return rc;
    if (max_beats < 1 || max_beats > BAR_MAX_BEATS) FAIL(YMT3_ERR_ARG, "max_beats=%lld outside [1, %lld]", max_beats, BAR_MAX_BEATS);
    if (max_notes < 1 || max_notes > BAR_MAX_NOTES) FAIL(YMT3_ERR_ARG, "max_notes=%lld outside [1, %lld]", max_notes, BAR_MAX_NOTES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    ymt3_sections c = new ymt3_sections_s{h, handle_device(h), p, max_beats, max_notes};
    return allocate_object(c, slots(c), "section tracker scratch", out);
}

extern "C" int ymt3_track_sections(ymt3_handle h, ymt3_sections c, const int32_t* beats_dev, const long long* beat_result_dev, const int32_t* metre_dev,
                                   const void* notes_dev, long long n_notes, const int32_t* count_dev, long long n_frames, int32_t* section_dev,
                                   long long section_cap, long long* novelty_dev, long long* result_dev, void* stream) {
    if (const int rc = check_owner(h, c, "section tracker")) return rc;
    if (!beats_dev) FAIL(YMT3_ERR_ARG, "beats_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beats_dev) % 4) FAIL(YMT3_ERR_ARG, "beats_dev is not aligned to 4 bytes");
    if (!beat_result_dev) FAIL(YMT3_ERR_ARG, "beat_result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(beat_result_dev) % 8) FAIL(YMT3_ERR_ARG, "beat_result_dev is not aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(metre_dev) % 4) FAIL(YMT3_ERR_ARG, "metre_dev is not aligned to 4 bytes");
    if (const int rc = check_count("n_notes", n_notes, c->max_notes, "max_notes")) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (n_frames < 1 || n_frames > BAR_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [1, %lld]", n_frames, BAR_MAX_FRAMES);
    if (!section_dev) FAIL(YMT3_ERR_ARG, "section_dev is NULL");
    if (reinterpret_cast<uintptr_t>(section_dev) % 4) FAIL(YMT3_ERR_ARG, "section_dev is not aligned to 4 bytes");
    if (section_cap < c->max_beats) FAIL(YMT3_ERR_ARG, "section_cap=%lld below the section tracker's max_beats=%lld", section_cap, c->max_beats);
    if (reinterpret_cast<uintptr_t>(novelty_dev) % 8) FAIL(YMT3_ERR_ARG, "novelty_dev is not aligned to 8 bytes");
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(c->device));
    SectionArgs a{};
    a.frames_per_second = c->p.frames_per_second; a.n_programs = c->p.n_programs; a.drum_program = c->p.drum_program;
    a.near_div = c->p.near_div; a.context = c->p.context; a.kernel_beats = c->p.kernel_beats; a.min_len = c->p.min_len; a.peak_div = c->p.peak_div;
    a.same_dist = c->p.same_dist; a.len_num = c->p.len_num; a.max_sections = c->p.max_sections;
    a.beats = beats_dev; a.beat_result = beat_result_dev; a.max_beats = c->max_beats; a.metre = metre_dev;
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = n_notes ? count_dev : nullptr; a.n_frames = n_frames;
    a.chroma = c->chroma; a.f = c->f; a.nov = c->nov; a.peak = c->peak; a.acc = c->acc; a.starts = c->starts; a.same = c->same;
    a.section = section_dev; a.novelty = novelty_dev; a.result = result_dev;
    LAUNCH(launch_track_sections(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}

// ---------------------------------------------------------------- hands over note records (include/ymt3.h)
struct ymt3_hands_s {
    ymt3_handle owner;
    int device;
    ymt3_hand_params p;
    long long max_frames, max_notes, slots, max_slices;     // slots = hand_slots(max_frames); max_slices = min(max_notes, slots)
    uint4* sets = nullptr;                  // [slots]
    int32_t* slice_of = nullptr;            // [slots]
    uint4* cset = nullptr;                  // [max_slices]
    int32_t* slot_of = nullptr;             // [max_slices]
    unsigned char* back = nullptr;          // [max_slices][HAND_BACK_ROW]
    unsigned char* cut = nullptr;           // [max_slices]
    unsigned long long* acc = nullptr;      // [HAND_ACC_WORDS]
};

static std::vector<Slot> slots(ymt3_hands c) {
    const size_t S = (size_t)c->slots, T = (size_t)c->max_slices;
    return {slot(&c->sets, S * sizeof(uint4)), slot(&c->slice_of, S * sizeof(int32_t)), slot(&c->cset, T * sizeof(uint4)),
            slot(&c->slot_of, T * sizeof(int32_t)), slot(&c->back, T * HAND_BACK_ROW), slot(&c->cut, T),
            slot(&c->acc, HAND_ACC_WORDS * sizeof(unsigned long long))};
}
extern "C" void ymt3_hands_destroy(ymt3_hands c) { destroy_object(c); }

extern "C" int ymt3_hands_create(ymt3_handle h, const ymt3_hand_params* params, long long max_frames, long long max_notes, ymt3_hands* out) {
    if (const int rc = create_prologue(reinterpret_cast<void**>(out), h, params, "params")) return rc;
    const ymt3_hand_params& p = *params;
    if (!std::isfinite(p.frames_per_second) || p.frames_per_second <= 0) FAIL(YMT3_ERR_ARG, "frames_per_second=%g must be finite and > 0", p.frames_per_second);
    const struct { const char* name; int v, lo, hi; } ranged[] = {
        {"slice_frames", p.slice_frames, 1, HAND_MAX_SLICE_FRAMES}, {"span", p.span, 1, 127}, {"w_span", p.w_span, 0, HAND_MAX_WEIGHT}, {"cut_min", p.cut_min, 0, 127},
        {"w_cut", p.w_cut, 0, HAND_MAX_WEIGHT}, {"w_centre", p.w_centre, 0, HAND_MAX_WEIGHT}, {"middle", p.middle, 0, 128}, {"mid_free", p.mid_free, 0, 128},
        {"w_mid", p.w_mid, 0, HAND_MAX_WEIGHT}, {"w_move", p.w_move, 0, HAND_MAX_WEIGHT}, {"w_switch", p.w_switch, 0, HAND_MAX_WEIGHT},
        {"rest_slots", p.rest_slots, 1, (int)HAND_MAX_REST}};
    for (const auto& q : ranged)
        if (q.v < q.lo || q.v > q.hi) FAIL(YMT3_ERR_ARG, "%s=%d outside [%d, %d]", q.name, q.v, q.lo, q.hi);
    if (const int rc = check_programs(p.n_programs, p.drum_program, BAR_MAX_PROGRAMS, "")) return rc;
    if (p.program_lo < 0 || p.program_lo > p.program_hi || p.program_hi >= p.n_programs)
        FAIL(YMT3_ERR_ARG, "program_lo=%d, program_hi=%d must satisfy 0 <= program_lo <= program_hi < n_programs=%d", p.program_lo, p.program_hi, p.n_programs);
    if (max_frames < 1 || max_frames > BAR_MAX_FRAMES) FAIL(YMT3_ERR_ARG, "max_frames=%lld outside [1, %lld]", max_frames, BAR_MAX_FRAMES);
    if (max_notes < 1 || max_notes > BAR_MAX_NOTES) FAIL(YMT3_ERR_ARG, "max_notes=%lld outside [1, %lld]", max_notes, BAR_MAX_NOTES);
    HIP_TRY(hipSetDevice(handle_device(h)));
    const long long n_slots = hand_slots(max_frames, p.slice_frames);
    ymt3_hands c = new ymt3_hands_s{h, handle_device(h), p, max_frames, max_notes, n_slots, std::min(max_notes, n_slots)};
    return allocate_object(c, slots(c), "hand splitter scratch", out);
}

extern "C" int ymt3_split_hands(ymt3_handle h, ymt3_hands c, const void* notes_dev, long long n_notes, const int32_t* count_dev, long long n_frames,
                                uint8_t* hand_dev, int32_t* split_dev, long long max_slices, long long* result_dev, void* stream) {
    if (const int rc = check_owner(h, c, "hand splitter")) return rc;
    if (const int rc = check_count("n_notes", n_notes, c->max_notes, "max_notes")) return rc;
    if (const int rc = check_record_ptr("notes_dev", notes_dev, n_notes)) return rc;
    if (reinterpret_cast<uintptr_t>(count_dev) % 4) FAIL(YMT3_ERR_ARG, "count_dev is not aligned to 4 bytes");
    if (n_frames < 1 || n_frames > c->max_frames) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [1, max_frames=%lld]", n_frames, c->max_frames);
    if (n_notes && !hand_dev) FAIL(YMT3_ERR_ARG, "hand_dev is NULL");
    if (reinterpret_cast<uintptr_t>(split_dev) % 4) FAIL(YMT3_ERR_ARG, "split_dev is not aligned to 4 bytes");
    const long long n_slots = hand_slots(n_frames, c->p.slice_frames), need = std::min(n_notes, n_slots);
    if (split_dev && max_slices < need) FAIL(YMT3_ERR_ARG, "max_slices=%lld below min(n_notes, ceil(n_frames / slice_frames)) = %lld", max_slices, need);
    if (!result_dev) FAIL(YMT3_ERR_ARG, "result_dev is NULL");
    if (reinterpret_cast<uintptr_t>(result_dev) % 8) FAIL(YMT3_ERR_ARG, "result_dev is not aligned to 8 bytes");
    HIP_TRY(hipSetDevice(c->device));
    HandArgs a{};
    a.frames_per_second = c->p.frames_per_second; a.n_programs = c->p.n_programs; a.drum_program = c->p.drum_program;
    a.slice_frames = c->p.slice_frames; a.program_lo = c->p.program_lo; a.program_hi = c->p.program_hi; a.span = c->p.span; a.w_span = c->p.w_span;
    a.cut_min = c->p.cut_min; a.w_cut = c->p.w_cut; a.w_centre = c->p.w_centre; a.middle = c->p.middle; a.mid_free = c->p.mid_free; a.w_mid = c->p.w_mid;
    a.w_move = c->p.w_move; a.w_switch = c->p.w_switch; a.rest_slots = c->p.rest_slots;
    a.notes = static_cast<const DetokNote*>(notes_dev); a.n = n_notes; a.count = n_notes ? count_dev : nullptr; a.n_frames = n_frames;
    a.n_slots = n_slots; a.max_slices = c->max_slices;
    a.sets = c->sets; a.slice_of = c->slice_of; a.cset = c->cset; a.slot_of = c->slot_of; a.back = c->back; a.cut = c->cut; a.acc = c->acc;
    a.hand = hand_dev; a.split = split_dev; a.result = result_dev;
    LAUNCH(launch_split_hands(a, static_cast<hipStream_t>(stream)));
    return YMT3_OK;
}
