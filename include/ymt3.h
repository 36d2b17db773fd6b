/*
 * ymt3.h -- C ABI of the MI355X (gfx950) audio -> MIDI-token hot path.
 *
 * Drop-in boundary.  The reference checkout holds no source
 * (/root/reference = README.md:1-13 + LICENSE), so no reference file:line can be cited for
 * the interface each entry point replaces; the names `transcribe()` / `TaskManager` /
 * `inference_file()` come from BASELINE.json `north_star` and SURVEY.md section 9 (unverified
 * recollection of upstream `model/ymt3.py::inference_file(bsz, audio_segments)`).  The entry
 * points below are what a ctypes / cffi / pybind stub on that Python path would bind:
 *
 *   inference_file(bsz, audio_segments)  ->  ymt3_transcribe_segments()
 *   spectrogram module forward           ->  ymt3_logmel()
 *   encoder forward                      ->  ymt3_encode()
 *   decoder generate (greedy, KV cache)  ->  ymt3_decode_greedy()
 *   inference(x, task_tokens, ...)       ->  ymt3_transcribe_segments_prompted() / ymt3_decode_prompted()
 *   generate(output_scores=True) + compute_transition_scores(normalize_logits=True)
 *                                        ->  ymt3_transcribe_segments_scored() / ymt3_decode_scored()
 *   generate(prefix_allowed_tokens_fn=...)  ->  ymt3_transcribe_segments_constrained() / ymt3_decode_constrained()
 *   forward(labels=...) (teacher-forced log-likelihood)  ->  ymt3_transcribe_segments_score() / ymt3_score_tokens()
 *   generate(num_beams=W, num_return_sequences=N, length_penalty=alpha, early_stopping=True)
 *                                        ->  ymt3_transcribe_segments_beam() / ymt3_decode_beam()
 *
 * Conventions
 *   - every pointer named *_dev is DEVICE memory on the handle's GPU, owned by the caller;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all calls are
 *     asynchronous with respect to the host and never synchronise the device.  Exceptions, all documented at their
 *     declarations: ymt3_transcribe_stream, ymt3_set_early_stop (opt-in), the ymt3_profile_decode / ymt3_debug_* measurement
 *     hooks, and -- on by default, ymt3_set_abort_recovery(h, 0) turns it off -- the one wait at the END of a decode call
 *     that ran the merged decode kernels of the 64-row regime (after its last step has been queued; nothing is
 *     launched behind it unless a kernel gave up);
 *   - the library owns weights, KV caches and scratch inside the handle; nothing is
 *     allocated after ymt3_create() except by ymt3_constraint_create() (the caller's automaton tables) and
 *     ymt3_detok_create() (the device detokeniser's scratch), ymt3_tok_create() (the device tokeniser's) and
 *     ymt3_metrics_create() (the note metrics') and ymt3_roll_create() (the piano roll's) and ymt3_ingest_stream_create() (the
 *     streaming ingest's history) and ymt3_detok_state_create() (the incremental detokeniser's state) and ymt3_velocity_create() (the note
 *     velocities' two tables);
 *   - return value: 0 = ok, non-zero = error; the message is in ymt3_last_error()
 *     (thread local).  No exception ever crosses this boundary;
 *   - one handle per device per host thread.  No internal host threads.
 */
#ifndef YMT3_H
#define YMT3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YMT3_ABI_VERSION 3

enum { YMT3_OK = 0, YMT3_ERR_ARG = 1, YMT3_ERR_BLOB = 2, YMT3_ERR_HIP = 3, YMT3_ERR_UNSUPPORTED = 4 };
enum { YMT3_ENC_T5 = 0, YMT3_ENC_PERCEIVER_TF = 1 };
enum { YMT3_FFN_DENSE = 0, YMT3_FFN_MOE = 1 };

/* Field order mirrors yourmt3_amd/config.py::CConfig. */
typedef struct ymt3_config {
    int32_t sample_rate, segment_samples, n_fft, hop, n_mels;
    float   f_min, f_max, log_floor;
    int32_t d_model, d_ff, n_heads, d_kv, n_enc_layers, n_dec_layers;
    int32_t vocab, rel_buckets, rel_max_distance;
    float   ln_eps;
    int32_t max_decode_len, n_channels, eos_id, pad_id;
    int32_t encoder_type, n_latents;
    int32_t dec_ffn, n_experts, moe_top_k, moe_fp8;
    int32_t ptf_d, ptf_blocks, ptf_dff;   /* Perceiver-TF encoder: token width (multiple of 64), blocks, FFN width; n_latents = latents per frame */
    int32_t max_batch;              /* segments per call the workspace is sized for */
} ymt3_config;

typedef struct ymt3_ctx* ymt3_handle;

int         ymt3_abi_version(void);
const char* ymt3_last_error(void);

/* Parse the weight blob (format: yourmt3_amd/weights.py), upload it to `device`, derive the
 * window / twiddle / mel / relative-position tables, allocate caches and scratch.
 * Shapes the kernels run, checked here (YMT3_ERR_UNSUPPORTED, the message names the field; nothing
 * accepted here is refused later by a launch):
 *   d_model 512, n_heads * d_kv = 8 * 64; vocab % 16 == 0; 0..64 encoder and 1..64 decoder layers;
 *   n_fft 512 or 2048; n_mels % 64 == 0; hop even and <= 256;
 *   n_frames = 1 + segment_samples / hop: 64, 128, 256 or 512 (Perceiver-TF: 64, 128 or 256);
 *   dense FFN: d_ff 512, 1024 or 2048; MoE FFN: d_ff 2048, 2..16 experts, top-2;
 *   Perceiver-TF: ptf_d 128 or 256, n_latents 32 or 64, n_mels 64, 128 or 256. */
int  ymt3_create(const ymt3_config* cfg, const void* blob_host, size_t blob_bytes, int device, ymt3_handle* out);
void ymt3_destroy(ymt3_handle h);

/* Bytes of device memory held by the handle (weights + caches + scratch). */
size_t ymt3_device_bytes(ymt3_handle h);

/* The step before the path: interleaved PCM on the device, (n_frames, n_channels)
 * int16 or f32 at any integer sample rate -> mono mix -> polyphase Kaiser-windowed-sinc resample to cfg.sample_rate
 * (the filter and alignment of scipy.signal.resample_poly) -> (n_segments, segment_samples) f32, zero padded: the
 * buffer ymt3_logmel / ymt3_transcribe_segments read.  ymt3_ingest_plan is host arithmetic only (how many samples
 * and segments n_frames become).  The first ymt3_ingest call for a new rate pair designs the filter and uploads
 * <= 2 MB synchronously (rate pairs whose reduced ratio exceeds 16384 are rejected); later calls allocate nothing and are asynchronous on `stream`. */
#define YMT3_PCM_S16 0
#define YMT3_PCM_F32 1
int ymt3_ingest_plan(ymt3_handle h, int64_t n_frames, int sample_rate_in, int64_t* n_samples_out, int* n_segments);
int ymt3_ingest(ymt3_handle h, const void* pcm_dev, int pcm_format, int64_t n_frames, int n_channels,
                int sample_rate_in, float* segments_dev, int n_segments, void* stream);

/* Streaming ingest: ymt3_ingest for PCM that arrives in chunks (YourMT3.compile_ingest_stream).  Take the rows that every
 * ymt3_ingest_stream_push and then ymt3_ingest_stream_finish write to segments_dev, in order: concatenated they are the (n_segments,
 * segment_samples) buffer ymt3_ingest writes for the concatenated PCM, BIT FOR BIT for finite PCM and for every way of cutting the PCM
 * into chunks (both forms mix a frame and sum a tap row with the same device functions of yourmt3_amd/csrc/ingest.hip).
 *   - finality: output sample n reads input frames k0(n) - J + 1 .. k0(n) with k0(n) = floor((n + r) * down / up) (up / down the reduced
 *     rate ratio, J the taps per phase, r the alignment of resample_poly), so once N frames have arrived exactly
 *     F(N) = max(0, ceil(N * up / down) - r) samples are final.  A push computes the samples that became final, keeps them in a partial
 *     segment inside the object, and writes to the caller only WHOLE segments: floor(F(N) / segment_samples) minus those already
 *     written.  The last r samples, and the zero padding of the last segment, come from ymt3_ingest_stream_finish, which takes the
 *     frames that never arrived as zeros: what ymt3_ingest computes.  A stream of zero frames finishes with one all-zero segment.
 *   - n_ready (may be NULL) is the number of rows the call wrote; it is host arithmetic on the frame counts (ymt3_ingest_stream_plan
 *     gives it for a push of n_frames without doing anything), so nothing is synchronised to learn it.  n_samples_total (may be NULL)
 *     is ymt3_ingest_plan's n_samples_out for all the frames pushed.
 *   - state: a ring of mono frames (every frame is mixed once, when it arrives; J - 1 + max_chunk_frames frames rounded up to a power
 *     of two) and two partial-segment buffers.  Allocated by ymt3_ingest_stream_create, which is synchronous and, for a new rate pair,
 *     designs the filter as the first ymt3_ingest call does.  The ring costs 4 bytes per frame of J - 1 + max_chunk_frames rounded up to a
 *     power of two -- up to twice that, 128 MB at the cap of 2^24 frames -- so size max_chunk_frames by the chunks that really arrive
 *     (100 ms at 48 kHz: 4800 frames, a 32 KB ring); rate pairs ymt3_ingest refuses are refused here with the same code.
 *     push / finish / reset allocate nothing and are asynchronous on `stream`: a push is two launches (mix, resample), a finish one.
 *     The calls of one object must be ordered on the device as they are on the host (one stream, or the caller's own events).
 *   - non-finite PCM: a zero-padding tap is multiplied by a clamped window sample in both forms, so a non-finite frame can reach
 *     a different few outputs in the neighbourhood of its own under a different workgroup alignment.  Guaranteed: every output
 *     whose input frames k0(n) - J + 1 .. k0(n) all lie more than W = floor(255 * down / up) + J + 2 frames (the kernels' LDS window) from
 *     every non-finite frame equals ymt3_ingest's, bit for bit.
 *   - YMT3_ERR_ARG, with object and handle still usable and the stream's state unchanged: n_frames < 0 or > max_chunk_frames,
 *     max_segments below the rows the call writes, a push, plan or finish after ymt3_ingest_stream_finish without a
 *     ymt3_ingest_stream_reset, a NULL pcm_dev with n_frames > 0, a NULL segments_dev when the call writes a row; at create
 *     max_chunk_frames outside [1, 2^24], n_channels outside [1, 64], an unknown pcm_format.
 * The object belongs to h; ymt3_ingest_stream_destroy frees it (NULL is a no-op), before or after the handle's destruction.
 * ymt3_ingest_stream_reset starts a new stream on the same object.  The handle's decode state is left alone. */
typedef struct ymt3_ingest_stream_s* ymt3_ingest_stream;
int  ymt3_ingest_stream_create(ymt3_handle h, int sample_rate_in, int n_channels, int pcm_format, int64_t max_chunk_frames,
                               ymt3_ingest_stream* out);
void ymt3_ingest_stream_destroy(ymt3_ingest_stream s);
int  ymt3_ingest_stream_reset(ymt3_handle h, ymt3_ingest_stream s, void* stream);
int  ymt3_ingest_stream_plan(ymt3_ingest_stream s, int64_t n_frames, int* n_ready);
int  ymt3_ingest_stream_push(ymt3_handle h, ymt3_ingest_stream s, const void* pcm_dev, int64_t n_frames, float* segments_dev,
                             int max_segments, int* n_ready, void* stream);
int  ymt3_ingest_stream_finish(ymt3_handle h, ymt3_ingest_stream s, float* segments_dev, int max_segments, int* n_ready,
                               int64_t* n_samples_total, void* stream);

/* a1+a2: audio (B, segment_samples) f32 -> log-mel (B, n_frames, n_mels) f32. */
int ymt3_logmel(ymt3_handle h, const float* audio_dev, int B, float* mel_dev, void* stream);

/* a3+a4 (or a9): log-mel (B, n_frames, n_mels) f32 -> encoder output (B, n_frames, d_model) bf16. */
int ymt3_encode(ymt3_handle h, const float* mel_dev, int B, void* enc_dev, void* stream);

/* a6+a7+a8(+a10): encoder output bf16 -> greedy token ids (B, n_channels, n_steps) int32.
 * forced_dev (may be NULL): (B, n_channels, n_steps) int32 teacher-forcing ids fed back instead of
 * the argmax.  logits_dev (may be NULL): (B, n_channels, n_steps, vocab) f32 per-step logits.
 * The emitted id is the lowest index among the maxima of the row's f32 logits.
 *
 * Non-finite values.  Float PCM is not range-limited, so a corrupt input can reach every stage; what then happens is defined:
 *   - front end: a NaN sample makes every frame that contains it NaN in every mel bin (a NaN power is not read as the floor); a
 *     power beyond the f32 range gives a non-finite log-mel (+inf, or NaN where a zero filter weight meets the infinite bin).
 *     Frames and segments without such a sample are untouched.
 *   - a segment with a non-finite log-mel has a NaN encoder output and NaN logits in all of its rows, and only in its rows: the other
 *     rows of the batch keep the bits they have in a clean batch, and the next call on the handle is not affected.
 *   - argmax: NaN logits take no part in the comparison.  A row in which no (allowed) logit compares greater than -3.4e38 -- all
 *     NaN, all -inf -- emits the lowest index, under a constraint the lowest index its state allows, as an exact tie does; the
 *     automaton follows that id.  Every id written to tokens_dev lies in [0, vocab) (or is pad_id), and no index derived from a
 *     logit reaches memory unclamped.
 *   - scores: the score of a step whose logits are NaN, or all -inf, is NaN. */
int ymt3_decode_greedy(ymt3_handle h, const void* enc_dev, int B, int n_steps, int32_t* tokens_dev,
                       const int32_t* forced_dev, float* logits_dev, void* stream);

/* Task prompts (the `task_tokens` of inference(x, task_tokens, max_token_length)): a prefix of ids fed to the decoder before
 * it emits, in the convention of HF `generate(decoder_input_ids=[[pad_id, *prompt]])`.
 *   - prompt_dev: (B, n_channels, n_prompt) int32 on the device; n_prompt = P is the same for every row of a call, the ids may
 *     differ per row.  P = 0 (prompt_dev may then be NULL) is exactly the unprompted call: ymt3_decode_greedy,
 *     ymt3_transcribe_segments and ymt3_transcribe_stream are the P = 0 cases of the *_prompted entry points.
 *   - step 0 consumes the decoder start id (pad_id); steps 0 .. P-1 feed prompt[r][t] instead of their argmax; the argmax of
 *     step P + j is emitted token j.  A call launches P + n_steps steps and needs P + n_steps <= max_decode_len (the cache).
 *   - prompt positions emit nothing: they write no token and no logits, and an argmax equal to eos_id there does not finish the
 *     row.  tokens_dev, forced_dev and logits_dev keep their shapes (B, n_channels, n_steps[, vocab]) and index emitted tokens
 *     only; forced_dev overrides the feed at emitted columns exactly as in ymt3_decode_greedy.
 *   - prompt ids are clamped into [0, vocab) where they are fed, as forced ids are.
 *   - ymt3_set_early_stop counts emitted steps only (the prompt's steps always run); ymt3_last_decode_steps reports LAUNCHED
 *     steps, the prompt's included.
 *   - YMT3_ERR_ARG (the handle stays usable): n_prompt < 0, n_prompt > 0 with a NULL prompt, P + n_steps > max_decode_len, or
 *     P > 0 while ymt3_debug_decode_start is pending.
 * Every decode kernel reads the prompt from device memory: no captured graph depends on it. */
int ymt3_decode_prompted(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                         int32_t* tokens_dev, const int32_t* forced_dev, float* logits_dev, void* stream);
int ymt3_transcribe_segments_prompted(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev,
                                      int n_prompt, int32_t* tokens_dev, void* stream);
/* As ymt3_transcribe_stream; prompt_dev is (n_segments, n_channels, n_prompt), each segment's rows fed their own prompt. */
int ymt3_transcribe_stream_prompted(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev,
                                    int n_prompt, int32_t* tokens_dev, int slots, int interval, void* stream);

/* Token scores: the log-probability of every emitted step, from the same f32 logits the argmax reads (HF `generate(output_scores=
 * True)` + `compute_transition_scores(normalize_logits=True)`), without writing the logits themselves.
 *   - scores_dev: (B, n_channels, n_steps) f32 on the device, indexed exactly as tokens_dev (emitted steps only; in
 *     ymt3_transcribe_stream_scored (n_segments, n_channels, n_steps)).
 *   - score[r][col] = log_softmax(logits of that step)[id], where id is the id fed to the next step: the emitted argmax token
 *     when the call is not forced, forced[r][col] (clamped into [0, vocab) like the feed) when it is.  Unforced scores are the
 *     log-probabilities of the emitted tokens, always <= 0; with forcing, the sum of a row is the teacher-forced
 *     log-likelihood of the forced sequence.
 *   - an unforced row that has already finished (EOS emitted, eos_id >= 0) scores its PAD columns exactly 0.0.
 *   - columns never launched score 0.0, like their PAD ids: the tail after an early stop (ymt3_set_early_stop) and the tail of
 *     a retired segment in ymt3_transcribe_stream_scored.
 *   - prompt positions write nothing, as for tokens.
 *   - a call whose ids are poisoned to INT32_MIN (ymt3_set_abort_recovery(h, 0)) has NaN scores.
 *   - the ids are bit-identical with and without scores_dev, in every decode regime; scores_dev == NULL makes each entry point
 *     exactly its *_prompted counterpart (which are these calls with scores_dev = NULL).
 * The kernels read the scores pointer from device memory: no captured graph depends on it. */
int ymt3_decode_scored(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                       int32_t* tokens_dev, float* scores_dev, const int32_t* forced_dev, float* logits_dev, void* stream);
int ymt3_transcribe_segments_scored(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev,
                                    int n_prompt, int32_t* tokens_dev, float* scores_dev, void* stream);
int ymt3_transcribe_stream_scored(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev,
                                  int n_prompt, int32_t* tokens_dev, float* scores_dev, int slots, int interval, void* stream);

/* Sequence scoring: the teacher-forced log-probability of GIVEN ids, all positions in one pass (HF forward with labels:
 * `model(inputs_embeds=..., labels=...)`).  Exactly what ymt3_decode_scored(..., forced_dev = tokens_dev) defines, without its n_prompt +
 * n_steps dependent steps: with the ids known every position of every row is computed at once (kernels: yourmt3_amd/csrc/dec_seq.hip).
 *   - tokens_dev: (B, n_channels, n_steps) int32, read only.  prompt_dev: (B, n_channels, n_prompt), the prompted calls' convention.
 *     Position 0 consumes pad_id, positions 1 .. P the prompt, position P + j + 1 tokens[j].
 *   - scores_dev: (B, n_channels, n_steps) f32.  score[r][j] = log_softmax(logits of position P + j)[tokens[r][j]]; ids are clamped into
 *     [0, vocab) both as feed and as target, as the forced path does.  Prompt positions write nothing.
 *   - logits_dev (may be NULL): (B, n_channels, n_steps, vocab) f32 raw logits.
 *   - lengths_dev (may be NULL: every column counts): (B, n_channels) int32, clamped into [0, n_steps].  Columns j >= lengths[r] score
 *     exactly 0.0 (their logits, if requested, are still written); the decoder is causal, so a length never changes an earlier column.
 *   - the score of a position whose logits are NaN, or all -inf, is NaN.  A non-finite segment has NaN scores in its own rows only;
 *     the other rows keep their bits.
 *   - the two evaluation orders (this pass and the step loop) agree within the parity tolerance of the logits, not bit for bit: the
 *     attention here rounds the softmax numerators to bf16 (the encoder kernel's contract), the step kernels keep them in f32.
 *   - YMT3_ERR_ARG (the handle stays usable): n_steps <= 0, n_prompt < 0, P + n_steps > max_decode_len, NULL tokens or scores, a NULL
 *     prompt with P > 0.
 *   - NOT SUPPORTED: the MoE decoder FFN (dec_ffn = YMT3_FFN_MOE) returns YMT3_ERR_UNSUPPORTED, the message names dec_ffn: the
 *     full-sequence pass has no grouped expert GEMMs yet.  Constraints are not part of this call.
 * Asynchronous on `stream`.  The pass works in the encoder's activation buffers and touches neither the self-attention cache nor the
 * decode loop state: a decode call after it is bit-identical to one before it.  Nothing is allocated after ymt3_create. */
int ymt3_score_tokens(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                      const int32_t* tokens_dev, const int32_t* lengths_dev, float* scores_dev, float* logits_dev, void* stream);
int ymt3_transcribe_segments_score(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                   const int32_t* tokens_dev, const int32_t* lengths_dev, float* scores_dev, void* stream);

/* Constraints: a token automaton limits which tokens each row may emit (HF `generate(prefix_allowed_tokens_fn=...)`, i.e. a
 * PrefixConstrainedLogitsProcessor, greedy).
 *   - an automaton has S states, allowed[S][V] (one bit per token, V = cfg.vocab) and next[S][V] (an int32 state for every
 *     (state, token) pair); every decoded row has a start state, given per (segment, channel) by start_state_dev: (B,
 *     n_channels) int32 on the device, (n_segments, n_channels) for ymt3_transcribe_stream_constrained, NULL = state 0 for all.
 *     A start state outside [0, S) is clamped into range on the device, as fed ids are.
 *   - at every emitted position of a live row in state s the emitted token is the lowest index among the maxima of the raw
 *     logits over {i : allowed[s][i]}; with f the fed id (the emitted token, or forced[...] clamped into [0, vocab) when forcing),
 *     the row's state becomes next[s][f].
 *   - prompt positions neither mask nor advance the state: the automaton starts at the first emitted token.
 *   - with eos_id >= 0 a row that has emitted EOS emits PAD (score 0.0 unless forced) and its state stays frozen.
 *   - scores_dev: log_softmax of the masked row (disallowed tokens -inf) at f -- HF compute_transition_scores(normalize_logits=
 *     True) behind the constraint's logits processor.  A forced id that is not allowed scores -inf.
 *   - logits_dev stays the raw, unmasked logits (HF `output_logits`).
 *   - constraint == NULL is the unconstrained call bit for bit (ids, logits, scores): each *_scored entry point is its
 *     *_constrained counterpart with constraint = NULL and start_state_dev = NULL.  start_state_dev without a constraint
 *     is an error.
 * The tables live in device memory owned by the constraint object; the kernels read them through the device-resident loop
 * state, so no captured graph depends on them.  Every decode regime selects through the same kernel. */
typedef struct ymt3_constraint_s* ymt3_constraint;
/* Validate once, then upload once.  allowed_bits_host: [n_states][ceil(vocab / 32)] uint32 (bit i % 32 of word i / 32 = token
 * i; bits at or beyond vocab are ignored); next_host: [n_states][vocab] int32.  Checks: vocab == the handle's cfg.vocab,
 * 1 <= n_states <= 1024, every next in [0, n_states), every state allows at least one token.  Synchronous (a blocking
 * upload).  The constraint belongs to h: using it on another handle is an error.  ymt3_constraint_destroy(c) frees it
 * (NULL is a no-op); it may run before or after the handle's ymt3_destroy(h). */
int  ymt3_constraint_create(ymt3_handle h, int n_states, int vocab, const uint32_t* allowed_bits_host, const int32_t* next_host,
                            ymt3_constraint* out);
void ymt3_constraint_destroy(ymt3_constraint c);
int ymt3_decode_constrained(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                            int32_t* tokens_dev, float* scores_dev, const int32_t* forced_dev, float* logits_dev,
                            ymt3_constraint constraint, const int32_t* start_state_dev, void* stream);
int ymt3_transcribe_segments_constrained(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev,
                                         int n_prompt, int32_t* tokens_dev, float* scores_dev, ymt3_constraint constraint,
                                         const int32_t* start_state_dev, void* stream);
int ymt3_transcribe_stream_constrained(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev,
                                       int n_prompt, int32_t* tokens_dev, float* scores_dev, int slots, int interval,
                                       ymt3_constraint constraint, const int32_t* start_state_dev, void* stream);

/* Beam search (HF `generate(num_beams=W, num_return_sequences=N, length_penalty=alpha, early_stopping=True, do_sample=False)`,
 * i.e. GenerationMixin._beam_search of transformers 5.x with one EOS id).  Per group g = (segment, channel), with NEG = -1e9:
 *   - state: W running beams with f32 cumulative log-probabilities run[w] (run[0] = 0, the others NEG: step 0 expands beam 0 only) and W
 *     finished slots, empty at first.
 *   - emitted step j (len = j + 1 tokens after it): lp[w][v] = log_softmax(logits of running beam w)[v] -- under a constraint of the row
 *     masked by the beam's automaton state, the quantity scores_dev holds in a greedy call -- and acc[w][v] = run[w] + lp[w][v] in f32.  The
 *     2W largest acc over the W * V candidates are taken in descending order; EQUAL scores are ordered by the lower flat index w * V + v.
 *     A candidate is `hit` if its token is eos_id or j + 1 == n_steps (the length limit finishes every candidate).  The next running
 *     beams are the best W of the 2W after NEG has been added to the hit ones, in order (first among equals); each records its parent beam
 *     and token, and its automaton state is next[state[parent]][token].  A candidate enters the finished slots only if it is hit AND among
 *     the first W of the 2W AND the group was not done before the step; its score is acc / len^alpha.  Old slots (first) and entering
 *     candidates (in candidate order) are merged and the best W kept, best first.  A group is DONE when its W slots are full: it changes
 *     nothing any more and its rows idle on pad_id.  Step n_steps - 1 finishes every candidate, so a call that ran all its steps has W
 *     full slots per group.
 *   - result: the first N = num_return slots, best first.  tokens_dev (B, n_channels, N, n_steps): a hypothesis' tokens up to and including
 *     its EOS, then pad_id (always PAD, as the greedy calls; HF fills with EOS when pad_token_id is 0).  seq_scores_dev (B, n_channels, N), may
 *     be NULL: acc / len^alpha (HF sequences_scores).  token_scores_dev (B, n_channels, N, n_steps), may be NULL: lp of every token of the
 *     returned hypothesis (HF compute_transition_scores with beam_indices), 0.0 at PAD; they sum to seq_score * len^alpha.
 *   - eos_id < 0: nothing finishes before the length limit.  num_beams = 1 is greedy search through this path.
 *   - prompts: prompt_dev is (B, n_channels, n_prompt); prompt positions feed all W rows of a group the same ids, emit nothing and do not
 *     touch the beam state; len counts emitted tokens only.  start_state_dev is (B, n_channels): a group's W beams start in the same state.
 *   - non-finite values: NaN logits are no candidates; a beam whose row holds a NaN (or no comparable logit) has NaN scores, and its
 *     candidates rank at NEG.  The groups of a non-finite segment return ids in range and NaN scores; the other groups keep their bits.
 *   - limits (YMT3_ERR_ARG naming the limit, the handle stays usable): 1 <= num_return <= num_beams <= 8; length_penalty finite and >= 0
 *     (a negative one breaks the early-stopping argument that lets a done group freeze); B * n_channels * num_beams <= max_batch *
 *     n_channels, the rows the handle's caches were created for; n_channels * num_beams <= 255; max_decode_len below 48 K.
 *   - not supported: forced ids with beams, early_stopping False / "never", sampling, diverse beam groups.
 * Rows: beam w of group g decodes as row g * W + w.  K/V of a position stays in the cache slab of the row that computed it; the
 * self-attention kernel follows a per-row ancestry table instead of the cache being reordered every step.  Beam calls run the separate
 * decode launches (one chain, lock-step), whatever the row count.  Asynchronous like the other decode calls (ymt3_set_early_stop: stops
 * once every group is done, synchronising once per interval; the result is the full-length one).  All beam scratch is allocated in
 * ymt3_create; the kernels read every per-call pointer and parameter from device memory, so no captured graph depends on them. */
typedef struct ymt3_beam_params { int32_t num_beams, num_return; float length_penalty; } ymt3_beam_params;
int ymt3_decode_beam(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                     const ymt3_beam_params* params, int32_t* tokens_dev, float* seq_scores_dev, float* token_scores_dev,
                     ymt3_constraint constraint, const int32_t* start_state_dev, void* stream);
int ymt3_transcribe_segments_beam(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                  const ymt3_beam_params* params, int32_t* tokens_dev, float* seq_scores_dev, float* token_scores_dev,
                                  ymt3_constraint constraint, const int32_t* start_state_dev, void* stream);
/* Beam search under continuous batching: ymt3_transcribe_stream's queue with slots of n_channels * num_beams rows.  audio_dev is
 * (n_segments, segment_samples), prompt_dev (n_segments, n_channels, n_prompt), start_state_dev (n_segments, n_channels); tokens_dev
 * (n_segments, n_channels, N, n_steps), seq_scores_dev (n_segments, n_channels, N) and token_scores_dev (n_segments, n_channels, N, n_steps;
 * both may be NULL) hold exactly what ymt3_transcribe_segments_beam leaves for the same segments.  `slots` counts segments (<= 0, or more than
 * fit: max_batch / num_beams; YMT3_ERR_ARG naming max_batch if that is 0), `interval` is ymt3_transcribe_stream's (0: 8).  Every `interval`
 * steps the host reads the rows' finished flags; a segment whose n_channels groups are all done is retired -- the result kernel runs over its
 * slot's groups -- and the slot restarts on the next pending segment (log-mel, encoder, cross-K/V into the slot's slabs, beam state reset);
 * done groups of a segment that is still live stay stopped on pad_id.  A group's results do not depend on what the other slots hold.  The
 * limits above apply with their messages.  Synchronises once per interval and returns when the queue is done; ymt3_last_decode_steps counts
 * launched steps (`interval` per round).  Allocates nothing after ymt3_create but the pinned flag buffer of ymt3_transcribe_stream. */
int ymt3_transcribe_stream_beam(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                const ymt3_beam_params* params, int32_t* tokens_dev, float* seq_scores_dev, float* token_scores_dev,
                                int slots, int interval, ymt3_constraint constraint, const int32_t* start_state_dev, void* stream);
/* Debug hook, gated like ymt3_debug_moe_trace (YMT3_DEBUG_HOOKS=1): from now on every beam call records, per emitted step, the new running
 * beams of every group: trace_dev[step][group][W][2] int32 = (parent beam, token), run_dev[step][group][W] f32 their cumulative
 * log-probabilities (may be NULL), logits_dev[step][group][W][V] f32 the raw logits of the running beams the step selected from (may be NULL;
 * not written for a done group).  Steps >= n_steps and groups >= n_groups are not recorded; W is the call's num_beams; trace_dev = NULL stops
 * recording.  The search is discrete: with the trace a test feeds the device's choices to the CPU oracle and compares every step.
 * ymt3_transcribe_stream_beam records under [emitted step of the group][segment * n_channels + channel] -- the group's index in the queue,
 * not its slot's -- and records nothing for a done group. */
int ymt3_debug_beam_trace(ymt3_handle h, int32_t* trace_dev, float* run_dev, float* logits_dev, int n_steps, int n_groups);

/* Opt-in early stop (first step): with eos_id >= 0 and interval > 0, ymt3_decode_greedy /
 * ymt3_transcribe_segments check on the host every `interval` steps whether every row has emitted EOS and stop
 * launching once all have (the remainder of each row is PAD, exactly what the full-length run produces).  In this mode the
 * call synchronises the stream once per interval.  interval = 0 (default) restores the loop that queues every step at once. */
int ymt3_set_early_stop(ymt3_handle h, int interval);

/* The whole hot path: audio (B, segment_samples) f32 -> token ids (B, n_channels, n_steps) int32. */
int ymt3_transcribe_segments(ymt3_handle h, const float* audio_dev, int B, int n_steps,
                             int32_t* tokens_dev, void* stream);

/* Continuous batching: transcribe a queue of `n_segments` segments, audio (n_segments,
 * segment_samples) f32 -> ids (n_segments, n_channels, n_steps) int32, through `slots` decoder slots (<= 0 or
 * > max_batch: max_batch).  Every row decodes at its own position; every `interval` steps (0: 8) the host reads the
 * per-row stop flags, retires segments whose rows have all emitted EOS (or n_steps tokens; the tail is PAD, exactly
 * what the lock-step calls produce) and encodes the next pending segments into the freed slots.  The ids are bit-identical
 * to ymt3_transcribe_segments on the same segments.  Synchronises the stream (once per interval) and returns when the
 * queue is done. */
int ymt3_transcribe_stream(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, int32_t* tokens_dev,
                           int slots, int interval, void* stream);

/* Number of decoder steps the last decode call on this handle actually launched (ymt3_decode_greedy,
 * ymt3_transcribe_segments: n_steps unless ymt3_set_early_stop cut it short; ymt3_transcribe_stream: every step of every round).
 * Prompted calls count the prompt's steps too: n_prompt + n_steps without an early stop. */
int ymt3_last_decode_steps(ymt3_handle h);

/* The merged decode kernels (up to 64 rows, one channel: a layer's two attentions as one launch, its four skinny GEMMs as one launch)
 * hand data between workgroups inside a launch and therefore need every workgroup of their grid resident at once; the handle enables
 * them only where the occupancy query says they fit.  If something else holds CUs while one runs (another process or handle on the
 * same GPU, a CU mask), a stage can wait in vain: every wait is bounded (1 s), then the kernel raises a sticky abort word and the
 * launch drains.  What follows is governed by `mode`:
 *   1 (default): ymt3_decode_greedy / ymt3_transcribe_segments / ymt3_transcribe_stream wait for their own work at the end of the call
 *      and look at the word.  Raised: the call is run AGAIN through the separate launches (fresh launches in the same process;
 *      the same arithmetic, bit-identical ids) and the handle stays on them.  The caller sees correct ids, later.
 *   0: calls stay fully asynchronous.  An aborted call's ids are all INT32_MIN (never plausible ids); the NEXT call on the handle
 *      notices, waits for the device, and switches to the separate launches before doing its own work.
 * ymt3_merged_fallbacks: how many times this handle has left the merged kernels that way (0 or 1; it never goes back).
 * (YMT3_ABORT_RECOVERY=0 in the environment at ymt3_create selects mode 0.) */
int ymt3_set_abort_recovery(ymt3_handle h, int mode);
int ymt3_merged_fallbacks(ymt3_handle h);

/* How many concurrent row ranges ("chains", each on a stream of the handle's own, joined into the caller's stream before the call returns
 * control of it) the last ymt3_decode_greedy / ymt3_transcribe_segments call decoded its batch as.  1 except for 168-256 rows of one channel
 * with the dense FFN, where two halves overlap (the attention kernels are bandwidth-bound there, the GEMMs between them latency-bound); the ids do
 * not depend on it.  YMT3_CHAINS=n in the environment at ymt3_create fixes the number (1..8). */
int ymt3_last_decode_chains(ymt3_handle h);

/* Layer 0's QKV projection as a table.  The residual stream entering layer 0 of a one-channel decoder is the embedding row of the fed
 * token and nothing else, so that projection is a function of the token id: ymt3_create builds it over the vocabulary ([vocab][3 * 512]
 * bf16, counted in ymt3_device_bytes) with the decode step's own kernels, and the kernel that feeds a row copies the id's table row where
 * the projection launch would have written it -- one launch less per step, the same bits.  Taken by every greedy decode call (lock-step and
 * stream; prompted, scored, constrained) whose steps would run the 16-row-tile projection kernel; not by multi-channel handles, beam calls,
 * ymt3_profile_decode, handles created under YMT3_STAMP or YMT3_STEP_KERNEL=1, or row counts from the mid-size tile threshold on.
 * YMT3_NO_QKV0_TABLE=1 in the environment at ymt3_create keeps the launch (A/B).
 * Returns 1 if the handle's last decode call skipped the layer-0 launch, else 0. */
int ymt3_qkv0_table_active(ymt3_handle h);

/* Device detokeniser: token ids -> notes without a host loop (TaskManager.tokens_to_notes_device; the specification is the host path,
 * NoteEventTokenizer.decode_segment + note_events_to_notes of yourmt3_amd/task_manager.py, which it reproduces exactly: the same notes, the
 * same f64 times bit for bit, the same invalid-token count).
 *   - token table: token_table_host[vocab] uint16 = class << 12 | value (TaskManager.token_table), so the kernels know nothing of the codec's
 *     layout.  Classes: 0 invalid (UNK, unused ids), 1 stop (PAD, EOS), 2 skip (task tokens), 3 shift, 4 pitch, 5 velocity, 6 tie,
 *     7 program, 8 drum.  An id outside [0, vocab) on the device is class 0 (so are the INT32_MIN ids of an aborted decode call).
 *   - tokens_dev: element (segment s, channel c, column j) is tokens_dev[s * seg_stride + c * chan_stride + j], strides in ELEMENTS, n_channels
 *     = cfg.n_channels; a contiguous (n, K, L) tensor has strides (K * L, L), and the (b, K, N, L) output of a beam call is read in place
 *     with hypothesis 0's strides (K * N * L, N * L).  scores_dev (may be NULL): f32 token scores in the same layout; a note then carries
 *     the score of its onset's token, a de-duplicated drum hit the first one unless a later one compares greater (a NaN neither replaces
 *     nor is replaced).  Without scores every record's score is NaN.
 *   - start_sec_dev: (n_segments,) f64 start time of every segment.  It MUST be strictly increasing: the kernels take the segment index
 *     for the host's order by start time and do not check (the Python wrapper does, and raises ValueError).  end_sec closes the notes
 *     still sounding after the last segment.  Event times are start_sec + step / steps_per_second in f64, that division and that add.
 *   - notes_dev: `capacity` records of 32 bytes { f64 onset, f64 offset, i32 program, i32 pitch, i32 is_drum, f32 score }, in no
 *     particular order.  Capacity bound: capacity >= n_segments * n_channels * n_steps (a token yields at most one note), else YMT3_ERR_ARG.
 *     counts_dev: [2] int32 = { n_notes, n_invalid }; the call zeroes it first.
 *   - kernels (yourmt3_amd/csrc/detok.hip): one wave per (segment, channel) row runs decode_segment as wave-level scans and compacts the
 *     row's events; one workgroup per channel buckets them by (program, pitch) with a counting sort in LDS, and one lane per key walks its
 *     bucket with the host's tie / re-trigger / offset / drum rules.
 * ymt3_detok_create: synchronous, like ymt3_constraint_create.  Checks (YMT3_ERR_ARG naming the argument): vocab == cfg.vocab,
 * max_segments >= 1, 1 <= max_steps <= max_decode_len, drum_program in [0, 4095], steps_per_second >= 1, table classes 0..8, pitch and
 * drum values below 128, velocity values 0 or 1; program values (and drum_program) above 255 are YMT3_ERR_UNSUPPORTED.  Allocates all
 * scratch, sized by max_segments * n_channels * max_steps (18 bytes per token: items, their keys, the bucketed copy) plus the key
 * offsets; the records are the caller's.  The object belongs to h; ymt3_detok_destroy frees it (NULL is a no-op), before or after the
 * handle's destruction.
 * ymt3_detokenize: asynchronous on `stream`, allocates nothing, leaves the handle's decode state alone.  YMT3_ERR_ARG, with handle and
 * detokeniser still usable, for n_segments > max_segments, n_steps outside [1, max_steps], NULL tokens_dev / start_sec_dev / notes_dev /
 * counts_dev, or a capacity below the bound; n_segments = 0 only zeroes the counts.  One object serves one call at a time. */
typedef struct ymt3_detok_s* ymt3_detok;
int  ymt3_detok_create(ymt3_handle h, const uint16_t* token_table_host, int vocab, int steps_per_second,
                       int drum_program, int max_segments, int max_steps, ymt3_detok* out);
void ymt3_detok_destroy(ymt3_detok d);
int  ymt3_detokenize(ymt3_handle h, ymt3_detok d, const int32_t* tokens_dev, const float* scores_dev /* may be NULL */,
                     int n_segments, int n_steps, long long seg_stride, long long chan_stride,
                     const double* start_sec_dev, double end_sec,
                     void* notes_dev, long long capacity, int32_t* counts_dev /* [2]: n_notes, n_invalid */, void* stream);

/* Incremental detokeniser: ymt3_detokenize for segments that arrive over time (Detokenizer.new_state / push_device / finish_device,
 * TaskManager.tokens_to_notes_stream).  The specification is the host's NoteStream (yourmt3_amd/task_manager.py), the incremental form of
 * note_events_to_notes: take the records that every ymt3_detokenize_push and then ymt3_detokenize_finish write, and they are, as a set,
 * the records ymt3_detokenize writes for all the segments at once with the same end_sec -- the same f64 times bit for bit, the same
 * scores -- for every way of cutting the segments into pushes, as long as no call reports n_forced != 0.  Per call the records are
 * exactly those NoteStream returns for the call.
 *   - records, token table, strides, scores and the time arithmetic are those of ymt3_detokenize; kernel (a) is the same kernel, the
 *     merge kernel is its form (c) (yourmt3_amd/csrc/detok.hip), which starts every key's walk from the carried state and stores it back.
 *   - a push: n_segments >= 0 segments, LATER than every segment pushed before; start_sec_dev (n_segments,) f64 strictly increasing
 *     (not checked on the device, as for ymt3_detokenize).  horizon_sec is the start time of the next segment not yet pushed; +inf means
 *     that no further segment can arrive before the finish.  n_segments = 0 only moves the horizon.
 *   - what a call writes: every pitched note that ended -- by an offset, a re-trigger, or a missing tie at a segment start.  A note still
 *     sounding after the push's last segment stays in the state (its onset, its score, a valid bit per (channel, program, pitch)) and is
 *     continued by a tie in the next push's first segment, else closed at that segment's start.  A pitched record never changes once
 *     written.  A drum hit can: a hit of a later segment at the same f64 time and pitch is merged into it and may raise its score, and
 *     every event of a later segment lies at or after that segment's start.  So a push writes the hits with time < horizon_sec and HOLDS
 *     the others in the state, still open to de-duplication; a later push whose horizon exceeds their time, or the finish, writes them.
 *   - the bound on held hits: every (channel, drum pitch) holds at most max_held.  When a push would leave more, the earliest surplus hits
 *     are written at once, earliest time first, and counted in n_forced: a non-zero n_forced tells the caller that exactness may have
 *     been lost (a later duplicate of a forced hit becomes a second record).
 *   - ymt3_detokenize_finish writes every held hit and closes every sounding note at end_sec (dropped if end_sec is not after its onset),
 *     the rule of the one-shot call's tail.  After it the state takes no call until ymt3_detok_state_reset.
 *   - counts_dev: [3] int32 = { n_notes, n_invalid, n_forced } of THIS call; the call zeroes it first.
 *   - capacity bound, exactly: capacity >= n_segments * n_channels * n_steps + ymt3_detok_state_carry(st), else YMT3_ERR_ARG (the finish:
 *     n_segments = 0).  ymt3_detok_state_carry = n_channels * 128 * (n_programs - 1 + max_held), n_programs being one more than the largest
 *     program of the token table (and of drum_program): a call can close one carried note per pitched key and write max_held held hits per
 *     drum pitch on top of the one record per token of ymt3_detokenize.
 *   - YMT3_ERR_ARG, with handle, detokeniser and state still usable and the state unchanged: the argument errors of ymt3_detokenize, a
 *     NULL notes_dev, a capacity below the bound, a state created for another detokeniser, a call after the finish without a reset, and a
 *     horizon_sec that is -inf, NaN or below the previous push's horizon (the start times are device memory and are not read: what the
 *     host can check of "before the last pushed start" is the previous horizon, which no later start may precede; the Python wrapper
 *     checks the start times themselves).
 * ymt3_detok_state_create: synchronous; allocates the state, 16 bytes per (channel, program, pitch) and 2 x 16 x max_held bytes per
 * (channel, drum pitch); max_held in [1, 4096].  The state belongs to h and to d; ymt3_detok_state_destroy frees it (NULL is a no-op),
 * before or after the handle's destruction.  ymt3_detok_state_reset empties it, asynchronously on `stream`.  push and finish are
 * asynchronous on `stream`, allocate nothing, use the detokeniser's scratch (one call at a time per detokeniser, whatever the state)
 * and leave the handle's decode state alone. */
typedef struct ymt3_detok_state_s* ymt3_detok_state;
int  ymt3_detok_state_create(ymt3_handle h, ymt3_detok d, int max_held, ymt3_detok_state* out);
void ymt3_detok_state_destroy(ymt3_detok_state st);
int  ymt3_detok_state_reset(ymt3_handle h, ymt3_detok_state st, void* stream);
long long ymt3_detok_state_carry(ymt3_detok_state st);
int  ymt3_detokenize_push(ymt3_handle h, ymt3_detok d, ymt3_detok_state st, const int32_t* tokens_dev, const float* scores_dev /* may be NULL */,
                          int n_segments, int n_steps, long long seg_stride, long long chan_stride,
                          const double* start_sec_dev, double horizon_sec,
                          void* notes_dev, long long capacity, int32_t* counts_dev /* [3]: n_notes, n_invalid, n_forced */, void* stream);
int  ymt3_detokenize_finish(ymt3_handle h, ymt3_detok d, ymt3_detok_state st, double end_sec,
                            void* notes_dev, long long capacity, int32_t* counts_dev /* [3] */, void* stream);

/* Device tokeniser: notes -> token ids without a host loop, the inverse of the device detokeniser (TaskManager.notes_to_tokens_device;
 * the specification is the host path, TaskManager.notes_to_tokens of yourmt3_amd/task_manager.py, which it reproduces exactly: the same
 * ids and the same lengths for every row that fits).
 *   - params: all the kernels know of the codec -- the first id of each of the shift (value 1), pitch, velocity, tie, program and drum
 *     ranges, max_shift_steps, steps_per_second, drum_program, and the EOS and PAD ids (TaskManager.tok_params).
 *     program_channel_host[n_programs] uint8: the decoder channel of every program (TaskManager.channel_of_program).
 *   - notes_dev: n_notes records of 32 bytes { f64 onset, f64 offset, i32 program, i32 pitch, i32 is_drum, f32 score }, the device
 *     detokeniser's own record, 8-byte aligned, in any order; `score` is not read, so the output of ymt3_detokenize can be fed back
 *     without touching the host.  A record with is_drum != 0 counts as program drum_program.  Dropped without an error: an onset
 *     outside [start_sec[0], end_sec) or NaN, a NaN offset of a pitched note, a program outside [0, n_programs), a pitch outside
 *     [0, 128) -- the host path raises for the last two; the Python wrapper checks a note list before it uploads it.
 *   - start_sec_dev: (n_segments,) f64 start time of every segment.  It MUST be strictly increasing: the kernels search it and do not
 *     check (the Python wrapper does, and raises ValueError).  Steps are rint((time - start_sec) * steps_per_second) in f64, that
 *     subtract and that multiply, half to even; they saturate at 2^31 - 2.
 *   - tokens_dev: (n_segments, n_channels, n_steps) int32, contiguous; every row is its ties, TIE, its events, EOS, then PAD.
 *     lengths_dev: (n_segments, n_channels) int32, the tokens the row needs, EOS included.  A row that needs more than n_steps reports a
 *     length > n_steps (a lower bound of the count when it has more than n_steps items or a gap of more than n_steps shifts) and
 *     holds an unspecified prefix: the caller must look at the lengths before it uses the ids.
 *   - kernels (yourmt3_amd/csrc/tok.hip): one lane per note finds its segments by binary search and appends one 64-bit item per event
 *     and per tied boundary to the owning row (a tie only once per segment and key, through a bitmap); one wave per row sorts its items in LDS and
 *     runs encode_segment as wave-level scans.
 * ymt3_tok_create: synchronous, like ymt3_detok_create.  Checks (YMT3_ERR_ARG naming the argument): params and program_channel_host not
 * NULL, n_programs >= 1, every id range inside [0, cfg.vocab), steps_per_second >= 1, max_shift_steps >= 1, drum_program in
 * [0, n_programs), every channel below cfg.n_channels, max_segments >= 1, 1 <= max_steps <= min(max_decode_len, 4096); n_programs above
 * 256 is YMT3_ERR_UNSUPPORTED.  Allocates all scratch: 8 bytes per output token of max_segments * n_channels * max_steps, a counter per
 * row and 16 * n_programs bytes per segment.  The object belongs to h; ymt3_tok_destroy frees it (NULL is a no-op), before or after the
 * handle's destruction.
 * ymt3_tokenize: asynchronous on `stream`, allocates nothing, leaves the handle's decode state alone.  YMT3_ERR_ARG, with handle and
 * tokeniser still usable, for n_segments > max_segments, n_steps outside [1, max_steps], n_notes outside [0, 2^29], a misaligned
 * notes_dev, or NULL notes_dev (with n_notes > 0) / start_sec_dev / tokens_dev / lengths_dev.  n_notes = 0 gives TIE, EOS rows;
 * n_segments = 0 is a no-op.  One object serves one call at a time. */
typedef struct ymt3_tok_params {
    int32_t shift_base, pitch_base, velocity_base, tie_base, program_base, drum_base;
    int32_t max_shift_steps, steps_per_second, drum_program;
    int32_t eos_id, pad_id;
} ymt3_tok_params;
typedef struct ymt3_tok_s* ymt3_tok;
int  ymt3_tok_create(ymt3_handle h, const ymt3_tok_params* params, const uint8_t* program_channel_host, int n_programs,
                     int max_segments, int max_steps, ymt3_tok* out);
void ymt3_tok_destroy(ymt3_tok t);
int  ymt3_tokenize(ymt3_handle h, ymt3_tok t, const void* notes_dev, long long n_notes, const double* start_sec_dev,
                   int n_segments, double end_sec, int n_steps, int32_t* tokens_dev, int32_t* lengths_dev, void* stream);

/* Device note metrics: how right is a transcription -- onset, onset+offset and drum F1 of an estimate against a reference, as integers
 * (YourMT3.compile_note_metrics, evaluate(); the specification is the host path, note_metrics of yourmt3_amd/metrics.py, which it
 * reproduces exactly: every integer of the result).  The rules are this repository's own, shaped after the usual note-transcription
 * metric.  Both sides are records of 32 bytes { f64 onset, f64 offset, i32 program, i32 pitch, i32 is_drum, f32 score }, the device
 * detokeniser's own record, 8-byte aligned, in any order; `score` is not read.
 *   - counted records: the onset is not NaN, the pitch lies in [0, 128), the effective program p lies in [0, n_programs) -- p =
 *     drum_program if is_drum != 0, else program: the drum rule of the tokeniser -- and, if the note is pitched, the offset is not NaN.  A
 *     record with p == drum_program is a drum note whatever is_drum says; every other counted record is pitched.  The other records are
 *     skipped and appear in skipped[] only.
 *   - distance rounding: d(a, b) = rint(|a - b| * 1e4) / 1e4 in f64, that subtract, multiply, round-half-even and divide, nothing
 *     contracted (times are start + step / 100, and |1.05 - 1.00| exceeds 0.05 in f64: with the rule, 50 ms apart on the grid hits).
 *   - hits of reference i and estimate j of one key: onset, d(on_i, on_j) <= onset_tol; onset+offset, the onset hit and d(off_i, off_j) <=
 *     max(offset_min_tol, offset_ratio * (off_i - on_i)), the tolerance not rounded.  Drum notes never look at offsets: their
 *     onset+offset numbers equal their onset numbers.
 *   - counts_dev: [(n_programs + 1) * 6 + 2] int32 = counts[row][metric][3] then skipped[2]; metric 0 onset, 1 onset+offset; the three are
 *     TP, n_ref, n_est; skipped = (ref, est) records not counted.  Row p < n_programs is instrument-aware: the notes of effective program
 *     p, matched only under the same pitch.  Row n_programs is instrument-agnostic: all pitched notes, keyed by pitch alone (drums have
 *     only their own row).  TP is the size of a MAXIMUM one-to-one matching of the hit graph, which is unique.
 *   - count pointers: ref_count_dev / est_count_dev (each may be NULL) are read ON THE DEVICE: the side then has min(n, max(*count, 0))
 *     records, and n only sizes the launches.  counts_dev[0] and notes_dev of ymt3_detokenize are an estimate in place: the host need
 *     not know how many notes were transcribed before the metrics are done.
 *   - kernels (yourmt3_amd/csrc/metrics.hip): one lane per record keys it and counts its keys; a scan and a scatter bucket the records'
 *     times by key; one wave per key sorts both buckets by onset, matches onsets with a two-pointer walk (a maximum matching, the hit
 *     intervals being monotone) and onset+offset by augmenting paths over an explicit stack.  No kernel waits on another workgroup and
 *     every search ends on any input; the cost is cubic in the notes of ONE key that lie within one onset window of each other.
 * ymt3_metrics_create: synchronous, like ymt3_detok_create; allocates all scratch (64 bytes per note of max_ref, 48 per note of max_est,
 * 24 per key).  Checks (YMT3_ERR_ARG naming the argument): params not NULL, the three tolerances finite and >= 0, n_programs >= 1,
 * drum_program in [0, n_programs), max_ref and max_est in [1, 2^24]; n_programs above 256 is YMT3_ERR_UNSUPPORTED.  The object belongs
 * to h; ymt3_metrics_destroy frees it (NULL is a no-op), before or after the handle's destruction.
 * ymt3_note_metrics: asynchronous on `stream`, allocates nothing, zeroes counts_dev first, leaves the handle's decode state alone.
 * YMT3_ERR_ARG, with handle and object still usable, for n_ref outside [0, max_ref], n_est outside [0, max_est], NULL counts_dev, or a
 * NULL or misaligned record pointer of a side with n > 0.  Either side may be empty.  One object serves one call at a time. */
typedef struct ymt3_metrics_params { double onset_tol, offset_min_tol, offset_ratio; int32_t n_programs, drum_program; } ymt3_metrics_params;
typedef struct ymt3_metrics_s* ymt3_metrics;
int  ymt3_metrics_create(ymt3_handle h, const ymt3_metrics_params* p, long long max_ref, long long max_est, ymt3_metrics* out);
void ymt3_metrics_destroy(ymt3_metrics m);
int  ymt3_note_metrics(ymt3_handle h, ymt3_metrics m,
                       const void* ref_notes_dev, long long n_ref, const int32_t* ref_count_dev /* may be NULL */,
                       const void* est_notes_dev, long long n_est, const int32_t* est_count_dev /* may be NULL */,
                       int32_t* counts_dev /* [(n_programs + 1) * 6 + 2] */, void* stream);

/* Device piano roll and frame metrics: a note set as a 0/1 roll, and frame-level F1 of an estimate against a reference -- how much of the
 * sounding (frame, pitch) area is right -- as integers (YourMT3.compile_piano_roll, piano_roll(), evaluate(frames=True); the
 * specification is the host path, piano_roll and frame_metrics of yourmt3_amd/metrics.py, which it reproduces exactly: every byte and
 * every integer).  The rules are this repository's own, shaped after the usual multi-pitch frame metric.  Records are the 32 bytes
 * { f64 onset, f64 offset, i32 program, i32 pitch, i32 is_drum, f32 score } of the device detokeniser, 8-byte aligned, in any order;
 * `score` is not read.
 *   - counted records: exactly the rule of the note metrics above (p = drum_program if is_drum != 0, else program; a record with
 *     p == drum_program is a drum note and counts even with a NaN offset); the others are skipped and appear in skipped[] only.
 *   - frame of a time: F(t) = rint(t * frames_per_second) in f64, that one multiply, round half to even (the tokeniser's step rule: at
 *     100 frames per second 0.57 * 100 = 56.99999999999999 lands on frame 57).
 *   - cells of a note: a pitched note sounds in frames [F(on), max(F(off), F(on) + 1)) clipped to [0, n_frames): it always shows in its
 *     onset frame, even when it is shorter than a frame or its offset lies before its onset.  A drum note sounds in [F(on), F(on) + 1),
 *     clipped; its offset is not read.  The clipping is done in f64 before any conversion to an integer: an onset of +inf gives no
 *     cell, an onset of -inf starts at frame 0, an offset of +inf ends at n_frames.
 *   - rows: those of the note metrics.  Row p < n_programs holds the notes of effective program p; row n_programs holds all pitched
 *     notes whatever their program (drums have only their own row).  A cell is a set member, not a count: overlapping or duplicate
 *     notes of one (row, pitch) sound once.
 *   - roll_dev: (n_rows, n_frames, 128) uint8 of 0 / 1 for the rows [first_row, first_row + n_rows), 16-byte aligned; every byte is
 *     written.
 *   - counts_dev: [(n_programs + 1) * 6 + 2] int64 = counts[row][6] then skipped[2].  With nr / ne the sounding pitches of reference /
 *     estimate in a frame and tp those sounding in both, the six are sums over the row's frames: TP = sum tp, N_REF = sum nr, N_EST =
 *     sum ne, SUB = sum (min(nr, ne) - tp), MISS = sum max(0, nr - ne), FA = sum max(0, ne - nr); skipped = (ref, est) records not counted.
 *   - count pointers: count_dev / ref_count_dev / est_count_dev (each may be NULL) are read ON THE DEVICE: the side then has
 *     min(n, max(*count, 0)) records, and n only sizes the launches (notes_dev and counts_dev[0] of ymt3_detokenize in place).
 *   - layout and kernels (yourmt3_amd/csrc/roll.hip): frame-major bit sets, one 16-byte word of 128 pitch bits per (side, row, frame).  A
 *     clear kernel zeroes the words in use; one wave per record sets its pitch bit in every frame of its interval with atomicOr; the
 *     metrics reduce one (row, frame) per lane with popc and one 64-bit atomicAdd per wave and non-zero counter; the roll call expands
 *     bits to bytes with 16-byte stores.  No kernel waits on another workgroup.
 * ymt3_roll_create: synchronous, like ymt3_metrics_create; allocates all scratch, 2 x (n_programs + 1) x max_frames x 16 bytes (about
 * 126 MB per side for 131 rows x 10 minutes at 100 frames per second).  Checks (YMT3_ERR_ARG naming the argument): params not NULL,
 * frames_per_second finite and > 0, n_programs >= 1, drum_program in [0, n_programs), max_frames in [1, 2^24]; n_programs above 256
 * is YMT3_ERR_UNSUPPORTED; a failed allocation is YMT3_ERR_HIP with nothing leaked and no object returned.  The object belongs to h;
 * ymt3_roll_destroy frees it (NULL is a no-op), before or after the handle's destruction.
 * ymt3_piano_roll / ymt3_frame_metrics: asynchronous on `stream`, allocate nothing, zero their output first, leave the handle's decode
 * state alone.  YMT3_ERR_ARG, with handle and object still usable, for n_frames outside [0, max_frames], a note count outside
 * [0, 2^29], NULL or misaligned roll_dev / counts_dev, a NULL or misaligned record pointer of a side with n > 0, or a row range outside
 * [0, n_programs] (n_rows >= 1).  n_frames = 0 gives zero counts, with skipped still counted, or an empty roll.  One object serves one
 * call at a time. */
typedef struct ymt3_roll_params { double frames_per_second; int32_t n_programs, drum_program; } ymt3_roll_params;
typedef struct ymt3_roll_s* ymt3_roll;
int  ymt3_roll_create(ymt3_handle h, const ymt3_roll_params* p, long long max_frames, ymt3_roll* out);
void ymt3_roll_destroy(ymt3_roll r);
int  ymt3_piano_roll(ymt3_handle h, ymt3_roll r, const void* notes_dev, long long n_notes, const int32_t* count_dev /* may be NULL */,
                     long long n_frames, int first_row, int n_rows, uint8_t* roll_dev /* (n_rows, n_frames, 128) */, void* stream);
int  ymt3_frame_metrics(ymt3_handle h, ymt3_roll r,
                        const void* ref_notes_dev, long long n_ref, const int32_t* ref_count_dev /* may be NULL */,
                        const void* est_notes_dev, long long n_est, const int32_t* est_count_dev /* may be NULL */,
                        long long n_frames, long long* counts_dev /* [(n_programs + 1) * 6 + 2] */, void* stream);

/* Device alignment: the monotone time map between a reference note set and an estimate, by banded dynamic time warping over frame-wise
 * pitch sets, and the reference carried onto the estimate's time axis (YourMT3.compile_aligner, align(), evaluate(align=True); the
 * specification is the host path, dtw_align and warp_notes of yourmt3_amd/metrics.py, which it reproduces exactly: every integer, and
 * every byte of the warped records, NaN payloads aside).  The rules are this repository's own.  Records are the 32 bytes of the device
 * detokeniser, 8-byte aligned, in any order; `score` is not read.
 *   - features: a side with n frames has 256 bits per frame: the instrument-agnostic row of the piano roll above (all pitched counted
 *     notes), then the drum row (row drum_program).  Counted records, F(t) = rint(t * frames_per_second), the one-frame rule, the
 *     clipping in f64 before any conversion to an integer and skipped[2] are the piano roll's rules, word for word.  The two sides have
 *     their OWN frame counts, n_ref_frames = Na and n_est_frames = Nb, each in [1, max_frames], max_frames <= 2^20.
 *   - cost: c(i, j) = popc(ref_i XOR est_j) over the 256 bits, the size of the symmetric difference: 0 ... 256.
 *   - band: with q = Na - 1, p = Nb - 1 and m = max(p, q, 1), cell (i, j) is in the band iff |i * p - j * q| <= band_frames * m, in
 *     int64; band_frames >= 1.  The rule is symmetric in the two sides; (0, 0) and (q, p) are always in the band.
 *   - recurrence: INF = 2^30.  D(0, 0) = c(0, 0); for every other in-band cell best = min(D(i-1, j-1), D(i-1, j), D(i, j-1)), a
 *     predecessor outside the rectangle or the band counting as INF, and D = min(best + c, INF).  The cell's step is the FIRST of
 *     (diagonal, (i-1, j), (i, j-1)) whose D equals best.  Out-of-band cells are INF.  A true cost stays below 2^29: int32 suffices.
 *   - path: the steps followed from (q, p) back to (0, 0), reported in forward order as (i, j) int32 pairs, path_len <= Na + Nb - 1;
 *     total = D(q, p); warp[i] = min { j : (i, j) on the path }, int32, non-decreasing, warp[0] = 0.  The path's last cell is (q, p), but
 *     warp[q] is the LOWEST j of the path in row q: warp[q] <= p, and < p whenever the path ends along the last row (any 1 x N call gives
 *     warp[0] = 0).  W therefore maps the reference's end to warp[q] / frames_per_second, not to the estimate's end.  If D(q, p) = INF
 *     (not known to occur) path_len = 0, every warp[i] = -1 and total = INF.
 *   - result_dev: [4] int64 = total, path_len, skipped ref, skipped est.  path_dev (may be NULL) is 8-byte aligned.
 *   - warping a time: W(t) in f64, each operation rounded once, nothing contracted: x = t * frames_per_second; k = floor(x) clamped to
 *     [0, q] in f64 before any conversion to an integer; f = x - k clamped to [0, 1]; a = warp[k], b = warp[min(k + 1, q)];
 *     W = (a + f * (b - a)) / frames_per_second.  A NaN stays NaN, -inf gives 0, a time at or past the end gives warp[q] /
 *     frames_per_second.  ymt3_warp_notes applies W to onset and offset of every record and copies program, pitch, is_drum and score: it
 *     filters nothing.  notes_out_dev may equal notes_dev.
 *   - count pointers (each may be NULL) are read ON THE DEVICE: the side then has min(n, max(*count, 0)) records.
 *   - layout and kernels (yourmt3_amd/csrc/align.hip): the dynamic programme is a tiled, skewed wavefront with the longer side on the
 *     lanes: one wave per tile of 256 x 64 cells, one launch per tile anti-diagonal, tiles wholly outside the band not run; a cell's
 *     three predecessors come from the lane's own register, one cross-lane move and the value moved the step before; tiles hand their
 *     last row, last column and last cell on through edge arrays in global memory.  Steps are 2 bits per cell, 16 consecutive cells of
 *     a column of the longer side per dword; one workgroup walks the path back tile by tile from LDS.  No kernel waits on another
 *     workgroup; the number of launches follows from the shapes alone.
 * ymt3_aligner_create: synchronous; allocates all scratch.  With B = min(band_frames, max_frames) (a wider band changes no cell) and
 * M = max_frames, in bytes: features 64 x M, step bits 4 x M x (B / 8 + 2), reversed path 8 x (2 x M - 1), edges about 8 x M + M / 12:
 * 60 000 frames under a band of 3000 take about 95 MB.  Checks (YMT3_ERR_ARG naming the argument): params not NULL, frames_per_second
 * finite and > 0, n_programs >= 1, drum_program in [0, n_programs), band_frames >= 1, max_frames in [1, 2^20]; n_programs above 256 is
 * YMT3_ERR_UNSUPPORTED; a failed allocation is YMT3_ERR_HIP with nothing leaked and no object returned.  The object belongs to h;
 * ymt3_aligner_destroy frees it (NULL is a no-op), before or after the handle's destruction.
 * ymt3_align_notes / ymt3_warp_notes: asynchronous on `stream`, allocate nothing, leave the handle's decode state alone.  YMT3_ERR_ARG,
 * with handle and object still usable, for a frame count outside [1, max_frames], a note count outside [0, 2^29], NULL or misaligned
 * warp_dev / result_dev, a misaligned path_dev, or a NULL or misaligned record pointer with n > 0.  One object serves one call at a
 * time. */
typedef struct ymt3_align_params { double frames_per_second; int32_t n_programs, drum_program, band_frames; } ymt3_align_params;
typedef struct ymt3_aligner_s* ymt3_aligner;
int  ymt3_aligner_create(ymt3_handle h, const ymt3_align_params* p, long long max_frames, ymt3_aligner* out);
void ymt3_aligner_destroy(ymt3_aligner a);
int  ymt3_align_notes(ymt3_handle h, ymt3_aligner a,
                      const void* ref_notes_dev, long long n_ref, const int32_t* ref_count_dev /* may be NULL */, long long n_ref_frames,
                      const void* est_notes_dev, long long n_est, const int32_t* est_count_dev /* may be NULL */, long long n_est_frames,
                      int32_t* warp_dev /* [n_ref_frames] */, int32_t* path_dev /* may be NULL; [(n_ref_frames + n_est_frames - 1) * 2] */,
                      long long* result_dev /* [4]: total, path_len, skipped ref, skipped est */, void* stream);
int  ymt3_warp_notes(ymt3_handle h, ymt3_aligner a, const void* notes_dev, long long n_notes, const int32_t* count_dev /* may be NULL */,
                     const int32_t* warp_dev, long long n_ref_frames, void* notes_out_dev, void* stream);

/* Note velocities from the audio: how loud is each note at its onset, as a MIDI velocity (YourMT3.compile_note_velocity,
 * transcribe(velocity=True), estimate_velocities(); the specification is the host path, note_velocities of yourmt3_amd/velocity.py, in
 * f64).  The vocabulary carries no dynamics, so the level is measured where it is: in the audio ymt3_ingest left on the device, under
 * each record of the device detokeniser.  The rules are this repository's own.  Records are the 32 bytes { f64 onset, f64 offset, i32
 * program, i32 pitch, i32 is_drum, f32 score } of the device detokeniser, 8-byte aligned, in any order; offset and score are not read.
 *   - audio: audio_dev[0 .. n_audio) f32 mono at params.sample_rate, which must be cfg.sample_rate (the (n_segments, segment_samples)
 *     buffer of ymt3_ingest, read flat).  Samples outside the range read as 0.
 *   - tables, built in f64 by ymt3_velocity_create: the window w[k] = f32(0.5 - 0.5 cos(2 pi (k + 0.5) / W)), W = window_samples, and the
 *     phase steps step[p][h - 1] = uint32(rint(h f(p) / sr * 2^32)), f(p) = 440 * 2^((p - 69) / 12), h = 1 .. n_harmonics, kept only where
 *     h f(p) < sr / 2 and 0 ("absent") elsewhere.
 *   - measured records: the onset is finite, the pitch lies in [0, 128), and the record is a drum (is_drum != 0 or program ==
 *     drum_program) or f(pitch) < sr / 2.  Every other record gets default_velocity and the energy NaN and is counted in counts[1];
 *     measured records are counted in counts[0].
 *   - window position: n0 = rint(onset * sr) in f64, that one multiply, round half to even (the roll's frame rule).  The window is
 *     always the W samples from n0, whatever the note's offset.  The clamp is done in f64 before any conversion to an integer: a window
 *     wholly outside the audio (an onset of 1e300) is all zeros, one that crosses an end reads zeros beyond it.
 *   - energy, with a[k] = w[k] x[n0 + k]: the window power P = 2 sum a^2 / sum w^2; a drum has E = P; a pitched note has E = 4 sum_h
 *     |sum_k a[k] e^(-i theta)|^2 / (sum w)^2 over the harmonics present, theta = phi 2 pi / 2^32 with the exact integer phase word phi =
 *     (step * k) mod 2^32, relative to the window start.  A steady sinusoid of amplitude A at f(p) gives E ~ A^2.  A non-finite E (a NaN
 *     or infinite sample under the window) makes the record unmeasured after all: default_velocity, counts[1], kept out of the peak.
 *   - peaks_dev: [2] f32 = the largest E over the measured pitched records, and over the measured drums; 0 for an empty class.
 *   - velocity: u = peak_velocity + velocity_per_db * (10 log10(max(E, 1e-12)) - 10 log10(max(ref, 1e-12))) in f64, ref being the peak of
 *     the record's class or, with a finite peak_db (an absolute level in dB re full scale; NaN: relative to the loudest measured note
 *     of this call), 10^(peak_db / 10) for both classes; velocity = clamp(rint(u), min_velocity, 127).
 *   - precision: the device sums in f32 and in another order than the specification, and takes sine and cosine from the integer phase
 *     word in f32.  Exact: counts, the measured / unmeasured split, the bytes of unmeasured records and of records beyond the count.
 *     Energies and peaks agree with the f64 specification within tau * max(P, 1e-12), tau as measured in DESIGN section 21; a velocity
 *     is the specification's wherever that interval rounds to one value.  Samples so large that sum a^2 leaves the f32 range count
 *     as non-finite.
 *   - count pointer: count_dev (may be NULL) is read ON THE DEVICE: min(n_notes, max(*count, 0)) records are live and n_notes only sizes
 *     the launches (notes_dev and counts_dev[0] of ymt3_detokenize in place).  Every byte of velocity_dev[0 .. n_notes) is written;
 *     records at or beyond the count get velocity 0 (and energy NaN).
 *   - kernels (yourmt3_amd/csrc/velocity.hip): one wave per record strides the window (coalesced rows of audio; overlapping notes meet
 *     in L2), keeps per lane the f32 power and the real and imaginary sums of each harmonic, finishes them with a shuffle butterfly in a
 *     fixed order, raises its class's peak with atomicMax on the bits of the non-negative finite f32 and bumps a counter; then one lane
 *     per record maps E to the velocity in f64.  With energy_dev = NULL there is nowhere to keep E, and the second kernel measures again
 *     (the same bits) before it maps.  No kernel waits on another workgroup.
 * ymt3_velocity_create: synchronous; builds and uploads the two tables (4 * window_samples + 4 KB).  Checks (YMT3_ERR_ARG naming the
 * argument): params not NULL, sample_rate == cfg.sample_rate, window_samples in [64, 4096], n_harmonics in [1, 8], velocity_per_db finite
 * and > 0, peak_velocity in [1, 127], min_velocity in [1, peak_velocity], default_velocity in [1, 127], peak_db finite or NaN,
 * drum_program >= 0.  The object belongs to h; ymt3_velocity_destroy frees it (NULL is a no-op), before or after the handle's destruction.
 * ymt3_note_velocities: asynchronous on `stream`, allocates nothing, zeroes peaks_dev and counts_dev first, leaves the handle's decode state
 * alone.  YMT3_ERR_ARG, with handle and object still usable, for n_audio < 0, a NULL audio_dev with n_audio > 0, n_notes outside
 * [0, 2^29], a NULL notes_dev or velocity_dev with n_notes > 0, NULL peaks_dev or counts_dev, a notes_dev not aligned to 8 bytes or an
 * audio_dev, count_dev, energy_dev, peaks_dev or counts_dev not aligned to 4.  n_notes = 0 only zeroes the outputs.  The object keeps no
 * state between calls: several calls may be in flight on one object. */
typedef struct ymt3_velocity_params {
    double  velocity_per_db, peak_db;
    int32_t sample_rate, window_samples, n_harmonics, peak_velocity, min_velocity, default_velocity, drum_program;
} ymt3_velocity_params;
typedef struct ymt3_velocity_s* ymt3_velocity;
int  ymt3_velocity_create(ymt3_handle h, const ymt3_velocity_params* params, ymt3_velocity* out);
void ymt3_velocity_destroy(ymt3_velocity v);
int  ymt3_note_velocities(ymt3_handle h, ymt3_velocity v, const float* audio_dev, long long n_audio, const void* notes_dev, long long n_notes,
                          const int32_t* count_dev /* may be NULL */, uint8_t* velocity_dev, float* energy_dev /* may be NULL */,
                          float* peaks_dev /* [2] */, int32_t* counts_dev /* [2] */, void* stream);

/* ---- beat tracking over note records ------------------------------------------------------------------------------------------
 * The vocabulary carries no metre; the notes do: their onsets are an onset-strength signal.  A ymt3_beats object finds a tempo per
 * window and the beats' frames from records on the device, and gives every record its position in beats, as MIDI ticks.  The rules are
 * this project's own (an autocorrelation tempogram and a dynamic-programming beat tracker); the host specification is
 * track_beats / beat_positions of yourmt3_amd/beats.py, and every output equals it bit for bit: everything is an integer, the two tables
 * are built on the host in f64, and the position is one f64 expression without contraction.  Integer divisions below are floor divisions.
 *
 * Parameters (ymt3_beats_create refuses, YMT3_ERR_ARG, what is outside): frames_per_second, bpm_min <= bpm_max, bpm_prior, prior_octaves,
 * tightness (<= 10000): finite and > 0; lag_min = ceil(60 fps / bpm_max) and lag_max = floor(60 fps / bpm_min) with
 * 4 <= lag_min <= lag_max <= 512; 2 lag_max <= window_frames (Wn) <= 2048; 1 <= hop_frames (Hn) <= Wn; 0 <= lag_step_max (D) <= 512;
 * 1 <= onset_cap <= 255; 1 <= n_programs <= 256, drum_program in [0, n_programs); 1 <= max_frames <= 2^20, and
 * ceil(max_frames / Hn) Wn (4 onset_cap)^2 65535 <= 2^62, which bounds every int64 sum below.
 *   tables    prior[L] = rint(65535 exp(-0.5 (log2(L / L0) / prior_octaves)^2)), L0 = 60 fps / bpm_prior;
 *             pen[t][d] = rint(tightness 1024 ln(d / t)^2) for t in [lag_min, lag_max], d in [ceil(t / 2), 2 t].
 *   envelope  a record counts by the rule of the note metrics (NaN onset, pitch outside [0, 128), program outside [0, n_programs), a
 *             pitched note with a NaN offset: skipped).  A counted record adds 1 to e[F], F = rint(onset fps) in f64, if 0 <= F < n_frames.
 *             e[f] = min(e[f], onset_cap); s[f] = e[f-1] + 2 e[f] + e[f+1], zeros outside [0, n_frames).
 *   tempogram nW = max(1, ceil(n_frames / Hn)); window w: c = w Hn + Hn / 2, f in [c - Wn / 2, c + Wn / 2) within [0, n_frames);
 *             A[w][L] = sum of s[f] s[f+L] over the window's f with f + L < n_frames; T[w][L] = A[w][L] prior[L].
 *   tempo     V[0] = T[0]; V[w][L] = T[w][L] + max of V[w-1][L'] over |L' - L| <= D inside the lag range, ties to the nearest L', then
 *             the smaller.  The end is the smallest L with V[nW-1][L] maximal; tempo[w] is the lag followed back from it.
 *   beats     t(f) = tempo[min(f / Hn, nW - 1)]; best(f) = max of C[p] - pen[t][f-p] over p in [max(0, f - 2 t), f - ceil(t / 2)]; with
 *             best > 0 back[f] is the LARGEST such p, else best = 0 and back[f] = -1; C[f] = 1024 s[f] + best.  The last beat is the
 *             SMALLEST f with C[f] maximal; the beats are the chain of back[] from it, ascending; max C = 0: no beats.
 * ymt3_track_beats: notes_dev / n_notes / count_dev as in the note metrics.  beats_dev[0 .. n_beats) are written, the rest is left alone;
 * max_beats >= n_frames / ceil(lag_min / 2) + 1 is required.  tempo_dev (may be NULL): nW lags, frames per beat.  result_dev[4]: n_beats,
 * max C, the maximum of V's last row, skipped records.
 * ymt3_beat_positions: ticks_dev[i] = {onset tick, offset tick} of record i at 480 ticks per beat; the number of beats K is read from
 * result_dev[0] on the device.  With K >= 2: x = t fps, i the largest index with b[i] <= x clamped to [0, K-2],
 * n0 = ceil(b[0] / (b[1] - b[0])), pos = (n0 + i) + (x - b[i]) / (b[i+1] - b[i]); Q = divisions, or 480 for divisions = 0 (divisions
 * divides 480); tick = clamp(rint(pos Q), 0, 2^20) (480 / Q), rint half to even.  With K < 2: tick = clamp(rint(t 960), 0, 2^29) and Q = 480.
 * A counted pitched record's offset tick is at least its onset tick + 480 / Q.  A NaN time, an uncounted record, a record at or beyond
 * the count: -1.  Every entry of ticks_dev is written.
 * Both calls are asynchronous on `stream`, allocate nothing, read nothing back and leave the handle's decode state alone.  The object's
 * scratch is used by ymt3_track_beats: calls on one object are ordered by their stream.  Bars, the time signature, downbeats and the
 * key are the next section's (ymt3_track_bars). */
typedef struct ymt3_beat_params {
    double  frames_per_second, bpm_min, bpm_max, bpm_prior, prior_octaves, tightness;
    int32_t window_frames, hop_frames, lag_step_max, onset_cap, n_programs, drum_program;
} ymt3_beat_params;
typedef struct ymt3_beats_s* ymt3_beats;
int  ymt3_beats_create(ymt3_handle h, const ymt3_beat_params* params, long long max_frames, ymt3_beats* out);
void ymt3_beats_destroy(ymt3_beats b);
int  ymt3_track_beats(ymt3_handle h, ymt3_beats b, const void* notes_dev, long long n_notes, const int32_t* count_dev /* may be NULL */,
                      long long n_frames, int32_t* beats_dev, long long max_beats, int32_t* tempo_dev /* may be NULL */,
                      long long* result_dev /* [4] */, void* stream);
int  ymt3_beat_positions(ymt3_handle h, ymt3_beats b, const int32_t* beats_dev, const long long* result_dev, const void* notes_dev,
                         long long n_notes, const int32_t* count_dev /* may be NULL */, int divisions, int32_t* ticks_dev /* [n_notes][2] */,
                         void* stream);

/* ---- bars and key over note records and tracked beats --------------------------------------------------------------------------
 * The beats give a tick a position; a ymt3_bars object gives every beat its metre and its place in the bar (so: the downbeats and the
 * time signatures) and the file one key, from the records and the beats where ymt3_track_beats left them.  The rules are this project's
 * own; the host specification is track_bars of yourmt3_amd/bars.py, and every output equals it bit for bit:
 * everything is an integer, and times stay f64 until they are known to lie inside the slots or the frames.  Integer divisions below are
 * floor divisions.
 *
 * Parameters (ymt3_bars_create refuses, YMT3_ERR_ARG, what is outside): frames_per_second finite and > 0; metres[0 .. n_metres), 1 to 5
 * distinct values in [2, 6], their order being the tie order; near_div (nd) in [2, 64]; accent_cap in [1, 255]; w_long, w_kick in
 * [0, 15]; 0 <= kick_lo <= kick_hi <= 127; w_accent in [0, 1024]; switch_cost in [0, 4096]; 1 <= n_programs <= 256, drum_program in
 * [0, n_programs); max_beats in [1, 2^20 + 1]; max_notes in [1, 2^20], which keeps a chroma cell inside 32 bits.
 *   slots     K beats b (K is read from beat_result_dev[0] on the device, clamped to [0, max_beats]).  With K >= 2: D[i] = b[i+1] - b[i],
 *             D[K-1] = D[K-2]; lo[0] = b[0] - D[0] / nd, lo[i] = b[i] - D[i-1] / nd; hi[i] = lo[i+1], hi[K-1] = b[K-1] + D[K-1] - D[K-1] / nd.
 *   accent    a record counts by the rule of the note metrics; the others are skipped.  F = rint(onset fps) in f64.  A counted record
 *             with F inside slot i and F <= b[i] + D[i] / nd adds to a[i]: 1, + w_kick for a drum with pitch in [kick_lo, kick_hi],
 *             + w_long for a pitched record with F(offset) - F >= D[i] (f64).  a[i] = min(a[i], accent_cap).
 *   chroma    a counted pitched record's span [F(on), max(F(off), F(on) + 1)) clipped to [0, n_frames) adds the frames it shares with
 *             slot i to c[i][pitch mod 12], for every slot it overlaps.  sum[i] = sum of c[i]; n[i][pc] = c[i][pc] 1024 / sum[i];
 *             h[0] = 0, h[i] = sum over pc of |n[i][pc] - n[i-1][pc]| if both sums are positive, else 0.
 *   salience  d[i] = w_accent a[i] + h[i]; mean_d = (sum of d) / K.
 *   bar path  states (m, k), m in metres' order, k = 0 .. m-1, k = 0 the downbeat; r(i, m, 0) = (60 / m) (m - 1) d[i],
 *             r(i, m, k > 0) = -(60 / m) d[i].  V[0][(m, k)] = r(0, m, k); V[i][(m, k > 0)] = V[i-1][(m, k-1)] + r;
 *             V[i][(m, 0)] = max(V[i-1][(m, m-1)], max over m' != m of V[i-1][(m', m'-1)] - switch_cost 60 mean_d) + r, ties to staying,
 *             then to the earliest m'.  The end is the first state in state order with V[K-1] maximal; the path is followed back.
 *   key       tot[pc] = sum over i of c[i][pc]; S[mode][t] = sum over pc of tot[pc] T_mode[(pc - t) mod 12] with the two tables of
 *             yourmt3_amd/bars.py (KEY_MAJOR, KEY_MINOR); key = 12 mode + t of the maximum, major before minor, then the smaller t; -1
 *             if the sum of tot is 0.
 * ymt3_track_bars: beats_dev / beat_result_dev as ymt3_track_beats wrote them; notes_dev / n_notes / count_dev as there, n_notes at most
 * the object's max_notes.  metre_dev[i] = 256 m + k for i < K, the rest is left alone; max_beats, its length, is at least the object's.
 * result_dev[8]: n_downbeats, max V[K-1], mean_d, key, the best S, the second-best S, skipped records, 0.  With K < 2 nothing is written
 * to metre_dev and result_dev = {0, 0, 0, -1, 0, 0, skipped, 0}.
 * Asynchronous on `stream`, allocates nothing, reads nothing back and leaves the handle's decode state alone.  The object's scratch is
 * used by the call: calls on one object are ordered by their stream.  YMT3_ERR_ARG, with handle and object still usable, for a NULL or
 * misaligned beats_dev, beat_result_dev, metre_dev or result_dev, a NULL notes_dev with n_notes > 0, a misaligned notes_dev or count_dev,
 * n_notes outside [0, max_notes], n_frames outside [1, 2^20], max_beats below the object's.  One key per file and the denominator 4:
 * modulations and compound metres are out of scope. */
typedef struct ymt3_bar_params {
    double  frames_per_second;
    int32_t n_metres, metres[5];
    int32_t near_div, accent_cap, w_long, w_kick, kick_lo, kick_hi, w_accent, switch_cost, n_programs, drum_program;
} ymt3_bar_params;
typedef struct ymt3_bars_s* ymt3_bars;
int  ymt3_bars_create(ymt3_handle h, const ymt3_bar_params* params, long long max_beats, long long max_notes, ymt3_bars* out);
void ymt3_bars_destroy(ymt3_bars b);
int  ymt3_track_bars(ymt3_handle h, ymt3_bars b, const int32_t* beats_dev, const long long* beat_result_dev, const void* notes_dev,
                     long long n_notes, const int32_t* count_dev /* may be NULL */, long long n_frames, int32_t* metre_dev, long long max_beats,
                     long long* result_dev /* [8] */, void* stream);

/* ---- chords over note records and tracked beats -----------------------------------------------------------------------------------
 * A ymt3_chords object gives every beat one chord, (quality, root) or N, from the records and the beats where ymt3_track_beats left
 * them, and optionally the metre ymt3_track_bars wrote.  The rules are this project's own, UNVERIFIED against any
 * package; the host specification is track_chords of yourmt3_amd/chords.py, and every output equals it bit for bit: everything is an
 * integer, and times stay f64 until they are known to lie inside the frames.  Integer divisions below are floor divisions.
 *
 * Parameters (ymt3_chords_create refuses, YMT3_ERR_ARG, what is outside): frames_per_second finite and > 0; qualities[0 .. n_qualities),
 * 1 to 8 distinct indices of the fixed table, their order being the state order and so the tie order; near_div (nd) in [2, 64];
 * bass_div in [1, 64]; w_bass, w_none in [0, 1024]; change_cost, change_cost_down in [0, 4096]; 1 <= n_programs <= 256, drum_program in
 * [0, n_programs); reserved is ignored; max_beats in [1, 2^20 + 1]; max_notes in [1, 2^20].
 *   table     q: 0 maj {0,4,7}, 1 min {0,3,7}, 2 dim {0,3,6}, 3 aug {0,4,8}, 4 sus4 {0,5,7}, 5 "7" {0,4,7,10}, 6 maj7 {0,4,7,11},
 *             7 min7 {0,3,7,10}; W_q = 591 for three tones, 512 for four (1024 / sqrt(n)).
 *   slots     the bars': K beats b (K is read from beat_result_dev[0] on the device, clamped to [0, max_beats]); with K >= 2:
 *             D[i] = b[i+1] - b[i], D[K-1] = D[K-2]; lo[0] = b[0] - D[0] / nd, lo[i] = b[i] - D[i-1] / nd; hi[i] = lo[i+1],
 *             hi[K-1] = b[K-1] + D[K-1] - D[K-1] / nd.
 *   chroma    the bars': a counted pitched record's span [F(on), max(F(off), F(on) + 1)) clipped to [0, n_frames) adds the frames it
 *             shares with slot i to c[i][pitch mod 12], for every slot it overlaps.  n[i][pc] = c[i][pc] 1024 / max(sum of c[i], 1) (64 bits).
 *   bass      bass[i] = the smallest pitch among the counted pitched records whose share with slot i satisfies
 *             bass_div share >= hi[i] - lo[i]; 255 with none.
 *   states    (q, r), q in qualities' order, r = 0 .. 11, then N last: S = 12 n_qualities + 1 <= 97.
 *   emission  e[i][(q, r)] = W_q (sum over s in the intervals of q of n[i][(r + s) mod 12]) + (1024 w_bass if bass[i] < 128 and
 *             bass[i] mod 12 = r); e[i][N] = 1024 w_none; e < 2^21.
 *   path      V[0] = e[0].  For i >= 1: j* = the first state with V[i-1] maximal; P_i = 1024 change_cost_down if metre_dev is given and
 *             metre_dev[i] & 255 = 0, else 1024 change_cost; jump = V[i-1][j*] - P_i; state s stays if V[i-1][s] >= jump, else it comes
 *             from j*; V[i][s] = max(V[i-1][s], jump) + e[i][s] (0 <= V < 2^42).  The end is the first state with V[K-1] maximal; the
 *             path is followed back.
 * ymt3_track_chords: beats_dev / beat_result_dev as ymt3_track_beats wrote them; metre_dev as ymt3_track_bars wrote it (at least K
 * entries), or NULL; notes_dev / n_notes / count_dev as there, n_notes at most the object's max_notes.  chord_dev[i] = 256 bass[i] +
 * label for i < K, the rest is left alone; label = 12 q + r with q the table's index, 255 for N; chord_cap, its length, is at least the
 * object's max_beats.  result_dev[8]: the number of runs of equal label, max V[K-1], the number of N beats, skipped records, 0, 0, 0, 0.
 * With K < 2 nothing is written to chord_dev and result_dev = {0, 0, 0, skipped, 0, 0, 0, 0}.
 * Asynchronous on `stream`, allocates nothing, reads nothing back and leaves the handle's decode state alone.  The object's scratch
 * (68 bytes per beat) is used by the call: calls on one object are ordered by their stream.  YMT3_ERR_ARG, with handle and object
 * still usable, for a NULL or misaligned beats_dev, beat_result_dev, chord_dev or result_dev, a misaligned metre_dev, a NULL notes_dev
 * with n_notes > 0, a misaligned notes_dev or count_dev, n_notes outside [0, max_notes], n_frames outside [1, 2^20], chord_cap below the
 * object's max_beats.  One chord per beat at the finest; chords beyond the table are out of scope. */
typedef struct ymt3_chord_params {
    double  frames_per_second;
    int32_t n_qualities, qualities[8];
    int32_t near_div, bass_div, w_bass, w_none, change_cost, change_cost_down, n_programs, drum_program, reserved;
} ymt3_chord_params;
typedef struct ymt3_chords_s* ymt3_chords;
int  ymt3_chords_create(ymt3_handle h, const ymt3_chord_params* params, long long max_beats, long long max_notes, ymt3_chords* out);
void ymt3_chords_destroy(ymt3_chords c);
int  ymt3_track_chords(ymt3_handle h, ymt3_chords c, const int32_t* beats_dev, const long long* beat_result_dev,
                       const int32_t* metre_dev /* may be NULL */, const void* notes_dev, long long n_notes,
                       const int32_t* count_dev /* may be NULL */, long long n_frames, int32_t* chord_dev, long long chord_cap,
                       long long* result_dev /* [8] */, void* stream);

/* ---- sections over note records and tracked beats ---------------------------------------------------------------------------------
 * A ymt3_sections object gives the beats their form: where a new section starts, and one letter per section, equal for sections that
 * repeat, from the records and the beats where ymt3_track_beats left them, and optionally the metre ymt3_track_bars wrote.  The rules
 * are this project's own, UNVERIFIED against any package; the host specification is track_sections of
 * yourmt3_amd/sections.py, and every output equals it bit for bit: everything is an integer, and times stay f64 until they are known to
 * lie inside the frames.  Integer divisions below are floor divisions.
 *
 * Parameters (ymt3_sections_create refuses, YMT3_ERR_ARG, what is outside): frames_per_second finite and > 0; near_div (nd) in [2, 64];
 * 1 <= n_programs <= 256, drum_program in [0, n_programs); context (w) in [1, 16]; kernel_beats (L) in [2, 64]; min_len (m) in [1, 256];
 * peak_div in [1, 1024]; same_dist in [0, 32768]; len_num in [1, 16]; max_sections (M) in [1, 64]; max_beats in [1, 2^20 + 1];
 * max_notes in [1, 2^20].
 *   chroma      the bars' and the chords' c[i][pc] over the bars' slots (K beats, K read from beat_result_dev[0] on the device and
 *               clamped to [0, max_beats]); n[i][pc] = c[i][pc] 1024 / max(sum of c[i], 1) (64 bits); empty[i] = (sum of c[i] = 0).
 *   context     f[i][pc] = sum over d < w of n[min(i + d, K - 1)][pc]; the sum of f[i] is at most 1024 w.
 *   similarity  D(i, j) = sum over pc of |f[i][pc] - f[j][pc]| <= 2048 w <= 32768; S(i, j) = 2048 w - D(i, j) >= 0.
 *   novelty     L_i = min(L, i, K - i), t[u] = L - u; nov[i] = sum over u, v < L_i of t[u] t[v] (S(i-1-u, i-1-v) + S(i+u, i+v)
 *               - S(i-1-u, i+v) - S(i+u, i-1-v)), signed, 64 bits; nov[0] = 0.  The quadrants are cut alike at the ends, nothing is
 *               zero-padded.  The sum of t[u] t[v] is at most (64 65 / 2)^2 < 2^23 per quadrant and S < 2^16: |nov| < 2^41.
 *   boundaries  candidates C: every i in [1, K), with metre_dev only those with metre_dev[i] & 255 = 0; top = the largest nov among C (0
 *               if C is empty).  i in C is a peak if nov[i] > 0, peak_div nov[i] >= top, and no j in C with 0 < |j - i| <= m has the
 *               larger key (nov[j], -j): a larger novelty, or an equal one at a smaller index.  Of more than M - 1 peaks the M - 1 with
 *               the largest key are kept.  Section starts: beat 0 and the kept peaks in time order; section s is [a_s, a_{s+1}), a_n = K.
 *   labels      a section whose beats are all empty is silent: label 255, it neither takes nor gives a letter.  For two others,
 *               m_st = min(len_s, len_t), d(s, t) = (sum over k < m_st of D(a_s + k, a_t + k)) / m_st (the sum is below 2^35); they are
 *               the same if len_num m_st >= max(len_s, len_t) and d(s, t) <= same_dist.  In time order, s takes the label of the
 *               earliest earlier non-silent t that is the same as it, else the next unused label from 0.
 * ymt3_track_sections: beats_dev / beat_result_dev as ymt3_track_beats wrote them; metre_dev as ymt3_track_bars wrote it (at least K
 * entries), or NULL; notes_dev / n_notes / count_dev as there, n_notes at most the object's max_notes.  section_dev[i] = 65536 start +
 * 256 s + label for i < K (start = 1 on a section's first beat), the rest is left alone; section_cap, its length, is at least the
 * object's max_beats.  novelty_dev[i] = nov[i] for i < K, or NULL (at least max_beats entries otherwise).  result_dev[8]: the number of
 * sections, the number of distinct letters, top, skipped records, the number of peaks before the cap, the number of silent sections, 0,
 * 0.  With K < 2 nothing is written to section_dev or novelty_dev and result_dev = {0, 0, 0, skipped, 0, 0, 0, 0}.
 * Asynchronous on `stream`, allocates nothing, reads nothing back and leaves the handle's decode state alone.  The object's scratch
 * (89 bytes per beat and 4 KiB) is used by the call: calls on one object are ordered by their stream.  YMT3_ERR_ARG, with handle and
 * object still usable, for a NULL or misaligned beats_dev, beat_result_dev, section_dev or result_dev, a misaligned metre_dev or
 * novelty_dev, a NULL notes_dev with n_notes > 0, a misaligned notes_dev or count_dev, n_notes outside [0, max_notes], n_frames outside
 * [1, 2^20], section_cap below the object's max_beats.  Sections are compared beat by beat along their diagonal: the same chords in
 * another order are another section; transposed repeats and functional names are out of scope. */
typedef struct ymt3_section_params {
    double  frames_per_second;
    int32_t near_div, n_programs, drum_program, context, kernel_beats, min_len, peak_div, same_dist, len_num, max_sections;
} ymt3_section_params;
typedef struct ymt3_sections_s* ymt3_sections;
int  ymt3_sections_create(ymt3_handle h, const ymt3_section_params* params, long long max_beats, long long max_notes, ymt3_sections* out);
void ymt3_sections_destroy(ymt3_sections c);
int  ymt3_track_sections(ymt3_handle h, ymt3_sections c, const int32_t* beats_dev, const long long* beat_result_dev,
                         const int32_t* metre_dev /* may be NULL */, const void* notes_dev, long long n_notes,
                         const int32_t* count_dev /* may be NULL */, long long n_frames, int32_t* section_dev, long long section_cap,
                         long long* novelty_dev /* may be NULL */, long long* result_dev /* [8] */, void* stream);

/* ---- hands over note records -------------------------------------------------------------------------------------------------------
 * A ymt3_hands object gives every note of the piano programs a hand, from the records where ymt3_detokenize left them: at every onset
 * slice the keyboard is cut at a split point, and the split points of the piece are one cheapest path.  It needs no beats.  The rules
 * are this project's own, UNVERIFIED against any package; the host specification is split_hands of
 * yourmt3_amd/hands.py, and every output equals it bit for bit: everything is an integer, and times stay f64 until they are known to
 * lie inside the frames.  Integer divisions below are floor divisions.
 *
 * Parameters (ymt3_hands_create refuses, YMT3_ERR_ARG, what is outside): frames_per_second finite and > 0; slice_frames in [1, 64];
 * span in [1, 127]; cut_min in [0, 127]; middle and mid_free in [0, 128]; every w_* in [0, 1024]; rest_slots in [1, 2^20];
 * 1 <= n_programs <= 256, drum_program in [0, n_programs); 0 <= program_lo <= program_hi < n_programs; max_frames in [1, 2^20];
 * max_notes in [1, 2^20].
 *   selected    a record the note rule counts (ymt3_note_metrics), not a drum, program_lo <= program <= program_hi, whose span
 *               [F(on), max(F(off), F(on) + 1)) clipped to [0, n_frames) is not empty; its slot q = (the span's first frame) / slice_frames.
 *   slices      the occupied slots in ascending order, t = 0 .. T-1, Q_t the slot, P_t the SET of pitches selected into it.
 *   states      s in [0, 128]: L = {p in P_t : p < s}, R = {p in P_t : p >= s}; span(X) = max X - min X, 0 for an empty X;
 *               class_t(s) = 0 if L is empty, 2 if R is empty, 1 otherwise.
 *   emission    e_t(s) = w_span (max(0, span(L) - span) + max(0, span(R) - span)) + cut_t(s) + w_mid max(0, |s - middle| - mid_free);
 *               cut_t(s) = w_cut max(0, cut_min - (min R - max L)) + w_centre (|2 s - (max L + min R + 1)| / 2) where class_t(s) = 1, else 0.
 *   transition  x_t(s', s) = 0 if Q_t - Q_{t-1} >= rest_slots, else w_move |s - s'| + w_switch [{class_{t-1}(s'), class_t(s)} = {0, 2}].
 *   path        C_0 = e_0; C_t(s) = e_t(s) + min over s' of (C_{t-1}(s') + x_t(s', s)), back_t(s) the SMALLEST minimiser; s_{T-1} the
 *               smallest minimiser of C_{T-1}, s_{t-1} = back_t(s_t); total = min C_{T-1} (64 bits; e <= 454 656 and x <= 132 096, so
 *               a step's costs lie within 2^20 of each other).
 * ymt3_split_hands: notes_dev / n_notes / count_dev as ymt3_track_beats takes them, n_notes at most the object's max_notes; n_frames
 * in [1, max_frames].  hand_dev[i] for i below the live count: 1 (right) if the record's pitch >= s_t of its slice, 0 (left) otherwise,
 * 255 if it is not selected; the rest is left alone.  split_dev[t] = 256 Q_t + s_t for t < T, or NULL; max_slices, its length, is at
 * least min(n_notes, ceil(n_frames / slice_frames)).  result_dev[8]: T, selected records, left records, right records, total, skipped
 * records (those the note rule does not count), hand-overs on the path (the t >= 1 with Q_t - Q_{t-1} < rest_slots and
 * {class_{t-1}(s_{t-1}), class_t(s_t)} = {0, 2}), 0.  With T = 0 every live hand is 255 and result_dev = {0, 0, 0, 0, 0, skipped, 0, 0}.
 * Asynchronous on `stream`, allocates nothing, reads nothing back (T stays on the device) and leaves the handle's decode state alone.
 * The object's scratch (20 bytes per slot of ceil(max_frames / slice_frames), 153 bytes per slice of min(max_notes, slots)) is used by
 * the call: calls on one object are ordered by their stream.  YMT3_ERR_ARG, with handle and object still usable, for n_notes outside
 * [0, max_notes], a NULL notes_dev or hand_dev with n_notes > 0, a misaligned notes_dev, count_dev, split_dev or result_dev, n_frames
 * outside [1, max_frames], max_slices too small for a split_dev that is given, a NULL result_dev.  Sounding notes are not held across
 * slices, there are two voices and no more, and only the program range is split. */
typedef struct ymt3_hand_params {
    double  frames_per_second;
    int32_t slice_frames, program_lo, program_hi, span, w_span, cut_min, w_cut, w_centre, middle, mid_free, w_mid, w_move, w_switch, rest_slots,
            n_programs, drum_program;
} ymt3_hand_params;                                                         /* 72 bytes, no padding */
typedef struct ymt3_hands_s* ymt3_hands;
int  ymt3_hands_create(ymt3_handle h, const ymt3_hand_params* params, long long max_frames, long long max_notes, ymt3_hands* out);
void ymt3_hands_destroy(ymt3_hands c);
int  ymt3_split_hands(ymt3_handle h, ymt3_hands c, const void* notes_dev, long long n_notes, const int32_t* count_dev /* may be NULL */,
                      long long n_frames, uint8_t* hand_dev, int32_t* split_dev /* may be NULL */, long long max_slices,
                      long long* result_dev /* [8] */, void* stream);

/* Measurement hook (bench.py `roofline`): decode eagerly (no graph) and bracket every kernel launch of
 * every `stride`-th step (positions stride/2, 3*stride/2, ...) with HIP events on `stream`; synchronises the stream before returning.
 * Classes: 0 qkv+cache GEMM, 1 self-attention, 2 self O-proj, 3 cross Q GEMM, 4 cross-attention,
 * 5 cross O-proj, 6 FFN wi, 7 FFN wo, 8 lm_head, 9 argmax+embed, 10 spans: ONE bracket around the stride-1
 * un-bracketed steps after each sampled step (true step time, used to calibrate out the stream time an
 * event pair itself costs).  Outputs are HOST arrays.
 * The profiled, eager step keeps layer 0's QKV launch: this call never takes the layer-0 table (ymt3_qkv0_table_active) that the timed,
 * graph-replayed calls use, so its launch sequence and class 0 are the pre-table ones (tests pin them). */
#define YMT3_PROFILE_CLASSES 16
int ymt3_profile_decode(ymt3_handle h, const void* enc_dev, int B, int n_steps, int stride, int32_t* tokens_dev,
                        float* ms_by_class, int32_t* launches_by_class, void* stream);

/* Measurement hook: when the handle was created with YMT3_STAMP=1 in the environment, every decode-step kernel records a
 * 100 MHz wall-clock value per workgroup at entry and at the end of its last wave (last step executed wins).  This call
 * synchronises the device and reduces them: for kernel i of the step (launch order; cls[i] = class as in
 * ymt3_profile_decode, grid[i] = workgroups) stats[4i..4i+3] = earliest entry, latest entry, earliest exit, latest exit.
 * Arrays hold 64 kernels. */
int ymt3_debug_step_stamps(ymt3_handle h, int32_t* cls, int32_t* grid, uint64_t* stats, int* n_kernels);
/* The raw (entry, exit) pairs of kernel `kernel` of the step, one per workgroup in blockIdx order (capacity in workgroups). */
int ymt3_debug_kernel_stamps(ymt3_handle h, int kernel, uint64_t* stamps, int capacity_wgs);

/* Debug hook, NOT part of the product surface: refused (YMT3_ERR_UNSUPPORTED) unless the handle was created with
 * YMT3_DEBUG_HOOKS=1 in the environment.  The NEXT ymt3_decode_greedy / ymt3_transcribe_segments call -- that one call
 * only -- starts at cache position `step0` instead of 0; cache positions [0, step0) are zero-filled here, so the call
 * reads defined memory, but its TOKENS are meaningless.  The memory traffic of positions step0.. is exactly that of a
 * real decode, which lets a counter pass (rocprofv3 --pmc) cover late positions with a short process. */
int ymt3_debug_decode_start(ymt3_handle h, int step0);

/* Debug hook, gated like the one above: marks the handle as if one of its merged decode kernels (the attention pair / GEMM chain of the
 * 64-row regime, whose stages wait for each other inside one launch) had given up waiting during the NEXT decode call.  What must
 * follow -- and what the test of this hook checks -- is what a real abort triggers (ymt3_set_abort_recovery): in mode 1 that call
 * returns the correct ids through the separate launches and ymt3_merged_fallbacks reports 1; in mode 0 its ids are all INT32_MIN and
 * the call after it runs, correctly, on the separate launches.  YMT3_ERR_UNSUPPORTED if the handle does not run those kernels (fewer
 * than 256 CUs, both switched off, or already fallen back). */
int ymt3_debug_force_stage_abort(ymt3_handle h);

/* Debug hook, gated like the ones above (MoE decoder FFN only): from now on every lock-step decode call records the router's choices,
 * trace_dev[step][layer][row][2] int32 (the two chosen experts, best first; steps >= n_steps or rows >= n_rows are not recorded); NULL
 * stops recording.  A routing choice is discrete: at a near-tie of the 2nd / 3rd router logit the HIP path may legitimately pick another
 * expert than the CPU oracle.  With the trace a test feeds the HIP path's choices to the oracle, checks each was within the numerical
 * noise of the oracle's own top two, and compares logits / ids at EVERY step instead of excluding the near-tie steps. */
int ymt3_debug_moe_trace(ymt3_handle h, int32_t* trace_dev, int n_steps, int n_rows);

/* Unit-test hooks: C = A(bf16 MxK) * W^T(bf16 NxK), f32 out; runs the encoder GEMM kernel. */
int ymt3_test_gemm(ymt3_handle h, const void* a_dev, const void* w_dev, float* c_dev, int M, int N, int K, void* stream);

/* Per-kernel test doors of the encoder.  Each validates its arguments and calls ONE launcher of the production path (nothing on that
 * path calls them).  They take raw device pointers, so what can be checked without knowing the allocations is checked here and refused
 * with YMT3_ERR_ARG and a text: null pointers, pointers not aligned to 16 bytes, and every shape the launcher would refuse.  The
 * EXTENTS behind the pointers are the caller's duty (yourmt3_amd/model.py computes them from the shape and the strides and refuses a
 * smaller tensor before it calls).  All asynchronous on `stream`; a refused call leaves the door usable.
 *
 * ymt3_test_gemm_ex: out (+)= A[M][K] (bf16, row stride lda) * W[N][K]^T (bf16, ldw) with epilogue 0..4 =
 *   0 f32 out[m * ldc + n] = acc (+ bias[n], bias may be NULL)      1 bf16 out = R(acc)      2 bf16 out = R(max(acc, 0))
 *   3 f32 out += acc                                                 4 bf16 out[n / (H*64)][m / T][h][m % T][64], needs M == n_seg * T
 * N % 128 == 0, K % 64 == 0, lda, ldw >= K and multiples of 8, ldc >= N and a multiple of 8 (epilogue 4 ignores ldc), bias with
 * epilogue 0 only.  M * N elements are written (rows >= M and columns >= N never). */
int ymt3_test_gemm_ex(ymt3_handle h, int epilogue, const void* a_dev, const void* w_dev, void* out_dev, const float* bias_dev, int M, int N,
                      int K, int lda, int ldw, int ldc, int T, int H, int n_seg, void* stream);
/* out bf16 [M][d] = R(x f32 [M][d] * rsqrt(mean(x^2) + eps) * gain f32 [d]);  d % 4 == 0 */
int ymt3_test_rmsnorm(ymt3_handle h, const float* x_dev, const float* gain_dev, void* out_dev, int M, int d, float eps, void* stream);
/* Encoder self-attention of B segments of T in {64, 128, 256, 512} positions, H heads of 64: query rows q + (b*T + t) * ldq + h*64,
 * key / value rows k|v + (b*T + t) * ldkv + h*64 (bf16), bias_off f32 [H][2T-1] indexed by key - query + T - 1,
 * out bf16 [B*T][H*64].  ldq, ldkv >= H*64 and multiples of 8. */
int ymt3_test_enc_attention(ymt3_handle h, const void* q_dev, int ldq, const void* k_dev, const void* v_dev, int ldkv, const float* bias_off_dev,
                            void* out_dev, int B, int T, int H, void* stream);
/* Batched small-sequence attention: sequence s = so * inner_n + si (so = s / inner_n) starts at element so * outer + si * inner of its
 * buffer, position t lies t * step further, head h at + h*64.  Tq % 16 == 0, Tk in {32, 64, 128, 256}; bias_off f32 [H][2*Tk-1] (needs
 * Tq == Tk) or NULL.  Strides are multiples of 8 elements, steps positive. */
typedef struct ymt3_seq_attn_args {
    const void* q; const void* k; const void* v; void* out;
    const float* bias_off;
    int32_t n_seq, H, Tq, Tk, inner_n;
    int64_t q_outer, q_inner, q_step, kv_outer, kv_inner, kv_step, o_outer, o_inner, o_step;
} ymt3_seq_attn_args;
int ymt3_test_seq_attention(ymt3_handle h, const ymt3_seq_attn_args* args, void* stream);
/* out bf16 [n_rows][d] = R(rmsnorm(mel[row] * w + pos[row % F]) * gain): mel f32 [n_rows], w f32 [d], pos bf16 [F][d], gain f32 [d];
 * d % 4 == 0, d <= 256 */
int ymt3_test_spec_embed(ymt3_handle h, const float* mel_dev, const float* w_dev, const void* pos_dev, const float* gain_dev, void* out_dev,
                         long long n_rows, int F, int d, float eps, void* stream);

/* Per-kernel test doors of the decoder step's SEPARATE-LAUNCH kernels (the merged, polling kernels -- attention pair, GEMM chain, step kernel,
 * MoE chain -- need a resident grid and have no door; their bits are tied to these launches by the bit-identity tests).  Same rules as the
 * encoder's doors: one production launcher each, nothing on the production path calls them, YMT3_ERR_ARG with a text for a null or
 * misaligned pointer, for everything the launcher would refuse and for everything it silently assumes; extents are the caller's duty
 * (yourmt3_amd/model.py).  The decode position: `row_pos` (int32 per row, indexed by the absolute row) or, when that is NULL, `step`, which
 * the door places in a DecodeShared block of its own (allocated at first use, freed with the handle): the handle's loop state, caches,
 * counters and graph cache are not touched, and a decode call gives the same bits after any door call.
 *
 * ymt3_test_dec_gemm: launch_dec_gemm.  mode 0 QKV + cache append, 1 bf16, 2 bf16 relu, 3 f32 logits (all four: x = x_f32[R][K] normed with
 * gain and the 32 carried sum(h^2) partials ssq[t][row], K = 512), 4 residual: out_f32[r][n] += a_bf16[R][K] . W[n]^T (N = 512, K in {512,
 * 1024, 2048}; + the eight `part` rows [R][8][512] when given) and ssq[n / 16][r] = this tile's share of sum(h_new^2).  Rows are
 * [row0, row0 + R) of every row-indexed buffer; ssq_stride >= row0 + R.  Mode 0: N = 3 * H * 64; columns [0, H*64) go to out_bf16[r][.],
 * the K and V thirds to cache[((r * H + h) * L + pos) * 64 + d]; `table` (not NULL) takes the packed row as table[r * N + n] instead.
 * pend_y [2R][K] (modes 0 and 3): x = x_f32 + (y[2r] + y[2r + 1]), sum(x^2) taken by the kernel; mode 0 also stores x to h_out.
 * mid_rows: row count from which the mid-size tile kernel runs (< 0: the built-in 512, 0: never); refused when it selects that kernel for a
 * shape it has no instantiation for. */
typedef struct ymt3_dec_gemm_args {
    const float* x_f32; const void* a_bf16; const float* gain; const void* W;
    void* out_bf16; float* out_f32; void* kcache; void* vcache;
    float* ssq; const float* part; const float* pend_y; float* h_out; void* table;
    const int32_t* row_pos;
    int32_t row0, R, N, K, H, L, ssq_stride, mid_rows, step;
    float eps;
} ymt3_dec_gemm_args;
int ymt3_test_dec_gemm(ymt3_handle h, int mode, const ymt3_dec_gemm_args* args, void* stream);
/* ymt3_test_dec_attention: launch_dec_attention, or launch_dec_attention_beam when `anc` is given.  One (row, head) per workgroup, rows
 * [row0, row0 + R), heads of 64; slab (r / rows_per_kv, h) of k / v starts at ((r / rows_per_kv) * H + h) * slab_keys * 64.
 * self_attn != 0: keys 0 .. pos of the slab, bias f32 [H][bias_stride == slab_keys] by distance; wo bf16 [512][H*64] (H == 8): no `out`,
 * opart f32 [R][8][512] instead.  self_attn == 0: n_keys_const in [1, slab_keys] keys, no bias; wq bf16 [H*64][512] (d == 512): the query
 * is projected from the residual row x_f32[r] (gain, and ssq partials or ipart [R][8][512] with H == 8) instead of read from q.
 * force_many: the 2-waves-per-(row, head) form.  anc u8 [2][anc_rows][anc_pitch], W: beam search (self-attention only). */
typedef struct ymt3_dec_attn_args {
    const void* q; const void* k; const void* v; void* out;
    const float* bias; const int32_t* row_pos;
    const void* wq; const float* x_f32; const float* gain; const float* ssq; const float* ipart;
    const void* wo; float* opart;
    const uint8_t* anc;
    int32_t self_attn, step, n_keys_const, slab_keys, rows_per_kv, row0, R, H, bias_stride, ssq_stride, force_many, anc_rows, anc_pitch, W, d;
    float eps;
} ymt3_dec_attn_args;
int ymt3_test_dec_attention(ymt3_handle h, const ymt3_dec_attn_args* args, void* stream);
/* ymt3_test_mc_cross_attention: launch_mc_cross_attention.  Rows row0 + seg * n_channels + channel; k / v bf16 [n_seg][H][T][64];
 * n_channels in [2, 16], T in {128, 256, 512}, d == 512, ssq_stride >= row0 + n_seg * n_channels. */
typedef struct ymt3_mc_cross_args {
    const float* x_f32; const float* gain; const float* ssq; const void* wq; const void* k; const void* v; void* out;
    int32_t row0, n_seg, n_channels, H, T, ssq_stride, d;
    float eps;
} ymt3_mc_cross_args;
int ymt3_test_mc_cross_attention(ymt3_handle h, const ymt3_mc_cross_args* args, void* stream);
/* The token-selection stage of the step (csrc/decode.hip: argmax_embed_kernel and its companions; csrc/beam.hip), by the same rules.  None of
 * these kernels waits on another workgroup, so a door is a plain launch.  The loop state the kernels read from device memory lives in blocks
 * owned by each door (a DecodeShared for ymt3_test_token_step; a DecodeShared and a BeamShared for ymt3_test_beam_step), never the handle's.
 * Before the launch the door writes its block(s) from the arguments on `stream`: step, step0, n_steps, n_prompt, done_count = 0, n_unfinished
 * = R, tokens_out, forced, logits_out, scores_out, prompt, c_allowed / c_next / c_words; alpha and the beam outputs.  keep_shared != 0 leaves
 * the blocks as the previous call of the same door left them (init -> select -> ... -> finalize then shows what the init kernels wrote);
 * such a call must repeat R, row0, n_steps, n_prompt and the presence of c_allowed, its step / step0 / output pointers are ignored, and the door
 * checks it against the position it knows the block to hold.  state_out (int32[4], may be NULL) receives step, done_count, n_unfinished
 * and n_steps of the door's DecodeShared after the launch.  ticket ([R / 32 + 1] lines of 32 words, zero before the launch) and zero_sync
 * (zero_lines lines of 32 words) are caller buffers.  Values behind pointers (positions, states, next-state tables, offsets) are the
 * caller's duty like the extents (yourmt3_amd/model.py checks both).
 *
 * ymt3_test_token_step, op =
 *   0 decode_init   launch_decode_init with one chain: rows [0, R) (row0 must be 0): h = embed[pad_id] (+ chan_embed[r % n_channels]), ssq, finished
 *                   = 0, row_state = c_start[r] clamped into [0, c_n_states) (0 without c_start), the layer-0 table row of pad_id at position step0;
 *                   the block is written by the kernel (step = step0, n_unfinished = R, ...)
 *   1 argmax_embed  launch_argmax_embed over rows [row0, row0 + R): lock-step at the block's `step` (emitted column step - step0 - n_prompt), or
 *                   slot mode when row_pos is given (row_out, and row_prompt with n_prompt > 0; neither forced nor logits_out)
 *   2 slot_start    launch_slot_start: rows [row0, row0 + n_channels); row_out[r] = first_out + channel * n_steps, row_prompt[r] = first_prompt +
 *                   channel * n_prompt, position 0, c_start indexed by the channel
 *   3 slot_retire   launch_slot_retire: PAD (scores 0.0) over [row_pos[r] + 1 - n_prompt, n_steps) of rows [row0, row0 + R) at row_out[r]
 *   4 pad_tail      launch_pad_tail: PAD (scores 0.0) over [from, n_steps) of rows [row0, row0 + R); 0 <= from <= n_steps
 *   5 qkv0_embed    launch_qkv0_embed: rows [0, R) of h / ssq = embed[v0 + i], no channel row (row0 == 0, v0 + R <= V)
 * The selection rule of op 1 (first maximum over the allowed, non-NaN logits that compare greater than -3.4e38, else the lowest allowed
 * index; EOS then PAD; clamped forced / prompt ids; the automaton follows the fed id and freezes after EOS) and its scores are the ones of
 * the decode entry points above.  Rules the kernels have beyond those sections:
 *   - a state that allows no token (ymt3_constraint_create refuses one; a raw table can hold it) emits V - 1, which it does not allow: the
 *     score is -inf, as for a forced disallowed id;
 *   - h[r] = f32(embed[fed]) + f32(chan_embed[r % n_channels]) in one fp32 add; ssq[0][r] = sum(h[r]^2) in fp32, ssq[1..31][r] = 0.0;
 *   - layer-0 table (qkv0 [V][1536] bf16, H == 8, d == 512, one channel): the fed id's q third goes to q0[r]; the k / v thirds go to
 *     kcache0 / vcache0[((r * 8 + head) * L + pos) * 64 ..] with pos = step + 1 (slot mode: the row's position after the step) only while
 *     pos < L; at pos == L the q third is still written and the caches are not touched;
 *   - slot mode: a stopped row (finished != 0) writes no token, score or state, keeps its position and feeds pad_id; the block's `step`
 *     still advances by one per launch and means nothing there;
 *   - after the launch: step + 1, done_count == 0, every ticket line zero, the zero_sync lines zero; with eos_id >= 0, n_unfinished = the
 *     rows of [row0, row0 + R) whose finished flag is 0 (eos_id < 0 leaves n_unfinished alone).
 *
 * ymt3_test_beam_step, op = 0 beam_init (launch_beam_init; the kernel writes both blocks), 1 beam_select (launch_beam_select; slot mode when
 * row_pos is given), 2 beam_finalize (launch_beam_finalize, N = hypotheses per group), 3 beam_slot_start (launch_beam_slot_start: the
 * n_channels * W rows from row0, queue indices first_group + channel), 4 beam_slot_finalize (launch_beam_slot_finalize).  Rows [0, R), R a
 * multiple of W <= 8, R <= anc_rows; anc u8 [2][anc_rows][anc_pitch], slot_anc u8 [R][anc_pitch], anc_pitch % 16 == 0, n_prompt + n_steps below
 * anc_pitch and fed_pitch; fed_tok / fed_lp [R][fed_pitch]; run, fin_* [R]; n_fin [R / W]; tokens_out [G][N][n_steps], seq_out [G][N],
 * tok_out [G][N][n_steps] (both may be NULL).  The selection follows the beam-search section above; what it leaves unsaid:
 *   - the select of position t reads ancestry buffer t & 1 and writes rows 0 .. W - 1 of buffer (t + 1) & 1, whole 32-bit words 0 .. (t + 1) / 4:
 *     entries 0 .. t are the parent's, entry t + 1 the row's own index; bytes of the last word beyond t + 1 are copied from the parent's row;
 *   - a hypothesis entering a slot takes the lowest snapshot row (fin_store) not held by a surviving old slot, and slot_anc[that row] =
 *     words 0 .. t / 4 of its parent's ancestry row; displaced slots free their rows for the same step's entries;
 *   - prompt positions and done groups copy the ancestry rows with every row its own parent, and feed the prompt id / pad_id. */
typedef struct ymt3_token_step_args {
    const float* logits; float* h; const void* embed; const void* chan_embed;
    int32_t* finished; float* ssq; int32_t* row_pos; int64_t* row_out; int64_t* row_prompt; int32_t* row_state;
    uint32_t* ticket; uint32_t* zero_sync;
    const void* qkv0; void* q0; void* kcache0; void* vcache0;
    int32_t* tokens_out; const int32_t* forced; float* logits_out; float* scores_out; const int32_t* prompt;
    const uint32_t* c_allowed; const int32_t* c_next; const int32_t* c_start;
    int32_t* state_out;
    int64_t first_out, first_prompt;
    int32_t ssq_stride, row0, R, V, d, n_channels, eos_id, pad_id, zero_lines, H, L;
    int32_t step, step0, n_steps, n_prompt, c_words, c_n_states, keep_shared, from, v0;
} ymt3_token_step_args;
int ymt3_test_token_step(ymt3_handle h, int op, const ymt3_token_step_args* args, void* stream);
typedef struct ymt3_beam_step_args {
    const float* logits; float* h; const void* embed; const void* chan_embed;
    int32_t* finished; float* ssq; int32_t* row_state;
    uint8_t* anc; int32_t* fed_tok; float* fed_lp; float* run;
    float* fin_score; int32_t* fin_len; int32_t* fin_store; int32_t* fin_tok; float* fin_lp; int32_t* n_fin; uint8_t* slot_anc;
    int32_t* row_pos; int64_t* row_out; int64_t* row_prompt;
    const int32_t* prompt; const uint32_t* c_allowed; const int32_t* c_next; const int32_t* c_start;
    int32_t* tokens_out; float* seq_out; float* tok_out;
    int32_t* state_out;
    int64_t first_group;
    int32_t ssq_stride, R, V, d, n_channels, eos_id, pad_id, W, anc_rows, anc_pitch, fed_pitch;
    int32_t step, n_steps, n_prompt, c_words, c_n_states, keep_shared, N, row0;
    float alpha;
} ymt3_beam_step_args;
int ymt3_test_beam_step(ymt3_handle h, int op, const ymt3_beam_step_args* args, void* stream);

/* Per-kernel test door of the mixture-of-experts decoder FFN's SEPARATE launches (csrc/moe.hip; the one-launch restatement moe_chain.hip is
 * tied to them by the bit-identity test).  Same rules as the doors above.  ymt3_test_moe_stage: launch_moe_stage with no routing trace.
 * stage 0 router: xn[r] = R(h[r] * rsqrt(sum_t ssq[t][r] / 512 + eps) * gain) (bf16), sel[2r], sel[2r + 1] = the two largest of
 *           xn[r] . router[e] (e < E), ties to the lower id, gate[2r], gate[2r + 1] = their softmax; rows r in [row0, row0 + R)
 * stage 1 expert wi: hidden[2 row0 + p] = R(relu(xn[row0 + (p >> 1)] . wi[sel[2 row0 + p]]^T)) for the pairs p in [0, 2R)
 * stage 2 expert wo: y[2 row0 + p] = gate[2 row0 + p] * (hidden[2 row0 + p] . wo[sel[2 row0 + p]]^T)
 * stage 3 combine:   h[r] += y[2r] + y[2r + 1]; ssq[0][r] = sum(h[r]^2), ssq[1..31][r] = 0
 * fp8 != 0 (stages 1, 2): weights wi_q8 / wo_q8 (OCP e4m3, same shapes) with one fp32 scale per expert (wi_s / wo_s [E]); the activation
 * rows are quantised per row by the kernel.  A pair whose sel lies outside [0, E) is written by no stage.  d_model = 512, d_ff = 2048,
 * top_k = 2, 2 <= E <= 16, 1 <= R <= 1536, ssq_stride >= row0 + R; only the pointers the stage reads or writes are looked at. */
typedef struct ymt3_moe_args {
    float* h; const float* gain; float* ssq; const void* router; const void* wi; const void* wo;
    const void* wi_q8; const void* wo_q8; const float* wi_s; const float* wo_s;
    void* xn; int32_t* sel; float* gate; void* hidden; float* y;
    int32_t ssq_stride, fp8, row0, R, E, top_k, d_model, d_ff;
    float eps;
} ymt3_moe_args;
int ymt3_test_moe_stage(ymt3_handle h, int stage, const ymt3_moe_args* args, void* stream);

/* Per-kernel test doors of the full-sequence scoring pass (csrc/dec_seq.hip), one production launcher each.  Same rules as the doors above;
 * none touches handle state.  Rows are [row0, row0 + n_rows) of prompt / tokens / lengths / scores / logits (indexed by the ABSOLUTE row);
 * h, q, out and xn start at the launch's first row.  d == 512, L == n_prompt + n_steps.
 * ymt3_test_seq_embed: launch_seq_embed.  h f32 [n_rows * L][512] = embed[fed id] (+ chan_embed[row % n_channels]): position 0 feeds pad_id,
 *   1 .. P the prompt, P + j + 1 tokens[j], every id clamped into [0, V).  chan_embed needs n_channels >= 1.
 * ymt3_test_dec_seq_attention: launch_dec_seq_attention.  Query row (r, t) at q + r * q_seq + t * ldq + 64 h, key / value row (b, t) at
 *   k|v + b * kv_seq + h * kv_head + t * ldkv with b = (row0 + r) / rows_per_kv, output row at out + r * o_seq + t * ldo + 64 h.  causal != 0:
 *   n_keys == L <= bias_stride, keys <= query, + bias[h][query - key] (f32 [H][bias_stride]); else every one of n_keys keys, no bias.  ldq, ldo
 *   >= 64 H, ldkv >= 64, strides multiples of 8 elements, H and n_rows <= 65535.
 * ymt3_test_seq_lm_head: launch_seq_lm_head_score.  xn bf16 [M][512] (M == n_rows * L), W bf16 [V][512], V % 16 == 0: scores[row][j] =
 *   logit[tokens[row][j]] - lse for j = position - n_prompt >= 0 (exactly 0.0 for j >= lengths[row] clamped into [0, n_steps]; lengths may be
 *   NULL), logits[row][j][V] when not NULL; prompt positions write nothing. */
typedef struct ymt3_seq_embed_args {
    float* h; const void* embed; const void* chan_embed; const int32_t* prompt; const int32_t* tokens;
    int32_t row0, n_rows, L, n_prompt, n_steps, V, d, n_channels, pad_id;
} ymt3_seq_embed_args;
int ymt3_test_seq_embed(ymt3_handle h, const ymt3_seq_embed_args* args, void* stream);
typedef struct ymt3_dec_seq_attn_args {
    const void* q; const void* k; const void* v; void* out; const float* bias;
    int64_t q_seq, kv_seq, o_seq;
    int32_t ldq, ldkv, ldo, kv_head, row0, n_rows, L, n_keys, rows_per_kv, H, bias_stride, causal;
} ymt3_dec_seq_attn_args;
int ymt3_test_dec_seq_attention(ymt3_handle h, const ymt3_dec_seq_attn_args* args, void* stream);
typedef struct ymt3_seq_lm_head_args {
    const void* xn; const void* W; const int32_t* tokens; const int32_t* lengths; float* scores; float* logits;
    int32_t M, L, n_prompt, n_steps, V, d, row0;
} ymt3_seq_lm_head_args;
int ymt3_test_seq_lm_head(ymt3_handle h, const ymt3_seq_lm_head_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YMT3_H */
