// C-ABI runtime of the hot path: handle, weight blob, workspace, kernel orchestration, hipGraph
// replay of the decode step.  Declarations and ownership rules: include/ymt3.h.
//
// Host logic only -- every FLOP is in frontend.hip / gemm.hip / norm.hip / enc_attn.hip /
// decode.hip; the note-side objects are in note_objects.hip.  There is no CPU fallback: a missing
// device, tensor or unsupported shape is an error.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <atomic>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/ymt3.h"
#include "common.h"
#include "kernels.h"
#include "runtime.h"

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void ymt3_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
struct Tensor {
    void* dev = nullptr;
    uint32_t dtype = 0, ndim = 0, shape[4] = {1, 1, 1, 1};
    size_t nbytes = 0;
};

struct StepGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool merged = false;            // the captured steps contain merged kernels (GEMM chain / attention pair): their abort word must be looked at
};
// The host-side inputs of one decoder step: everything that decides its launches and is not read from device memory.  Built once per
// call (step_shape, chain_shape) and passed down by value; nothing about a step is kept on the handle between calls.
enum StepMode { SM_LOCKSTEP = 0, SM_BEAM, SM_SLOT, SM_SLOT_BEAM };
struct StepShape {
    StepMode mode = SM_LOCKSTEP;
    int B = 0;                      // segments of the call (lock-step, beam) or slots (slot modes)
    int W = 0;                      // beams per group of a beam call, 0 otherwise
    int n_chains = 1, chain = 0;    // chains the call uses, and which of them this step belongs to
    int row0 = 0, R = 0;            // the step's rows [row0, row0 + R): the chain's share of the call's rows
    bool solo = true;               // the only decode stream of the handle while it runs (n_chains == 1)
    bool qkv0 = false;              // layer 0's q / k / v come from the table (qkv0_applies): the steps launch no layer-0 projection
    bool profiled = false;          // ymt3_profile_decode's call: its launch sequence is the one the profile classes are defined by
    bool slot() const { return mode == SM_SLOT || mode == SM_SLOT_BEAM; }     // rows at their own positions (row_pos / row_out / row_prompt)
};
// What a cached step graph is filed under.  Derived from the shape (step_key) and from nothing else: row0, R, solo and qkv0 follow from
// (mode, B, W, n_chains, chain) and the handle's create-time configuration, and a profiled call replays no graph.
struct StepKey {
    StepMode mode;
    int B, n_chains, chain, beams, steps;       // steps: decode steps in the graph
    bool operator<(const StepKey& o) const {
        return std::tie(mode, B, n_chains, chain, beams, steps) < std::tie(o.mode, o.B, o.n_chains, o.chain, o.beams, o.steps);
    }
};
static StepKey step_key(const StepShape& S, int steps) { return StepKey{S.mode, S.B, S.n_chains, S.chain, S.W, steps}; }

// The decoder's weights, looked up in the blob once (create_impl: bind_dec_weights) with the dtype and minimum size the kernels rely on.
struct LayerW {
    const float *ln1 = nullptr, *ln2 = nullptr, *ln3 = nullptr;
    const bf16_t *wqkv = nullptr, *wo = nullptr, *wq_c = nullptr, *wo_c = nullptr, *wi = nullptr, *wo2 = nullptr, *router = nullptr;
    const uint8_t *wi_q8 = nullptr, *wo_q8 = nullptr;      // MoE experts in fp8 (then wi / wo2 are null) and their scales
    const float *wi_s = nullptr, *wo_s = nullptr;
};
struct DecWeights {
    std::vector<LayerW> layer;
    const bf16_t *embed = nullptr, *chan_embed = nullptr, *lm_head = nullptr;      // chan_embed: null with one channel
    const float *ln_f = nullptr, *bias_dist = nullptr;
};

struct ymt3_ctx {
    ymt3_config cfg{};
    int device = 0;
    int T = 0, inner = 0, maxB = 0, maxR = 0;
    char* blob_dev = nullptr;
    size_t blob_bytes = 0;
    std::map<std::string, Tensor> tensors;
    DecWeights dec;
    std::vector<void*> allocs;
    size_t dev_bytes = 0;
    FrontendTables fe{};
    // encoder workspace
    float* mel = nullptr;
    bf16_t* mel_bf = nullptr;
    float* h_enc = nullptr;
    bf16_t *xn = nullptr, *qkv = nullptr, *attn = nullptr, *ff = nullptr, *enc_out = nullptr;
    size_t act_rows = 0;                // rows of h_enc / xn / qkv / attn / ff: max(max_batch * n_frames, max_decode_len) -- the full-sequence decoder
                                        // pass (ymt3_score_tokens) reuses them in chunks of whole decoder rows and needs room for one
    // Perceiver-TF encoder workspace (a9): N1 = B*T*F' spectral tokens, N2 = B*T*K latent rows, D = ptf_d
    bf16_t *p_xs = nullptr, *p_kvs = nullptr;      // [N1][D] normed spectral tokens, [N1][2D] their K/V of one block
    float* p_z = nullptr;                          // [N2][D] fp32 latent residual stream, layout [b][t][k][:]
    bf16_t *p_zn = nullptr, *p_qkv = nullptr, *p_att = nullptr, *p_ff = nullptr;   // [N2][D], [N2][3D], [N2][D], [N2][ptf_dff]
    // decoder workspace
    bf16_t* wkv_all = nullptr;          // [n_dec*2*inner][d]
    bf16_t* ckv = nullptr;              // [n_dec*2][B][H][T][64]
    bf16_t *kcache = nullptr, *vcache = nullptr;   // [n_dec][maxR][H][L][64]
    float* h_dec = nullptr;
    float* h_dec2 = nullptr;            // MoE decoder: the second residual buffer of the folded combine (layers alternate between the two)
    bf16_t *dq = nullptr, *dattn = nullptr, *dff = nullptr;
    float* logits = nullptr;
    float* ssq = nullptr;               // [SSQ_TILES][maxR]
    float* opart = nullptr;             // [maxR][H][d]: per-head O-projection partials of the self-attention kernel (fold_o)
    MoeArgs moe{};                      // scratch pointers of the MoE FFN (dec_ffn == YMT3_FFN_MOE)
    int* finished = nullptr;
    // slot modes (ymt3_transcribe_stream*): per-row positions and output offsets, wired into the launches of a step whose shape says slot()
    int* row_pos = nullptr;             // [maxR]
    long long* row_out = nullptr;       // [maxR]
    long long* row_prompt = nullptr;    // [maxR]: slot mode, offset of the row's prompt in the caller's prompt buffer
    int* row_state = nullptr;           // [maxR]: every row's token-automaton state (include/ymt3.h, constraints)
    int* host_rows = nullptr;           // pinned [maxR]: copy of `finished` for the host's retire/admit decisions
    DecodeShared* shared = nullptr;     // [MAX_CHAINS] per-chain loop state
    DecodeShared* test_shared = nullptr;   // the decoder test doors' own block (ymt3_test_dec_gemm / _dec_attention), allocated at first use
    // the token-selection doors' own blocks (ymt3_test_token_step / _beam_step) and what the host knows of them: the position the next launch
    // reads and the call geometry they were written for (a keep_shared call is checked against these, not against its arguments)
    struct DoorLoop { bool valid = false; int step = 0, step0 = 0, n_steps = 0, n_prompt = 0; bool constrained = false; int row0 = 0, R = 0; };
    DecodeShared* test_tok_shared = nullptr;
    DecodeShared* test_beam_shared = nullptr;
    BeamShared* test_beam_params = nullptr;
    DoorLoop test_tok_loop, test_beam_loop;
    hipStream_t cap_stream = nullptr;
    // Decode rows are independent, so a batch CAN be cut into `n_chains` contiguous row ranges whose step graphs replay
    // concurrently on separate HIP streams.  Measured on MI355X in both rounds (profiles/r01_chain_sweep.txt with one host thread
    // feeding all chains, profiles/r02_chain_sweep_threads.txt with one launcher thread per chain): it loses -- 2 chains 289.8 ms
    // per batch against 279.8 for one, 3 / 4 chains 474 / 486 ms -- so the chains do not overlap on the device either.
    // Default 1; YMT3_CHAINS overrides (kept as a tested option: any row split must give identical ids).
    int n_chains = 1;
    // Round 3, many rows: with 168-256 rows of one channel the attention kernels are bandwidth-bound and the GEMMs between them latency-bound, and
    // two chains of 84-128 rows do overlap: 626 against 690 ms per batch of 256, -6 % at 176 and 192 (profiles/r03_chains_many_rows.txt; -1 % at 160, slower from
    // 512).  `auto_chains` (YMT3_CHAINS unset) takes two chains exactly there -- both halves and the whole stay in the same kernel regime (8-wave
    // attention, 16-row-tile GEMMs, no folded O-projection), so the ids do not depend on the choice (tested); decode_run checks just that
    // on the plans of the whole and of both halves (bits_agree) before it takes them.
    bool auto_chains = true;
    int last_chains = 1;                    // chains of the last decode call (ymt3_last_decode_chains)
    bool last_qkv0 = false;                 // the last decode call took layer 0's q / k / v from the table (ymt3_qkv0_table_active)
    hipStream_t chain_stream[8] = {};
    hipEvent_t fork_ev = nullptr, join_ev[8] = {};
    std::map<StepKey, StepGraph> step_graphs;
    bool use_graph = true;
    int graph_steps = 16;                   // decode steps per replayed graph (YMT3_GRAPH_STEPS): a graph launch costs ~7 us of stream time on top of its kernels
    bool fuse_q = true;                     // cross-attention computes its own query projection
    bool moe_fold_combine = true;           // MoE: h += y0 + y1 is done by the next norm GEMM's prologue (YMT3_MOE_COMBINE_LAUNCH=1: own launch)
    bool fold_o = true;                     // self-attention ends with its head's O-projection partial; no separate O-projection launch
    bool gemm_chain = true;                 // cross O -> FFN-in -> FFN-out -> next QKV / lm_head as one launch (dec_chain.hip; YMT3_NO_GEMM_CHAIN=1: four launches)
    unsigned* chain_sync = nullptr;         // [CHAIN_SYNC_WORDS] device: the chain kernel's arrival counters + sticky abort word
    unsigned* chain_host_abort = nullptr;   // pinned: set by the chain kernel together with the abort word; checked at every call
    bool forced_abort = false;              // ymt3_debug_force_stage_abort: raise the host word after the next decode call, as a kernel would during it
    // What happens when a merged kernel gives up waiting (ymt3_set_abort_recovery): 1 (default) = every decode call that ran merged kernels ends
    // by waiting for its stream and looking at the abort word; an abort re-runs the call through the separate launches (same bits) and the
    // handle stays on them.  0 = fully asynchronous calls: an aborted call's ids are INT32_MIN and the NEXT call on the handle switches over.
    int abort_recovery = 1;
    int fallback_count = 0;                 // how often this handle fell back from the merged kernels to the separate launches (0 or 1)
    int mid_rows = -1;                      // YMT3_DEC_GEMM_MID_ROWS at create: decode GEMMs take mid-size tiles from this many rows on (-1: DEC_GEMM_MID_ROWS, 0: never)
    bool force_2wave = false;               // YMT3_SELF_ATTN_2WAVE=1 at create (test knob): the many-row 2-wave self-attention at any row count
    bool attn_pair = true;                  // a layer's self- and cross-attention as one launch (decode.hip: dec_attn_pair_kernel; YMT3_NO_ATTN_PAIR=1: two)
    unsigned* pair_rows = nullptr;          // [maxR <= 64][2] counter lines of that kernel (zero between launches)
    bool step_kernel = false;               // a step's six layers as ONE launch (dec_step.hip): YMT3_STEP_KERNEL=1; default: attention pair + GEMM chain per layer
    bool moe_chain = false;                 // MoE decoder: a layer's five skinny launches as one (moe_chain.hip; YMT3_NO_MOE_CHAIN=1: separate launches)
    int merged_max_rows = 64;               // YMT3_MERGED_MAX_ROWS: the attention pair / GEMM chain are taken up to this many rows (<= 256)
    bool step_tiles_free = false;           // YMT3_STEP_TILES_FREE=1 (A/B): the step kernel's four row tiles as independent pipelines instead of in step
    // Layer 0's QKV projection as a table (kernels.h, ArgmaxArgs::qkv0): [vocab][3 * inner] bf16, built at create for a one-channel decoder
    // (YMT3_NO_QKV0_TABLE=1: not built; neither under YMT3_STAMP nor with the per-step kernel, whose launch sequences stay as they were).
    // Whether a call gathers from it is decided per call (qkv0_applies) and carried in the call's StepShape.
    bf16_t* qkv0_table = nullptr;
    unsigned* ticket = nullptr;             // [maxR / 32 + 1] lines: the argmax kernel's two-level ticket (many rows)
    unsigned* step_sync = nullptr;          // [STEP_SYNC_LINES] counter lines of that kernel (zeroed by the step's argmax kernel / before a decode call)
    // sampled per-kernel-class timing (ymt3_profile_decode): events bracket single launches
    bool prof_on = false;
    size_t prof_span_idx = 0;
    bool prof_span_open = false;
    int last_steps = 0;                     // steps launched by the last decode call (ymt3_last_decode_steps)
    int early_stop_interval = 0;            // ymt3_set_early_stop: host checks `n_unfinished` every N steps (0 = never)
    int* host_flag = nullptr;               // pinned, for that check
    bool debug_hooks = false;               // YMT3_DEBUG_HOOKS=1 at create: ymt3_debug_decode_start is accepted
    int prof_step0 = 0;                     // ymt3_debug_decode_start: the next decode call begins at this position (one shot)
    int32_t* moe_trace = nullptr;           // ymt3_debug_moe_trace: caller's [steps][layers][rows][2] buffer the MoE router records its choices in
    int moe_trace_steps = 0, moe_trace_rows = 0;
    // beam search (include/ymt3.h): all scratch is sized at create by the handle's rows and max_decode_len.  A step whose shape has W > 0
    // addresses the self-attention cache through the ancestry table and ends with the selection kernel
    BeamArgs beam{};                        // the scratch pointers (anc, fed_tok, run, finished slots, ...)
    BeamShared* beam_shared = nullptr;      // device: the call's parameters and the debug trace pointers
    BeamShared beam_trace{};                // ymt3_debug_beam_trace: host copy of the trace fields (carried into every call's parameters)
    std::vector<hipEvent_t> prof_ev;        // pairs
    std::vector<int> prof_cls;
    // measurement (YMT3_STAMP=1): per-workgroup wall-clock stamps of the decode-step kernels, slot = launch order in the step
    unsigned long long* stamp_buf = nullptr;   // [STAMP_NODES][STAMP_WGS][2]
    int stamp_n = 0, stamp_cls[64] = {}, stamp_grid[64] = {};
    // ymt3_ingest: polyphase low-pass per (up, down), built on first use
    struct Resampler { float* taps = nullptr; int up = 1, down = 1, J = 1, Jp = 4, window = 0; long long r = 0; };
    std::map<std::pair<int, int>, Resampler> resamplers;
};

constexpr int STAMP_NODES = 64, STAMP_WGS = 8192;
static unsigned long long* next_stamp(ymt3_ctx* c, int cls, int grid) {
    if (!c->stamp_buf || c->stamp_n >= STAMP_NODES || grid > STAMP_WGS) return nullptr;
    const int i = c->stamp_n++;
    c->stamp_cls[i] = cls;
    c->stamp_grid[i] = grid;
    return c->stamp_buf + (size_t)i * STAMP_WGS * 2;
}

enum { PC_QKV = 0, PC_SELF_ATTN, PC_SELF_O, PC_CROSS_Q, PC_CROSS_ATTN, PC_CROSS_O, PC_FFN_WI, PC_FFN_WO, PC_LM_HEAD, PC_ARGMAX, PC_SPAN, PC_CHAIN, PC_ATTN_PAIR, PC_STEP, PC_COUNT };

struct ProfScope {
    ymt3_ctx* c; hipStream_t s; bool on;
    ProfScope(ymt3_ctx* c_, int cls, hipStream_t s_) : c(c_), s(s_), on(c_->prof_on) {
        if (!on) return;
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
        c->prof_ev.push_back(a); c->prof_ev.push_back(b); c->prof_cls.push_back(cls);
        (void)hipEventRecord(a, s);
    }
    ~ProfScope() { if (on) (void)hipEventRecord(c->prof_ev.back(), s); }
};
#define PLAUNCH(cls, expr) do { ProfScope _ps(h, cls, s); LAUNCH(expr); } while (0)

static int dev_alloc(ymt3_ctx* c, void** p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
    c->allocs.push_back(*p);
    c->dev_bytes += bytes;
    return 0;
}

template <typename T>
static int get(ymt3_ctx* c, const std::string& name, uint32_t dtype, T** out, size_t min_elems = 0) {
    auto it = c->tensors.find(name);
    if (it == c->tensors.end()) FAIL(YMT3_ERR_BLOB, "weight blob has no tensor '%s'", name.c_str());
    if (it->second.dtype != dtype) FAIL(YMT3_ERR_BLOB, "tensor '%s' has dtype %u, expected %u", name.c_str(), it->second.dtype, dtype);
    const size_t esz = dtype == 1 ? 2 : (dtype == 3 ? 1 : 4);
    if (it->second.nbytes < min_elems * esz)
        FAIL(YMT3_ERR_BLOB, "tensor '%s' holds %zu bytes, expected at least %zu", name.c_str(), it->second.nbytes, min_elems * esz);
    *out = reinterpret_cast<T*>(it->second.dev);
    return 0;
}
#define GET(...)                     \
    do {                             \
        int _rc = get(__VA_ARGS__);  \
        if (_rc) return _rc;         \
    } while (0)

#pragma pack(push, 1)
struct BlobEntry {
    char name[48];
    uint32_t dtype, ndim, shape[4];
    uint64_t offset, nbytes;
};
#pragma pack(pop)
static_assert(sizeof(BlobEntry) == 88, "blob entry layout");

static int parse_blob(ymt3_ctx* c, const void* blob, size_t nbytes) {
    const char* b = static_cast<const char*>(blob);
    if (nbytes < 16 || memcmp(b, "YMT3BLOB", 8) != 0) FAIL(YMT3_ERR_BLOB, "bad weight blob magic");
    uint32_t ver, n;
    memcpy(&ver, b + 8, 4);
    memcpy(&n, b + 12, 4);
    if (ver != 1) FAIL(YMT3_ERR_BLOB, "unsupported blob version %u", ver);
    if (16 + (size_t)n * sizeof(BlobEntry) > nbytes) FAIL(YMT3_ERR_BLOB, "truncated blob header");
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->blob_dev), nbytes));
    c->allocs.push_back(c->blob_dev);
    c->dev_bytes += nbytes;
    c->blob_bytes = nbytes;
    HIP_TRY(hipMemcpy(c->blob_dev, blob, nbytes, hipMemcpyHostToDevice));
    for (uint32_t i = 0; i < n; ++i) {
        BlobEntry e;
        memcpy(&e, b + 16 + (size_t)i * sizeof(BlobEntry), sizeof(e));
        const size_t header_end = 16 + (size_t)n * sizeof(BlobEntry);
        if (e.offset % 16 || e.offset < header_end || e.offset > nbytes || e.nbytes > nbytes - e.offset)     // no wrap-around
            FAIL(YMT3_ERR_BLOB, "tensor %u out of bounds / misaligned", i);
        e.name[47] = 0;
        Tensor t;
        t.dev = c->blob_dev + e.offset;
        t.dtype = e.dtype;
        t.ndim = e.ndim;
        memcpy(t.shape, e.shape, sizeof(t.shape));
        t.nbytes = e.nbytes;
        c->tensors[e.name] = t;
    }
    return 0;
}

static void clear_step_graphs(ymt3_ctx* h) {
    for (auto& kv : h->step_graphs) {
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    }
    h->step_graphs.clear();
}

// ------------------------------------------------------------------------------------------------
int handle_device(ymt3_handle h) { return h->device; }
const ymt3_config& handle_config(ymt3_handle h) { return h->cfg; }

extern "C" int ymt3_abi_version(void) { return YMT3_ABI_VERSION; }
extern "C" const char* ymt3_last_error(void) { return g_err; }

extern "C" void ymt3_destroy(ymt3_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    clear_step_graphs(h);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->host_flag) (void)hipHostFree(h->host_flag);
    if (h->chain_host_abort) (void)hipHostFree(h->chain_host_abort);
    if (h->host_rows) (void)hipHostFree(h->host_rows);
    for (int i = 0; i < 8; ++i) {
        if (h->chain_stream[i]) (void)hipStreamDestroy(h->chain_stream[i]);
        if (h->join_ev[i]) (void)hipEventDestroy(h->join_ev[i]);
    }
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
}

extern "C" size_t ymt3_device_bytes(ymt3_handle h) { return h ? h->dev_bytes : 0; }
extern "C" int ymt3_qkv0_table_active(ymt3_handle h) { return h && h->last_qkv0 ? 1 : 0; }

// Layer 0's QKV projection over the whole vocabulary (kernels.h, ArgmaxArgs::qkv0): the decode step's own two kernels -- embed_row, then the
// 16-row-tile dec_gemm_kernel<DG_NORM_QKV_CACHE> writing its packed rows to the table -- with the token ids as rows, in chunks of 256 (below
// every mid-tile threshold, and mid_rows = 0 says so whatever the handle's) through scratch of that size.  A row of the kernel depends on
// that row's h and sum(h^2) tiles alone, so table[v] is what the launch writes for any row fed v, bit for bit.
static int build_qkv0_table(ymt3_ctx* c) {
    const ymt3_config& k = c->cfg;
    const int d = k.d_model, V = k.vocab, N = 3 * c->inner, CH = 256;
    if (dev_alloc(c, (void**)&c->qkv0_table, (size_t)V * N * 2)) return YMT3_ERR_HIP;
    float *hs = nullptr, *ssq = nullptr;
    struct Scratch { float** a; float** b; ~Scratch() { if (*a) (void)hipFree(*a); if (*b) (void)hipFree(*b); } } scratch{&hs, &ssq};
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&hs), (size_t)CH * d * 4));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ssq), (size_t)SSQ_TILES * CH * 4));
    ArgmaxArgs e{};
    e.h = hs; e.ssq = ssq; e.ssq_stride = CH; e.V = V; e.d = d; e.n_channels = 1;
    e.embed = c->dec.embed;
    DecGemmArgs a{};
    a.x_f32 = hs; a.ssq = ssq; a.ssq_stride = CH; a.N = N; a.K = d; a.eps = k.ln_eps; a.H = k.n_heads; a.L = k.max_decode_len;
    a.shared = c->shared;                     // (the kernel requests the cache position with its operands; the table path does not use it)
    a.mid_rows = 0;
    a.gain = c->dec.layer[0].ln1; a.W = c->dec.layer[0].wqkv;
    for (int v0 = 0; v0 < V; v0 += CH) {
        const int n = std::min(CH, V - v0);
        hipStream_t s = nullptr;
        LAUNCH(launch_qkv0_embed(e, v0, n, s));
        a.row0 = 0; a.R = n; a.table = c->qkv0_table + (size_t)v0 * N;
        LAUNCH(launch_dec_gemm(DG_NORM_QKV_CACHE, a, s));
    }
    HIP_TRY(hipDeviceSynchronize());
    return YMT3_OK;
}

// create_impl's helper: every decoder tensor the step kernels, the qkv0 table and the scoring pass read, with its dtype and minimum size
static int bind_dec_weights(ymt3_ctx* c) {
    const ymt3_config& k = c->cfg;
    const size_t d = k.d_model, inner = c->inner, V = k.vocab;
    const bool moe = k.dec_ffn == YMT3_FFN_MOE;
    const size_t ne = moe ? (size_t)k.n_experts : 1;
    DecWeights& D = c->dec;
    D.layer.assign((size_t)k.n_dec_layers, LayerW{});
    for (int l = 0; l < k.n_dec_layers; ++l) {
        const std::string p = "dec." + std::to_string(l) + ".";
        LayerW& W = D.layer[(size_t)l];
        GET(c, p + "ln1", 0u, &W.ln1, d);
        GET(c, p + "ln2", 0u, &W.ln2, d);
        GET(c, p + "ln3", 0u, &W.ln3, d);
        GET(c, p + "wqkv", 1u, &W.wqkv, 3 * inner * d);
        GET(c, p + "wo", 1u, &W.wo, d * inner);
        GET(c, p + "wq_c", 1u, &W.wq_c, inner * d);
        GET(c, p + "wo_c", 1u, &W.wo_c, d * inner);
        if (moe && k.moe_fp8) {
            GET(c, p + "wi_q8", 3u, &W.wi_q8, ne * k.d_ff * d);
            GET(c, p + "wo2_q8", 3u, &W.wo_q8, ne * d * k.d_ff);
            GET(c, p + "wi_s", 0u, &W.wi_s, ne);
            GET(c, p + "wo2_s", 0u, &W.wo_s, ne);
        } else {
            GET(c, p + "wi", 1u, &W.wi, ne * k.d_ff * d);
            GET(c, p + "wo2", 1u, &W.wo2, ne * d * k.d_ff);
        }
        if (moe) GET(c, p + "router", 1u, &W.router, (size_t)k.n_experts * d);
    }
    GET(c, "dec.embed", 1u, &D.embed, V * d);
    if (k.n_channels > 1) GET(c, "dec.chan_embed", 1u, &D.chan_embed, (size_t)k.n_channels * d);
    GET(c, "dec.ln_f", 0u, &D.ln_f, d);
    GET(c, "dec.lm_head", 1u, &D.lm_head, V * d);
    GET(c, "dec.bias_dist", 0u, &D.bias_dist, (size_t)k.n_heads * k.max_decode_len);
    return YMT3_OK;
}

static int create_impl(ymt3_ctx* c, const ymt3_config* cfg, const void* blob, size_t nbytes) {
    const ymt3_config& k = c->cfg;
    if (k.d_kv != 64) FAIL(YMT3_ERR_UNSUPPORTED, "d_kv must be 64 (got %d)", k.d_kv);
    if (k.d_model != 16 * SSQ_TILES) FAIL(YMT3_ERR_UNSUPPORTED, "d_model must be 512 (got %d)", k.d_model);
    if (k.n_heads * k.d_kv != 512) FAIL(YMT3_ERR_UNSUPPORTED, "n_heads*d_kv must be 512");
    if (k.encoder_type != YMT3_ENC_T5 && k.encoder_type != YMT3_ENC_PERCEIVER_TF) FAIL(YMT3_ERR_UNSUPPORTED, "unknown encoder_type %d", k.encoder_type);
    if (k.dec_ffn == YMT3_FFN_MOE && (k.moe_top_k != 2 || k.n_experts < 2 || k.n_experts > 16 || k.d_ff != 2048))
        FAIL(YMT3_ERR_UNSUPPORTED, "MoE FFN needs top_k = 2, 2..16 experts, d_ff = 2048");
    if (k.max_batch <= 0 || k.n_channels <= 0 || k.max_decode_len <= 0) FAIL(YMT3_ERR_ARG, "bad max_batch / n_channels / max_decode_len");
    if (k.hop <= 0 || k.sample_rate <= 0 || k.segment_samples <= 0 || k.n_fft <= 0 || k.n_mels <= 0 || k.vocab <= 0 || k.d_ff <= 0 ||
        k.n_enc_layers < 0 || k.n_dec_layers <= 0 || k.n_enc_layers > 64 || k.n_dec_layers > 64 || k.n_channels > 64 ||
        k.max_decode_len > 65536 || (long long)k.max_batch * k.n_channels > 65536)
        FAIL(YMT3_ERR_ARG, "a size field of the config is zero, negative or absurd");
    c->T = 1 + k.segment_samples / k.hop;
    c->inner = k.n_heads * k.d_kv;
    c->maxB = k.max_batch;
    c->maxR = k.max_batch * k.n_channels;
    if (c->T % 64) FAIL(YMT3_ERR_UNSUPPORTED, "n_frames must be a multiple of 64 (got %d)", c->T);
    if (k.segment_samples <= k.n_fft / 2) FAIL(YMT3_ERR_UNSUPPORTED, "segment_samples must exceed n_fft/2 (reflect padding)");
    if (k.pad_id < 0 || k.pad_id >= k.vocab || k.eos_id >= k.vocab) FAIL(YMT3_ERR_ARG, "pad_id / eos_id outside the vocabulary");
    if (k.vocab % 16 || k.d_ff % 128) FAIL(YMT3_ERR_UNSUPPORTED, "vocab %% 16 and d_ff %% 128 must be 0");
    // shapes the kernels' launch guards refuse: an error here, naming the field, and not "rejected its shape" from the first encode / decode
    if (k.n_fft != 2048 && k.n_fft != 512) FAIL(YMT3_ERR_UNSUPPORTED, "n_fft must be 2048 or 512 (got %d)", k.n_fft);
    if (k.n_mels % 64) FAIL(YMT3_ERR_UNSUPPORTED, "n_mels must be a multiple of 64 (got %d)", k.n_mels);
    if (k.hop > 256 || k.hop % 2)
        FAIL(YMT3_ERR_UNSUPPORTED, "hop must be even and at most 256 (got %d): the log-mel kernel stages 8 frames in LDS and reads sample pairs", k.hop);
    if (k.encoder_type == YMT3_ENC_T5 && c->T != 64 && c->T != 128 && c->T != 256 && c->T != 512)
        FAIL(YMT3_ERR_UNSUPPORTED, "n_frames must be 64, 128, 256 or 512 for the T5 encoder's self-attention (got %d)", c->T);
    if (k.encoder_type == YMT3_ENC_PERCEIVER_TF && c->T != 64 && c->T != 128 && c->T != 256)
        FAIL(YMT3_ERR_UNSUPPORTED, "n_frames must be 64, 128 or 256 for the Perceiver-TF temporal attention (got %d)", c->T);
    if (k.dec_ffn == YMT3_FFN_DENSE && k.d_ff != 512 && k.d_ff != 1024 && k.d_ff != 2048)
        FAIL(YMT3_ERR_UNSUPPORTED, "a dense d_ff must be 512, 1024 or 2048 (got %d): the decoder's FFN-out kernel is instantiated at those K", k.d_ff);
    if (k.dec_ffn != YMT3_FFN_DENSE && k.dec_ffn != YMT3_FFN_MOE) FAIL(YMT3_ERR_UNSUPPORTED, "unknown dec_ffn %d", k.dec_ffn);

    HIP_TRY(hipSetDevice(c->device));
    int rc = parse_blob(c, blob, nbytes);
    if (rc) return rc;
    if (init_gemm_kernels() || init_enc_attn_kernels() || init_decode_kernels() || init_moe_kernels() || init_mc_cross_kernels()) FAIL(YMT3_ERR_HIP, "hipFuncSetAttribute(max dynamic LDS) failed");

    // front-end tables (built by yourmt3_amd/tables.py, carried in the blob)
    const int nfft = k.n_fft;
    FrontendTables& fe = c->fe;
    GET(c, "fe.window", 0u, const_cast<float**>(&fe.window), (size_t)nfft);
    GET(c, "fe.tw", 0u, reinterpret_cast<float**>(const_cast<float2**>(&fe.tw)), (size_t)nfft);
    GET(c, "fe.untw", 0u, reinterpret_cast<float**>(const_cast<float2**>(&fe.untw)), (size_t)nfft + 2);
    GET(c, "fe.mel_start", 2u, const_cast<int**>(&fe.mel_start), (size_t)k.n_mels);
    GET(c, "fe.mel_len", 2u, const_cast<int**>(&fe.mel_len), (size_t)k.n_mels);
    GET(c, "fe.mel_off", 2u, const_cast<int**>(&fe.mel_off), (size_t)k.n_mels);
    GET(c, "fe.mel_w", 0u, const_cast<float**>(&fe.mel_w), 1);
    fe.n_mel_w = (int)(c->tensors["fe.mel_w"].nbytes / 4);
    fe.n_fft = nfft; fe.hop = k.hop; fe.n_mels = k.n_mels; fe.n_samples = k.segment_samples;
    fe.n_frames = c->T; fe.log_floor = k.log_floor;
    if (fe.n_mel_w > 2304) FAIL(YMT3_ERR_UNSUPPORTED, "fe.mel_w holds %d filterbank weights; the log-mel kernel stages at most 2304", fe.n_mel_w);

    const size_t BT = (size_t)c->maxB * c->T, d = k.d_model, R = c->maxR;
    if (dev_alloc(c, (void**)&c->mel, BT * k.n_mels * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->mel_bf, BT * k.n_mels * 2)) return YMT3_ERR_HIP;
    const size_t AR = c->act_rows = std::max(BT, (size_t)k.max_decode_len);
    if (dev_alloc(c, (void**)&c->h_enc, AR * d * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->xn, AR * d * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->qkv, AR * 3 * c->inner * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->attn, AR * c->inner * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->ff, AR * k.d_ff * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->enc_out, BT * d * 2)) return YMT3_ERR_HIP;
    if (k.encoder_type == YMT3_ENC_PERCEIVER_TF) {
        const int D = k.ptf_d, K = k.n_latents;
        if (D <= 0 || D % 64 || D > 256) FAIL(YMT3_ERR_UNSUPPORTED, "ptf_d must be 64, 128, 192 or 256 (got %d)", D);
        if (K < 16 || K > 64 || K % 16) FAIL(YMT3_ERR_UNSUPPORTED, "n_latents must be 16, 32, 48 or 64 latents per frame (got %d)", K);
        if (k.ptf_blocks < 1 || k.ptf_blocks > 16 || k.ptf_dff <= 0 || k.ptf_dff % 128) FAIL(YMT3_ERR_UNSUPPORTED, "ptf_blocks must be 1..16 and ptf_dff a multiple of 128");
        if (D % 128 || (3 * D) % 128) FAIL(YMT3_ERR_UNSUPPORTED, "ptf_d must be a multiple of 128 (GEMM column tiles)");
        if (c->T > 256 || (k.n_mels != 64 && k.n_mels != 128 && k.n_mels != 256)) FAIL(YMT3_ERR_UNSUPPORTED, "the Perceiver-TF encoder needs n_frames <= 256 and n_mels in {64, 128, 256}");
        if (K != 32 && K != 64) FAIL(YMT3_ERR_UNSUPPORTED, "n_latents must be 32 or 64 (latent self-attention key tiles)");
        const size_t N1 = (size_t)c->maxB * c->T * k.n_mels, N2 = (size_t)c->maxB * c->T * K;
        if (N1 > 0x7fffffffULL / 2) FAIL(YMT3_ERR_UNSUPPORTED, "max_batch too large for the Perceiver-TF encoder workspace");
        if (dev_alloc(c, (void**)&c->p_xs, N1 * D * 2) || dev_alloc(c, (void**)&c->p_kvs, N1 * 2 * D * 2) || dev_alloc(c, (void**)&c->p_z, N2 * D * 4) ||
            dev_alloc(c, (void**)&c->p_zn, N2 * D * 2) || dev_alloc(c, (void**)&c->p_qkv, N2 * 3 * D * 2) || dev_alloc(c, (void**)&c->p_att, N2 * D * 2) ||
            dev_alloc(c, (void**)&c->p_ff, N2 * k.ptf_dff * 2))
            return YMT3_ERR_HIP;
        std::vector<std::string> names = {"spec_w", "spec_pos", "ln_x", "latents", "bias_off", "ln_out", "out_w"};
        for (int b = 0; b < k.ptf_blocks; ++b) {
            const std::string p = std::to_string(b) + ".";
            for (const char* n : {"s.ln_q", "s.wq", "s.wkv", "s.wo", "l.ln1", "l.wqkv", "l.wo", "t.ln1", "t.wqkv", "t.wo"}) names.push_back(p + n);
            for (const char* sub : {"s.", "l.", "t."})
                for (const char* n : {"ln_ff", "wi", "wo2"}) names.push_back(p + sub + n);
        }
        for (const std::string& n : names)
            if (!c->tensors.count("ptf." + n)) FAIL(YMT3_ERR_BLOB, "missing ptf.%s", n.c_str());
    }

    const int nd = k.n_dec_layers;
    const size_t wkv_elems = (size_t)2 * c->inner * d;
    if (dev_alloc(c, (void**)&c->wkv_all, nd * wkv_elems * 2)) return YMT3_ERR_HIP;
    for (int l = 0; l < nd; ++l) {
        bf16_t* src;
        GET(c, "dec." + std::to_string(l) + ".wkv_c", 1u, &src, wkv_elems);
        HIP_TRY(hipMemcpy(c->wkv_all + l * wkv_elems, src, wkv_elems * 2, hipMemcpyDeviceToDevice));
    }
    if (dev_alloc(c, (void**)&c->ckv, (size_t)nd * 2 * BT * c->inner * 2)) return YMT3_ERR_HIP;
    const size_t cache_elems = (size_t)nd * R * k.n_heads * k.max_decode_len * 64;
    if (dev_alloc(c, (void**)&c->kcache, cache_elems * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->vcache, cache_elems * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->h_dec, R * d * 4)) return YMT3_ERR_HIP;
    if (k.dec_ffn == YMT3_FFN_MOE && dev_alloc(c, (void**)&c->h_dec2, R * d * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->dq, R * c->inner * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->dattn, R * c->inner * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->dff, R * k.d_ff * 2)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->logits, R * k.vocab * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->finished, R * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->row_pos, R * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->row_out, R * 8)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->row_prompt, R * 8)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->row_state, R * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->ssq, (size_t)SSQ_TILES * R * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->opart, R * k.n_heads * d * 4)) return YMT3_ERR_HIP;
    if (dev_alloc(c, (void**)&c->ticket, (R / 32 + 1) * CHAIN_LINE * sizeof(unsigned))) return YMT3_ERR_HIP;
    HIP_TRY(hipMemset(c->ticket, 0, (R / 32 + 1) * CHAIN_LINE * sizeof(unsigned)));
    {   // The merged decode kernels (GEMM chain: 256 workgroups of 143 KB LDS; attention pair: 512 of 72 KB) wait for each other inside one
        // launch, so every workgroup of their grids must be resident at once: a kernel is enabled only if the switch allows it AND the
        // runtime's occupancy answer x CUs covers its grid.  YMT3_TEST_CHAIN_UNFIT / YMT3_TEST_PAIR_UNFIT = 1 force "does not fit" for
        // one kernel (tests: a partition on which only one of the two fits must take the separate launches for the other).
        auto env1 = [](const char* n) { const char* v = getenv(n); return v && v[0] == '1'; };
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, c->device));
        const bool init_ok = init_chain_kernels() == 0;
        c->gemm_chain = !env1("YMT3_NO_GEMM_CHAIN") && init_ok && !env1("YMT3_TEST_CHAIN_UNFIT") && dec_chain_fits(prop.multiProcessorCount);
        c->attn_pair = !env1("YMT3_NO_ATTN_PAIR") && init_ok && !env1("YMT3_TEST_PAIR_UNFIT") && dec_attention_pair_fits(prop.multiProcessorCount);
        // ... and the per-step kernel (all six layers in one launch: 512 workgroups of 76 KB) where both of the above are in use
        // -- measured SLOWER than the per-layer launches (271-296 ms per batch against 247: profiles/r03_step_kernel.md), so it is an option
        // (YMT3_STEP_KERNEL=1), bit-identical and tested, not the default
        c->step_kernel = c->gemm_chain && c->attn_pair && env1("YMT3_STEP_KERNEL") && !env1("YMT3_TEST_STEP_UNFIT") && init_step_kernel() == 0 &&
                         dec_step_fits(prop.multiProcessorCount);
        c->moe_chain = k.dec_ffn == YMT3_FFN_MOE && k.n_experts == 8 && c->attn_pair && !env1("YMT3_NO_MOE_CHAIN") && !env1("YMT3_NO_GEMM_CHAIN") &&
                       !env1("YMT3_TEST_CHAIN_UNFIT") && init_moe_chain_kernels() == 0 && moe_chain_fits(prop.multiProcessorCount, k.moe_fp8 != 0);
        if (c->step_kernel) {
            if (dev_alloc(c, (void**)&c->step_sync, (size_t)STEP_SYNC_LINES * CHAIN_LINE * sizeof(unsigned))) return YMT3_ERR_HIP;
            HIP_TRY(hipMemset(c->step_sync, 0, (size_t)STEP_SYNC_LINES * CHAIN_LINE * sizeof(unsigned)));
        }
        if (c->gemm_chain || c->attn_pair || c->moe_chain) {
            if (dev_alloc(c, (void**)&c->chain_sync, CHAIN_SYNC_WORDS * sizeof(unsigned))) return YMT3_ERR_HIP;
            HIP_TRY(hipMemset(c->chain_sync, 0, CHAIN_SYNC_WORDS * sizeof(unsigned)));
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->chain_host_abort), sizeof(unsigned), hipHostMallocDefault));
            *c->chain_host_abort = 0u;
            if (dev_alloc(c, (void**)&c->pair_rows, (size_t)16 * CHAIN_TILES_MAX * 2 * CHAIN_LINE * sizeof(unsigned))) return YMT3_ERR_HIP;
            HIP_TRY(hipMemset(c->pair_rows, 0, (size_t)16 * CHAIN_TILES_MAX * 2 * CHAIN_LINE * sizeof(unsigned)));
        }
    }
    if (k.dec_ffn == YMT3_FFN_MOE) {
        MoeArgs& m = c->moe;
        const size_t P = 2 * R;
        if (R > 1536) FAIL(YMT3_ERR_UNSUPPORTED, "the MoE FFN holds its pair list in LDS: at most 1536 decoder rows (got %zu)", R);
        if (dev_alloc(c, (void**)&m.xn, R * d * 2) || dev_alloc(c, (void**)&m.sel, P * 4) || dev_alloc(c, (void**)&m.gate, P * 4) ||
            dev_alloc(c, (void**)&m.hidden, P * k.d_ff * 2) || dev_alloc(c, (void**)&m.y, P * d * 4))
            return YMT3_ERR_HIP;
        m.E = k.n_experts; m.top_k = k.moe_top_k; m.d_model = d; m.d_ff = k.d_ff; m.eps = k.ln_eps;
    }
    {   // beam search scratch: ancestry tables (two buffers) and snapshots, one byte per (row, position); fed tokens and their log-probabilities
        BeamArgs& b = c->beam;
        b.anc_rows = (int)R;
        b.anc_pitch = (k.max_decode_len + 1 + 15) / 16 * 16;
        b.fed_pitch = k.max_decode_len + 1;
        if (dev_alloc(c, (void**)&b.anc, (size_t)2 * R * b.anc_pitch) || dev_alloc(c, (void**)&b.slot_anc, R * b.anc_pitch) ||
            dev_alloc(c, (void**)&b.fed_tok, R * b.fed_pitch * 4) || dev_alloc(c, (void**)&b.fed_lp, R * b.fed_pitch * 4) ||
            dev_alloc(c, (void**)&b.run, R * 4) || dev_alloc(c, (void**)&b.fin_score, R * 4) || dev_alloc(c, (void**)&b.fin_len, R * 4) ||
            dev_alloc(c, (void**)&b.fin_store, R * 4) || dev_alloc(c, (void**)&b.fin_tok, R * 4) || dev_alloc(c, (void**)&b.fin_lp, R * 4) ||
            dev_alloc(c, (void**)&b.n_fin, R * 4) || dev_alloc(c, (void**)&c->beam_shared, sizeof(BeamShared)))
            return YMT3_ERR_HIP;
        HIP_TRY(hipMemset(b.anc, 0, (size_t)2 * R * b.anc_pitch));
        HIP_TRY(hipMemset(b.slot_anc, 0, R * b.anc_pitch));
        HIP_TRY(hipMemset(b.fed_tok, 0, R * b.fed_pitch * 4));
        HIP_TRY(hipMemset(b.fed_lp, 0, R * b.fed_pitch * 4));
        HIP_TRY(hipMemset(c->beam_shared, 0, sizeof(BeamShared)));
    }
    if (dev_alloc(c, (void**)&c->shared, 8 * sizeof(DecodeShared))) return YMT3_ERR_HIP;
    HIP_TRY(hipMemset(c->shared, 0, 8 * sizeof(DecodeShared)));
    if (getenv("YMT3_STAMP")) {
        if (dev_alloc(c, (void**)&c->stamp_buf, (size_t)STAMP_NODES * STAMP_WGS * 2 * sizeof(unsigned long long))) return YMT3_ERR_HIP;
        HIP_TRY(hipMemset(c->stamp_buf, 0, (size_t)STAMP_NODES * STAMP_WGS * 2 * sizeof(unsigned long long)));
    }
    HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    const char* dh = getenv("YMT3_DEBUG_HOOKS");
    c->debug_hooks = dh && dh[0] == '1';
    const char* ng = getenv("YMT3_NO_GRAPH");
    c->use_graph = !(ng && ng[0] == '1');
    if (const char* gs = getenv("YMT3_GRAPH_STEPS")) { const int v = atoi(gs); if (v >= 1 && v <= 64) c->graph_steps = v; }
    const char* nf = getenv("YMT3_NO_FUSEQ");
    c->fuse_q = !(nf && nf[0] == '1');
    const char* mcl = getenv("YMT3_MOE_COMBINE_LAUNCH");
    c->moe_fold_combine = !(mcl && mcl[0] == '1');
    const char* nfo = getenv("YMT3_NO_FOLD_O");          // A/B: keep the separate self-attention O-projection launch
    c->fold_o = !(nfo && nfo[0] == '1');
    // (YMT3_NO_GEMM_CHAIN / YMT3_NO_ATTN_PAIR = 1 -- the skinny GEMMs as four launches, the two attentions as two -- are read above, with the fit decisions)
    if (const char* mr = getenv("YMT3_DEC_GEMM_MID_ROWS")) c->mid_rows = atoi(mr) < 0 ? -1 : atoi(mr);
    const char* f2 = getenv("YMT3_SELF_ATTN_2WAVE");
    c->force_2wave = f2 && f2[0] == '1';
    if (const char* mm = getenv("YMT3_MERGED_MAX_ROWS")) { const int v = atoi(mm); if (v >= 16 && v <= 16 * CHAIN_TILES_MAX) c->merged_max_rows = v; }
    { const char* tf = getenv("YMT3_STEP_TILES_FREE"); c->step_tiles_free = tf && tf[0] == '1'; }
    if (const char* ar = getenv("YMT3_ABORT_RECOVERY")) c->abort_recovery = ar[0] == '0' ? 0 : 1;
    const char* nc = getenv("YMT3_CHAINS");
    if (nc && atoi(nc) >= 1) { c->n_chains = atoi(nc) > 8 ? 8 : atoi(nc); c->auto_chains = false; }
    for (int i = 0; i < std::max(c->n_chains, 2); ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&c->chain_stream[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));

    // every tensor the kernels will ask for must be present now, not at the first call
    const char* enc_names[] = {"ln1", "wqkv", "wo", "ln2", "wi", "wo2"};
    for (int l = 0; l < k.n_enc_layers; ++l)
        for (const char* n : enc_names)
            if (!c->tensors.count("enc." + std::to_string(l) + "." + n)) FAIL(YMT3_ERR_BLOB, "missing enc.%d.%s", l, n);
    rc = bind_dec_weights(c);                // (the decoder's are bound with dtype and size: wrong ones are refused here, not inside a stream capture)
    if (rc) return rc;
    {
        const char* nt = getenv("YMT3_NO_QKV0_TABLE");       // A/B: keep layer 0's QKV projection launch
        if (!(nt && nt[0] == '1') && k.n_channels == 1 && !c->step_kernel && !c->stamp_buf && 3 * c->inner == QKV0_COLS) {
            rc = build_qkv0_table(c);
            if (rc) return rc;
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    return YMT3_OK;
}

extern "C" int ymt3_create(const ymt3_config* cfg, const void* blob, size_t nbytes, int device, ymt3_handle* out) {
    if (!cfg || !blob || !out) FAIL(YMT3_ERR_ARG, "null argument to ymt3_create");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FAIL(YMT3_ERR_HIP, "no HIP device visible: the HIP path cannot run (there is no CPU fallback)");
    if (device < 0 || device >= ndev) FAIL(YMT3_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
    ymt3_ctx* c = new ymt3_ctx();
    c->cfg = *cfg;
    c->device = device;
    int rc = create_impl(c, cfg, blob, nbytes);
    if (rc != YMT3_OK) {
        ymt3_destroy(c);
        return rc;
    }
    *out = c;
    return YMT3_OK;
}

// ------------------------------------------------------------------------------------------------
// A merged decode kernel gave up waiting (its sticky abort word is raised): leave the merged kernels for good.  The caller has made sure
// nothing of this handle is still running.  Counters, abort words and the cached step graphs (they hold merged launches) are reset; the
// separate launches compute the same bits, so the handle goes on working.
static int merged_fallback(ymt3_ctx* h) {
    h->gemm_chain = h->attn_pair = h->step_kernel = h->moe_chain = false;
    ++h->fallback_count;
    h->forced_abort = false;
    clear_step_graphs(h);
    if (h->chain_sync) HIP_TRY(hipMemset(h->chain_sync, 0, CHAIN_SYNC_WORDS * sizeof(unsigned)));
    if (h->pair_rows) HIP_TRY(hipMemset(h->pair_rows, 0, (size_t)16 * CHAIN_TILES_MAX * 2 * CHAIN_LINE * sizeof(unsigned)));
    if (h->step_sync) HIP_TRY(hipMemset(h->step_sync, 0, (size_t)STEP_SYNC_LINES * CHAIN_LINE * sizeof(unsigned)));
    HIP_TRY(hipDeviceSynchronize());
    if (h->chain_host_abort) *h->chain_host_abort = 0u;
    return YMT3_OK;
}

static int check_call(ymt3_handle h, int B) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (B < 0 || B > h->maxB) FAIL(YMT3_ERR_ARG, "B=%d outside [0, max_batch=%d]", B, h->maxB);
    HIP_TRY(hipSetDevice(h->device));
    if (h->chain_host_abort && *static_cast<volatile unsigned*>(h->chain_host_abort)) {
        // an earlier call's merged kernel gave up (> 1 s without its co-resident workgroups: were all CUs available to it?) and nobody has
        // dealt with it yet (ymt3_set_abort_recovery(h, 0), or a measurement call): that call's ids are INT32_MIN; this and every later
        // call run the separate launches
        HIP_TRY(hipDeviceSynchronize());
        int rc = merged_fallback(h);
        if (rc) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------- constraints (include/ymt3.h)
struct ymt3_constraint_s {
    ymt3_ctx* owner;
    int device, n_states, vocab, words;
    uint32_t* allowed = nullptr;        // [n_states][words]
    int32_t* next = nullptr;            // [n_states][vocab]
};

extern "C" void ymt3_constraint_destroy(ymt3_constraint c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->allowed) (void)hipFree(c->allowed);
    if (c->next) (void)hipFree(c->next);
    delete c;
}

extern "C" int ymt3_constraint_create(ymt3_handle h, int n_states, int vocab, const uint32_t* allowed_bits_host, const int32_t* next_host,
                                      ymt3_constraint* out) {
    if (!out) FAIL(YMT3_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!allowed_bits_host || !next_host) FAIL(YMT3_ERR_ARG, "null automaton table");
    if (vocab != h->cfg.vocab) FAIL(YMT3_ERR_ARG, "constraint vocab=%d != the model's vocab=%d", vocab, h->cfg.vocab);
    if (n_states < 1 || n_states > 1024) FAIL(YMT3_ERR_ARG, "n_states=%d outside [1, 1024]", n_states);
    const int words = (vocab + 31) / 32;
    for (int st = 0; st < n_states; ++st) {
        bool any = false;
        for (int i = 0; i < vocab && !any; ++i) any = (allowed_bits_host[(size_t)st * words + i / 32] >> (i % 32)) & 1u;
        if (!any) FAIL(YMT3_ERR_ARG, "state %d allows no token", st);
        for (int i = 0; i < vocab; ++i) {
            const int32_t nx = next_host[(size_t)st * vocab + i];
            if (nx < 0 || nx >= n_states) FAIL(YMT3_ERR_ARG, "next[%d][%d]=%d outside [0, %d)", st, i, nx, n_states);
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    ymt3_constraint c = new ymt3_constraint_s{h, h->device, n_states, vocab, words};
    const size_t ab = (size_t)n_states * words * sizeof(uint32_t), nb = (size_t)n_states * vocab * sizeof(int32_t);
    if (hipMalloc(reinterpret_cast<void**>(&c->allowed), ab) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&c->next), nb) != hipSuccess ||
        hipMemcpy(c->allowed, allowed_bits_host, ab, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->next, next_host, nb, hipMemcpyHostToDevice) != hipSuccess) {
        ymt3_constraint_destroy(c);
        FAIL(YMT3_ERR_HIP, "constraint upload (%zu bytes) failed", ab + nb);
    }
    *out = c;
    return YMT3_OK;
}

// the kernels' view of a call's constraint (all null without one)
static int constraint_view(ymt3_handle h, ymt3_constraint c, const int32_t* start_state_dev, ConstraintView* cv) {
    *cv = ConstraintView{};
    if (!c) {
        if (start_state_dev) FAIL(YMT3_ERR_ARG, "start states without a constraint");
        return 0;
    }
    if (c->owner != h) FAIL(YMT3_ERR_ARG, "the constraint belongs to another handle");
    if (c->vocab != h->cfg.vocab) FAIL(YMT3_ERR_ARG, "constraint vocab=%d != the model's vocab=%d", c->vocab, h->cfg.vocab);
    cv->allowed = c->allowed;
    cv->next = c->next;
    cv->words = c->words;
    cv->n_states = c->n_states;
    cv->start = start_state_dev;
    return 0;
}

extern "C" int ymt3_logmel(ymt3_handle h, const float* audio_dev, int B, float* mel_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!audio_dev || !mel_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    LAUNCH(launch_logmel(h->fe, audio_dev, mel_dev, B, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

// a9: Perceiver-TF encoder (build-defined spec: oracle/perceiver_oracle.py).  Every FLOP is in the GEMM,
// norm and sequence-attention kernels the T5 encoder uses; this is their orchestration over the (B, T, F', C) spectral tokens
// and the (B, T, K, D) latent array.
static int encode_ptf(ymt3_handle h, const float* mel, int B, bf16_t* enc_out, hipStream_t s) {
    const ymt3_config& k = h->cfg;
    const int T = h->T, F = k.n_mels, K = k.n_latents, D = k.ptf_d, Hs = D / 64, dff = k.ptf_dff, d = k.d_model;
    const int N1 = B * T * F, N2 = B * T * K;
    bf16_t *w, *lat, *pos;
    float *f, *specw;
    const float* tbias;
    GET(h, "ptf.spec_w", 0u, &specw, (size_t)D);
    GET(h, "ptf.spec_pos", 1u, &pos, (size_t)F * D);
    GET(h, "ptf.ln_x", 0u, &f, (size_t)D);
    LAUNCH(launch_spec_embed(mel, specw, pos, f, h->p_xs, (long long)N1, F, D, k.ln_eps, s));
    GET(h, "ptf.latents", 1u, &lat, (size_t)K * D);
    LAUNCH(launch_broadcast_bf16(lat, h->p_z, B * T, (size_t)K * D, s));
    GET(h, "ptf.bias_off", 0u, const_cast<float**>(&tbias), (size_t)Hs * (2 * T - 1));
    auto gemm = [&](int epi, const bf16_t* A, const bf16_t* Wt, void* out, int M, int N, int Kd) -> int {
        GemmArgs g{A, Wt, out, nullptr, M, N, Kd, Kd, Kd, N, 0, 0, 0};
        LAUNCH(launch_gemm(epi, g, s));
        return YMT3_OK;
    };
    auto ffn = [&](const std::string& p) -> int {
        GET(h, p + "ln_ff", 0u, &f, (size_t)D);
        LAUNCH(launch_rmsnorm(h->p_z, f, h->p_zn, N2, D, k.ln_eps, s));
        GET(h, p + "wi", 1u, &w, (size_t)dff * D);
        int rc = gemm(EPI_BF16_RELU, h->p_zn, w, h->p_ff, N2, dff, D);
        if (rc) return rc;
        GET(h, p + "wo2", 1u, &w, (size_t)D * dff);
        return gemm(EPI_RESID, h->p_ff, w, h->p_z, N2, D, dff);
    };
    for (int blk = 0; blk < k.ptf_blocks; ++blk) {
        const std::string p = "ptf." + std::to_string(blk) + ".";
        int rc;
        // spectral cross-attention: one sequence per (segment, frame), K latent queries over the frame's F' spectral tokens
        GET(h, p + "s.wkv", 1u, &w, (size_t)2 * D * D);
        if ((rc = gemm(EPI_BF16, h->p_xs, w, h->p_kvs, N1, 2 * D, D))) return rc;
        GET(h, p + "s.ln_q", 0u, &f, (size_t)D);
        LAUNCH(launch_rmsnorm(h->p_z, f, h->p_zn, N2, D, k.ln_eps, s));
        GET(h, p + "s.wq", 1u, &w, (size_t)D * D);
        if ((rc = gemm(EPI_BF16, h->p_zn, w, h->p_qkv, N2, D, D))) return rc;
        {
            SeqAttnArgs a{};
            a.q = h->p_qkv; a.k = h->p_kvs; a.v = h->p_kvs + D; a.out = h->p_att; a.bias_off = nullptr;
            a.n_seq = B * T; a.H = Hs; a.Tq = K; a.Tk = F; a.inner_n = 1;
            a.q_outer = (long long)K * D; a.q_step = D; a.kv_outer = (long long)F * 2 * D; a.kv_step = 2 * D; a.o_outer = (long long)K * D; a.o_step = D;
            LAUNCH(launch_seq_attention(a, s));
        }
        GET(h, p + "s.wo", 1u, &w, (size_t)D * D);
        if ((rc = gemm(EPI_RESID, h->p_att, w, h->p_z, N2, D, D))) return rc;
        if ((rc = ffn(p + "s."))) return rc;
        // latent transformer: the same sequences, self-attention among the K latents
        GET(h, p + "l.ln1", 0u, &f, (size_t)D);
        LAUNCH(launch_rmsnorm(h->p_z, f, h->p_zn, N2, D, k.ln_eps, s));
        GET(h, p + "l.wqkv", 1u, &w, (size_t)3 * D * D);
        if ((rc = gemm(EPI_BF16, h->p_zn, w, h->p_qkv, N2, 3 * D, D))) return rc;
        {
            SeqAttnArgs a{};
            a.q = h->p_qkv; a.k = h->p_qkv + D; a.v = h->p_qkv + 2 * D; a.out = h->p_att; a.bias_off = nullptr;
            a.n_seq = B * T; a.H = Hs; a.Tq = K; a.Tk = K; a.inner_n = 1;
            a.q_outer = a.kv_outer = (long long)K * 3 * D; a.q_step = a.kv_step = 3 * D; a.o_outer = (long long)K * D; a.o_step = D;
            LAUNCH(launch_seq_attention(a, s));
        }
        GET(h, p + "l.wo", 1u, &w, (size_t)D * D);
        if ((rc = gemm(EPI_RESID, h->p_att, w, h->p_z, N2, D, D))) return rc;
        if ((rc = ffn(p + "l."))) return rc;
        // temporal transformer: one sequence per (segment, latent), positions = the T frames (stride K rows), T5 relative bias
        GET(h, p + "t.ln1", 0u, &f, (size_t)D);
        LAUNCH(launch_rmsnorm(h->p_z, f, h->p_zn, N2, D, k.ln_eps, s));
        GET(h, p + "t.wqkv", 1u, &w, (size_t)3 * D * D);
        if ((rc = gemm(EPI_BF16, h->p_zn, w, h->p_qkv, N2, 3 * D, D))) return rc;
        {
            SeqAttnArgs a{};
            a.q = h->p_qkv; a.k = h->p_qkv + D; a.v = h->p_qkv + 2 * D; a.out = h->p_att; a.bias_off = tbias;
            a.n_seq = B * K; a.H = Hs; a.Tq = T; a.Tk = T; a.inner_n = K;
            a.q_outer = a.kv_outer = (long long)T * K * 3 * D; a.q_inner = a.kv_inner = 3 * D; a.q_step = a.kv_step = (long long)K * 3 * D;
            a.o_outer = (long long)T * K * D; a.o_inner = D; a.o_step = (long long)K * D;
            LAUNCH(launch_seq_attention(a, s));
        }
        GET(h, p + "t.wo", 1u, &w, (size_t)D * D);
        if ((rc = gemm(EPI_RESID, h->p_att, w, h->p_z, N2, D, D))) return rc;
        if ((rc = ffn(p + "t."))) return rc;
    }
    // (B, T, K, D) -> per-latent norm -> the K latents of a frame side by side -> d_model
    GET(h, "ptf.ln_out", 0u, &f, (size_t)D);
    LAUNCH(launch_rmsnorm(h->p_z, f, h->p_zn, N2, D, k.ln_eps, s));
    GET(h, "ptf.out_w", 1u, &w, (size_t)d * K * D);
    int rc = gemm(EPI_F32, h->p_zn, w, h->h_enc, B * T, d, K * D);
    if (rc) return rc;
    GET(h, "enc.ln_f", 0u, &f, (size_t)d);
    LAUNCH(launch_rmsnorm(h->h_enc, f, enc_out, B * T, d, k.ln_eps, s));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

static int encode_impl(ymt3_handle h, const float* mel, int B, bf16_t* enc_out, hipStream_t s) {
    const ymt3_config& k = h->cfg;
    if (k.encoder_type == YMT3_ENC_PERCEIVER_TF) return encode_ptf(h, mel, B, enc_out, s);
    const int M = B * h->T, d = k.d_model, inner = h->inner;
    LAUNCH(launch_f32_to_bf16(mel, h->mel_bf, (size_t)M * k.n_mels, s));
    bf16_t* w;
    float* f;
    {
        float* bias;
        GET(h, "in_proj.w", 1u, &w, (size_t)d * k.n_mels);
        GET(h, "in_proj.b", 0u, &bias, (size_t)d);
        GemmArgs g{h->mel_bf, w, h->h_enc, bias, M, d, k.n_mels, k.n_mels, k.n_mels, d, 0, 0, 0};
        LAUNCH(launch_gemm(EPI_F32, g, s));
    }
    const float* bias_off;
    GET(h, "enc.bias_off", 0u, const_cast<float**>(&bias_off), (size_t)k.n_heads * (2 * h->T - 1));
    for (int l = 0; l < k.n_enc_layers; ++l) {
        const std::string p = "enc." + std::to_string(l) + ".";
        GET(h, p + "ln1", 0u, &f, (size_t)d);
        LAUNCH(launch_rmsnorm(h->h_enc, f, h->xn, M, d, k.ln_eps, s));
        GET(h, p + "wqkv", 1u, &w, (size_t)3 * inner * d);
        { GemmArgs g{h->xn, w, h->qkv, nullptr, M, 3 * inner, d, d, d, 3 * inner, 0, 0, 0}; LAUNCH(launch_gemm(EPI_BF16, g, s)); }
        LAUNCH(launch_enc_attention(h->qkv, bias_off, h->attn, B, h->T, k.n_heads, s));
        GET(h, p + "wo", 1u, &w, (size_t)d * inner);
        { GemmArgs g{h->attn, w, h->h_enc, nullptr, M, d, inner, inner, inner, d, 0, 0, 0}; LAUNCH(launch_gemm(EPI_RESID, g, s)); }
        GET(h, p + "ln2", 0u, &f, (size_t)d);
        LAUNCH(launch_rmsnorm(h->h_enc, f, h->xn, M, d, k.ln_eps, s));
        GET(h, p + "wi", 1u, &w, (size_t)k.d_ff * d);
        { GemmArgs g{h->xn, w, h->ff, nullptr, M, k.d_ff, d, d, d, k.d_ff, 0, 0, 0}; LAUNCH(launch_gemm(EPI_BF16_RELU, g, s)); }
        GET(h, p + "wo2", 1u, &w, (size_t)d * k.d_ff);
        { GemmArgs g{h->ff, w, h->h_enc, nullptr, M, d, k.d_ff, k.d_ff, k.d_ff, d, 0, 0, 0}; LAUNCH(launch_gemm(EPI_RESID, g, s)); }
    }
    GET(h, "enc.ln_f", 0u, &f, (size_t)d);
    LAUNCH(launch_rmsnorm(h->h_enc, f, enc_out, M, d, k.ln_eps, s));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_encode(ymt3_handle h, const float* mel_dev, int B, void* enc_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!mel_dev || !enc_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    return encode_impl(h, mel_dev, B, static_cast<bf16_t*>(enc_dev), (hipStream_t)stream);
}

// the beam kernels' arguments for R rows of W beams: the handle's scratch, the step's buffers, the embedding tables
static BeamArgs beam_args(ymt3_handle h, int R, int W, DecodeShared* shared, bool slot) {
    const ymt3_config& k = h->cfg;
    BeamArgs b = h->beam;
    b.logits = h->logits; b.h = h->h_dec; b.shared = shared; b.beam = h->beam_shared; b.finished = h->finished; b.ssq = h->ssq; b.ssq_stride = h->maxR;
    b.R = R; b.V = k.vocab; b.d = k.d_model; b.n_channels = k.n_channels; b.eos_id = k.eos_id; b.pad_id = k.pad_id; b.W = W; b.row_state = h->row_state;
    if (slot) { b.row_pos = h->row_pos; b.row_out = h->row_out; b.row_prompt = h->row_prompt; }
    b.embed = h->dec.embed; b.chan_embed = h->dec.chan_embed;
    return b;
}

// what every user of ArgmaxArgs fills alike for R rows (the step's feeding kernel, decode_init, the slot kernels): loop state, the
// embedding tables, the automaton states and, in a slot mode, the per-row positions and offsets
static ArgmaxArgs argmax_base(ymt3_handle h, int R, bool slot) {
    const ymt3_config& k = h->cfg;
    ArgmaxArgs a{};
    a.h = h->h_dec; a.shared = h->shared; a.finished = h->finished; a.ssq = h->ssq; a.ssq_stride = h->maxR;
    a.R = R; a.V = k.vocab; a.d = k.d_model; a.n_channels = k.n_channels; a.eos_id = k.eos_id; a.pad_id = k.pad_id;
    a.embed = h->dec.embed; a.chan_embed = h->dec.chan_embed; a.row_state = h->row_state;
    if (slot) { a.row_pos = h->row_pos; a.row_out = h->row_out; a.row_prompt = h->row_prompt; }
    return a;
}

// The two row-count thresholds at which a launcher takes a kernel that sums in another order, so that a step's bits depend on which side
// of them its R lies.  The qkv0 table's gate, plan_step and decode_run's two-chains rule all ask here.
// Do R rows take the mid-size tile decode GEMMs?  launch_dec_gemm's rule over DecGemmArgs::mid_rows, which every GEMM of a step gets from
// the handle (YMT3_DEC_GEMM_MID_ROWS at create; < 0: DEC_GEMM_MID_ROWS, 0: never); they accumulate K in one chain, not in eight slices.
static bool gemm_mid_tiles(ymt3_handle h, int R) { return h->mid_rows != 0 && R >= (h->mid_rows > 0 ? h->mid_rows : DEC_GEMM_MID_ROWS); }
// Do R rows take the 2-waves-per-(row, head) attention?  launch_dec_attention's `many`: beyond 2048 (row, head) workgroups, or forced by
// DecAttnArgs::force_many.  (That launcher holds the figure as a literal; it is repeated here and nowhere else in this file.)
static bool attn_many_rows(ymt3_handle h, int R) { return h->force_2wave || R * h->cfg.n_heads > 2048; }

// Does a decode call whose largest step has `rows` rows take layer 0's q / k / v from the table?  Only where the launch it replaces is the
// 16-row-tile kernel, whose bits the table holds (the mid-size tiles accumulate K differently); never a beam call (its selection kernels
// do not gather) and never the profiled call (ymt3_profile_decode keeps the launch sequence its classes are defined by).
static bool qkv0_applies(ymt3_handle h, int rows, bool beam, bool profiled) {
    return h->qkv0_table && !beam && !profiled && h->cfg.n_channels == 1 && !gemm_mid_tiles(h, rows);
}
// the feeding kernels' side of it: where the fed id's table row goes
static void qkv0_wire(ymt3_handle h, bool qkv0, ArgmaxArgs* a) {
    if (!qkv0) return;
    a->qkv0 = h->qkv0_table; a->q0 = h->dq; a->kcache0 = h->kcache; a->vcache0 = h->vcache; a->H = h->cfg.n_heads; a->L = h->cfg.max_decode_len;
}

// The shape of a call's steps: `R` rows in all, cut into n_chains contiguous, near-equal row ranges (chain_shape picks one).
static StepShape step_shape(ymt3_handle h, StepMode mode, int B, int W, int R, int n_chains, bool profiled) {
    StepShape S;
    S.mode = mode; S.B = B; S.W = W; S.n_chains = n_chains; S.R = R; S.solo = n_chains == 1; S.profiled = profiled;
    S.qkv0 = qkv0_applies(h, (R + n_chains - 1) / n_chains, W > 0, profiled);      // (the largest chain's rows)
    return S;
}
static StepShape chain_shape(StepShape S, int c) {
    const int R = S.R, n = S.n_chains;
    S.chain = c;
    S.row0 = c * (R / n) + std::min(c, R % n);
    S.R = R / n + (c < R % n ? 1 : 0);
    return S;
}

// Which kernels a step takes: a pure function of the handle's create-time configuration and the step's shape.  mid_tiles and attn_many
// name kernels that sum in another order (bits_agree); every other choice gives the same bits and differs in launches and time.
struct StepPlan {
    int rows_kv;            // decoder rows per segment's cross-attention K/V: n_channels, times W in a beam call
    bool mid_tiles, attn_many;
    bool fold_combine, mc, fold, merged_regime, chain, pair_ok, moe_chain, stepk;
    bool merged() const { return chain || pair_ok || moe_chain; }      // the step holds merged kernels: their abort word must be looked at
};
static bool bits_agree(const StepPlan& a, const StepPlan& b) { return a.mid_tiles == b.mid_tiles && a.attn_many == b.attn_many; }
static StepPlan plan_step(ymt3_handle h, const StepShape& S) {
    const ymt3_config& k = h->cfg;
    const int d = k.d_model, inner = h->inner, H = k.n_heads, bW = S.W, row0 = S.row0, R = S.R;
    const bool solo = S.solo;
    StepPlan p{};
    p.mid_tiles = gemm_mid_tiles(h, R);
    p.attn_many = attn_many_rows(h, R);
    // MoE with the combine folded away: after an MoE FFN the residual stream is hcur + (y[2r] + y[2r+1]) until the next norm GEMM
    // (the next layer's QKV projection, or lm_head) has formed it; that QKV kernel stores it to the other buffer, which the rest of
    // its layer then uses.  Needs the 16-row decode GEMMs (below the mid-size tile threshold).
    p.fold_combine = k.dec_ffn == YMT3_FFN_MOE && h->moe_fold_combine && !p.mid_tiles;
    // all channels of a segment share its cross-attention K/V: one workgroup per (segment, head) serves them together (mc_cross_attn.hip)
    // (a beam call: the W beams of a group share their segment's K/V exactly as channels do -- rows_kv = n_channels * W rows per segment)
    p.rows_kv = k.n_channels * (bW > 0 ? bW : 1);
    p.mc = h->fuse_q && p.rows_kv >= 2 && p.rows_kv <= 16 && (h->T == 128 || h->T == 256 || h->T == 512) &&
           row0 % p.rows_kv == 0 && R % p.rows_kv == 0;
    // fold_o: the self-attention kernel leaves per-head O-projection partials; the fused cross-attention and the cross
    // O-projection's residual read sum them (one launch less per layer, same bits).  Needs the 8-wave attention kernels
    // and the per-row fused cross-attention
    // and pays only while the per-(row, head) pull of wo (64 KB each) stays small against the launch it removes: +0.3 % at 64 rows,
    // -1.4 % at 128, -3.5 % at 256 (profiles/r02_b256_fold_fuseq_variants.txt); same bits either way
    const bool merged_rows = solo && k.n_channels == 1 && row0 == 0 && R <= h->merged_max_rows && h->attn_pair && h->pair_rows;     // (the pair kernel keeps the fold worthwhile beyond 96 rows)
    // (not for one of several concurrent chains: its 64 KB weight pulls per (row, head) share the chip badly -- two 96-row halves with it are no
    // faster than one 192-row chain, without it 6 % faster: profiles/r03_chains_many_rows.txt)
    // (a beam call runs the separate launches: its self-attention follows the ancestry table and has no folded form)
    p.fold = bW == 0 && h->fold_o && h->fuse_q && !p.mc && !h->force_2wave && H == 8 && d == 512 && ((R <= 96 && solo) || merged_rows);
    // The merged kernels' regime: one channel, up to 64 rows, and this step the only decode stream of the handle (`solo`: with YMT3_CHAINS > 1
    // other row ranges replay on other streams, and the merged kernels need every CU for their own workgroups while they run).
    p.merged_regime = p.fold && solo && k.n_channels == 1 && R <= h->merged_max_rows && row0 == 0;
    // GEMM chain (dec_chain.hip): after a layer's cross-attention, ONE launch does the cross O-projection, the FFN and the NEXT
    // layer's QKV projection (or lm_head) -- decided per step shape, same bits as the four launches.
    p.chain = h->gemm_chain && h->chain_sync && p.merged_regime && k.dec_ffn != YMT3_FFN_MOE && inner == 512 && k.d_ff == 2048 &&
              k.vocab % 32 == 0 && k.vocab / 32 >= 32 && k.vocab / 32 <= 64;
    // attention pair (decode.hip: dec_attn_pair_kernel): a layer's two attention kernels as one launch wherever the folded
    // O-projection and the fused query projection apply to one channel of up to 64 rows (dense or MoE FFN alike)
    p.pair_ok = h->attn_pair && h->pair_rows && p.merged_regime;
    // MoE chain (moe_chain.hip): cross O-projection -> router -> expert FFN-in -> expert FFN-out -> the next QKV projection / lm_head as one launch
    p.moe_chain = h->moe_chain && h->chain_sync && p.pair_ok && p.fold_combine && k.dec_ffn == YMT3_FFN_MOE && k.n_experts == 8 && inner == 512 && k.d_ff == 2048 &&
                  k.vocab % 32 == 0 && k.vocab / 32 >= 32 && k.vocab / 32 <= 64 && h->h_dec2;
    // the per-step kernel (dec_step.hip): layer 0's QKV projection, then ALL layers' attention pairs and GEMM chains as one launch
    p.stepk = h->step_kernel && h->step_sync && p.chain && p.pair_ok && R <= 64 && k.n_dec_layers <= 8 && h->T <= 0xfff;
    return p;
}

// What layer l's merged launch (GEMM chain, MoE chain, a layer of the step kernel) ends with: the NEXT layer's QKV projection into that
// layer's cache slabs, or after the last layer the lm_head (no cache).
struct NextStage { bool last; const bf16_t* w3; const float* gain3; int mode3, N3; bf16_t *kcache, *vcache; };
static NextStage next_stage(ymt3_handle h, int l) {
    const ymt3_config& k = h->cfg;
    if (l + 1 == k.n_dec_layers) return {true, h->dec.lm_head, h->dec.ln_f, DG_NORM_LOGITS, k.vocab, nullptr, nullptr};
    const size_t next_cache = (size_t)(l + 1) * h->maxR * k.n_heads * k.max_decode_len * 64;
    const LayerW& N = h->dec.layer[(size_t)l + 1];
    return {false, N.wqkv, N.ln1, DG_NORM_QKV_CACHE, 3 * h->inner, h->kcache + next_cache, h->vcache + next_cache};
}

// ---------------------------------------------------------------- one decoder step
// What one stage of a step hands to the next.
struct StepCarry {
    float* hcur;            // the residual buffer in use.  Set: h_dec at the step's start; moved to the other buffer by whoever forms h + (y0 + y1) there -- the QKV
                            // projection with a pending combine (layer_projection), the MoE chain's next-QKV stage (layer_tail).  Read: every launch on the stream
    const float* pend;      // MoE with the combine folded away: expert outputs still to be added.  Set: layer_tail's separate stages.  Consumed: the next
                            // layer_projection, or the lm_head
    bool qkv_done;          // the next layer's QKV projection is done.  Set: layer_tail's merged launch.  Consumed: the next layer_projection
    bool lm_done;           // so is the lm_head.  Set: the last layer's merged launch.  Consumed: Step::run
};
// One step being launched: its shape, the plan that follows from it, the chain's loop state (every kernel reads the position from it, or
// from row_pos in a slot mode) and the stream; then one argument builder per kind of launch, and the stages that launch them.
// A builder returns a freshly value-initialised struct holding the fields its launcher and kernel read (the kernels take the struct by
// value; what a launch does not read stays zero).  No struct is changed after a launch has used it, none serves two launches.
struct Step {
    ymt3_handle h;
    StepShape S;
    StepPlan P;
    DecodeShared* shared;
    hipStream_t s;
    const ymt3_config& k() const { return h->cfg; }
    const LayerW& W(int l) const { return h->dec.layer[(size_t)l]; }
    const int* row_pos() const { return S.slot() ? h->row_pos : nullptr; }
    size_t layer_cache(int l) const { return (size_t)l * h->maxR * k().n_heads * k().max_decode_len * 64; }       // layer l's self-attention K (or V)
    bf16_t* cross_kv(int l, int v) const { return h->ckv + (size_t)(2 * l + v) * S.B * k().n_heads * h->T * 64; }  // layer l's cross-attention K (v = 1: V) slabs
    float* other(const float* hcur) const { return hcur == h->h_dec ? h->h_dec2 : h->h_dec; }                      // MoE: the residual buffer not in use

    // the decode GEMMs: every one reads its rows, the sum(h^2) partials (norm prologue: read; DG_RESID: written), the tile threshold, its stamp slot
    DecGemmArgs gemm_base(int cls, const bf16_t* Wt, int N, int K) const {
        DecGemmArgs a{};
        a.row0 = S.row0; a.R = S.R; a.W = Wt; a.N = N; a.K = K; a.ssq = h->ssq; a.ssq_stride = h->maxR; a.mid_rows = h->mid_rows;
        a.stamp = next_stamp(h, cls, a.N / 16 * ((S.R + 15) / 16));
        return a;
    }
    // out = norm(x) * gain . W^T: cross Q-projection, FFN-in; the base of the QKV projection and the lm_head
    DecGemmArgs gemm_norm(int cls, const float* x, const float* gain, const bf16_t* Wt, int N, bf16_t* out) const {
        DecGemmArgs a = gemm_base(cls, Wt, N, k().d_model);
        a.x_f32 = x; a.gain = gain; a.eps = k().ln_eps; a.out_bf16 = out;
        return a;
    }
    // hcur += in . W^T: self and cross O-projection, FFN-out; part: the folded self-attention O-projection's partials, added first (cross O only)
    DecGemmArgs gemm_resid(int cls, const bf16_t* in, const bf16_t* Wt, int K, float* hcur, const float* part = nullptr) const {
        DecGemmArgs a = gemm_base(cls, Wt, k().d_model, K);
        a.a_bf16 = in; a.out_f32 = hcur; a.part = part;
        return a;
    }
    // layer l's QKV projection: q to dq, this position's k / v into the layer's cache slabs; a pending combine is formed in the prologue
    // and the completed residual row stored to the other buffer
    DecGemmArgs qkv_args(int l, const StepCarry& y) const {
        DecGemmArgs a = gemm_norm(PC_QKV, y.hcur, W(l).ln1, W(l).wqkv, 3 * h->inner, h->dq);
        a.kcache = h->kcache + layer_cache(l); a.vcache = h->vcache + layer_cache(l); a.H = k().n_heads; a.L = k().max_decode_len;
        a.shared = shared; a.row_pos = row_pos();
        if (y.pend) { a.pend_y = y.pend; a.h_out = other(y.hcur); }
        return a;
    }
    DecGemmArgs lm_head_args(const StepCarry& y) const {
        DecGemmArgs a = gemm_norm(PC_LM_HEAD, y.hcur, h->dec.ln_f, h->dec.lm_head, k().vocab, nullptr);
        a.out_f32 = h->logits;
        a.pend_y = y.pend;                               // the last layer's expert outputs, if their combine was folded away
        return a;
    }
    // the self-attention half of layer l: its cache slabs up to the row's position; with the fold it ends in the head's O-projection partial
    DecAttnArgs self_attn_args(int l) const {
        const int L = k().max_decode_len;
        DecAttnArgs t{};
        t.q = h->dq; t.k = h->kcache + layer_cache(l); t.v = h->vcache + layer_cache(l); t.out = h->dattn; t.bias = h->dec.bias_dist;
        t.shared = shared; t.row_pos = row_pos(); t.row0 = S.row0; t.R = S.R; t.H = k().n_heads;
        t.slab_keys = L; t.bias_stride = L; t.rows_per_kv = 1; t.force_many = h->force_2wave ? 1 : 0;
        if (P.fold) { t.wo = W(l).wo; t.opart = h->opart; }
        return t;
    }
    // the cross-attention half of layer l, per row: the segment's T keys.  Fused query projection (default): the kernel norms the residual
    // row itself -- with the fold, h + the self-attention's partials.  Else q comes from the separate projection's dq.
    DecAttnArgs cross_attn_args(int l, const float* hcur) const {
        DecAttnArgs t{};
        t.k = cross_kv(l, 0); t.v = cross_kv(l, 1); t.out = h->dattn;
        t.n_keys_const = h->T; t.slab_keys = h->T; t.rows_per_kv = P.rows_kv; t.row0 = S.row0; t.R = S.R; t.H = k().n_heads;
        t.force_many = h->force_2wave ? 1 : 0;           // (the launcher's choice of the unfused kernel; it refuses the fold with it)
        if (h->fuse_q) {
            t.wq = W(l).wq_c; t.x_f32 = hcur; t.gain = W(l).ln2; t.ssq = h->ssq; t.ssq_stride = h->maxR; t.eps = k().ln_eps;
            if (P.fold) t.ipart = h->opart;
        } else t.q = h->dq;
        if (P.chain || P.moe_chain) t.chain_sync = h->chain_sync;      // it zeroes the arrival counters of the merged tail launched next
        return t;
    }
    // all channels (beams) of a segment share its cross-attention K/V: one workgroup per (segment, head) serves them together, query projection fused
    McCrossArgs mc_cross_args(int l, const float* hcur) const {
        const size_t seg0 = (size_t)(S.row0 / P.rows_kv) * k().n_heads * h->T * 64;
        McCrossArgs mcx{};
        mcx.x_f32 = hcur; mcx.gain = W(l).ln2; mcx.ssq = h->ssq; mcx.ssq_stride = h->maxR; mcx.eps = k().ln_eps;
        mcx.wq = W(l).wq_c; mcx.k = cross_kv(l, 0) + seg0; mcx.v = cross_kv(l, 1) + seg0;
        mcx.out = h->dattn; mcx.row0 = S.row0; mcx.n_seg = S.R / P.rows_kv; mcx.n_channels = P.rows_kv; mcx.H = k().n_heads; mcx.T = h->T;
        return mcx;
    }
    // GEMM chain (dec_chain.hip): layer l's cross O-projection, FFN-in, FFN-out and `ns` as one launch
    ChainArgs chain_args(int l, float* hcur, const NextStage& ns) const {
        ChainArgs cg{};
        cg.w0 = W(l).wo_c; cg.w1 = W(l).wi; cg.w2 = W(l).wo2; cg.w3 = ns.w3;
        cg.attn = h->dattn; cg.part = h->opart; cg.h = hcur; cg.ssq = h->ssq; cg.ssq_stride = h->maxR;
        cg.gain1 = W(l).ln3; cg.gain3 = ns.gain3;
        cg.dff = h->dff; cg.d_ff = k().d_ff;
        cg.mode3 = ns.mode3; cg.N3 = ns.N3;
        cg.out_q = h->dq; cg.kcache = ns.kcache; cg.vcache = ns.vcache;
        cg.logits = h->logits; cg.H = k().n_heads; cg.L = k().max_decode_len; cg.shared = shared; cg.row_pos = row_pos();
        cg.row0 = S.row0; cg.R = S.R; cg.eps = k().ln_eps;
        cg.sync = h->chain_sync; cg.host_abort = h->chain_host_abort;
        { static const int nsub_env = [] { const char* e = getenv("YMT3_CHAIN_NSUB"); return e ? (int)strtol(e, nullptr, 16) : 0; }(); cg.nsub = nsub_env; }
        cg.stamp = next_stamp(h, PC_CHAIN, 256);
        return cg;
    }
    // MoE chain (moe_chain.hip): cross O-projection -> router -> expert FFN-in -> expert FFN-out -> `ns`, which also forms the combine
    MoeChainArgs moe_chain_args(int l, float* hcur, const NextStage& ns) const {
        MoeChainArgs mc2{};
        mc2.wo_c = W(l).wo_c; mc2.w3 = ns.w3;
        if (k().moe_fp8) { mc2.wi = W(l).wi_q8; mc2.wo = W(l).wo_q8; mc2.wi_s = W(l).wi_s; mc2.wo_s = W(l).wo_s; }
        else { mc2.wi = W(l).wi; mc2.wo = W(l).wo2; }
        mc2.attn = h->dattn; mc2.h = hcur; mc2.part = h->opart; mc2.ssq = h->ssq; mc2.ssq_stride = h->maxR;
        mc2.gain_r = W(l).ln3; mc2.router = W(l).router; mc2.xn = h->moe.xn; mc2.sel = h->moe.sel; mc2.gate = h->moe.gate; mc2.hidden = h->moe.hidden; mc2.y = h->moe.y;
        mc2.gain3 = ns.gain3; mc2.mode3 = ns.mode3; mc2.N3 = ns.N3;
        mc2.h_out = ns.last ? nullptr : other(hcur);
        mc2.out_q = h->dq; mc2.kcache = ns.kcache; mc2.vcache = ns.vcache;
        mc2.logits = h->logits; mc2.H = k().n_heads; mc2.L = k().max_decode_len; mc2.shared = shared; mc2.row_pos = row_pos();
        mc2.R = S.R; mc2.E = k().n_experts; mc2.fp8 = k().moe_fp8; mc2.eps = k().ln_eps;
        mc2.sync = h->chain_sync; mc2.host_abort = h->chain_host_abort;
        mc2.sel_trace = S.slot() ? nullptr : h->moe_trace; mc2.layer = l; mc2.n_layers = k().n_dec_layers;      // (no trace in a slot mode: its rows are at their own steps)
        mc2.trace_rows = h->moe_trace_rows; mc2.trace_steps = h->moe_trace_steps;
        mc2.stamp = next_stamp(h, PC_CHAIN, 256);
        return mc2;
    }
    // the MoE FFN of layer l as separate stages: router, expert FFN-in, expert FFN-out, combine
    MoeArgs moe_stage_args(int l, float* hcur) const {
        MoeArgs mo = h->moe;
        mo.h = hcur; mo.gain = W(l).ln3; mo.ssq = h->ssq; mo.ssq_stride = h->maxR;
        mo.router = W(l).router; mo.wi = W(l).wi; mo.wo = W(l).wo2; mo.row0 = S.row0; mo.R = S.R;
        mo.wi_q8 = W(l).wi_q8; mo.wo_q8 = W(l).wo_q8; mo.wi_s = W(l).wi_s; mo.wo_s = W(l).wo_s; mo.fp8 = k().moe_fp8;
        mo.sel_trace = S.slot() ? nullptr : h->moe_trace; mo.shared = shared; mo.layer = l; mo.n_layers = k().n_dec_layers;
        mo.trace_rows = h->moe_trace_rows; mo.trace_steps = h->moe_trace_steps;
        return mo;
    }
    // the per-step kernel (dec_step.hip): every layer's attention pair and GEMM chain
    StepArgs step_kernel_args() const {
        StepArgs sa{};
        sa.n_layers = k().n_dec_layers; sa.R = S.R; sa.T = h->T; sa.L = k().max_decode_len; sa.ssq_stride = h->maxR; sa.eps = k().ln_eps;
        sa.tiles_free = h->step_tiles_free ? 1 : 0;
        sa.q = h->dq; sa.attn = h->dattn; sa.opart = h->opart; sa.h = h->h_dec; sa.ssq = h->ssq; sa.dff = h->dff; sa.logits = h->logits;
        sa.bias = h->dec.bias_dist; sa.shared = shared; sa.row_pos = row_pos();
        sa.sync = h->step_sync; sa.pair_rows = h->pair_rows; sa.abort_word = h->chain_sync + CHAIN_ABORT_WORD; sa.host_abort = h->chain_host_abort;
        for (int j = 0; j < k().n_dec_layers; ++j) {
            const LayerW& J = W(j);
            const NextStage ns = next_stage(h, j);
            StepLayer& SL = sa.layer[j];
            SL.wo = J.wo; SL.wq_c = J.wq_c; SL.wo_c = J.wo_c; SL.wi = J.wi; SL.wo2 = J.wo2; SL.w3 = ns.w3;
            SL.ln2 = J.ln2; SL.ln3 = J.ln3; SL.gain3 = ns.gain3;
            SL.kself = h->kcache + layer_cache(j); SL.vself = h->vcache + layer_cache(j);
            SL.kcross = cross_kv(j, 0); SL.vcross = cross_kv(j, 1);
            SL.knext = ns.kcache; SL.vnext = ns.vcache;
            SL.N3 = ns.N3; SL.last = ns.last ? 1 : 0;
        }
        sa.stamp = next_stamp(h, PC_STEP, ((S.R + 15) / 16) * 128);
        return sa;
    }

    // The end of every step: the selection kernel picks the rows' next ids from the logits, advances the loop state and embeds the ids
    // (gathering layer 0's q / k / v where the shape says so).  A beam step: the groups' top-W continuations.
    int selection() const {
        if (S.W > 0) {
            BeamArgs b = beam_args(h, S.R, S.W, shared, S.slot());
            b.stamp = next_stamp(h, PC_ARGMAX, S.R / S.W);
            PLAUNCH(PC_ARGMAX, launch_beam_select(b, s));
            return YMT3_OK;
        }
        ArgmaxArgs g = argmax_base(h, S.R, S.slot());
        g.logits = h->logits; g.shared = shared; g.row0 = S.row0;
        qkv0_wire(h, S.qkv0, &g);
        if (S.solo) g.ticket = h->ticket;                // (row ranges of several chains would share groups)
        if (P.stepk) { g.zero_sync = h->step_sync; g.zero_lines = k().n_dec_layers * STEP_SYNC_LINES_PER_LAYER; }
        g.stamp = next_stamp(h, PC_ARGMAX, S.R);
        PLAUNCH(PC_ARGMAX, launch_argmax_embed(g, s));
        return YMT3_OK;
    }
    // The step kernel's regime (YMT3_STEP_KERNEL=1): layer 0's QKV projection unless the table provides it, every layer in one launch, selection.
    int step_kernel_regime() const {
        if (!S.qkv0) {
            const DecGemmArgs a = qkv_args(0, StepCarry{h->h_dec, nullptr, false, false});
            PLAUNCH(PC_QKV, launch_dec_gemm(DG_NORM_QKV_CACHE, a, s));
        }
        const StepArgs sa = step_kernel_args();
        PLAUNCH(PC_STEP, launch_dec_step(sa, s));
        return selection();
    }
    // A layer of the other regimes, part 1: its QKV projection -- unless the previous layer's merged tail did it, or (layer 0, no combine
    // ever pending there) the kernel that fed the rows has written q and this position's k / v from the table.
    int layer_projection(int l, StepCarry& y) const {
        if (!y.qkv_done && !(l == 0 && S.qkv0 && !y.pend)) {
            const DecGemmArgs a = qkv_args(l, y);
            PLAUNCH(PC_QKV, launch_dec_gemm(DG_NORM_QKV_CACHE, a, s));
        }
        y.qkv_done = false;
        if (y.pend) { y.hcur = other(y.hcur); y.pend = nullptr; }      // the projection has formed h + (y0 + y1) in the other buffer
        return YMT3_OK;
    }
    // Part 2, attention.  Self: through the ancestry table (beam), inside the pair, or on its own; then its O-projection unless folded.  Cross:
    // multi-channel, or per row -- after the separate query projection where that is not fused (YMT3_NO_FUSEQ=1) -- as the pair's second half or alone.
    int layer_attention(int l, const StepCarry& y) const {
        const int grid = S.R * k().n_heads;
        if (S.W > 0) {
            DecAttnArgs t = self_attn_args(l);
            const BeamAttn ba{h->beam.anc, h->beam.anc_rows, h->beam.anc_pitch, S.W};
            t.stamp = next_stamp(h, PC_SELF_ATTN, grid);
            PLAUNCH(PC_SELF_ATTN, launch_dec_attention_beam(t, ba, s));
        } else if (!P.pair_ok) {
            DecAttnArgs t = self_attn_args(l);
            t.stamp = next_stamp(h, PC_SELF_ATTN, grid);
            PLAUNCH(PC_SELF_ATTN, launch_dec_attention(true, t, s));
        }
        if (!P.fold) {
            const DecGemmArgs a = gemm_resid(PC_SELF_O, h->dattn, W(l).wo, h->inner, y.hcur);
            PLAUNCH(PC_SELF_O, launch_dec_gemm(DG_RESID, a, s));
        }
        if (P.mc) {
            const McCrossArgs mcx = mc_cross_args(l, y.hcur);
            PLAUNCH(PC_CROSS_ATTN, launch_mc_cross_attention(mcx, s));
            return YMT3_OK;
        }
        if (!h->fuse_q) {
            const DecGemmArgs a = gemm_norm(PC_CROSS_Q, y.hcur, W(l).ln2, W(l).wq_c, h->inner, h->dq);
            PLAUNCH(PC_CROSS_Q, launch_dec_gemm(DG_NORM_BF16, a, s));
        }
        DecAttnArgs t = cross_attn_args(l, y.hcur);
        if (P.pair_ok) {
            DecAttnArgs ts = self_attn_args(l);          // (the pair's two halves, built side by side: one stamp slot)
            ts.stamp = t.stamp = next_stamp(h, PC_ATTN_PAIR, grid);
            PLAUNCH(PC_ATTN_PAIR, launch_dec_attention_pair(ts, t, h->pair_rows, h->chain_sync + CHAIN_ABORT_WORD, h->chain_host_abort, s));
        } else {
            t.stamp = next_stamp(h, PC_CROSS_ATTN, grid);
            PLAUNCH(PC_CROSS_ATTN, launch_dec_attention(false, t, s));
        }
        return YMT3_OK;
    }
    // Part 3, the tail: cross O-projection, FFN and the next stage (next_stage) as one merged launch -- GEMM chain or MoE chain -- or the cross
    // O-projection and the FFN as separate launches, which leave the next stage to the next layer_projection / the lm_head.
    int layer_tail(int l, StepCarry& y) const {
        if (P.chain || P.moe_chain) {
            const NextStage ns = next_stage(h, l);
            if (P.chain) {
                const ChainArgs cg = chain_args(l, y.hcur, ns);
                PLAUNCH(PC_CHAIN, launch_dec_chain(cg, s));
            } else {
                const MoeChainArgs mc2 = moe_chain_args(l, y.hcur, ns);
                PLAUNCH(PC_CHAIN, launch_moe_chain(mc2, s));
                if (!ns.last) y.hcur = mc2.h_out;
            }
            (ns.last ? y.lm_done : y.qkv_done) = true;
            return YMT3_OK;
        }
        {
            const DecGemmArgs a = gemm_resid(PC_CROSS_O, h->dattn, W(l).wo_c, h->inner, y.hcur, P.fold ? h->opart : nullptr);
            PLAUNCH(PC_CROSS_O, launch_dec_gemm(DG_RESID, a, s));
        }
        if (k().dec_ffn == YMT3_FFN_MOE) {
            const MoeArgs mo = moe_stage_args(l, y.hcur);
            { ProfScope _ps(h, PC_FFN_WI, s); LAUNCH(launch_moe_stage(0, mo, s)); LAUNCH(launch_moe_stage(1, mo, s)); }
            { ProfScope _ps(h, PC_FFN_WO, s); LAUNCH(launch_moe_stage(2, mo, s)); if (!P.fold_combine) LAUNCH(launch_moe_stage(3, mo, s)); }
            if (P.fold_combine) y.pend = mo.y;
            return YMT3_OK;
        }
        {
            const DecGemmArgs a = gemm_norm(PC_FFN_WI, y.hcur, W(l).ln3, W(l).wi, k().d_ff, h->dff);
            PLAUNCH(PC_FFN_WI, launch_dec_gemm(DG_NORM_BF16_RELU, a, s));
        }
        const DecGemmArgs a = gemm_resid(PC_FFN_WO, h->dff, W(l).wo2, k().d_ff, y.hcur);
        PLAUNCH(PC_FFN_WO, launch_dec_gemm(DG_RESID, a, s));
        return YMT3_OK;
    }
    // per layer QKV projection, attention, tail; then lm_head and selection
    int run() const {
        if (P.stepk) return step_kernel_regime();
        StepCarry y{h->h_dec, nullptr, false, false};
        for (int l = 0; l < k().n_dec_layers; ++l) {
            int rc = layer_projection(l, y);
            if (!rc) rc = layer_attention(l, y);
            if (!rc) rc = layer_tail(l, y);
            if (rc) return rc;
        }
        if (!y.lm_done) {
            const DecGemmArgs a = lm_head_args(y);
            PLAUNCH(PC_LM_HEAD, launch_dec_gemm(DG_NORM_LOGITS, a, s));
        }
        return selection();
    }
};

// One decoder step of shape S, every kernel reading the position from the chain's DecodeShared (or row_pos).  *merged is raised when
// the step holds merged kernels.
static int launch_step(ymt3_handle h, const StepShape& S, DecodeShared* shared, hipStream_t s, bool* merged = nullptr) {
    const Step step{h, S, plan_step(h, S), shared, s};
    h->stamp_n = 0;
    if (merged && step.P.merged()) *merged = true;
    return step.run();
}

// The cached graph of G consecutive steps of shape S, filed under step_key(S, G) and captured on first use.  A capture that fails leaves
// nothing behind: the capture is ended, what it recorded destroyed and the cache left without the entry.  *merged is raised when the
// graph holds merged kernels.
static int step_graph(ymt3_handle h, const StepShape& S, DecodeShared* shared, int G, hipGraphExec_t* out, bool* merged = nullptr) {
    const StepKey key = step_key(S, G);
    auto it = h->step_graphs.find(key);
    if (it == h->step_graphs.end()) {
        StepGraph sg;
        HIP_TRY(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
        int rc = 0;
        for (int i = 0; i < G && !rc; ++i) rc = launch_step(h, S, shared, h->cap_stream, &sg.merged);
        hipError_t e = hipStreamEndCapture(h->cap_stream, &sg.graph);
        if (!rc && e != hipSuccess) { ymt3_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); rc = YMT3_ERR_HIP; }
        if (!rc && (e = hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0)) != hipSuccess) {
            ymt3_set_error("instantiating the step graph: %s", hipGetErrorString(e));
            rc = YMT3_ERR_HIP;
        }
        if (rc) {
            if (sg.graph) (void)hipGraphDestroy(sg.graph);
            return rc;
        }
        it = h->step_graphs.emplace(key, sg).first;
    }
    *out = it->second.exec;
    if (merged && it->second.merged) *merged = true;
    return YMT3_OK;
}

// a6: the cross-attention K/V of every decoder layer in one GEMM over `n_seg` encoded segments, stored as per-(segment, head) slabs from
// segment `first` on in a call whose layers each hold `call_segs` segments.  A lock-step call: (enc, B); a slot admission: (enc, 1, slot, slots).
static int launch_cross_kv(ymt3_handle h, const bf16_t* enc, int n_seg, int first, int call_segs, hipStream_t s) {
    const ymt3_config& k = h->cfg;
    const int d = k.d_model;
    GemmArgs g{enc, h->wkv_all, h->ckv + (size_t)first * k.n_heads * h->T * 64, nullptr, n_seg * h->T, k.n_dec_layers * 2 * h->inner, d, d, d, 0, h->T, k.n_heads, call_segs};
    LAUNCH(launch_gemm(EPI_KV_HEADMAJOR, g, s));
    return YMT3_OK;
}
static int launch_cross_kv(ymt3_handle h, const bf16_t* enc, int B, hipStream_t s) { return launch_cross_kv(h, enc, B, 0, B, s); }

// before a greedy call's init kernel: the step kernel's counter lines start at zero (each step's selection kernel zeroes them again)
static int zero_step_sync(ymt3_handle h, hipStream_t s) {
    if (h->step_kernel && h->step_sync) HIP_TRY(hipMemsetAsync(h->step_sync, 0, (size_t)STEP_SYNC_LINES * CHAIN_LINE * sizeof(unsigned), s));
    return YMT3_OK;
}

// n_total steps on `s`: whole G-step graphs (`many`, or null: none), then the tail step by step.  G consecutive steps are ONE replayed
// graph (every kernel reads the position from device memory, so a graph of G steps is the step's kernels G times): the boundary between
// two graph launches costs ~7 us of stream time that a kernel boundary inside a graph does not (eager launches ran 2.9 % faster than
// one-step graphs, profiles/r02_graph_steps.txt)
static int replay(hipGraphExec_t many, int G, hipGraphExec_t one, int n_total, hipStream_t s) {
    int t = 0;
    if (many)
        for (; t + G <= n_total; t += G) HIP_TRY(hipGraphLaunch(many, s));
    for (; t < n_total; ++t) HIP_TRY(hipGraphLaunch(one, s));
    return YMT3_OK;
}

// opt-in (ymt3_set_early_stop): every `interval` steps the host reads how many rows (beam call: groups) are still decoding and
// stops launching once none is; the rest of every row is PAD by the EOS fill rule (a beam call's finished slots are complete by
// then).  This path synchronises the stream (the only one that does).  Only emitted steps count: the prompt's steps go first, then
// the host checks every `interval` emitted steps.  *emitted: the emitted steps launched.
static int replay_early_stop(ymt3_handle h, hipGraphExec_t one, int n_prompt, int n_steps, hipStream_t s, int* emitted) {
    int rc = replay(nullptr, 1, one, n_prompt, s);
    if (rc) return rc;
    int t = 0;
    while (t < n_steps) {
        const int chunk = std::min(h->early_stop_interval, n_steps - t);
        rc = replay(nullptr, 1, one, chunk, s);
        if (rc) return rc;
        t += chunk;
        if (t >= n_steps) break;
        HIP_TRY(hipMemcpyAsync(h->host_flag, &h->shared->n_unfinished, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (*h->host_flag == 0) break;
    }
    h->last_steps = n_prompt + t;
    *emitted = t;
    return YMT3_OK;
}

// The step range of a decode call: n_prompt fed steps, then n_steps emitted ones, from position step0 (ymt3_debug_decode_start, else 0).
static int check_steps(ymt3_handle h, int n_steps, const int32_t* prompt, int n_prompt, int step0) {
    if (n_prompt < 0) FAIL(YMT3_ERR_ARG, "n_prompt=%d < 0", n_prompt);
    if (n_prompt > 0 && !prompt) FAIL(YMT3_ERR_ARG, "n_prompt=%d with a null prompt", n_prompt);
    if (n_prompt > 0 && step0 > 0) FAIL(YMT3_ERR_ARG, "ymt3_debug_decode_start does not combine with a prompt (n_prompt=%d)", n_prompt);
    if (n_steps <= 0 || step0 + n_prompt + n_steps > h->cfg.max_decode_len)
        FAIL(YMT3_ERR_ARG, "n_steps=%d outside [1, max_decode_len - n_prompt=%d]", n_steps, h->cfg.max_decode_len - step0 - n_prompt);
    return YMT3_OK;
}

static int decode_run(ymt3_handle h, const bf16_t* enc, int B, int n_steps, const int32_t* prompt, int n_prompt, int32_t* tokens,
                      float* scores, const int32_t* forced, float* logits_out, const ConstraintView& cv, hipStream_t s, int prof_stride,
                      int step0);

// A call launches n_prompt + n_steps steps: the first n_prompt feed prompt[r][t] and emit nothing (argmax_embed_kernel), the rest
// emit tokens 0 .. n_steps-1.  n_prompt = 0 is the plain decode.  `scores` (or null): [R][n_steps] f32, the log-probability of the id
// fed after each emitted token (include/ymt3.h, token scores), written by the same kernels as the tokens.  `cv`: the call's token
// automaton (include/ymt3.h, constraints), seeded by decode_init -- so an abort re-run starts from the same states.
static int decode_impl(ymt3_handle h, const bf16_t* enc, int B, int n_steps, const int32_t* prompt, int n_prompt, int32_t* tokens,
                       float* scores, const int32_t* forced, float* logits_out, const ConstraintView& cv, hipStream_t s,
                       int prof_stride = 0) {
    const int step0 = h->prof_step0;          // one shot (debug hook): consumed by this call whatever its outcome
    h->prof_step0 = 0;
    int rc = check_steps(h, n_steps, prompt, n_prompt, step0);
    if (rc) return rc;
    return decode_run(h, enc, B, n_steps, prompt, n_prompt, tokens, scores, forced, logits_out, cv, s, prof_stride, step0);
}

static int decode_run(ymt3_handle h, const bf16_t* enc, int B, int n_steps, const int32_t* prompt, int n_prompt, int32_t* tokens,
                      float* scores, const int32_t* forced, float* logits_out, const ConstraintView& cv, hipStream_t s, int prof_stride,
                      int step0) {
    const ymt3_config& k = h->cfg;
    bool merged = false;                      // some step of this call ran merged kernels
    const int n_total = n_prompt + n_steps;   // steps launched
    const int R = B * k.n_channels;
    const bool profiled = prof_stride > 0;
    int rc = launch_cross_kv(h, enc, B, s);
    if (rc) return rc;

    ArgmaxArgs a = argmax_base(h, R, false);
    // chains: contiguous, near-equal row ranges
    int n_chains = (!h->use_graph || profiled || k.dec_ffn == YMT3_FFN_MOE) ? 1 : h->n_chains;   // MoE pair tables are per handle
    // the early-stop loop (replay_early_stop) runs one chain; with forced tokens the trajectory is fixed, so it is not used
    const bool early = h->early_stop_interval > 0 && k.eos_id >= 0 && !forced;
    if (h->auto_chains && n_chains == 1 && h->use_graph && !profiled && k.dec_ffn != YMT3_FFN_MOE && k.n_channels == 1 && R >= 168 && R <= 256 &&
        !early) {
        // (see auto_chains) ... and only where the ids cannot depend on the choice: the whole batch as one chain and both halves take
        // kernels that sum in the same order
        const StepShape two = step_shape(h, SM_LOCKSTEP, B, 0, R, 2, false);
        const StepPlan whole = plan_step(h, step_shape(h, SM_LOCKSTEP, B, 0, R, 1, false));
        if (bits_agree(whole, plan_step(h, chain_shape(two, 0))) && bits_agree(whole, plan_step(h, chain_shape(two, 1)))) n_chains = 2;
    }
    if (n_chains > R) n_chains = R;
    const StepShape S = step_shape(h, SM_LOCKSTEP, B, 0, R, n_chains, profiled);
    h->last_chains = n_chains;
    h->last_qkv0 = S.qkv0;
    qkv0_wire(h, S.qkv0, &a);
    rc = zero_step_sync(h, s);
    if (rc) return rc;
    LAUNCH(launch_decode_init(a, n_chains, n_steps, step0, tokens, forced, logits_out, prompt, n_prompt, scores, cv, s));
    h->last_steps = n_total;

    if (!h->use_graph || profiled) {
        // sampled steps (mid-stride: unbiased mean position) bracket every launch; the stride-1 unsampled steps that
        // follow each of them are bracketed as ONE span, which gives the true step time the per-launch brackets are
        // calibrated against (an event pair adds stream time of its own)
        for (int t = 0; t < n_total; ++t) {
            const bool sampled = prof_stride > 0 && (t % prof_stride) == prof_stride / 2;
            const bool span_begin = prof_stride > 1 && (t % prof_stride) == prof_stride / 2 + 1 && t + prof_stride - 1 <= n_total;
            const bool span_end = prof_stride > 1 && t >= prof_stride && (t % prof_stride) == prof_stride / 2 && !h->prof_ev.empty() && h->prof_span_open;
            if (span_end) { (void)hipEventRecord(h->prof_ev[h->prof_span_idx], s); h->prof_span_open = false; }
            if (span_begin) {
                hipEvent_t ea, eb;
                if (hipEventCreate(&ea) == hipSuccess && hipEventCreate(&eb) == hipSuccess) {
                    h->prof_ev.push_back(ea); h->prof_ev.push_back(eb); h->prof_cls.push_back(PC_SPAN);
                    h->prof_span_idx = h->prof_ev.size() - 1; h->prof_span_open = true;
                    (void)hipEventRecord(ea, s);
                }
            }
            h->prof_on = sampled;
            rc = launch_step(h, S, h->shared, s, &merged);
            h->prof_on = false;
            if (rc) return rc;
        }
        if (h->prof_span_open) {            // a span the loop never closed: drop it (its end event was never recorded)
            (void)hipEventRecord(h->prof_ev[h->prof_span_idx], s);
            h->prof_cls[h->prof_span_idx / 2] = -1;
            h->prof_span_open = false;
        }
    } else {
        // every chain's one-step graph, and its G-step graph where the call has G steps to replay at once
        const int G = h->graph_steps;
        const bool stop_early = early && n_chains == 1;
        hipGraphExec_t one[8], many[8] = {};
        auto chain_graphs = [&](int steps, hipGraphExec_t* out) -> int {
            for (int c = 0; c < n_chains; ++c) {
                int rcg = step_graph(h, chain_shape(S, c), h->shared + c, steps, &out[c], &merged);
                if (rcg) return rcg;
            }
            return YMT3_OK;
        };
        rc = chain_graphs(1, one);
        if (!rc && !stop_early && G > 1 && n_total >= G) rc = chain_graphs(G, many);
        if (rc) return rc;
        if (stop_early) {
            int t = 0;
            rc = replay_early_stop(h, one[0], n_prompt, n_steps, s, &t);
            if (rc) return rc;
            LAUNCH(launch_pad_tail(tokens, scores, 0, R, n_steps, t, k.pad_id, s));
        } else if (n_chains == 1) {
            rc = replay(many[0], G, one[0], n_total, s);
            if (rc) return rc;
        } else {
            // fork: every chain stream waits for the cross-KV GEMM + init on the caller's stream
            HIP_TRY(hipEventRecord(h->fork_ev, s));
            for (int c = 0; c < n_chains; ++c) HIP_TRY(hipStreamWaitEvent(h->chain_stream[c], h->fork_ev, 0));
            // one host thread per chain: a hipGraphLaunch of the ~44-node step costs the host 60-150 us, so ONE thread
            // feeding n chains is host-bound as soon as a chain's step is shorter than n launches
            std::atomic<int> bad{0};
            std::vector<std::thread> th;
            for (int c = 1; c < n_chains; ++c)
                th.emplace_back([&, c] {
                    if (hipSetDevice(h->device) != hipSuccess || replay(many[c], G, one[c], n_total, h->chain_stream[c])) bad = 1;
                });
            if (replay(many[0], G, one[0], n_total, h->chain_stream[0])) bad = 1;
            for (auto& t : th) t.join();
            if (bad) FAIL(YMT3_ERR_HIP, "hipGraphLaunch failed on a decode chain: %s", hipGetErrorString(hipGetLastError()));
            // join: the caller's stream continues only after every chain has emitted its last token
            for (int c = 0; c < n_chains; ++c) {
                HIP_TRY(hipEventRecord(h->join_ev[c], h->chain_stream[c]));
                HIP_TRY(hipStreamWaitEvent(s, h->join_ev[c], 0));
            }
        }
    }
    if (merged) {
        // a merged launch that gave up on a stage (dec_chain.hip, dec_attn_pair_kernel) must not leave plausible ids behind
        LAUNCH(launch_chain_poison(h->chain_sync, tokens, scores, (long long)R * n_steps, s));
        HIP_TRY(hipGetLastError());
        if (h->abort_recovery && prof_stride == 0) {
            // Recovery (ymt3_set_abort_recovery, default on): wait for the call's own work and look at the abort word.  Raised -- a
            // stage waited > 1 s for workgroups that were not resident: another kernel held CUs -- the call is run again through the
            // separate launches (fresh launches in this process, the same arithmetic bit for bit) and the handle stays on them.
            HIP_TRY(hipStreamSynchronize(s));
            if (h->forced_abort && h->chain_host_abort) *h->chain_host_abort = 1u;      // debug hook: as a kernel would have during the call
            if (h->chain_host_abort && *static_cast<volatile unsigned*>(h->chain_host_abort)) {
                rc = merged_fallback(h);
                if (rc) return rc;
                return decode_run(h, enc, B, n_steps, prompt, n_prompt, tokens, scores, forced, logits_out, cv, s, prof_stride, step0);
            }
        } else if (h->forced_abort && h->chain_host_abort) {
            *h->chain_host_abort = 1u;            // asynchronous mode: the next call on the handle finds the word (check_call)
            h->forced_abort = false;
        }
    }
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_decode_constrained(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                       int32_t* tokens_dev, float* scores_dev, const int32_t* forced_dev, float* logits_dev,
                                       ymt3_constraint constraint, const int32_t* start_state_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    ConstraintView cv{};
    rc = constraint_view(h, constraint, start_state_dev, &cv);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!enc_dev || !tokens_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    return decode_impl(h, static_cast<const bf16_t*>(enc_dev), B, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev, forced_dev,
                       logits_dev, cv, (hipStream_t)stream);
}

extern "C" int ymt3_decode_scored(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                  int32_t* tokens_dev, float* scores_dev, const int32_t* forced_dev, float* logits_dev, void* stream) {
    return ymt3_decode_constrained(h, enc_dev, B, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev, forced_dev, logits_dev, nullptr,
                                   nullptr, stream);
}

extern "C" int ymt3_decode_prompted(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                    int32_t* tokens_dev, const int32_t* forced_dev, float* logits_dev, void* stream) {
    return ymt3_decode_scored(h, enc_dev, B, n_steps, prompt_dev, n_prompt, tokens_dev, nullptr, forced_dev, logits_dev, stream);
}

extern "C" int ymt3_decode_greedy(ymt3_handle h, const void* enc_dev, int B, int n_steps, int32_t* tokens_dev,
                                  const int32_t* forced_dev, float* logits_dev, void* stream) {
    return ymt3_decode_prompted(h, enc_dev, B, n_steps, nullptr, 0, tokens_dev, forced_dev, logits_dev, stream);
}

extern "C" int ymt3_transcribe_segments_constrained(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev,
                                                    int n_prompt, int32_t* tokens_dev, float* scores_dev, ymt3_constraint constraint,
                                                    const int32_t* start_state_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    ConstraintView cv{};
    rc = constraint_view(h, constraint, start_state_dev, &cv);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!audio_dev || !tokens_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    rc = check_steps(h, n_steps, prompt_dev, n_prompt, 0);      // before any work is queued (decode_impl checks again, with the debug start)
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(launch_logmel(h->fe, audio_dev, h->mel, B, s));
    rc = encode_impl(h, h->mel, B, h->enc_out, s);
    if (rc) return rc;
    return decode_impl(h, h->enc_out, B, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev, nullptr, nullptr, cv, s);
}

extern "C" int ymt3_transcribe_segments_scored(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev,
                                               int n_prompt, int32_t* tokens_dev, float* scores_dev, void* stream) {
    return ymt3_transcribe_segments_constrained(h, audio_dev, B, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev, nullptr, nullptr,
                                                stream);
}

extern "C" int ymt3_transcribe_segments_prompted(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev,
                                                 int n_prompt, int32_t* tokens_dev, void* stream) {
    return ymt3_transcribe_segments_scored(h, audio_dev, B, n_steps, prompt_dev, n_prompt, tokens_dev, nullptr, stream);
}

extern "C" int ymt3_transcribe_segments(ymt3_handle h, const float* audio_dev, int B, int n_steps, int32_t* tokens_dev,
                                        void* stream) {
    return ymt3_transcribe_segments_prompted(h, audio_dev, B, n_steps, nullptr, 0, tokens_dev, stream);
}

// ---------------------------------------------------------------- sequence scoring (include/ymt3.h; kernels: dec_seq.hip)
// The teacher-forced pass: with the ids given nothing is sequential, so every position of every decoder row goes through the layers
// at once -- launch_gemm / launch_rmsnorm over rows x positions, the causal and the cross attention and the scoring lm_head of
// dec_seq.hip.  Activations live in the encoder's buffers (idle once the cross-K/V GEMM has read the encoder output), act_rows rows of
// them: the pass runs in chunks of floor(act_rows / (P + n_steps)) whole decoder rows, queued back to back.  It writes neither the
// self-attention cache nor the loop state of the step kernels.
static int score_check(ymt3_handle h, int n_steps, const int32_t* prompt, int n_prompt, const int32_t* tokens, const float* scores) {
    const ymt3_config& k = h->cfg;
    if (k.dec_ffn == YMT3_FFN_MOE)
        FAIL(YMT3_ERR_UNSUPPORTED, "sequence scoring does not run the MoE decoder FFN (dec_ffn = %d): the full-sequence pass has no grouped expert GEMMs", k.dec_ffn);
    if (n_prompt < 0) FAIL(YMT3_ERR_ARG, "n_prompt=%d < 0", n_prompt);
    if (n_prompt > 0 && !prompt) FAIL(YMT3_ERR_ARG, "n_prompt=%d with a null prompt", n_prompt);
    if (n_steps <= 0 || n_prompt + n_steps > k.max_decode_len)
        FAIL(YMT3_ERR_ARG, "n_steps=%d outside [1, max_decode_len - n_prompt=%d]", n_steps, k.max_decode_len - n_prompt);
    if (!tokens || !scores) FAIL(YMT3_ERR_ARG, "null tokens or scores buffer");
    return YMT3_OK;
}

static int score_impl(ymt3_handle h, const bf16_t* enc, int B, int n_steps, const int32_t* prompt, int n_prompt, const int32_t* tokens,
                      const int32_t* lengths, float* scores, float* logits_out, hipStream_t s) {
    const ymt3_config& k = h->cfg;
    const int d = k.d_model, inner = h->inner, H = k.n_heads, T = h->T, R = B * k.n_channels, L = n_prompt + n_steps;
    if (int rc = launch_cross_kv(h, enc, B, s)) return rc;      // as the decode calls
    SeqEmbedArgs e{};
    e.h = h->h_enc; e.prompt = prompt; e.tokens = tokens; e.L = L; e.n_prompt = n_prompt; e.n_steps = n_steps; e.V = k.vocab; e.d = d;
    e.n_channels = k.n_channels; e.pad_id = k.pad_id;
    e.embed = h->dec.embed; e.chan_embed = h->dec.chan_embed;
    const size_t slab = (size_t)B * H * T * 64;                    // one layer's K (or V) slabs of this call
    // >= 1: act_rows >= max_decode_len >= L; at most 65535 rows, the attention grid's z extent
    const int rows_per_chunk = (int)std::min<size_t>(std::min<size_t>(h->act_rows / (size_t)L, (size_t)R), 65535);
    for (int row0 = 0; row0 < R; row0 += rows_per_chunk) {
        const int nr = std::min(rows_per_chunk, R - row0), M = nr * L;
        e.row0 = row0; e.n_rows = nr;
        LAUNCH(launch_seq_embed(e, s));
        for (int l = 0; l < k.n_dec_layers; ++l) {
            const LayerW& W = h->dec.layer[(size_t)l];
            LAUNCH(launch_rmsnorm(h->h_enc, W.ln1, h->xn, M, d, k.ln_eps, s));
            { GemmArgs q{h->xn, W.wqkv, h->qkv, nullptr, M, 3 * inner, d, d, d, 3 * inner, 0, 0, 0}; LAUNCH(launch_gemm(EPI_BF16, q, s)); }
            SeqAttnDecArgs sa{};
            sa.q = h->qkv; sa.k = h->qkv + inner; sa.v = h->qkv + 2 * inner; sa.out = h->attn; sa.bias = h->dec.bias_dist;
            sa.q_seq = sa.kv_seq = (long long)L * 3 * inner; sa.o_seq = (long long)L * inner;
            sa.ldq = sa.ldkv = 3 * inner; sa.ldo = inner; sa.kv_head = 64;
            sa.row0 = 0; sa.n_rows = nr; sa.L = L; sa.n_keys = L; sa.rows_per_kv = 1; sa.H = H; sa.bias_stride = k.max_decode_len;
            LAUNCH(launch_dec_seq_attention(true, sa, s));
            { GemmArgs q{h->attn, W.wo, h->h_enc, nullptr, M, d, inner, inner, inner, d, 0, 0, 0}; LAUNCH(launch_gemm(EPI_RESID, q, s)); }
            LAUNCH(launch_rmsnorm(h->h_enc, W.ln2, h->xn, M, d, k.ln_eps, s));
            { GemmArgs q{h->xn, W.wq_c, h->qkv, nullptr, M, inner, d, d, d, inner, 0, 0, 0}; LAUNCH(launch_gemm(EPI_BF16, q, s)); }
            SeqAttnDecArgs ca{};
            ca.q = h->qkv; ca.k = h->ckv + (size_t)(2 * l) * slab; ca.v = h->ckv + (size_t)(2 * l + 1) * slab; ca.out = h->attn;
            ca.q_seq = ca.o_seq = (long long)L * inner; ca.kv_seq = (long long)H * T * 64;
            ca.ldq = ca.ldo = inner; ca.ldkv = 64; ca.kv_head = T * 64;
            ca.row0 = row0; ca.n_rows = nr; ca.L = L; ca.n_keys = T; ca.rows_per_kv = k.n_channels; ca.H = H;
            LAUNCH(launch_dec_seq_attention(false, ca, s));
            { GemmArgs q{h->attn, W.wo_c, h->h_enc, nullptr, M, d, inner, inner, inner, d, 0, 0, 0}; LAUNCH(launch_gemm(EPI_RESID, q, s)); }
            LAUNCH(launch_rmsnorm(h->h_enc, W.ln3, h->xn, M, d, k.ln_eps, s));
            { GemmArgs q{h->xn, W.wi, h->ff, nullptr, M, k.d_ff, d, d, d, k.d_ff, 0, 0, 0}; LAUNCH(launch_gemm(EPI_BF16_RELU, q, s)); }
            { GemmArgs q{h->ff, W.wo2, h->h_enc, nullptr, M, d, k.d_ff, k.d_ff, k.d_ff, d, 0, 0, 0}; LAUNCH(launch_gemm(EPI_RESID, q, s)); }
        }
        LAUNCH(launch_rmsnorm(h->h_enc, h->dec.ln_f, h->xn, M, d, k.ln_eps, s));
        SeqLmHeadArgs lm{};
        lm.xn = h->xn; lm.W = h->dec.lm_head; lm.tokens = tokens; lm.lengths = lengths; lm.scores = scores; lm.logits = logits_out;
        lm.M = M; lm.L = L; lm.n_prompt = n_prompt; lm.n_steps = n_steps; lm.V = k.vocab; lm.d = d; lm.row0 = row0;
        LAUNCH(launch_seq_lm_head_score(lm, s));
    }
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_score_tokens(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                 const int32_t* tokens_dev, const int32_t* lengths_dev, float* scores_dev, float* logits_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    rc = score_check(h, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!enc_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    return score_impl(h, static_cast<const bf16_t*>(enc_dev), B, n_steps, prompt_dev, n_prompt, tokens_dev, lengths_dev, scores_dev, logits_dev,
                      (hipStream_t)stream);
}

extern "C" int ymt3_transcribe_segments_score(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                              const int32_t* tokens_dev, const int32_t* lengths_dev, float* scores_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    rc = score_check(h, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev);      // before any work is queued
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!audio_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(launch_logmel(h->fe, audio_dev, h->mel, B, s));
    rc = encode_impl(h, h->mel, B, h->enc_out, s);
    if (rc) return rc;
    return score_impl(h, h->enc_out, B, n_steps, prompt_dev, n_prompt, tokens_dev, lengths_dev, scores_dev, nullptr, s);
}

// ---------------------------------------------------------------- beam search (include/ymt3.h)
static int beam_check(ymt3_handle h, int B, int n_steps, const int32_t* prompt, int n_prompt, const ymt3_beam_params* p, const int32_t* tokens) {
    const ymt3_config& k = h->cfg;
    if (!p) FAIL(YMT3_ERR_ARG, "null beam parameters");
    if (p->num_beams < 1 || p->num_beams > BEAM_MAX) FAIL(YMT3_ERR_ARG, "num_beams=%d outside [1, %d]", p->num_beams, BEAM_MAX);
    if (p->num_return < 1 || p->num_return > p->num_beams) FAIL(YMT3_ERR_ARG, "num_return=%d outside [1, num_beams=%d]", p->num_return, p->num_beams);
    if (!(p->length_penalty >= 0.f) || p->length_penalty > 3.0e38f) FAIL(YMT3_ERR_ARG, "length_penalty=%g must be finite and >= 0", (double)p->length_penalty);
    if ((long long)B * k.n_channels * p->num_beams > h->maxR)
        FAIL(YMT3_ERR_ARG, "B * n_channels * num_beams = %lld rows exceed the max_batch * n_channels = %d rows the handle was created for",
             (long long)B * k.n_channels * p->num_beams, h->maxR);
    if (k.n_channels * p->num_beams > 255) FAIL(YMT3_ERR_ARG, "n_channels * num_beams = %d exceeds 255 rows per segment", k.n_channels * p->num_beams);
    if (h->beam.anc_pitch > 48 * 1024) FAIL(YMT3_ERR_ARG, "beam search needs max_decode_len < %d (the staged ancestry table)", 48 * 1024 - 16);
    if (int rc = check_steps(h, n_steps, prompt, n_prompt, 0)) return rc;
    if (h->prof_step0) FAIL(YMT3_ERR_ARG, "ymt3_debug_decode_start is pending: it does not combine with beams");
    if (B > 0 && !tokens) FAIL(YMT3_ERR_ARG, "null buffer");
    return 0;
}

// One chain, lock-step, the separate launches (a step shape with W set); the step graphs are cached under a mode of their own (SM_BEAM: B, W).
static int decode_beam_impl(ymt3_handle h, const bf16_t* enc, int B, int n_steps, const int32_t* prompt, int n_prompt, const ymt3_beam_params* p,
                            int32_t* tokens, float* seq_scores, float* token_scores, const ConstraintView& cv, hipStream_t s) {
    const ymt3_config& k = h->cfg;
    const int W = p->num_beams, R = B * k.n_channels * W, n_total = n_prompt + n_steps;
    int rc = launch_cross_kv(h, enc, B, s);
    if (rc) return rc;
    const StepShape S = step_shape(h, SM_BEAM, B, W, R, 1, false);
    const BeamArgs b = beam_args(h, R, W, h->shared, false);
    BeamShared params = h->beam_trace;
    params.alpha = p->length_penalty; params.tokens_out = tokens; params.seq_out = seq_scores; params.tok_out = token_scores;
    h->last_chains = 1;
    h->last_qkv0 = S.qkv0;
    LAUNCH(launch_beam_init(b, n_steps, prompt, n_prompt, cv, params, s));
    h->last_steps = n_total;
    const int G = h->graph_steps;
    hipGraphExec_t many = nullptr, one = nullptr;
    if (!h->use_graph) {
        for (int t = 0; t < n_total && !rc; ++t) rc = launch_step(h, S, h->shared, s);
    } else if (h->early_stop_interval > 0) {
        int emitted = 0;
        rc = step_graph(h, S, h->shared, 1, &one);
        if (!rc) rc = replay_early_stop(h, one, n_prompt, n_steps, s, &emitted);
    } else {
        // (the one-step graph is captured only by a call with a tail)
        if (G > 1 && n_total >= G) rc = step_graph(h, S, h->shared, G, &many);
        if (!rc && (!many || n_total % G)) rc = step_graph(h, S, h->shared, 1, &one);
        if (!rc) rc = replay(many, G, one, n_total, s);
    }
    if (rc) return rc;
    LAUNCH(launch_beam_finalize(b, p->num_return, s));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_decode_beam(ymt3_handle h, const void* enc_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                const ymt3_beam_params* params, int32_t* tokens_dev, float* seq_scores_dev, float* token_scores_dev,
                                ymt3_constraint constraint, const int32_t* start_state_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    ConstraintView cv{};
    rc = constraint_view(h, constraint, start_state_dev, &cv);
    if (rc) return rc;
    rc = beam_check(h, B, n_steps, prompt_dev, n_prompt, params, tokens_dev);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!enc_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    return decode_beam_impl(h, static_cast<const bf16_t*>(enc_dev), B, n_steps, prompt_dev, n_prompt, params, tokens_dev, seq_scores_dev,
                            token_scores_dev, cv, (hipStream_t)stream);
}

extern "C" int ymt3_transcribe_segments_beam(ymt3_handle h, const float* audio_dev, int B, int n_steps, const int32_t* prompt_dev, int n_prompt,
                                             const ymt3_beam_params* params, int32_t* tokens_dev, float* seq_scores_dev,
                                             float* token_scores_dev, ymt3_constraint constraint, const int32_t* start_state_dev, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    ConstraintView cv{};
    rc = constraint_view(h, constraint, start_state_dev, &cv);
    if (rc) return rc;
    rc = beam_check(h, B, n_steps, prompt_dev, n_prompt, params, tokens_dev);
    if (rc) return rc;
    if (B == 0) return YMT3_OK;
    if (!audio_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(launch_logmel(h->fe, audio_dev, h->mel, B, s));
    rc = encode_impl(h, h->mel, B, h->enc_out, s);
    if (rc) return rc;
    return decode_beam_impl(h, h->enc_out, B, n_steps, prompt_dev, n_prompt, params, tokens_dev, seq_scores_dev, token_scores_dev, cv, s);
}

extern "C" int ymt3_debug_beam_trace(ymt3_handle h, int32_t* trace_dev, float* run_dev, float* logits_dev, int n_steps, int n_groups) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!h->debug_hooks) FAIL(YMT3_ERR_UNSUPPORTED, "debug hooks are accepted only by a handle created with YMT3_DEBUG_HOOKS=1 in the environment");
    if (trace_dev && (n_steps <= 0 || n_groups <= 0)) FAIL(YMT3_ERR_ARG, "n_steps=%d n_groups=%d", n_steps, n_groups);
    if (!trace_dev && (run_dev || logits_dev)) FAIL(YMT3_ERR_ARG, "run / logits traces need the (parent, token) trace");
    // (the kernels read these from the device-resident parameters every call writes: no cached graph holds them)
    h->beam_trace = BeamShared{};
    h->beam_trace.trace = trace_dev;
    h->beam_trace.trace_run = trace_dev ? run_dev : nullptr;
    h->beam_trace.trace_logits = trace_dev ? logits_dev : nullptr;
    h->beam_trace.trace_steps = trace_dev ? n_steps : 0;
    h->beam_trace.trace_groups = trace_dev ? n_groups : 0;
    return YMT3_OK;
}

// The queue loop of the stream calls (ymt3_transcribe_stream*, ymt3_transcribe_stream_beam).  `slots` decoder slots of `rows` rows each are
// kept busy from the queue of segments: a round is `interval` steps of all slots (one replayed graph, cached under `key`), then the host
// reads the per-row `finished` flags, retires the segments whose rows have all stopped and admits the next pending ones into the freed
// slots: log-mel + encoder batched over the admissions, cross-K/V written into each slot's slabs, then start(slot, segment).
// retire(slot) launches whatever leaves the slot's results in the caller's buffers.  `S`: the shape of the queue's steps (a slot mode, S.B
// slots, S.R = slots * rows rows); the caller has launched its init kernel.  watch_abort: the steps may hold merged kernels; restart() runs
// when one gave up.
template <class Start, class Retire, class Restart>
static int run_slot_queue(ymt3_handle h, const float* audio_dev, int n_segments, const StepShape& S, int rows, int interval, int n_total,
                          bool watch_abort, Start start, Retire retire, Restart restart, hipStream_t s) {
    const ymt3_config& k = h->cfg;
    const int slots = S.B, R = S.R, d = k.d_model, T = h->T;
    const size_t seg_samples = (size_t)k.segment_samples;
    int rc;
    hipGraphExec_t exec = nullptr;
    // one replayed graph per round of `interval` steps when that is at most 64 steps (a graph launch costs ~7 us of stream time on
    // top of its kernels, see replay); else one per step
    const int per_graph = interval <= 64 ? interval : 1;
    if (!h->host_rows) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->host_rows), (size_t)h->maxR * sizeof(int), hipHostMallocDefault));
    // loop state (after the caller's init kernel): every row starts stopped; admissions start them
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->finished), 1, (size_t)R, s));
    HIP_TRY(hipMemsetAsync(h->row_pos, 0, (size_t)R * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(h->row_out, 0, (size_t)R * sizeof(long long), s));
    HIP_TRY(hipMemsetAsync(h->row_prompt, 0, (size_t)R * sizeof(long long), s));
    if (h->use_graph) {
        rc = step_graph(h, S, h->shared, per_graph, &exec);
        if (rc) return rc;
    }

    std::vector<int> slot_seg((size_t)slots, -1), free_slots;
    auto admit = [&](int first_seg, int nb) -> int {
        LAUNCH(launch_logmel(h->fe, audio_dev + (size_t)first_seg * seg_samples, h->mel, nb, s));
        int rce = encode_impl(h, h->mel, nb, h->enc_out, s);
        if (rce) return rce;
        for (int i = 0; i < nb; ++i) {
            const int slot = free_slots[(size_t)i];
            rce = launch_cross_kv(h, h->enc_out + (size_t)i * T * d, 1, slot, slots, s);
            if (!rce) rce = start(slot, first_seg + i);
            if (rce) return rce;
            slot_seg[(size_t)slot] = first_seg + i;
        }
        return YMT3_OK;
    };
    for (int i = 0; i < slots; ++i) free_slots.push_back(i);
    rc = admit(0, slots);
    if (rc) return rc;
    int next = slots, live = slots;
    // every live segment stops within n_total steps, so the loop is bounded; the guard only catches a logic error
    const long max_rounds = ((long)n_segments / slots + 2) * ((n_total + interval - 1) / interval + 1);
    h->last_steps = 0;
    for (long round = 0; live > 0; ++round) {
        h->last_steps += interval;
        if (round > max_rounds) FAIL(YMT3_ERR_HIP, "slot scheduler made no progress (%d live, %d admitted of %d)", live, next, n_segments);
        for (int i = 0; i < interval; i += exec ? per_graph : 1) {
            if (exec) HIP_TRY(hipGraphLaunch(exec, s));
            else { int rcs = launch_step(h, S, h->shared, s); if (rcs) return rcs; }
        }
        HIP_TRY(hipMemcpyAsync(h->host_rows, h->finished, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (watch_abort) {
            if (h->forced_abort && h->chain_host_abort) *h->chain_host_abort = 1u;          // debug hook: as a kernel would have during the round
            if (h->chain_host_abort && *static_cast<volatile unsigned*>(h->chain_host_abort)) return restart();
        }
        free_slots.clear();
        for (int slot = 0; slot < slots; ++slot) {
            if (slot_seg[(size_t)slot] < 0) continue;
            bool all = true;
            for (int c = 0; c < rows; ++c) all = all && h->host_rows[slot * rows + c] != 0;
            if (!all) continue;
            rc = retire(slot);
            if (rc) return rc;
            slot_seg[(size_t)slot] = -1;
            --live;
            free_slots.push_back(slot);
        }
        const int nb = std::min((int)free_slots.size(), n_segments - next);
        if (nb > 0) {
            rc = admit(next, nb);
            if (rc) return rc;
            next += nb;
            live += nb;
        }
    }
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

// continuous batching.  `slots` decoder slots are kept busy from a queue of segments: each row
// decodes at its own position (slot mode of the step kernels), the host looks at the per-row `finished` flags every
// `interval` steps, pads and retires segments whose rows have all stopped, and encodes the next pending segments straight
// into the freed slots (log-mel + encoder batched over the admissions, cross-K/V written into each slot's slabs).  Rows are
// independent in every kernel, so the ids equal those of lock-step batches bit for bit.
extern "C" int ymt3_transcribe_stream_constrained(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps,
                                                  const int32_t* prompt_dev, int n_prompt, int32_t* tokens_dev, float* scores_dev, int slots,
                                                  int interval, ymt3_constraint constraint, const int32_t* start_state_dev, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    ConstraintView cv{};
    rc = constraint_view(h, constraint, start_state_dev, &cv);
    if (rc) return rc;
    if (n_segments < 0) FAIL(YMT3_ERR_ARG, "n_segments=%d", n_segments);
    if (n_segments == 0) return YMT3_OK;
    if (!audio_dev || !tokens_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    const ymt3_config& k = h->cfg;
    rc = check_steps(h, n_steps, prompt_dev, n_prompt, 0);
    if (rc) return rc;
    if (interval < 0) FAIL(YMT3_ERR_ARG, "interval=%d", interval);
    if (h->prof_step0) FAIL(YMT3_ERR_UNSUPPORTED, "ymt3_debug_decode_start is pending: it applies to lock-step decode calls only");
    if (interval == 0) interval = 8;
    if (slots <= 0 || slots > h->maxB) slots = h->maxB;
    if (slots > n_segments) slots = n_segments;
    hipStream_t s = (hipStream_t)stream;
    const int K = k.n_channels, R = slots * K;

    const StepShape S = step_shape(h, SM_SLOT, slots, 0, R, 1, false);
    ArgmaxArgs a = argmax_base(h, R, true);  // (slot mode: with the per-row positions and offsets)
    h->last_qkv0 = S.qkv0;
    qkv0_wire(h, S.qkv0, &a);
    rc = zero_step_sync(h, s);
    if (rc) return rc;
    ConstraintView cv_init = cv;
    cv_init.start = nullptr;                  // (the rows' states are seeded at admission, from their segment's start states)
    LAUNCH(launch_decode_init(a, 1, n_steps, 0, tokens_dev, nullptr, nullptr, prompt_dev, n_prompt, scores_dev, cv_init, s));

    auto start = [&](int slot, int seg) -> int {
        ConstraintView cv_seg = cv;
        if (cv.start) cv_seg.start = cv.start + (size_t)seg * K;
        LAUNCH(launch_slot_start(a, slot * K, (long long)seg * K * n_steps, n_steps, h->row_out, (long long)seg * K * n_prompt, n_prompt,
                                 h->row_prompt, cv_seg, s));
        return YMT3_OK;
    };
    auto retire = [&](int slot) -> int {
        LAUNCH(launch_slot_retire(a, slot * K, K, n_steps, n_prompt, tokens_dev, scores_dev, s));
        return YMT3_OK;
    };
    // a merged kernel gave up (the stream is idle when this is called): start the queue again on the separate launches -- same ids
    auto restart = [&]() -> int {
        int rcf = merged_fallback(h);
        if (rcf) return rcf;
        return ymt3_transcribe_stream_constrained(h, audio_dev, n_segments, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev, slots, interval,
                                                  constraint, start_state_dev, stream);
    };
    return run_slot_queue(h, audio_dev, n_segments, S, K, interval, n_prompt + n_steps, true, start, retire, restart, s);
}

extern "C" int ymt3_transcribe_stream_scored(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev,
                                             int n_prompt, int32_t* tokens_dev, float* scores_dev, int slots, int interval, void* stream) {
    return ymt3_transcribe_stream_constrained(h, audio_dev, n_segments, n_steps, prompt_dev, n_prompt, tokens_dev, scores_dev, slots, interval,
                                              nullptr, nullptr, stream);
}

extern "C" int ymt3_transcribe_stream_prompted(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev,
                                               int n_prompt, int32_t* tokens_dev, int slots, int interval, void* stream) {
    return ymt3_transcribe_stream_scored(h, audio_dev, n_segments, n_steps, prompt_dev, n_prompt, tokens_dev, nullptr, slots, interval, stream);
}

extern "C" int ymt3_transcribe_stream(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, int32_t* tokens_dev,
                                      int slots, int interval, void* stream) {
    return ymt3_transcribe_stream_prompted(h, audio_dev, n_segments, n_steps, nullptr, 0, tokens_dev, slots, interval, stream);
}

// Beam search under continuous batching (include/ymt3.h): the queue loop above with slots of n_channels * W rows.  A slot is started by
// beam_slot_start_kernel and harvested by the result kernel over its groups when all of them are done; the steps are launch_step's beam
// steps with per-row positions (mode SM_SLOT_BEAM).  Every per-call and per-slot value lives in device memory, so the step
// graph depends on (slots, W, steps per graph) only.
extern "C" int ymt3_transcribe_stream_beam(ymt3_handle h, const float* audio_dev, int n_segments, int n_steps, const int32_t* prompt_dev,
                                           int n_prompt, const ymt3_beam_params* params, int32_t* tokens_dev, float* seq_scores_dev,
                                           float* token_scores_dev, int slots, int interval, ymt3_constraint constraint,
                                           const int32_t* start_state_dev, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    ConstraintView cv{};
    rc = constraint_view(h, constraint, start_state_dev, &cv);
    if (rc) return rc;
    if (n_segments < 0) FAIL(YMT3_ERR_ARG, "n_segments=%d", n_segments);
    rc = beam_check(h, 0, n_steps, prompt_dev, n_prompt, params, tokens_dev);
    if (rc) return rc;
    if (interval < 0) FAIL(YMT3_ERR_ARG, "interval=%d", interval);
    const ymt3_config& k = h->cfg;
    const int W = params->num_beams, K = k.n_channels;
    if (h->maxB / W < 1) FAIL(YMT3_ERR_ARG, "num_beams=%d exceeds max_batch=%d: not one slot of n_channels * num_beams rows fits", W, h->maxB);
    if (n_segments == 0) return YMT3_OK;
    if (!audio_dev || !tokens_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    if (interval == 0) interval = 8;
    if (slots <= 0 || slots > h->maxB / W) slots = h->maxB / W;
    if (slots > n_segments) slots = n_segments;
    hipStream_t s = (hipStream_t)stream;
    const int rows = K * W, R = slots * rows;

    const StepShape S = step_shape(h, SM_SLOT_BEAM, slots, W, R, 1, false);
    const BeamArgs b = beam_args(h, R, W, h->shared, true);
    BeamShared bp = h->beam_trace;
    bp.alpha = params->length_penalty; bp.tokens_out = tokens_dev; bp.seq_out = seq_scores_dev; bp.tok_out = token_scores_dev;
    h->last_chains = 1;
    h->last_qkv0 = S.qkv0;
    ConstraintView cv_init = cv;
    cv_init.start = nullptr;                  // (the groups' states are seeded at admission, from their segment's start states)
    LAUNCH(launch_beam_init(b, n_steps, prompt_dev, n_prompt, cv_init, bp, s));

    const int N = params->num_return;
    auto start = [&](int slot, int seg) -> int {
        ConstraintView cv_seg = cv;
        if (cv.start) cv_seg.start = cv.start + (size_t)seg * K;
        LAUNCH(launch_beam_slot_start(b, slot * rows, (long long)seg * K, n_prompt, cv_seg, s));
        return YMT3_OK;
    };
    auto retire = [&](int slot) -> int {
        LAUNCH(launch_beam_slot_finalize(b, slot * rows, N, s));
        return YMT3_OK;
    };
    auto restart = []() -> int { return YMT3_OK; };      // (beam steps hold no merged kernel)
    return run_slot_queue(h, audio_dev, n_segments, S, rows, interval, n_prompt + n_steps, false, start, retire, restart, s);
}

extern "C" int ymt3_test_gemm(ymt3_handle h, const void* a_dev, const void* w_dev, float* c_dev, int M, int N, int K, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    GemmArgs g{static_cast<const bf16_t*>(a_dev), static_cast<const bf16_t*>(w_dev), c_dev, nullptr, M, N, K, K, K, N, 0, 0, 0};
    LAUNCH(launch_gemm(EPI_F32, g, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

// ---------------------------------------------------------------- per-kernel test doors (include/ymt3.h)
// What a raw pointer can be checked for; the extents behind it are the caller's (model.py).
static bool door_ptr_ok(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
#define DOOR_PTR(p) do { if (!door_ptr_ok(p)) FAIL(YMT3_ERR_ARG, "%s: %s is %s", __func__, #p, (p) ? "not aligned to 16 bytes" : "null"); } while (0)
#define DOOR_REQUIRE(cond) do { if (!(cond)) FAIL(YMT3_ERR_ARG, "%s: needs %s", __func__, #cond); } while (0)

extern "C" int ymt3_test_gemm_ex(ymt3_handle h, int epilogue, const void* a_dev, const void* w_dev, void* out_dev, const float* bias_dev, int M,
                                 int N, int K, int lda, int ldw, int ldc, int T, int H, int n_seg, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    DOOR_PTR(a_dev); DOOR_PTR(w_dev); DOOR_PTR(out_dev);
    if (bias_dev) DOOR_PTR(bias_dev);
    DOOR_REQUIRE(epilogue >= EPI_F32 && epilogue <= EPI_KV_HEADMAJOR);
    DOOR_REQUIRE(bias_dev == nullptr || epilogue == EPI_F32);
    DOOR_REQUIRE(M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 64 == 0);
    DOOR_REQUIRE(lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0);
    if (epilogue == EPI_KV_HEADMAJOR) {
        DOOR_REQUIRE(T > 0 && H > 0 && n_seg > 0 && N % (H * 64) == 0);
        DOOR_REQUIRE((long long)n_seg * T == M);
    } else {
        DOOR_REQUIRE(ldc >= N && ldc % 8 == 0);
    }
    GemmArgs g{static_cast<const bf16_t*>(a_dev), static_cast<const bf16_t*>(w_dev), out_dev, bias_dev, M, N, K, lda, ldw, ldc, T, H, n_seg};
    LAUNCH(launch_gemm(epilogue, g, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_rmsnorm(ymt3_handle h, const float* x_dev, const float* gain_dev, void* out_dev, int M, int d, float eps, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    DOOR_PTR(x_dev); DOOR_PTR(gain_dev); DOOR_PTR(out_dev);
    DOOR_REQUIRE(M > 0 && d > 0 && d % 4 == 0);
    LAUNCH(launch_rmsnorm(x_dev, gain_dev, static_cast<bf16_t*>(out_dev), M, d, eps, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_enc_attention(ymt3_handle h, const void* q_dev, int ldq, const void* k_dev, const void* v_dev, int ldkv,
                                       const float* bias_off_dev, void* out_dev, int B, int T, int H, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    DOOR_PTR(q_dev); DOOR_PTR(k_dev); DOOR_PTR(v_dev); DOOR_PTR(bias_off_dev); DOOR_PTR(out_dev);
    DOOR_REQUIRE(T == 64 || T == 128 || T == 256 || T == 512);
    DOOR_REQUIRE(B > 0 && H > 0 && H <= 65535 && B <= 65535);
    DOOR_REQUIRE(ldq >= H * 64 && ldkv >= H * 64 && ldq % 8 == 0 && ldkv % 8 == 0);
    LAUNCH(launch_enc_attention_qkv(static_cast<const bf16_t*>(q_dev), ldq, static_cast<const bf16_t*>(k_dev), static_cast<const bf16_t*>(v_dev), ldkv,
                                    bias_off_dev, static_cast<bf16_t*>(out_dev), B, T, H, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_seq_attention(ymt3_handle h, const ymt3_seq_attn_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_seq_attn_args& c = *args;
    DOOR_PTR(c.q); DOOR_PTR(c.k); DOOR_PTR(c.v); DOOR_PTR(c.out);
    if (c.bias_off) DOOR_PTR(c.bias_off);
    DOOR_REQUIRE(c.n_seq > 0 && c.H > 0 && c.inner_n > 0);
    DOOR_REQUIRE(c.Tq > 0 && c.Tq % 16 == 0);
    DOOR_REQUIRE(c.Tk == 32 || c.Tk == 64 || c.Tk == 128 || c.Tk == 256);
    DOOR_REQUIRE(c.bias_off == nullptr || c.Tq == c.Tk);
    DOOR_REQUIRE(c.q_step > 0 && c.kv_step > 0 && c.o_step > 0);
    DOOR_REQUIRE(c.q_outer >= 0 && c.q_inner >= 0 && c.kv_outer >= 0 && c.kv_inner >= 0 && c.o_outer >= 0 && c.o_inner >= 0);
    DOOR_REQUIRE((c.q_step | c.kv_step | c.o_step | c.q_outer | c.q_inner | c.kv_outer | c.kv_inner | c.o_outer | c.o_inner) % 8 == 0);
    SeqAttnArgs a{};
    a.q = static_cast<const bf16_t*>(c.q); a.k = static_cast<const bf16_t*>(c.k); a.v = static_cast<const bf16_t*>(c.v);
    a.out = static_cast<bf16_t*>(c.out); a.bias_off = c.bias_off;
    a.n_seq = c.n_seq; a.H = c.H; a.Tq = c.Tq; a.Tk = c.Tk; a.inner_n = c.inner_n;
    a.q_outer = c.q_outer; a.q_inner = c.q_inner; a.q_step = c.q_step;
    a.kv_outer = c.kv_outer; a.kv_inner = c.kv_inner; a.kv_step = c.kv_step;
    a.o_outer = c.o_outer; a.o_inner = c.o_inner; a.o_step = c.o_step;
    LAUNCH(launch_seq_attention(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_spec_embed(ymt3_handle h, const float* mel_dev, const float* w_dev, const void* pos_dev, const float* gain_dev,
                                    void* out_dev, long long n_rows, int F, int d, float eps, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    DOOR_PTR(mel_dev); DOOR_PTR(w_dev); DOOR_PTR(pos_dev); DOOR_PTR(gain_dev); DOOR_PTR(out_dev);
    DOOR_REQUIRE(n_rows > 0 && F > 0 && d > 0 && d % 4 == 0 && d <= 256);
    LAUNCH(launch_spec_embed(mel_dev, w_dev, static_cast<const bf16_t*>(pos_dev), gain_dev, static_cast<bf16_t*>(out_dev), n_rows, F, d, eps,
                             (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

// The decoder doors' own DecodeShared (never the handle's h->shared, which the decode loop owns): zero but for `step`, set on the caller's stream
// in front of the launch that reads it.
static int door_shared(ymt3_ctx* c, int step, hipStream_t s, const DecodeShared** out) {
    if (!c->test_shared) {
        if (dev_alloc(c, (void**)&c->test_shared, sizeof(DecodeShared))) return YMT3_ERR_HIP;
        HIP_TRY(hipMemset(c->test_shared, 0, sizeof(DecodeShared)));
    }
    static_assert(offsetof(DecodeShared, step) == 0, "the position is the block's first word");
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->test_shared), step, 1, s));
    *out = c->test_shared;
    return YMT3_OK;
}

extern "C" int ymt3_test_dec_gemm(ymt3_handle h, int mode, const ymt3_dec_gemm_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_dec_gemm_args& c = *args;
    DOOR_REQUIRE(mode >= DG_NORM_QKV_CACHE && mode <= DG_RESID);
    const bool norm = mode != DG_RESID, qkv = mode == DG_NORM_QKV_CACHE;
    DOOR_PTR(c.W);
    DOOR_REQUIRE(c.R > 0 && c.row0 >= 0 && c.row0 <= 0xffff && c.R <= 0xffff && c.N > 0 && c.N % 16 == 0);
    DOOR_REQUIRE(norm ? c.K == 512 : (c.K == 512 || c.K == 1024 || c.K == 2048));
    DOOR_REQUIRE(c.pend_y == nullptr || qkv || mode == DG_NORM_LOGITS);
    DOOR_REQUIRE(c.part == nullptr || !norm);
    DOOR_REQUIRE(c.table == nullptr || (qkv && c.pend_y == nullptr));
    DOOR_REQUIRE(c.h_out == nullptr || (qkv && c.pend_y != nullptr));
    if (norm) {
        DOOR_PTR(c.x_f32); DOOR_PTR(c.gain);
        if (c.pend_y) DOOR_PTR(c.pend_y);
        else { DOOR_PTR(c.ssq); DOOR_REQUIRE(c.ssq_stride >= c.row0 + c.R); }
    } else {
        DOOR_PTR(c.a_bf16); DOOR_PTR(c.out_f32); DOOR_PTR(c.ssq);
        DOOR_REQUIRE(c.ssq_stride >= c.row0 + c.R);
        DOOR_REQUIRE(c.N == 16 * SSQ_TILES);
        if (c.part) DOOR_PTR(c.part);
    }
    if (qkv) {
        DOOR_REQUIRE(c.H > 0 && c.H <= 0xff && c.L > 0 && c.L <= 0xfffff && c.N == 3 * c.H * 64);
        if (c.table) DOOR_PTR(c.table);
        else { DOOR_PTR(c.out_bf16); DOOR_PTR(c.kcache); DOOR_PTR(c.vcache); }
        if (c.pend_y) { DOOR_PTR(c.h_out); DOOR_REQUIRE(c.h_out != c.x_f32); }
        if (c.row_pos) DOOR_PTR(c.row_pos);
        else DOOR_REQUIRE(c.step >= 0 && c.step < c.L);
    } else if (mode == DG_NORM_LOGITS) {
        DOOR_PTR(c.out_f32);
    } else if (norm) {
        DOOR_PTR(c.out_bf16);
    }
    const int mid = c.mid_rows >= 0 ? c.mid_rows : DEC_GEMM_MID_ROWS;
    if (mid > 0 && c.R >= mid)      // the mid-size tile kernel: launch_dec_gemm falls back to the 16-row tiles where it has no instantiation
        DOOR_REQUIRE(c.N % 64 == 0 && c.part == nullptr && c.pend_y == nullptr && c.table == nullptr && (c.K == 512 || (c.K == 2048 && !norm)));
    DecGemmArgs a{};
    a.x_f32 = c.x_f32; a.gain = c.gain; a.a_bf16 = static_cast<const bf16_t*>(c.a_bf16); a.W = static_cast<const bf16_t*>(c.W);
    a.row0 = c.row0; a.R = c.R; a.N = c.N; a.K = c.K; a.eps = c.eps;
    a.out_bf16 = static_cast<bf16_t*>(c.out_bf16); a.out_f32 = c.out_f32;
    a.kcache = static_cast<bf16_t*>(c.kcache); a.vcache = static_cast<bf16_t*>(c.vcache); a.H = c.H; a.L = c.L;
    a.row_pos = c.row_pos; a.ssq = c.ssq; a.ssq_stride = c.ssq_stride;
    a.part = c.part; a.pend_y = c.pend_y; a.h_out = c.h_out; a.mid_rows = c.mid_rows; a.table = static_cast<bf16_t*>(c.table);
    if (qkv) {                      // (the table build reads the position too, and ignores it)
        rc = door_shared(h, c.row_pos || c.table ? 0 : c.step, (hipStream_t)stream, &a.shared);
        if (rc) return rc;
    }
    LAUNCH(launch_dec_gemm(mode, a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_dec_attention(ymt3_handle h, const ymt3_dec_attn_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_dec_attn_args& c = *args;
    const bool self = c.self_attn != 0;
    DOOR_PTR(c.k); DOOR_PTR(c.v);
    DOOR_REQUIRE(c.R > 0 && c.row0 >= 0 && c.row0 <= 0xffff && c.R <= 0xffff && c.H >= 1 && c.H <= 0xff);
    DOOR_REQUIRE(c.slab_keys >= 1 && c.slab_keys <= 0xfffff && c.rows_per_kv >= 1 && c.rows_per_kv <= 0xff);
    const bool many = c.force_many || c.R * c.H > 2048;
    DecAttnArgs a{};
    if (self) {
        DOOR_PTR(c.q); DOOR_PTR(c.bias);
        DOOR_REQUIRE(c.bias_stride == c.slab_keys && c.n_keys_const == 0);
        DOOR_REQUIRE(c.wq == nullptr && c.x_f32 == nullptr && c.gain == nullptr && c.ssq == nullptr && c.ipart == nullptr);
        if (c.row_pos) DOOR_PTR(c.row_pos);
        else DOOR_REQUIRE(c.step >= 0 && c.step < c.slab_keys);
        if (c.wo) {
            DOOR_PTR(c.wo); DOOR_PTR(c.opart);
            DOOR_REQUIRE(c.H == 8 && !many && c.anc == nullptr);
        } else {
            DOOR_PTR(c.out);
            DOOR_REQUIRE(c.opart == nullptr);
        }
        if (c.anc) {
            DOOR_PTR(c.anc);
            DOOR_REQUIRE(c.W >= 1 && c.W <= BEAM_MAX && c.R % c.W == 0 && c.row0 % c.W == 0 && c.rows_per_kv == 1);
            DOOR_REQUIRE(c.anc_pitch % 16 == 0 && c.anc_pitch > c.slab_keys && c.anc_pitch <= 48 * 1024 && c.row0 + c.R <= c.anc_rows);
        }
    } else {
        DOOR_PTR(c.out);
        DOOR_REQUIRE(c.bias == nullptr && c.row_pos == nullptr && c.anc == nullptr && c.wo == nullptr && c.opart == nullptr);
        DOOR_REQUIRE(c.n_keys_const >= 1 && c.n_keys_const <= c.slab_keys && c.n_keys_const <= 0xfff);
        if (c.wq) {
            DOOR_PTR(c.wq); DOOR_PTR(c.x_f32); DOOR_PTR(c.gain);
            DOOR_REQUIRE(c.d == 512 && !c.force_many);          // one thread per element of the residual row; 8 waves whatever the row count
            if (c.ipart) { DOOR_PTR(c.ipart); DOOR_REQUIRE(c.H == 8 && c.ssq == nullptr && !many); }
            else { DOOR_PTR(c.ssq); DOOR_REQUIRE(c.ssq_stride >= c.row0 + c.R); }
        } else {
            DOOR_PTR(c.q);
            DOOR_REQUIRE(c.x_f32 == nullptr && c.gain == nullptr && c.ssq == nullptr && c.ipart == nullptr);
        }
    }
    a.q = static_cast<const bf16_t*>(c.q); a.k = static_cast<const bf16_t*>(c.k); a.v = static_cast<const bf16_t*>(c.v);
    a.out = static_cast<bf16_t*>(c.out); a.bias = c.bias; a.row_pos = c.row_pos;
    a.n_keys_const = c.n_keys_const; a.slab_keys = c.slab_keys; a.rows_per_kv = c.rows_per_kv;
    a.row0 = c.row0; a.R = c.R; a.H = c.H; a.bias_stride = c.bias_stride;
    a.wq = static_cast<const bf16_t*>(c.wq); a.x_f32 = c.x_f32; a.gain = c.gain; a.ssq = c.ssq; a.ssq_stride = c.ssq_stride; a.eps = c.eps;
    a.wo = static_cast<const bf16_t*>(c.wo); a.opart = c.opart; a.ipart = c.ipart; a.force_many = c.force_many ? 1 : 0;
    if (self) {
        rc = door_shared(h, c.row_pos ? 0 : c.step, (hipStream_t)stream, &a.shared);
        if (rc) return rc;
    }
    if (c.anc) {
        const BeamAttn ba{c.anc, c.anc_rows, c.anc_pitch, c.W};
        LAUNCH(launch_dec_attention_beam(a, ba, (hipStream_t)stream));
    } else {
        LAUNCH(launch_dec_attention(self, a, (hipStream_t)stream));
    }
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_mc_cross_attention(ymt3_handle h, const ymt3_mc_cross_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_mc_cross_args& c = *args;
    DOOR_PTR(c.x_f32); DOOR_PTR(c.gain); DOOR_PTR(c.ssq); DOOR_PTR(c.wq); DOOR_PTR(c.k); DOOR_PTR(c.v); DOOR_PTR(c.out);
    DOOR_REQUIRE(c.n_seg > 0 && c.n_seg <= 65535 && c.H >= 1 && c.H <= 0xff && c.row0 >= 0 && c.row0 <= 0xffff);
    DOOR_REQUIRE(c.n_channels >= 2 && c.n_channels <= 16);
    DOOR_REQUIRE(c.T == 128 || c.T == 256 || c.T == 512);
    DOOR_REQUIRE(c.d == 512 && c.ssq_stride >= c.row0 + c.n_seg * c.n_channels);
    McCrossArgs a{};
    a.x_f32 = c.x_f32; a.gain = c.gain; a.ssq = c.ssq; a.ssq_stride = c.ssq_stride; a.wq = static_cast<const bf16_t*>(c.wq);
    a.k = static_cast<const bf16_t*>(c.k); a.v = static_cast<const bf16_t*>(c.v); a.out = static_cast<bf16_t*>(c.out);
    a.row0 = c.row0; a.n_seg = c.n_seg; a.n_channels = c.n_channels; a.H = c.H; a.T = c.T; a.eps = c.eps;
    LAUNCH(launch_mc_cross_attention(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_moe_stage(ymt3_handle h, int stage, const ymt3_moe_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_moe_args& c = *args;
    DOOR_REQUIRE(stage >= 0 && stage <= 3);
    DOOR_REQUIRE(c.d_model == 512 && c.d_ff == 2048 && c.top_k == 2);
    DOOR_REQUIRE(c.E >= 2 && c.E <= 16);
    DOOR_REQUIRE(c.R >= 1 && c.R <= 1536 && c.row0 >= 0 && c.row0 <= 0xffff && c.ssq_stride >= c.row0 + c.R);
    const bool fp8 = c.fp8 != 0;
    if (stage == 0) {
        DOOR_PTR(c.h); DOOR_PTR(c.gain); DOOR_PTR(c.ssq); DOOR_PTR(c.router); DOOR_PTR(c.xn); DOOR_PTR(c.sel); DOOR_PTR(c.gate);
    } else if (stage == 1) {
        DOOR_PTR(c.xn); DOOR_PTR(c.sel); DOOR_PTR(c.hidden);
        if (fp8) { DOOR_PTR(c.wi_q8); DOOR_PTR(c.wi_s); } else DOOR_PTR(c.wi);
    } else if (stage == 2) {
        DOOR_PTR(c.hidden); DOOR_PTR(c.sel); DOOR_PTR(c.gate); DOOR_PTR(c.y);
        if (fp8) { DOOR_PTR(c.wo_q8); DOOR_PTR(c.wo_s); } else DOOR_PTR(c.wo);
    } else {
        DOOR_PTR(c.h); DOOR_PTR(c.y); DOOR_PTR(c.ssq);
    }
    MoeArgs a{};                    // sel_trace stays null: the router records nothing and reads no DecodeShared
    a.h = c.h; a.gain = c.gain; a.ssq = c.ssq; a.ssq_stride = c.ssq_stride; a.router = static_cast<const bf16_t*>(c.router);
    a.wi = static_cast<const bf16_t*>(c.wi); a.wo = static_cast<const bf16_t*>(c.wo);
    a.wi_q8 = static_cast<const uint8_t*>(c.wi_q8); a.wo_q8 = static_cast<const uint8_t*>(c.wo_q8); a.wi_s = c.wi_s; a.wo_s = c.wo_s;
    a.fp8 = fp8 ? 1 : 0;
    a.xn = static_cast<bf16_t*>(c.xn); a.sel = c.sel; a.gate = c.gate; a.hidden = static_cast<bf16_t*>(c.hidden); a.y = c.y;
    a.row0 = c.row0; a.R = c.R; a.E = c.E; a.top_k = c.top_k; a.d_model = c.d_model; a.d_ff = c.d_ff; a.eps = c.eps;
    LAUNCH(launch_moe_stage(stage, a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_seq_embed(ymt3_handle h, const ymt3_seq_embed_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_seq_embed_args& c = *args;
    DOOR_PTR(c.h); DOOR_PTR(c.embed); DOOR_PTR(c.tokens);
    if (c.chan_embed) { DOOR_PTR(c.chan_embed); DOOR_REQUIRE(c.n_channels >= 1); }
    if (c.n_prompt > 0) DOOR_PTR(c.prompt);
    DOOR_REQUIRE(c.row0 >= 0 && c.n_rows >= 1 && c.n_prompt >= 0 && c.n_steps >= 1 && c.L == c.n_prompt + c.n_steps && c.V >= 1 && c.d == 512);
    SeqEmbedArgs a{};
    a.h = c.h; a.embed = static_cast<const bf16_t*>(c.embed); a.chan_embed = static_cast<const bf16_t*>(c.chan_embed);
    a.prompt = c.n_prompt > 0 ? c.prompt : nullptr; a.tokens = c.tokens;
    a.row0 = c.row0; a.n_rows = c.n_rows; a.L = c.L; a.n_prompt = c.n_prompt; a.n_steps = c.n_steps; a.V = c.V; a.d = c.d;
    a.n_channels = c.n_channels; a.pad_id = c.pad_id;
    LAUNCH(launch_seq_embed(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_dec_seq_attention(ymt3_handle h, const ymt3_dec_seq_attn_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_dec_seq_attn_args& c = *args;
    DOOR_PTR(c.q); DOOR_PTR(c.k); DOOR_PTR(c.v); DOOR_PTR(c.out);
    DOOR_REQUIRE(c.row0 >= 0 && c.n_rows >= 1 && c.n_rows <= 65535 && c.L >= 1 && c.n_keys >= 1 && c.rows_per_kv >= 1 && c.H >= 1 && c.H <= 65535);
    DOOR_REQUIRE(c.ldq >= c.H * 64 && c.ldo >= c.H * 64 && c.ldkv >= 64 && c.kv_head >= 64 && c.q_seq >= 0 && c.kv_seq >= 0 && c.o_seq >= 0);
    // heads inside a key's row (ldkv >= H * 64 when kv_head == 64), or keys inside a head's slab (head-major): no two (head, key) rows overlap
    DOOR_REQUIRE(c.ldkv >= (long long)(c.H - 1) * c.kv_head + 64 || c.kv_head >= (long long)(c.n_keys - 1) * c.ldkv + 64);
    DOOR_REQUIRE((c.ldq | c.ldkv | c.ldo | c.kv_head) % 8 == 0 && (c.q_seq | c.kv_seq | c.o_seq) % 8 == 0);
    if (c.causal) {                 // the kernel clamps a distance beyond the table silently
        DOOR_PTR(c.bias);
        DOOR_REQUIRE(c.n_keys == c.L && c.L <= c.bias_stride);
    } else {
        DOOR_REQUIRE(c.bias == nullptr);
    }
    SeqAttnDecArgs a{};
    a.q = static_cast<const bf16_t*>(c.q); a.k = static_cast<const bf16_t*>(c.k); a.v = static_cast<const bf16_t*>(c.v);
    a.out = static_cast<bf16_t*>(c.out); a.bias = c.bias; a.q_seq = c.q_seq; a.kv_seq = c.kv_seq; a.o_seq = c.o_seq;
    a.ldq = c.ldq; a.ldkv = c.ldkv; a.ldo = c.ldo; a.kv_head = c.kv_head; a.row0 = c.row0; a.n_rows = c.n_rows; a.L = c.L; a.n_keys = c.n_keys;
    a.rows_per_kv = c.rows_per_kv; a.H = c.H; a.bias_stride = c.bias_stride;
    LAUNCH(launch_dec_seq_attention(c.causal != 0, a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_seq_lm_head(ymt3_handle h, const ymt3_seq_lm_head_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_seq_lm_head_args& c = *args;
    DOOR_PTR(c.xn); DOOR_PTR(c.W); DOOR_PTR(c.tokens); DOOR_PTR(c.scores);
    if (c.lengths) DOOR_PTR(c.lengths);
    if (c.logits) DOOR_PTR(c.logits);
    DOOR_REQUIRE(c.row0 >= 0 && c.M >= 1 && c.L >= 1 && c.M % c.L == 0 && c.n_prompt >= 0 && c.n_steps >= 1 && c.L == c.n_prompt + c.n_steps);
    DOOR_REQUIRE(c.d == 512 && c.V >= 16 && c.V % 16 == 0);
    SeqLmHeadArgs a{};
    a.xn = static_cast<const bf16_t*>(c.xn); a.W = static_cast<const bf16_t*>(c.W); a.tokens = c.tokens; a.lengths = c.lengths;
    a.scores = c.scores; a.logits = c.logits; a.M = c.M; a.L = c.L; a.n_prompt = c.n_prompt; a.n_steps = c.n_steps; a.V = c.V; a.d = c.d;
    a.row0 = c.row0;
    LAUNCH(launch_seq_lm_head_score(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

// The token-selection doors' own loop state: a DecodeShared and a BeamShared block per door (never the handle's, never the block of the doors
// above), allocated at first use.  Both are written and read back by one-thread kernels on the caller's stream, so a door call stays asynchronous.
template <typename T>
__global__ void door_block_set_kernel(T* dst, T v) { *dst = v; }
__global__ void door_state_out_kernel(const DecodeShared* sh, int32_t* out) {
    out[0] = sh->step; out[1] = sh->done_count; out[2] = sh->n_unfinished; out[3] = sh->n_steps;
}
static int door_blocks(ymt3_ctx* c, DecodeShared** sh, BeamShared** bs) {
    DecodeShared*& d = bs ? c->test_beam_shared : c->test_tok_shared;
    if (!d) {
        if (dev_alloc(c, (void**)&d, sizeof(DecodeShared))) return YMT3_ERR_HIP;
        HIP_TRY(hipMemset(d, 0, sizeof(DecodeShared)));
    }
    if (bs && !c->test_beam_params) {
        if (dev_alloc(c, (void**)&c->test_beam_params, sizeof(BeamShared))) return YMT3_ERR_HIP;
        HIP_TRY(hipMemset(c->test_beam_params, 0, sizeof(BeamShared)));
    }
    *sh = d;
    if (bs) *bs = c->test_beam_params;
    return YMT3_OK;
}

extern "C" int ymt3_test_token_step(ymt3_handle h, int op, const ymt3_token_step_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_token_step_args& c = *args;
    hipStream_t s = (hipStream_t)stream;
    DOOR_REQUIRE(op >= 0 && op <= 5);
    DOOR_REQUIRE(c.R >= 1 && c.R <= 0xffff && c.row0 >= 0 && c.row0 <= 0xffff);
    DOOR_REQUIRE(c.n_steps >= 1 && c.n_prompt >= 0);
    if (c.state_out) DOOR_PTR(c.state_out);
    const bool embeds = op != 3 && op != 4, slot = c.row_pos != nullptr;
    ArgmaxArgs a{};
    ConstraintView cv{};
    if (embeds) {
        DOOR_PTR(c.h); DOOR_PTR(c.embed); DOOR_PTR(c.ssq);
        DOOR_REQUIRE(c.V >= 1 && c.d >= 1 && c.n_channels >= 1);
        DOOR_REQUIRE(c.pad_id >= 0 && c.pad_id < c.V && c.eos_id < c.V);
        if (c.chan_embed) DOOR_PTR(c.chan_embed);
    }
    if (op <= 2) {
        DOOR_PTR(c.finished);
        // the rows a launch covers: decode_init ignores row0 (rows [0, R)), slot_start restarts the n_channels rows of one segment
        DOOR_REQUIRE(op != 0 || c.row0 == 0);
        DOOR_REQUIRE(c.ssq_stride >= c.row0 + (op == 2 ? c.n_channels : c.R));
        if (c.qkv0) {
            DOOR_PTR(c.qkv0); DOOR_PTR(c.q0); DOOR_PTR(c.kcache0); DOOR_PTR(c.vcache0);
            DOOR_REQUIRE(c.H * 64 * 3 == QKV0_COLS && c.d == QKV0_COLS / 3 && c.L >= 1 && c.chan_embed == nullptr && c.n_channels == 1);
        }
        if (c.row_state) DOOR_PTR(c.row_state);
        if (c.c_allowed) {
            DOOR_PTR(c.c_allowed); DOOR_PTR(c.c_next); DOOR_PTR(c.row_state);
            DOOR_REQUIRE(c.c_n_states >= 1 && c.c_words >= 1 && c.c_words <= (1 << 20) && c.c_words * 32 >= c.V);
        } else {
            DOOR_REQUIRE(c.c_next == nullptr);
        }
        if (c.c_start) {
            DOOR_PTR(c.c_start);
            DOOR_REQUIRE(op != 1 && c.row_state != nullptr && c.c_n_states >= 1);
        }
        cv.allowed = c.c_allowed; cv.next = c.c_next; cv.words = c.c_words; cv.n_states = c.c_n_states; cv.start = c.c_start;
    }
    if (slot) {
        DOOR_REQUIRE(op == 1 || op == 2 || op == 3);
        DOOR_PTR(c.row_pos); DOOR_PTR(c.row_out);
    } else {
        DOOR_REQUIRE(op != 2 && op != 3);
        DOOR_REQUIRE(c.row_out == nullptr && c.row_prompt == nullptr);
    }
    if (c.tokens_out) DOOR_PTR(c.tokens_out);
    if (c.forced) DOOR_PTR(c.forced);
    if (c.logits_out) DOOR_PTR(c.logits_out);
    if (c.scores_out) DOOR_PTR(c.scores_out);
    if (c.prompt) DOOR_PTR(c.prompt);
    DOOR_REQUIRE(c.n_prompt == 0 || op >= 2 || c.prompt != nullptr);      // (slot_start only lays the prompt offsets out)
    a.logits = c.logits; a.h = c.h; a.embed = static_cast<const bf16_t*>(c.embed); a.chan_embed = static_cast<const bf16_t*>(c.chan_embed);
    a.finished = c.finished; a.ssq = c.ssq; a.ssq_stride = c.ssq_stride;
    a.row0 = c.row0; a.R = c.R; a.V = c.V; a.d = c.d; a.n_channels = c.n_channels; a.eos_id = c.eos_id; a.pad_id = c.pad_id;
    a.row_pos = c.row_pos; a.row_out = reinterpret_cast<const long long*>(c.row_out); a.row_prompt = reinterpret_cast<const long long*>(c.row_prompt);
    a.ticket = c.ticket; a.zero_sync = c.zero_sync; a.zero_lines = c.zero_lines; a.row_state = c.row_state;
    a.qkv0 = static_cast<const bf16_t*>(c.qkv0); a.q0 = static_cast<bf16_t*>(c.q0);
    a.kcache0 = static_cast<bf16_t*>(c.kcache0); a.vcache0 = static_cast<bf16_t*>(c.vcache0); a.H = c.H; a.L = c.L;
    static_assert(sizeof(long long) == sizeof(int64_t), "row_out / row_prompt are 64-bit offsets");
    rc = door_blocks(h, &a.shared, nullptr);
    if (rc) return rc;
    switch (op) {
    case 0:
        DOOR_REQUIRE(c.step0 >= 0 && (c.qkv0 == nullptr || c.step0 < c.L));
        DOOR_REQUIRE(c.forced == nullptr || c.tokens_out != nullptr);
        LAUNCH(launch_decode_init(a, 1, c.n_steps, c.step0, c.tokens_out, c.forced, c.logits_out, c.prompt, c.n_prompt, c.scores_out, cv, s));
        h->test_tok_loop = {true, c.step0, c.step0, c.n_steps, c.n_prompt, c.c_allowed != nullptr, 0, c.R};
        break;
    case 1: {
        DOOR_PTR(c.logits); DOOR_PTR(c.tokens_out);
        if (c.ticket) DOOR_PTR(c.ticket);
        if (c.zero_sync) { DOOR_PTR(c.zero_sync); DOOR_REQUIRE(c.zero_lines >= 1); }
        else DOOR_REQUIRE(c.zero_lines == 0);
        ymt3_ctx::DoorLoop loop{true, slot ? 0 : c.step, slot ? 0 : c.step0, c.n_steps, c.n_prompt, c.c_allowed != nullptr, c.row0, c.R};
        if (c.keep_shared) {
            // the block as the previous call of this door left it: its geometry must be this call's (the extents were judged by it)
            DOOR_REQUIRE(h->test_tok_loop.valid && h->test_tok_loop.n_steps == c.n_steps && h->test_tok_loop.n_prompt == c.n_prompt);
            DOOR_REQUIRE(h->test_tok_loop.constrained == (c.c_allowed != nullptr));
            // the rows too: n_unfinished and the extents of the block's output pointers were written and judged for them
            DOOR_REQUIRE(h->test_tok_loop.row0 == c.row0 && h->test_tok_loop.R == c.R);
            loop = h->test_tok_loop;
        }
        if (slot) {
            // slot mode reads neither forced ids nor the logits copy; positions are per row (their values: the caller's, model.py)
            DOOR_REQUIRE(c.forced == nullptr && c.logits_out == nullptr);
            if (c.n_prompt > 0) DOOR_PTR(c.row_prompt);
        } else {
            // the emitted column of this step lies in [-n_prompt, n_steps); the table gather writes q at step + 1 <= L
            DOOR_REQUIRE(loop.step0 >= 0 && loop.step >= loop.step0 && loop.step - loop.step0 - c.n_prompt < c.n_steps);
            DOOR_REQUIRE(c.qkv0 == nullptr || loop.step < c.L);
        }
        if (!c.keep_shared) {
            DecodeShared v{};
            v.step = loop.step; v.step0 = loop.step0; v.done_count = 0; v.n_steps = c.n_steps; v.n_unfinished = c.R;
            v.n_prompt = c.n_prompt; v.tokens_out = c.tokens_out; v.forced = c.forced; v.logits_out = c.logits_out; v.prompt = c.prompt;
            v.scores_out = c.scores_out; v.c_allowed = c.c_allowed; v.c_next = c.c_next; v.c_words = c.c_words;
            door_block_set_kernel<DecodeShared><<<1, 1, 0, s>>>(a.shared, v);
        }
        LAUNCH(launch_argmax_embed(a, s));
        ++loop.step;                               // the last workgroup advances the block's position
        h->test_tok_loop = loop;
        break;
    }
    case 2:
        DOOR_PTR(c.row_prompt);
        DOOR_REQUIRE(c.first_out >= 0 && c.first_prompt >= 0);
        LAUNCH(launch_slot_start(a, c.row0, c.first_out, c.n_steps, reinterpret_cast<long long*>(c.row_out), c.first_prompt, c.n_prompt,
                                 reinterpret_cast<long long*>(c.row_prompt), cv, s));
        break;
    case 3:
        DOOR_PTR(c.tokens_out);
        LAUNCH(launch_slot_retire(a, c.row0, c.R, c.n_steps, c.n_prompt, c.tokens_out, c.scores_out, s));
        break;
    case 4:
        DOOR_PTR(c.tokens_out);
        DOOR_REQUIRE(c.from >= 0 && c.from <= c.n_steps);
        LAUNCH(launch_pad_tail(c.tokens_out, c.scores_out, c.row0, c.R, c.n_steps, c.from, c.pad_id, s));
        break;
    default:
        // rows [0, R) of h and ssq take the embeddings of ids [v0, v0 + R)
        DOOR_REQUIRE(c.row0 == 0 && c.chan_embed == nullptr && c.v0 >= 0 && c.v0 + c.R <= c.V && c.ssq_stride >= c.R);
        LAUNCH(launch_qkv0_embed(a, c.v0, c.R, s));
        break;
    }
    if (c.state_out) door_state_out_kernel<<<1, 1, 0, s>>>(a.shared, c.state_out);
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

extern "C" int ymt3_test_beam_step(ymt3_handle h, int op, const ymt3_beam_step_args* args, void* stream) {
    int rc = check_call(h, 0);
    if (rc) return rc;
    if (!args) FAIL(YMT3_ERR_ARG, "%s: args is null", __func__);
    const ymt3_beam_step_args& c = *args;
    hipStream_t s = (hipStream_t)stream;
    DOOR_REQUIRE(op >= 0 && op <= 4);
    DOOR_PTR(c.h); DOOR_PTR(c.embed); DOOR_PTR(c.ssq); DOOR_PTR(c.finished); DOOR_PTR(c.anc); DOOR_PTR(c.slot_anc);
    DOOR_PTR(c.fed_tok); DOOR_PTR(c.fed_lp); DOOR_PTR(c.run);
    DOOR_PTR(c.fin_score); DOOR_PTR(c.fin_len); DOOR_PTR(c.fin_store); DOOR_PTR(c.fin_tok); DOOR_PTR(c.fin_lp); DOOR_PTR(c.n_fin);
    if (c.chan_embed) DOOR_PTR(c.chan_embed);
    if (c.state_out) DOOR_PTR(c.state_out);
    DOOR_REQUIRE(c.W >= 1 && c.W <= BEAM_MAX && c.R >= 1 && c.R <= 0xffff && c.R % c.W == 0 && c.R <= c.anc_rows);
    DOOR_REQUIRE(c.V >= 1 && c.d >= 1 && c.n_channels >= 1 && c.ssq_stride >= c.R);
    DOOR_REQUIRE(c.pad_id >= 0 && c.pad_id < c.V && c.eos_id < c.V);
    DOOR_REQUIRE(c.n_steps >= 1 && c.n_prompt >= 0 && (c.n_prompt == 0 || c.prompt != nullptr));
    DOOR_REQUIRE(c.anc_pitch % 16 == 0 && c.anc_pitch <= 48 * 1024 && c.n_prompt + c.n_steps < c.anc_pitch && c.n_prompt + c.n_steps < c.fed_pitch);
    if (c.prompt) DOOR_PTR(c.prompt);
    if (c.row_state) DOOR_PTR(c.row_state);
    if (c.c_allowed) {
        DOOR_PTR(c.c_allowed); DOOR_PTR(c.c_next); DOOR_PTR(c.row_state);
        DOOR_REQUIRE(c.c_n_states >= 1 && c.c_words >= 1 && c.c_words <= (1 << 20) && c.c_words * 32 >= c.V);
    } else {
        DOOR_REQUIRE(c.c_next == nullptr);
    }
    if (c.c_start) {
        DOOR_PTR(c.c_start);
        DOOR_REQUIRE((op == 0 || op == 3) && c.row_state != nullptr && c.c_n_states >= 1);
    }
    const bool slot = c.row_pos != nullptr;
    if (slot) {
        DOOR_REQUIRE(op == 1 || op == 3 || op == 4);
        DOOR_PTR(c.row_pos); DOOR_PTR(c.row_out); DOOR_PTR(c.row_prompt);
    } else {
        DOOR_REQUIRE(op != 3 && op != 4 && c.row_out == nullptr && c.row_prompt == nullptr);
    }
    const ConstraintView cv{c.c_allowed, c.c_next, c.c_words, c.c_n_states, c.c_start};
    BeamArgs a{};
    a.logits = c.logits; a.h = c.h; a.embed = static_cast<const bf16_t*>(c.embed); a.chan_embed = static_cast<const bf16_t*>(c.chan_embed);
    a.finished = c.finished; a.ssq = c.ssq; a.ssq_stride = c.ssq_stride;
    a.R = c.R; a.V = c.V; a.d = c.d; a.n_channels = c.n_channels; a.eos_id = c.eos_id; a.pad_id = c.pad_id; a.W = c.W;
    a.row_state = c.row_state; a.anc = c.anc; a.anc_rows = c.anc_rows; a.anc_pitch = c.anc_pitch;
    a.fed_tok = c.fed_tok; a.fed_lp = c.fed_lp; a.fed_pitch = c.fed_pitch; a.run = c.run;
    a.fin_score = c.fin_score; a.fin_len = c.fin_len; a.fin_store = c.fin_store; a.fin_tok = c.fin_tok; a.fin_lp = c.fin_lp; a.n_fin = c.n_fin;
    a.slot_anc = c.slot_anc;
    a.row_pos = c.row_pos; a.row_out = reinterpret_cast<long long*>(c.row_out); a.row_prompt = reinterpret_cast<long long*>(c.row_prompt);
    rc = door_blocks(h, &a.shared, &a.beam);
    if (rc) return rc;
    BeamShared params{};
    params.alpha = c.alpha; params.tokens_out = c.tokens_out; params.seq_out = c.seq_out; params.tok_out = c.tok_out;
    if (op == 0 || !c.keep_shared) {
        // what the kernels read from the blocks: the outputs and alpha (init, the result kernels, and select's length penalty)
        DOOR_PTR(c.tokens_out);
        if (c.seq_out) DOOR_PTR(c.seq_out);
        if (c.tok_out) DOOR_PTR(c.tok_out);
        DOOR_REQUIRE(c.alpha >= 0.f && c.alpha <= 16.f);
    }
    ymt3_ctx::DoorLoop loop{true, slot || op == 0 ? 0 : c.step, 0, c.n_steps, c.n_prompt, c.c_allowed != nullptr, 0, c.R};
    if (c.keep_shared && op != 0 && op != 3) {
        // the blocks as the previous call of this door left them: their geometry must be this call's (the extents were judged by it)
        DOOR_REQUIRE(h->test_beam_loop.valid && h->test_beam_loop.n_steps == c.n_steps && h->test_beam_loop.n_prompt == c.n_prompt);
        DOOR_REQUIRE(h->test_beam_loop.constrained == (c.c_allowed != nullptr));
        DOOR_REQUIRE(h->test_beam_loop.R == c.R);
        loop = h->test_beam_loop;
    }
    auto set_blocks = [&](int step) {
        DecodeShared v{};
        v.step = step; v.n_steps = c.n_steps; v.n_unfinished = c.R; v.n_prompt = c.n_prompt; v.prompt = c.prompt;
        v.c_allowed = c.c_allowed; v.c_next = c.c_next; v.c_words = c.c_words;
        door_block_set_kernel<DecodeShared><<<1, 1, 0, s>>>(a.shared, v);
        door_block_set_kernel<BeamShared><<<1, 1, 0, s>>>(a.beam, params);
    };
    switch (op) {
    case 0:
        LAUNCH(launch_beam_init(a, c.n_steps, c.prompt, c.n_prompt, cv, params, s));
        h->test_beam_loop = loop;
        break;
    case 1:
        DOOR_PTR(c.logits);
        // lock-step: position `step` writes ancestry entry and fed token step + 1, below both pitches by the rule above
        if (!slot) DOOR_REQUIRE(loop.step >= 0 && loop.step - c.n_prompt < c.n_steps);
        if (!c.keep_shared) set_blocks(loop.step);
        LAUNCH(launch_beam_select(a, s));
        if (!slot) ++loop.step;                    // the last workgroup advances the block's position (slot mode: the rows' own)
        h->test_beam_loop = loop;
        break;
    case 2:
        DOOR_REQUIRE(c.N >= 1 && c.N <= c.W);
        if (!c.keep_shared) { set_blocks(loop.step); h->test_beam_loop = loop; }
        LAUNCH(launch_beam_finalize(a, c.N, s));
        break;
    case 3:
        DOOR_REQUIRE(c.row0 >= 0 && c.row0 % (c.n_channels * c.W) == 0 && c.row0 + c.n_channels * c.W <= c.R && c.first_group >= 0);
        LAUNCH(launch_beam_slot_start(a, c.row0, c.first_group, c.n_prompt, cv, s));
        break;
    default:
        DOOR_REQUIRE(c.N >= 1 && c.N <= c.W);
        DOOR_REQUIRE(c.row0 >= 0 && c.row0 % (c.n_channels * c.W) == 0 && c.row0 + c.n_channels * c.W <= c.R);
        if (!c.keep_shared) { set_blocks(0); h->test_beam_loop = loop; }
        LAUNCH(launch_beam_slot_finalize(a, c.row0, c.N, s));
        break;
    }
    if (c.state_out) door_state_out_kernel<<<1, 1, 0, s>>>(a.shared, c.state_out);
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}
#undef DOOR_PTR
#undef DOOR_REQUIRE

extern "C" int ymt3_profile_decode(ymt3_handle h, const void* enc_dev, int B, int n_steps, int stride, int32_t* tokens_dev,
                                   float* ms_by_class, int32_t* launches_by_class, void* stream) {
    int rc = check_call(h, B);
    if (rc) return rc;
    if (!enc_dev || !tokens_dev || !ms_by_class || !launches_by_class || stride <= 0 || B == 0) FAIL(YMT3_ERR_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    h->prof_ev.clear();
    h->prof_cls.clear();
    rc = decode_impl(h, static_cast<const bf16_t*>(enc_dev), B, n_steps, nullptr, 0, tokens_dev, nullptr, nullptr, nullptr, ConstraintView{}, s,
                     stride);
    hipError_t e = hipStreamSynchronize(s);
    for (int i = 0; i < YMT3_PROFILE_CLASSES; ++i) { ms_by_class[i] = 0.f; launches_by_class[i] = 0; }
    for (size_t i = 0; i < h->prof_cls.size(); ++i) {
        float ms = 0.f;
        if (rc == 0 && e == hipSuccess && h->prof_cls[i] >= 0 &&
            hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]) == hipSuccess) {
            ms_by_class[h->prof_cls[i]] += ms;
            launches_by_class[h->prof_cls[i]] += 1;
        }
        (void)hipEventDestroy(h->prof_ev[2 * i]);
        (void)hipEventDestroy(h->prof_ev[2 * i + 1]);
    }
    h->prof_ev.clear();
    h->prof_cls.clear();
    if (rc) return rc;
    if (e != hipSuccess) FAIL(YMT3_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    return YMT3_OK;
}
static_assert(PC_COUNT <= YMT3_PROFILE_CLASSES, "profile class table");

extern "C" int ymt3_debug_step_stamps(ymt3_handle h, int32_t* cls, int32_t* grid, uint64_t* stats, int* n_kernels) {
    if (!h || !cls || !grid || !stats || !n_kernels) FAIL(YMT3_ERR_ARG, "null argument");
    if (!h->stamp_buf) FAIL(YMT3_ERR_UNSUPPORTED, "stamps are recorded only by a handle created with YMT3_STAMP=1 in the environment");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> host((size_t)STAMP_WGS * 2);
    *n_kernels = h->stamp_n;
    for (int i = 0; i < h->stamp_n; ++i) {
        const int gsz = h->stamp_grid[i];
        HIP_TRY(hipMemcpy(host.data(), h->stamp_buf + (size_t)i * STAMP_WGS * 2, (size_t)gsz * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long in_min = ~0ull, in_max = 0, out_min = ~0ull, out_max = 0;
        for (int w = 0; w < gsz; ++w) {
            if (host[2 * w] == 0) continue;                          // a launcher may use fewer workgroups than the slot reserves
            in_min = std::min(in_min, host[2 * w]); in_max = std::max(in_max, host[2 * w]);
            out_min = std::min(out_min, host[2 * w + 1]); out_max = std::max(out_max, host[2 * w + 1]);
        }
        cls[i] = h->stamp_cls[i]; grid[i] = gsz;
        stats[4 * i] = in_min; stats[4 * i + 1] = in_max; stats[4 * i + 2] = out_min; stats[4 * i + 3] = out_max;
    }
    return YMT3_OK;
}

extern "C" int ymt3_debug_kernel_stamps(ymt3_handle h, int kernel, uint64_t* stamps, int capacity_wgs) {
    if (!h || !stamps) FAIL(YMT3_ERR_ARG, "null argument");
    if (!h->stamp_buf) FAIL(YMT3_ERR_UNSUPPORTED, "stamps are recorded only by a handle created with YMT3_STAMP=1 in the environment");
    if (kernel < 0 || kernel >= h->stamp_n || capacity_wgs < h->stamp_grid[kernel]) FAIL(YMT3_ERR_ARG, "kernel=%d of %d, capacity %d", kernel, h->stamp_n, capacity_wgs);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    // the caller's capacity decides how much of the kernel's slot comes back (the GEMM chain keeps stage marks behind its [grid][2] stamps)
    const size_t n_wgs = capacity_wgs < STAMP_WGS ? (size_t)capacity_wgs : (size_t)STAMP_WGS;
    HIP_TRY(hipMemcpy(stamps, h->stamp_buf + (size_t)kernel * STAMP_WGS * 2, n_wgs * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return YMT3_OK;
}

extern "C" int ymt3_debug_force_stage_abort(ymt3_handle h) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!h->debug_hooks) FAIL(YMT3_ERR_UNSUPPORTED, "debug hooks are accepted only by a handle created with YMT3_DEBUG_HOOKS=1 in the environment");
    if (!h->chain_sync || !h->chain_host_abort || !(h->gemm_chain || h->attn_pair || h->moe_chain)) FAIL(YMT3_ERR_UNSUPPORTED, "this handle does not run the merged decode kernels");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const unsigned one = 1u;
    // the device word now (what the kernels and the poison pass look at); the host word is what a kernel would set with it --
    // left for the poison pass's caller to observe: set it only after the next decode call, as the kernel would during that call
    HIP_TRY(hipMemcpy(h->chain_sync + CHAIN_ABORT_WORD, &one, sizeof(one), hipMemcpyHostToDevice));
    h->forced_abort = true;
    return YMT3_OK;
}

extern "C" int ymt3_debug_moe_trace(ymt3_handle h, int32_t* trace_dev, int n_steps, int n_rows) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!h->debug_hooks) FAIL(YMT3_ERR_UNSUPPORTED, "debug hooks are accepted only by a handle created with YMT3_DEBUG_HOOKS=1 in the environment");
    if (h->cfg.dec_ffn != YMT3_FFN_MOE) FAIL(YMT3_ERR_UNSUPPORTED, "this handle has no MoE router");
    if (trace_dev && (n_steps <= 0 || n_rows <= 0)) FAIL(YMT3_ERR_ARG, "n_steps=%d n_rows=%d", n_steps, n_rows);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    clear_step_graphs(h);                    // cached step graphs carry the old pointer in their kernel arguments
    h->moe_trace = trace_dev;
    h->moe_trace_steps = trace_dev ? n_steps : 0;
    h->moe_trace_rows = trace_dev ? n_rows : 0;
    return YMT3_OK;
}

extern "C" int ymt3_debug_decode_start(ymt3_handle h, int step0) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!h->debug_hooks) FAIL(YMT3_ERR_UNSUPPORTED, "debug hooks are accepted only by a handle created with YMT3_DEBUG_HOOKS=1 in the environment");
    if (step0 < 0 || step0 >= h->cfg.max_decode_len) FAIL(YMT3_ERR_ARG, "step0=%d outside [0, %d)", step0, h->cfg.max_decode_len);
    HIP_TRY(hipSetDevice(h->device));
    if (step0 > 0) {
        // positions [0, step0) of every (layer, row, head) slab: defined (zero) keys and values instead of whatever hipMalloc left
        const ymt3_config& k = h->cfg;
        const size_t slabs = (size_t)k.n_dec_layers * h->maxR * k.n_heads, pitch = (size_t)k.max_decode_len * 64 * sizeof(bf16_t);
        HIP_TRY(hipMemset2D(h->kcache, pitch, 0, (size_t)step0 * 64 * sizeof(bf16_t), slabs));
        HIP_TRY(hipMemset2D(h->vcache, pitch, 0, (size_t)step0 * 64 * sizeof(bf16_t), slabs));
        HIP_TRY(hipDeviceSynchronize());
    }
    h->prof_step0 = step0;
    return YMT3_OK;
}

// ------------------------------------------------------------------------------------------------
// Audio ingest.  Filter design on the host, in double: the Kaiser(5.0) windowed-sinc
// low-pass and the alignment of TP: scipy/signal/_signaltools.py resample_poly (restated in oracle/ingest_oracle.py).
static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= x / (2.0 * k);
        const double t2 = term * term;
        sum += t2;
        if (t2 < 1e-20 * sum) break;
    }
    return sum;
}

static long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

static int get_resampler(ymt3_ctx* c, int sr_in, const ymt3_ctx::Resampler** out) {
    const long long g = gcd_ll(sr_in, c->cfg.sample_rate);
    const int up = (int)(c->cfg.sample_rate / g), down = (int)(sr_in / g);
    auto it = c->resamplers.find({up, down});
    if (it != c->resamplers.end()) { *out = &it->second; return YMT3_OK; }
    const int max_rate = std::max(up, down);
    if (max_rate > 16384) FAIL(YMT3_ERR_UNSUPPORTED, "resampling ratio %d/%d needs a %d-tap filter; unsupported", up, down, 20 * max_rate + 1);
    ymt3_ctx::Resampler rs;
    rs.up = up; rs.down = down;
    std::vector<double> hp;
    if (up == 1 && down == 1) {
        hp.assign(1, 1.0);
        rs.r = 0;
    } else {
        const int half_len = 10 * max_rate, n = 2 * half_len + 1;
        const int n_pre_pad = down - half_len % down;
        rs.r = (half_len + n_pre_pad) / down;
        hp.assign((size_t)n_pre_pad + n, 0.0);
        const double fc = 1.0 / max_rate, i0b = bessel_i0(5.0), pi = 3.14159265358979323846;
        double sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const double m = (double)(i - half_len), xx = pi * fc * m;
            const double sinc = m == 0.0 ? 1.0 : std::sin(xx) / xx;
            const double rel = m / half_len;
            const double w = bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - rel * rel))) / i0b;
            hp[(size_t)n_pre_pad + i] = fc * sinc * w;
            sum += hp[(size_t)n_pre_pad + i];
        }
        for (int i = 0; i < n; ++i) hp[(size_t)n_pre_pad + i] *= (double)up / sum;
    }
    rs.J = (int)((hp.size() + up - 1) / up);
    rs.Jp = (rs.J + 3) / 4 * 4;
    rs.window = (int)((255LL * down) / up) + rs.J + 2;
    if ((size_t)rs.window * sizeof(float) > 64 * 1024) FAIL(YMT3_ERR_UNSUPPORTED, "resampling ratio %d/%d needs a %d-sample LDS window; unsupported", up, down, rs.window);
    std::vector<float> P((size_t)up * rs.Jp, 0.f);
    for (size_t i = 0; i < hp.size(); ++i) P[(i % up) * rs.Jp + i / up] = (float)hp[i];
    void* dev = nullptr;
    int rc = dev_alloc(c, &dev, P.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dev, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice));
    rs.taps = static_cast<float*>(dev);
    *out = &(c->resamplers[{up, down}] = rs);
    return YMT3_OK;
}

extern "C" int ymt3_ingest_plan(ymt3_handle h, int64_t n_frames, int sample_rate_in, int64_t* n_samples_out, int* n_segments) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (n_frames < 0 || sample_rate_in <= 0) FAIL(YMT3_ERR_ARG, "n_frames=%lld sample_rate_in=%d", (long long)n_frames, sample_rate_in);
    const long long g = gcd_ll(sample_rate_in, h->cfg.sample_rate);
    const long long up = h->cfg.sample_rate / g, down = sample_rate_in / g;
    const long long n_out = (n_frames * up + down - 1) / down;
    const long long S = h->cfg.segment_samples;
    const long long n_seg = std::max(1LL, (n_out + S - 1) / S);
    if (n_seg > 0x7fffffffLL) FAIL(YMT3_ERR_ARG, "too many segments");
    if (n_samples_out) *n_samples_out = n_out;
    if (n_segments) *n_segments = (int)n_seg;
    return YMT3_OK;
}

extern "C" int ymt3_ingest(ymt3_handle h, const void* pcm_dev, int pcm_format, int64_t n_frames, int n_channels,
                           int sample_rate_in, float* segments_dev, int n_segments, void* stream) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (pcm_format != YMT3_PCM_S16 && pcm_format != YMT3_PCM_F32) FAIL(YMT3_ERR_ARG, "pcm_format=%d", pcm_format);
    if (n_frames < 0 || n_channels < 1 || n_channels > 64 || sample_rate_in <= 0 || n_segments < 1)
        FAIL(YMT3_ERR_ARG, "n_frames=%lld n_channels=%d sample_rate_in=%d n_segments=%d", (long long)n_frames, n_channels, sample_rate_in, n_segments);
    if (!segments_dev || (n_frames > 0 && !pcm_dev)) FAIL(YMT3_ERR_ARG, "null buffer");
    int64_t n_out = 0;
    int need = 0;
    int rc = ymt3_ingest_plan(h, n_frames, sample_rate_in, &n_out, &need);
    if (rc) return rc;
    if (n_segments < need) FAIL(YMT3_ERR_ARG, "n_segments=%d but %lld resampled samples need %d", n_segments, (long long)n_out, need);
    HIP_TRY(hipSetDevice(h->device));
    const ymt3_ctx::Resampler* rs = nullptr;
    rc = get_resampler(h, sample_rate_in, &rs);
    if (rc) return rc;
    IngestArgs a{};
    a.pcm = pcm_dev; a.taps = rs->taps; a.out = segments_dev;
    a.n_in = n_frames; a.n_out = n_out; a.n_total = (long long)n_segments * h->cfg.segment_samples; a.r = rs->r;
    a.up = rs->up; a.down = rs->down; a.J = rs->J; a.Jp = rs->Jp; a.n_channels = n_channels; a.s16 = pcm_format == YMT3_PCM_S16; a.window = rs->window;
    LAUNCH(launch_ingest(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return YMT3_OK;
}

// ---------------------------------------------------------------- streaming ingest (include/ymt3.h)
// Output sample n reads input frames k0(n) - J + 1 .. k0(n), k0(n) = (n + r) * down / up, so with N frames arrived the samples with
// k0(n) <= N - 1 are final: n + r < ceil(N * up / down), i.e. the first max(0, ceil(N * up / down) - r) of them.
struct ymt3_ingest_stream_s {
    ymt3_ctx* owner;
    int device, sample_rate_in, n_channels, s16;
    long long max_chunk;
    ymt3_ctx::Resampler rs;                 // the taps belong to the handle
    float* hist = nullptr;                  // [hist_mask + 1] mono ring
    long long hist_mask = 0;
    float* part[2] = {nullptr, nullptr};    // [segment_samples] each: the partial segment, and the one the next completing push starts
    int cur = 0;
    long long n_in = 0, n_done = 0, delivered = 0;   // frames arrived, samples computed, segments handed to the caller
    bool finished = false;
};

static long long ingest_final(const ymt3_ingest_stream_s* s, long long n_in) {
    return std::max(0LL, (n_in * s->rs.up + s->rs.down - 1) / s->rs.down - s->rs.r);
}

extern "C" void ymt3_ingest_stream_destroy(ymt3_ingest_stream s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (void* p : {(void*)s->hist, (void*)s->part[0], (void*)s->part[1]})
        if (p) (void)hipFree(p);
    delete s;
}

extern "C" int ymt3_ingest_stream_create(ymt3_handle h, int sample_rate_in, int n_channels, int pcm_format, int64_t max_chunk_frames,
                                         ymt3_ingest_stream* out) {
    if (!out) FAIL(YMT3_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (pcm_format != YMT3_PCM_S16 && pcm_format != YMT3_PCM_F32) FAIL(YMT3_ERR_ARG, "pcm_format=%d", pcm_format);
    if (n_channels < 1 || n_channels > 64 || sample_rate_in <= 0) FAIL(YMT3_ERR_ARG, "n_channels=%d sample_rate_in=%d", n_channels, sample_rate_in);
    if (max_chunk_frames < 1 || max_chunk_frames > (1LL << 24)) FAIL(YMT3_ERR_ARG, "max_chunk_frames=%lld outside [1, 2^24]", (long long)max_chunk_frames);
    HIP_TRY(hipSetDevice(h->device));
    const ymt3_ctx::Resampler* rs = nullptr;
    int rc = get_resampler(h, sample_rate_in, &rs);
    if (rc) return rc;
    ymt3_ingest_stream s = new ymt3_ingest_stream_s{h, h->device, sample_rate_in, n_channels, pcm_format == YMT3_PCM_S16, (long long)max_chunk_frames, *rs};
    long long ring = 1;
    while (ring < rs->J - 1 + max_chunk_frames) ring <<= 1;
    s->hist_mask = ring - 1;
    const size_t seg = (size_t)h->cfg.segment_samples * sizeof(float);
    if (hipMalloc(reinterpret_cast<void**>(&s->hist), (size_t)ring * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&s->part[0]), seg) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&s->part[1]), seg) != hipSuccess) {
        ymt3_ingest_stream_destroy(s);
        FAIL(YMT3_ERR_HIP, "ingest stream buffers (%zu bytes) could not be allocated", (size_t)ring * sizeof(float) + 2 * seg);
    }
    *out = s;
    return YMT3_OK;
}

extern "C" int ymt3_ingest_stream_reset(ymt3_handle h, ymt3_ingest_stream s, void* stream) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!s) FAIL(YMT3_ERR_ARG, "null ingest stream");
    if (s->owner != h) FAIL(YMT3_ERR_ARG, "the ingest stream belongs to another handle");
    (void)stream;   // nothing on the device carries over: frames outside [0, n_in) are never read from the ring
    s->n_in = s->n_done = s->delivered = 0;
    s->cur = 0;
    s->finished = false;
    return YMT3_OK;
}

extern "C" int ymt3_ingest_stream_plan(ymt3_ingest_stream s, int64_t n_frames, int* n_ready) {
    if (!s) FAIL(YMT3_ERR_ARG, "null ingest stream");
    if (s->finished) FAIL(YMT3_ERR_ARG, "the stream has been finished: reset it first");
    if (n_frames < 0 || n_frames > s->max_chunk) FAIL(YMT3_ERR_ARG, "n_frames=%lld outside [0, max_chunk_frames=%lld]", (long long)n_frames, s->max_chunk);
    const long long ready = ingest_final(s, s->n_in + n_frames) / s->owner->cfg.segment_samples - s->delivered;
    if (ready > 0x7fffffffLL) FAIL(YMT3_ERR_ARG, "too many segments");
    if (n_ready) *n_ready = (int)ready;
    return YMT3_OK;
}

static IngestStreamArgs ingest_stream_args(const ymt3_ingest_stream_s* s) {
    IngestStreamArgs a{};
    a.hist = s->hist; a.hist_mask = s->hist_mask; a.taps = s->rs.taps; a.part_old = s->part[s->cur];
    a.n_done = s->n_done; a.n_row0 = s->delivered * s->owner->cfg.segment_samples; a.r = s->rs.r;
    a.up = s->rs.up; a.down = s->rs.down; a.J = s->rs.J; a.Jp = s->rs.Jp; a.n_channels = s->n_channels; a.s16 = s->s16; a.window = s->rs.window;
    return a;
}

extern "C" int ymt3_ingest_stream_push(ymt3_handle h, ymt3_ingest_stream s, const void* pcm_dev, int64_t n_frames, float* segments_dev,
                                       int max_segments, int* n_ready, void* stream) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!s) FAIL(YMT3_ERR_ARG, "null ingest stream");
    if (s->owner != h) FAIL(YMT3_ERR_ARG, "the ingest stream belongs to another handle");
    int ready = 0;
    int rc = ymt3_ingest_stream_plan(s, n_frames, &ready);
    if (rc) return rc;
    if (max_segments < ready) FAIL(YMT3_ERR_ARG, "max_segments=%d but this push completes %d segments", max_segments, ready);
    if ((n_frames > 0 && !pcm_dev) || (ready > 0 && !segments_dev)) FAIL(YMT3_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(h->device));
    const long long S = h->cfg.segment_samples, n_in = s->n_in + n_frames, n_final = ingest_final(s, n_in);
    IngestStreamArgs a = ingest_stream_args(s);
    a.pcm = pcm_dev; a.out = segments_dev; a.n_new = n_frames; a.n_in = n_in;
    a.n_end = a.n_total = n_final;
    a.n_row_end = a.n_row0 + ready * S;
    a.g0 = ready > 0 ? a.n_row0 : s->n_done;                 // a completed segment takes its first part from the partial buffer
    a.part_new = s->part[ready > 0 ? s->cur ^ 1 : s->cur];   // and the next partial segment starts in the other one
    LAUNCH(launch_ingest_stream(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    s->n_in = n_in; s->n_done = n_final; s->delivered += ready;
    if (ready > 0) s->cur ^= 1;
    if (n_ready) *n_ready = ready;
    return YMT3_OK;
}

extern "C" int ymt3_ingest_stream_finish(ymt3_handle h, ymt3_ingest_stream s, float* segments_dev, int max_segments, int* n_ready,
                                         int64_t* n_samples_total, void* stream) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (!s) FAIL(YMT3_ERR_ARG, "null ingest stream");
    if (s->owner != h) FAIL(YMT3_ERR_ARG, "the ingest stream belongs to another handle");
    if (s->finished) FAIL(YMT3_ERR_ARG, "the stream has been finished: reset it first");
    const long long S = h->cfg.segment_samples, n_out = (s->n_in * s->rs.up + s->rs.down - 1) / s->rs.down;
    const long long n_seg = std::max(1LL, (n_out + S - 1) / S), ready = n_seg - s->delivered;
    if (max_segments < ready) FAIL(YMT3_ERR_ARG, "max_segments=%d but the finish completes %lld segments", max_segments, ready);
    if (ready > 0 && !segments_dev) FAIL(YMT3_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(h->device));
    IngestStreamArgs a = ingest_stream_args(s);
    a.out = segments_dev; a.n_new = 0; a.n_in = s->n_in;
    a.n_end = n_out; a.n_total = a.n_row_end = n_seg * S;    // frames that never came are zeros, as the one-shot call pads
    a.g0 = a.n_row0;
    a.part_new = s->part[s->cur];                            // not written: every sample lies in the caller's rows
    LAUNCH(launch_ingest_stream(a, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    s->n_done = n_out; s->delivered = n_seg; s->finished = true;
    if (n_ready) *n_ready = (int)ready;
    if (n_samples_total) *n_samples_total = n_out;
    return YMT3_OK;
}

extern "C" int ymt3_last_decode_steps(ymt3_handle h) { return h ? h->last_steps : 0; }

extern "C" int ymt3_merged_fallbacks(ymt3_handle h) { return h ? h->fallback_count : 0; }
extern "C" int ymt3_last_decode_chains(ymt3_handle h) { return h ? h->last_chains : 0; }

extern "C" int ymt3_set_abort_recovery(ymt3_handle h, int mode) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (mode != 0 && mode != 1) FAIL(YMT3_ERR_ARG, "mode must be 0 (asynchronous, lazy) or 1 (verify every merged decode call)");
    h->abort_recovery = mode;
    return YMT3_OK;
}

extern "C" int ymt3_set_early_stop(ymt3_handle h, int interval) {
    if (!h) FAIL(YMT3_ERR_ARG, "null handle");
    if (interval < 0) FAIL(YMT3_ERR_ARG, "interval must be >= 0");
    HIP_TRY(hipSetDevice(h->device));
    if (interval > 0 && !h->host_flag) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->host_flag), sizeof(int), hipHostMallocDefault));
    h->early_stop_interval = interval;
    return YMT3_OK;
}
