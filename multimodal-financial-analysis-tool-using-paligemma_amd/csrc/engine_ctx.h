// engine_ctx.h -- what the engine_*.hip files of libpgmi's host side share: the error path, the weight table and
// the context struct, the small helpers that read them, and the declarations of the internal functions that cross
// files (namespace pgmi_eng, hidden: the library exports the C ABI of include/pgmi.h and the launchers alone).
//
//   engine_weights.hip     create / destroy, slab layout, loading, pgmi_prepare, the RCCL broadcast
//   engine_images.hip      the fragment-major and 13-bit weight images of the decode step
//   engine_lora.hip        LoRA adapters
//   engine_prefill.hip     vision tower, projector, language-model forward, lm_head, log-probabilities
//   engine_decode.hip      the decode step and its entry points, argmax, eos, sampling
//   engine_host_rules.hip  the host-only rules (logit processors, beam search)
//   engine_debug.hip       stage and buffer hooks, tuning calls, single ops
//   engine_graph.h         the graph caches and the replay contract
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pgmi.h"
#include "common.h"
#include "launch.h"
#include "lora.h"
#include "pack13.h"

using namespace pgmi;

namespace pgmi_eng __attribute__((visibility("hidden"))) {

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// a launcher's own refusal (launch_error_set): reported like a failed launch
inline int launcher_error() {
    const char* what = "";
    const hipError_t e = pgmi::launch_error_take(&what);
    if (e == hipSuccess) return 0;
    return fail(PGMI_E_HIP, std::string("kernel launch: ") + what + ": " + hipGetErrorString(e));
}

}  // namespace pgmi_eng

using namespace pgmi_eng;

// Prefill (vision tower, projector, language-model forward) runs at most this many images / sequences per pass: a
// larger batch goes through as row groups, each at a GEMM shape whose plans were measured (M = 8 x 256 / 288 rows),
// inside the 64 MiB split-K workspace, and with results that do not depend on the batch the group came in.
constexpr int kPrefillGroup = 8;

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(PGMI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define LAUNCHCHK()                                                                        \
    do {                                                                                   \
        if (int r_ = launcher_error()) return r_;                                          \
        hipError_t e_ = hipGetLastError();                                                 \
        if (e_ != hipSuccess) return fail(PGMI_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

struct Slot {
    std::string name;
    int64_t off;
    int64_t shape[4];
    int ndim;
    int64_t numel;
};

// Captured hipGraphs of one kind of call, keyed by every pointer and size the captured body reads (so a replay
// is that call).  Bounded: see run_graphed.  The struct is here because pgmi_ctx holds two of them; everything
// that fills or empties one is in engine_graph.h.
struct GraphCache {
    std::map<std::vector<intptr_t>, hipGraphExec_t> map;  // null: the key was seen once (run eagerly), no graph yet
    void clear();  // engine_graph.h
};

// Weight pointers into the bound slab, resolved once by pgmi_bind_weights (bind_tables); fused projections
// (q|k|v, gate|up) are named by their first tensor, the others follow it in the slab (build_layout).
struct VisionLayerW {
    const uint16_t *qkv_w, *qkv_b, *out_w, *out_b, *ln1_w, *ln1_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ln2_w, *ln2_b;
};
struct TextLayerW {
    const uint16_t *qkv, *o, *gate_up, *down, *in_norm, *post_norm;
    // batched decode (B >= 3): this layer's fragment-major images (ensure_mf_image), null while the image is absent
    const uint16_t *mf_gate_up = nullptr, *mf_qkv = nullptr, *mf_o = nullptr, *mf_down = nullptr;
    // the 13-bit images of gate|up and down by form (PkForm: row-major segments for B <= 2, fragment-major ones for
    // B >= 3; ensure_pk_image), img null while absent or raw
    PkW pk_gate_up[2], pk_down[2];
};
struct WeightTable {
    const uint16_t *patch_conv_w, *patch_b, *pos_emb, *post_ln_w, *post_ln_b, *proj_w, *proj_b, *embed, *final_norm;
    std::vector<VisionLayerW> v;
    std::vector<TextLayerW> t;
    // the tied embedding's 13-bit images as lm_head reads them, by form (the raw rows stay for look-up and prefill;
    // the fragment-major form's rows are padded to a whole 16-row group)
    PkW pk_embed[2];
};

// The 13-bit images (pack13.h) of one form: every layer's gate|up and down rows and the tied embedding, one buffer per
// kind (PK_GATE_UP, PK_DOWN, PK_LM_HEAD); built by ensure_pk_image, read through w.t[i].pk_*[form] / w.pk_embed[form].
// mask: the kinds a step of that form reads packed (row form: pgmi_set_decode_packed, < 0 the per-batch default,
// pk_mask_for; fragment form: pgmi_set_decode_packed_batched, never negative); done: the kinds scanned (and packed,
// where they fit) or given up since the last pgmi_prepare; alloc_failed: a kind's buffer could not be allocated
struct PkImages {
    uint8_t* buf[3];
    int mask, done;
    bool alloc_failed;
};

// weight kinds with a 13-bit image (bits of pgmi_set_decode_packed's mask)
enum { PK_GATE_UP = 1, PK_DOWN = 2, PK_LM_HEAD = 4, PK_ALL = 7 };
// the default: the kinds whose kernel measured faster packed, per batch (at B = 2 gate|up and
// down are VALU-limited and lose 4 %, lm_head still gains 8 %)
constexpr int kPkDefaultB1 = PK_ALL, kPkDefaultB2 = PK_LM_HEAD;

// LoRA adapters (pgmi_lora_*): an adapter is a list of targets, each a slab weight with its resident fp32 factors
struct LoraTarget {
    int slot;        // index into pgmi_ctx::slots: a 2-D Linear weight [N][K]
    int r;
    float scaling;
    float *A, *B;    // device fp32 [r][K], [N][r]
};
struct LoraAdapter {
    bool used = false;
    std::vector<LoraTarget> targets;
    int64_t factor_bytes = 0;
};
// the pristine (base) copy of a slab weight some adapter was merged into; valid: it holds the base as of now
struct LoraPristine {
    uint16_t* copy = nullptr;
    bool valid = false;
};

struct pgmi_ctx {
    pgmi_config c;
    int device;
    std::vector<Slot> slots;
    std::unordered_map<std::string, int> index;
    int64_t slab_bytes = 0;
    uint8_t* slab = nullptr;
    WeightTable w;
    std::vector<float> inv_freq;
    std::vector<uint16_t> host_cos, host_sin;  // optional exact table
    bool prepared = false;
    std::vector<void*> allocs;
    // derived
    uint16_t* patch_w = nullptr;  // [v_hidden][kpad]
    int kpad = 0;
    uint16_t* cosT = nullptr;
    uint16_t* sinT = nullptr;
    // text prefill workspace (Hs, Tn, dpos, dids_tmp: max_batch*max_seq rows; the per-layer scratch QKV, Qr, AO, ACT:
    // one prefill group's, min(max_batch, 8)*max_seq rows)
    uint16_t *Hs, *Tn, *QKV, *Qr, *AO, *ACT, *lastrows;
    long tn_rows = 0;  // rows of Tn holding the final RMSNorm of the last pgmi_lm_forward (pgmi_lm_final_hidden)
    int64_t* dpos;
    int64_t* dids_tmp;
    // vision workspace (one prefill group's rows: min(max_batch, 8)*N)
    uint16_t *vX, *vT, *vQKV, *vAO, *vH, *vP;
    float* ws;
    size_t ws_bytes;
    // decode workspace
    uint16_t *dH, *dQ, *dAO, *dACT;
    uint16_t* dHn;  // batched decode (B >= 3): the RMSNorm'd rows the unstaged MFMA projections read
    float* dSS;     // batched decode: o_proj's 16-column partial sums of squares of h, [B][H / 16]
    // batched decode (max_batch >= 3): fragment-major images of every layer's gate|up, q|k|v (in the GEMV's row
    // order), o_proj and down weights (mf_swizzle); laid out by ensure_mf_image, read through w.t[i].mf_*
    uint16_t* mfw = nullptr;
    bool mfw_dirty = false;  // the fragment-major images are (re)built by the next batched decode step
    bool mfw_alloc_failed = false;  // their allocation failed: the batched decode reads the row-major weights
    // the 13-bit images by form: [PK_FORM_ROWS] decode at B <= 2 (default mask: per batch), [PK_FORM_FRAG] batched
    // decode at B >= 3 (default: none; with every kind on up to 3.80 GB beside mfw at the 3B shapes).  pk_stat: the
    // scan results of a build, shared
    PkImages pk[2] = {{{nullptr, nullptr, nullptr}, -1, 0, false}, {{nullptr, nullptr, nullptr}, 0, 0, false}};
    unsigned* pk_stat = nullptr;
    float *opart, *pmax, *dlogits, *amax_v;
    int *pidx, *amax_i;
    int max_chunks;
    StepState* step;
    StepState* pstep;  // the generate-loop prefill's last-row attention (flash-decoding over the prompt's keys)
    StepState* rstep;  // the ragged step's records, one per batch row ([max_batch], pgmi_decode_ragged)
    int* d_rlens;      // ragged prefill: [0, 16) each row's token count, [16, 32) its attended key count;
                       // prefix prefill: [16, 32) as well (lock-step rows: kv_start + L), [32, 48) its prefix length
    int64_t* d_ids;
    uint16_t* d_emb;             // staged input rows of pgmi_decode_embeds ([max_batch][hidden] bf16)
    float* d_mask;               // staged additive decode mask ([max_batch][max_kv] fp32, pgmi_decode_embeds_dev)
    float* d_zero;               // one zero word: the "no mask" mask of the decode attention
    int64_t* d_next;             // argmax target when the caller passes none
    unsigned* lm_done;           // lm_head arrival counter (argmax folded into its last workgroup)
    hipStream_t cap_stream = nullptr;
    // prefill graphs (vision tower, language-model forward) and decode graphs (the captured steps): replayed
    // for repeated calls with identical pointer/shape arguments (a replay is the eager call: kernels read the
    // same addresses at run time), captured on the second such call (run_graphed)
    GraphCache pgraphs, dgraphs;
    bool prefill_graph = true;
    int mf_staged = -1;  // batched decode RMSNorm form (mf_staged()); -1 = default (unstaged)
    // device step state as the last enqueued per-phase decode step leaves it (advanced in-graph)
    bool step_known = false;
    int step_kv = 0, step_pos = 0;
    // the same for the ragged step's per-row records (rows [0, rstep_B))
    bool rstep_known = false;
    int rstep_B = 0;
    int rstep_kv[kMaxRows] = {0}, rstep_pos[kMaxRows] = {0};
    // in-situ timing probe of the prefill MLP GEMMs (pgmi_prefill_probe): events around layer i's gate|up
    // GEMM (ev[4i], ev[4i+1]) and down GEMM (ev[4i+2], ev[4i+3]) of eager forwards
    std::vector<hipEvent_t> probe_ev;
    bool probe_on = false;
    bool graph_before_probe = true;  // prefill_graph as the caller left it before the probe turned it off
    // LoRA: the adapters, the one merged into the slab now (-1: none, the slab holds the base) and the pristine
    // copies by slot (allocated at the first activation that needs them, owned here, not in `allocs`)
    LoraAdapter lora[PGMI_LORA_MAX];
    int lora_active = -1;
    std::map<int, LoraPristine> lora_pristine;
};

namespace pgmi_eng __attribute__((visibility("hidden"))) {

// the form a B-row step's GEMVs read: row-major segments (the streaming forms) or fragment-major ones (the MFMA forms)
inline PkForm pk_form_of(int B) { return B >= gemv_mf_min_batch() ? PK_FORM_FRAG : PK_FORM_ROWS; }

// the kinds a B-row step reads packed: the caller's mask for B's form, or (row form) the measured default of that
// batch size
inline int pk_mask_for(const pgmi_ctx* x, int B) {
    const int mask = x->pk[pk_form_of(B)].mask;
    return mask >= 0 ? mask : B <= 1 ? kPkDefaultB1 : kPkDefaultB2;
}

// the image a B-row decode GEMV of `kind` reads now: w[form of B], or none (the bf16 weights) while the kind is
// switched off for that batch, not built since the last pgmi_prepare, or the tensor did not fit (img null).
inline PkW pk_use(const pgmi_ctx* x, int B, int kind, const PkW (&w)[2]) {
    const PkForm f = pk_form_of(B);
    return (pk_mask_for(x, B) & x->pk[f].done & kind) ? w[f] : PkW{};
}
// the same for a caller with no batched packed form: the prefill's last-row GEMVs (lm_last_row_tail, lm_logits),
// which at B >= 3 launch the bf16 weights whatever the fragment form's state (its changes do not drop their graphs)
inline PkW pk_use_rows(const pgmi_ctx* x, int B, int kind, const PkW (&w)[2]) {
    return pk_form_of(B) == PK_FORM_ROWS ? pk_use(x, B, kind, w) : PkW{};
}

// does this context's batched decode (B >= 3) read fragment-major images at all
inline bool mf_wanted(const pgmi_config& c) {
    return c.max_batch >= gemv_mf_min_batch() && c.t_intermediate % 32 == 0 && c.t_hidden % 32 == 0;
}

inline int n_img(const pgmi_config& c) { return (c.v_image / c.v_patch) * (c.v_image / c.v_patch); }

inline uint16_t host_f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

inline float bf16_round_host(float f) {
    uint32_t u = (uint32_t)host_f2bf(f) << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

inline float embed_normalizer(const pgmi_ctx* x) { return bf16_round_host(std::sqrt((float)x->c.t_hidden)); }

// One prefill row group's launches, shared by lm_rows and the stage hook (pgmi_debug_prefill_stage): what the
// stages read besides the context.  A group's rows of Hs / Tn / lastrows, its positions, lengths, KV rows and
// logits are its slice of the batch's (b0); QKV, Qr, AO, ACT and the split-K workspace are scratch the groups share.
struct PrefillRun {
    hipStream_t s;
    int b0, B, L;            // the group's first batch row, its rows, the slots of a row
    void* kv;
    int kv_batch, kv_max, kv_start;
    float* logits;           // the batch's logits (lm_logits takes the group's slice)
    int logits_rows;
    bool ragged;
    bool prefix = false;     // a prefix-LM call with at least one row whose prefix is shorter than the row
};

// One decode step's launches, shared by decode_body and the stage hook (pgmi_debug_decode_stage): what the
// head, each layer and the tail read besides the context.
struct DecodeRun {
    hipStream_t s;
    const int64_t* ids;      // token ids (null: h is given -- embeds, or the hook's caller wrote dH)
    const uint16_t* embeds;  // given input rows (pgmi_decode_embeds), else null
    int B;
    void* kv;
    int kv_batch, kv_max;
    int launch_keys;         // upper bound on kv_len + 1 (sizes the attention grid)
    int masked;              // 0: no mask, 1: staged bf16 mask, 2: staged fp32 mask
    bool ragged;             // one step record per row (x->rstep), else x->step
};

inline const char* const kLoraActiveMsg =
    "a LoRA adapter is merged into the weights: deactivate first (pgmi_lora_set(ctx, -1))";

// engine_weights.hip
int ensure_prepared(pgmi_ctx* x);
// engine_images.hip
void pk_forget(pgmi_ctx* x);
void pk_forget_kinds(pgmi_ctx* x, int kinds);
int ensure_mf_image(pgmi_ctx* x, hipStream_t s);
int ensure_pk_image(pgmi_ctx* x, hipStream_t s, int B);      // the 13-bit images of B's form
int ensure_decode_images(pgmi_ctx* x, hipStream_t s, int B);  // what a B-row decode step reads: mfw, then those
// engine_lora.hip
void lora_forget_pristine(pgmi_ctx* x);
// engine_prefill.hip: what a prefill does before its launches, then the stages of one row group (PrefillRun) --
// lm_rows' order, and the stage numbers of pgmi_debug_prefill_stage
int lm_begin(pgmi_ctx* x, const int64_t* ids, const void* embeds, int B, int L, const int64_t* positions,
             const int32_t* lens, bool ragged, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
             int* logits_rows_io, void* stream);
void lm_entry(const pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
              const void* embeds, int B, int L, bool ragged);
bool run_last_only(const pgmi_ctx* x, const PrefillRun& r);
void lm_in_norm(const pgmi_ctx* x, const PrefillRun& r);
void lm_qkv(const pgmi_ctx* x, const PrefillRun& r, int i);
void lm_attn(const pgmi_ctx* x, const PrefillRun& r, int i);
// the prefix form's row values to the device (d_rlens segments 2 and 3), outside any graph
void set_prefix_rows(const pgmi_ctx* x, hipStream_t s, const RowInts& klen, const RowInts& pfx, int B);
// the attention launcher of lm_attn: a with the group's key counts (ragged or causal) and prefix lengths (causal)
void lm_attn_launch(const pgmi_ctx* x, hipStream_t s, AttnArgs a, int b0, int kv_start, bool ragged, bool causal);
void lm_o_proj(const pgmi_ctx* x, const PrefillRun& r, int i);
void lm_gate_up(const pgmi_ctx* x, const PrefillRun& r, int i);
void lm_down(const pgmi_ctx* x, const PrefillRun& r, int i);
int lm_last_row_tail(const pgmi_ctx* x, const PrefillRun& r, int i);
int lm_logits(const pgmi_ctx* x, const PrefillRun& r);
int lm_logprobs_run(pgmi_ctx* x, const void* normed, const uint16_t* W, int rows, int V, int K, const int64_t* labels,
                    int64_t ignore_index, float* logprob, float* lse, void* stream);
// engine_decode.hip: the parts of one decode step (DecodeRun)
void decode_head(const pgmi_ctx* x, const DecodeRun& r);
void decode_layer(const pgmi_ctx* x, const DecodeRun& r, int i, int stage = 0);
void decode_tail(const pgmi_ctx* x, const DecodeRun& r, float* logits, int64_t* next_ids, int64_t* hist);

}  // namespace pgmi_eng
