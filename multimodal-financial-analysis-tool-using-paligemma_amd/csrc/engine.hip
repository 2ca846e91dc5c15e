// engine.hip -- libpgmi host side: weight layout, workspaces, forward orchestration, hipGraph
// decode, and the extern "C" ABI declared in include/pgmi.h.
//
// Orchestration restates the reference's call stacks:
//   vision   SiglipVisionTransformer.forward   modeling_siglip.py:236-244
//   lm       GemmaModel/GemmaForCausalLM        modeling_gemma.py:357-427
//   decode   one inference.py loop iteration    inference.py:56-78
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

#include <dlfcn.h>

#include <rccl/rccl.h>  // types only: librccl is dlopen'ed on first use

#include "../../include/pgmi.h"
#include "beam_rule.h"
#include "common.h"
#include "launch.h"
#include "logits_rule.h"
#include "lora.h"
#include "pack13.h"
#include "safetensors_hdr.h"

using namespace pgmi;

static thread_local std::string g_err;

// Prefill (vision tower, projector, language-model forward) runs at most this many images / sequences per pass: a
// larger batch goes through as row groups, each at a GEMM shape whose plans were measured (M = 8 x 256 / 288 rows),
// inside the 64 MiB split-K workspace, and with results that do not depend on the batch the group came in.
constexpr int kPrefillGroup = 8;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(PGMI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// a launcher's own refusal (launch_error_set): reported like a failed launch
static int launcher_error() {
    const char* what = "";
    const hipError_t e = pgmi::launch_error_take(&what);
    if (e == hipSuccess) return 0;
    return fail(PGMI_E_HIP, std::string("kernel launch: ") + what + ": " + hipGetErrorString(e));
}

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
// is that call).  Bounded: see run_graphed.
struct GraphCache {
    std::map<std::vector<intptr_t>, hipGraphExec_t> map;  // null: the key was seen once (run eagerly), no graph yet
    void clear() {
        for (auto& kv : map)
            if (kv.second) (void)hipGraphExecDestroy(kv.second);
        map.clear();
    }
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
    // decode at B <= 2: the 13-bit images of gate|up and down (ensure_pk_image), img null while absent or raw
    PkW pk_gate_up, pk_down;
};
struct WeightTable {
    const uint16_t *patch_conv_w, *patch_b, *pos_emb, *post_ln_w, *post_ln_b, *proj_w, *proj_b, *embed, *final_norm;
    std::vector<VisionLayerW> v;
    std::vector<TextLayerW> t;
    PkW pk_embed;  // the tied embedding's 13-bit image as lm_head reads it (the raw rows stay for look-up and prefill)
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
    // decode at B <= 2: 13-bit images (pack13.h) of every layer's gate|up and down rows and of the tied embedding,
    // one buffer per kind (PK_GATE_UP, PK_DOWN, PK_LM_HEAD); built by ensure_pk_image, read through w.t[i].pk_* /
    // w.pk_embed.  pk_mask: the kinds the step reads packed (pgmi_set_decode_packed; < 0: the per-batch default,
    // pk_mask_for); pk_done: the kinds scanned (and packed, where they fit) or given up since the last pgmi_prepare
    uint8_t* pk_buf[3] = {nullptr, nullptr, nullptr};
    unsigned* pk_stat = nullptr;
    int pk_mask = -1, pk_done = 0;
    bool pk_alloc_failed = false;
    float *opart, *pmax, *dlogits, *amax_v;
    int *pidx, *amax_i;
    int max_chunks;
    StepState* step;
    StepState* pstep;  // the generate-loop prefill's last-row attention (flash-decoding over the prompt's keys)
    StepState* rstep;  // the ragged step's records, one per batch row ([max_batch], pgmi_decode_ragged)
    int* d_rlens;      // ragged prefill: [0, 16) each row's token count, [16, 32) its attended key count
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

namespace {

// the kinds a B-row step reads packed: the caller's mask, or the measured default of that batch size
int pk_mask_for(const pgmi_ctx* x, int B) {
    return x->pk_mask >= 0 ? x->pk_mask : B <= 1 ? kPkDefaultB1 : kPkDefaultB2;
}

// the image a B-row streaming GEMV of `kind` reads now: w, or none (the bf16 rows) while the kind is switched
// off, not built since the last pgmi_prepare, or the tensor did not fit (w.img null)
PkW pk_use(const pgmi_ctx* x, int B, int kind, const PkW& w) {
    const bool on = B <= 2 && B < gemv_mf_min_batch() && (pk_mask_for(x, B) & x->pk_done & kind);
    return on ? w : PkW{};
}

// the weights changed (pgmi_prepare, a new slab): no image is valid until ensure_pk_image has rebuilt it
void pk_forget(pgmi_ctx* x) {
    x->pk_done = 0;
    x->pk_alloc_failed = false;
    x->w.pk_embed = PkW{};
    for (auto& t : x->w.t) t.pk_gate_up = t.pk_down = PkW{};
}

// forget the 13-bit images of the kinds in `kinds` alone (their tensors changed): the next B <= 2 step rescans
// and repacks those, the other kinds' images stay
void pk_forget_kinds(pgmi_ctx* x, int kinds) {
    x->pk_done &= ~kinds;
    for (auto& t : x->w.t) {
        if (kinds & PK_GATE_UP) t.pk_gate_up = PkW{};
        if (kinds & PK_DOWN) t.pk_down = PkW{};
    }
    if (kinds & PK_LM_HEAD) x->w.pk_embed = PkW{};
}

// does this context's batched decode (B >= 3) read fragment-major images at all
bool mf_wanted(const pgmi_config& c) {
    return c.max_batch >= gemv_mf_min_batch() && c.t_intermediate % 32 == 0 && c.t_hidden % 32 == 0;
}

bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = std::strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// a LoRA target: the 2-D weight of a Linear module (not an embedding, the patch convolution, a norm or a bias)
bool lora_targetable(const Slot& s) {
    if (s.ndim != 2) return false;
    for (const char* m : {"q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "out_proj.weight",
                          "gate_proj.weight", "up_proj.weight", "down_proj.weight", "mlp.fc1.weight", "mlp.fc2.weight",
                          "multi_modal_projector.linear.weight"})
        if (ends_with(s.name, m)) return true;
    return false;
}

void lora_forget_pristine(pgmi_ctx* x) {
    for (auto& kv : x->lora_pristine) kv.second.valid = false;
}

const char* kLoraActiveMsg = "a LoRA adapter is merged into the weights: deactivate first (pgmi_lora_set(ctx, -1))";

int n_img(const pgmi_config& c) { return (c.v_image / c.v_patch) * (c.v_image / c.v_patch); }

void add_slot(pgmi_ctx* x, const std::string& name, std::initializer_list<int64_t> shape) {
    Slot s;
    s.name = name;
    s.ndim = (int)shape.size();
    s.numel = 1;
    int i = 0;
    for (int64_t d : shape) { s.shape[i++] = d; s.numel *= d; }
    for (; i < 4; ++i) s.shape[i] = 1;
    s.off = x->slab_bytes;
    x->slab_bytes += (s.numel * 2 + 255) / 256 * 256;
    x->index[name] = (int)x->slots.size();
    x->slots.push_back(s);
}

// Slab layout: the reference state-dict tensors, ordered so that the projections that are
// fused into one GEMM/GEMV are adjacent (q|k|v weights and biases, gate|up).
void build_layout(pgmi_ctx* x) {
    const pgmi_config& c = x->c;
    const int64_t D = c.v_hidden, I = c.v_intermediate, P = c.v_patch, C = c.v_channels, N = n_img(c);
    const std::string vp = "vision_tower.vision_model.";
    add_slot(x, vp + "embeddings.patch_embedding.weight", {D, C, P, P});
    add_slot(x, vp + "embeddings.patch_embedding.bias", {D});
    add_slot(x, vp + "embeddings.position_embedding.weight", {N, D});
    for (int i = 0; i < c.v_layers; ++i) {
        const std::string lp = vp + "encoder.layers." + std::to_string(i) + ".";
        for (const char* nm : {"q_proj", "k_proj", "v_proj"}) add_slot(x, lp + "self_attn." + nm + ".weight", {D, D});
        for (const char* nm : {"q_proj", "k_proj", "v_proj"}) add_slot(x, lp + "self_attn." + nm + ".bias", {D});
        add_slot(x, lp + "self_attn.out_proj.weight", {D, D});
        add_slot(x, lp + "self_attn.out_proj.bias", {D});
        add_slot(x, lp + "layer_norm1.weight", {D});
        add_slot(x, lp + "layer_norm1.bias", {D});
        add_slot(x, lp + "mlp.fc1.weight", {I, D});
        add_slot(x, lp + "mlp.fc1.bias", {I});
        add_slot(x, lp + "mlp.fc2.weight", {D, I});
        add_slot(x, lp + "mlp.fc2.bias", {D});
        add_slot(x, lp + "layer_norm2.weight", {D});
        add_slot(x, lp + "layer_norm2.bias", {D});
    }
    add_slot(x, vp + "post_layernorm.weight", {D});
    add_slot(x, vp + "post_layernorm.bias", {D});
    add_slot(x, "multi_modal_projector.linear.weight", {c.projection_dim, D});
    add_slot(x, "multi_modal_projector.linear.bias", {c.projection_dim});
    const int64_t H = c.t_hidden, TI = c.t_intermediate, V = c.t_vocab, HD = c.t_head_dim;
    add_slot(x, "language_model.model.embed_tokens.weight", {V, H});
    for (int i = 0; i < c.t_layers; ++i) {
        const std::string lp = "language_model.model.layers." + std::to_string(i) + ".";
        add_slot(x, lp + "self_attn.q_proj.weight", {c.t_heads * HD, H});
        add_slot(x, lp + "self_attn.k_proj.weight", {c.t_kv_heads * HD, H});
        add_slot(x, lp + "self_attn.v_proj.weight", {c.t_kv_heads * HD, H});
        add_slot(x, lp + "self_attn.o_proj.weight", {H, c.t_heads * HD});
        add_slot(x, lp + "mlp.gate_proj.weight", {TI, H});
        add_slot(x, lp + "mlp.up_proj.weight", {TI, H});
        add_slot(x, lp + "mlp.down_proj.weight", {H, TI});
        add_slot(x, lp + "input_layernorm.weight", {H});
        add_slot(x, lp + "post_attention_layernorm.weight", {H});
    }
    add_slot(x, "language_model.model.norm.weight", {H});
}

// Resolve every weight the forward passes read, once per bound slab: a name without a slot is an error here,
// not a null kernel argument later.
int bind_tables(pgmi_ctx* x) {
    std::string missing;
    auto W = [&](const std::string& name) -> const uint16_t* {
        auto it = x->index.find(name);
        if (it == x->index.end()) {
            if (missing.empty()) missing = name;
            return nullptr;
        }
        return reinterpret_cast<const uint16_t*>(x->slab + x->slots[it->second].off);
    };
    WeightTable& w = x->w;
    const std::string vp = "vision_tower.vision_model.", tp = "language_model.model.";
    w.patch_conv_w = W(vp + "embeddings.patch_embedding.weight");
    w.patch_b = W(vp + "embeddings.patch_embedding.bias");
    w.pos_emb = W(vp + "embeddings.position_embedding.weight");
    w.post_ln_w = W(vp + "post_layernorm.weight");
    w.post_ln_b = W(vp + "post_layernorm.bias");
    w.proj_w = W("multi_modal_projector.linear.weight");
    w.proj_b = W("multi_modal_projector.linear.bias");
    w.embed = W(tp + "embed_tokens.weight");
    w.final_norm = W(tp + "norm.weight");
    w.v.resize(x->c.v_layers);
    for (int i = 0; i < x->c.v_layers; ++i) {
        const std::string lp = vp + "encoder.layers." + std::to_string(i) + ".";
        w.v[i] = {W(lp + "self_attn.q_proj.weight"), W(lp + "self_attn.q_proj.bias"),  // q|k|v adjacent
                  W(lp + "self_attn.out_proj.weight"), W(lp + "self_attn.out_proj.bias"),
                  W(lp + "layer_norm1.weight"), W(lp + "layer_norm1.bias"), W(lp + "mlp.fc1.weight"),
                  W(lp + "mlp.fc1.bias"), W(lp + "mlp.fc2.weight"), W(lp + "mlp.fc2.bias"),
                  W(lp + "layer_norm2.weight"), W(lp + "layer_norm2.bias")};
    }
    w.t.resize(x->c.t_layers);  // (keeps a built fragment-major image's pointers)
    for (int i = 0; i < x->c.t_layers; ++i) {
        const std::string lp = tp + "layers." + std::to_string(i) + ".";
        TextLayerW& t = w.t[i];
        t.qkv = W(lp + "self_attn.q_proj.weight");  // q|k|v adjacent
        t.o = W(lp + "self_attn.o_proj.weight");
        t.gate_up = W(lp + "mlp.gate_proj.weight");  // gate rows, then up rows
        t.down = W(lp + "mlp.down_proj.weight");
        t.in_norm = W(lp + "input_layernorm.weight");
        t.post_norm = W(lp + "post_attention_layernorm.weight");
    }
    if (!missing.empty()) return fail(PGMI_E_STATE, "weight layout has no tensor named " + missing);
    return 0;
}

uint16_t host_f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

float bf16_round_host(float f) {
    uint32_t u = (uint32_t)host_f2bf(f) << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

uint64_t fnv1a(const char* s) {
    uint64_t h = 0xCBF29CE484222325ULL;
    for (const unsigned char* p = (const unsigned char*)s; *p; ++p) { h ^= *p; h *= 0x100000001B3ULL; }
    return h;
}

uint64_t splitmix64_h(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__global__ void k_convert(const void* src, int dtype, long n, uint16_t* dst) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (dtype == PGMI_DTYPE_F32) dst[i] = f2bf(reinterpret_cast<const float*>(src)[i]);
        else dst[i] = f2bf((float)reinterpret_cast<const _Float16*>(src)[i]);
    }
}

int dalloc(pgmi_ctx* x, void** p, size_t bytes) {
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(PGMI_E_NOMEM, std::string("hipMalloc ") + std::to_string(bytes) + ": " + hipGetErrorString(e));
    x->allocs.push_back(*p);
    return 0;
}

template <typename T>
int dalloc_t(pgmi_ctx* x, T** p, size_t count) {
    return dalloc(x, reinterpret_cast<void**>(p), count * sizeof(T));
}

// RoPE tables: freqs = fp32(pos * inv_freq) (modeling_gemma.py:178), cos/sin in fp32 (:182-183),
// cast to bf16 (:185).  cos/sin of the fp32 angle are evaluated in double and rounded once.
void build_rope_host(pgmi_ctx* x, std::vector<uint16_t>& cs, std::vector<uint16_t>& sn) {
    const int half = x->c.t_head_dim / 2, mp = x->c.t_max_pos;
    cs.resize((size_t)mp * half);
    sn.resize((size_t)mp * half);
    for (int p = 0; p < mp; ++p)
        for (int i = 0; i < half; ++i) {
            const float ang = (float)p * x->inv_freq[i];
            cs[(size_t)p * half + i] = host_f2bf((float)std::cos((double)ang));
            sn[(size_t)p * half + i] = host_f2bf((float)std::sin((double)ang));
        }
}

int ensure_prepared(pgmi_ctx* x) {
    // the entry of every compute call: a launcher error that an earlier call on this thread left untaken (a path
    // without a launch check) is that call's, not this one's
    (void)pgmi::launch_error_take(nullptr);
    if (!x->prepared) return fail(PGMI_E_STATE, "pgmi_prepare() has not been called");
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound (pgmi_bind_weights)");
    return 0;
}

// The one graph policy: the first call with a key runs body(s) eagerly (kernel attributes are set on first launch),
// the second captures body(cap_stream), instantiates and launches, later ones replay.  A key that would be entry
// PGMI_GRAPH_CACHE_MAX + 1 drops the whole cache first (fresh buffers every call must not grow it without bound).
// sync_before_capture: the decode step's hipStreamSynchronize(s); the prefill has none (pgmi_vision may be called
// where a synchronise is not allowed).
template <class F>
int run_graphed(pgmi_ctx* x, GraphCache& gc, hipStream_t s, const std::vector<intptr_t>& key, F body,
                bool sync_before_capture) {
    auto it = gc.map.find(key);
    if (it == gc.map.end()) {
        if (gc.map.size() >= PGMI_GRAPH_CACHE_MAX) gc.clear();
        gc.map[key] = nullptr;
        return body(s);
    }
    if (it->second) {
        HIPCHK(hipGraphLaunch(it->second, s));
        return 0;
    }
    // Capture.  Whatever fails from here on: an opened capture is ended, a graph we got is destroyed and the key's
    // entry is erased (the next call with it starts over, eagerly); the first error is the one reported.
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    int rc = 0;
    hipError_t e = sync_before_capture ? hipStreamSynchronize(s) : hipSuccess;
    if (e == hipSuccess && (e = hipStreamBeginCapture(x->cap_stream, hipStreamCaptureModeThreadLocal)) == hipSuccess) {
        rc = body(x->cap_stream);  // may fail and return (HIPCHK) with the capture open: it is ended here
        const hipError_t end = hipStreamEndCapture(x->cap_stream, &g);
        if (rc == 0) e = end;
    }
    if (rc == 0 && e == hipSuccess) e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    if (rc == 0 && e == hipSuccess) e = hipGraphLaunch(exec, s);
    if (rc == 0 && e == hipSuccess) {
        gc.map[key] = exec;
        return 0;
    }
    if (exec) (void)hipGraphExecDestroy(exec);
    gc.map.erase(key);
    return rc ? rc : fail(PGMI_E_HIP, std::string("hipGraph capture: ") + hipGetErrorString(e));
}

// prefill calls (vision tower, language-model forward): one body, and no graph at all while prefill_graph is off
template <class F>
int run_prefill(pgmi_ctx* x, hipStream_t s, const std::vector<intptr_t>& key, F body) {
    if (!x->prefill_graph) return body(s);
    return run_graphed(x, x->pgraphs, s, key, body, false);
}

}  // namespace

// ================================================================ C ABI
// RCCL is loaded on first use (dlopen), so a single-GPU process -- and the CPU tests that only load
// the library -- need no librccl; the four entry points it uses are resolved once.
namespace {
struct Rccl {
    void* h = nullptr;
    std::string why;  // dlerror() of the failed load
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
};

// thread-safe one-time load (a function-local static is initialised exactly once)
Rccl& rccl() {
    static Rccl r = [] {
        Rccl t;
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            if ((t.h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
            const char* e = dlerror();
            if (e) t.why = e;
        }
        if (t.h) {
            t.get_unique_id = reinterpret_cast<decltype(t.get_unique_id)>(dlsym(t.h, "ncclGetUniqueId"));
            t.comm_init_rank = reinterpret_cast<decltype(t.comm_init_rank)>(dlsym(t.h, "ncclCommInitRank"));
            t.comm_destroy = reinterpret_cast<decltype(t.comm_destroy)>(dlsym(t.h, "ncclCommDestroy"));
            t.broadcast = reinterpret_cast<decltype(t.broadcast)>(dlsym(t.h, "ncclBroadcast"));
            t.error_string = reinterpret_cast<decltype(t.error_string)>(dlsym(t.h, "ncclGetErrorString"));
        }
        return t;
    }();
    return r;
}
}  // namespace

extern "C" {

const char* pgmi_last_error(void) { return g_err.c_str(); }
const char* pgmi_version(void) { return "pgmi 0.1.0 (gfx950)"; }

int pgmi_create(int device, const pgmi_config* cfg, pgmi_ctx** out) {
    if (!cfg || !out) return fail(PGMI_E_ARG, "null argument");
    const pgmi_config& c = *cfg;
    if (c.t_head_dim != 256) return fail(PGMI_E_ARG, "head_dim must be 256 (Gemma)");
    if (c.t_hidden != 2048) return fail(PGMI_E_ARG, "text hidden must be 2048 (decode kernels are specialised)");
    if (c.t_intermediate % 8 != 0 || c.v_intermediate % 8 != 0) return fail(PGMI_E_ARG, "intermediate sizes must be multiples of 8");
    if (c.v_hidden % c.v_heads != 0 || c.v_hidden / c.v_heads != 72) return fail(PGMI_E_ARG, "SigLIP head_dim must be 72");
    if (c.t_kv_heads != 1 || c.t_heads > 8)
        return fail(PGMI_E_ARG, "decode path is specialised for MQA with <= 8 query heads (num_key_value_heads = 1)");
    if (c.max_batch < 1 || c.max_batch > kMaxRows) return fail(PGMI_E_ARG, "max_batch must be in [1, 16]");
    if (c.v_hidden > 4096) return fail(PGMI_E_ARG, "v_hidden too large for the LayerNorm kernel");
    auto* x = new pgmi_ctx();
    x->c = c;
    if (x->c.max_kv <= 0) x->c.max_kv = c.t_max_pos;
    x->device = device;
    build_layout(x);
    x->inv_freq.resize(c.t_head_dim / 2);
    for (int i = 0; i < c.t_head_dim / 2; ++i) {
        // 1.0 / (base ** (arange(0, dim, 2).float() / dim)), fp32 (modeling_gemma.py:151)
        const float e = (float)(2 * i) / (float)c.t_head_dim;
        const float p = (float)std::pow((double)c.t_rope_theta, (double)e);
        x->inv_freq[i] = 1.0f / p;
    }
    *out = x;
    return 0;
}

int pgmi_destroy(pgmi_ctx* x) {
    if (!x) return 0;
    for (auto& e : x->probe_ev) (void)hipEventDestroy(e);
    x->dgraphs.clear();
    x->pgraphs.clear();
    for (auto& a : x->lora)
        for (auto& t : a.targets) { (void)hipFree(t.A); (void)hipFree(t.B); }
    for (auto& kv : x->lora_pristine) (void)hipFree(kv.second.copy);
    for (void* p : x->allocs) (void)hipFree(p);
    if (x->cap_stream) (void)hipStreamDestroy(x->cap_stream);
    delete x;
    return 0;
}

int64_t pgmi_weights_bytes(const pgmi_ctx* x) { return x ? x->slab_bytes : -1; }
int pgmi_weight_count(const pgmi_ctx* x) { return x ? (int)x->slots.size() : -1; }

int pgmi_weight_info(const pgmi_ctx* x, int idx, const char** name, int64_t* off, int64_t* shape4, int* ndim) {
    if (!x || idx < 0 || idx >= (int)x->slots.size()) return fail(PGMI_E_ARG, "weight index out of range");
    const Slot& s = x->slots[idx];
    if (name) *name = s.name.c_str();
    if (off) *off = s.off;
    if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = s.shape[i];
    if (ndim) *ndim = s.ndim;
    return 0;
}

int pgmi_bind_weights(pgmi_ctx* x, void* slab) {
    if (!x || !slab) return fail(PGMI_E_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(slab) % 256 != 0) return fail(PGMI_E_ARG, "weight slab must be 256-byte aligned");
    x->slab = reinterpret_cast<uint8_t*>(slab);
    x->lora_active = -1;  // a new slab holds its own base: nothing is merged into it
    lora_forget_pristine(x);
    pk_forget(x);
    x->dgraphs.clear();
    x->pgraphs.clear();
    return bind_tables(x);
}

int pgmi_load_weight(pgmi_ctx* x, const char* name, const void* src, int dtype, int on_device, void* stream) {
    if (!x || !name || !src) return fail(PGMI_E_ARG, "null argument");
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound");
    if (x->lora_active >= 0) return fail(PGMI_E_STATE, kLoraActiveMsg);
    auto it = x->index.find(name);
    if (it == x->index.end()) return fail(PGMI_E_ARG, std::string("unknown weight ") + name);
    const Slot& s = x->slots[it->second];
    uint16_t* dst = reinterpret_cast<uint16_t*>(x->slab + s.off);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(x->device));
    if (dtype == PGMI_DTYPE_BF16) {
        HIPCHK(hipMemcpyAsync(dst, src, s.numel * 2, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    } else if (dtype == PGMI_DTYPE_F32 || dtype == PGMI_DTYPE_F16) {
        if (on_device) {
            hipLaunchKernelGGL(k_convert, dim3(1024), dim3(256), 0, st, src, dtype, (long)s.numel, dst);
            LAUNCHCHK();
        } else {
            std::vector<uint16_t> tmp(s.numel);
            for (int64_t i = 0; i < s.numel; ++i) {
                float f = dtype == PGMI_DTYPE_F32 ? reinterpret_cast<const float*>(src)[i]
                                                 : (float)reinterpret_cast<const _Float16*>(src)[i];
                tmp[i] = host_f2bf(f);
            }
            HIPCHK(hipMemcpyAsync(dst, tmp.data(), s.numel * 2, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    } else {
        return fail(PGMI_E_ARG, "unsupported dtype");
    }
    return 0;
}

int pgmi_safetensors_count(const char* path, int* n) {
    if (!path || !n) return fail(PGMI_E_ARG, "null argument");
    StFile f;
    if (!st_open(path, f)) return fail(PGMI_E_ARG, f.error);
    *n = (int)f.entries.size();
    return 0;
}

int pgmi_safetensors_entry(const char* path, int i, char* name, int name_cap, int* dtype, int64_t* shape4, int* ndim,
                           int64_t* begin, int64_t* end) {
    if (!path || !name || name_cap < 1 || !dtype || !shape4 || !ndim || !begin || !end)
        return fail(PGMI_E_ARG, "null argument");
    StFile f;
    if (!st_open(path, f)) return fail(PGMI_E_ARG, f.error);
    if (i < 0 || i >= (int)f.entries.size()) return fail(PGMI_E_ARG, "entry index out of range");
    const StEntry& e = f.entries[i];
    std::snprintf(name, (size_t)name_cap, "%s", e.name.c_str());
    *dtype = e.dtype == "BF16" ? PGMI_DTYPE_BF16 : e.dtype == "F16" ? PGMI_DTYPE_F16 : e.dtype == "F32" ? PGMI_DTYPE_F32 : -1;
    *ndim = (int)e.shape.size();
    for (int d = 0; d < 4; ++d) shape4[d] = d < *ndim ? e.shape[d] : 0;
    *begin = e.begin;
    *end = e.end;
    return 0;
}

// utils.py:19-44 (safe_open shard loop + load_state_dict(strict=False)) for one shard: tensors
// named like slab weights are shape-checked, converted to bf16 and written into the slab; BF16
// bytes go host -> slab directly from the mapped file, F32/F16 through the split-K scratch in
// chunks and a device-side RNE conversion.  Synchronises the stream before unmapping.
int pgmi_load_safetensors(pgmi_ctx* x, const char* path, int* n_loaded, int* n_skipped, void* stream) {
    if (!x || !path) return fail(PGMI_E_ARG, "null argument");
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound");
    if (x->lora_active >= 0) return fail(PGMI_E_STATE, kLoraActiveMsg);
    HIPCHK(hipSetDevice(x->device));
    StFile f;
    if (!st_open(path, f)) return fail(PGMI_E_ARG, f.error);
    hipStream_t st = (hipStream_t)stream;
    // scratch for conversions: the context's workspace if prepared, else a temporary buffer
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    uint8_t* scratch = reinterpret_cast<uint8_t*>(x->ws);
    size_t scratch_bytes = x->ws ? x->ws_bytes : 0;
    int loaded = 0, skipped = 0;
    int rc = 0;
    for (const StEntry& e : f.entries) {
        auto it = x->index.find(e.name);
        if (it == x->index.end()) {
            ++skipped;
            continue;
        }
        const Slot& sl = x->slots[it->second];
        bool same = (int)e.shape.size() == sl.ndim;
        for (int d = 0; same && d < sl.ndim; ++d) same = e.shape[d] == sl.shape[d];
        if (!same) {
            rc = fail(PGMI_E_ARG, "shape mismatch for " + e.name);
            break;
        }
        const int eb = st_elem_bytes(e.dtype);
        if (eb == 0) {
            rc = fail(PGMI_E_ARG, "unsupported dtype " + e.dtype + " for " + e.name);
            break;
        }
        if (e.end - e.begin != sl.numel * eb) {
            rc = fail(PGMI_E_ARG, "byte size mismatch for " + e.name);
            break;
        }
        const uint8_t* src = f.map + f.data0 + e.begin;
        uint16_t* dst = reinterpret_cast<uint16_t*>(x->slab + sl.off);
        if (e.dtype == "BF16") {
            if (hipMemcpyAsync(dst, src, (size_t)sl.numel * 2, hipMemcpyHostToDevice, st) != hipSuccess) {
                rc = fail(PGMI_E_HIP, "upload of " + e.name);
                break;
            }
        } else {
            const int dt = e.dtype == "F32" ? PGMI_DTYPE_F32 : PGMI_DTYPE_F16;
            if (scratch_bytes < ((size_t)8 << 20)) {
                if (!tmp) {
                    tmp_bytes = (size_t)64 << 20;
                    if (hipMalloc(&tmp, tmp_bytes) != hipSuccess) {
                        rc = fail(PGMI_E_NOMEM, "conversion scratch");
                        break;
                    }
                }
                scratch = reinterpret_cast<uint8_t*>(tmp);
                scratch_bytes = tmp_bytes;
            }
            const int64_t per = (int64_t)(scratch_bytes / (size_t)eb);
            for (int64_t i0 = 0; i0 < sl.numel && rc == 0; i0 += per) {
                const int64_t n = std::min<int64_t>(per, sl.numel - i0);
                if (hipMemcpyAsync(scratch, src + i0 * eb, (size_t)n * eb, hipMemcpyHostToDevice, st) != hipSuccess) {
                    rc = fail(PGMI_E_HIP, "upload of " + e.name);
                    break;
                }
                hipLaunchKernelGGL(k_convert, dim3(1024), dim3(256), 0, st, scratch, dt, (long)n, dst + i0);
            }
            if (rc) break;
        }
        ++loaded;
    }
    const hipError_t se = hipStreamSynchronize(st);  // the mapped bytes must outlive the copies
    if (tmp) (void)hipFree(tmp);
    if (rc) return rc;
    if (se != hipSuccess) return fail(PGMI_E_HIP, std::string("safetensors upload: ") + hipGetErrorString(se));
    x->prepared = false;  // derived tensors (padded patch matrix, ...) are rebuilt by pgmi_prepare
    if (n_loaded) *n_loaded = loaded;
    if (n_skipped) *n_skipped = skipped;
    return 0;
}

uint64_t pgmi_synthetic_key(const char* name, uint64_t seed) { return splitmix64_h(seed ^ fnv1a(name)); }

int pgmi_fill_synthetic(pgmi_ctx* x, const char* name, uint64_t key, float scale, float offset, void* stream) {
    if (!x || !name) return fail(PGMI_E_ARG, "null argument");
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound");
    if (x->lora_active >= 0) return fail(PGMI_E_STATE, kLoraActiveMsg);
    auto it = x->index.find(name);
    if (it == x->index.end()) return fail(PGMI_E_ARG, std::string("unknown weight ") + name);
    const Slot& s = x->slots[it->second];
    HIPCHK(hipSetDevice(x->device));
    fill_synthetic((hipStream_t)stream, reinterpret_cast<uint16_t*>(x->slab + s.off), (long)s.numel, key, scale, offset);
    LAUNCHCHK();
    return 0;
}

int pgmi_set_rope_inv_freq(pgmi_ctx* x, const float* inv) {
    if (!x || !inv) return fail(PGMI_E_ARG, "null argument");
    for (int i = 0; i < x->c.t_head_dim / 2; ++i) x->inv_freq[i] = inv[i];
    x->host_cos.clear();
    x->host_sin.clear();
    x->prepared = false;
    return 0;
}

int pgmi_set_rope_table(pgmi_ctx* x, const uint16_t* cs, const uint16_t* sn, int max_pos) {
    if (!x || !cs || !sn) return fail(PGMI_E_ARG, "null argument");
    if (max_pos != x->c.t_max_pos) return fail(PGMI_E_ARG, "rope table must cover max_position_embeddings");
    const size_t n = (size_t)max_pos * (x->c.t_head_dim / 2);
    x->host_cos.assign(cs, cs + n);
    x->host_sin.assign(sn, sn + n);
    x->prepared = false;
    return 0;
}

int pgmi_prepare(pgmi_ctx* x) {
    if (!x) return fail(PGMI_E_ARG, "null argument");
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound");
    HIPCHK(hipSetDevice(x->device));
    const pgmi_config& c = x->c;
    int rc;
    if (!x->cosT) {
        const int N = n_img(c);
        // R: every row of a batch (the hidden state, its norm, positions); RG / RV: one prefill group's rows, all that
        // the per-layer scratch and the vision workspace ever hold at a time
        const size_t R = (size_t)c.max_batch * c.max_seq, RG = (size_t)std::min(c.max_batch, kPrefillGroup) * c.max_seq,
                     RV = (size_t)std::min(c.max_batch, kPrefillGroup) * N;
        const int H = c.t_hidden, QKVN = (c.t_heads + 2 * c.t_kv_heads) * c.t_head_dim;
        x->kpad = (c.v_channels * c.v_patch * c.v_patch + 63) / 64 * 64;
        if ((rc = dalloc_t(x, &x->patch_w, (size_t)c.v_hidden * x->kpad))) return rc;
        if ((rc = dalloc_t(x, &x->cosT, (size_t)c.t_max_pos * c.t_head_dim / 2))) return rc;
        if ((rc = dalloc_t(x, &x->sinT, (size_t)c.t_max_pos * c.t_head_dim / 2))) return rc;
        if ((rc = dalloc_t(x, &x->Hs, R * H))) return rc;
        if ((rc = dalloc_t(x, &x->Tn, R * H))) return rc;
        if ((rc = dalloc_t(x, &x->QKV, RG * QKVN))) return rc;
        if ((rc = dalloc_t(x, &x->Qr, RG * c.t_heads * c.t_head_dim))) return rc;
        if ((rc = dalloc_t(x, &x->AO, RG * H))) return rc;
        if ((rc = dalloc_t(x, &x->ACT, RG * c.t_intermediate))) return rc;
        if ((rc = dalloc_t(x, &x->lastrows, (size_t)c.max_batch * H))) return rc;
        if ((rc = dalloc_t(x, &x->dpos, R))) return rc;
        if ((rc = dalloc_t(x, &x->dids_tmp, R))) return rc;
        if ((rc = dalloc_t(x, &x->vX, RV * c.v_hidden))) return rc;
        if ((rc = dalloc_t(x, &x->vT, RV * c.v_hidden))) return rc;
        if ((rc = dalloc_t(x, &x->vQKV, RV * 3 * c.v_hidden))) return rc;
        if ((rc = dalloc_t(x, &x->vAO, RV * c.v_hidden))) return rc;
        if ((rc = dalloc_t(x, &x->vH, RV * c.v_intermediate))) return rc;
        if ((rc = dalloc_t(x, &x->vP, RV * x->kpad))) return rc;
        x->ws_bytes = (size_t)64 << 20;
        if ((rc = dalloc(x, reinterpret_cast<void**>(&x->ws), x->ws_bytes))) return rc;
        const int B = c.max_batch;
        if ((rc = dalloc_t(x, &x->dH, (size_t)B * H))) return rc;
        if ((rc = dalloc_t(x, &x->dQ, (size_t)B * c.t_heads * c.t_head_dim))) return rc;
        if ((rc = dalloc_t(x, &x->dAO, (size_t)B * H))) return rc;
        if ((rc = dalloc_t(x, &x->dACT, (size_t)B * c.t_intermediate))) return rc;
        if ((rc = dalloc_t(x, &x->dHn, (size_t)B * H))) return rc;
        if ((rc = dalloc_t(x, &x->dSS, (size_t)B * (H / 16)))) return rc;
        x->max_chunks = (c.max_kv + 63) / 64;
        if ((rc = dalloc_t(x, &x->opart, attention_decode_part_floats(B, c.t_kv_heads, x->max_chunks)))) return rc;
        if ((rc = dalloc_t(x, &x->pmax, (size_t)B * gemv_logits_blocks()))) return rc;
        if ((rc = dalloc_t(x, &x->dlogits, (size_t)B * c.t_vocab))) return rc;
        if ((rc = dalloc_t(x, &x->pidx, (size_t)B * gemv_logits_blocks()))) return rc;
        if ((rc = dalloc_t(x, &x->step, 1))) return rc;
        if ((rc = dalloc_t(x, &x->pstep, 1))) return rc;
        if ((rc = dalloc_t(x, &x->rstep, kMaxRows))) return rc;
        if ((rc = dalloc_t(x, &x->d_rlens, 2 * kMaxRows))) return rc;
        if ((rc = dalloc_t(x, &x->amax_v, (size_t)argmax_scratch_parts()))) return rc;
        if ((rc = dalloc_t(x, &x->amax_i, (size_t)argmax_scratch_parts()))) return rc;
        if ((rc = dalloc_t(x, &x->d_ids, (size_t)B))) return rc;
        if ((rc = dalloc_t(x, &x->d_emb, (size_t)B * H))) return rc;
        if ((rc = dalloc_t(x, &x->d_mask, (size_t)B * c.max_kv))) return rc;
        if ((rc = dalloc_t(x, &x->d_zero, 64))) return rc;
        HIPCHK(hipMemset(x->d_zero, 0, 64 * sizeof(float)));
        if ((rc = dalloc_t(x, &x->d_next, (size_t)B))) return rc;
        if ((rc = dalloc_t(x, &x->lm_done, 33 * 32))) return rc;  // top word + 32 shards, a 128-B line each
        HIPCHK(hipMemset(x->lm_done, 0, 33 * 32 * sizeof(unsigned)));
        HIPCHK(hipStreamCreateWithFlags(&x->cap_stream, hipStreamNonBlocking));
    }
    // derived tensors
    pad_rows(nullptr, x->w.patch_conv_w, c.v_hidden, c.v_channels * c.v_patch * c.v_patch, x->kpad, x->patch_w);
    LAUNCHCHK();
    // the batched decode's fragment-major weight images: built by the first decode step with B >= 3 after this
    // call (ensure_mf_image), not here -- a context that never decodes a batch (the drop-in's single-sequence
    // loop on its max_batch-8 context) neither allocates their 3.96 GB nor pays for the swizzle
    x->mfw_dirty = mf_wanted(c);
    // the 13-bit images of the B <= 2 step likewise: rebuilt from the new weights by the next such step
    pk_forget(x);
    // LoRA: with no adapter merged the base may have changed, so the pristine copies are taken anew at the next
    // activation; with one merged the slab is derived from as it is and the copies still hold its base
    if (x->lora_active < 0) lora_forget_pristine(x);
    std::vector<uint16_t> cs, sn;
    if (!x->host_cos.empty()) {
        cs = x->host_cos;
        sn = x->host_sin;
    } else {
        build_rope_host(x, cs, sn);
    }
    HIPCHK(hipMemcpy(x->cosT, cs.data(), cs.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->sinT, sn.data(), sn.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    x->dgraphs.clear();
    x->pgraphs.clear();
    x->prepared = true;
    return 0;
}

int64_t pgmi_kv_bytes(const pgmi_ctx* x, int batch, int max_tokens) {
    if (!x) return -1;
    return (int64_t)x->c.t_layers * 2 * batch * max_tokens * x->c.t_kv_heads * x->c.t_head_dim * 2;
}

int pgmi_graph_count(const pgmi_ctx* x, int which) {
    if (!x) return -1;
    return (int)(which == 0 ? x->pgraphs : x->dgraphs).map.size();
}

static int vision_body(pgmi_ctx* x, hipStream_t s, const void* pixels, int dtype, int B, void* feats);

int pgmi_vision(pgmi_ctx* x, const void* pixels, int dtype, int B, void* feats, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (B < 1 || B > c.max_batch) return fail(PGMI_E_ARG, "batch exceeds max_batch");
    if (!pixels || !feats) return fail(PGMI_E_ARG, "null argument");
    const std::vector<intptr_t> key{1, (intptr_t)pixels, dtype, B, (intptr_t)feats};
    // more than kPrefillGroup images: row groups of that many, one after the other through the same workspace, each
    // with the plans measured for it -- an image's features do not depend on how many images share the call
    const size_t px_img = (size_t)c.v_channels * c.v_image * c.v_image * (dtype == PGMI_DTYPE_F32 ? 4 : 2);
    const size_t ft_img = (size_t)n_img(c) * c.v_hidden * sizeof(uint16_t);
    rc = run_prefill(x, (hipStream_t)stream, key, [&](hipStream_t st) {
        for (int b0 = 0; b0 < B; b0 += kPrefillGroup) {
            const int r = vision_body(x, st, reinterpret_cast<const char*>(pixels) + b0 * px_img, dtype,
                                      std::min(kPrefillGroup, B - b0), reinterpret_cast<char*>(feats) + b0 * ft_img);
            if (r) return r;
        }
        return 0;
    });
    if (rc) return rc;
    LAUNCHCHK();
    return 0;
}

static int vision_body(pgmi_ctx* x, hipStream_t s, const void* pixels, int dtype, int B, void* feats) {
    const pgmi_config& c = x->c;
    const WeightTable& w = x->w;
    const int N = n_img(c), D = c.v_hidden, Iv = c.v_intermediate, rows = B * N;
    const float eps = c.v_ln_eps;
    patchify(s, pixels, dtype == PGMI_DTYPE_F32, B, c.v_channels, c.v_image, c.v_image, c.v_patch, x->kpad, x->vP);
    // Conv2d + bias + position embedding (modeling_siglip.py:67,76)
    EpiArgs e{};
    e.bias = w.patch_b;
    e.pos = w.pos_emb;
    e.npos = N;
    e.out = x->vX;
    e.ldo = D;
    gemm(s, x->vP, x->kpad, x->patch_w, x->kpad, rows, D, x->kpad, EPI_BIAS_POS, e, x->ws, x->ws_bytes);
    const float scale = (float)std::pow((double)(D / c.v_heads), -0.5);  // head_dim**-0.5 (:89)
    // LayerNorm1 of layer 0; every later LayerNorm is fused with the preceding projection's
    // split-K reduction + bias + residual (splitk_res_norm)
    if (c.v_layers > 0) layernorm(s, x->vX, w.v[0].ln1_w, w.v[0].ln1_b, eps, x->vT, rows, D);
    for (int i = 0; i < c.v_layers; ++i) {
        const bool last = i + 1 == c.v_layers;
        const VisionLayerW& l = w.v[i];
        EpiArgs q{};
        q.bias = l.qkv_b;
        q.out = x->vQKV;
        q.ldo = 3 * D;
        gemm(s, x->vT, D, l.qkv_w, D, rows, 3 * D, D, EPI_BIAS, q, x->ws, x->ws_bytes);
        AttnArgs a{};
        a.q = x->vQKV; a.q_b_stride = (long)N * 3 * D; a.q_row_stride = 3 * D; a.q_head_stride = 72;
        a.k = x->vQKV + D; a.k_b_stride = a.q_b_stride; a.k_row_stride = 3 * D; a.k_head_stride = 72;
        a.v = x->vQKV + 2 * D; a.v_b_stride = a.q_b_stride; a.v_row_stride = 3 * D; a.v_head_stride = 72;
        a.o = x->vAO; a.o_b_stride = (long)N * D; a.o_row_stride = D; a.o_head_stride = 72;
        a.Lq = N; a.Lk = N; a.G = 1; a.n_kv = c.v_heads; a.B = B; a.scale = scale;
        a.ws = x->ws; a.ws_floats = (long)(x->ws_bytes / sizeof(float));
        attention_prefill(s, 72, a);
        EpiArgs o{};
        o.bias = l.out_b;
        o.res = x->vX; o.ldr = D; o.out = x->vX; o.ldo = D;
        const int spo = gemm(s, x->vAO, D, l.out_w, D, rows, D, D, EPI_BIAS_RES, o, x->ws, x->ws_bytes, 0, true);
        splitk_res_norm(s, x->ws, spo, o.bias, x->vX, l.ln2_w, l.ln2_b, eps, x->vT, rows, D);
        EpiArgs f1{};
        f1.bias = l.fc1_b; f1.out = x->vH; f1.ldo = Iv;
        gemm(s, x->vT, D, l.fc1_w, D, rows, Iv, D, EPI_BIAS_GELU, f1, x->ws, x->ws_bytes);
        EpiArgs f2{};
        f2.bias = l.fc2_b; f2.res = x->vX; f2.ldr = D; f2.out = x->vX; f2.ldo = D;
        const int sp = gemm(s, x->vH, Iv, l.fc2_w, Iv, rows, D, Iv, EPI_BIAS_RES, f2, x->ws, x->ws_bytes, 0, true);
        splitk_res_norm(s, x->ws, sp, f2.bias, x->vX, last ? w.post_ln_w : w.v[i + 1].ln1_w,
                        last ? w.post_ln_b : w.v[i + 1].ln1_b, eps, last ? reinterpret_cast<uint16_t*>(feats) : x->vT,
                        rows, D);
    }
    if (c.v_layers == 0)
        layernorm(s, x->vX, w.post_ln_w, w.post_ln_b, eps, reinterpret_cast<uint16_t*>(feats), rows, D);
    LAUNCHCHK();
    return 0;
}

int pgmi_project(pgmi_ctx* x, const void* feats, int rows, void* out, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (!feats || !out || rows < 1) return fail(PGMI_E_ARG, "bad argument");
    if (rows > x->c.max_batch * n_img(x->c)) return fail(PGMI_E_ARG, "rows exceed workspace capacity");
    EpiArgs e{};
    e.bias = x->w.proj_b;
    e.out = reinterpret_cast<uint16_t*>(out);
    e.ldo = x->c.projection_dim;
    const int grp = kPrefillGroup * n_img(x->c);  // row groups of kPrefillGroup images, as pgmi_vision
    for (int r0 = 0; r0 < rows; r0 += grp) {
        e.out = reinterpret_cast<uint16_t*>(out) + (size_t)r0 * x->c.projection_dim;
        gemm((hipStream_t)stream, reinterpret_cast<const uint16_t*>(feats) + (size_t)r0 * x->c.v_hidden, x->c.v_hidden,
             x->w.proj_w, x->c.v_hidden, std::min(grp, rows - r0), x->c.projection_dim, x->c.v_hidden, EPI_BIAS, e, x->ws,
             x->ws_bytes);
    }
    LAUNCHCHK();
    return 0;
}

int pgmi_embed(pgmi_ctx* x, const int64_t* ids, int rows, void* out, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (!ids || !out) return fail(PGMI_E_ARG, "null argument");
    // plain lookup: normalizer 1, no pad zeroing (nn.Embedding, modeling_gemma.py:565)
    embed_rows((hipStream_t)stream, ids, rows, x->w.embed, x->c.t_hidden, 1.0f, INT64_MIN,
               reinterpret_cast<uint16_t*>(out));
    LAUNCHCHK();
    return 0;
}

static int lm_body(pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
                   const void* embeds, int B, int L, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
                   int logits_rows, bool ragged);

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
};
static int lm_rows(pgmi_ctx* x, const PrefillRun& r);

static int lm_forward(pgmi_ctx* x, const int64_t* ids, const void* image_feats, int n_img_rows, const void* embeds,
                      int B, int L, const int64_t* positions, const int32_t* lens, bool ragged, void* kv, int kv_batch,
                      int kv_max, int kv_start, float* logits, int logits_rows, void* stream);

int pgmi_lm_forward(pgmi_ctx* x, const int64_t* ids, const void* image_feats, int n_img_rows, const void* embeds,
                    int B, int L, const int64_t* positions, void* kv, int kv_batch, int kv_max, int kv_start,
                    float* logits, int logits_rows, void* stream) {
    return lm_forward(x, ids, image_feats, n_img_rows, embeds, B, L, positions, nullptr, false, kv, kv_batch, kv_max,
                      kv_start, logits, logits_rows, stream);
}

int pgmi_lm_forward_ragged(pgmi_ctx* x, const int64_t* ids, const void* image_feats, int n_img_rows,
                           const void* embeds, int B, int L, const int64_t* positions, const int32_t* lens, void* kv,
                           int kv_batch, int kv_max, int kv_start, float* logits, int logits_rows, void* stream) {
    if (!lens) return fail(PGMI_E_ARG, "null argument");
    return lm_forward(x, ids, image_feats, n_img_rows, embeds, B, L, positions, lens, true, kv, kv_batch, kv_max,
                      kv_start, logits, logits_rows, stream);
}

// What a language-model prefill does before its launches, shared by lm_forward and the stage hook
// (pgmi_debug_prefill_stage): the argument checks, the ragged rows' lengths and the positions to the device.
static int lm_begin(pgmi_ctx* x, const int64_t* ids, const void* embeds, int B, int L, const int64_t* positions,
                    const int32_t* lens, bool ragged, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
                    int* logits_rows_io, void* stream) {
    int rc;
    int logits_rows = *logits_rows_io;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (B < 1 || B > c.max_batch || B > kv_batch) return fail(PGMI_E_ARG, "batch exceeds capacity");
    if (L < 1 || L > c.max_seq) return fail(PGMI_E_ARG, "sequence length exceeds max_seq");
    if (kv_start < 0 || kv_start + L > kv_max) return fail(PGMI_E_ARG, "KV cache capacity exceeded");
    if (!positions || !kv || !logits || (!embeds && !ids)) return fail(PGMI_E_ARG, "null argument");
    if (logits_rows < 0 || logits_rows > 2) return fail(PGMI_E_ARG, "logits_rows must be 0, 1 or 2");
    if (ragged) {
        // per-row token counts -> the context's device buffer, outside any graph (a replay reads this call's)
        if (embeds || !ids) return fail(PGMI_E_ARG, "ragged prefill takes token ids (pad slots enter as zero rows)");
        RowInts rl{}, rk{};
        for (int b = 0; b < B; ++b) {
            if (lens[b] < 1 || lens[b] > L) return fail(PGMI_E_ARG, "lens[b] must be in [1, L]");
            rl.v[b] = lens[b];
            rk.v[b] = kv_start + lens[b];
        }
        set_row_ints((hipStream_t)stream, x->d_rlens, rl, rk, B);
        LAUNCHCHK();
        if (logits_rows == 2) logits_rows = 1;  // the last-row-only form is the lock-step prefill's
    }
    // host positions -> device (outside any graph: a pageable host copy is not captured)
    HIPCHK(hipMemcpyAsync(x->dpos, positions, (size_t)B * L * sizeof(int64_t), hipMemcpyHostToDevice,
                          (hipStream_t)stream));
    // Tn is overwritten from here on: no row of it is valid until this call has succeeded
    x->tn_rows = 0;
    *logits_rows_io = logits_rows;
    return 0;
}

static int lm_forward(pgmi_ctx* x, const int64_t* ids, const void* image_feats, int n_img_rows, const void* embeds,
                      int B, int L, const int64_t* positions, const int32_t* lens, bool ragged, void* kv, int kv_batch,
                      int kv_max, int kv_start, float* logits, int logits_rows, void* stream) {
    int rc;
    if ((rc = lm_begin(x, ids, embeds, B, L, positions, lens, ragged, kv, kv_batch, kv_max, kv_start, logits,
                       &logits_rows, stream)))
        return rc;
    const std::vector<intptr_t> key{2, (intptr_t)ids, (intptr_t)image_feats, n_img_rows, (intptr_t)embeds, B, L,
                                    (intptr_t)kv, kv_batch, kv_max, kv_start, (intptr_t)logits, logits_rows,
                                    (intptr_t)ragged};
    rc = run_prefill(x, (hipStream_t)stream, key, [&](hipStream_t st) {
        return lm_body(x, st, ids, image_feats, n_img_rows, embeds, B, L, kv, kv_batch, kv_max, kv_start, logits,
                       logits_rows, ragged);
    });
    if (rc) return rc;
    x->tn_rows = logits_rows == 2 && L > 1 ? 0 : (long)B * L;
    LAUNCHCHK();
    return 0;
}

// the prefill's entry, for the whole batch: the merged (or given) embeddings x the normalizer -> Hs
static void lm_entry(pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
                     const void* embeds, int B, int L, bool ragged) {
    const pgmi_config& c = x->c;
    // ragged: row b holds lens[b] tokens (d_rlens, set outside the graph), the rest of its L slots is padding
    const int* rlens = ragged ? x->d_rlens : nullptr;
    const int H = c.t_hidden, R = B * L;
    const float normalizer = bf16_round_host(std::sqrt((float)H));  // torch.tensor(H**0.5, dtype=bf16) (:367)
    const uint16_t* E = x->w.embed;
    if (embeds) {
        scale_rows(s, reinterpret_cast<const uint16_t*>(embeds), (long)R * H, normalizer, x->Hs);
    } else {
        merge_embed(s, ids, B, L, E, H, reinterpret_cast<const uint16_t*>(image_feats), image_feats ? n_img_rows : 0,
                    c.image_token_index, c.pad_token_id, (float)std::sqrt((double)H), normalizer, nullptr,
                    reinterpret_cast<int*>(x->dids_tmp), x->Hs, rlens);
    }
}

static int lm_body(pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
                   const void* embeds, int B, int L, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
                   int logits_rows, bool ragged) {
    lm_entry(x, s, ids, image_feats, n_img_rows, embeds, B, L, ragged);
    // the layers: row groups of at most kPrefillGroup sequences, one after the other (the merge above ran for the
    // whole batch: the k-th <image> token of the batch takes image row k); a group's rows of Hs / Tn, its positions,
    // lengths, KV rows and logits are its slice of the batch's, everything else is scratch that the groups share
    for (int b0 = 0; b0 < B; b0 += kPrefillGroup) {
        const PrefillRun r{s, b0, std::min(kPrefillGroup, B - b0), L, kv, kv_batch, kv_max, kv_start, logits,
                           logits_rows, ragged};
        if (int rc = lm_rows(x, r)) return rc;
    }
    return 0;
}

// the group's slices and the per-layer cache rows
static uint16_t* run_hs(const pgmi_ctx* x, const PrefillRun& r) { return x->Hs + (size_t)r.b0 * r.L * x->c.t_hidden; }
static uint16_t* run_tn(const pgmi_ctx* x, const PrefillRun& r) { return x->Tn + (size_t)r.b0 * r.L * x->c.t_hidden; }
static uint16_t* run_lastrows(const pgmi_ctx* x, const PrefillRun& r) {
    return x->lastrows + (size_t)r.b0 * x->c.t_hidden;
}
static long run_kvb(const pgmi_ctx* x, const PrefillRun& r) {
    return (long)r.kv_max * x->c.t_kv_heads * x->c.t_head_dim;
}
// layer i's K (v = 0) or V (v = 1) rows of the group
static uint16_t* run_cache(const pgmi_ctx* x, const PrefillRun& r, int i, int v) {
    const long kvb = run_kvb(x, r);
    return reinterpret_cast<uint16_t*>(r.kv) + (long)r.b0 * kvb + ((long)(i * 2 + v) * r.kv_batch) * kvb;
}
// logits_rows == 2: the last layer's post-projection work runs for the last row of each sequence alone
static bool run_last_only(const pgmi_ctx* x, const PrefillRun& r) {
    return r.logits_rows == 2 && r.L > 1 && x->c.t_layers > 0;
}

// input RMSNorm of layer 0; every later RMSNorm (and the final norm) is fused with the
// preceding projection's split-K reduction + residual (splitk_res_norm)
static void lm_in_norm(pgmi_ctx* x, const PrefillRun& r) {
    const pgmi_config& c = x->c;
    rmsnorm(r.s, run_hs(x, r), c.t_layers ? x->w.t[0].in_norm : x->w.final_norm, c.t_rms_eps, run_tn(x, r), r.B * r.L,
            c.t_hidden);
}

// layer i's q|k|v with RoPE and the KV append: Tn -> Qr, the cache rows
static void lm_qkv(pgmi_ctx* x, const PrefillRun& r, int i) {
    const pgmi_config& c = x->c;
    hipStream_t s = r.s;
    const int H = c.t_hidden, R = r.B * r.L, NH = c.t_heads, NKV = c.t_kv_heads, HD = c.t_head_dim;
    const int QKVN = (NH + 2 * NKV) * HD;
    const long kvb = run_kvb(x, r);
    const TextLayerW& w = x->w.t[i];
    uint16_t* const Tn = run_tn(x, r);
    const int64_t* const dpos = x->dpos + (size_t)r.b0 * r.L;
    uint16_t* Kc = run_cache(x, r, i, 0);
    uint16_t* Vc = run_cache(x, r, i, 1);
    EpiArgs q{};
    q.out = x->QKV; q.ldo = QKVN;
    // RoPE + KV append in the projection's epilogue where the shape's plan allows it
    q.rpos = dpos; q.cosT = x->cosT; q.sinT = x->sinT; q.max_pos = c.t_max_pos;
    q.q_out = x->Qr; q.kc = Kc; q.vc = Vc; q.kv_b_stride = kvb; q.kv_start = r.kv_start;
    q.L = r.L; q.nh = NH; q.nkv = NKV;
    if (HD != 256 || !gemm_qkv_rope(s, Tn, H, w.qkv, H, R, QKVN, H, q)) {
        int sp = gemm(s, Tn, H, w.qkv, H, R, QKVN, H, EPI_STORE, q, x->ws, x->ws_bytes, 0, true);
        rope_kv_append(s, x->QKV, x->ws, sp, r.B, r.L, NH, NKV, dpos, x->cosT, x->sinT, c.t_max_pos, x->Qr, Kc, Vc,
                       kvb, r.kv_start);
    }
}

// layer i's attention arguments: every query row of the group over the cache rows [0, kv_start + L)
static AttnArgs lm_attn_args(const pgmi_ctx* x, const PrefillRun& r, int i) {
    const pgmi_config& c = x->c;
    const int H = c.t_hidden, NH = c.t_heads, NKV = c.t_kv_heads, HD = c.t_head_dim;
    const long kvd = (long)NKV * HD, kvb = run_kvb(x, r);
    AttnArgs a{};
    a.q = x->Qr; a.q_b_stride = (long)r.L * NH * HD; a.q_row_stride = NH * HD; a.q_head_stride = HD;
    a.k = run_cache(x, r, i, 0); a.k_b_stride = kvb; a.k_row_stride = (int)kvd; a.k_head_stride = HD;
    a.v = run_cache(x, r, i, 1); a.v_b_stride = kvb; a.v_row_stride = (int)kvd; a.v_head_stride = HD;
    a.o = x->AO; a.o_b_stride = (long)r.L * H; a.o_row_stride = H; a.o_head_stride = HD;
    a.Lq = r.L; a.Lk = r.kv_start + r.L; a.G = NH / NKV; a.n_kv = NKV; a.B = r.B;
    a.scale = 1.0f / std::sqrt((float)HD);  // / math.sqrt(head_dim) (:266): exact power of two
    a.ws = x->ws; a.ws_floats = (long)(x->ws_bytes / sizeof(float));
    // ragged: row b's real tokens attend its own real keys only
    a.klen = r.ragged ? x->d_rlens + kMaxRows + r.b0 : nullptr;
    return a;
}

// layer i's attention: Qr, the cache rows -> AO
static void lm_attn(pgmi_ctx* x, const PrefillRun& r, int i) { attention_prefill(r.s, 256, lm_attn_args(x, r, i)); }

// layer i's o_proj partial slabs, then their sum + residual and the post-attention norm: AO, Hs -> Hs, Tn
static void lm_o_proj(pgmi_ctx* x, const PrefillRun& r, int i) {
    const pgmi_config& c = x->c;
    const int H = c.t_hidden, R = r.B * r.L;
    const TextLayerW& w = x->w.t[i];
    uint16_t* const Hs = run_hs(x, r);
    EpiArgs o{};
    o.res = Hs; o.ldr = H; o.out = Hs; o.ldo = H;
    int sp = gemm(r.s, x->AO, H, w.o, H, R, H, c.t_heads * c.t_head_dim, EPI_RES, o, x->ws, x->ws_bytes, 0, true);
    splitk_res_norm(r.s, x->ws, sp, nullptr, Hs, w.post_norm, nullptr, c.t_rms_eps, run_tn(x, r), R, H);
}

// layer i's gate|up + GeGLU: Tn -> ACT
static void lm_gate_up(pgmi_ctx* x, const PrefillRun& r, int i) {
    const pgmi_config& c = x->c;
    const int H = c.t_hidden;
    EpiArgs g{};
    g.out = x->ACT; g.ldo = c.t_intermediate;
    // probe: the GEMM kernel itself carries the events (its own start / end, gemm_probe_events)
    const bool probe = x->probe_on && (size_t)(4 * i + 3) < x->probe_ev.size();
    if (probe) gemm_probe_events(x->probe_ev[4 * i], x->probe_ev[4 * i + 1]);
    gemm(r.s, run_tn(x, r), H, x->w.t[i].gate_up, H, r.B * r.L, c.t_intermediate, H, EPI_GEGLU, g, x->ws, x->ws_bytes,
         c.t_intermediate);
}

// layer i's down partial slabs, then their sum + residual and the next input norm (the final norm after the last
// layer): ACT, Hs -> Hs, Tn
static void lm_down(pgmi_ctx* x, const PrefillRun& r, int i) {
    const pgmi_config& c = x->c;
    const int H = c.t_hidden, R = r.B * r.L;
    uint16_t* const Hs = run_hs(x, r);
    EpiArgs d{};
    d.res = Hs; d.ldr = H; d.out = Hs; d.ldo = H;
    const bool probe = x->probe_on && (size_t)(4 * i + 3) < x->probe_ev.size();
    if (probe) gemm_probe_events(x->probe_ev[4 * i + 2], x->probe_ev[4 * i + 3]);
    const int sp = gemm(r.s, x->ACT, c.t_intermediate, x->w.t[i].down, c.t_intermediate, R, H, c.t_intermediate,
                        EPI_RES, d, x->ws, x->ws_bytes, 0, true);
    const bool last = i + 1 == c.t_layers;
    splitk_res_norm(r.s, x->ws, sp, nullptr, Hs, last ? x->w.final_norm : x->w.t[i + 1].in_norm, nullptr, c.t_rms_eps,
                    run_tn(x, r), R, H);
}

// logits_rows == 2, last layer: the K/V rows of every token are written by lm_qkv (the cache
// the decode loop reads); the rest of the layer feeds only the final hidden state, and the
// caller reads that for the last row alone, so attention, o_proj, the MLP and the final
// norm run for the last row of each sequence (row-wise ops: the same values as the
// all-row pass up to GEMV-vs-GEMM accumulation order), on the decode GEMVs: Qr, the cache rows, Hs -> lastrows
static int lm_last_row_tail(pgmi_ctx* x, const PrefillRun& r, int i) {
    const pgmi_config& c = x->c;
    hipStream_t s = r.s;
    const int B = r.B, L = r.L, H = c.t_hidden, NH = c.t_heads, HD = c.t_head_dim;
    const float eps = c.t_rms_eps;
    const TextLayerW& w = x->w.t[i];
    uint16_t* const lastrows = run_lastrows(x, r);
    AttnArgs a = lm_attn_args(x, r, i);
    a.q = x->Qr + (size_t)(L - 1) * NH * HD;
    a.o = x->dAO; a.o_b_stride = (long)H;
    a.Lq = 1;
    HIPCHK(hipMemcpy2DAsync(lastrows, (size_t)H * 2, run_hs(x, r) + (size_t)(L - 1) * H, (size_t)L * H * 2,
                            (size_t)H * 2, B, hipMemcpyDeviceToDevice, s));
    if (r.kv_start + L <= c.max_kv) {
        // one query row over the prompt's keys: the decode step's flash-decoding (64-key chunks
        // in parallel, kv_len from a device step record set by a memset node) and its o_proj
        // GEMV with the chunk combine in the prologue; a single 16-row prefill workgroup
        // would walk every key alone
        a.Lk = 0;
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&x->pstep->kv_len), r.kv_start + L - 1, 1, s));
        a.mask = x->d_zero; a.mask_b_stride = 0; a.mask_k_stride = 0; a.mask_round = 1;
        attention_decode(s, a, x->pstep, r.kv_start + L, x->opart, x->max_chunks);
        gemv_o_attn(s, B, NH, x->opart, x->max_chunks, x->pstep, w.o, H, lastrows,
                    B >= gemv_mf_min_batch() ? x->dAO : nullptr);
    } else {
        attention_prefill(s, 256, a);
        gemv_res(s, B, NH * HD, x->dAO, w.o, H, lastrows, x->ws);
    }
    gemv_geglu(s, B, lastrows, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, nullptr, nullptr,
               pk_use(x, B, PK_GATE_UP, w.pk_gate_up));
    gemv_res(s, B, c.t_intermediate, x->dACT, w.down, H, lastrows, x->ws, pk_use(x, B, PK_DOWN, w.pk_down));
    return 0;
}

// the group's logits: every row's (logits_rows 0, Tn holds the final RMSNorm, modeling_gemma.py:379) or each
// sequence's last row's (lastrows: copied or gathered here, or lm_last_row_tail's)
static int lm_logits(pgmi_ctx* x, const PrefillRun& r) {
    const pgmi_config& c = x->c;
    hipStream_t s = r.s;
    const int B = r.B, L = r.L, H = c.t_hidden;
    const uint16_t* E = x->w.embed;
    uint16_t* const lastrows = run_lastrows(x, r);
    float* const logits = r.logits + (size_t)r.b0 * (r.logits_rows == 0 ? L : 1) * c.t_vocab;
    if (r.logits_rows == 0) {
        EpiArgs l{};
        l.out_f32 = logits; l.ldo = c.t_vocab;
        gemm(s, run_tn(x, r), H, E, H, B * L, c.t_vocab, H, EPI_F32, l, x->ws, x->ws_bytes);
    } else {
        if (r.ragged)  // each row's last real token, lens[b] - 1
            gather_last_rows(s, run_hs(x, r), B, L, H, x->d_rlens + r.b0, lastrows);
        else if (!run_last_only(x, r))
            HIPCHK(hipMemcpy2DAsync(lastrows, (size_t)H * 2, run_hs(x, r) + (size_t)(L - 1) * H, (size_t)L * H * 2,
                                    (size_t)H * 2, B, hipMemcpyDeviceToDevice, s));
        int nparts = 0;
        gemv_logits(s, B, lastrows, x->w.final_norm, c.t_rms_eps, E, c.t_vocab, logits, x->pmax, x->pidx, &nparts,
                    nullptr, nullptr, nullptr, nullptr, 1, pk_use(x, B, PK_LM_HEAD, x->w.pk_embed));
    }
    return 0;
}

static int lm_rows(pgmi_ctx* x, const PrefillRun& r) {
    const int layers = x->c.t_layers;
    int rc;
    lm_in_norm(x, r);
    for (int i = 0; i < layers; ++i) {
        lm_qkv(x, r, i);
        if (run_last_only(x, r) && i + 1 == layers) {
            if ((rc = lm_last_row_tail(x, r, i))) return rc;
            break;
        }
        lm_attn(x, r, i);
        lm_o_proj(x, r, i);
        lm_gate_up(x, r, i);
        lm_down(x, r, i);
    }
    if ((rc = lm_logits(x, r))) return rc;
    LAUNCHCHK();
    return 0;
}

// The batched form's RMSNorms: computed once per row -- the input norm by the down projection's combine for
// the next layer (k_mf_combine_norm; q|k|v reads dHn unstaged), the post-attention norm from o_proj's 16-column
// partial sums of squares, applied by gate|up as it loads h (default) -- or each projection stages and
// normalises its rows itself (pgmi_set_decode_staged_norm,
// tested by test_batch_rows_teacher_forced_vs_own_reference[8-1]).  Round 4, the unstaged form reading rows
// normalised by separate passes against the staged form: equal
// while the weight streams were non-temporal (B = 8 step 1.5449 vs 1.5452 ms); with the default cache policy
// (kernels_gemv_mfma.hip PGMI_MF_NT) the unstaged form wins, same box: 1.4523 / 1.4550 -> 1.4330 / 1.4320 ms
static bool mf_staged(const pgmi_ctx* x) { return x->mf_staged > 0; }

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

static StepState* run_step(const pgmi_ctx* x, const DecodeRun& r) { return r.ragged ? x->rstep : x->step; }
// B <= 2: the embedding row is read by layer 0's q|k|v GEMV itself (one launch fewer per step)
static bool run_folds(const pgmi_ctx* x, const DecodeRun& r) {
    return !r.embeds && r.ids && gemv_qkv_folds_embed(r.B) && x->c.t_layers > 0;
}
// B >= 3 (MFMA projections): every RMSNorm is computed once per row -- the input norm fused into the
// down projection's combine for the next layer (q|k|v reads dHn unstaged), the post-attention norm's
// sums of squares written by o_proj's epilogue (dSS) and applied by gate|up as it loads h.  (Round 5,
// the input norm the same way -- the down combine writing partials, q|k|v normalising on load: q|k|v
// 5.97 -> 7.59 us for a combine no shorter, 4.63 -> 4.72 us; with the combine inside the down launch,
// B = 8 step 1.437 -> 1.446-1.465 ms, same box.)
static bool run_mf(const pgmi_ctx* x, const DecodeRun& r) { return r.B >= gemv_mf_min_batch() && !mf_staged(x); }
static float embed_normalizer(const pgmi_ctx* x) { return bf16_round_host(std::sqrt((float)x->c.t_hidden)); }

// the step's entry: h (unless layer 0's q|k|v folds the embedding) and, unstaged, layer 0's normed rows
static void decode_head(pgmi_ctx* x, const DecodeRun& r) {
    const pgmi_config& c = x->c;
    const int H = c.t_hidden;
    // given input rows (a caller's merge, pgmi_decode_embeds): h = rows x bf16(sqrt(hidden)) (modeling_gemma.py:367-368)
    if (r.embeds) scale_rows(r.s, r.embeds, (long)r.B * H, embed_normalizer(x), x->dH);
    else if (r.ids && !run_folds(x, r))
        embed_rows(r.s, r.ids, r.B, x->w.embed, H, embed_normalizer(x), c.pad_token_id, x->dH);
    if (run_mf(x, r) && c.t_layers > 0) rows_norm(r.s, x->dH, x->w.t[0].in_norm, c.t_rms_eps, r.B, H, x->dHn);
}

// layer i's launches; stage 0: all of them, 1..4: that one alone (1 q|k|v, 2 attention + o_proj,
// 3 gate|up, 4 down -- the stage numbers of pgmi_debug_decode_stage)
static void decode_layer(pgmi_ctx* x, const DecodeRun& r, int i, int stage = 0) {
    const pgmi_config& c = x->c;
    hipStream_t s = r.s;
    const int B = r.B;
    StepState* const st = run_step(x, r);
    const int sts = r.ragged ? 1 : 0;
    const int H = c.t_hidden, NH = c.t_heads, NKV = c.t_kv_heads, HD = c.t_head_dim;
    const float eps = c.t_rms_eps;
    const long kvd = (long)NKV * HD, kvb = (long)r.kv_max * kvd;
    uint16_t* kvp = reinterpret_cast<uint16_t*>(r.kv);
    const bool mf = run_mf(x, r);
    const auto on = [stage](int k) { return stage == 0 || stage == k; };
    uint16_t* Kc = kvp + ((long)(i * 2 + 0) * r.kv_batch) * kvb;
    uint16_t* Vc = kvp + ((long)(i * 2 + 1) * r.kv_batch) * kvb;
    // w.mf_*: the fragment-major images of this layer's weights (ensure_mf_image), null until built
    const TextLayerW& w = x->w.t[i];
    if (on(1)) {
        const EmbedFold emb{r.ids, x->w.embed, embed_normalizer(x), c.pad_token_id, x->dH};
        gemv_qkv(s, B, NH, NKV, mf ? x->dHn : x->dH, mf ? nullptr : w.in_norm, eps, w.qkv, x->cosT, x->sinT,
                 c.t_max_pos, st, x->dQ, Kc, Vc, kvb, x->ws, (run_folds(x, r) && i == 0) ? &emb : nullptr, w.mf_qkv,
                 sts);
    }
    if (on(2)) {
        AttnArgs a{};
        a.q = x->dQ; a.q_b_stride = (long)NH * HD; a.q_row_stride = NH * HD; a.q_head_stride = HD;
        a.k = Kc; a.k_b_stride = kvb; a.k_row_stride = (int)kvd; a.k_head_stride = HD;
        a.v = Vc; a.v_b_stride = kvb; a.v_row_stride = (int)kvd; a.v_head_stride = HD;
        a.o = x->dAO; a.o_b_stride = (long)H; a.o_row_stride = H; a.o_head_stride = HD;
        a.Lq = 1; a.Lk = 0; a.G = NH / NKV; a.n_kv = NKV; a.B = B; a.scale = 1.0f / std::sqrt((float)HD);
        if (r.masked) {  // the staged additive mask (pgmi_decode_embeds_dev), row stride max_kv
            a.mask = x->d_mask; a.mask_b_stride = c.max_kv; a.mask_k_stride = 1; a.mask_round = r.masked == 1;
        } else {
            a.mask = x->d_zero; a.mask_b_stride = 0; a.mask_k_stride = 0; a.mask_round = 1;
        }
        attention_decode(s, a, st, r.launch_keys, x->opart, x->max_chunks, sts);
        gemv_o_attn(s, B, NH, x->opart, x->max_chunks, st, w.o, H, x->dH, B >= gemv_mf_min_batch() ? x->dAO : nullptr,
                    mf ? x->dSS : nullptr, w.mf_o, sts);
    }
    if (mf) {
        // the post-attention RMSNorm: its sums of squares come from o_proj's epilogue (dSS), gate|up
        // normalises h on load (no k_rows_norm pass: B = 8 step -5 us per layer)
        if (on(3))
            gemv_geglu(s, B, x->dH, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, x->dSS, w.mf_gate_up);
        if (on(4))
            gemv_res_norm(s, B, c.t_intermediate, x->dACT, w.down, H, x->dH, x->ws,
                          i + 1 < c.t_layers ? x->w.t[i + 1].in_norm : nullptr, eps, x->dHn, w.mf_down);
        return;
    }
    if (on(3))
        gemv_geglu(s, B, x->dH, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, nullptr, nullptr,
                   pk_use(x, B, PK_GATE_UP, w.pk_gate_up));
    if (on(4))
        gemv_res(s, B, c.t_intermediate, x->dACT, w.down, H, x->dH, x->ws, pk_use(x, B, PK_DOWN, w.pk_down));
}

// final norm + lm_head + argmax.  The step's last work also advances the device step state (pgmi_decode
// skips its host-side set when the next call continues the sequence): lm_head's last workgroup, or argmax_finish
static void decode_tail(pgmi_ctx* x, const DecodeRun& r, float* logits, int64_t* next_ids, int64_t* hist) {
    const pgmi_config& c = x->c;
    StepState* const st = run_step(x, r);
    const int adv_n = r.ragged ? r.B : 1;
    int nparts = 0;
    int64_t* nx = next_ids ? next_ids : x->d_next;
    if (!gemv_logits(r.s, r.B, x->dH, x->w.final_norm, c.t_rms_eps, x->w.embed, c.t_vocab, logits, x->pmax, x->pidx,
                     &nparts, x->lm_done, nx, st, hist, adv_n, pk_use(x, r.B, PK_LM_HEAD, x->w.pk_embed)))
        argmax_finish(r.s, r.B, x->pmax, x->pidx, nparts, nx, st, hist, adv_n);
}

static int decode_body(pgmi_ctx* x, hipStream_t s, const int64_t* ids, int B, void* kv, int kv_batch, int kv_max,
                       int launch_keys, float* logits, int64_t* next_ids, const uint16_t* embeds = nullptr,
                       int masked = 0, int64_t* hist = nullptr, bool ragged = false) {
    const DecodeRun r{s, ids, embeds, B, kv, kv_batch, kv_max, launch_keys, masked, ragged};
    decode_head(x, r);
    for (int i = 0; i < x->c.t_layers; ++i) decode_layer(x, r, i);
    decode_tail(x, r, logits, next_ids, hist);
    return launcher_error();  // (inside a capture too: a step with a launch missing is never instantiated)
}

int pgmi_prefill_probe(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (on && x->probe_ev.empty()) {
        x->probe_ev.resize((size_t)4 * x->c.t_layers);
        for (auto& e : x->probe_ev) HIPCHK(hipEventCreate(&e));
    }
    // the probe records its events in eager forwards: prefill graphs are off while it is on, and the
    // caller's own setting (pgmi_set_prefill_graph) is restored when it is turned off
    if (on && !x->probe_on) x->graph_before_probe = x->prefill_graph;
    if (!on && x->probe_on) x->prefill_graph = x->graph_before_probe;
    x->probe_on = on != 0;
    if (x->probe_on) x->prefill_graph = false;
    x->pgraphs.clear();
    return 0;
}

int pgmi_prefill_probe_times(pgmi_ctx* x, float* us, int n) {
    if (!x || !us) return fail(PGMI_E_ARG, "null argument");
    if (x->probe_ev.empty()) return fail(PGMI_E_STATE, "pgmi_prefill_probe(ctx, 1) has not been called");
    const int L = x->c.t_layers;
    if (n < 2 * L) return fail(PGMI_E_ARG, "us needs 2 x layers entries");
    HIPCHK(hipEventSynchronize(x->probe_ev.back()));
    for (int i = 0; i < L; ++i) {
        float a = 0.f, b = 0.f;
        HIPCHK(hipEventElapsedTime(&a, x->probe_ev[4 * i], x->probe_ev[4 * i + 1]));
        HIPCHK(hipEventElapsedTime(&b, x->probe_ev[4 * i + 2], x->probe_ev[4 * i + 3]));
        us[i] = a * 1e3f;
        us[L + i] = b * 1e3f;
    }
    return 0;
}

int pgmi_set_decode_staged_norm(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    x->mf_staged = on < 0 ? -1 : on != 0;
    x->dgraphs.clear();  // captured steps hold the other form's launches
    return 0;
}

int pgmi_set_prefill_graph(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (x->probe_on) x->graph_before_probe = on != 0;  // applied when the probe is turned off
    else x->prefill_graph = on != 0;
    x->pgraphs.clear();
    return 0;
}

// device-side inputs of a decode step over merged rows (pgmi_decode_embeds_dev): the rotary position
// and the additive mask come from the caller's merge outputs without a host read
struct DevStepIn {
    const void* pos = nullptr;  // (B, 1) position tensor on the device, dtype code (set_step_dev)
    int pos_dtype = 0;
    const void* mask = nullptr;  // additive mask rows (kv_len + 1 keys each)
    int mask_dtype = 0;
    long mask_b_stride = 0;
};

// The fragment-major images of every layer's gate|up, q|k|v, o_proj and down weights that the batched (B >= 3)
// decode projections read (kernels_gemv_mfma.hip; round 5), (re)built on stream s after a pgmi_prepare.  If the
// 3.96 GB (at the 3B shapes) cannot be allocated the batched decode reads the row-major weights instead (the
// same values in the same lanes: bit-identical results, slower), so the context stays usable.
static int ensure_mf_image(pgmi_ctx* x, hipStream_t s) {
    if (!x->mfw_dirty) return 0;
    const pgmi_config& c = x->c;
    const size_t I = c.t_intermediate, H = c.t_hidden, QKVN = (size_t)(c.t_heads + 2 * c.t_kv_heads) * c.t_head_dim,
                 OK = (size_t)c.t_heads * c.t_head_dim, per = 2 * I * H + QKVN * H + H * OK + H * I;
    x->mfw_dirty = false;
    if (!x->mfw) {
        void* p = nullptr;
        if (hipMalloc(&p, per * c.t_layers * sizeof(uint16_t)) != hipSuccess) {
            (void)hipGetLastError();  // out of memory: keep the row-major form
            x->mfw_alloc_failed = true;  // (reported by pgmi_decode_packed_info)
            return 0;
        }
        x->mfw_alloc_failed = false;
        x->allocs.push_back(p);
        x->mfw = reinterpret_cast<uint16_t*>(p);
        x->dgraphs.clear();  // steps captured before held the row-major launches
    }
    // the image's layout, defined here alone: [layer][gate|up 2 I x H | q|k|v QKVN x H | o_proj H x OK | down H x I]
    for (int i = 0; i < c.t_layers; ++i) {
        TextLayerW& w = x->w.t[i];
        uint16_t *gu = x->mfw + per * i, *qkv = gu + 2 * I * H, *o = qkv + QKVN * H, *down = o + H * OK;
        mf_swizzle(s, w.gate_up, (int)(2 * I), (int)H, gu);  // gate rows, then up rows
        mf_swizzle(s, w.qkv, (int)QKVN, (int)H, qkv, true);  // q|k|v in the GEMV's row order
        mf_swizzle(s, w.o, (int)H, (int)OK, o);
        mf_swizzle(s, w.down, (int)H, (int)I, down);
        w.mf_gate_up = gu; w.mf_qkv = qkv; w.mf_o = o; w.mf_down = down;
    }
    LAUNCHCHK();
    return 0;
}

// captured decode steps of B <= 2 rows (key[0] = B, decode_step): they hold the launches of the other weight form
static void drop_small_batch_graphs(GraphCache& g) {
    for (auto it = g.map.begin(); it != g.map.end();) {
        if (!it->first.empty() && it->first[0] <= 2) {
            if (it->second) (void)hipGraphExecDestroy(it->second);
            it = g.map.erase(it);
        } else {
            ++it;
        }
    }
}

// The 13-bit images (pack13.h) that the streaming GEMVs of the B <= 2 decode step read instead of the bf16 rows:
// every layer's gate|up (one 2 I x H tensor) and down, and the tied embedding as lm_head reads it -- 2 L + 1
// candidate tensors, 13/16 of their bytes (3.80 GB beside the resident bf16 weights at the 3B shapes).  (Re)built
// on stream s by the first such step after a pgmi_prepare, outside any capture: pass one scans each tensor's
// exponent range, the host reads the 2 L + 1 results (one stream synchronisation) and packs the tensors that fit;
// a tensor that does not fit keeps the bf16 kernel, as does a whole kind whose buffer cannot be allocated.
static int ensure_pk_image(pgmi_ctx* x, hipStream_t s, int B) {
    const int want = pk_mask_for(x, B) & ~x->pk_done;
    if (!want) return 0;
    const pgmi_config& c = x->c;
    // the PK kernels are the K = 2048 / K = 16384 forms
    if (c.t_hidden != 2048 || c.t_intermediate != 16384) {
        x->pk_done |= want;
        return 0;
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return 0;  // a caller's capture: this step reads the bf16 rows, a later one builds the image
    }
    const int L = c.t_layers;
    const int64_t I = c.t_intermediate, H = c.t_hidden, V = c.t_vocab;
    struct Cand { int kind; const uint16_t* W; int64_t rows, K; PkW* dst; uint8_t* out; };
    std::vector<Cand> cands;
    const int64_t gu_b = pk_image_bytes(2 * I, H), dn_b = pk_image_bytes(H, I), em_b = pk_image_bytes(V, H);
    const int64_t kind_bytes[3] = {gu_b * L, dn_b * L, em_b};
    int got = 0;
    for (int k = 0; k < 3; ++k) {
        if (!(want & (1 << k)) || kind_bytes[k] == 0) continue;
        if (!x->pk_buf[k]) {
            void* p = nullptr;
            if (hipMalloc(&p, (size_t)kind_bytes[k]) != hipSuccess) {
                (void)hipGetLastError();  // out of memory: this kind keeps the bf16 kernels
                x->pk_alloc_failed = true;
                continue;
            }
            x->allocs.push_back(p);
            x->pk_buf[k] = reinterpret_cast<uint8_t*>(p);
        }
        got |= 1 << k;
    }
    for (int i = 0; i < L; ++i) {
        TextLayerW& w = x->w.t[i];
        if (got & PK_GATE_UP) cands.push_back({PK_GATE_UP, w.gate_up, 2 * I, H, &w.pk_gate_up, x->pk_buf[0] + gu_b * i});
        if (got & PK_DOWN) cands.push_back({PK_DOWN, w.down, H, I, &w.pk_down, x->pk_buf[1] + dn_b * i});
    }
    if (got & PK_LM_HEAD) cands.push_back({PK_LM_HEAD, x->w.embed, V, H, &x->w.pk_embed, x->pk_buf[2]});
    if (!cands.empty()) {
        const size_t n = cands.size(), cap_n = (size_t)2 * L + 1;
        if (!x->pk_stat) {
            void* p = nullptr;
            HIPCHK(hipMalloc(&p, cap_n * 2 * sizeof(unsigned)));
            x->allocs.push_back(p);
            x->pk_stat = reinterpret_cast<unsigned*>(p);
        }
        // stat[2 t] = largest exponent field (from 0), stat[2 t + 1] = smallest one >= 1 (from 0xFFFFFFFF)
        std::vector<unsigned> st(2 * n);
        for (size_t t = 0; t < n; ++t) { st[2 * t] = 0; st[2 * t + 1] = 0xFFFFFFFFu; }
        HIPCHK(hipMemcpyAsync(x->pk_stat, st.data(), st.size() * sizeof(unsigned), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));  // (st is reused below)
        for (size_t t = 0; t < n; ++t) pk_scan(s, cands[t].W, (long)(cands[t].rows * cands[t].K), x->pk_stat + 2 * t);
        LAUNCHCHK();
        HIPCHK(hipMemcpyAsync(st.data(), x->pk_stat, st.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t t = 0; t < n; ++t) {
            const int e_hi = (int)st[2 * t], e_lo = st[2 * t + 1] > 255u ? 256 : (int)st[2 * t + 1];
            if (!pk_fits(e_hi, e_lo)) {
                *cands[t].dst = PkW{};
                continue;
            }
            pk_pack(s, cands[t].W, (long)cands[t].rows, (int)cands[t].K, e_hi, cands[t].out);
            cands[t].dst->img = cands[t].out;
            cands[t].dst->base2 = pk_base2(e_hi);
        }
        LAUNCHCHK();
    }
    x->pk_done |= want;
    drop_small_batch_graphs(x->dgraphs);  // steps captured before held the bf16 launches
    return 0;
}

int pgmi_set_decode_packed(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (on > PK_ALL) return fail(PGMI_E_ARG, "decode_packed: 0 off, 1..7 a mask of kinds (1 gate|up, 2 down, 4 lm_head), < 0 default");
    x->pk_mask = on < 0 ? -1 : on;
    drop_small_batch_graphs(x->dgraphs);  // captured steps hold the other form's launches
    x->pgraphs.clear();                   // (a last-row-only prefill's GEMVs follow the setting)
    return 0;
}

int pgmi_decode_packed_info(const pgmi_ctx* x, int64_t* info, int n) {
    if (!x || !info) return fail(PGMI_E_ARG, "null argument");
    if (n < PGMI_PACKED_INFO_N) return fail(PGMI_E_ARG, "info needs PGMI_PACKED_INFO_N entries");
    const pgmi_config& c = x->c;
    const int64_t I = c.t_intermediate, H = c.t_hidden, V = c.t_vocab;
    const bool shapes = H == 2048 && I == 16384;
    int64_t np = 0, nr = 0, bp = 0, br = 0;
    auto count = [&](int kind, const PkW& w, int64_t rows, int64_t K) {
        if ((pk_mask_for(x, 1) & x->pk_done & kind) && w.img && shapes) { ++np; bp += pk_image_bytes(rows, K); }
        else { ++nr; br += rows * K * 2; }
    };
    for (size_t i = 0; i < x->w.t.size(); ++i) {
        count(PK_GATE_UP, x->w.t[i].pk_gate_up, 2 * I, H);
        count(PK_DOWN, x->w.t[i].pk_down, H, I);
    }
    count(PK_LM_HEAD, x->w.pk_embed, V, H);
    info[0] = pk_mask_for(x, 1); info[8] = pk_mask_for(x, 2); info[1] = np; info[2] = nr; info[3] = bp; info[4] = br;
    info[5] = x->pk_alloc_failed; info[6] = x->mfw_alloc_failed; info[7] = x->pk_done;
    return 0;
}

int pgmi_decode_packed_tensor(const pgmi_ctx* x, int kind, int layer) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (kind != PK_GATE_UP && kind != PK_DOWN && kind != PK_LM_HEAD) return fail(PGMI_E_ARG, "kind: 1 gate|up, 2 down, 4 lm_head");
    if (kind != PK_LM_HEAD && (layer < 0 || layer >= (int)x->w.t.size())) return fail(PGMI_E_ARG, "layer out of range");
    const PkW& w = kind == PK_LM_HEAD ? x->w.pk_embed : kind == PK_GATE_UP ? x->w.t[layer].pk_gate_up : x->w.t[layer].pk_down;
    return (pk_mask_for(x, 1) & x->pk_done & kind) && w.img ? 1 : 0;
}

// The format on the host, for tests (no device): e_hi / fit of n bf16 values, their image and its decode through
// the very functions the kernels use (pack13.h).  rows x K values, K a multiple of 2048.
int pgmi_pack13_scan(const uint16_t* w, int64_t n, int* e_hi, int* fits) {
    if (!w || !e_hi || !fits) return fail(PGMI_E_ARG, "null argument");
    if (n < 1) return fail(PGMI_E_ARG, "pack13: no values");
    int hi = 0, lo = 256;
    for (int64_t i = 0; i < n; ++i) {
        const int ex = (w[i] >> 7) & 0xFF;
        hi = std::max(hi, ex);
        if (ex) lo = std::min(lo, ex);
    }
    *e_hi = hi;
    *fits = pk_fits(hi, lo) ? 1 : 0;
    return 0;
}

int64_t pgmi_pack13_bytes(int64_t rows, int64_t K) {
    if (rows < 1 || K < kPkSegK || K % kPkSegK != 0) return -1;
    return pk_image_bytes(rows, K);
}

static const uint8_t* pk_host_seg(const uint8_t* image, int64_t seg) { return image + seg * kPkSegBytes; }

int pgmi_pack13_encode(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image) {
    if (!w || !image) return fail(PGMI_E_ARG, "null argument");
    if (pgmi_pack13_bytes(rows, K) < 0) return fail(PGMI_E_ARG, "pack13: K must be a positive multiple of 2048, rows >= 1");
    if (e_hi < 0 || e_hi > 255) return fail(PGMI_E_ARG, "pack13: e_hi is an exponent field (0..255)");
    for (int64_t seg = 0; seg < rows * (K / kPkSegK); ++seg)
        for (int l = 0; l < 64; ++l) {
            uint4 f[4];
            for (int ch = 0; ch < 4; ++ch) std::memcpy(&f[ch], w + seg * kPkSegK + 512 * ch + 8 * l, 16);
            const PkSeg sg = pk_encode(f, e_hi);
            uint8_t* d = image + seg * kPkSegBytes;
            std::memcpy(d + pk_off_a(l), &sg.a, 16);
            std::memcpy(d + pk_off_b(l), &sg.b, 16);
            std::memcpy(d + pk_off_n(l), &sg.n, 16);
            std::memcpy(d + pk_off_h(l), &sg.h, 4);
        }
    return 0;
}

int pgmi_pack13_decode(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w) {
    if (!w || !image) return fail(PGMI_E_ARG, "null argument");
    if (pgmi_pack13_bytes(rows, K) < 0) return fail(PGMI_E_ARG, "pack13: K must be a positive multiple of 2048, rows >= 1");
    if (e_hi < 0 || e_hi > 255) return fail(PGMI_E_ARG, "pack13: e_hi is an exponent field (0..255)");
    const unsigned b2 = pk_base2(e_hi);
    for (int64_t seg = 0; seg < rows * (K / kPkSegK); ++seg)
        for (int l = 0; l < 64; ++l) {
            const uint8_t* d = pk_host_seg(image, seg);
            PkSeg sg;
            std::memcpy(&sg.a, d + pk_off_a(l), 16);
            std::memcpy(&sg.b, d + pk_off_b(l), 16);
            std::memcpy(&sg.n, d + pk_off_n(l), 16);
            std::memcpy(&sg.h, d + pk_off_h(l), 4);
            for (int ch = 0; ch < 4; ++ch) {
                const uint4 f = pk_chunk(sg, ch, b2);
                std::memcpy(w + seg * kPkSegK + 512 * ch + 8 * l, &f, 16);
            }
        }
    return 0;
}

// ---------------------------------------------------------------- LoRA adapters (pgmi.h; the rule: lora.h)
static LoraAdapter* lora_get(pgmi_ctx* x, int id) {
    return x && id >= 0 && id < PGMI_LORA_MAX && x->lora[id].used ? &x->lora[id] : nullptr;
}

static const LoraTarget* lora_find(const LoraAdapter* a, int slot) {
    if (a)
        for (const LoraTarget& t : a->targets)
            if (t.slot == slot) return &t;
    return nullptr;
}

int pgmi_lora_create(pgmi_ctx* x, int* id) {
    if (!x || !id) return fail(PGMI_E_ARG, "null argument");
    for (int i = 0; i < PGMI_LORA_MAX; ++i)
        if (!x->lora[i].used) {
            x->lora[i] = LoraAdapter{};
            x->lora[i].used = true;
            *id = i;
            return 0;
        }
    return fail(PGMI_E_STATE, "a context holds at most " + std::to_string(PGMI_LORA_MAX) + " LoRA adapters: free one first");
}

// one factor to its resident fp32 form: host values are widened here, device values by k_lora_widen
static int lora_upload(pgmi_ctx* x, hipStream_t st, const void* src, int dtype, int64_t n, int on_device, float** out) {
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)n * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PGMI_E_NOMEM, "LoRA factor: hipMalloc of " + std::to_string(n * 4) + " bytes");
    }
    *out = reinterpret_cast<float*>(p);
    if (on_device) {
        lora_widen(st, src, dtype, (long)n, *out);
        LAUNCHCHK();
        return 0;
    }
    std::vector<float> tmp;
    const float* h = reinterpret_cast<const float*>(src);
    if (dtype != PGMI_DTYPE_F32) {
        tmp.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            tmp[i] = dtype == PGMI_DTYPE_F16 ? (float)reinterpret_cast<const _Float16*>(src)[i]
                                             : lora_bits_f((uint32_t)reinterpret_cast<const uint16_t*>(src)[i] << 16);
        h = tmp.data();
    }
    HIPCHK(hipMemcpyAsync(*out, h, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (tmp, and the caller's buffer, may go after the return)
    return 0;
}

int pgmi_lora_add(pgmi_ctx* x, int id, const char* name, const void* A, int a_dtype, const int64_t* a_shape,
                  const void* B, int b_dtype, const int64_t* b_shape, float scaling, int on_device, void* stream) {
    if (!x || !name || !A || !B || !a_shape || !b_shape) return fail(PGMI_E_ARG, "null argument");
    LoraAdapter* a = lora_get(x, id);
    if (!a) return fail(PGMI_E_ARG, "unknown LoRA adapter id " + std::to_string(id));
    for (int dt : {a_dtype, b_dtype})
        if (dt != PGMI_DTYPE_BF16 && dt != PGMI_DTYPE_F16 && dt != PGMI_DTYPE_F32) return fail(PGMI_E_ARG, "unsupported dtype");
    auto it = x->index.find(name);
    if (it == x->index.end()) return fail(PGMI_E_ARG, std::string("unknown weight ") + name);
    const Slot& s = x->slots[it->second];
    if (!lora_targetable(s))
        return fail(PGMI_E_ARG, std::string(name) + " is not the 2-D weight of a Linear module: not a LoRA target");
    const int64_t r = a_shape[0];
    if (r < 1 || r > kLoraMaxRank) return fail(PGMI_E_ARG, std::string(name) + ": LoRA rank " + std::to_string(r) + " outside [1, 256]");
    if (a_shape[1] != s.shape[1] || b_shape[0] != s.shape[0] || b_shape[1] != r)
        return fail(PGMI_E_ARG, std::string(name) + ": lora_A must be [r][" + std::to_string(s.shape[1]) + "] and lora_B [" +
                                    std::to_string(s.shape[0]) + "][r]");
    if (s.shape[1] % 8 != 0) return fail(PGMI_E_ARG, std::string(name) + ": K must be a multiple of 8");
    if (lora_find(a, it->second)) return fail(PGMI_E_ARG, std::string(name) + ": the adapter already has this target");
    if (x->lora_active == id) return fail(PGMI_E_STATE, kLoraActiveMsg);
    HIPCHK(hipSetDevice(x->device));
    hipStream_t st = (hipStream_t)stream;
    LoraTarget t{it->second, (int)r, scaling, nullptr, nullptr};
    int rc = lora_upload(x, st, A, a_dtype, r * s.shape[1], on_device, &t.A);
    if (!rc) rc = lora_upload(x, st, B, b_dtype, s.shape[0] * r, on_device, &t.B);
    if (!rc && on_device && hipStreamSynchronize(st) != hipSuccess) rc = fail(PGMI_E_HIP, "LoRA factor upload");
    if (rc) {
        if (t.A) (void)hipFree(t.A);
        if (t.B) (void)hipFree(t.B);
        return rc;
    }
    a->targets.push_back(t);
    a->factor_bytes += (r * s.shape[1] + s.shape[0] * r) * (int64_t)sizeof(float);
    return 0;
}

int pgmi_lora_active(const pgmi_ctx* x) { return x ? x->lora_active : -1; }

int pgmi_lora_info(const pgmi_ctx* x, int id, int64_t* info, int n) {
    if (!x || !info) return fail(PGMI_E_ARG, "null argument");
    const LoraAdapter* a = lora_get(const_cast<pgmi_ctx*>(x), id);
    if (!a) return fail(PGMI_E_ARG, "unknown LoRA adapter id " + std::to_string(id));
    if (n < PGMI_LORA_INFO_N) return fail(PGMI_E_ARG, "info needs PGMI_LORA_INFO_N entries");
    int64_t pristine = 0;
    for (const LoraTarget& t : a->targets) {
        auto it = x->lora_pristine.find(t.slot);
        if (it != x->lora_pristine.end() && it->second.copy) pristine += x->slots[t.slot].numel * 2;
    }
    info[0] = (int64_t)a->targets.size(); info[1] = a->factor_bytes; info[2] = pristine;
    return 0;
}

// The switch: restore what the outgoing adapter alone had changed, merge the incoming one's targets from their
// pristine copies, then mark what was derived from a changed tensor.  Everything that can be refused is refused,
// and every missing copy allocated, before the slab is touched.
int pgmi_lora_set(pgmi_ctx* x, int id, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null argument");
    LoraAdapter* in = id == -1 ? nullptr : lora_get(x, id);
    if (id != -1 && !in) return fail(PGMI_E_ARG, "unknown LoRA adapter id " + std::to_string(id));
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound");
    HIPCHK(hipSetDevice(x->device));
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(PGMI_E_STATE, "pgmi_lora_set inside a stream capture");
    HIPCHK(hipDeviceSynchronize());
    if (id == x->lora_active) return 0;
    const LoraAdapter* out = x->lora_active >= 0 ? &x->lora[x->lora_active] : nullptr;
    if (in)
        for (const LoraTarget& t : in->targets) {
            LoraPristine& p = x->lora_pristine[t.slot];
            if (p.copy) continue;
            void* d = nullptr;
            if (hipMalloc(&d, (size_t)x->slots[t.slot].numel * 2) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PGMI_E_NOMEM, "pristine copy of " + x->slots[t.slot].name);
            }
            p.copy = reinterpret_cast<uint16_t*>(d);
            p.valid = false;
        }
    std::vector<int> changed;
    if (out)
        for (const LoraTarget& t : out->targets) {
            if (lora_find(in, t.slot)) continue;
            const Slot& sl = x->slots[t.slot];
            const LoraPristine& p = x->lora_pristine[t.slot];  // valid: it was merged from
            HIPCHK(hipMemcpyAsync(x->slab + sl.off, p.copy, (size_t)sl.numel * 2, hipMemcpyDeviceToDevice, s));
            changed.push_back(t.slot);
        }
    x->lora_active = -1;  // (until the merges are enqueued: a failure below leaves no adapter claimed)
    if (in)
        for (const LoraTarget& t : in->targets) {
            const Slot& sl = x->slots[t.slot];
            LoraPristine& p = x->lora_pristine[t.slot];
            uint16_t* w = reinterpret_cast<uint16_t*>(x->slab + sl.off);
            if (!p.valid) {  // (never a target of `out`: those copies are valid) the slab holds this tensor's base
                HIPCHK(hipMemcpyAsync(p.copy, w, (size_t)sl.numel * 2, hipMemcpyDeviceToDevice, s));
                p.valid = true;
            }
            lora_merge(s, p.copy, (int)sl.shape[0], (int)sl.shape[1], t.A, t.B, t.r, t.scaling, w);
            changed.push_back(t.slot);
        }
    LAUNCHCHK();
    x->lora_active = id;
    // derived tensors: only what was built from a changed tensor
    int kinds = 0;
    for (int slot : changed) {
        const std::string& nm = x->slots[slot].name;
        if (nm.compare(0, 28, "language_model.model.layers.") != 0) continue;
        if (mf_wanted(x->c)) x->mfw_dirty = true;  // rebuilt in place by the next B >= 3 step: its graphs stay valid
        if (ends_with(nm, "mlp.gate_proj.weight") || ends_with(nm, "mlp.up_proj.weight")) kinds |= PK_GATE_UP;
        if (ends_with(nm, "mlp.down_proj.weight")) kinds |= PK_DOWN;
    }
    if (kinds & x->pk_done) {
        pk_forget_kinds(x, kinds);
        drop_small_batch_graphs(x->dgraphs);  // they hold the old images' launches (packed or raw, exponent base)
        x->pgraphs.clear();                   // (a last-row-only prefill's GEMVs likewise)
    }
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int pgmi_lora_free(pgmi_ctx* x, int id) {
    if (!x) return fail(PGMI_E_ARG, "null argument");
    LoraAdapter* a = lora_get(x, id);
    if (!a) return fail(PGMI_E_ARG, "unknown LoRA adapter id " + std::to_string(id));
    if (x->lora_active == id) return fail(PGMI_E_STATE, kLoraActiveMsg);
    if (!a->targets.empty()) {
        HIPCHK(hipSetDevice(x->device));
        HIPCHK(hipDeviceSynchronize());
    }
    for (LoraTarget& t : a->targets) { (void)hipFree(t.A); (void)hipFree(t.B); }
    *a = LoraAdapter{};
    // pristine copies no remaining adapter targets go too
    for (auto it = x->lora_pristine.begin(); it != x->lora_pristine.end();) {
        bool wanted = false;
        for (const LoraAdapter& o : x->lora) wanted = wanted || (o.used && lora_find(&o, it->first));
        if (wanted) { ++it; continue; }
        if (it->second.copy) (void)hipFree(it->second.copy);
        it = x->lora_pristine.erase(it);
    }
    return 0;
}

int pgmi_lora_merge_host(const uint16_t* W, int64_t N, int64_t K, const float* A, const float* B, int r, float scaling,
                         uint16_t* out) {
    if (!W || !A || !B || !out) return fail(PGMI_E_ARG, "null argument");
    if (N < 1 || K < 1) return fail(PGMI_E_ARG, "lora_merge: N, K >= 1");
    if (r < 1 || r > kLoraMaxRank) return fail(PGMI_E_ARG, "lora_merge: rank outside [1, 256]");
    for (int64_t n = 0; n < N; ++n)
        for (int64_t k = 0; k < K; ++k) {
            float acc = 0.0f;
            for (int j = 0; j < r; ++j) acc = lora_step(acc, B[n * r + j], A[(int64_t)j * K + k]);
            out[n * K + k] = lora_finish(W[n * K + k], acc, scaling);
        }
    return 0;
}

int pgmi_op_lora_merge(pgmi_ctx* x, const void* W, int N, int K, const void* A, const void* B, int r, float scaling,
                       void* out, void* stream) {
    if (!x || !W || !A || !B || !out) return fail(PGMI_E_ARG, "null argument");
    if (N < 1 || K < 8 || K % 8 != 0) return fail(PGMI_E_ARG, "lora_merge: N >= 1, K a positive multiple of 8");
    if (r < 1 || r > kLoraMaxRank) return fail(PGMI_E_ARG, "lora_merge: rank outside [1, 256]");
    for (const void* p : {W, A, B, (const void*)out})
        if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return fail(PGMI_E_ARG, "lora_merge: tensors must be 16-byte aligned");
    HIPCHK(hipSetDevice(x->device));
    (void)pgmi::launch_error_take(nullptr);
    lora_merge((hipStream_t)stream, reinterpret_cast<const uint16_t*>(W), N, K, reinterpret_cast<const float*>(A),
               reinterpret_cast<const float*>(B), r, scaling, reinterpret_cast<uint16_t*>(out));
    LAUNCHCHK();
    return 0;
}

static int decode_step(pgmi_ctx* x, const int64_t* ids, const void* embeds, int B, void* kv, int kv_batch, int kv_max,
                       int kv_len, int position, float* logits, int64_t* next_ids, int use_graph, void* stream,
                       const DevStepIn* dev = nullptr, int n_steps = 1, int64_t* tokens = nullptr,
                       const int32_t* r_kv = nullptr, const int32_t* r_pos = nullptr) {
    int rc;
    // ragged (pgmi_decode_ragged): host arrays of each row's KV write row and rotary position; kv_len is
    // then the largest row's (it sizes the eager launches' attention grid)
    const bool ragged = r_kv != nullptr;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (B < 1 || B > c.max_batch || B > kv_batch) return fail(PGMI_E_ARG, "batch exceeds capacity");
    if (n_steps < 1) return fail(PGMI_E_ARG, "n_steps must be >= 1");
    if (n_steps > 1 && (!ids || embeds || dev)) return fail(PGMI_E_ARG, "multi-step decode: token ids only");
    if (ragged) {
        if (!r_pos) return fail(PGMI_E_ARG, "null argument");
        kv_len = 0;
        for (int b = 0; b < B; ++b) {
            if (r_kv[b] < 0 || (long)r_kv[b] + n_steps - 1 >= kv_max)
                return fail(PGMI_E_ARG, "KV cache capacity exceeded (a row's kv_lens[b] + n_steps > kv_max)");
            kv_len = std::max(kv_len, (int)r_kv[b]);
        }
    }
    if (kv_len < 0 || (long)kv_len + n_steps - 1 >= kv_max) return fail(PGMI_E_ARG, "KV cache capacity exceeded");
    if (kv_max > c.max_kv) return fail(PGMI_E_ARG, "kv_max exceeds config max_kv");
    if ((!ids && !embeds) || !kv || !logits) return fail(PGMI_E_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (B >= gemv_mf_min_batch() && (rc = ensure_mf_image(x, s))) return rc;
    if (B < gemv_mf_min_batch() && (rc = ensure_pk_image(x, s, B))) return rc;
    int masked = 0;
    if (dev) {
        // position read on the device; the host no longer knows it, so the next call sets the state again
        set_step_dev(s, x->step, kv_len, dev->pos, dev->pos_dtype);
        if (dev->mask) {
            stage_mask(s, dev->mask, dev->mask_dtype, B, dev->mask_b_stride, kv_len + 1, x->d_mask, c.max_kv);
            masked = dev->mask_dtype == PGMI_DTYPE_F32 ? 2 : 1;
        }
    } else if (ragged) {
        // the per-row records are set only when this call does not continue the previous ragged one
        bool same = x->rstep_known && x->rstep_B == B;
        for (int b = 0; same && b < B; ++b) same = x->rstep_kv[b] == r_kv[b] && x->rstep_pos[b] == r_pos[b];
        if (!same) {
            RowInts rk{}, rp{};
            for (int b = 0; b < B; ++b) { rk.v[b] = r_kv[b]; rp.v[b] = r_pos[b]; }
            set_step_rows(s, x->rstep, rk, rp, B);
        }
    } else if (!x->step_known || x->step_kv != kv_len || x->step_pos != position) {
        set_step(s, x->step, kv_len, position);
    }
    // the step advances the device state itself (its last kernel); known only once this call has
    // enqueued its steps successfully (a ragged call leaves the lock-step record, and its mirror, alone)
    if (ragged) x->rstep_known = false;
    else x->step_known = false;
    auto advanced = [&]() {
        if (ragged) {
            x->rstep_known = true;
            x->rstep_B = B;
            for (int b = 0; b < B; ++b) {
                x->rstep_kv[b] = r_kv[b] + n_steps;
                x->rstep_pos[b] = r_pos[b] + n_steps;
            }
            return;
        }
        x->step_known = dev == nullptr;
        x->step_kv = kv_len + n_steps;
        x->step_pos = position + n_steps;
    };
    // input rows are always staged into the context's buffer (a stable address the graph reads)
    const uint16_t* erows = nullptr;
    if (embeds) {
        HIPCHK(hipMemcpyAsync(x->d_emb, embeds, (size_t)B * c.t_hidden * 2, hipMemcpyDeviceToDevice, s));
        erows = x->d_emb;
    }
    // n_steps greedy steps back to back: step t > 0 reads the argmax step t - 1 wrote (next_ids, or the
    // context's d_next when the caller passes none); step t's token also goes to tokens[t][B] when given
    int64_t* fb = next_ids ? next_ids : x->d_next;
    auto body = [&](hipStream_t st, const int64_t* first, int keys0, bool grow) -> int {
        for (int t = 0; t < n_steps; ++t) {
            const int r = decode_body(x, st, t == 0 ? first : fb, B, kv, kv_batch, kv_max, grow ? keys0 + t : keys0,
                                      logits, next_ids, erows, masked, tokens ? tokens + (long)t * B : nullptr,
                                      ragged);
            if (r) return r;
        }
        return 0;
    };
    if (!use_graph) {
        if ((rc = body(s, ids, kv_len + 1, true))) return rc;
        LAUNCHCHK();
        advanced();
        return 0;
    }
    // in-place feedback (next_ids == ids: the step reads its tokens first and writes the next
    // ones last) needs no staging copy; other callers' ids are staged into the context's buffer
    const int64_t* gids = ids;
    if (!embeds && ids != next_ids) {
        HIPCHK(hipMemcpyAsync(x->d_ids, ids, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        gids = x->d_ids;
    }
    if (embeds) gids = nullptr;
    const std::vector<intptr_t> key{
        B, (intptr_t)kv, kv_batch, kv_max, (intptr_t)logits, (intptr_t)next_ids,
        (intptr_t)gids,      // the ids buffer the graph reads (the context's staging copy, or in place)
        embeds != nullptr,   // the step's input is the staged embedding rows (pgmi_decode_embeds), not ids
        masked,              // 0: no mask (a zero word), 1: staged bf16 mask (sum rounded), 2: staged fp32 mask
        n_steps,             // decode steps captured back to back (pgmi_decode_steps; 1 otherwise)
        (intptr_t)tokens,    // their per-step token record ([n_steps][B], may be null)
        ragged};             // per-row step records (pgmi_decode_ragged): never aliases a lock-step graph
    // eager under use_graph and captured alike: every launch sized for kv_max keys (the step record bounds them)
    rc = run_graphed(x, x->dgraphs, s, key, [&](hipStream_t st) { return body(st, gids, kv_max, false); }, true);
    if (rc) return rc;
    LAUNCHCHK();
    advanced();
    return 0;
}

int pgmi_decode(pgmi_ctx* x, const int64_t* ids, int B, void* kv, int kv_batch, int kv_max, int kv_len, int position,
                float* logits, int64_t* next_ids, int use_graph, void* stream) {
    if (!ids) return fail(PGMI_E_ARG, "null argument");
    return decode_step(x, ids, nullptr, B, kv, kv_batch, kv_max, kv_len, position, logits, next_ids, use_graph, stream);
}

int pgmi_decode_steps(pgmi_ctx* x, int64_t* ids, int B, void* kv, int kv_batch, int kv_max, int kv_len, int position,
                      int n_steps, float* logits, int64_t* tokens, int use_graph, void* stream) {
    if (!ids) return fail(PGMI_E_ARG, "null argument");
    return decode_step(x, ids, nullptr, B, kv, kv_batch, kv_max, kv_len, position, logits, ids, use_graph, stream,
                       nullptr, n_steps, tokens);
}

int pgmi_decode_ragged(pgmi_ctx* x, const int64_t* ids, int B, void* kv, int kv_batch, int kv_max,
                       const int32_t* kv_lens, const int32_t* positions, int n_steps, float* logits, int64_t* next_ids,
                       int64_t* tokens, int use_graph, void* stream) {
    if (!ids || !kv_lens || !positions) return fail(PGMI_E_ARG, "null argument");
    if (n_steps > 1 && !next_ids) return fail(PGMI_E_ARG, "multi-step decode: next_ids carries the token fed back");
    if (x && (B < 1 || B > x->c.max_batch || B > kMaxRows)) return fail(PGMI_E_ARG, "batch exceeds capacity");
    return decode_step(x, ids, nullptr, B, kv, kv_batch, kv_max, 0, 0, logits, next_ids, use_graph, stream, nullptr,
                       n_steps, tokens, kv_lens, positions);
}

int pgmi_decode_embeds(pgmi_ctx* x, const void* embeds, int B, void* kv, int kv_batch, int kv_max, int kv_len,
                       int position, float* logits, int64_t* next_ids, int use_graph, void* stream) {
    if (!embeds) return fail(PGMI_E_ARG, "null argument");
    return decode_step(x, nullptr, embeds, B, kv, kv_batch, kv_max, kv_len, position, logits, next_ids, use_graph,
                       stream);
}

int pgmi_decode_embeds_dev(pgmi_ctx* x, const void* embeds, int B, void* kv, int kv_batch, int kv_max, int kv_len,
                           const void* position, int position_dtype, const void* mask, int mask_dtype,
                           int64_t mask_b_stride, float* logits, int64_t* next_ids, int use_graph, void* stream) {
    if (!embeds || !position) return fail(PGMI_E_ARG, "null argument");
    if (position_dtype != PGMI_DTYPE_BF16 && position_dtype != PGMI_DTYPE_F32 && position_dtype != 10 &&
        position_dtype != 11 && position_dtype != 12)
        return fail(PGMI_E_ARG, "position dtype must be bf16, fp32, fp64, int64 or int32");
    if (mask && mask_dtype != PGMI_DTYPE_BF16 && mask_dtype != PGMI_DTYPE_F32)
        return fail(PGMI_E_ARG, "mask dtype must be bf16 or fp32");
    if (B != 1) return fail(PGMI_E_ARG, "device-side positions: one sequence per step (B = 1)");
    DevStepIn d;
    d.pos = position; d.pos_dtype = position_dtype; d.mask = mask; d.mask_dtype = mask_dtype;
    d.mask_b_stride = (long)mask_b_stride;
    return decode_step(x, nullptr, embeds, B, kv, kv_batch, kv_max, kv_len, -1, logits, next_ids, use_graph, stream,
                       &d);
}

int pgmi_lm_head(pgmi_ctx* x, const void* normed, int rows, float* logits, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (!normed || !logits) return fail(PGMI_E_ARG, "null argument");
    if (rows < 1) return fail(PGMI_E_ARG, "lm_head: no rows");
    const pgmi_config& c = x->c;
    EpiArgs l{};
    l.out_f32 = logits;
    l.ldo = c.t_vocab;
    gemm((hipStream_t)stream, reinterpret_cast<const uint16_t*>(normed), c.t_hidden, x->w.embed, c.t_hidden, rows,
         c.t_vocab, c.t_hidden, EPI_F32, l, x->ws, x->ws_bytes);
    LAUNCHCHK();
    return 0;
}

// The lm_head GEMM with the EPI_LSE epilogue + the combine, over row chunks whose tile pairs fit the split-K
// workspace (pairs [chunk][column tiles] first, the label logits [chunk] behind them): nothing of rows x V is kept.
static int lm_logprobs_run(pgmi_ctx* x, const void* normed, const uint16_t* W, int rows, int V, int K,
                           const int64_t* labels, int64_t ignore_index, float* logprob, float* lse, void* stream) {
    if (!x->ws) return fail(PGMI_E_STATE, "workspace not allocated (pgmi_prepare)");
    if (V < 1 || K < 8 || K % 8 != 0) return fail(PGMI_E_ARG, "lm_logprobs: V >= 1 and K a positive multiple of 8");
    // the narrowest column tile of an EPI_LSE configuration is 64 wide: a bound on the pairs per row for any plan
    const size_t per_row = (size_t)((V + 63) / 64) * sizeof(float2) + sizeof(float);
    const int per = (int)std::min<size_t>((size_t)rows, x->ws_bytes / per_row);
    if (per < 1) return fail(PGMI_E_ARG, "lm_logprobs: vocabulary exceeds the scratch");
    float2* part = reinterpret_cast<float2*>(x->ws);
    float* lab = reinterpret_cast<float*>(reinterpret_cast<char*>(x->ws) + (size_t)per * (per_row - sizeof(float)));
    const uint16_t* A = reinterpret_cast<const uint16_t*>(normed);
    hipStream_t s = (hipStream_t)stream;
    for (int r0 = 0; r0 < rows; r0 += per) {
        const int nr = std::min(per, rows - r0);
        const int n_nt = gemm_lse_tiles(nr, V, K);
        if (n_nt < 1 || !gemm_lse(s, A + (size_t)r0 * K, K, W, K, nr, V, K, labels + r0, part, lab))
            return fail(PGMI_E_ARG, "lm_logprobs: the forced GEMM configuration has no log-sum-exp epilogue");
        lse_combine(s, part, n_nt, lab, labels + r0, nr, V, ignore_index, logprob + r0, lse ? lse + r0 : nullptr);
    }
    LAUNCHCHK();
    return 0;
}

int pgmi_lm_logprobs(pgmi_ctx* x, const void* normed, int rows, const int64_t* labels, int64_t ignore_index,
                     float* logprob, float* lse, void* stream) {
    if (!x || !normed || !labels || !logprob) return fail(PGMI_E_ARG, "null argument");
    if (rows < 1) return fail(PGMI_E_ARG, "lm_logprobs: no rows");
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    return lm_logprobs_run(x, normed, x->w.embed, rows, x->c.t_vocab, x->c.t_hidden, labels, ignore_index, logprob, lse,
                           stream);
}

int pgmi_logprobs(pgmi_ctx* x, const float* logits, int rows, int V, const int64_t* ids, int64_t ignore_index,
                  float* logprob, float* lse, void* stream) {
    if (!x || !logits || !ids || !logprob) return fail(PGMI_E_ARG, "null argument");
    if (rows < 1 || V < 1) return fail(PGMI_E_ARG, "logprobs: empty logits");
    if (!x->amax_v || !x->amax_i) return fail(PGMI_E_STATE, "logprobs scratch missing (pgmi_prepare)");
    static_assert(sizeof(float) == sizeof(int), "the argmax index scratch holds the partial sums");
    const int per = argmax_scratch_parts();
    for (int r0 = 0; r0 < rows; r0 += per)  // row batches the scratch covers (stream-ordered)
        logprob_rows((hipStream_t)stream, logits + (size_t)r0 * V, std::min(per, rows - r0), V, ids + r0, ignore_index,
                     x->amax_v, reinterpret_cast<float*>(x->amax_i), logprob + r0, lse ? lse + r0 : nullptr);
    LAUNCHCHK();
    return 0;
}

int pgmi_lm_final_hidden(pgmi_ctx* x, void* out, int rows, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (!out) return fail(PGMI_E_ARG, "null argument");
    if (rows < 1 || rows > x->c.max_batch * x->c.max_seq) return fail(PGMI_E_ARG, "rows exceed the prefill workspace");
    if (rows > x->tn_rows)
        return fail(PGMI_E_STATE, "the last pgmi_lm_forward did not keep these rows' final hidden states (logits_rows 2)");
    HIPCHK(hipMemcpyAsync(out, x->Tn, (size_t)rows * x->c.t_hidden * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---------------------------------------------------------------- replicas: load-time broadcast
#define RCCL_READY()                                                                       \
    do {                                                                                   \
        const Rccl& r_ = rccl();                                                           \
        if (!r_.get_unique_id || !r_.comm_init_rank || !r_.comm_destroy || !r_.broadcast || !r_.error_string) \
            return fail(PGMI_E_STATE, std::string("librccl could not be loaded (dlopen librccl.so.1): ") + \
                        (r_.h ? "missing nccl* symbols" : r_.why));                        \
    } while (0)

#define NCCLCHK(expr)                                                                      \
    do {                                                                                   \
        ncclResult_t r_ = (expr);                                                          \
        if (r_ != ncclSuccess) return fail(PGMI_E_HIP, std::string(#expr) + ": " + rccl().error_string(r_)); \
    } while (0)

int pgmi_comm_unique_id(void* id_out) {
    if (!id_out) return fail(PGMI_E_ARG, "null argument");
    RCCL_READY();
    static_assert(sizeof(ncclUniqueId) == PGMI_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHK(rccl().get_unique_id(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

int pgmi_comm_init(int device, int nranks, int rank, const void* id, void** comm_out) {
    if (!id || !comm_out) return fail(PGMI_E_ARG, "null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PGMI_E_ARG, "bad rank / world size");
    RCCL_READY();
    // the communicator binds to the current device: switch for the init, then give the caller's
    // thread its own current device back (torch keeps its own notion of it)
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = rccl().comm_init_rank(&comm, nranks, uid, rank);
    HIPCHK(hipSetDevice(prev));
    if (r != ncclSuccess) return fail(PGMI_E_HIP, std::string("ncclCommInitRank: ") + rccl().error_string(r));
    *comm_out = comm;
    return 0;
}

int pgmi_comm_destroy(void* comm) {
    if (!comm) return 0;
    RCCL_READY();
    NCCLCHK(rccl().comm_destroy(reinterpret_cast<ncclComm_t>(comm)));
    return 0;
}

int pgmi_broadcast_weights(pgmi_ctx* x, void* comm, int root, void* stream) {
    if (!x || !comm) return fail(PGMI_E_ARG, "null argument");
    if (x->lora_active >= 0) return fail(PGMI_E_STATE, kLoraActiveMsg);  // (a merged slab, and copies that do not match)
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound (pgmi_bind_weights)");
    RCCL_READY();
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(x->device));
    // the whole slab in one in-place collective: rank `root`'s bytes land in every replica
    const ncclResult_t r = rccl().broadcast(x->slab, x->slab, (size_t)x->slab_bytes, ncclUint8, root,
                                            reinterpret_cast<ncclComm_t>(comm), (hipStream_t)stream);
    HIPCHK(hipSetDevice(prev));
    if (r != ncclSuccess) return fail(PGMI_E_HIP, std::string("ncclBroadcast: ") + rccl().error_string(r));
    x->prepared = false;  // derived tensors are rebuilt from the received weights by pgmi_prepare
    return 0;
}

int pgmi_argmax(pgmi_ctx* x, const float* logits, int rows, int V, int64_t* out, void* stream) {
    if (!x || !logits || !out) return fail(PGMI_E_ARG, "null argument");
    if (rows <= 0 || V <= 0) return fail(PGMI_E_ARG, "argmax: empty logits");
    if (!x->amax_v) return fail(PGMI_E_STATE, "argmax scratch missing");
    argmax_rows((hipStream_t)stream, logits, rows, V, x->amax_v, x->amax_i, out);
    LAUNCHCHK();
    return 0;
}

int pgmi_eos_update(pgmi_ctx* x, int64_t* next_ids, int32_t* finished, int B, int64_t eos_id, int64_t pad_id,
                    int32_t* n_alive, void* stream) {
    if (!x || !next_ids || !finished) return fail(PGMI_E_ARG, "null argument");
    if (B <= 0) return fail(PGMI_E_ARG, "eos_update: empty batch");
    eos_update((hipStream_t)stream, next_ids, finished, B, eos_id, pad_id, n_alive);
    LAUNCHCHK();
    return 0;
}

int pgmi_decode_kernel(pgmi_ctx* x, int which, int layer, int B, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (B < 1 || B > c.max_batch) return fail(PGMI_E_ARG, "batch exceeds max_batch");
    if (layer < 0 || layer >= c.t_layers) return fail(PGMI_E_ARG, "layer out of range");
    hipStream_t s = (hipStream_t)stream;
    const float eps = c.t_rms_eps;
    const int H = c.t_hidden;
    // which 2, 3 and 4 read what the decode step reads: the 13-bit images at B <= 2 (pgmi_set_decode_packed)
    if (which >= 2 && B < gemv_mf_min_batch() && (rc = ensure_pk_image(x, s, B))) return rc;
    const TextLayerW& w = x->w.t[layer];
    switch (which) {
        case 1: gemv_res(s, B, c.t_heads * c.t_head_dim, x->dAO, w.o, H, x->dH, x->ws); break;
        case 2:
            gemv_geglu(s, B, x->dH, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, nullptr, nullptr,
                       pk_use(x, B, PK_GATE_UP, w.pk_gate_up));
            break;
        case 3:
            gemv_res(s, B, c.t_intermediate, x->dACT, w.down, H, x->dH, x->ws, pk_use(x, B, PK_DOWN, w.pk_down));
            break;
        case 4: {
            int nparts = 0;
            gemv_logits(s, B, x->dH, x->w.final_norm, eps, x->w.embed, c.t_vocab, x->dlogits, x->pmax, x->pidx,
                        &nparts, nullptr, nullptr, nullptr, nullptr, 1, pk_use(x, B, PK_LM_HEAD, x->w.pk_embed));
            break;
        }
        default: return fail(PGMI_E_ARG, "unknown kernel id");
    }
    LAUNCHCHK();
    return 0;
}

int pgmi_debug_decode_stage(pgmi_ctx* x, int stage, int layer, int B, const int64_t* ids, void* kv, int kv_batch,
                            int kv_max, const int32_t* kv_lens, const int32_t* positions, int ragged, const void* mask,
                            int mask_dtype, void* stream) {
    int rc;
    if (!x || !kv || !kv_lens || !positions) return fail(PGMI_E_ARG, "null argument");
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (stage < 0 || stage > 5)
        return fail(PGMI_E_ARG, "decode stage: 0 entry, 1 q|k|v, 2 attention + o_proj, 3 gate|up, 4 down, 5 lm_head");
    if (B < 1 || B > c.max_batch || B > kv_batch || B > kMaxRows) return fail(PGMI_E_ARG, "batch exceeds capacity");
    if (stage >= 1 && stage <= 4 && (layer < 0 || layer >= c.t_layers)) return fail(PGMI_E_ARG, "layer out of range");
    if (kv_max > c.max_kv) return fail(PGMI_E_ARG, "kv_max exceeds config max_kv");
    if (mask && B != 1) return fail(PGMI_E_ARG, "a mask: one sequence per step (B = 1)");
    if (mask && mask_dtype != PGMI_DTYPE_BF16 && mask_dtype != PGMI_DTYPE_F32)
        return fail(PGMI_E_ARG, "mask dtype must be bf16 or fp32");
    const int rows = ragged ? B : 1;
    int kv_len = 0;
    for (int b = 0; b < rows; ++b) {
        if (kv_lens[b] < 0 || (long)kv_lens[b] + 1 > kv_max)
            return fail(PGMI_E_ARG, "KV cache capacity exceeded (kv_lens[b] + 1 > kv_max)");
        kv_len = std::max(kv_len, (int)kv_lens[b]);
    }
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(PGMI_E_STATE, "pgmi_debug_decode_stage inside a stream capture");
    if (B >= gemv_mf_min_batch() && (rc = ensure_mf_image(x, s))) return rc;
    if (B < gemv_mf_min_batch() && (rc = ensure_pk_image(x, s, B))) return rc;
    // the step record(s) are set by every call (and so restored after stage 5, whose last kernel advances
    // them); the decode entry points set theirs again afterwards
    const auto set_records = [&]() {
        if (ragged) {
            RowInts rk{}, rp{};
            for (int b = 0; b < B; ++b) { rk.v[b] = kv_lens[b]; rp.v[b] = positions[b]; }
            set_step_rows(s, x->rstep, rk, rp, B);
            x->rstep_known = false;
        } else {
            set_step(s, x->step, kv_lens[0], positions[0]);
            x->step_known = false;
        }
    };
    set_records();
    int masked = 0;
    if (mask) {
        stage_mask(s, mask, mask_dtype, B, kv_len + 1, kv_len + 1, x->d_mask, c.max_kv);
        masked = mask_dtype == PGMI_DTYPE_F32 ? 2 : 1;
    }
    const DecodeRun r{s, ids, nullptr, B, kv, kv_batch, kv_max, kv_len + 1, masked, ragged != 0};
    if (stage == 0) {
        if (layer == 0) decode_head(x, r);
    } else if (stage <= 4) {
        decode_layer(x, r, layer, stage);
    } else {
        decode_tail(x, r, x->dlogits, nullptr, nullptr);
        set_records();
    }
    LAUNCHCHK();
    return 0;
}

int pgmi_debug_decode_buffer(pgmi_ctx* x, int which, void* buf, int64_t bytes, int write, void* stream) {
    int rc;
    if (!x || !buf) return fail(PGMI_E_ARG, "null argument");
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    void* p;
    int64_t cap;
    switch (which) {
        case 0: p = x->dH; cap = (int64_t)c.max_batch * c.t_hidden * 2; break;
        case 1: p = x->dACT; cap = (int64_t)c.max_batch * c.t_intermediate * 2; break;
        case 2: p = x->dlogits; cap = (int64_t)c.max_batch * c.t_vocab * 4; break;
        case 3: p = x->dQ; cap = (int64_t)c.max_batch * c.t_heads * c.t_head_dim * 2; break;
        case 4: p = x->dAO; cap = (int64_t)c.max_batch * c.t_hidden * 2; break;
        case 5: p = x->dHn; cap = (int64_t)c.max_batch * c.t_hidden * 2; break;
        case 6: p = x->dSS; cap = (int64_t)c.max_batch * (c.t_hidden / 16) * 4; break;
        case 7: p = x->d_next; cap = (int64_t)c.max_batch * 8; break;
        default: return fail(PGMI_E_ARG, "decode buffer: 0 h, 1 act, 2 logits, 3 q, 4 ao, 5 hn, 6 ssq, 7 next ids");
    }
    if (bytes < 1 || bytes > cap) return fail(PGMI_E_ARG, "decode buffer: byte count outside the buffer");
    HIPCHK(hipMemcpyAsync(write ? p : buf, write ? buf : p, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int pgmi_debug_prefill_stage(pgmi_ctx* x, int stage, int layer, int group, const int64_t* ids, const void* image_feats,
                             int n_img_rows, const void* embeds, int B, int L, const int64_t* positions,
                             const int32_t* lens, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
                             int logits_rows, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null argument");
    if (stage < 0 || stage > 7)
        return fail(PGMI_E_ARG, "prefill stage: 0 entry, 1 q|k|v, 2 attention, 3 o_proj, 4 gate|up, 5 down, 6 logits, "
                                "7 last-row tail");
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(PGMI_E_STATE, "pgmi_debug_prefill_stage inside a stream capture");
    const bool ragged = lens != nullptr;
    int rc;
    // everything lm_forward refuses, then the row lengths and the positions to the device, as it does
    if ((rc = lm_begin(x, ids, embeds, B, L, positions, lens, ragged, kv, kv_batch, kv_max, kv_start, logits,
                       &logits_rows, stream)))
        return rc;
    const pgmi_config& c = x->c;
    const int groups = (B + kPrefillGroup - 1) / kPrefillGroup;
    if (stage != 0 && (group < 0 || group >= groups)) return fail(PGMI_E_ARG, "group out of range");
    if (stage != 0 && stage != 6 && (layer < 0 || layer >= c.t_layers)) return fail(PGMI_E_ARG, "layer out of range");
    const auto run = [&](int g) {
        const int b0 = g * kPrefillGroup;
        return PrefillRun{s, b0, std::min(kPrefillGroup, B - b0), L, kv, kv_batch, kv_max, kv_start, logits, logits_rows,
                          ragged};
    };
    if (stage == 0) {
        lm_entry(x, s, ids, image_feats, n_img_rows, embeds, B, L, ragged);
        for (int g = 0; g < groups; ++g) lm_in_norm(x, run(g));
        LAUNCHCHK();
        return 0;
    }
    const PrefillRun r = run(group);
    switch (stage) {
        case 1: lm_qkv(x, r, layer); break;
        case 2: lm_attn(x, r, layer); break;
        case 3: lm_o_proj(x, r, layer); break;
        case 4: lm_gate_up(x, r, layer); break;
        case 5: lm_down(x, r, layer); break;
        case 6:
            if ((rc = lm_logits(x, r))) return rc;
            break;
        default:
            if (!run_last_only(x, r) || layer + 1 != c.t_layers)
                return fail(PGMI_E_ARG, "prefill stage 7: the last layer of a lock-step logits_rows 2 call with L > 1");
            if ((rc = lm_last_row_tail(x, r, layer))) return rc;
    }
    LAUNCHCHK();
    return 0;
}

int pgmi_debug_prefill_buffer(pgmi_ctx* x, int which, void* buf, int64_t bytes, int write, void* stream) {
    int rc;
    if (!x || !buf) return fail(PGMI_E_ARG, "null argument");
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    const int64_t R = (int64_t)c.max_batch * c.max_seq, RG = (int64_t)std::min(c.max_batch, kPrefillGroup) * c.max_seq;
    void* p;
    int64_t cap;
    switch (which) {
        case 0: p = x->Hs; cap = R * c.t_hidden * 2; break;
        case 1: p = x->Tn; cap = R * c.t_hidden * 2; break;
        case 2: p = x->QKV; cap = RG * (c.t_heads + 2 * c.t_kv_heads) * c.t_head_dim * 2; break;
        case 3: p = x->Qr; cap = RG * c.t_heads * c.t_head_dim * 2; break;
        case 4: p = x->AO; cap = RG * c.t_hidden * 2; break;
        case 5: p = x->ACT; cap = RG * c.t_intermediate * 2; break;
        case 6: p = x->lastrows; cap = (int64_t)c.max_batch * c.t_hidden * 2; break;
        case 7: p = x->dAO; cap = (int64_t)c.max_batch * c.t_hidden * 2; break;
        default:
            return fail(PGMI_E_ARG, "prefill buffer: 0 Hs, 1 Tn, 2 QKV, 3 Qr, 4 AO, 5 ACT, 6 lastrows, 7 dAO");
    }
    if (bytes < 1 || bytes > cap) return fail(PGMI_E_ARG, "prefill buffer: byte count outside the buffer");
    HIPCHK(hipMemcpyAsync(write ? p : buf, write ? buf : p, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int pgmi_preprocess(pgmi_ctx* x, const void* src_hwc, int H, int W, int out_h, int out_w, float* out_chw,
                    void* stream) {
    if (!x || !src_hwc || !out_chw) return fail(PGMI_E_ARG, "null argument");
    if (H < 1 || W < 1 || out_h < 1 || out_w < 1) return fail(PGMI_E_ARG, "empty image");
    if (!x->ws) return fail(PGMI_E_STATE, "workspace not allocated (pgmi_prepare)");
    if (preprocess_scratch_bytes(H, W, out_h, out_w) > x->ws_bytes)
        return fail(PGMI_E_ARG, "image too large for the preprocessing scratch");
    preprocess((hipStream_t)stream, reinterpret_cast<const uint8_t*>(src_hwc), H, W, out_h, out_w, out_chw, x->ws);
    LAUNCHCHK();
    return 0;
}

int pgmi_prefill_kernel(pgmi_ctx* x, int which, int layer, int rows, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (rows < 1 || rows > std::min(c.max_batch, kPrefillGroup) * c.max_seq)
        return fail(PGMI_E_ARG, "rows exceed the prefill workspace (one group of 8 sequences)");
    if (layer < 0 || layer >= c.t_layers) return fail(PGMI_E_ARG, "layer out of range");
    hipStream_t s = (hipStream_t)stream;
    const int H = c.t_hidden;
    const TextLayerW& w = x->w.t[layer];
    switch (which) {
        case 0: {  // gate|up GEMM + GeGLU epilogue (modeling_gemma.py:134): Tn -> ACT
            EpiArgs g{};
            g.out = x->ACT; g.ldo = c.t_intermediate;
            gemm(s, x->Tn, H, w.gate_up, H, rows, c.t_intermediate, H, EPI_GEGLU, g, x->ws, x->ws_bytes,
                 c.t_intermediate);
            break;
        }
        case 1: {  // down GEMM as the prefill runs it: split-K partials (reduced by the next norm)
            EpiArgs d{};
            d.res = x->Hs; d.ldr = H; d.out = x->Hs; d.ldo = H;
            gemm(s, x->ACT, c.t_intermediate, w.down, c.t_intermediate, rows, H, c.t_intermediate, EPI_RES, d, x->ws,
                 x->ws_bytes, 0, true);
            break;
        }
        default: return fail(PGMI_E_ARG, "unknown kernel id");
    }
    LAUNCHCHK();
    return 0;
}

int pgmi_debug_gemm_tiles(int n_mt, int n_nt, int S, int BM, int BN, int K, int* mt, int* nt, int* z) {
    if (n_mt < 1 || n_nt < 1 || S < 1 || !mt || !nt || !z) return fail(PGMI_E_ARG, "bad argument");
    return gemm_tile_order(n_mt, n_nt, S, BM, BN, K, mt, nt, z);
}

int pgmi_debug_gemm_plan(int M, int N, int K, int dual, int* cfg, int* bm, int* bn, int* split) {
    if (M < 1 || N < 1 || K < 1 || !cfg || !bm || !bn || !split) return fail(PGMI_E_ARG, "bad argument");
    gemm_plan(M, N, K, dual, cfg, bm, bn, split);
    return 0;
}

int pgmi_tune_gemm(int cfg, int split) {
    if ((cfg >= 0 && !gemm_cfg_valid(cfg)) || split < 0 || split > 32) return fail(PGMI_E_ARG, "bad GEMM plan");
    gemm_force_plan(cfg, split);
    return 0;
}

int pgmi_tune_gemm_shape(int M, int N, int K, int dual, int cfg, int split) {
    if ((cfg >= 0 && !gemm_cfg_valid(cfg)) || split < 0 || split > 16) return fail(PGMI_E_ARG, "bad GEMM plan");
    if (gemm_force_shape(M, N, K, dual, cfg, split)) return fail(PGMI_E_ARG, "too many per-shape GEMM plans");
    return 0;
}

int pgmi_tune_attention(int variant) {
    static const int ok[] = {-1, 0, 7, 8, 41, 42, 21, 22, 44, 24, 9, 91, 92, 94, 81, 82};
    for (int v : ok)
        if (v == variant) {
            attention_force_variant(variant);
            return 0;
        }
    return fail(PGMI_E_ARG, "unknown attention variant");
}

int pgmi_sample_top_p(pgmi_ctx* x, const float* logits, int rows, int V, float temperature, float top_p,
                      const float* u, int64_t* out, float* kept_mass, void* stream) {
    if (!x || !logits || !u || !out) return fail(PGMI_E_ARG, "null argument");
    if (rows <= 0 || V <= 0) return fail(PGMI_E_ARG, "sample_top_p: empty probabilities");
    if (!(top_p >= 0.f)) return fail(PGMI_E_ARG, "sample_top_p: top_p must be >= 0");
    if (!x->ws) return fail(PGMI_E_STATE, "workspace not allocated (pgmi_prepare)");
    const int per = (int)std::min<size_t>((size_t)rows, x->ws_bytes / sample_scratch_bytes(1, V));
    if (per < 1) return fail(PGMI_E_ARG, "sample_top_p: vocabulary exceeds the scratch");
    for (int r0 = 0; r0 < rows; r0 += per) {  // row batches that fit the scratch (stream-ordered)
        const int nr = std::min(per, rows - r0);
        sample_top_p((hipStream_t)stream, logits + (size_t)r0 * V, nr, V, temperature, top_p, u + r0, x->ws,
                     out + r0, kept_mass ? kept_mass + r0 : nullptr);
    }
    LAUNCHCHK();
    return 0;
}

// pgmi_logits_params -> the rule's own record, with what the ABI refuses
static int logits_rule_from(const pgmi_logits_params* p, int rows, int V, const uint32_t* history,
                            const int32_t* emitted, LogitsRule* R) {
    if (!p) return fail(PGMI_E_ARG, "null argument");
    if (rows <= 0 || V <= 0) return fail(PGMI_E_ARG, "logits_process: empty logits");
    if (!std::isfinite(p->rp) || !(p->rp > 0.f)) return fail(PGMI_E_ARG, "logits_process: rp must be finite and > 0");
    if (!std::isfinite(p->pp) || !std::isfinite(p->fp))
        return fail(PGMI_E_ARG, "logits_process: pp and fp must be finite");
    if (p->top_k < 0) return fail(PGMI_E_ARG, "logits_process: top_k must be >= 0");
    if (!(p->min_p_delta <= 0.f)) return fail(PGMI_E_ARG, "logits_process: min_p_delta must be <= 0 (-inf: off)");
    R->rp = p->rp; R->pp = p->pp; R->fp = p->fp;
    R->use_rp = p->rp != 1.f;
    R->use_pp = p->pp != 0.f;
    R->use_fp = p->fp != 0.f;
    if ((R->use_rp || R->use_pp || R->use_fp) && !history)
        return fail(PGMI_E_ARG, "logits_process: a penalty needs the token history");
    const bool sup = p->suppress_id >= 0 && p->min_new_tokens > 0;
    if (sup && p->suppress_id >= V) return fail(PGMI_E_ARG, "logits_process: suppress_id outside the vocabulary");
    if (sup && !emitted) return fail(PGMI_E_ARG, "logits_process: the suppress needs the emitted counts");
    R->suppress_id = sup ? p->suppress_id : -1;
    R->min_new_tokens = sup ? p->min_new_tokens : 0;
    R->top_k = p->top_k >= V ? 0 : p->top_k;
    R->delta = p->min_p_delta;
    return 0;
}

int pgmi_logits_process_host(const float* logits, int rows, int V, const uint32_t* history, const float* bias,
                             const pgmi_logits_params* params, const int32_t* emitted, float* y) {
    if (!logits || !y) return fail(PGMI_E_ARG, "null argument");
    LogitsRule R;
    if (int rc = logits_rule_from(params, rows, V, history, emitted, &R)) return rc;
    std::vector<float> y1((size_t)V), sorted;
    for (int r = 0; r < rows; ++r) {
        const float* xr = logits + (size_t)r * V;
        const uint32_t* hr = history ? history + (size_t)r * V : nullptr;
        float* yr = y + (size_t)r * V;
        const bool sup = R.suppress_id >= 0 && emitted[r] < R.min_new_tokens;
        float m = lgr_neg_inf();
        for (int v = 0; v < V; ++v) {
            float e = lgr_stage1(xr[v], hr ? hr[v] : 0u, R, bias != nullptr, bias ? bias[v] : 0.f);
            if (sup && v == R.suppress_id) e = lgr_neg_inf();
            y1[v] = e;
            if (e > m) m = e;
        }
        if (m == lgr_neg_inf()) {  // the guard: everything banned -> the raw row
            if (yr != xr) std::memmove(yr, xr, (size_t)V * sizeof(float));
            continue;
        }
        float kth = lgr_neg_inf();
        if (R.top_k > 0) {
            sorted = y1;
            std::sort(sorted.begin(), sorted.end(), [](float a, float b) { return a > b; });
            kth = sorted[R.top_k - 1];
        }
        const float thr = lgr_threshold(kth, m, R.delta);
        for (int v = 0; v < V; ++v) yr[v] = lgr_stage2(y1[v], thr);
    }
    return 0;
}

// ---------------------------------------------------------------- beam search: the rule on the host (beam_rule.h)
int64_t pgmi_beam_state_bytes(int G, int K, int n_tokens, int V) {
    BeamLayout L;
    if (!bmr_layout(G, K, n_tokens, V, &L)) return -1;
    return L.total_words * 4;
}

int pgmi_beam_state_layout(int G, int K, int n_tokens, int V, int64_t* out, int n) {
    BeamLayout L;
    if (!out || n < 14) return fail(PGMI_E_ARG, "beam_state_layout: 14 values");
    if (!bmr_layout(G, K, n_tokens, V, &L))
        return fail(PGMI_E_ARG, "beam: need 1 <= K <= 16, G * K <= 16, n_tokens >= 1 and V >= 2K (at most 1.5M)");
    const int64_t v[14] = {L.den, L.run, L.heur, L.frozen, L.pool_score, L.pool_valid, L.pool_step, L.pool_parent,
                           L.pool_token, L.hist_parent, L.hist_token, L.state_words, L.total_words, L.nb};
    std::memcpy(out, v, sizeof(v));
    return 0;
}

int pgmi_beam_reset_host(void* state, int G, int K, int n_tokens, int V, int eos, int early_stopping, const float* den) {
    BeamLayout L;
    if (!state || !den) return fail(PGMI_E_ARG, "null argument");
    if (!bmr_layout(G, K, n_tokens, V, &L))
        return fail(PGMI_E_ARG, "beam: need 1 <= K <= 16, G * K <= 16, n_tokens >= 1 and V >= 2K (at most 1.5M)");
    if (eos < -1 || eos >= V) return fail(PGMI_E_ARG, "beam: eos outside the vocabulary (-1: none)");
    int* w = reinterpret_cast<int*>(state);
    std::memset(w, 0, (size_t)L.state_words * 4);
    const int hdr[kBeamHdrWords] = {G, K, n_tokens, eos, early_stopping ? 1 : 0, V, 0, 0};
    std::memcpy(w, hdr, sizeof(hdr));
    std::memcpy(w + L.den, den, (size_t)(n_tokens + 1) * 4);
    for (int g = 0; g < G; ++g) w[L.heur + g] = 1;
    float* f = reinterpret_cast<float*>(state);
    for (int i = 0; i < G * K; ++i) f[L.pool_score + i] = lgr_neg_inf();
    for (long i = 0; i < 2L * n_tokens * G * K; ++i) w[L.hist_parent + i] = -1;
    return 0;
}

int pgmi_beam_step_host(void* state, const float* logits, int rows_in, int t, const float* lse_in, int64_t* next_ids,
                        int32_t* parent, int32_t* n_open, float* lse_out) {
    if (!state || !logits || !next_ids || !parent) return fail(PGMI_E_ARG, "null argument");
    int* w = reinterpret_cast<int*>(state);
    float* f = reinterpret_cast<float*>(state);
    BeamLayout L;
    if (!bmr_layout(w[0], w[1], w[2], w[5], &L)) return fail(PGMI_E_ARG, "beam_step: the state was not reset");
    const int G = L.G, K = L.K, C = L.C, V = L.V;
    if (rows_in != 1 && rows_in != K) return fail(PGMI_E_ARG, "beam_step: rows_in is 1 or K");
    if (t < 0 || t >= L.n_tokens) return fail(PGMI_E_ARG, "beam_step: step outside [0, n_tokens)");
    std::vector<uint64_t> keys((size_t)V);
    std::vector<float> cx((size_t)rows_in * C), lse((size_t)rows_in);
    std::vector<int> ctok((size_t)rows_in * C);
    for (int g = 0; g < G; ++g) {
        for (int r = 0; r < rows_in; ++r) {
            const int row = g * rows_in + r;
            const float* xr = logits + (size_t)row * V;
            for (int v = 0; v < V; ++v) keys[v] = bmr_key(xr[v], v);
            std::partial_sort(keys.begin(), keys.begin() + C, keys.end(), std::greater<uint64_t>());
            for (int c = 0; c < C; ++c) {
                cx[r * C + c] = bmr_key_x(keys[c]);
                ctok[r * C + c] = bmr_key_tok(keys[c]);
            }
            if (lse_in) {
                lse[r] = lse_in[row];
            } else {  // the row's log-sum-exp in fp64, rounded once
                float m = lgr_neg_inf();
                for (int v = 0; v < V; ++v) m = xr[v] > m ? xr[v] : m;
                const double ms = m == lgr_neg_inf() ? 0.0 : (double)m;
                double acc = 0.0;
                for (int v = 0; v < V; ++v) acc += std::exp((double)xr[v] - ms);
                lse[r] = (float)((double)m + std::log(acc));
            }
            if (lse_out) lse_out[row] = lse[r];
        }
        const int o = g * K;
        BeamGroup st{f + L.run + o, w + L.heur + g, w + L.frozen + g, f + L.pool_score + o, w + L.pool_valid + o,
                     w + L.pool_step + o, w + L.pool_parent + o, w + L.pool_token + o};
        bmr_group_step(g, K, L.n_tokens, w[3], w[4], t, rows_in, cx.data(), ctok.data(), lse.data(), f + L.den, st,
                       next_ids + o, parent + o, w + L.hist_parent + (long)t * G * K + o,
                       w + L.hist_token + (long)t * G * K + o);
    }
    if (n_open) {
        int n = 0;
        for (int g = 0; g < G; ++g) n += w[L.frozen + g] == 0;
        *n_open = n;
    }
    return 0;
}

// ---------------------------------------------------------------- single ops (tests)
int pgmi_op_gemm(pgmi_ctx* x, const void* A, const void* Wt, int M, int N, int K, int epi, const void* bias,
                 const void* res, void* out, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (K % 8 != 0) return fail(PGMI_E_ARG, "K must be a multiple of 8");
    EpiArgs e{};
    e.bias = reinterpret_cast<const uint16_t*>(bias);
    e.res = reinterpret_cast<const uint16_t*>(res);
    e.ldr = N;
    e.ldo = N;
    if (epi == EPI_F32) e.out_f32 = reinterpret_cast<float*>(out);
    else e.out = reinterpret_cast<uint16_t*>(out);
    gemm((hipStream_t)stream, reinterpret_cast<const uint16_t*>(A), K, reinterpret_cast<const uint16_t*>(Wt), K, M, N,
         K, (Epi)epi, e, x->ws, x->ws_bytes, epi == EPI_GEGLU ? N : 0);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_lm_logprobs(pgmi_ctx* x, const void* normed, const void* W, int rows, int V, int K, const int64_t* labels,
                        int64_t ignore_index, float* logprob, float* lse, void* stream) {
    if (!x || !normed || !W || !labels || !logprob) return fail(PGMI_E_ARG, "null argument");
    if (rows < 1) return fail(PGMI_E_ARG, "lm_logprobs: no rows");
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    return lm_logprobs_run(x, normed, reinterpret_cast<const uint16_t*>(W), rows, V, K, labels, ignore_index, logprob,
                           lse, stream);
}

int pgmi_op_gemm_strided(pgmi_ctx* x, const void* A, int lda, const void* Wt, int ldw, int M, int N, int K, int epi,
                         const void* bias, const void* res, void* out, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (K % 8 != 0 || lda < K || ldw < K || lda % 8 != 0 || ldw % 8 != 0)
        return fail(PGMI_E_ARG, "K, lda, ldw must be multiples of 8 with lda, ldw >= K");
    EpiArgs e{};
    e.bias = reinterpret_cast<const uint16_t*>(bias);
    e.res = reinterpret_cast<const uint16_t*>(res);
    e.ldr = N;
    e.ldo = N;
    if (epi == EPI_F32) e.out_f32 = reinterpret_cast<float*>(out);
    else e.out = reinterpret_cast<uint16_t*>(out);
    gemm((hipStream_t)stream, reinterpret_cast<const uint16_t*>(A), lda, reinterpret_cast<const uint16_t*>(Wt), ldw, M,
         N, K, (Epi)epi, e, x->ws, x->ws_bytes, epi == EPI_GEGLU ? N : 0);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_rmsnorm(pgmi_ctx* x, const void* in, const void* w, int rows, int D, float eps, void* out, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    rmsnorm((hipStream_t)stream, reinterpret_cast<const uint16_t*>(in), reinterpret_cast<const uint16_t*>(w), eps,
            reinterpret_cast<uint16_t*>(out), rows, D);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_layernorm(pgmi_ctx* x, const void* in, const void* w, const void* b, int rows, int D, float eps, void* out,
                      void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    layernorm((hipStream_t)stream, reinterpret_cast<const uint16_t*>(in), reinterpret_cast<const uint16_t*>(w),
              reinterpret_cast<const uint16_t*>(b), eps, reinterpret_cast<uint16_t*>(out), rows, D);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_add(pgmi_ctx* x, const void* a, const void* b, int64_t n, void* out, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    if (!a || !b || !out || n < 0) return fail(PGMI_E_ARG, "bad argument");
    if (n % 8 != 0) return fail(PGMI_E_ARG, "n must be a multiple of 8");
    if (n == 0) return 0;
    add_rows((hipStream_t)stream, reinterpret_cast<const uint16_t*>(a), reinterpret_cast<const uint16_t*>(b), (long)n,
             reinterpret_cast<uint16_t*>(out));
    LAUNCHCHK();
    return 0;
}

int pgmi_op_patch_embed(pgmi_ctx* x, const void* pixels, int pixel_dtype, int B, int C, int H, int P, const void* conv_w,
                        const void* conv_b, const void* pos, int D, void* out, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    if (!pixels || !conv_w || !conv_b || !pos || !out) return fail(PGMI_E_ARG, "null argument");
    if (pixel_dtype != PGMI_DTYPE_F32 && pixel_dtype != PGMI_DTYPE_BF16) return fail(PGMI_E_ARG, "pixels must be fp32 or bf16");
    if (B < 1 || C < 1 || P < 1 || H < P || H % P != 0 || D < 1 || D % 8 != 0) return fail(PGMI_E_ARG, "bad shape");
    const int N = (H / P) * (H / P), K = C * P * P, Kpad = (K + 63) / 64 * 64;
    // scratch: the conv weight padded to Kpad columns, then the patch rows (modeling_siglip.py:67 as a GEMM)
    const size_t wbytes = ((size_t)D * Kpad * 2 + 255) & ~(size_t)255, pbytes = ((size_t)B * N * Kpad * 2 + 255) & ~(size_t)255;
    if (wbytes + pbytes > x->ws_bytes) return fail(PGMI_E_ARG, "batch too large for the scratch");
    hipStream_t s = (hipStream_t)stream;
    uint16_t* wpad = reinterpret_cast<uint16_t*>(x->ws);
    uint16_t* rows = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(x->ws) + wbytes);
    pad_rows(s, reinterpret_cast<const uint16_t*>(conv_w), D, K, Kpad, wpad);
    patchify(s, pixels, pixel_dtype == PGMI_DTYPE_F32, B, C, H, H, P, Kpad, rows);
    EpiArgs e{};
    e.bias = reinterpret_cast<const uint16_t*>(conv_b);
    e.pos = reinterpret_cast<const uint16_t*>(pos);
    e.npos = N;
    e.out = reinterpret_cast<uint16_t*>(out);
    e.ldo = D;
    float* gws = reinterpret_cast<float*>(reinterpret_cast<char*>(x->ws) + wbytes + pbytes);
    gemm(s, rows, Kpad, wpad, Kpad, B * N, D, Kpad, EPI_BIAS_POS, e, gws, x->ws_bytes - wbytes - pbytes);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_attention(pgmi_ctx* x, const void* q, const void* k, const void* v, void* o, int B, int Lq, int Lk, int H,
                      int Hkv, int hd, float scale, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    if (hd != 256 && hd != 72) return fail(PGMI_E_ARG, "head_dim must be 72 or 256");
    if (H % Hkv != 0 || H / Hkv > 16) return fail(PGMI_E_ARG, "bad head grouping");
    AttnArgs a{};
    a.q = reinterpret_cast<const uint16_t*>(q); a.q_b_stride = (long)Lq * H * hd; a.q_row_stride = H * hd; a.q_head_stride = hd;
    a.k = reinterpret_cast<const uint16_t*>(k); a.k_b_stride = (long)Lk * Hkv * hd; a.k_row_stride = Hkv * hd; a.k_head_stride = hd;
    a.v = reinterpret_cast<const uint16_t*>(v); a.v_b_stride = a.k_b_stride; a.v_row_stride = Hkv * hd; a.v_head_stride = hd;
    a.o = reinterpret_cast<uint16_t*>(o); a.o_b_stride = a.q_b_stride; a.o_row_stride = H * hd; a.o_head_stride = hd;
    a.Lq = Lq; a.Lk = Lk; a.G = H / Hkv; a.n_kv = Hkv; a.B = B; a.scale = scale;
    a.ws = x->ws; a.ws_floats = (long)(x->ws_bytes / sizeof(float));
    attention_prefill((hipStream_t)stream, hd, a);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_attention_ex(pgmi_ctx* x, const void* q, const void* k, const void* v, void* o, int B, int Lq, int Lk,
                         int H, int Hkv, int hd, int kv_layout, float scale, int scale_div, const void* mask,
                         int mask_dtype, int64_t m_b_stride, int64_t m_h_stride, int64_t m_q_stride, void* probs,
                         void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    if (!q || !k || !v || !o) return fail(PGMI_E_ARG, "null argument");
    if (B < 1 || Lq < 1 || Lk < 1 || H < 1 || Hkv < 1 || H % Hkv != 0) return fail(PGMI_E_ARG, "bad shape");
    if (hd < 1 || hd > 256) return fail(PGMI_E_ARG, "head_dim must be in [1, 256]");
    if (kv_layout != 0 && kv_layout != 1) return fail(PGMI_E_ARG, "kv_layout must be 0 (B,L,Hkv,hd) or 1 (B,Hkv,L,hd)");
    if (mask && mask_dtype != PGMI_DTYPE_BF16 && mask_dtype != PGMI_DTYPE_F32)
        return fail(PGMI_E_ARG, "mask must be bf16 or fp32");
    if (attention_exact_lds(Lk, hd) > 160 * 1024) return fail(PGMI_E_ARG, "too many keys for one workgroup's scores");
    ModAttnArgs a{};
    a.q = reinterpret_cast<const uint16_t*>(q);
    a.k = reinterpret_cast<const uint16_t*>(k);
    a.v = reinterpret_cast<const uint16_t*>(v);
    a.kv_b_stride = (long)Lk * Hkv * hd;
    a.kv_h_stride = kv_layout == 0 ? hd : (long)Lk * hd;
    a.kv_row_stride = kv_layout == 0 ? (long)Hkv * hd : hd;
    a.o = reinterpret_cast<uint16_t*>(o);
    a.probs = reinterpret_cast<uint16_t*>(probs);
    a.mask = mask;
    a.m_b_stride = m_b_stride;
    a.m_h_stride = m_h_stride;
    a.m_q_stride = m_q_stride;
    a.mask_f32 = mask_dtype == PGMI_DTYPE_F32;
    a.B = B; a.Lq = Lq; a.Lk = Lk; a.H = H; a.Hkv = Hkv; a.hd = hd;
    a.scale = scale;
    a.scale_div = scale_div != 0;
    attention_exact((hipStream_t)stream, a);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_rope(pgmi_ctx* x, const void* in, const void* cos_rows, const void* sin_rows, int64_t rows, int heads,
                 int hd, void* out, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    if (!in || !cos_rows || !sin_rows || !out) return fail(PGMI_E_ARG, "null argument");
    if (rows < 0 || heads < 1 || hd < 2 || hd % 2 != 0) return fail(PGMI_E_ARG, "bad shape");
    if (rows == 0) return 0;
    rope_rows((hipStream_t)stream, reinterpret_cast<const uint16_t*>(in), reinterpret_cast<const uint16_t*>(cos_rows),
              reinterpret_cast<const uint16_t*>(sin_rows), (long)rows, heads, hd, reinterpret_cast<uint16_t*>(out));
    LAUNCHCHK();
    return 0;
}

int pgmi_op_scale(pgmi_ctx* x, const void* in, float a, int64_t n, void* out, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    if (!in || !out || n < 0) return fail(PGMI_E_ARG, "bad argument");
    if (n % 8 != 0) return fail(PGMI_E_ARG, "n must be a multiple of 8");
    if (n == 0) return 0;
    scale_rows((hipStream_t)stream, reinterpret_cast<const uint16_t*>(in), (long)n, a, reinterpret_cast<uint16_t*>(out));
    LAUNCHCHK();
    return 0;
}

int pgmi_op_gemv_res(pgmi_ctx* x, const void* in, const void* Wt, int B, int N, int K, void* h, void* stream) {
    if (!x) return fail(PGMI_E_ARG, "null ctx");
    if (K != 2048 && K != 16384) return fail(PGMI_E_ARG, "K must be 2048 or 16384");
    if (B < 1 || B > kMaxRows) return fail(PGMI_E_ARG, "B must be in [1, 16]");
    if (!x->ws) return fail(PGMI_E_STATE, "workspace not allocated (pgmi_prepare)");
    if ((size_t)(K / 2048) * B * N * sizeof(float) > x->ws_bytes) return fail(PGMI_E_ARG, "N too large for the scratch");
    gemv_res((hipStream_t)stream, B, K, reinterpret_cast<const uint16_t*>(in), reinterpret_cast<const uint16_t*>(Wt), N,
             reinterpret_cast<uint16_t*>(h), x->ws);
    LAUNCHCHK();
    return 0;
}

}  // extern "C"
