// engine_weights.hip -- libpgmi host side: context create / destroy, the weight slab's layout and loading
// (host buffers, safetensors, synthetic fill), the RoPE tables, pgmi_prepare and the load-time RCCL broadcast.
//
// Orchestration restates the reference's call stacks:
//   vision   SiglipVisionTransformer.forward   modeling_siglip.py:236-244     engine_prefill.hip
//   lm       GemmaModel/GemmaForCausalLM        modeling_gemma.py:357-427      engine_prefill.hip
//   decode   one inference.py loop iteration    inference.py:56-78             engine_decode.hip
#include <dlfcn.h>

#include <rccl/rccl.h>  // types only: librccl is dlopen'ed on first use

#include "engine_graph.h"
#include "safetensors_hdr.h"

namespace pgmi_eng __attribute__((visibility("hidden"))) {
namespace {

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

}  // namespace
}  // namespace pgmi_eng

namespace pgmi_eng __attribute__((visibility("hidden"))) {

int ensure_prepared(pgmi_ctx* x) {
    // the entry of every compute call: a launcher error that an earlier call on this thread left untaken (a path
    // without a launch check) is that call's, not this one's
    (void)pgmi::launch_error_take(nullptr);
    if (!x->prepared) return fail(PGMI_E_STATE, "pgmi_prepare() has not been called");
    if (!x->slab) return fail(PGMI_E_STATE, "weights are not bound (pgmi_bind_weights)");
    return 0;
}

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

}  // namespace pgmi_eng

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
    graphs_drop(x, GRAPHS_ALL);
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
    graphs_drop(x, GRAPHS_ALL);  // every weight pointer a captured launch holds
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
            convert_to_bf16(st, src, dtype, (long)s.numel, dst);
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
                convert_to_bf16(st, scratch, dt, (long)n, dst + i0);
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
        if ((rc = dalloc_t(x, &x->d_rlens, 3 * kMaxRows))) return rc;
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
    graphs_drop(x, GRAPHS_ALL);  // the weight images are forgotten: the packed and fragment-major launches go
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

}  // extern "C"
