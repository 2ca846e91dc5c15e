// engine_lora.hip -- libpgmi host side: LoRA adapters (include/pgmi.h; the rule: lora.h) -- resident factors,
// the switch that merges one into the slab from pristine copies, and the merge on the host and as a single op.
#include "engine_graph.h"

namespace pgmi_eng __attribute__((visibility("hidden"))) {
namespace {

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

}  // namespace
}  // namespace pgmi_eng

namespace pgmi_eng __attribute__((visibility("hidden"))) {

void lora_forget_pristine(pgmi_ctx* x) {
    for (auto& kv : x->lora_pristine) kv.second.valid = false;
}

}  // namespace pgmi_eng

extern "C" {

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
    // captured steps hold the old images' launches (packed or raw, exponent base), each form's in the graphs that read
    // it (pk_graphs)
    int drop = 0;
    for (int f = 0; f < 2; ++f)
        if (kinds & x->pk[f].done) drop |= pk_graphs((PkForm)f);
    if (drop) {
        pk_forget_kinds(x, kinds);
        graphs_drop(x, drop);
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

}  // extern "C"
