// engine_images.hip -- libpgmi host side: the weight images the decode step reads instead of the slab's rows --
// fragment-major (B >= 3, kernels_gemv_mfma.hip) and 13-bit (pack13.h) -- built on demand by the first step that
// wants them, their switch and info calls, and the 13-bit format on the host.  The 13-bit images come in two forms
// (PkForm: row-major segments for B <= 2, fragment-major ones for B >= 3) with one table (pgmi_ctx::pk[form]), one
// builder and one query each: a form is an index here, and a gather in pack13.h.
#include "engine_graph.h"

namespace pgmi_eng __attribute__((visibility("hidden"))) {

// forget the 13-bit images of the kinds in `kinds` alone (their tensors changed), in both forms: the next step that
// wants them rescans and repacks those, the other kinds' images stay
void pk_forget_kinds(pgmi_ctx* x, int kinds) {
    for (int f = 0; f < 2; ++f) {
        x->pk[f].done &= ~kinds;
        for (auto& t : x->w.t) {
            if (kinds & PK_GATE_UP) t.pk_gate_up[f] = PkW{};
            if (kinds & PK_DOWN) t.pk_down[f] = PkW{};
        }
        if (kinds & PK_LM_HEAD) x->w.pk_embed[f] = PkW{};
    }
}

// the weights changed (pgmi_prepare, a new slab): no image is valid until ensure_pk_image has rebuilt it
void pk_forget(pgmi_ctx* x) {
    pk_forget_kinds(x, PK_ALL);
    for (PkImages& im : x->pk) im.alloc_failed = false;
}

// The fragment-major images of every layer's gate|up, q|k|v, o_proj and down weights that the batched (B >= 3)
// decode projections read (kernels_gemv_mfma.hip; round 5), (re)built on stream s after a pgmi_prepare.  If the
// 3.96 GB (at the 3B shapes) cannot be allocated the batched decode reads the row-major weights instead (the
// same values in the same lanes: bit-identical results, slower), so the context stays usable.
int ensure_mf_image(pgmi_ctx* x, hipStream_t s) {
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
        graphs_drop(x, GRAPHS_DECODE);  // steps captured before held the row-major launches
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

// the PK kernels are the K = 2048 / K = 16384 forms: other shapes stay raw
static bool pk_shapes(const pgmi_config& c) { return c.t_hidden == 2048 && c.t_intermediate == 16384; }

// The 13-bit images (pack13.h) of form f that the decode GEMVs read instead of the bf16 weights -- the streaming
// GEMVs of a B <= 2 step the row form, the MFMA GEMVs of a batched step the fragment form (beside the bf16
// fragment-major image mfw, which stays): every layer's gate|up (one 2 I x H tensor) and down, and the tied embedding
// as lm_head reads it (fragment form: its rows padded to a whole group) -- 2 L + 1 candidate tensors, 13/16 of their
// bytes (3.80 GB beside the resident bf16 weights at the 3B shapes).  (Re)built on stream s by the first step of
// that form that wants them after a pgmi_prepare, outside any capture: pass one scans each tensor's exponent range,
// the host reads the 2 L + 1 results (one stream synchronisation) and packs the tensors that fit; a tensor that does
// not fit keeps the bf16 kernel, as does a whole kind whose buffer cannot be allocated.  The forms share the
// candidates, the scan and the fit rule; each has its gather (pk_pack), buffers and PkW entries.
// settled: the kinds now scanned, or given up for this weight set; 0 inside a capture.
static int pk_build(pgmi_ctx* x, hipStream_t s, int want, PkForm f, int* settled) {
    *settled = 0;
    const pgmi_config& c = x->c;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return 0;  // a caller's capture: this step reads the bf16 rows, a later one builds the image
    }
    const int L = c.t_layers;
    const int64_t I = c.t_intermediate, H = c.t_hidden, V = c.t_vocab;
    struct Cand { int kind; const uint16_t* W; int64_t rows, K; PkW* dst; uint8_t* out; };
    std::vector<Cand> cands;
    const int64_t gu_b = pk_image_bytes(f, 2 * I, H), dn_b = pk_image_bytes(f, H, I), em_b = pk_image_bytes(f, V, H);
    const int64_t kind_bytes[3] = {gu_b * L, dn_b * L, em_b};
    uint8_t** bufs = x->pk[f].buf;
    int got = 0;
    for (int k = 0; k < 3; ++k) {
        if (!(want & (1 << k)) || kind_bytes[k] == 0) continue;
        if (!bufs[k]) {
            void* p = nullptr;
            if (hipMalloc(&p, (size_t)kind_bytes[k]) != hipSuccess) {
                (void)hipGetLastError();  // out of memory: this kind keeps the bf16 kernels
                x->pk[f].alloc_failed = true;
                continue;
            }
            x->allocs.push_back(p);
            bufs[k] = reinterpret_cast<uint8_t*>(p);
        }
        got |= 1 << k;
    }
    for (int i = 0; i < L; ++i) {
        TextLayerW& w = x->w.t[i];
        if (got & PK_GATE_UP) cands.push_back({PK_GATE_UP, w.gate_up, 2 * I, H, &w.pk_gate_up[f], bufs[0] + gu_b * i});
        if (got & PK_DOWN) cands.push_back({PK_DOWN, w.down, H, I, &w.pk_down[f], bufs[1] + dn_b * i});
    }
    if (got & PK_LM_HEAD) cands.push_back({PK_LM_HEAD, x->w.embed, V, H, &x->w.pk_embed[f], bufs[2]});
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
            pk_pack(s, f, cands[t].W, (long)cands[t].rows, (int)cands[t].K, e_hi, cands[t].out);
            cands[t].dst->img = cands[t].out;
            cands[t].dst->base2 = pk_base2(e_hi);
        }
        LAUNCHCHK();
    }
    *settled = want;
    return 0;
}

// the 13-bit images a B-row step reads: B's form, the kinds its mask wants and that are not settled yet
int ensure_pk_image(pgmi_ctx* x, hipStream_t s, int B) {
    const PkForm f = pk_form_of(B);
    PkImages& im = x->pk[f];
    const int want = pk_mask_for(x, B) & ~im.done;
    if (!want) return 0;
    if (!pk_shapes(x->c)) {
        im.done |= want;
        return 0;
    }
    int settled = 0;
    if (int rc = pk_build(x, s, want, f, &settled)) return rc;
    if (!settled) return 0;
    im.done |= settled;
    // steps captured before held the bf16 launches, and (row form) so did a prefill's last-row GEMVs
    // (lm_last_row_tail, lm_logits: pk_use reads done); a prefill key merely seen before runs eagerly again, in the
    // packed form.  The prefill never reads the fragment form (pk_use: its last-row GEMVs refuse it).
    graphs_drop(x, pk_graphs(f));
    return 0;
}

int ensure_decode_images(pgmi_ctx* x, hipStream_t s, int B) {
    if (B >= gemv_mf_min_batch())
        if (int rc = ensure_mf_image(x, s)) return rc;
    return ensure_pk_image(x, s, B);
}

// the kinds form f's steps read packed now (row form: as a B = 1 step does)
static int pk_on(const pgmi_ctx* x, PkForm f) {
    return pk_mask_for(x, f == PK_FORM_FRAG ? gemv_mf_min_batch() : 1) & x->pk[f].done;
}

// how form f's steps read the 2 L + 1 candidate tensors now
struct PkCount { int64_t packed, raw, packed_bytes, raw_bytes; };
static PkCount pk_count(const pgmi_ctx* x, PkForm f) {
    const pgmi_config& c = x->c;
    const int64_t I = c.t_intermediate, H = c.t_hidden, V = c.t_vocab;
    const int on = pk_shapes(c) ? pk_on(x, f) : 0;
    PkCount n{0, 0, 0, 0};
    const auto count = [&](int kind, const PkW& w, int64_t rows, int64_t K) {
        if ((on & kind) && w.img) { ++n.packed; n.packed_bytes += pk_image_bytes(f, rows, K); }
        else { ++n.raw; n.raw_bytes += rows * K * 2; }
    };
    for (const TextLayerW& t : x->w.t) {
        count(PK_GATE_UP, t.pk_gate_up[f], 2 * I, H);
        count(PK_DOWN, t.pk_down[f], H, I);
    }
    count(PK_LM_HEAD, x->w.pk_embed[f], V, H);
    return n;
}

// 1: form f's steps read tensor (kind, layer) packed now, 0: raw
static int pk_tensor(const pgmi_ctx* x, PkForm f, int kind, int layer) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (kind != PK_GATE_UP && kind != PK_DOWN && kind != PK_LM_HEAD) return fail(PGMI_E_ARG, "kind: 1 gate|up, 2 down, 4 lm_head");
    if (kind != PK_LM_HEAD && (layer < 0 || layer >= (int)x->w.t.size())) return fail(PGMI_E_ARG, "layer out of range");
    const PkW& w = kind == PK_LM_HEAD ? x->w.pk_embed[f] : kind == PK_GATE_UP ? x->w.t[layer].pk_gate_up[f] : x->w.t[layer].pk_down[f];
    return (pk_on(x, f) & kind) && w.img ? 1 : 0;
}

// captured steps of form f hold the other setting's launches (row form: a last-row-only prefill's GEMVs follow it too)
static int pk_set_mask(pgmi_ctx* x, PkForm f, int mask) {
    x->pk[f].mask = mask;
    graphs_drop(x, pk_graphs(f));
    return 0;
}

}  // namespace pgmi_eng

extern "C" {

int pgmi_set_decode_packed(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (on > PK_ALL) return fail(PGMI_E_ARG, "decode_packed: 0 off, 1..7 a mask of kinds (1 gate|up, 2 down, 4 lm_head), < 0 default");
    return pk_set_mask(x, PK_FORM_ROWS, on < 0 ? -1 : on);
}

int pgmi_set_decode_packed_batched(pgmi_ctx* x, int mask) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (mask < 0 || mask > PK_ALL)
        return fail(PGMI_E_ARG, "decode_packed_batched: 0 off, 1..7 a mask of kinds (1 gate|up, 2 down, 4 lm_head)");
    return pk_set_mask(x, PK_FORM_FRAG, mask);
}

int pgmi_decode_packed_batched_info(const pgmi_ctx* x, int64_t* info, int n) {
    if (!x || !info) return fail(PGMI_E_ARG, "null argument");
    if (n < PGMI_PACKED_BATCHED_INFO_N) return fail(PGMI_E_ARG, "info needs PGMI_PACKED_BATCHED_INFO_N entries");
    const PkImages& im = x->pk[PK_FORM_FRAG];
    const PkCount k = pk_count(x, PK_FORM_FRAG);
    info[0] = im.mask; info[1] = im.done; info[2] = k.packed; info[3] = k.raw; info[4] = k.packed_bytes;
    info[5] = im.alloc_failed;
    return 0;
}

int pgmi_decode_packed_batched_tensor(const pgmi_ctx* x, int kind, int layer) {
    return pk_tensor(x, PK_FORM_FRAG, kind, layer);
}

int pgmi_decode_packed_info(const pgmi_ctx* x, int64_t* info, int n) {
    if (!x || !info) return fail(PGMI_E_ARG, "null argument");
    if (n < PGMI_PACKED_INFO_N) return fail(PGMI_E_ARG, "info needs PGMI_PACKED_INFO_N entries");
    const PkImages& im = x->pk[PK_FORM_ROWS];
    const PkCount k = pk_count(x, PK_FORM_ROWS);
    info[0] = pk_mask_for(x, 1); info[8] = pk_mask_for(x, 2); info[1] = k.packed; info[2] = k.raw;
    info[3] = k.packed_bytes; info[4] = k.raw_bytes;
    info[5] = im.alloc_failed; info[6] = x->mfw_alloc_failed; info[7] = im.done;
    return 0;
}

int pgmi_decode_packed_tensor(const pgmi_ctx* x, int kind, int layer) {
    return pk_tensor(x, PK_FORM_ROWS, kind, layer);
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

// either form's image takes K in whole row-major segments: the shapes the PK kernels accept
static int64_t pk_host_bytes(PkForm f, int64_t rows, int64_t K) {
    if (rows < 1 || K < kPkSegK || K % kPkSegK != 0) return -1;
    return pk_image_bytes(f, rows, K);
}

static int pk_host_args(PkForm f, const void* w, const void* image, int64_t rows, int64_t K, int e_hi) {
    if (!w || !image) return fail(PGMI_E_ARG, "null argument");
    if (pk_host_bytes(f, rows, K) < 0) return fail(PGMI_E_ARG, "pack13: K must be a positive multiple of 2048, rows >= 1");
    if (e_hi < 0 || e_hi > 255) return fail(PGMI_E_ARG, "pack13: e_hi is an exponent field (0..255)");
    return 0;
}

int64_t pgmi_pack13_bytes(int64_t rows, int64_t K) { return pk_host_bytes(PK_FORM_ROWS, rows, K); }

int pgmi_pack13_encode(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image) {
    if (int rc = pk_host_args(PK_FORM_ROWS, w, image, rows, K, e_hi)) return rc;
    pk_encode_host<PK_FORM_ROWS>(w, rows, K, e_hi, image);
    return 0;
}

int pgmi_pack13_decode(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w) {
    if (int rc = pk_host_args(PK_FORM_ROWS, w, image, rows, K, e_hi)) return rc;
    pk_decode_host<PK_FORM_ROWS>(image, rows, K, e_hi, w);
    return 0;
}

// The fragment-major gather (the batched step's image): ceil(rows / 16) x K / 128 segments, rows past the last
// encoded as zeros.
int64_t pgmi_pack13_bytes_mf(int64_t rows, int64_t K) { return pk_host_bytes(PK_FORM_FRAG, rows, K); }

int pgmi_pack13_encode_mf(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image) {
    if (int rc = pk_host_args(PK_FORM_FRAG, w, image, rows, K, e_hi)) return rc;
    pk_encode_host<PK_FORM_FRAG>(w, rows, K, e_hi, image);
    return 0;
}

// w: pk_mf_groups(rows) * 16 rows of K values (the pad rows included: they decode to +0)
int pgmi_pack13_decode_mf(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w) {
    if (int rc = pk_host_args(PK_FORM_FRAG, w, image, rows, K, e_hi)) return rc;
    pk_decode_host<PK_FORM_FRAG>(image, rows, K, e_hi, w);
    return 0;
}

}  // extern "C"

