// engine_images.hip -- libpgmi host side: the weight images the decode step reads instead of the slab's rows --
// fragment-major (B >= 3, kernels_gemv_mfma.hip) and 13-bit (pack13.h: row-major segments for B <= 2, fragment-major
// ones for B >= 3) -- built on demand by the first step that wants them, their switch and info calls, and the
// 13-bit format on the host.
#include "engine_graph.h"

namespace pgmi_eng __attribute__((visibility("hidden"))) {

// the weights changed (pgmi_prepare, a new slab): no image is valid until ensure_pk_image has rebuilt it
void pk_forget(pgmi_ctx* x) {
    x->pk_done = x->pk_done_batched = 0;
    x->pk_alloc_failed = x->pkb_alloc_failed = false;
    x->w.pk_embed = x->w.pkb_embed = PkW{};
    for (auto& t : x->w.t) t.pk_gate_up = t.pk_down = t.pkb_gate_up = t.pkb_down = PkW{};
}

// forget the 13-bit images of the kinds in `kinds` alone (their tensors changed), row-major and fragment-major: the
// next step that wants them rescans and repacks those, the other kinds' images stay
void pk_forget_kinds(pgmi_ctx* x, int kinds) {
    x->pk_done &= ~kinds;
    x->pk_done_batched &= ~kinds;
    for (auto& t : x->w.t) {
        if (kinds & PK_GATE_UP) t.pk_gate_up = t.pkb_gate_up = PkW{};
        if (kinds & PK_DOWN) t.pk_down = t.pkb_down = PkW{};
    }
    if (kinds & PK_LM_HEAD) x->w.pk_embed = x->w.pkb_embed = PkW{};
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

// The 13-bit images (pack13.h) that the streaming GEMVs of the B <= 2 decode step read instead of the bf16 rows:
// every layer's gate|up (one 2 I x H tensor) and down, and the tied embedding as lm_head reads it -- 2 L + 1
// candidate tensors, 13/16 of their bytes (3.80 GB beside the resident bf16 weights at the 3B shapes).  (Re)built
// on stream s by the first such step after a pgmi_prepare, outside any capture: pass one scans each tensor's
// exponent range, the host reads the 2 L + 1 results (one stream synchronisation) and packs the tensors that fit;
// a tensor that does not fit keeps the bf16 kernel, as does a whole kind whose buffer cannot be allocated.
//
// mf: the fragment-major images of the batched (B >= 3) step instead (ensure_pk_image_mf) -- the same candidates,
// scan and fit rule, pk_pack_mf's gather, buffers and PkW entries of their own (pkb_*), lm_head's rows padded to a
// whole group.  settled: the kinds now scanned, or given up for this weight set; 0 inside a capture.
static int pk_build(pgmi_ctx* x, hipStream_t s, int want, bool mf, int* settled) {
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
    const auto bytes = [mf](int64_t rows, int64_t K) { return mf ? pk_image_bytes_mf(rows, K) : pk_image_bytes(rows, K); };
    const int64_t gu_b = bytes(2 * I, H), dn_b = bytes(H, I), em_b = bytes(V, H);
    const int64_t kind_bytes[3] = {gu_b * L, dn_b * L, em_b};
    uint8_t** bufs = mf ? x->pkb_buf : x->pk_buf;
    int got = 0;
    for (int k = 0; k < 3; ++k) {
        if (!(want & (1 << k)) || kind_bytes[k] == 0) continue;
        if (!bufs[k]) {
            void* p = nullptr;
            if (hipMalloc(&p, (size_t)kind_bytes[k]) != hipSuccess) {
                (void)hipGetLastError();  // out of memory: this kind keeps the bf16 kernels
                (mf ? x->pkb_alloc_failed : x->pk_alloc_failed) = true;
                continue;
            }
            x->allocs.push_back(p);
            bufs[k] = reinterpret_cast<uint8_t*>(p);
        }
        got |= 1 << k;
    }
    for (int i = 0; i < L; ++i) {
        TextLayerW& w = x->w.t[i];
        if (got & PK_GATE_UP)
            cands.push_back({PK_GATE_UP, w.gate_up, 2 * I, H, mf ? &w.pkb_gate_up : &w.pk_gate_up, bufs[0] + gu_b * i});
        if (got & PK_DOWN) cands.push_back({PK_DOWN, w.down, H, I, mf ? &w.pkb_down : &w.pk_down, bufs[1] + dn_b * i});
    }
    if (got & PK_LM_HEAD) cands.push_back({PK_LM_HEAD, x->w.embed, V, H, mf ? &x->w.pkb_embed : &x->w.pk_embed, bufs[2]});
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
            if (mf) pk_pack_mf(s, cands[t].W, (long)cands[t].rows, (int)cands[t].K, e_hi, cands[t].out);
            else pk_pack(s, cands[t].W, (long)cands[t].rows, (int)cands[t].K, e_hi, cands[t].out);
            cands[t].dst->img = cands[t].out;
            cands[t].dst->base2 = pk_base2(e_hi);
        }
        LAUNCHCHK();
    }
    *settled = want;
    return 0;
}

int ensure_pk_image(pgmi_ctx* x, hipStream_t s, int B) {
    const int want = pk_mask_for(x, B) & ~x->pk_done;
    if (!want) return 0;
    if (!pk_shapes(x->c)) {
        x->pk_done |= want;
        return 0;
    }
    int settled = 0;
    if (int rc = pk_build(x, s, want, false, &settled)) return rc;
    if (!settled) return 0;
    x->pk_done |= settled;
    // steps captured before held the bf16 launches, and so did a prefill's last-row GEMVs (lm_last_row_tail,
    // lm_logits: pk_use reads pk_done); a prefill key merely seen before runs eagerly again, in the packed form
    graphs_drop(x, GRAPHS_DECODE_SMALL | GRAPHS_PREFILL);
    return 0;
}

// The fragment-major 13-bit images the batched step's gate|up, down and lm_head launches read under
// pgmi_set_decode_packed_batched: built like the B <= 2 ones (pk_build), by the first B >= 3 step that wants them
// after a pgmi_prepare.  The bf16 fragment-major image mfw stays: a B >= 3 engine with every kind on holds both
// (up to 3.80 GB more at the 3B shapes).  The prefill never reads these (pk_use: its last-row GEMVs pass none).
int ensure_pk_image_mf(pgmi_ctx* x, hipStream_t s) {
    const int want = x->pk_mask_batched & ~x->pk_done_batched;
    if (!want) return 0;
    if (!pk_shapes(x->c)) {
        x->pk_done_batched |= want;
        return 0;
    }
    int settled = 0;
    if (int rc = pk_build(x, s, want, true, &settled)) return rc;
    if (!settled) return 0;
    x->pk_done_batched |= settled;
    graphs_drop(x, GRAPHS_DECODE_BATCHED);  // steps captured before held the bf16 launches
    return 0;
}

}  // namespace pgmi_eng

extern "C" {

int pgmi_set_decode_packed(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (on > PK_ALL) return fail(PGMI_E_ARG, "decode_packed: 0 off, 1..7 a mask of kinds (1 gate|up, 2 down, 4 lm_head), < 0 default");
    x->pk_mask = on < 0 ? -1 : on;
    // captured steps hold the other form's launches (a last-row-only prefill's GEMVs follow the setting)
    graphs_drop(x, GRAPHS_DECODE_SMALL | GRAPHS_PREFILL);
    return 0;
}

int pgmi_set_decode_packed_batched(pgmi_ctx* x, int mask) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (mask < 0 || mask > PK_ALL)
        return fail(PGMI_E_ARG, "decode_packed_batched: 0 off, 1..7 a mask of kinds (1 gate|up, 2 down, 4 lm_head)");
    x->pk_mask_batched = mask;
    graphs_drop(x, GRAPHS_DECODE_BATCHED);  // captured B >= 3 steps hold the other form's launches
    return 0;
}

int pgmi_decode_packed_batched_info(const pgmi_ctx* x, int64_t* info, int n) {
    if (!x || !info) return fail(PGMI_E_ARG, "null argument");
    if (n < PGMI_PACKED_BATCHED_INFO_N) return fail(PGMI_E_ARG, "info needs PGMI_PACKED_BATCHED_INFO_N entries");
    const pgmi_config& c = x->c;
    const int64_t I = c.t_intermediate, H = c.t_hidden, V = c.t_vocab;
    const bool shapes = H == 2048 && I == 16384;
    const int on = x->pk_mask_batched & x->pk_done_batched;
    int64_t np = 0, nr = 0, bp = 0;
    auto count = [&](int kind, const PkW& w, int64_t rows, int64_t K) {
        if ((on & kind) && w.img && shapes) { ++np; bp += pk_image_bytes_mf(rows, K); }
        else ++nr;
    };
    for (size_t i = 0; i < x->w.t.size(); ++i) {
        count(PK_GATE_UP, x->w.t[i].pkb_gate_up, 2 * I, H);
        count(PK_DOWN, x->w.t[i].pkb_down, H, I);
    }
    count(PK_LM_HEAD, x->w.pkb_embed, V, H);
    info[0] = x->pk_mask_batched; info[1] = x->pk_done_batched; info[2] = np; info[3] = nr; info[4] = bp;
    info[5] = x->pkb_alloc_failed;
    return 0;
}

int pgmi_decode_packed_batched_tensor(const pgmi_ctx* x, int kind, int layer) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (kind != PK_GATE_UP && kind != PK_DOWN && kind != PK_LM_HEAD) return fail(PGMI_E_ARG, "kind: 1 gate|up, 2 down, 4 lm_head");
    if (kind != PK_LM_HEAD && (layer < 0 || layer >= (int)x->w.t.size())) return fail(PGMI_E_ARG, "layer out of range");
    const PkW& w = kind == PK_LM_HEAD ? x->w.pkb_embed : kind == PK_GATE_UP ? x->w.t[layer].pkb_gate_up : x->w.t[layer].pkb_down;
    return (x->pk_mask_batched & x->pk_done_batched & kind) && w.img ? 1 : 0;
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

// The fragment-major gather (the batched step's image): ceil(rows / 16) x K / 128 segments, rows past the last
// encoded as zeros.
int64_t pgmi_pack13_bytes_mf(int64_t rows, int64_t K) {
    if (rows < 1 || K < kPkSegK || K % kPkSegK != 0) return -1;
    return pk_image_bytes_mf(rows, K);
}

int pgmi_pack13_encode_mf(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image) {
    if (!w || !image) return fail(PGMI_E_ARG, "null argument");
    if (pgmi_pack13_bytes_mf(rows, K) < 0) return fail(PGMI_E_ARG, "pack13: K must be a positive multiple of 2048, rows >= 1");
    if (e_hi < 0 || e_hi > 255) return fail(PGMI_E_ARG, "pack13: e_hi is an exponent field (0..255)");
    for (int64_t gr = 0; gr < pk_mf_groups(rows); ++gr)
        for (int64_t kb = 0; kb < K / kPkMfK; ++kb)
            for (int l = 0; l < 64; ++l) {
                uint4 f[4];
                const int64_t row = pk_mf_row(gr, l);
                for (int ch = 0; ch < 4; ++ch) {
                    if (row < rows) std::memcpy(&f[ch], w + row * K + pk_mf_k(kb, l, ch), 16);
                    else f[ch] = make_uint4(0, 0, 0, 0);
                }
                const PkSeg sg = pk_encode(f, e_hi);
                uint8_t* d = image + pk_mf_seg(gr, kb, K) * kPkSegBytes;
                std::memcpy(d + pk_off_a(l), &sg.a, 16);
                std::memcpy(d + pk_off_b(l), &sg.b, 16);
                std::memcpy(d + pk_off_n(l), &sg.n, 16);
                std::memcpy(d + pk_off_h(l), &sg.h, 4);
            }
    return 0;
}

// w: pk_mf_groups(rows) * 16 rows of K values (the pad rows included: they decode to +0)
int pgmi_pack13_decode_mf(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w) {
    if (!w || !image) return fail(PGMI_E_ARG, "null argument");
    if (pgmi_pack13_bytes_mf(rows, K) < 0) return fail(PGMI_E_ARG, "pack13: K must be a positive multiple of 2048, rows >= 1");
    if (e_hi < 0 || e_hi > 255) return fail(PGMI_E_ARG, "pack13: e_hi is an exponent field (0..255)");
    const unsigned b2 = pk_base2(e_hi);
    for (int64_t gr = 0; gr < pk_mf_groups(rows); ++gr)
        for (int64_t kb = 0; kb < K / kPkMfK; ++kb)
            for (int l = 0; l < 64; ++l) {
                const uint8_t* d = pk_host_seg(image, pk_mf_seg(gr, kb, K));
                PkSeg sg;
                std::memcpy(&sg.a, d + pk_off_a(l), 16);
                std::memcpy(&sg.b, d + pk_off_b(l), 16);
                std::memcpy(&sg.n, d + pk_off_n(l), 16);
                std::memcpy(&sg.h, d + pk_off_h(l), 4);
                for (int ch = 0; ch < 4; ++ch) {
                    const uint4 f = pk_chunk(sg, ch, b2);
                    std::memcpy(w + pk_mf_row(gr, l) * K + pk_mf_k(kb, l, ch), &f, 16);
                }
            }
    return 0;
}

}  // extern "C"
