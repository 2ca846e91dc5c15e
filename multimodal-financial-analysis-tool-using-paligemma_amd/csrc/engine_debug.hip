// engine_debug.hip -- libpgmi host side: what tests, probes and tools call beside the forward passes -- single
// kernels of the decode step and the prefill, the stage and buffer hooks, the GEMM / attention tuning calls, image
// preprocessing and the single ops (pgmi_op_*).
#include "engine_ctx.h"

extern "C" {

int pgmi_decode_kernel(pgmi_ctx* x, int which, int layer, int B, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (B < 1 || B > c.max_batch) return fail(PGMI_E_ARG, "batch exceeds max_batch");
    if (layer < 0 || layer >= c.t_layers) return fail(PGMI_E_ARG, "layer out of range");
    hipStream_t s = (hipStream_t)stream;
    const float eps = c.t_rms_eps;
    const int H = c.t_hidden;
    // which 2, 3 and 4 read what the decode step reads: the 13-bit images of B's form (pgmi_set_decode_packed at
    // B <= 2, pgmi_set_decode_packed_batched at B >= 3); not the bf16 fragment-major image, which they do not pass
    if (which >= 2 && (rc = ensure_pk_image(x, s, B))) return rc;
    const TextLayerW& w = x->w.t[layer];
    switch (which) {
        case 1: gemv_res(s, B, c.t_heads * c.t_head_dim, x->dAO, w.o, H, x->dH, x->ws); break;
        case 2:
            gemv_geglu(s, B, x->dH, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, nullptr, nullptr,
                       pk_use(x, B, PK_GATE_UP, w.pk_gate_up));
            break;
        case 3:
            gemv_res(s, B, c.t_intermediate, x->dACT, w.down, H, x->dH, x->ws,
                     pk_use(x, B, PK_DOWN, w.pk_down));
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
    if ((rc = ensure_decode_images(x, s, B))) return rc;
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

int pgmi_debug_decode_partials(pgmi_ctx* x, void* buf, int64_t bytes, int write, void* stream) {
    int rc;
    if (!x || !buf) return fail(PGMI_E_ARG, "null argument");
    if ((rc = ensure_prepared(x))) return rc;
    const int64_t cap = (int64_t)attention_decode_part_floats(x->c.max_batch, x->c.t_kv_heads, x->max_chunks) * 4;
    if (bytes < 1 || bytes > cap) return fail(PGMI_E_ARG, "decode partials: byte count outside the buffer");
    HIPCHK(hipMemcpyAsync(write ? (void*)x->opart : buf, write ? buf : (void*)x->opart, (size_t)bytes,
                          hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int pgmi_debug_lane_reduce(pgmi_ctx* x, int op, const float* in, int rows, float* out, void* stream) {
    if (!x || !in || !out) return fail(PGMI_E_ARG, "null argument");
    if (op < 0 || op >= kLaneReduceOps) return fail(PGMI_E_ARG, "lane reduce: unknown op");
    if (rows < 1) return fail(PGMI_E_ARG, "lane reduce: no rows");
    lane_reduce_rows((hipStream_t)stream, op, in, rows, out);
    LAUNCHCHK();
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

int pgmi_debug_attention_plan(int head_dim, int B, int Lq, int Lk, int G, int n_kv, int ragged, int64_t ws_floats,
                              int* kernel, int* waves, int* ranges, int* tiles_per_range) {
    if ((head_dim != 72 && head_dim != 256) || B < 1 || Lq < 1 || Lk < 1 || G < 1 || n_kv < 1 || ws_floats < 0 ||
        !kernel || !waves || !ranges || !tiles_per_range)
        return fail(PGMI_E_ARG, "bad argument");
    const AttnPlan p = attention_prefill_plan(head_dim, B, Lq, Lk, G, n_kv, ragged != 0, (long)ws_floats);
    *kernel = p.kernel;
    *waves = p.nw;
    *ranges = p.ns;
    *tiles_per_range = p.tps;
    return 0;
}

int pgmi_tune_gemm(int cfg, int split) {
    if ((cfg >= 0 && !gemm_cfg_valid(cfg)) || split < 0 || split > 32) return fail(PGMI_E_ARG, "bad GEMM plan");
    gemm_force_plan(cfg, split);
    tune_epoch(1);
    return 0;
}

int pgmi_tune_gemm_shape(int M, int N, int K, int dual, int cfg, int split) {
    if ((cfg >= 0 && !gemm_cfg_valid(cfg)) || split < 0 || split > 16) return fail(PGMI_E_ARG, "bad GEMM plan");
    if (gemm_force_shape(M, N, K, dual, cfg, split)) return fail(PGMI_E_ARG, "too many per-shape GEMM plans");
    tune_epoch(1);
    return 0;
}

int pgmi_tune_attention(int variant) {
    static const int ok[] = {-1, 0, 7, 41, 42, 21, 22, 44, 24, 9, 91, 92, 94, 81, 82};
    for (int v : ok)
        if (v == variant) {
            attention_force_variant(variant);
            tune_epoch(1);
            return 0;
        }
    return fail(PGMI_E_ARG, "unknown attention variant");
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

int pgmi_op_attention_prefix(pgmi_ctx* x, const void* q, const void* k, const void* v, void* o, int B, int Lq, int Lk,
                             int H, int Hkv, int hd, int kv_layout, float scale, int kv_start, const int32_t* klen,
                             const int32_t* prefix_lens, void* stream) {
    int rc;
    if (!x || !q || !k || !v || !o || !prefix_lens) return fail(PGMI_E_ARG, "null argument");
    if ((rc = ensure_prepared(x))) return rc;
    if (hd != 256) return fail(PGMI_E_ARG, "head_dim must be 256");
    if (B < 1 || B > kMaxRows || Lq < 1 || Hkv < 1 || H < 1 || H % Hkv != 0 || H / Hkv > 16)
        return fail(PGMI_E_ARG, "bad shape");
    if (kv_layout != 0 && kv_layout != 1) return fail(PGMI_E_ARG, "kv_layout must be 0 (B,L,Hkv,hd) or 1 (B,Hkv,L,hd)");
    if (kv_start < 0 || Lk < 1 || kv_start + Lq > Lk) return fail(PGMI_E_ARG, "kv_start + Lq keys exceed Lk");
    RowInts rk{}, rp{};
    bool causal = false;
    for (int b = 0; b < B; ++b) {
        const int kl = klen ? klen[b] : kv_start + Lq;
        if (kl <= kv_start || kl > kv_start + Lq) return fail(PGMI_E_ARG, "klen[b] must be in (kv_start, kv_start + Lq]");
        if (prefix_lens[b] < 0 || prefix_lens[b] > kl - kv_start)
            return fail(PGMI_E_ARG, "prefix_lens[b] must be in [0, klen[b] - kv_start]");
        rk.v[b] = kl;
        rp.v[b] = prefix_lens[b];
        causal = causal || prefix_lens[b] < kl - kv_start;
    }
    hipStream_t s = (hipStream_t)stream;
    set_prefix_rows(x, s, rk, rp, B);
    AttnArgs a{};
    a.q = reinterpret_cast<const uint16_t*>(q); a.q_b_stride = (long)Lq * H * hd; a.q_row_stride = H * hd; a.q_head_stride = hd;
    a.k = reinterpret_cast<const uint16_t*>(k); a.k_b_stride = (long)Lk * Hkv * hd;
    a.k_row_stride = kv_layout == 0 ? Hkv * hd : hd; a.k_head_stride = kv_layout == 0 ? hd : Lk * hd;
    a.v = reinterpret_cast<const uint16_t*>(v); a.v_b_stride = a.k_b_stride;
    a.v_row_stride = a.k_row_stride; a.v_head_stride = a.k_head_stride;
    a.o = reinterpret_cast<uint16_t*>(o); a.o_b_stride = a.q_b_stride; a.o_row_stride = H * hd; a.o_head_stride = hd;
    a.Lq = Lq; a.Lk = kv_start + Lq; a.G = H / Hkv; a.n_kv = Hkv; a.B = B; a.scale = scale;
    a.ws = x->ws; a.ws_floats = (long)(x->ws_bytes / sizeof(float));
    lm_attn_launch(x, s, a, 0, kv_start, klen != nullptr, causal);
    LAUNCHCHK();
    return 0;
}

int pgmi_op_attention_prefix_splits(pgmi_ctx* x, int B, int Lq, int H, int Hkv, int kv_start) {
    int rc;
    if (!x) return fail(PGMI_E_ARG, "null argument");
    if ((rc = ensure_prepared(x))) return rc;
    if (B < 1 || B > kMaxRows || Lq < 1 || Hkv < 1 || H < 1 || H % Hkv != 0 || kv_start < 0)
        return fail(PGMI_E_ARG, "bad shape");
    AttnArgs a{};
    a.Lq = Lq; a.Lk = kv_start + Lq; a.G = H / Hkv; a.n_kv = Hkv; a.B = B;
    a.ws = x->ws; a.ws_floats = (long)(x->ws_bytes / sizeof(float));
    return attention_prefill_splits(a);
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
