// engine_prefill.hip -- libpgmi host side: the prefill -- vision tower, projector, embedding, the language-model
// forward (lock-step and ragged) in row groups and stages, lm_head, log-probabilities, the final hidden states,
// the in-situ GEMM probe and the prefill graph switch.
#include "engine_graph.h"

namespace pgmi_eng __attribute__((visibility("hidden"))) {

// What a language-model prefill does before its launches, shared by lm_forward and the stage hook
// (pgmi_debug_prefill_stage): the argument checks, the ragged rows' lengths and the positions to the device.
int lm_begin(pgmi_ctx* x, const int64_t* ids, const void* embeds, int B, int L, const int64_t* positions,
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

// the prefill's entry, for the whole batch: the merged (or given) embeddings x the normalizer -> Hs
void lm_entry(const pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
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
bool run_last_only(const pgmi_ctx* x, const PrefillRun& r) {
    return r.logits_rows == 2 && r.L > 1 && x->c.t_layers > 0;
}

// input RMSNorm of layer 0; every later RMSNorm (and the final norm) is fused with the
// preceding projection's split-K reduction + residual (splitk_res_norm)
void lm_in_norm(const pgmi_ctx* x, const PrefillRun& r) {
    const pgmi_config& c = x->c;
    rmsnorm(r.s, run_hs(x, r), c.t_layers ? x->w.t[0].in_norm : x->w.final_norm, c.t_rms_eps, run_tn(x, r), r.B * r.L,
            c.t_hidden);
}

// layer i's q|k|v with RoPE and the KV append: Tn -> Qr, the cache rows
void lm_qkv(const pgmi_ctx* x, const PrefillRun& r, int i) {
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
    return a;  // klen: lm_attn_launch (the last-row tail is lock-step)
}

void set_prefix_rows(const pgmi_ctx* x, hipStream_t s, const RowInts& klen, const RowInts& pfx, int B) {
    set_row_ints(s, x->d_rlens + kMaxRows, klen, pfx, B);
}

// The one launcher of the prefill attention with per-row values (lm_attn and pgmi_op_attention_prefix): causal --
// some row of the call has tokens after its prefix -- takes the per-query key limits of k_attn_fs over the rows'
// key counts and prefix lengths (set_prefix_rows); otherwise a call is what it was, the ragged form over the key
// counts (a ragged row's real tokens attend its own real keys only) or the lock-step kernels.
void lm_attn_launch(const pgmi_ctx* x, hipStream_t s, AttnArgs a, int b0, int kv_start, bool ragged, bool causal) {
    a.klen = ragged || causal ? x->d_rlens + kMaxRows + b0 : nullptr;
    if (!causal) {
        attention_prefill(s, 256, a);
        return;
    }
    AttnPrefixArgs p{};
    static_cast<AttnArgs&>(p) = a;
    p.pfx = x->d_rlens + 2 * kMaxRows + b0;
    p.kv_start = kv_start;
    attention_prefill_prefix(s, p);
}

// layer i's attention: Qr, the cache rows -> AO
void lm_attn(const pgmi_ctx* x, const PrefillRun& r, int i) {
    lm_attn_launch(x, r.s, lm_attn_args(x, r, i), r.b0, r.kv_start, r.ragged, r.prefix);
}

// layer i's o_proj partial slabs, then their sum + residual and the post-attention norm: AO, Hs -> Hs, Tn
void lm_o_proj(const pgmi_ctx* x, const PrefillRun& r, int i) {
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
void lm_gate_up(const pgmi_ctx* x, const PrefillRun& r, int i) {
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
void lm_down(const pgmi_ctx* x, const PrefillRun& r, int i) {
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
int lm_last_row_tail(const pgmi_ctx* x, const PrefillRun& r, int i) {
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
               pk_use_rows(x, B, PK_GATE_UP, w.pk_gate_up));
    gemv_res(s, B, c.t_intermediate, x->dACT, w.down, H, lastrows, x->ws,
             pk_use_rows(x, B, PK_DOWN, w.pk_down));
    return 0;
}

// the group's logits: every row's (logits_rows 0, Tn holds the final RMSNorm, modeling_gemma.py:379) or each
// sequence's last row's (lastrows: copied or gathered here, or lm_last_row_tail's)
int lm_logits(const pgmi_ctx* x, const PrefillRun& r) {
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
                    nullptr, nullptr, nullptr, nullptr, 1, pk_use_rows(x, B, PK_LM_HEAD, x->w.pk_embed));
    }
    return 0;
}

// The lm_head GEMM with the EPI_LSE epilogue + the combine, over row chunks whose tile pairs fit the split-K
// workspace (pairs [chunk][column tiles] first, the label logits [chunk] behind them): nothing of rows x V is kept.
int lm_logprobs_run(pgmi_ctx* x, const void* normed, const uint16_t* W, int rows, int V, int K,
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

}  // namespace pgmi_eng

extern "C" {

static int vision_body(const pgmi_ctx* x, hipStream_t s, const void* pixels, int dtype, int B, void* feats);

int pgmi_vision(pgmi_ctx* x, const void* pixels, int dtype, int B, void* feats, void* stream) {
    int rc;
    if ((rc = ensure_prepared(x))) return rc;
    const pgmi_config& c = x->c;
    if (B < 1 || B > c.max_batch) return fail(PGMI_E_ARG, "batch exceeds max_batch");
    if (!pixels || !feats) return fail(PGMI_E_ARG, "null argument");
    const std::vector<intptr_t> key = prefill_key(1, {(intptr_t)pixels, dtype, B, (intptr_t)feats});
    const pgmi_ctx* const cx = x;  // the body's view of the context (engine_graph.h)
    // more than kPrefillGroup images: row groups of that many, one after the other through the same workspace, each
    // with the plans measured for it -- an image's features do not depend on how many images share the call
    const size_t px_img = (size_t)c.v_channels * c.v_image * c.v_image * (dtype == PGMI_DTYPE_F32 ? 4 : 2);
    const size_t ft_img = (size_t)n_img(c) * c.v_hidden * sizeof(uint16_t);
    rc = run_prefill(x, (hipStream_t)stream, key, [&, cx](hipStream_t st) {
        for (int b0 = 0; b0 < B; b0 += kPrefillGroup) {
            const int r = vision_body(cx, st, reinterpret_cast<const char*>(pixels) + b0 * px_img, dtype,
                                      std::min(kPrefillGroup, B - b0), reinterpret_cast<char*>(feats) + b0 * ft_img);
            if (r) return r;
        }
        return 0;
    });
    if (rc) return rc;
    LAUNCHCHK();
    return 0;
}

static int vision_body(const pgmi_ctx* x, hipStream_t s, const void* pixels, int dtype, int B, void* feats) {
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

static int lm_body(const pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
                   const void* embeds, int B, int L, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
                   int logits_rows, bool ragged, bool prefix = false);

static int lm_rows(const pgmi_ctx* x, const PrefillRun& r);

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

static int lm_forward(pgmi_ctx* x, const int64_t* ids, const void* image_feats, int n_img_rows, const void* embeds,
                      int B, int L, const int64_t* positions, const int32_t* lens, bool ragged, void* kv, int kv_batch,
                      int kv_max, int kv_start, float* logits, int logits_rows, void* stream) {
    int rc;
    if ((rc = lm_begin(x, ids, embeds, B, L, positions, lens, ragged, kv, kv_batch, kv_max, kv_start, logits,
                       &logits_rows, stream)))
        return rc;
    const std::vector<intptr_t> key =
        prefill_key(2, {(intptr_t)ids, (intptr_t)image_feats, n_img_rows, (intptr_t)embeds, B, L, (intptr_t)kv, kv_batch,
                        kv_max, kv_start, (intptr_t)logits, logits_rows, (intptr_t)ragged});
    const pgmi_ctx* const cx = x;  // the body's view of the context (engine_graph.h)
    rc = run_prefill(x, (hipStream_t)stream, key, [&, cx](hipStream_t st) {
        return lm_body(cx, st, ids, image_feats, n_img_rows, embeds, B, L, kv, kv_batch, kv_max, kv_start, logits,
                       logits_rows, ragged);
    });
    if (rc) return rc;
    x->tn_rows = logits_rows == 2 && L > 1 ? 0 : (long)B * L;
    LAUNCHCHK();
    return 0;
}

int pgmi_lm_forward_prefix(pgmi_ctx* x, const int64_t* ids, const void* image_feats, int n_img_rows, int B, int L,
                           const int64_t* positions, const int32_t* lens, const int32_t* prefix_lens, void* kv,
                           int kv_batch, int kv_max, int kv_start, float* logits, int logits_rows, void* stream) {
    if (!prefix_lens || !ids) return fail(PGMI_E_ARG, "null argument");
    const bool ragged = lens != nullptr;
    // before lm_begin writes anything: a refused call leaves the last call's positions, lengths and final rows
    for (int b = 0; b < B && b < kMaxRows; ++b)
        if (prefix_lens[b] < 0 || prefix_lens[b] > (ragged ? lens[b] : L))
            return fail(PGMI_E_ARG, "prefix_lens[b] must be in [0, lens[b]]");
    int rc;
    if ((rc = lm_begin(x, ids, nullptr, B, L, positions, lens, ragged, kv, kv_batch, kv_max, kv_start, logits,
                       &logits_rows, stream)))
        return rc;
    // the rows' key counts and prefix lengths -> the device, outside any graph (there is none here); causal: some
    // row has tokens after its prefix -- otherwise every launch is pgmi_lm_forward's / _ragged's
    RowInts rk{}, rp{};
    bool causal = false;
    for (int b = 0; b < B; ++b) {
        const int len = ragged ? lens[b] : L;
        rk.v[b] = kv_start + len;
        rp.v[b] = prefix_lens[b];
        causal = causal || prefix_lens[b] < len;
    }
    set_prefix_rows(x, (hipStream_t)stream, rk, rp, B);
    LAUNCHCHK();
    // eager, on the caller's stream: no key is looked up or inserted (engine_graph.h, point 4)
    if ((rc = lm_body(x, (hipStream_t)stream, ids, image_feats, n_img_rows, nullptr, B, L, kv, kv_batch, kv_max,
                      kv_start, logits, logits_rows, ragged, causal)))
        return rc;
    x->tn_rows = logits_rows == 2 && L > 1 ? 0 : (long)B * L;
    LAUNCHCHK();
    return 0;
}

static int lm_body(const pgmi_ctx* x, hipStream_t s, const int64_t* ids, const void* image_feats, int n_img_rows,
                   const void* embeds, int B, int L, void* kv, int kv_batch, int kv_max, int kv_start, float* logits,
                   int logits_rows, bool ragged, bool prefix) {
    lm_entry(x, s, ids, image_feats, n_img_rows, embeds, B, L, ragged);
    // the layers: row groups of at most kPrefillGroup sequences, one after the other (the merge above ran for the
    // whole batch: the k-th <image> token of the batch takes image row k); a group's rows of Hs / Tn, its positions,
    // lengths, KV rows and logits are its slice of the batch's, everything else is scratch that the groups share
    for (int b0 = 0; b0 < B; b0 += kPrefillGroup) {
        const PrefillRun r{s, b0, std::min(kPrefillGroup, B - b0), L, kv, kv_batch, kv_max, kv_start, logits,
                           logits_rows, ragged, prefix};
        if (int rc = lm_rows(x, r)) return rc;
    }
    return 0;
}

static int lm_rows(const pgmi_ctx* x, const PrefillRun& r) {
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
    graphs_drop(x, GRAPHS_PREFILL);
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

int pgmi_set_prefill_graph(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    if (x->probe_on) x->graph_before_probe = on != 0;  // applied when the probe is turned off
    else x->prefill_graph = on != 0;
    graphs_drop(x, GRAPHS_PREFILL);
    return 0;
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

}  // extern "C"
