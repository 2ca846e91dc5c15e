// engine_decode.hip -- libpgmi host side: one decode step (head, layers, tail), the step's entry points (token
// ids, embeddings, ragged rows, several steps per call) with their graph cache, and what follows a step: argmax,
// end-of-sequence update and nucleus sampling.
#include "engine_graph.h"

namespace pgmi_eng __attribute__((visibility("hidden"))) {

// The batched form's RMSNorms: computed once per row -- the input norm by the down projection's combine for
// the next layer (k_mf_combine_norm; q|k|v reads dHn unstaged), the post-attention norm from o_proj's 16-column
// partial sums of squares, applied by gate|up as it loads h (default) -- or each projection stages and
// normalises its rows itself (pgmi_set_decode_staged_norm,
// tested by test_batch_rows_teacher_forced_vs_own_reference[8-1]).  Round 4, the unstaged form reading rows
// normalised by separate passes against the staged form: equal
// while the weight streams were non-temporal (B = 8 step 1.5449 vs 1.5452 ms); with the default cache policy
// (kernels_gemv_mfma.hip PGMI_MF_NT) the unstaged form wins, same box: 1.4523 / 1.4550 -> 1.4330 / 1.4320 ms
static bool mf_staged(const pgmi_ctx* x) { return x->mf_staged > 0; }

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

// the step's entry: h (unless layer 0's q|k|v folds the embedding) and, unstaged, layer 0's normed rows
void decode_head(const pgmi_ctx* x, const DecodeRun& r) {
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
void decode_layer(const pgmi_ctx* x, const DecodeRun& r, int i, int stage) {
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
            gemv_geglu(s, B, x->dH, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, x->dSS, w.mf_gate_up,
                       pk_use(x, B, PK_GATE_UP, w.pk_gate_up));
        if (on(4))
            gemv_res_norm(s, B, c.t_intermediate, x->dACT, w.down, H, x->dH, x->ws,
                          i + 1 < c.t_layers ? x->w.t[i + 1].in_norm : nullptr, eps, x->dHn, w.mf_down,
                          pk_use(x, B, PK_DOWN, w.pk_down));
        return;
    }
    if (on(3))
        gemv_geglu(s, B, x->dH, w.post_norm, eps, w.gate_up, c.t_intermediate, x->dACT, nullptr, nullptr,
                   pk_use(x, B, PK_GATE_UP, w.pk_gate_up));
    if (on(4))
        gemv_res(s, B, c.t_intermediate, x->dACT, w.down, H, x->dH, x->ws,
                 pk_use(x, B, PK_DOWN, w.pk_down));
}

// final norm + lm_head + argmax.  The step's last work also advances the device step state (pgmi_decode
// skips its host-side set when the next call continues the sequence): lm_head's last workgroup, or argmax_finish
void decode_tail(const pgmi_ctx* x, const DecodeRun& r, float* logits, int64_t* next_ids, int64_t* hist) {
    const pgmi_config& c = x->c;
    StepState* const st = run_step(x, r);
    const int adv_n = r.ragged ? r.B : 1;
    int nparts = 0;
    int64_t* nx = next_ids ? next_ids : x->d_next;
    if (!gemv_logits(r.s, r.B, x->dH, x->w.final_norm, c.t_rms_eps, x->w.embed, c.t_vocab, logits, x->pmax, x->pidx,
                     &nparts, x->lm_done, nx, st, hist, adv_n, pk_use(x, r.B, PK_LM_HEAD, x->w.pk_embed)))
        argmax_finish(r.s, r.B, x->pmax, x->pidx, nparts, nx, st, hist, adv_n);
}

}  // namespace pgmi_eng

extern "C" {

static int decode_body(const pgmi_ctx* x, hipStream_t s, const int64_t* ids, int B, void* kv, int kv_batch,
                       int kv_max, int launch_keys, float* logits, int64_t* next_ids, const uint16_t* embeds = nullptr,
                       int masked = 0, int64_t* hist = nullptr, bool ragged = false) {
    const DecodeRun r{s, ids, embeds, B, kv, kv_batch, kv_max, launch_keys, masked, ragged};
    decode_head(x, r);
    for (int i = 0; i < x->c.t_layers; ++i) decode_layer(x, r, i);
    decode_tail(x, r, logits, next_ids, hist);
    return launcher_error();  // (inside a capture too: a step with a launch missing is never instantiated)
}

int pgmi_set_decode_staged_norm(pgmi_ctx* x, int on) {
    if (!x) return fail(PGMI_E_ARG, "null context");
    x->mf_staged = on < 0 ? -1 : on != 0;
    graphs_drop(x, GRAPHS_DECODE);  // captured steps hold the other form's launches
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
    if ((rc = ensure_decode_images(x, s, B))) return rc;
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
    const pgmi_ctx* const cx = x;  // the body's view of the context (engine_graph.h)
    auto body = [&, cx](hipStream_t st, const int64_t* first, int keys0, bool grow) -> int {
        for (int t = 0; t < n_steps; ++t) {
            const int r = decode_body(cx, st, t == 0 ? first : fb, B, kv, kv_batch, kv_max, grow ? keys0 + t : keys0,
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
    const std::vector<intptr_t> key = decode_key(B, {
        (intptr_t)kv, kv_batch, kv_max, (intptr_t)logits, (intptr_t)next_ids,
        (intptr_t)gids,      // the ids buffer the graph reads (the context's staging copy, or in place)
        embeds != nullptr,   // the step's input is the staged embedding rows (pgmi_decode_embeds), not ids
        masked,              // 0: no mask (a zero word), 1: staged bf16 mask (sum rounded), 2: staged fp32 mask
        n_steps,             // decode steps captured back to back (pgmi_decode_steps; 1 otherwise)
        (intptr_t)tokens,    // their per-step token record ([n_steps][B], may be null)
        ragged});            // per-row step records (pgmi_decode_ragged): never aliases a lock-step graph
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

}  // extern "C"
