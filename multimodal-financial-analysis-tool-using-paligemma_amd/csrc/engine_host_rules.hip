// engine_host_rules.hip -- libpgmi host side: the rules that run on the host alone, through the very functions
// the kernels use (logits_rule.h, beam_rule.h).  They need no context and no GPU.
#include "engine_ctx.h"
#include "beam_rule.h"
#include "logits_rule.h"

extern "C" {

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

}  // extern "C"
