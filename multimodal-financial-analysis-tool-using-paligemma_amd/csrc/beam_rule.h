#pragma once
// beam_rule.h -- the rule of one beam-search step: transformers' _beam_search with
// do_sample=False, one stop token and early_stopping in {False, True}, restated so that every fp32 operation and
// every tie has one answer.  Written for the host and the device alike (LGR_HD).  Today only the host compiles it in
// (pgmi_beam_step_host runs bmr_group_step below): the device kernels are left out of the tree.
// pgmi/beam_np.py says the same in numpy.
//
// G groups (prompts) of K beams, C = 2K candidates per step, steps t = 0 .. n_tokens - 1 (t = 0 picks from the
// prefill's logits: one input row per group), one stop token eos (-1: none), V >= 2K.
//
//   value    x with -0 taken as +0 (so that "x descending" is an order on bit patterns); rows with NaN and rows
//            without a finite maximum are outside the rule, but tokens and parents stay in range for them too
//   score    s = fp32(fp32(x - lse_r) + run_r): lse_r the row's fp32 log-sum-exp (an INPUT of the rule), run_r
//            its running score (0 after a reset); two rounded operations, never contracted
//   in a row candidates rank by (x descending, token ascending); fp32 - and + are monotone, so a row's top C by
//            that rank are all the group's top C can hold of it
//   in a group the C candidates are the first C by (s descending, row ascending, in-row rank ascending)
//   hit_j    token_j == eos, or t == n_tokens - 1 (then every candidate hits)
//   running  beams for t + 1: the first K candidates with hit = 0, each (parent row, token, s); on the last step
//            none exists and the first K candidates are written instead, so ids and parents stay in range
//   pool     K slots per group (score, valid, step, parent row, token), valid slots first, score descending.
//            Unless the group is frozen, a candidate with hit_j and j < K enters with fp32(s_j / den[t + 1])
//            (IEEE division; den[n] = fp32(float64(n) ** length_penalty) comes from the host); the best K of old
//            and new stay: score descending, old before new, then candidate rank; empty slots lose to everything
//   freeze   after the merge heur_g &= fp32(run_best / den[t + 1]) > worst, worst the smallest pool score of a
//            full pool, else -inf, run_best the new first running score; the group is frozen once heur_g is 0,
//            and with early_stopping once its pool is full.  A frozen group's pool never changes again.
//   history  parent[t][row], token[t][row] of the running beams: written once per step, never overwritten; pool
//            slots point into it (step, parent row) and sequences are rebuilt on the host by walking back.
#include "logits_rule.h"

namespace pgmi {

constexpr int kBeamMaxK = 16;             // beams per group (G * K <= kMaxRows rows of one decode step)
constexpr int kBeamMaxC = 2 * kBeamMaxK;  // candidates per step
constexpr int kBeamHdrWords = 8;          // G, K, n_tokens, eos, early_stopping, V, 0, 0
constexpr int kBeamMinSlice = 2048;       // elements per slice of the device's first pass
constexpr int kBeamMaxParts = 4096;       // slices x C keys one row's merge holds in LDS (32 KiB)
constexpr int kBeamMaxSlices = 512;
constexpr int kBeamMaxSliceElems = 12288; // a slice's values in LDS (48 KiB)

// a candidate of one row as one integer: larger key = earlier in the row's rank.  0 is "no candidate" (a real
// key's low word is ~token >= 0x80000000).
LGR_HD uint64_t bmr_key(float x, int tok) {
    if (x == 0.f) x = 0.f;  // -0 -> +0
    return ((uint64_t)lgr_key(x) << 32) | (uint32_t)~(uint32_t)tok;
}
LGR_HD float bmr_key_x(uint64_t k) { return lgr_unkey((uint32_t)(k >> 32)); }
LGR_HD int bmr_key_tok(uint64_t k) { return (int)~(uint32_t)k; }

LGR_HD float bmr_score(float x, float lse, float run) { return lgr_add(lgr_sub(x, lse), run); }

LGR_HD float bmr_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// the state blob: offsets in 4-byte words.  [0, state_words) is the state proper (what a final read copies);
// the rest is the device step's scratch.
struct BeamLayout {
    int G, K, C, n_tokens, V, nb, slice;
    long den, run, heur, frozen, pool_score, pool_valid, pool_step, pool_parent, pool_token, hist_parent, hist_token;
    long state_words;
    long pm, ps, row_lse, part_keys, row_keys, total_words;
};

// false: the arguments are outside what a state can be laid out for
inline bool bmr_layout(int G, int K, int n_tokens, int V, BeamLayout* L) {
    if (G < 1 || K < 1 || K > kBeamMaxK || (long)G * K > 16 || n_tokens < 1 || V < 2 * K) return false;
    const int C = 2 * K;
    const int cap = kBeamMaxParts / C < kBeamMaxSlices ? kBeamMaxParts / C : kBeamMaxSlices;
    int slice = (V + cap - 1) / cap;
    slice = (slice + 255) / 256 * 256;
    if (slice < kBeamMinSlice) slice = kBeamMinSlice;
    if (slice > kBeamMaxSliceElems) return false;
    const long GK = (long)G * K;
    L->G = G; L->K = K; L->C = C; L->n_tokens = n_tokens; L->V = V;
    L->slice = slice;
    L->nb = (V + slice - 1) / slice;
    long o = kBeamHdrWords;
    L->den = o;         o += n_tokens + 1;
    L->run = o;         o += GK;
    L->heur = o;        o += G;
    L->frozen = o;      o += G;
    L->pool_score = o;  o += GK;
    L->pool_valid = o;  o += GK;
    L->pool_step = o;   o += GK;
    L->pool_parent = o; o += GK;
    L->pool_token = o;  o += GK;
    L->hist_parent = o; o += (long)n_tokens * GK;
    L->hist_token = o;  o += (long)n_tokens * GK;
    o = (o + 3) & ~3L;  // the scratch starts 16-byte aligned
    L->state_words = o;
    L->pm = o;          o += GK * L->nb;
    L->ps = o;          o += GK * L->nb;
    L->row_lse = o;     o += GK;
    o = (o + 3) & ~3L;
    L->part_keys = o;   o += 2 * GK * L->nb * C;
    L->row_keys = o;    o += 2 * GK * C;
    L->total_words = o;
    return true;
}

// one group's state, the pointers already at the group's first entry
struct BeamGroup {
    float* run;                                           // [K]
    int* heur;                                            // [1]
    int* frozen;                                          // [1]
    float* pool_score;                                    // [K]
    int *pool_valid, *pool_step, *pool_parent, *pool_token;
};

// One step of group g.  cx / ctok: each input row's top C in rank order, [rows_in][C], ctok < 0 where the row has
// no further candidate; lse: [rows_in]; den: the whole table.  next_ids, parent, hist_parent, hist_token: the
// group's K entries of the step's outputs and of history row t.
LGR_HD void bmr_group_step(int g, int K, int n_tokens, int eos, int early, int t, int rows_in, const float* cx,
                           const int* ctok, const float* lse, const float* den, const BeamGroup& st,
                           int64_t* next_ids, int* parent, int* hist_parent, int* hist_token) {
    const int C = 2 * K;
    float cs[kBeamMaxC];
    int crow[kBeamMaxC], ct[kBeamMaxC], ptr[kBeamMaxK];
    for (int r = 0; r < rows_in; ++r) ptr[r] = 0;
    for (int j = 0; j < C; ++j) {  // (s descending, row ascending, in-row rank ascending)
        int best = -1;
        float bs = 0.f;
        for (int r = 0; r < rows_in; ++r) {
            if (ptr[r] >= C || ctok[r * C + ptr[r]] < 0) continue;
            const float s = bmr_score(cx[r * C + ptr[r]], lse[r], st.run[r]);
            if (best < 0 || s > bs) {
                best = r;
                bs = s;
            }
        }
        if (best < 0) {  // V >= 2K leaves C candidates; kept in range all the same
            cs[j] = lgr_neg_inf();
            crow[j] = 0;
            ct[j] = 0;
            continue;
        }
        cs[j] = bs;
        crow[j] = best;
        ct[j] = ctok[best * C + ptr[best]];
        ++ptr[best];
    }
    const bool last = t >= n_tokens - 1;
    // running beams: the first K that do not hit, then (last step only) the first that do
    int n = 0;
    for (int pass = 0; pass < 2 && n < K; ++pass)
        for (int j = 0; j < C && n < K; ++j) {
            const bool hit = last || ct[j] == eos;
            if (hit != (pass == 1)) continue;
            st.run[n] = cs[j];
            next_ids[n] = ct[j];
            parent[n] = g * K + crow[j];
            hist_parent[n] = g * K + crow[j];
            hist_token[n] = ct[j];
            ++n;
        }
    const float d = den[t + 1];
    if (!*st.frozen) {
        for (int j = 0; j < K; ++j) {
            if (!(last || ct[j] == eos)) continue;
            const float sc = bmr_div(cs[j], d);
            int p = 0;
            while (p < K && st.pool_valid[p] && !(sc > st.pool_score[p])) ++p;
            if (p >= K) continue;
            for (int q = K - 1; q > p; --q) {
                st.pool_score[q] = st.pool_score[q - 1];
                st.pool_valid[q] = st.pool_valid[q - 1];
                st.pool_step[q] = st.pool_step[q - 1];
                st.pool_parent[q] = st.pool_parent[q - 1];
                st.pool_token[q] = st.pool_token[q - 1];
            }
            st.pool_score[p] = sc;
            st.pool_valid[p] = 1;
            st.pool_step[p] = t;
            st.pool_parent[p] = g * K + crow[j];
            st.pool_token[p] = ct[j];
        }
    }
    const bool full = st.pool_valid[K - 1] != 0;
    const float worst = full ? st.pool_score[K - 1] : lgr_neg_inf();
    if (!(bmr_div(st.run[0], d) > worst)) *st.heur = 0;
    if (!*st.heur || (early && full)) *st.frozen = 1;
}

}  // namespace pgmi
