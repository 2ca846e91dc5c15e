#pragma once
// logits_rule.h -- the rule by which generate's logit processors edit one row of step logits,
// written for the host and the device alike (LGR_HD).  Today only the host compiles it in (pgmi_logits_process_host,
// the tests' statement of the rule): the device kernels are left out of the tree.
// pgmi/logits_np.py says the same in numpy.
//
// One row x[V] (fp32) and its history word h[v] (uint32): in_prompt = h >> 31, n_out = h & 0x7fffffff,
// seen = in_prompt | (n_out > 0).
//
// Stage 1, per element, in this order; a step whose parameter is neutral is SKIPPED (never x + 0 or x / 1), so
// neutral parameters leave every bit of x, -0 included:
//   1. rp != 1 and seen:  x = x < 0 ? x * rp : x / rp      HF RepetitionPenaltyLogitsProcessor, over prompt and output;
//                                                          one correctly rounded fp32 operation
//   2. fp != 0:           t = fp * float(n_out); x = x - t   frequency penalty over emitted tokens (OpenAI / vLLM):
//                                                          a multiply, then a subtract, not fused
//      pp != 0, n_out > 0: x = x - pp                       presence penalty
//   3. bias present:      x = x + bias[v]                   -inf bans; +inf / NaN are refused by the caller
//   4. suppress on:       x[suppress_id] = -inf             while the row has emitted < min_new_tokens tokens
//
// Stage 2 (sampling only), on the stage-1 row y with m = max(y): thr = max(kth, m + delta) where kth is the k-th
// largest VALUE of y (top-k on: 1 <= k < V; else -inf) and delta = fp32(T ln(min_p)) <= 0 comes from the host
// (-inf: min-p off); y < thr becomes -inf.  A comparison by value: ties at kth all stay, -0 == +0, and the maximum
// always survives.  Guard: m == -inf (everything banned) returns the RAW x.  Rows with NaN are outside the rule.
#include "common.h"

namespace pgmi {

#define LGR_HD __host__ __device__ __forceinline__

struct LogitsRule {  // pgmi_logits_params, with the on / off decisions taken once
    float rp, pp, fp;
    int use_rp, use_pp, use_fp;
    int suppress_id;      // -1: off
    int min_new_tokens;
    int top_k;            // 0: off (k <= 0 or k >= V)
    float delta;          // min-p: keep y >= m + delta; -inf: off
};

LGR_HD float lgr_bits_f(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}

LGR_HD uint32_t lgr_f_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
#endif
}

LGR_HD float lgr_neg_inf() { return lgr_bits_f(0xFF800000u); }

LGR_HD float lgr_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

LGR_HD float lgr_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

LGR_HD float lgr_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// stage 1, steps 1-3, of one element
LGR_HD float lgr_stage1(float x, uint32_t h, const LogitsRule& R, bool has_bias, float bias) {
    const uint32_t n_out = h & 0x7FFFFFFFu;
    if (R.use_rp && h != 0u) x = x < 0.f ? lgr_mul(x, R.rp) : x / R.rp;
    if (R.use_fp) x = lgr_sub(x, lgr_mul(R.fp, (float)n_out));
    if (R.use_pp && n_out != 0u) x = lgr_sub(x, R.pp);
    if (has_bias) x = lgr_add(x, bias);
    return x;
}

// the row's threshold from its k-th largest value (-inf: top-k off) and its maximum
LGR_HD float lgr_threshold(float kth, float m, float delta) {
    float thr = kth;
    if (delta != lgr_neg_inf()) {
        const float t = lgr_add(m, delta);
        if (t > thr) thr = t;
    }
    return thr;
}

LGR_HD float lgr_stage2(float y, float thr) { return y < thr ? lgr_neg_inf() : y; }

// order-preserving key of a non-NaN fp32: a < b as floats => key(a) < key(b) as unsigned (-0 sorts just below +0;
// the threshold compare is by value, so which zero the k-th key names does not matter)
LGR_HD uint32_t lgr_key(float v) {
    const uint32_t u = lgr_f_bits(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

LGR_HD float lgr_unkey(uint32_t k) { return lgr_bits_f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

}  // namespace pgmi
