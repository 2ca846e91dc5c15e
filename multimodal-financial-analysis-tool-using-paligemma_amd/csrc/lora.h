#pragma once
// lora.h -- the rule by which a LoRA adapter is merged into a bf16 weight, compiled for
// the host (pgmi_lora_merge_host, the tests' statement of the rule) and for the device (kernels_lora.hip).
//
// For a weight W[N][K] (bf16, the PRISTINE base), factors A[r][K] and B[N][r] in fp32 and a scale s in fp32:
//
//   acc = 0.0f
//   for j = 0 .. r-1, ascending:  acc = acc + (B[n][j] * A[j][k])      fp32 multiply, then fp32 add: not fused
//   W'[n][k] = bf16_rne( fp32(W[n][k]) + acc * s )                      again a multiply, then an add
//
// One rounding, always from the pristine base: switching adapters any number of times cannot drift.  Every
// element is a function of its own row of B, its own column of A and its own W alone, in a fixed order, so which
// thread (or which host loop) owns an element cannot change a bit of it.  The multiply and the add are kept
// apart by the contraction pragma in the two functions that spell them, on both sides, not by a compiler flag:
// built without -ffp-contract=off the kernel still has no fused multiply-add.  (HIP's __fmul_rn / __fadd_rn
// would not do that: the headers define them as a plain x * y / x + y under the translation unit's own
// contraction mode, and the pair fuses -- seen in the ISA.)  The bf16 rounding is the integer form on both sides
// (a NaN becomes the quiet NaN of its sign), so host and device agree for every input.
#include "common.h"

namespace pgmi {

#define LORA_HD __host__ __device__ __forceinline__

constexpr int kLoraMaxRank = 256;  // r of a target, taken from its factors' shapes, lies in [1, 256]

LORA_HD float lora_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

LORA_HD float lora_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

LORA_HD float lora_bits_f(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}

LORA_HD uint32_t lora_f_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
#endif
}

// fp32 -> bf16, round to nearest even
LORA_HD uint16_t lora_bf16_rne(float f) {
    const uint32_t u = lora_f_bits(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// one step of the rank loop
LORA_HD float lora_step(float acc, float b, float a) { return lora_add(acc, lora_mul(b, a)); }

// the merged element from the pristine one and the finished rank sum
LORA_HD uint16_t lora_finish(uint16_t w, float acc, float s) {
    return lora_bf16_rne(lora_add(lora_bits_f((uint32_t)w << 16), lora_mul(acc, s)));
}

}  // namespace pgmi
