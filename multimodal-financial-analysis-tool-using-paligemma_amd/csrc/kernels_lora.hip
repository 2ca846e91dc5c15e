// kernels_lora.hip -- merges a LoRA adapter into one bf16 weight by the rule of lora.h.  Run when an adapter is
// activated or switched (pgmi_lora_set), off the hot path: the forward kernels read the merged slab as they read
// the base.  Memory-bound: the pristine W is read once in 16-B lanes, the merged W written once; the fp32 A rows
// (r x K, at most a few MB) are read coalesced and stay in L2, B[n][.] is uniform per row.
#include "launch.h"
#include "lora.h"

namespace pgmi {

constexpr int kLoraRows = 4;  // rows per workgroup: each A value a thread loads serves this many rows

// One thread owns the 8 weights k0 .. k0 + 7 of kLoraRows consecutive rows.  K is a multiple of 8, so a thread's
// 16-B lane of W and its two 16-B lanes of A lie inside their rows or the thread has nothing to do (K tail); rows
// past N are neither loaded nor stored (row tail; the B loads of such a row read row N - 1 instead).
__global__ void __launch_bounds__(256) k_lora_merge(const uint16_t* __restrict__ W, int N, int K,
                                                    const float* __restrict__ A, const float* __restrict__ B, int r,
                                                    float s, uint16_t* __restrict__ out) {
    const long k0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (k0 >= K) return;
    for (long n0 = (long)blockIdx.y * kLoraRows; n0 < N; n0 += (long)gridDim.y * kLoraRows) {
        float acc[kLoraRows][8];
        const float* brow[kLoraRows];
#pragma unroll
        for (int i = 0; i < kLoraRows; ++i) {
            const long n = n0 + i < N ? n0 + i : (long)N - 1;
            brow[i] = B + n * r;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
        }
        for (int j = 0; j < r; ++j) {
            const float4 a0 = *reinterpret_cast<const float4*>(A + (long)j * K + k0);
            const float4 a1 = *reinterpret_cast<const float4*>(A + (long)j * K + k0 + 4);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int i = 0; i < kLoraRows; ++i) {
                const float b = brow[i][j];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[i][e] = lora_step(acc[i][e], b, a[e]);
            }
        }
#pragma unroll
        for (int i = 0; i < kLoraRows; ++i) {
            if (n0 + i >= N) break;
            const u16x8 w = *reinterpret_cast<const u16x8*>(W + (n0 + i) * K + k0);
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o.v[e] = lora_finish(w.v[e], acc[i][e], s);
            *reinterpret_cast<u16x8*>(out + (n0 + i) * K + k0) = o;
        }
    }
}

// factors as they arrive on the device (BF16 / F16 / F32) widened to the resident fp32 form, exactly
__global__ void __launch_bounds__(256) k_lora_widen(const void* __restrict__ src, int dtype, long n,
                                                    float* __restrict__ dst) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (dtype == 2) dst[i] = reinterpret_cast<const float*>(src)[i];
        else if (dtype == 1) dst[i] = (float)reinterpret_cast<const _Float16*>(src)[i];
        else dst[i] = bf2f(reinterpret_cast<const uint16_t*>(src)[i]);
    }
}

void lora_merge(hipStream_t s, const uint16_t* W, int N, int K, const float* A, const float* B, int r, float scaling,
                uint16_t* out) {
    if (N < 1 || K < 8 || K % 8 != 0 || r < 1 || r > kLoraMaxRank) {
        launch_error_set(hipErrorInvalidValue, "lora_merge: N >= 1, K a positive multiple of 8, r in [1, 256]");
        return;
    }
    const long gx = ((long)K / 8 + 255) / 256;
    long gy = ((long)N + kLoraRows - 1) / kLoraRows;
    if (gy > 32768) gy = 32768;  // further rows: the kernel's row loop
    hipLaunchKernelGGL(k_lora_merge, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, W, N, K, A, B, r, scaling, out);
}

void lora_widen(hipStream_t s, const void* src, int dtype, long n, float* dst) {
    long blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_lora_widen, dim3((unsigned)blocks), dim3(256), 0, s, src, dtype, n, dst);
}

}  // namespace pgmi
