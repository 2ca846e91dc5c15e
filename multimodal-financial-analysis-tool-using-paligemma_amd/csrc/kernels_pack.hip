// kernels_pack.hip -- builds the 13-bit weight images of the decode GEMVs (pack13.h; row-major segments for batch
// 1-2, fragment-major ones for the batched step): pass one finds
// a tensor's exponent range (does it fit?), pass two writes the image.  Run once per pgmi_prepare, off the hot path.
#include "launch.h"
#include "pack13.h"

namespace pgmi {

// stat[0] = largest exponent field, stat[1] = smallest exponent field >= 1 (untouched 0xFFFFFFFF: none)
__global__ void __launch_bounds__(256) k_pk_scan(const uint16_t* __restrict__ W, long n16, unsigned* __restrict__ stat) {
    unsigned hi = 0, lo = 0xFFFFFFFFu;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
        const uint4 v = ldg16(W + i * 8);
        const uint16_t* e = reinterpret_cast<const uint16_t*>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned ex = (e[j] >> 7) & 0xFFu;
            hi = ex > hi ? ex : hi;
            if (ex) lo = ex < lo ? ex : lo;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned h2 = __shfl_xor(hi, o, 64), l2 = __shfl_xor(lo, o, 64);
        hi = h2 > hi ? h2 : hi;
        lo = l2 < lo ? l2 : lo;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(stat, hi);
        atomicMin(stat + 1, lo);
    }
}

// one thread per (segment, lane): four 16-B fragments in, the lane's 52 bytes of the segment out
__global__ void __launch_bounds__(256) k_pk_pack(const uint16_t* __restrict__ W, long n_items, int e_hi,
                                                 uint8_t* __restrict__ out) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    const int l = (int)(t & 63);
    const long seg = t >> 6;
    const uint16_t* src = W + seg * kPkSegK + 8 * l;
    uint4 f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = ldg16(src + 512 * c);
    const PkSeg s = pk_encode(f, e_hi);
    uint8_t* dst = out + seg * kPkSegBytes;
    *reinterpret_cast<uint4*>(dst + pk_off_a(l)) = s.a;
    *reinterpret_cast<uint4*>(dst + pk_off_b(l)) = s.b;
    *reinterpret_cast<uint4*>(dst + pk_off_n(l)) = s.n;
    *reinterpret_cast<unsigned*>(dst + pk_off_h(l)) = s.h;
}

// the fragment-major gather (pack13.h): one thread per (segment, lane) of the ceil(rows / 16) x K / 128 segments; a
// lane whose row is past the last one encodes zeros
__global__ void __launch_bounds__(256) k_pk_pack_mf(const uint16_t* __restrict__ W, long rows, int K, long n_items,
                                                    int e_hi, uint8_t* __restrict__ out) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    const int l = (int)(t & 63);
    const long seg = t >> 6, kbs = K / kPkMfK;
    const long gr = seg / kbs, kb = seg % kbs;
    const long row = pk_mf_row(gr, l);
    uint4 f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        f[c] = row < rows ? ldg16(W + row * K + pk_mf_k(kb, l, c)) : make_uint4(0, 0, 0, 0);
    const PkSeg s = pk_encode(f, e_hi);
    uint8_t* dst = out + seg * kPkSegBytes;
    *reinterpret_cast<uint4*>(dst + pk_off_a(l)) = s.a;
    *reinterpret_cast<uint4*>(dst + pk_off_b(l)) = s.b;
    *reinterpret_cast<uint4*>(dst + pk_off_n(l)) = s.n;
    *reinterpret_cast<unsigned*>(dst + pk_off_h(l)) = s.h;
}

void pk_scan(hipStream_t s, const uint16_t* W, long numel, unsigned* stat) {
    const long n16 = numel / 8;
    long blocks = (n16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_pk_scan, dim3((unsigned)blocks), dim3(256), 0, s, W, n16, stat);
}

void pk_pack(hipStream_t s, const uint16_t* W, long rows, int K, int e_hi, uint8_t* out) {
    const long n = rows * (K / kPkSegK) * 64;
    hipLaunchKernelGGL(k_pk_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, n, e_hi, out);
}

void pk_pack_mf(hipStream_t s, const uint16_t* W, long rows, int K, int e_hi, uint8_t* out) {
    const long n = (long)pk_mf_groups(rows) * (K / kPkMfK) * 64;
    hipLaunchKernelGGL(k_pk_pack_mf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, rows, K, n, e_hi, out);
}

}  // namespace pgmi
