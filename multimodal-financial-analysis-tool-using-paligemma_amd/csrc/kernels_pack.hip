// kernels_pack.hip -- builds the 13-bit weight images of the decode GEMVs (pack13.h; row-major segments for batch
// 1-2, fragment-major ones for the batched step): pass one finds a tensor's exponent range (does it fit?), pass two
// writes the image, one kernel over the form.  Run once per pgmi_prepare, off the hot path.
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

// one thread per (segment, lane) of either form's image (pack13.h: pk_segs, pk_src): four 16-B fragments in -- zeros
// for a lane whose row is past the last one -- the lane's 52 bytes of the segment out
template <PkForm F>
__global__ void __launch_bounds__(256) k_pk_pack(const uint16_t* __restrict__ W, long rows, int K, long n_items,
                                                 int e_hi, uint8_t* __restrict__ out) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    const int l = (int)(t & 63);
    const long seg = t >> 6;
    uint4 f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long off = pk_src(F, seg, l, c, K);
        f[c] = off < rows * K ? ldg16(W + off) : make_uint4(0, 0, 0, 0);
    }
    pk_put(out + seg * kPkSegBytes, l, pk_encode(f, e_hi));
}

void pk_scan(hipStream_t s, const uint16_t* W, long numel, unsigned* stat) {
    const long n16 = numel / 8;
    long blocks = (n16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_pk_scan, dim3((unsigned)blocks), dim3(256), 0, s, W, n16, stat);
}

void pk_pack(hipStream_t s, int form, const uint16_t* W, long rows, int K, int e_hi, uint8_t* out) {
    const long n = (long)pk_segs((PkForm)form, rows, K) * 64;
    const auto k = form == PK_FORM_FRAG ? k_pk_pack<PK_FORM_FRAG> : k_pk_pack<PK_FORM_ROWS>;
    hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, rows, K, n, e_hi, out);
}

}  // namespace pgmi
