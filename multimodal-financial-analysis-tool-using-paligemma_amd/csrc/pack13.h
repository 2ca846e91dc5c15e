#pragma once
// pack13.h -- the lossless 13-bit image of a bf16 weight matrix that the streaming decode GEMVs read at
// batch 1-2 (gemv_body.h, PK kernels).
//
// A bf16 weight is sign(1) | exponent field(8) | mantissa(7).  With e_hi the largest exponent field of the
// tensor, a weight is stored as
//   - one byte sm = sign << 7 | mantissa, and
//   - a 5-bit code c = e_hi - exponent (0..30), or c = 31 for exponent field 0 (zeros of either sign and
//     denormals, whose mantissa and sign stay in sm).
// A tensor FITS when no element has an exponent field in [1, e_hi - 31]; a tensor that does not fit keeps the
// bf16 kernel as a whole (no escape inside the image).  The planes hold u = 31 - c (= c ^ 31), so that the
// exponent field is rebuilt as u ? u + (e_hi - 31) : 0 without a subtraction from a per-tensor constant.
//
// Byte layout.  A row of K weights (K a multiple of 2048) is K / 2048 segments of 3328 bytes; rows follow each
// other without padding.  A segment serves the 64 lanes of one wave: lane l owns the weights
// k = 512 c + 8 l + j (chunk c < 4, j < 8) -- the four 16-byte fragments the bf16 kernel loads for it -- and
//   bytes [   0, 1024): 16 B per lane, sm of chunk 0 (j = 0..7) then chunk 1
//   bytes [1024, 2048): 16 B per lane, sm of chunks 2 and 3
//   bytes [2048, 3072): 16 B per lane, dword c = the low 4 bits of u for chunk c: weight j = 2p at bits
//                       [4p, 4p + 4), weight j = 2p + 1 at bits [16 + 4p, 16 + 4p + 4)
//   bytes [3072, 3328):  4 B per lane, bit 4 of u: weight (c, 2p) at bit 4c + p, (c, 2p + 1) at bit 16 + 4c + p
// so every wave load reads one contiguous, 128-byte-aligned run.  A pair of weights (2p, 2p + 1) -- one dword of
// the bf16 fragment -- comes out of each plane with one shift, both halves at once.
//
// The fragment-major image (batched decode, B >= 3: kernels_gemv_mfma.hip, the PK forms).  The same record and
// the same four pieces, another gather: a segment is one 16-row group x 128-k block of a [rows][K] matrix, and lane
// l = (n = l & 15, g = l >> 4), chunk c < 4, element j < 8 holds row 16 gr + n at k = 128 kb + 32 c + 8 g + j -- the
// four B fragments k_gemv_mf's issue loads for k block kb.  Segments follow the fragment-major bf16 image: segment
// gr * (K / 128) + kb over the ceil(rows / 16) groups (gate|up as one 2 I x H matrix: the up rows' groups after the
// gate rows').  Rows past the last one are encoded as zeros (exponent field 0, u = 0); their results are never stored.
//
// The two forms differ in the gather alone (PkForm, pk_segs, pk_src below); the record, its four pieces and their
// offsets in a segment are common.
#include "common.h"

namespace pgmi {

#define PK_HD __host__ __device__ __forceinline__

constexpr int kPkSegK = 2048;      // weights per segment
constexpr int kPkSegBytes = 3328;  // 13 bits each
constexpr unsigned kPkExpMask = 0x7F807F80u;  // the exponent fields of a bf16 pair

struct PkSeg {
    uint4 a, b, n;
    unsigned h;
};

typedef unsigned short pk_u16x2 __attribute__((ext_vector_type(2)));

// the per-tensor kernel argument: (e_hi - 31) mod 2^16 in both halves
PK_HD unsigned pk_base2(int e_hi) {
    const unsigned b = (unsigned)(e_hi - 31) & 0xFFFFu;
    return b | (b << 16);
}

PK_HD bool pk_fits(int e_hi, int e_lo_nonzero) {  // e_lo_nonzero: smallest exponent field >= 1 (none: > 255)
    return e_lo_nonzero > 255 || e_lo_nonzero >= e_hi - 30;
}

PK_HD unsigned pk_shl(unsigned v, int s) { return s >= 0 ? v << (s & 31) : v >> ((-s) & 31); }

PK_HD unsigned pk_word(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// bytes (b_lo, b_lo, b_hi, b_hi) of S, b_lo = byte 2 * odd, b_hi = the next: sign and mantissa of a pair,
// each where bf16 has them (bits 15 and 6..0 of its half); the rest is overwritten by the exponent
PK_HD unsigned pk_spread(unsigned S, int odd) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(S, S, odd ? 0x03030202u : 0x01010000u);
#else
    const unsigned lo = (S >> (odd ? 16 : 0)) & 0xFFu, hi = (S >> (odd ? 24 : 8)) & 0xFFu;
    return lo | (lo << 8) | (hi << 16) | (hi << 24);
#endif
}

// dword p (weights 2p, 2p + 1) of the lane's bf16 fragment of chunk c (compile-time c and p after unrolling)
PK_HD unsigned pk_pair(const PkSeg& s, int c, int p, unsigned base2) {
    const unsigned G = pk_spread(pk_word(c < 2 ? s.a : s.b, (c & 1) * 2 + (p >> 1)), p & 1);
    const unsigned n = pk_shl(pk_word(s.n, c), 7 - 4 * p) & 0x07800780u;
    const unsigned u7 = (pk_shl(s.h, 11 - 4 * c - p) & 0x08000800u) | n;  // u << 7 in each half
    // exponent field << 7 = u ? (u + e_hi - 31) << 7 : 0
    const pk_u16x2 u = __builtin_bit_cast(pk_u16x2, u7);
    const pk_u16x2 one = __builtin_elementwise_min(u, (pk_u16x2)(0x80));
    const pk_u16x2 e = one * __builtin_bit_cast(pk_u16x2, base2) + u;
    return (__builtin_bit_cast(unsigned, e) & kPkExpMask) | (G & ~kPkExpMask);
}

PK_HD uint4 pk_chunk(const PkSeg& s, int c, unsigned base2) {
    return make_uint4(pk_pair(s, c, 0, base2), pk_pair(s, c, 1, base2), pk_pair(s, c, 2, base2),
                      pk_pair(s, c, 3, base2));
}

// the segment record of one lane from its four bf16 fragments (the inverse of pk_chunk for a tensor that fits)
PK_HD PkSeg pk_encode(const uint4 (&f)[4], int e_hi) {
    unsigned sm[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nib[4] = {0, 0, 0, 0}, h = 0;
    for (int c = 0; c < 4; ++c)
        for (int j = 0; j < 8; ++j) {
            const unsigned w = (pk_word(f[c], j >> 1) >> (16 * (j & 1))) & 0xFFFFu;
            const unsigned ex = (w >> 7) & 0xFFu;
            const unsigned u = ex ? (unsigned)((int)ex - (e_hi - 31)) & 31u : 0u;
            sm[c * 2 + (j >> 2)] |= (((w >> 8) & 0x80u) | (w & 0x7Fu)) << (8 * (j & 3));
            const int p = j >> 1, odd = j & 1;
            nib[c] |= (u & 15u) << (16 * odd + 4 * p);
            h |= (u >> 4) << (16 * odd + 4 * c + p);
        }
    PkSeg s;
    s.a = make_uint4(sm[0], sm[1], sm[2], sm[3]);
    s.b = make_uint4(sm[4], sm[5], sm[6], sm[7]);
    s.n = make_uint4(nib[0], nib[1], nib[2], nib[3]);
    s.h = h;
    return s;
}

// byte offsets of lane l's four loads inside a segment
PK_HD int pk_off_a(int l) { return 16 * l; }
PK_HD int pk_off_b(int l) { return 1024 + 16 * l; }
PK_HD int pk_off_n(int l) { return 2048 + 16 * l; }
PK_HD int pk_off_h(int l) { return 3072 + 4 * l; }

// ---- the fragment-major gather (16-row group x 128-k block per segment)
constexpr int kPkMfRows = 16, kPkMfK = 128;

PK_HD int64_t pk_mf_groups(int64_t rows) { return (rows + kPkMfRows - 1) / kPkMfRows; }
PK_HD int64_t pk_mf_seg(int64_t gr, int64_t kb, int64_t K) { return gr * (K / kPkMfK) + kb; }
// the weight at (lane l, chunk c, element 0) of segment (gr, kb): its row (may be past the last: a zero) and k
PK_HD int64_t pk_mf_row(int64_t gr, int l) { return kPkMfRows * gr + (l & 15); }
PK_HD int64_t pk_mf_k(int64_t kb, int l, int c) { return kPkMfK * kb + 32 * c + 8 * (l >> 4); }

// ---- the two gathers, stated once: what differs between the forms is which weights a segment holds.  Everything
// that builds or reads back an image (the pack kernel, the host encode / decode below) goes through these three.
enum PkForm { PK_FORM_ROWS = 0, PK_FORM_FRAG = 1 };  // row-major segments (B <= 2), fragment-major ones (B >= 3)

// the segments of the image of a [rows][K] matrix, and its bytes
PK_HD int64_t pk_segs(PkForm f, int64_t rows, int64_t K) {
    return f == PK_FORM_FRAG ? pk_mf_groups(rows) * (K / kPkMfK) : rows * (K / kPkSegK);
}
PK_HD int64_t pk_image_bytes(PkForm f, int64_t rows, int64_t K) { return pk_segs(f, rows, K) * kPkSegBytes; }

// the element offset in W[rows][K] of the 8 weights at (segment seg, lane l, chunk c); >= rows * K: a pad row of
// the fragment-major form's last group (encoded as zeros; a decode writes it, into a matrix of whole groups)
PK_HD int64_t pk_src(PkForm f, int64_t seg, int l, int c, int64_t K) {
    if (f == PK_FORM_ROWS) return seg * kPkSegK + 512 * c + 8 * l;
    const int64_t kbs = K / kPkMfK;
    return pk_mf_row(seg / kbs, l) * K + pk_mf_k(seg % kbs, l, c);
}

// lane l's record <-> its four pieces in the segment at seg (no alignment assumed: the host's images are a caller's)
PK_HD void pk_put(uint8_t* seg, int l, const PkSeg& s) {
    __builtin_memcpy(seg + pk_off_a(l), &s.a, 16);
    __builtin_memcpy(seg + pk_off_b(l), &s.b, 16);
    __builtin_memcpy(seg + pk_off_n(l), &s.n, 16);
    __builtin_memcpy(seg + pk_off_h(l), &s.h, 4);
}
PK_HD PkSeg pk_get(const uint8_t* seg, int l) {
    PkSeg s;
    __builtin_memcpy(&s.a, seg + pk_off_a(l), 16);
    __builtin_memcpy(&s.b, seg + pk_off_b(l), 16);
    __builtin_memcpy(&s.n, seg + pk_off_n(l), 16);
    __builtin_memcpy(&s.h, seg + pk_off_h(l), 4);
    return s;
}

// The format on the host (tests, no device): the image of w[rows][K] and its decode, through the very functions the
// kernels use.  The fragment-major decode writes pk_mf_groups(rows) * 16 rows (the pad rows decode to +0).
template <PkForm F>
inline void pk_encode_host(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image) {
    for (int64_t seg = 0; seg < pk_segs(F, rows, K); ++seg)
        for (int l = 0; l < 64; ++l) {
            uint4 f[4];
            for (int c = 0; c < 4; ++c) {
                const int64_t off = pk_src(F, seg, l, c, K);
                f[c] = make_uint4(0, 0, 0, 0);
                if (off < rows * K) __builtin_memcpy(&f[c], w + off, 16);
            }
            pk_put(image + seg * kPkSegBytes, l, pk_encode(f, e_hi));
        }
}

template <PkForm F>
inline void pk_decode_host(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w) {
    const unsigned b2 = pk_base2(e_hi);
    for (int64_t seg = 0; seg < pk_segs(F, rows, K); ++seg)
        for (int l = 0; l < 64; ++l) {
            const PkSeg s = pk_get(image + seg * kPkSegBytes, l);
            for (int c = 0; c < 4; ++c) {
                const uint4 f = pk_chunk(s, c, b2);
                __builtin_memcpy(w + pk_src(F, seg, l, c, K), &f, 16);
            }
        }
}

}  // namespace pgmi
