"""The lossless 13-bit weight format of the batch 1-2 decode step, stated in numpy (csrc/pack13.h is the
device form; DESIGN.md sec.2 the byte layout).

A bf16 weight is sign(1) | exponent field(8) | mantissa(7).  With e_hi the largest exponent field of a tensor,
a weight is kept as the byte sign << 7 | mantissa and a 5-bit code: c = e_hi - exponent in 0..30, or c = 31 for
exponent field 0 (zeros of either sign and denormals, whose sign and mantissa stay in the byte).  A tensor fits
when no element has an exponent field in [1, e_hi - 31]."""
from __future__ import annotations

import numpy as np

KINDS = {"gate_up": 1, "down": 2, "lm_head": 4}
ALL_KINDS = 7
SEG_WEIGHTS, SEG_BYTES = 2048, 3328


def exponent_fields(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.int32) >> 7) & 0xFF


def e_hi_np(bits: np.ndarray) -> int:
    return int(exponent_fields(bits).max())


def fits_np(bits: np.ndarray) -> bool:
    e = exponent_fields(bits)
    hi = int(e.max())
    return not bool(((e >= 1) & (e <= hi - 31)).any())


def pack_np(bits: np.ndarray, e_hi: int):
    """(sign/mantissa bytes, 5-bit codes) of bf16 bit patterns that fit under e_hi."""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    e = (b >> 7) & 0xFF
    code = np.where(e == 0, 31, e_hi - e)
    if ((code < 0) | (code > 31) | ((e != 0) & (code == 31))).any():
        raise ValueError("tensor does not fit the 5-bit exponent code")
    sm = ((b >> 8) & 0x80) | (b & 0x7F)
    return sm.astype(np.uint8), code.astype(np.uint8)


def unpack_np(sm: np.ndarray, code: np.ndarray, e_hi: int) -> np.ndarray:
    s, c = sm.astype(np.int32), code.astype(np.int32)
    e = np.where(c == 31, 0, e_hi - c)
    return (((s & 0x80) << 8) | (e << 7) | (s & 0x7F)).astype(np.uint16)


def image_bytes(rows: int, K: int) -> int:
    return rows * (K // SEG_WEIGHTS) * SEG_BYTES


# ---- the fragment-major gather of the batched (3..16 rows) decode step: the same 52-byte lane record, a segment
# being one 16-row group x 128-k block -- the four B fragments k_gemv_mf loads per lane and k block.
MF_ROWS, MF_K = 16, 128


def mf_groups(rows: int) -> int:
    return (rows + MF_ROWS - 1) // MF_ROWS


def image_bytes_mf(rows: int, K: int) -> int:
    return mf_groups(rows) * (K // MF_K) * SEG_BYTES


def frag_index_np(rows: int, K: int):
    """(row, k) of every weight of the fragment-major image, each of shape [groups][K / 128][64 lanes][4 chunks][8]:
    lane l = (n = l & 15, g = l >> 4), chunk c, element j hold row 16 gr + n (>= rows: a pad row, encoded as zero)
    at k = 128 kb + 32 c + 8 g + j.  Segment gr * (K / 128) + kb."""
    gr, kb, l, c, j = np.meshgrid(np.arange(mf_groups(rows)), np.arange(K // MF_K), np.arange(64), np.arange(4),
                                  np.arange(8), indexing="ij")
    return MF_ROWS * gr + (l & 15), MF_K * kb + 32 * c + 8 * (l >> 4) + j


def seg_image_np(bits: np.ndarray, e_hi: int) -> np.ndarray:
    """The bytes of segments given the bf16 patterns of their weights, bits[..., 64 lanes, 4 chunks, 8] ->
    uint8[..., 3328] (the byte layout of csrc/pack13.h, stated independently of it)."""
    sm, code = pack_np(bits, e_hi)
    u = (31 - code.astype(np.int64)).astype(np.uint32)     # the planes hold u = 31 - c
    lead = bits.shape[:-3]
    img = np.zeros(lead + (SEG_BYTES,), np.uint8)
    # bytes [0, 2048): 16 B per lane, sm of chunks 0|1, then of chunks 2|3
    img[..., 0:1024] = sm[..., :, 0:2, :].reshape(lead + (1024,))
    img[..., 1024:2048] = sm[..., :, 2:4, :].reshape(lead + (1024,))
    # bytes [2048, 3072): dword c of a lane: low 4 bits of u, weight j = 2p at bit 4p, j = 2p + 1 at bit 16 + 4p
    j = np.arange(8)
    sh_n = (16 * (j & 1) + 4 * (j >> 1)).astype(np.uint32)
    nib = np.bitwise_or.reduce((u & 15) << sh_n, axis=-1).astype("<u4")            # [..., 64, 4]
    img[..., 2048:3072] = nib.view(np.uint8).reshape(lead + (1024,))
    # bytes [3072, 3328): one dword per lane: bit 4 of u, weight (c, 2p) at bit 4c + p, (c, 2p + 1) at bit 16 + 4c + p
    c = np.arange(4)[:, None]
    sh_h = (16 * (j & 1)[None, :] + 4 * c + (j >> 1)[None, :]).astype(np.uint32)
    hi = np.bitwise_or.reduce(np.bitwise_or.reduce((u >> 4) << sh_h, axis=-1), axis=-1).astype("<u4")   # [..., 64]
    img[..., 3072:3328] = hi.view(np.uint8).reshape(lead + (256,))
    return img


def encode_mf_np(bits: np.ndarray, e_hi: int) -> np.ndarray:
    """The fragment-major image of a [rows][K] matrix of bf16 patterns (K a multiple of 128), as flat bytes."""
    w = np.asarray(bits, np.uint16)
    rows, K = w.shape
    padded = np.zeros((mf_groups(rows) * MF_ROWS, K), np.uint16)
    padded[:rows] = w
    r, k = frag_index_np(rows, K)
    return seg_image_np(padded[r, k], e_hi).reshape(-1)
