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
