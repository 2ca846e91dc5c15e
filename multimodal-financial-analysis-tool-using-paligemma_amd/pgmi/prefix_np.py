"""The prefix-LM rule of pgmi_lm_forward_prefix in numpy (no GPU): which keys a token attends, and its position.

A row of L new tokens behind kv_start cached ones has lens[b] real tokens, the first prefix_lens[b] of them its
prefix (the prompt).  Token j attends keys [0, min(kv_start + lens[b], kv_start + max(prefix_lens[b], j + 1))): the
cached rows and the prefix from everywhere -- the reference's zero prefill mask (modeling_gemma.py:506-511) -- and
the tokens after the prefix causally, as the decode loop would have seen them one at a time.
"""
from __future__ import annotations

import numpy as np


def _rows(x, B: int, name: str) -> np.ndarray:
    a = np.asarray(x, dtype=np.int64).reshape(-1)
    if a.shape[0] != B:
        raise ValueError(f"{name} has {a.shape[0]} entries for a batch of {B}")
    return a


def prefix_limits(L: int, kv_start: int, lens, prefix_lens) -> np.ndarray:
    """(B, L) int64: the number of keys token j of row b attends.  lens None: L for every row."""
    p = np.asarray(prefix_lens, dtype=np.int64).reshape(-1)
    B = p.shape[0]
    ln = np.full(B, L, dtype=np.int64) if lens is None else _rows(lens, B, "lens")
    if L < 1 or kv_start < 0 or (ln < 1).any() or (ln > L).any():
        raise ValueError("need L >= 1, kv_start >= 0 and 1 <= lens[b] <= L")
    if (p < 0).any() or (p > ln).any():
        raise ValueError("prefix_lens[b] must be in [0, lens[b]]")
    j = np.arange(L, dtype=np.int64)[None, :]
    return np.minimum(kv_start + ln[:, None], kv_start + np.maximum(p[:, None], j + 1))


def prefix_mask(L: int, kv_start: int, lens, prefix_lens) -> np.ndarray:
    """The additive mask (B, 1, L, kv_start + L) fp32: 0 where token j attends key k, -inf elsewhere."""
    lim = prefix_limits(L, kv_start, lens, prefix_lens)
    k = np.arange(kv_start + L, dtype=np.int64)[None, None, :]
    return np.where(k < lim[:, :, None], np.float32(0), np.float32(-np.inf)).astype(np.float32)[:, None]


def prefix_positions(L: int, prefix_lens, gap: bool = True) -> np.ndarray:
    """(B, L) int64 rotary positions: j for the prefix; j + 1 after it (gap) -- the reference's first decode
    position after a P-token prefill is P + 1 (attention_mask.cumsum(-1)[:, -1] of modeling_gemma.py:526), so a
    one-pass row continues as the decode loop would -- or j throughout (gap False)."""
    p = np.asarray(prefix_lens, dtype=np.int64).reshape(-1)
    j = np.broadcast_to(np.arange(L, dtype=np.int64)[None, :], (p.shape[0], L))
    return j + ((j >= p[:, None]) & bool(gap))
