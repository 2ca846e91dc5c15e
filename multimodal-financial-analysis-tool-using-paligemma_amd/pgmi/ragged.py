"""Ragged batches: per-row prompt lengths from a processor's attention mask (pure torch, no GPU).

PaliGemmaProcessor(padding="longest") pads a batch of different prompts to one length and returns an
attention_mask of ones over each row's real tokens; the tokenizer may pad on either side.  The engine's
ragged path (Engine.generate(..., attention_mask=...)) takes right-padded ids plus int32 row lengths.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def _lengths_and_shift(attention_mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    m = torch.as_tensor(attention_mask)
    if m.dim() != 2:
        raise ValueError(f"attention_mask must be (B, L), got shape {tuple(m.shape)}")
    m = m.detach().cpu()
    if m.dtype == torch.bool:
        m = m.to(torch.int64)
    if m.is_floating_point():
        if not bool(((m == 0) | (m == 1)).all()):
            raise ValueError("attention_mask must hold only 0 and 1")
        m = m.to(torch.int64)
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("attention_mask must hold only 0 and 1")
    m = m.to(torch.int64)
    B, L = m.shape
    lens = m.sum(1)
    if L == 0 or bool((lens < 1).any()):
        raise ValueError("attention_mask has an empty row")
    first = m.argmax(1)  # first real token of each row
    idx = torch.arange(L)[None, :]
    run = ((idx >= first[:, None]) & (idx < (first + lens)[:, None])).to(torch.int64)
    if not torch.equal(run, m):
        raise ValueError("attention_mask has a hole: each row's real tokens must be contiguous")
    left = first > 0
    if bool((left & (first + lens != L)).any()):
        raise ValueError("attention_mask rows must be padded on the left or on the right, not both")
    return lens.to(torch.int32), first.to(torch.int64)


def lengths_from_mask(attention_mask: Optional[torch.Tensor]):
    """Row lengths of a padded batch.

    None / an all-ones mask -> None (equal lengths: the lock-step path).
    A right-padded mask     -> int32 lengths (B,).
    A left-padded mask      -> (int32 lengths (B,), int64 shift (B,)): row b's tokens start at shift[b].
    A mask with a hole, an empty row or values other than 0 / 1 raises ValueError."""
    if attention_mask is None:
        return None
    lens, shift = _lengths_and_shift(attention_mask)
    if bool((lens == torch.as_tensor(attention_mask).shape[1]).all()):
        return None
    if bool((shift > 0).any()):
        return lens, shift
    return lens


def right_pad(input_ids: torch.Tensor, attention_mask: torch.Tensor, pad_id: int = 0):
    """Move a padded batch to the right-padded form: returns (ids, lens) with row b's tokens at
    ids[b, :lens[b]] and pad_id after them.  Right-padded input passes through (pads rewritten to pad_id)."""
    ids = torch.as_tensor(input_ids)
    if ids.dim() != 2 or tuple(ids.shape) != tuple(torch.as_tensor(attention_mask).shape):
        raise ValueError("input_ids and attention_mask must have the same (B, L) shape")
    lens, shift = _lengths_and_shift(attention_mask)
    B, L = ids.shape
    idx = torch.arange(L)[None, :]
    src = (idx + shift[:, None]).clamp_(max=L - 1).to(ids.device)
    out = torch.gather(ids, 1, src)
    keep = (idx < lens[:, None].to(torch.int64)).to(ids.device)
    out = torch.where(keep, out, torch.full_like(out, pad_id))
    return out, lens
