"""Token log-probabilities and the shifted loss in float64 numpy (no torch): the rule the native paths are held to.

The reference's PaliGemmaForConditionalGeneration.forward(labels=...) (modeling_gemma.py:596-603) shifts --
position j predicts labels[:, j + 1] -- and takes CrossEntropyLoss(ignore_index) over the flattened rows: the
mean of -log_softmax(logits)[label] over the rows whose label is not ignore_index (NaN when none is left).
"""
from __future__ import annotations

import numpy as np


def logsumexp_np(logits) -> np.ndarray:
    """logsumexp over the last axis in float64; a row of -inf gives -inf."""
    x = np.asarray(logits, dtype=np.float64)
    m = np.max(x, axis=-1, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (ms + np.log(np.sum(np.exp(x - ms), axis=-1, keepdims=True)))[..., 0]


def logprobs_np(logits, labels, ignore_index: int = -100) -> np.ndarray:
    """log_softmax(logits)[..., label] per row, float64: logits (..., V), labels (...) integers.
    A row whose label is ignore_index gives 0; any other label outside [0, V) gives NaN."""
    x = np.asarray(logits, dtype=np.float64)
    lb = np.asarray(labels).astype(np.int64)
    if lb.shape != x.shape[:-1]:
        raise ValueError(f"labels {lb.shape} do not match logits {x.shape}")
    V = x.shape[-1]
    ok = (lb >= 0) & (lb < V)
    picked = np.take_along_axis(x, np.where(ok, lb, 0)[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        lp = picked - logsumexp_np(x)
    lp = np.where(ok, lp, np.nan)
    return np.where(lb == ignore_index, 0.0, lp)


def loss_from_logprobs_np(logprobs, labels, ignore_index: int = -100) -> float:
    """-mean(logprob over the rows whose label is not ignore_index); NaN when no row is left."""
    lp = np.asarray(logprobs, dtype=np.float64).reshape(-1)
    live = np.asarray(labels).reshape(-1) != ignore_index
    if not live.any():
        return float("nan")
    return float(-np.sum(lp[live]) / np.count_nonzero(live))


def shifted_loss_np(logits, labels, ignore_index: int = -100) -> float:
    """The reference's loss: logits (B, L, V), labels (B, L); position j is scored against labels[:, j + 1]."""
    x = np.asarray(logits)
    lb = np.asarray(labels)
    sl = lb[..., 1:]
    return loss_from_logprobs_np(logprobs_np(x[..., :-1, :], sl, ignore_index), sl, ignore_index)
