"""The logit-processor rule of csrc/logits_rule.h in numpy -- the second statement of the
rule, held bit for bit equal to pgmi_logits_process_host by tests/test_cpu_logits.py.

For one row x[V] (fp32) and its history word h[v] (uint32): in_prompt = h >> 31, n_out = h & 0x7fffffff,
seen = in_prompt | (n_out > 0).  Stage 1, per element, in this order, each step skipped when its parameter is
neutral (so neutral parameters return x's bits, -0 included):
  1. rp != 1 and seen:    x = x * rp if x < 0 else x / rp      (one fp32 operation)
  2. fp != 0:             x = x - fp32(fp * fp32(n_out))       (two rounded operations)
     pp != 0, n_out > 0:  x = x - pp
  3. bias given:          x = x + bias[v]
  4. suppress on and emitted[row] < min_new_tokens:  x[suppress_id] = -inf
Stage 2 on the stage-1 row y, m = max(y): thr = max(kth, fp32(m + delta)), kth the k-th largest value (1 <= k < V,
else off) and delta = fp32(T ln(min_p)) (-inf: off); y < thr -> -inf.  Guard: m == -inf returns the raw x."""
from __future__ import annotations

import math

import numpy as np

NEG_INF = np.float32(-np.inf)


def min_p_delta(min_p: float, temperature: float = 1.0) -> np.float32:
    """delta = fp32(T * ln(min_p)), computed in float64 and rounded once; -inf when min-p is off."""
    if not min_p > 0.0:
        return NEG_INF
    return np.float32(float(temperature) * math.log(float(min_p)))


def history_np(V: int, prompts, outputs) -> np.ndarray:
    """The history array as bincounts: prompts / outputs are one sequence of ids per row."""
    h = np.zeros((len(prompts), V), dtype=np.uint32)
    for r, (p, o) in enumerate(zip(prompts, outputs)):
        p = np.asarray(p, dtype=np.int64).reshape(-1)
        o = np.asarray(o, dtype=np.int64).reshape(-1)
        h[r] = np.bincount(o, minlength=V).astype(np.uint32)
        h[r, np.unique(p)] |= np.uint32(0x80000000)
    return h


def stage1(x, h=None, rp=1.0, pp=0.0, fp=0.0, bias=None, suppress_id=-1, min_new_tokens=0, emitted=None):
    x = np.asarray(x, dtype=np.float32)
    y = x.copy()
    rp, pp, fp = np.float32(rp), np.float32(pp), np.float32(fp)
    with np.errstate(all="ignore"):
        if h is not None:
            h = np.asarray(h, dtype=np.uint32)
            n_out = h & np.uint32(0x7FFFFFFF)
            if rp != 1:
                y = np.where(h != 0, np.where(y < 0, y * rp, y / rp), y).astype(np.float32)
            if fp != 0:
                y = (y - (fp * n_out.astype(np.float32)).astype(np.float32)).astype(np.float32)
            if pp != 0:
                y = np.where(n_out != 0, y - pp, y).astype(np.float32)
        if bias is not None:
            y = (y + np.asarray(bias, dtype=np.float32)[None, :]).astype(np.float32)
    if suppress_id is not None and suppress_id >= 0 and min_new_tokens > 0:
        e = np.asarray(emitted).reshape(-1)
        y[e < min_new_tokens, suppress_id] = NEG_INF
    return y


def process(x, h=None, rp=1.0, pp=0.0, fp=0.0, bias=None, top_k=0, delta=NEG_INF, suppress_id=-1, min_new_tokens=0,
            emitted=None):
    """x (rows, V) fp32 -> the processed rows (a new array)."""
    x = np.asarray(x, dtype=np.float32)
    rows, V = x.shape
    y = stage1(x, h, rp, pp, fp, bias, suppress_id, min_new_tokens, emitted)
    delta = np.float32(delta)
    k = int(top_k) if 1 <= int(top_k) < V else 0
    out = np.empty_like(y)
    for r in range(rows):
        m = y[r].max()
        if m == NEG_INF:  # the guard
            out[r] = x[r]
            continue
        thr = NEG_INF
        if k:
            thr = np.partition(y[r], V - k)[V - k]  # the k-th largest value
        if delta != NEG_INF:
            with np.errstate(all="ignore"):
                t = np.float32(m + delta)
            if t > thr:
                thr = t
        out[r] = np.where(y[r] < thr, NEG_INF, y[r])
    return out
