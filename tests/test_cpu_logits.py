"""The logit-processor rule (csrc/logits_rule.h) without a GPU:

1. pgmi_logits_process_host (the C statement, compiled from the header device kernels are to use) equals
   pgmi/logits_np.py (the numpy statement) bit for bit on the input family of tests/logits_cases.py -- the family
   a device implementation is to be held to.
2. The numpy statement equals transformers' RepetitionPenaltyLogitsProcessor (bits), TopKLogitsWarper (kept set)
   and MinPLogitsWarper after a temperature (kept set) where transformers imports.
3. Neutral parameters return the input bits; every refused argument is refused."""
import math

import numpy as np
import pytest

import logits_cases as C
from pgmi import logits_np as LN


def _np_process(c):
    kw = c["kw"]
    return LN.process(c["x"], c["h"], kw["rp"], kw["pp"], kw["fp"], c["bias"], kw["top_k"], kw["delta"],
                      kw["suppress_id"], kw["min_new_tokens"], c["emitted"])


@pytest.mark.parametrize("V", C.VS)
def test_host_rule_equals_numpy_rule(V):
    n = 0
    for rows, k, name, c in C.iter_cases(V):
        want = _np_process(c)
        got = C.host_process(c["x"], c["h"], c["bias"], c["emitted"], **c["kw"])
        assert C.same_bits(got, want), (V, rows, k, name)
        if 1 <= k < V and c["bias"] is None and c["kw"]["delta"] == -np.inf and np.isfinite(c["x"]).all():
            # ties at the k-th value all stay, so at least k survive
            assert int((got > -np.inf).sum(1).min()) >= k, (V, rows, k, name)
        n += 1
    assert n >= 13


def test_guard_returns_the_raw_row():
    V = 2049
    x = C.rows_of(V, 3, 50, 0)
    ban = np.full(V, -np.inf, np.float32)
    h = C.history_words(V, 3, 0)
    for k in (0, 50):
        got = C.host_process(x, h, ban, rp=1.3, fp=0.2, top_k=k)
        assert C.same_bits(got, x)
        assert C.same_bits(LN.process(x, h, 1.3, 0.0, 0.2, ban, k), x)


def test_neutral_parameters_return_the_input_bits():
    V = 4096
    x = C.rows_of(V, 16, 0, 4)  # every family: -0, -inf and ties included
    x[0, :4] = [-0.0, 0.0, -np.inf, np.float32(1e-42)]
    h = C.history_words(V, 16, 4)
    for hist in (None, h):
        for k in (0, V, V + 5):
            assert C.same_bits(C.host_process(x, hist, top_k=k), x)
            assert C.same_bits(LN.process(x, hist, top_k=k), x)
    # a suppress that no row is subject to any more
    e = np.full(16, 3, np.int32)
    assert C.same_bits(C.host_process(x, None, None, e, suppress_id=7, min_new_tokens=3), x)


def test_host_refuses_bad_arguments():
    from pgmi import _native as N
    x = np.zeros((2, 16), np.float32)
    h = np.zeros((2, 16), np.uint32)
    e = np.zeros(2, np.int32)
    bad = [dict(rp=0.0), dict(rp=-1.0), dict(rp=math.inf), dict(rp=math.nan), dict(pp=math.inf), dict(fp=math.nan),
           dict(top_k=-1), dict(delta=0.5), dict(delta=math.nan)]
    for kw in bad:
        C.host_process(x, h, None, e, expect=N.PGMI_E_ARG, **kw)
    for kw in (dict(rp=1.3), dict(pp=0.1), dict(fp=0.1)):  # a penalty without a history
        C.host_process(x, None, expect=N.PGMI_E_ARG, **kw)
    C.host_process(x, None, None, None, suppress_id=3, min_new_tokens=1, expect=N.PGMI_E_ARG)  # no emitted counts
    C.host_process(x, None, None, e, suppress_id=16, min_new_tokens=1, expect=N.PGMI_E_ARG)    # id outside V
    p = N.PgmiLogitsParams(1.0, 0.0, 0.0, 0, -math.inf, -1, 0)
    import ctypes
    xp = x.ctypes.data_as(ctypes.c_void_p)
    for rows, V in ((0, 16), (2, 0), (-1, 16)):
        assert N.lib().pgmi_logits_process_host(xp, rows, V, None, None, ctypes.byref(p), None, xp) == N.PGMI_E_ARG


def test_min_p_delta_is_rounded_once():
    """delta = fp32(T ln(min_p)) from float64; the C struct's float field rounds the same double the same way."""
    from pgmi import _native as N
    for min_p, T in ((0.05, 0.8), (0.2, 1.0), (0.01, 1.5), (1.0, 0.7)):
        d = T * math.log(min_p)
        assert np.float32(N.PgmiLogitsParams(1.0, 0.0, 0.0, 0, d, -1, 0).min_p_delta) == LN.min_p_delta(min_p, T)
    assert LN.min_p_delta(0.0) == -np.inf


# ---------------------------------------------------------------- against transformers' processors
def _hf():
    pytest.importorskip("transformers")
    import torch
    from transformers import generation as G
    return torch, G


def test_repetition_penalty_is_transformers_bit_for_bit():
    torch, G = _hf()
    V, rows = 4096, 4
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    x[:, :8] = [0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0, 1e-42, -1e-42]
    prompt = [np.concatenate([np.arange(8), rng.integers(0, V, 200)]) for _ in range(rows)]
    h = LN.history_np(V, prompt, [[] for _ in range(rows)])
    for rp in (1.3, 0.7, 1.05):
        want = G.RepetitionPenaltyLogitsProcessor(penalty=rp)(torch.from_numpy(np.stack(prompt)),
                                                              torch.from_numpy(x.copy())).numpy()
        assert C.same_bits(LN.process(x, h, rp=rp), want), rp
        assert C.same_bits(C.host_process(x, h, rp=rp), want), rp


def test_top_k_keeps_transformers_set_ties_included():
    torch, G = _hf()
    V, rows = 2049, 6
    for k in (1, 2, 50, V - 1):
        x = np.stack([C.family_row(f, V, k, np.random.default_rng([k, f])) for f in (0, 1, 2, 4, 6, 6)])
        want = G.TopKLogitsWarper(top_k=k)(None, torch.from_numpy(x.copy())).numpy()
        got = LN.process(x, top_k=k)
        assert np.array_equal(got > -np.inf, want > -np.inf), k
        assert C.same_bits(got, want), k


def test_min_p_keeps_transformers_set():
    torch, G = _hf()
    V, rows = 4096, 8
    left_out = 0
    for seed, (min_p, T) in enumerate(((0.05, 0.8), (0.2, 1.0), (0.01, 1.5))):
        x = (np.random.default_rng(seed).standard_normal((rows, V)) * 3).astype(np.float32)
        xt = G.TemperatureLogitsWarper(T)(None, torch.from_numpy(x.copy()))
        want = G.MinPLogitsWarper(min_p=min_p)(None, xt).numpy() > -np.inf
        got = LN.process(x, delta=LN.min_p_delta(min_p, T)) > -np.inf
        p = np.exp((x.astype(np.float64) - x.max(1, keepdims=True)) / T)
        p /= p.sum(1, keepdims=True)
        edge = min_p * p.max(1, keepdims=True)
        near = (np.abs(p - edge) <= 1e-6 * edge).any(1)  # rows with an entry at the boundary: left out
        left_out += int(near.sum())
        assert np.array_equal(got[~near], want[~near]), (min_p, T)
    assert left_out == 0  # the seeds were chosen so that every row is compared
