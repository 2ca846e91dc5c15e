"""Token log-probabilities and the shifted loss, the parts that need no GPU: the float64 numpy rule
(pgmi/scoring.py) against torch's cross_entropy / log_softmax on the CPU, the three C entries' argument checks
on a context that owns no device memory, and the Python switches' defaults."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _rows(seed, rows, V, scale=3.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, V)) * scale).astype(np.float32)


@pytest.mark.parametrize("rows,V,ignore", [(1, 7, -100), (13, 1000, -100), (64, 257, 5)])
def test_logprobs_np_matches_torch(rows, V, ignore):
    from pgmi.scoring import logprobs_np, logsumexp_np, loss_from_logprobs_np
    x = _rows(rows * 31 + V, rows, V)
    rng = np.random.default_rng(V)
    lb = rng.integers(0, V, rows)
    lb[::3] = ignore
    if ignore >= 0:
        lb[1] = (ignore + 1) % V   # a live row beside the ignored ones when ignore_index is itself a column
    xt, lt = torch.from_numpy(x).double(), torch.from_numpy(lb)
    ls = F.log_softmax(xt, -1)
    live = lb != ignore
    want = np.where(live, ls.gather(1, torch.from_numpy(np.where(live, lb, 0))[:, None])[:, 0].numpy(), 0.0)
    got = logprobs_np(x, lb, ignore)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(logsumexp_np(x), torch.logsumexp(xt, -1).numpy(), rtol=0, atol=1e-12)
    if live.any():
        ce = F.cross_entropy(xt, lt, ignore_index=ignore).item()
        assert abs(loss_from_logprobs_np(got, lb, ignore) - ce) <= 1e-12 * max(1.0, abs(ce))


def test_shifted_loss_np_matches_torch():
    from pgmi.scoring import shifted_loss_np
    B, L, V = 3, 9, 50
    x = _rows(3, B * L, V).reshape(B, L, V)
    lb = np.random.default_rng(4).integers(0, V, (B, L))
    lb[:, :4] = -100          # the prompt is masked, as in fine-tuning data
    lb[1, 6] = -100
    xt, lt = torch.from_numpy(x).double(), torch.from_numpy(lb)
    ce = F.cross_entropy(xt[:, :-1].reshape(-1, V), lt[:, 1:].reshape(-1), ignore_index=-100).item()
    assert abs(shifted_loss_np(x, lb) - ce) <= 1e-12 * max(1.0, abs(ce))
    # labels[:, 0] is never scored
    lb2 = lb.copy()
    lb2[:, 0] = 7
    assert shifted_loss_np(x, lb2) == shifted_loss_np(x, lb)


def test_all_ignored_and_out_of_range():
    from pgmi.scoring import logprobs_np, loss_from_logprobs_np, shifted_loss_np
    x = _rows(9, 4, 11)
    ign = np.full(4, -100)
    assert (logprobs_np(x, ign) == 0).all()
    assert np.isnan(loss_from_logprobs_np(logprobs_np(x, ign), ign))
    assert np.isnan(shifted_loss_np(x.reshape(1, 4, 11), np.full((1, 4), -100)))
    assert np.isnan(F.cross_entropy(torch.from_numpy(x), torch.from_numpy(ign)).item())   # as torch gives
    lb = np.array([0, 11, -1, -100])    # V, and a negative that is not ignore_index: NaN; nothing is read
    got = logprobs_np(x, lb)
    assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isnan(got[2]) and got[3] == 0
    assert np.isnan(loss_from_logprobs_np(got, lb))
    # -inf entries and a constant row
    y = np.zeros((2, 8), np.float32)
    y[0, 3:] = -np.inf
    np.testing.assert_allclose(logprobs_np(y, np.array([0, 5])), [-np.log(3.0), -np.log(8.0)], atol=1e-15)
    assert logprobs_np(y, np.array([4, 0]))[0] == -np.inf


def _bare_ctx(N):
    """A context that owns no device memory (pgmi_create builds only the weight layout)."""
    from pgmi.engine import config_dict
    from oracle import weights as W
    cd = config_dict(W.small_config())
    c = N.PgmiConfig()
    for k, _ in N.PgmiConfig._fields_:
        if k not in ("max_batch", "max_seq", "max_kv"):
            setattr(c, k, cd[k])
    c.max_batch, c.max_seq, c.max_kv = 1, 64, 128
    h = ctypes.c_void_p()
    assert N.lib().pgmi_create(0, ctypes.byref(c), ctypes.byref(h)) == 0
    return h


def test_c_entries_refuse_bad_arguments_without_a_device():
    from pgmi import _native as N
    lib = N.lib()
    for name in ("pgmi_lm_logprobs", "pgmi_op_lm_logprobs", "pgmi_logprobs"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    h = _bare_ctx(N)
    try:
        p = 4096   # never dereferenced: every call below is refused before any launch
        # null pointers (lse alone may be NULL)
        assert lib.pgmi_lm_logprobs(None, p, 1, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_lm_logprobs(h, None, 1, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_lm_logprobs(h, p, 1, None, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_lm_logprobs(h, p, 1, p, -100, None, None, None) == N.PGMI_E_ARG
        assert b"null" in lib.pgmi_last_error()
        assert lib.pgmi_op_lm_logprobs(h, p, None, 1, 64, 64, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_op_lm_logprobs(None, p, p, 1, 64, 64, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_logprobs(h, None, 1, 8, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_logprobs(h, p, 1, 8, None, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_logprobs(h, p, 1, 8, p, -100, None, None, None) == N.PGMI_E_ARG
        # empty
        assert lib.pgmi_lm_logprobs(h, p, 0, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_op_lm_logprobs(h, p, p, 0, 64, 64, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_logprobs(h, p, 0, 8, p, -100, p, None, None) == N.PGMI_E_ARG
        assert lib.pgmi_logprobs(h, p, 1, 0, p, -100, p, None, None) == N.PGMI_E_ARG
        # well-formed calls on a context that was never prepared
        assert lib.pgmi_lm_logprobs(h, p, 1, p, -100, p, None, None) == N.PGMI_E_STATE
        assert lib.pgmi_op_lm_logprobs(h, p, p, 1, 64, 64, p, -100, p, None, None) == N.PGMI_E_STATE
        assert lib.pgmi_logprobs(h, p, 1, 8, p, -100, p, None, None) == N.PGMI_E_STATE
    finally:
        lib.pgmi_destroy(h)


def test_reference_loss_fixture_is_consistent(golden_dir):
    """tests/golden/small_loss.npz: the reference's loss is the float64 rule applied to its own per-token
    log-probabilities (its CrossEntropyLoss ran in fp32: 1e-6 relative)."""
    import os
    from pgmi.scoring import loss_from_logprobs_np
    g = np.load(os.path.join(golden_dir, "small_loss.npz"))
    sl = g["labels"][:, 1:]
    assert g["ids"].shape == g["labels"].shape and (sl != -100).sum() == 30
    for tag in ("bf16", "fp32"):
        lp = g["logprobs_" + tag]
        assert lp.shape == sl.shape and np.all(lp[sl == -100] == 0) and np.all(lp[sl != -100] < 0)
        want = loss_from_logprobs_np(lp, sl)
        assert abs(float(g["loss_" + tag]) - want) <= 1e-6 * want


def test_switches_default_off():
    import modeling_gemma as MG
    from pgmi import Engine
    from pgmi.lazy_logits import LazyLogits
    sig = inspect.signature(Engine.generate)
    assert sig.parameters["return_logprobs"].default is False
    assert MG.PaliGemmaForConditionalGeneration.pgmi_fused_loss is False
    s = inspect.signature(Engine.score)
    assert s.parameters["ignore_index"].default == -100 and s.parameters["attention_mask"].default is None
    assert inspect.signature(Engine.lm_logprobs).parameters["return_lse"].default is False
    assert inspect.signature(Engine.logprobs).parameters["ignore_index"].default == -100
    assert inspect.signature(LazyLogits.__init__).parameters["shifted_logprobs"].default is None
