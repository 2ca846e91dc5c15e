"""16 images per GPU at the full PaliGemma-3B / 224 px shapes, run as ONE batch (16-row prefill, lock-step
KV-cached decode with the batch filling the 16-row MFMA tile of kernels_gemv_mfma.hip).  No new fixture:
rows 0-7 are the eight images of tests/golden/full_batch8_bf16.npz, rows 8-15 the same images in the order
3, 4, 5, 6, 7, 0, 1, 2 (every image once in each half of the tile, no row beside its own copy), and each row
is held to the rules of tests/test_gpu_full_batch.py against ITS image's reference run (fp32 truth:
full_batch8_fp32.npz), teacher-forced over the fixture's full 256 steps; then free-running generate.

Per step only the columns the rules read are kept (the reference's top-8, the sampled vocabulary, the
argmax): 16 x 257,216 logits for 256 steps would be about 4 GB.
"""
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests_helpers import check_model_parity, pixels_from_u8

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
SEED = 1234
KV_CAP = 576
IMG = list(range(8)) + [3, 4, 5, 6, 7, 0, 1, 2]   # row -> fixture image
B = len(IMG)


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "full_batch8_bf16.npz"))


@pytest.fixture(scope="module")
def F(golden_dir):
    return np.load(os.path.join(golden_dir, "full_batch8_fp32.npz"))


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.full_config(224), max_batch=B, max_seq=288, max_kv=KV_CAP)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    yield e
    del e
    torch.cuda.empty_cache()


def _inputs(G):
    px = torch.from_numpy(np.stack([pixels_from_u8(G["u8"][i]) for i in IMG])).cuda()
    ids = torch.from_numpy(G["ids"][IMG]).cuda()
    return ids, px


@torch.no_grad()
def test_16_rows_teacher_forced_vs_own_reference(eng, G, F):
    ids, px = _inputs(G)
    L = ids.shape[1]
    kv = eng.new_kv(B, KV_CAP)
    ref_toks = G["tokens"][IMG]
    n_steps = ref_toks.shape[1]
    feats = eng.project(eng.vision(px))
    lg = eng.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=1)[:, 0].clone()
    sidx = torch.from_numpy(G["sample_idx"]).cuda()
    topk = torch.from_numpy(G["topk_idx"][IMG]).cuda()            # (B, n_steps, 8)
    tops, samples, argmaxes = [], [], []

    def keep(t, x):
        tops.append(torch.gather(x, 1, topk[:, t]))
        samples.append(x[:, sidx])
        argmaxes.append(x.argmax(-1))

    keep(0, lg)
    logits = torch.empty_like(lg)
    for t in range(1, n_steps):
        cur = torch.from_numpy(ref_toks[:, t - 1].copy()).cuda()
        eng.decode(cur, kv, L + t - 1, L + t, logits=logits, graph=True)
        keep(t, logits)
    top = torch.stack(tops, 1).cpu().numpy()                      # (B, n_steps, 8)
    s = torch.stack(samples, 1).cpu().numpy()                     # (B, n_steps, sampled vocabulary)
    am = torch.stack(argmaxes, 1).cpu().numpy()                   # (B, n_steps)
    for b, i in enumerate(IMG):
        assert np.abs(top[b] - G["topk_val"][i]).max() <= 0.25, (b, i, np.abs(top[b] - G["topk_val"][i]).max())
        decisive = G["margin"][i] > 0.25
        assert np.array_equal(am[b][decisive], ref_toks[b][decisive]), (b, i, am[b], ref_toks[b])
        check_model_parity(f"batch16/row{b}_image{i}", s[b], G["sample_vals"][i], F["sample_vals"][i])


@torch.no_grad()
def test_16_rows_free_running_vs_own_reference(eng, G):
    ids, px = _inputs(G)
    toks = eng.generate(ids, px, G["tokens"].shape[1], graph=True).cpu().numpy()
    for b, i in enumerate(IMG):
        ref = G["tokens"][i]
        diff = np.nonzero(toks[b] != ref)[0]
        if len(diff):
            assert G["margin"][i, diff[0]] < 0.25, (b, i, diff[0], toks[b][:diff[0] + 2], ref[:diff[0] + 2])
