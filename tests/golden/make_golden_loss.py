"""Generate tests/golden/small_loss.npz by running the REFERENCE model's forward(labels=...).

Runs where make_golden.py runs (it imports the reference modules through it); the committed .npz is data: the
inputs and the reference's loss and per-token log-probabilities on the 2+2-layer full-width model with the
deterministic synthetic weights, in bf16 and in fp32 (the truth of the 1.5x rule).

    python tests/golden/make_golden_loss.py

The prompt and the pixels are small_bf16.npz's (not stored again); the labels mask the image tokens and <bos>,
as fine-tuning data masks the image and the prompt.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MGOLD  # noqa: E402
from oracle import weights as W  # noqa: E402

IGN = -100


def main():
    cfg = W.small_config()
    gold = np.load(os.path.join(HERE, "small_bf16.npz"))
    ids = gold["ids"].astype(np.int64)
    px = torch.from_numpy(gold["pixels_bits"].view(np.int16)).view(torch.bfloat16)
    L = ids.shape[1]
    n_img = W.num_image_tokens(cfg)
    rng = np.random.default_rng(21)
    labels = np.full((1, L), IGN, dtype=np.int64)
    first = n_img + 1
    labels[0, first:] = rng.integers(0, cfg["text_config"]["vocab_size"], L - first)
    labels[0, first + 3] = IGN     # an ignored label among the live ones
    out = {"ids": ids, "labels": labels}
    for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        model, pcfg = MGOLD.build_model(cfg, dtype)
        assert pcfg.ignore_index == IGN
        with torch.no_grad():
            r = model(input_ids=torch.from_numpy(ids), pixel_values=px.to(dtype),
                      attention_mask=torch.ones((1, L), dtype=torch.int64), labels=torch.from_numpy(labels))
        sl = torch.from_numpy(labels[:, 1:])
        lp = torch.log_softmax(r["logits"][:, :-1].double(), -1).gather(-1, sl.clamp(min=0)[..., None])[..., 0]
        lp = torch.where(sl == IGN, torch.zeros_like(lp), lp)
        out[f"loss_{tag}"] = np.float64(r["loss"].double().item())
        out[f"logprobs_{tag}"] = lp.numpy()
        n = int((sl != IGN).sum())
        print(tag, "loss", out[f"loss_{tag}"], "from the per-token values", float(-lp.sum() / n), "live", n)
        del model
    np.savez_compressed(os.path.join(HERE, "small_loss.npz"), **out)
    print("wrote small_loss.npz", os.path.getsize(os.path.join(HERE, "small_loss.npz")), "bytes")


if __name__ == "__main__":
    main()
