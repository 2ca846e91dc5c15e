"""Probe: the B-row decode step, lock-step (pgmi_decode_steps) against the ragged step (pgmi_decode_ragged),
alternating on one engine, n steps per hipGraph launch:
  lock     equal lengths 288, the shared step record
  ragged-a equal lengths 288, per-row records (must equal `lock` within noise, and bit for bit in tokens)
  ragged-b lengths spread over 259-320 (differs from (a) by the attention chunks only: the weights dominate
           the bytes moved and are the same)
Prints ms per step per form and round.

    python tools/probes/ragged_probe.py [--batch 8] [--steps 64] [--rounds 3] [--n 8]
"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "multimodal-financial-analysis-tool-using-paligemma_amd"))
from pgmi import Engine  # noqa: E402
from pgmi.synthetic import init_policy, paligemma_3b_config, prompt_ids  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=8)
    a = ap.parse_args()
    cfg = paligemma_3b_config(224)
    n_img, B, n = 256, a.batch, a.n
    L = n_img + 32
    spread = [259 + (320 - 259) * b // max(1, B - 1) for b in range(B)]
    Lmax = max(L, max(spread))
    cap = (Lmax + a.steps + 8 + 63) // 64 * 64
    eng = Engine(cfg, max_batch=B, max_seq=Lmax, max_kv=cap)
    eng.fill_synthetic(1234, init_policy)
    eng.prepare()
    g = torch.Generator(device="cuda").manual_seed(5)
    px = (torch.rand((B, 3, 224, 224), generator=g, device="cuda") * 2 - 1).contiguous()
    V = cfg["text_config"]["vocab_size"]
    base = torch.from_numpy(prompt_ids(cfg["image_token_index"], n_img, V)).cuda()[0]
    feats = eng.project(eng.vision(px))
    logits = torch.empty((B, V), dtype=torch.float32, device="cuda")

    def prompt(lens):
        width = max(lens)
        ids = torch.zeros((B, width), dtype=torch.int64, device="cuda")
        for b, ln in enumerate(lens):
            ids[b, :min(ln, L)] = base[:min(ln, L)]
            if ln > L:  # longer rows: the text tail repeated
                ids[b, L:ln] = base[n_img + 1:].repeat(2)[:ln - L]
        return ids.contiguous(), width

    forms = {}
    # lock-step
    kv_l = eng.new_kv(B, cap)
    ids, w = prompt([L] * B)
    lg = eng.lm_forward(kv_l, 0, torch.arange(w).expand(B, w), ids=ids, image_feats=feats, logits_rows=2)
    first_l = eng.argmax(lg[:, 0])
    rec_l = torch.empty((a.steps, B), dtype=torch.int64, device="cuda")

    def lock(rec):
        cur = first_l.clone()
        t = 0
        while t < a.steps:
            k = min(n, a.steps - t)
            eng.decode_steps(cur, kv_l, L + t, L + t + 1, k, logits=logits, tokens=rec[t:t + k] if rec is not None else None,
                             graph=True)
            t += k
    forms["lock"] = lock

    def ragged_form(lens):
        kv = eng.new_kv(B, cap)
        ids, w = prompt(lens)
        lg = eng.lm_forward(kv, 0, torch.arange(w).expand(B, w), ids=ids, image_feats=feats, logits_rows=1, lens=lens)
        first = eng.argmax(lg[:, 0])
        ln = torch.tensor(lens, dtype=torch.int32)

        def run(rec):
            cur = first.clone()
            t = 0
            while t < a.steps:
                k = min(n, a.steps - t)
                eng.decode_ragged(cur, kv, ln + t, ln + t + 1, k, logits=logits,
                                  tokens=rec[t:t + k] if rec is not None else None, graph=True)
                t += k
        return run

    forms["ragged-a (288 x B)"] = ragged_form([L] * B)
    forms[f"ragged-b ({spread[0]}..{spread[-1]})"] = ragged_form(spread)
    rec_a = torch.empty((a.steps, B), dtype=torch.int64, device="cuda")
    # capture every form's graphs (first call eager, second captured)
    for name, fn in forms.items():
        for _ in range(3):
            fn(rec_l if name == "lock" else (rec_a if name.startswith("ragged-a") else None))
    torch.cuda.synchronize()
    # (the two prefills differ in attention variant, so the first tokens may; the records are informative)
    print(f"ragged-a token record equal to lock-step: {bool(torch.equal(rec_a, rec_l))}", flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for r in range(a.rounds):
        print(f"round {r}: B={B} ms/step " + ", ".join(f"{k} {timed(fn):.4f}" for k, fn in forms.items()), flush=True)


if __name__ == "__main__":
    main()
