"""Probe: what the prefix-LM prefill costs at the full PaliGemma-3B / 224 px shapes with synthetic weights: a prompt
of 256 image + 32 text tokens and a 32-token answer (L = 320), one engine (max_batch = 8).

  - the language-model prefill alone (Engine.lm_forward, logits_rows 1, a pair of events around it) with
    prefix_lens = 288 against without, at B = 1 and B = 8;
  - Engine.score end to end (vision tower, projector, prefill, the live rows' lm_head; host clock, the call ends in a
    host read) with prefix_lens = 288 against without, at B = 1 and B = 8;
  - Engine.score_candidates with 8 candidates of 32 tokens against 8 separate one-row score calls.

The legs of a pair alternate in one process after a warm pass of each; a figure is the median of --reps (5).  Prefill
graphs are switched off for the whole run (pgmi_set_prefill_graph(0)): the prefix form is eager by design, and the
plain form is compared launch for launch, not replay against eager.

    timeout -k 10 600 python tools/probes/prefix_probe.py [--reps 5] > profiles/prefix_probe.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "multimodal-financial-analysis-tool-using-paligemma_amd"))
from pgmi import Engine  # noqa: E402
from pgmi import prefix_np as PX  # noqa: E402
from pgmi.synthetic import init_policy, paligemma_3b_config, prompt_ids  # noqa: E402

N_ANS, IGN = 32, -100


def med(xs):
    return f"median {statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cfg = paligemma_3b_config(224)
    n_img, V = 256, cfg["text_config"]["vocab_size"]
    P = n_img + 32
    L = P + N_ANS
    eng = Engine(cfg, max_batch=8, max_seq=L, max_kv=L)
    eng.fill_synthetic(1234, init_policy)
    eng.prepare()
    eng.set_prefill_graph(False)
    g = torch.Generator(device="cuda").manual_seed(5)
    px = (torch.rand((8, 3, 224, 224), generator=g, device="cuda") * 2 - 1).contiguous()
    prompt = torch.from_numpy(prompt_ids(cfg["image_token_index"], n_img, V)).cuda()
    answers = torch.randint(3, 250000, (8, N_ANS), generator=g, device="cuda")
    full = torch.cat([prompt.expand(8, -1), answers], 1).contiguous()
    labels = torch.full_like(full, IGN)
    labels[:, P:] = answers
    print(f"PaliGemma-3B shapes, 224 px, prompt {P} tokens + answer {N_ANS}; prefill graphs off; {a.reps} reps per leg")

    def alternate(legs):
        """legs: {name: fn -> ms}.  One warm pass of each, then reps rounds in the given order."""
        for fn in legs.values():
            fn()
        out = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                out[k].append(fn())
        return out

    for B in (1, 8):
        ids, lab, pxb = full[:B].contiguous(), labels[:B].contiguous(), px[:B].contiguous()
        feats = eng.project(eng.vision(pxb))
        kv = eng.new_kv(B, L)
        plain_pos = torch.arange(L).expand(B, L)
        pfx_pos = torch.from_numpy(PX.prefix_positions(L, [P] * B))

        def lm(prefix):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.lm_forward(kv, 0, pfx_pos if prefix else plain_pos, ids=ids, image_feats=feats, logits_rows=1,
                           prefix_lens=[P] * B if prefix else None)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def score(prefix):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc = eng.score(ids, pxb, lab, prefix_lens=[P] * B if prefix else None)
            float(sc.loss)
            return (time.perf_counter() - t0) * 1e3

        r = alternate({"plain": lambda: lm(False), "prefix": lambda: lm(True)})
        print(f"B={B} lm_forward (events)  plain  {med(r['plain'])}")
        print(f"B={B} lm_forward (events)  prefix {med(r['prefix'])}")
        r = alternate({"plain": lambda: score(False), "prefix": lambda: score(True)})
        print(f"B={B} score (host clock)   plain  {med(r['plain'])}")
        print(f"B={B} score (host clock)   prefix {med(r['prefix'])}")

    cands = [[int(t) for t in row] for row in answers.cpu()]

    def together():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cs = eng.score_candidates(prompt, px[:1], cands)
        cs.sums.cpu()
        return (time.perf_counter() - t0) * 1e3

    def separate():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(8):
            float(eng.score(full[b:b + 1], px[:1], labels[b:b + 1], prefix_lens=[P]).sums[0])
        return (time.perf_counter() - t0) * 1e3

    r = alternate({"together": together, "separate": separate})
    print(f"8 candidates: score_candidates {med(r['together'])}")
    print(f"8 candidates: 8 score calls    {med(r['separate'])}")


if __name__ == "__main__":
    main()
