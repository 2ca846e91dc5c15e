"""Probe: what forward(labels=...) costs through the drop-in model with pgmi_fused_loss off (torch's
CrossEntropyLoss on the materialised (B, L, V) logits) and on (Engine.lm_logprobs on the live hidden rows), at the
full PaliGemma-3B / 224 px shapes (L = 288, V = 257,216) with synthetic weights.  Three label patterns: B = 1 with
all 287 shifted labels live, B = 1 with the last 32 live, B = 8 with the last 32 of every row live.  Off and on
alternate in one process; each call is timed with a pair of events around the whole forward (prefill included)
and its torch.cuda.max_memory_allocated growth is taken from a reset peak.  Prints every pass, then the medians.

    timeout -k 10 600 python tools/probes/score_probe.py [--passes 5] > profiles/score_probe.txt
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "multimodal-financial-analysis-tool-using-paligemma_amd"))
import modeling_gemma as MG  # noqa: E402
import utils as U  # noqa: E402
from pgmi.synthetic import init_policy, paligemma_3b_config, prompt_ids  # noqa: E402


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    cfg = paligemma_3b_config(224)
    pcfg = MG.PaliGemmaConfig(**{k: v for k, v in cfg.items() if k not in ("bos_token_id", "eos_token_id")})
    model = U.build_model(pcfg, device="cuda")
    model.tie_weights()
    eng = model._pgmi_engine()
    eng.fill_synthetic(1234, init_policy)
    eng.prepare()
    model.eval()
    V = cfg["text_config"]["vocab_size"]
    n_img = 256
    g = torch.Generator(device="cuda").manual_seed(5)
    px = (torch.rand((8, 3, 224, 224), generator=g, device="cuda") * 2 - 1).contiguous()
    row = torch.from_numpy(prompt_ids(cfg["image_token_index"], n_img, V)).cuda()
    L = row.numel()
    ign = pcfg.ignore_index

    def labels(B, live):
        lb = torch.randint(0, V, (B, L), generator=g, device="cuda")
        lb[:, :L - live] = ign
        return lb

    cases = [("B=1, all 287 labels live", 1, labels(1, L)), ("B=1, last 32 labels live", 1, labels(1, 32)),
             ("B=8, last 32 labels live", 8, labels(8, 32))]

    def call(B, lb, fused):
        model.pgmi_fused_loss = fused
        ids = row.expand(B, -1).contiguous()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = model(input_ids=ids, pixel_values=px[:B], attention_mask=torch.ones_like(ids), labels=lb)
        loss = out["loss"]
        e1.record()
        e1.synchronize()
        grow = torch.cuda.max_memory_allocated() - before
        return e0.elapsed_time(e1), grow, float(loss), out["logits"].is_materialized

    print(f"L = {L}, V = {V}; one (L, V) fp32 tensor: {L * V * 4 / 2**20:.0f} MiB", flush=True)
    for name, B, lb in cases:
        res = {False: [], True: []}
        for p in range(a.passes + 1):   # pass 0: warm-up (kernel attributes, allocator), not counted
            for fused in (False, True):
                ms, grow, loss, mat = call(B, lb, fused)
                if p:
                    res[fused].append((ms, grow))
                print(f"{name}: pass {p} fused_loss={'on ' if fused else 'off'} {ms:8.3f} ms  "
                      f"memory growth {grow / 2**20:9.1f} MiB  loss {loss:.6f}  logits materialised: {mat}", flush=True)
        for fused in (False, True):
            t = [r[0] for r in res[fused]]
            m = max(r[1] for r in res[fused])
            print(f"{name}: fused_loss={'on ' if fused else 'off'} median {statistics.median(t):.3f} ms (min {min(t):.3f}, "
                  f"max {max(t):.3f}, {len(t)} passes), memory growth {m / 2**20:.1f} MiB", flush=True)
        off, on = statistics.median(r[0] for r in res[False]), statistics.median(r[0] for r in res[True])
        print(f"{name}: off / on = {off / on:.2f}x", flush=True)


if __name__ == "__main__":
    main()
