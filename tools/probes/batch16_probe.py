"""Probe: what a decode step costs at 8 and at 16 rows per GPU, on one engine (max_batch = 16) at the full
PaliGemma-3B / 224 px shapes with synthetic weights.  Greedy decode, hipGraphs on, 8 steps per launch
(pgmi_decode_steps, what Engine.generate runs); every pass restarts at KV row L, so all passes of a batch
size decode the same tokens.  B = 8 and B = 16 alternate in one process; each pass is timed with a pair of
events around its steps.  Prints ms per step and tokens/s per pass, then the median and the spread.

    timeout -k 10 300 python tools/probes/batch16_probe.py [--steps 256] [--passes 5] [--chunk 8]
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "multimodal-financial-analysis-tool-using-paligemma_amd"))
from pgmi import Engine  # noqa: E402
from pgmi.synthetic import init_policy, paligemma_3b_config, prompt_ids  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--batches", default="8,16")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    cfg = paligemma_3b_config(224)
    n_img = 256
    L = n_img + 32
    cap = (L + a.steps + 8 + 63) // 64 * 64
    eng = Engine(cfg, max_batch=max(batches), max_seq=L, max_kv=cap)
    eng.fill_synthetic(1234, init_policy)
    eng.prepare()
    V = cfg["text_config"]["vocab_size"]
    g = torch.Generator(device="cuda").manual_seed(5)
    px = (torch.rand((max(batches), 3, 224, 224), generator=g, device="cuda") * 2 - 1).contiguous()
    row = torch.from_numpy(prompt_ids(cfg["image_token_index"], n_img, V)).cuda()

    state = {}
    for B in batches:   # one cache, one logits buffer and one token record per batch size: stable graph keys
        ids = row.expand(B, -1).contiguous()
        kv = eng.new_kv(B, cap)
        feats = eng.project(eng.vision(px[:B].contiguous()))
        lg = eng.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=2)
        state[B] = dict(kv=kv, first=eng.argmax(lg[:, 0]).clone(), cur=torch.empty(B, dtype=torch.int64, device="cuda"),
                        logits=torch.empty((B, V), dtype=torch.float32, device="cuda"),
                        rec=torch.empty((a.steps, B), dtype=torch.int64, device="cuda"),
                        chunk=torch.empty((a.chunk, B), dtype=torch.int64, device="cuda"))

    def run(B):
        s = state[B]
        s["cur"].copy_(s["first"])
        t = 0
        while t < a.steps:
            k = min(a.chunk, a.steps - t)
            # the launch's token record is one buffer (one graph per step count, as Engine.generate), copied out
            eng.decode_steps(s["cur"], s["kv"], L + t, L + t + 1, k, logits=s["logits"], tokens=s["chunk"], graph=True)
            s["rec"][t:t + k].copy_(s["chunk"][:k])
            t += k

    # warm-up: the eager pass (kernel attributes, the fragment-major weight images), the capturing pass, one replay
    ref = {}
    for i in range(3):
        for B in batches:
            run(B)
            torch.cuda.synchronize()
            if i == 0:
                ref[B] = state[B]["rec"].clone()
            else:
                assert torch.equal(state[B]["rec"], ref[B]), f"B = {B}: pass {i} decoded other tokens than the eager pass"
    lo = min(batches)
    # rows 0..lo-1 hold the same images and prompt in every batch size; a prefill of more than 8 rows runs as groups of
    # 8 and the decode steps do not depend on the batch, so they decode the same tokens
    for B in batches:
        same = bool(torch.equal(ref[B][:, :lo], ref[lo]))
        print(f"B={B}: rows 0..{lo - 1} decode the tokens of the B={lo} run: {same}", flush=True)

    times = {B: [] for B in batches}
    for p in range(a.passes):
        for B in batches:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(B)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            times[B].append(ms)
            print(f"pass {p}: B={B} {ms:.4f} ms/step, {B / ms * 1e3:.0f} tokens/s", flush=True)
    for B in batches:
        t = times[B]
        med = statistics.median(t)
        print(f"B={B}: median {med:.4f} ms/step (min {min(t):.4f}, max {max(t):.4f}, {len(t)} passes of {a.steps} steps, "
              f"{a.chunk} steps per launch) = {B / med * 1e3:.0f} tokens/s per GPU", flush=True)
    if len(batches) == 2:
        b0, b1 = batches
        r = (b1 / statistics.median(times[b1])) / (b0 / statistics.median(times[b0]))
        print(f"tokens/s at B={b1} over B={b0}: {r:.3f}x", flush=True)
    mem = torch.cuda.max_memory_allocated() / 2**30
    print(f"torch allocations (weights, KV caches, buffers): {mem:.2f} GiB peak; "
          f"KV cache of {max(batches)} rows x {cap} tokens: {eng.lib.pgmi_kv_bytes(eng.ctx, max(batches), cap) / 2**20:.0f} MiB",
          flush=True)


if __name__ == "__main__":
    main()
