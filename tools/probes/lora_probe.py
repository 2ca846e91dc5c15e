"""Probe: what LoRA adapters cost at the full PaliGemma-3B / 224 px shapes with synthetic weights -- two q/k/v
adapters of rank 16 on both towers (the reference's own LoraConfig targets), one engine (max_batch = 8).

  - wall time of Engine.set_lora (host clock; the call synchronises the device on entry and its stream on exit):
    base -> a (first activation: the pristine copies are allocated and taken), a -> b, b -> a, a -> base, base -> a
    (copies held);
  - the first B = 1 and the first B = 8 decode step after a switch (host clock around step + synchronise; the B = 8
    one rebuilds the fragment-major images), against a warm step;
  - factor bytes and pristine-copy bytes (pgmi_lora_info);
  - B = 1 ms per decode step over --steps graphed steps with the adapter active against the base: one process,
    alternating, --pairs pairs, each pass timed by a pair of events after a warm pass under the same weights.  The
    step runs the same kernels on the same bytes either way; the base's own pass-to-pass spread is the yardstick.

    timeout -k 10 600 python tools/probes/lora_probe.py [--steps 256] [--pairs 3] > profiles/lora_probe.txt
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
from pgmi.lora import scaling_of  # noqa: E402
from pgmi.synthetic import init_policy, paligemma_3b_config, prompt_ids  # noqa: E402

R = 16


def qkv_adapter(eng, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, v in eng.views.items():
        if name.endswith(("q_proj.weight", "k_proj.weight", "v_proj.weight")):
            N, K = v.shape
            out[name] = (torch.randn((R, K), generator=g) * 0.02, torch.randn((N, R), generator=g) * 0.02,
                         scaling_of(2 * R, R))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    cfg = paligemma_3b_config(224)
    n_img, V = 256, cfg["text_config"]["vocab_size"]
    L = n_img + 32
    cap = (L + a.steps + 8 + 63) // 64 * 64
    eng = Engine(cfg, max_batch=8, max_seq=L, max_kv=cap)
    eng.fill_synthetic(1234, init_policy)
    eng.prepare()
    for name, seed in (("a", 1), ("b", 2)):
        eng.load_lora(qkv_adapter(eng, seed), name)
    g = torch.Generator(device="cuda").manual_seed(5)
    px = (torch.rand((8, 3, 224, 224), generator=g, device="cuda") * 2 - 1).contiguous()
    row = torch.from_numpy(prompt_ids(cfg["image_token_index"], n_img, V)).cuda()
    st = {}
    for B in (1, 8):
        st[B] = dict(ids=row.expand(B, -1).contiguous(), kv=eng.new_kv(B, cap),
                     cur=torch.empty(B, dtype=torch.int64, device="cuda"),
                     logits=torch.empty((B, V), dtype=torch.float32, device="cuda"))

    def prefill(B):
        s = st[B]
        feats = eng.project(eng.vision(px[:B].contiguous()))
        lg = eng.lm_forward(s["kv"], 0, torch.arange(L).expand(B, L), ids=s["ids"], image_feats=feats, logits_rows=2)
        s["first"] = eng.argmax(lg[:, 0]).clone()

    def steps(B, n):
        s = st[B]
        s["cur"].copy_(s["first"])
        for t in range(n):
            eng.decode(s["cur"], s["kv"], L + t, L + t + 1, logits=s["logits"], next_ids=s["cur"], graph=True)

    def one_step_ms(B):
        s = st[B]
        s["cur"].copy_(s["first"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode(s["cur"], s["kv"], L, L + 1, logits=s["logits"], next_ids=s["cur"], graph=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def switch(name, label):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_lora(name)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"set_lora {label}: {ms:.2f} ms", flush=True)

    for B in (1, 8):   # warm: eager, capture, replay; the 13-bit and fragment-major images are built here
        prefill(B)
        for _ in range(3):
            steps(B, 4)
        torch.cuda.synchronize()
        print(f"B={B}: warm step under the base {one_step_ms(B):.3f} ms (host clock, one step)", flush=True)

    switch("a", "base -> a (first activation: copies allocated and taken)")
    for B in (1, 8):
        print(f"B={B}: first step after the switch {one_step_ms(B):.3f} ms, the next {one_step_ms(B):.3f} ms", flush=True)
    switch("b", "a -> b")
    switch("a", "b -> a")
    switch(None, "a -> base")
    for B in (1, 8):
        print(f"B={B}: first step after a -> base {one_step_ms(B):.3f} ms, the next {one_step_ms(B):.3f} ms", flush=True)
    switch("a", "base -> a (copies held)")
    info = eng.lora_info("a")
    print(f"adapter a: {info['targets']} targets, factors {info['factor_bytes'] / 2**20:.2f} MiB resident (fp32), "
          f"pristine copies {info['pristine_bytes'] / 2**20:.2f} MiB", flush=True)
    print(f"13-bit images after the switches: {eng.decode_packed_info()}", flush=True)

    times = {"base": [], "a": []}
    for p in range(a.pairs):
        for label in ("base", "a"):
            eng.set_lora(None if label == "base" else "a")
            prefill(1)
            steps(1, a.steps)   # warm pass under these weights
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            steps(1, a.steps)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            times[label].append(ms)
            print(f"pair {p}: {label:4s} B=1 {ms:.4f} ms/step over {a.steps} steps", flush=True)
    for label, t in times.items():
        print(f"{label:4s}: median {statistics.median(t):.4f} ms/step (min {min(t):.4f}, max {max(t):.4f})", flush=True)
    d = statistics.median(times["a"]) - statistics.median(times["base"])
    print(f"adapter - base: {d * 1e3:+.2f} us/step; the base's own spread over the pairs: "
          f"{(max(times['base']) - min(times['base'])) * 1e3:.2f} us", flush=True)


if __name__ == "__main__":
    main()
