"""Probe: what the batched decode step (8 and 16 rows per GPU) costs with its gate|up, down and lm_head read from the
fragment-major 13-bit images (pgmi_set_decode_packed_batched) against the bf16 images, on one engine (max_batch =
16) at the full PaliGemma-3B / 224 px shapes with synthetic weights.  Greedy decode, hipGraphs on, 8 steps per
launch (pgmi_decode_steps, what Engine.generate runs).  No prefill: KV rows [0, L) come from a seeded generator
and the ids are random, so the probe runs the decode path alone; every pass restarts at KV row L and decodes the
same tokens.  The masks of --seq run one after the other in one process, each at every batch size; a pass is timed
with a pair of events around its steps (after one untimed pass that builds the images and captures the graphs).
Prints ms per step per pass, whether each pass's token record equals the first mask-0 pass's, and a summary: the
spread of the mask-0 passes is the yardstick for the others.

    timeout -k 10 600 python tools/probes/packed_batched_probe.py [--steps 256] [--seq 0,7,0,7,0,7,1,2,4]
    ... --seq 0,0,0 under PGMI_LIB_PATH=<an older build>: the bf16 step of that build (the setter is never called)
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "multimodal-financial-analysis-tool-using-paligemma_amd"))
from pgmi import Engine  # noqa: E402
from pgmi.synthetic import init_policy, paligemma_3b_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--batches", default="8,16")
    ap.add_argument("--seq", default="0,7,0,7,0,7,1,2,4")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    seq = [int(x) for x in a.seq.split(",")]
    cfg = paligemma_3b_config(224)
    L = 256 + 32
    cap = (L + a.steps + 8 + 63) // 64 * 64
    eng = Engine(cfg, max_batch=max(batches), max_seq=L, max_kv=cap)
    eng.fill_synthetic(1234, init_policy)
    eng.prepare()
    V = cfg["text_config"]["vocab_size"]
    has_setter = hasattr(eng.lib, "pgmi_set_decode_packed_batched")
    if not has_setter and any(seq):
        raise SystemExit("this build has no pgmi_set_decode_packed_batched: --seq 0,0,...")

    state = {}
    for B in batches:   # one cache, one logits buffer and one token record per batch size: stable graph keys
        g = torch.Generator(device="cuda").manual_seed(5 + B)
        kv = torch.zeros_like(eng.new_kv(B, cap))
        kv[:, :, :, :L] = (torch.randn(kv[:, :, :, :L].shape, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
        state[B] = dict(kv=kv, first=torch.randint(3, V - 64, (B,), generator=g, device="cuda"),
                        cur=torch.empty(B, dtype=torch.int64, device="cuda"),
                        logits=torch.empty((B, V), dtype=torch.float32, device="cuda"),
                        rec=torch.empty((a.steps, B), dtype=torch.int64, device="cuda"),
                        chunk=torch.empty((a.chunk, B), dtype=torch.int64, device="cuda"), ref=None)

    def run(B):
        s = state[B]
        s["cur"].copy_(s["first"])
        t = 0
        while t < a.steps:
            k = min(a.chunk, a.steps - t)
            eng.decode_steps(s["cur"], s["kv"], L + t, L + t, k, logits=s["logits"], tokens=s["chunk"], graph=True)
            s["rec"][t:t + k].copy_(s["chunk"][:k])
            t += k

    results = []
    for mask in seq:
        if has_setter:
            eng.set_decode_packed_batched(mask)   # drops the batched graphs: the untimed pass captures them again
        for B in batches:
            run(B)
            run(B)   # (first call of a key runs eagerly, the second captures)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(B)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            s = state[B]
            if s["ref"] is None:
                s["ref"] = s["rec"].clone()
            same = bool(torch.equal(s["rec"], s["ref"]))
            info = eng.decode_packed_batched_info() if has_setter else {"packed": 0}
            results.append((mask, B, ms))
            print(f"{a.tag}mask {mask} B {B:2d}: {ms:.4f} ms/step  {B * 1000.0 / ms:8.1f} tok/s  packed tensors "
                  f"{info['packed']}  tokens equal to the first pass: {same}", flush=True)
    for B in batches:
        base = [ms for m, b, ms in results if m == 0 and b == B]
        if not base:
            continue
        lo, hi = min(base), max(base)
        print(f"{a.tag}B {B:2d}: mask 0 passes {', '.join(f'{x:.4f}' for x in base)} ms/step, spread {hi - lo:.4f}")
        for m in sorted({m for m, _, _ in results if m}):
            ours = [ms for mm, b, ms in results if mm == m and b == B]
            verdict = "faster" if max(ours) < lo - (hi - lo) else "not faster"
            print(f"{a.tag}B {B:2d}: mask {m} passes {', '.join(f'{x:.4f}' for x in ours)} ms/step; slowest of them "
                  f"against the fastest mask-0 pass: {max(ours) - lo:+.4f} ms ({verdict} by more than the spread)")


if __name__ == "__main__":
    main()
