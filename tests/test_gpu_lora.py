"""LoRA adapters on the device: the merge kernel against the numpy rule, and an engine that switches adapters in
place against fresh engines whose weights are the numpy merge of the base, loaded through load_state_dict.  Every
result is compared as raw bits.  The 2-text-layer full-width config, a 224 px image and a 31-token prompt, as
smoke(); the adapters are peft directories written into tmp_path from a seeded generator."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import paligemma_np as O
from oracle import weights as W

pytestmark = pytest.mark.gpu
SEED, V, KV, NTOK = 1234, 4096, 512, 4
CFG = W.small_config(vision_layers=1, text_layers=2, vocab=V)
SHAPES = [(7, 24, 1), (256, 2048, 8), (1152, 1152, 16), (1152, 4304, 64), (33, 16384, 256)]
TL = "language_model.model.layers.%d."
VL = "vision_tower.vision_model.encoder.layers.0."
GATE1 = TL % 1 + "mlp.gate_proj"
Q0 = TL % 0 + "self_attn.q_proj"
QKV = [TL % i + "self_attn." + p for i in (0, 1) for p in ("q_proj", "k_proj", "v_proj")] + \
      [VL + "self_attn." + p for p in ("q_proj", "k_proj", "v_proj")]
# adapter b: other targets than a's -- o_proj, the MLP of layer 1, the vision fc1 and the projector
OTHER = [TL % 0 + "self_attn.o_proj", TL % 1 + "self_attn.o_proj", GATE1, TL % 1 + "mlp.up_proj",
         TL % 1 + "mlp.down_proj", VL + "mlp.fc1", "multi_modal_projector.linear"]


def new_engine(max_batch=3):
    from pgmi import Engine
    return Engine(CFG, max_batch=max_batch, max_seq=320, max_kv=KV)


def write_adapter(path, shapes, modules, r, alpha, seed, zero_b=False, single=None):
    """A peft directory: adapter_config.json + adapter_model.safetensors; returns {weight name: (A, B, s)}."""
    from safetensors.numpy import save_file
    from pgmi import lora as LR
    g = np.random.default_rng(seed)
    tensors, targets = {}, {}
    for m in modules:
        N, K = shapes[m + ".weight"]
        A = g.standard_normal((r, K), dtype=np.float32) * np.float32(0.02)
        B = g.standard_normal((N, r), dtype=np.float32) * np.float32(0.02)
        if zero_b:
            B[:] = 0     # peft's initial state
        if single is not None:   # one delta element: B[n0][0] * A[0][k0] * s
            n0, k0, val = single
            A[:], B[:] = 0, 0
            A[0, k0], B[n0, 0] = val, 1
        tensors[f"base_model.model.{m}.lora_A.weight"] = A
        tensors[f"base_model.model.{m}.lora_B.weight"] = B
        targets[m + ".weight"] = (A, B, LR.scaling_of(alpha, r))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "use_dora": False,
                   "use_rslora": False, "fan_in_fan_out": False, "alpha_pattern": {}}, f)
    save_file(tensors, os.path.join(path, "adapter_model.safetensors"))
    return targets


def merged_sd(base, *target_dicts, changes=None):
    """The base state dict with merge_np applied to every target (on the host)."""
    from pgmi import lora as LR
    sd = dict(base)
    for name, t in (changes or {}).items():
        sd[name] = t
    for targets in target_dicts:
        for name, (A, B, s) in targets.items():
            bits = sd[name].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            sd[name] = torch.from_numpy(LR.merge_np(bits, A, B, s).view(np.int16)).view(torch.bfloat16)
    return sd


class State:
    pass


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    s = State()
    s.eng = new_engine()
    s.eng.fill_synthetic(SEED, W.init_policy)
    s.eng.prepare()
    torch.cuda.synchronize()
    s.base = {n: v.clone() for n, v in s.eng.views.items()}   # before the first activation
    shapes = {n: tuple(v.shape) for n, v in s.eng.views.items()}
    d = tmp_path_factory.mktemp("adapters")
    s.path, s.targets = {}, {}
    for name, kw in {"a": dict(modules=QKV, r=8, alpha=16, seed=1), "b": dict(modules=OTHER, r=16, alpha=32, seed=2),
                     "zero": dict(modules=QKV, r=8, alpha=16, seed=3, zero_b=True),
                     "big": dict(modules=[GATE1], r=1, alpha=1, seed=4, single=(5, 77, np.float32(2.0 ** 12)))}.items():
        s.path[name] = str(d / name)
        s.targets[name] = write_adapter(s.path[name], shapes, **kw)
        s.eng.load_lora(s.path[name], name)   # through read_peft
    rng = np.random.default_rng(0)
    n_img = W.num_image_tokens(CFG)
    s.inputs, s.kv = {}, {}
    for B in (1, 2, 3):
        px = O.bf16(rng.uniform(-1, 1, (B, 3, 224, 224)).astype(np.float32))
        ids = np.array([[CFG["image_token_index"]] * n_img + [2] + list(rng.integers(3, 4000, 30)) + [108]
                        for _ in range(B)])
        s.inputs[B] = (torch.from_numpy(ids).cuda(), torch.from_numpy(px).cuda())
    s.base_out = {B: [run(s, s.eng, B) for _ in range(2)][1] for B in (1, 2, 3)}   # twice: graphs captured
    s.fresh = {}
    return s


def run(s, e, B):
    """Prefill logits (last row), NTOK greedy tokens and the final step's logits of a batch of B."""
    ids, px = s.inputs[B]
    kv = s.kv.setdefault((id(e), B), e.new_kv(B, KV))   # the same buffers every time: graphs are replayed
    L = ids.shape[1]
    feats = e.project(e.vision(px))
    pre = e.lm_forward(kv, 0, torch.arange(L)[None], ids=ids, image_feats=feats, logits_rows=1)[:, 0].clone()
    toks = e.generate(ids, px, NTOK, graph=True, kv=kv).clone()
    last = e._gen_buf[B][0].clone()
    torch.cuda.synchronize()
    return pre, toks, last


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def fresh(s, *names, changes=None, key=None):
    """A new engine whose weights are merge_np of the base under the named adapters, through load_state_dict."""
    key = key or names
    if key not in s.fresh:
        e = new_engine()
        e.load_state_dict(merged_sd(s.base, *(s.targets[n] for n in names), changes=changes))
        e.prepare()
        s.fresh[key] = e
    return s.fresh[key]


def packed_all(e):
    return [e.decode_packed_tensor(k, l) for k in (1, 2) for l in (0, 1)] + [e.decode_packed_tensor(4)]


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("N,K,r", SHAPES)
def test_kernel_equals_rule(S, N, K, r):
    from pgmi import _native as Nt
    from pgmi import lora as LR
    g = np.random.default_rng(100 + r)
    Wf = (g.standard_normal((N, K), dtype=np.float32) * np.float32(0.05))
    Wb = torch.from_numpy(Wf).to(torch.bfloat16)
    A = g.standard_normal((r, K), dtype=np.float32) * np.float32(0.1)
    B = g.standard_normal((N, r), dtype=np.float32) * np.float32(0.1)
    s = np.float32(16.0 / r)
    ref = LR.merge_np(Wb.view(torch.int16).numpy().view(np.uint16), A, B, s)
    dW, dA, dB = Wb.cuda(), torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    out = torch.full((N + 1, K), -1.0, dtype=torch.bfloat16, device="cuda")   # a guard row behind the tensor
    Nt.check(Nt.lib().pgmi_op_lora_merge(S.eng.ctx, dW.data_ptr(), N, K, dA.data_ptr(), dB.data_ptr(), r, float(s),
                                         out.data_ptr(), None), "pgmi_op_lora_merge")
    torch.cuda.synchronize()
    got = out[:N].view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert bool((out[N] == -1.0).all())   # nothing past the last row
    assert int((got != Wb.view(torch.int16).numpy().view(np.uint16)).sum()) > N * K // 2


# ---------------------------------------------------------------- 2. q/k/v adapter against a fresh engine
def test_qkv_adapter_equals_fresh_engine(S):
    e = S.eng
    e.set_lora(None)
    run(S, e, 1)
    assert e.decode_packed_info()["scanned"] == 7
    e.set_lora("a")
    assert e.active_lora == "a"
    assert e.decode_packed_info()["scanned"] == 7       # no kind forgotten by a q/k/v switch ...
    ref = fresh(S, "a")
    for B in (1, 2, 3):
        want = run(S, ref, B)
        for _ in range(2):                               # graphs captured under the base are replayed
            got = run(S, e, B)
            assert same(got, want), B
        assert not torch.equal(got[0], S.base_out[B][0])  # and the adapter does change the logits
        if B == 1:
            info = e.decode_packed_info()
            assert info["scanned"] == 7 and info["packed"] == 5 and all(packed_all(e))   # ... nor rescanned
    li = e.lora_info("a")
    n_el = sum(int(np.prod(e.views[m + ".weight"].shape)) for m in QKV)
    assert li["targets"] == len(QKV) and li["pristine_bytes"] == 2 * n_el
    assert li["factor_bytes"] == sum(4 * 8 * sum(e.views[m + ".weight"].shape) for m in QKV)


# ---------------------------------------------------------------- 3. back to the base
def test_deactivation_restores_every_byte(S):
    e = S.eng
    e.set_lora("a")
    assert not torch.equal(e.views[Q0 + ".weight"], S.base[Q0 + ".weight"])
    e.set_lora("b")
    e.set_lora(None)
    assert e.active_lora is None
    for n, v in e.views.items():
        assert torch.equal(v.view(torch.int16), S.base[n].view(torch.int16)), n
    for B in (1, 2, 3):
        assert same(run(S, e, B), S.base_out[B]), B


# ---------------------------------------------------------------- 4. two adapters with different targets
def test_switching_between_adapters(S):
    e = S.eng
    e.set_lora(None)
    run(S, e, 1)
    e.set_lora("a")
    e.set_lora("b")
    assert e.decode_packed_info()["scanned"] == 4        # gate|up and down are rebuilt, lm_head is kept
    rb = fresh(S, "b")
    for B in (1, 2, 3):
        assert same(run(S, e, B), run(S, rb, B)), B
        if B == 1:
            assert e.decode_packed_info()["scanned"] == 7 and all(packed_all(e))   # the merged tensors, packed
    # a's targets that b lacks were restored, b's were merged from the base: the slab is the fresh engine's
    for n, v in e.views.items():
        assert torch.equal(v.view(torch.int16), rb.views[n].view(torch.int16)), n
    e.set_lora("a")
    ra = fresh(S, "a")
    for B in (1, 3):
        assert same(run(S, e, B), run(S, ra, B)), B
    # generate(adapter=...) switches as set_lora does
    ids, px = S.inputs[1]
    kv = S.kv[(id(e), 1)]
    toks = e.generate(ids, px, NTOK, kv=kv, adapter="b")
    assert e.active_lora == "b" and torch.equal(toks, run(S, rb, 1)[1])
    assert torch.equal(e.generate(ids, px, NTOK, kv=kv), toks) and e.active_lora == "b"   # left out: stays
    toks = e.generate(ids, px, NTOK, kv=kv, adapter=None)
    assert e.active_lora is None and torch.equal(toks, S.base_out[1][1])


# ---------------------------------------------------------------- 5. an adapter that breaks a 13-bit fit
def test_adapter_that_breaks_the_13_bit_fit(S):
    from pgmi import _native as Nt
    e = S.eng
    e.set_lora(None)
    sd = merged_sd(S.base, S.targets["big"])
    gu = torch.cat([sd[GATE1 + ".weight"].cpu(), sd[TL % 1 + "mlp.up_proj.weight"].cpu()]).contiguous()
    host = gu.view(torch.int16).cpu().numpy().view(np.uint16)
    e_hi, fits = ctypes.c_int(), ctypes.c_int()
    Nt.check(Nt.lib().pgmi_pack13_scan(host.ctypes.data, host.size, ctypes.byref(e_hi), ctypes.byref(fits)))
    assert fits.value == 0, e_hi.value                   # the precondition: the merged gate|up does not fit
    e.set_lora("big")
    got = run(S, e, 1)
    assert packed_all(e) == [True, False, True, True, True]   # layer 1's gate|up raw, the others packed
    info = e.decode_packed_info()
    assert (info["packed"], info["raw"]) == (4, 1)
    ref = fresh(S, "big")
    assert same(got, run(S, ref, 1)) and same(run(S, e, 2), run(S, ref, 2))
    assert not torch.equal(got[0], S.base_out[1][0])
    e.set_lora(None)
    assert same(run(S, e, 1), S.base_out[1])
    assert all(packed_all(e))                            # the packed image is back


# ---------------------------------------------------------------- 6. B = 0
def test_zero_B_adapter_is_the_base(S):
    e = S.eng
    e.set_lora("zero")
    for B in (1, 3):
        assert same(run(S, e, B), S.base_out[B]), B
    e.set_lora(None)


# ---------------------------------------------------------------- 7. guards
def test_guards(S):
    e = S.eng
    e.set_lora("a")
    with pytest.raises(RuntimeError, match="deactivate first"):
        e.load_state_dict(S.base)
    with pytest.raises(RuntimeError, match="deactivate first"):
        e.fill_synthetic(SEED, W.init_policy)
    with pytest.raises(RuntimeError, match="deactivate first"):
        e.unload_lora("a")
    name = (Q0 + ".weight").encode()
    src = S.base[Q0 + ".weight"]
    from pgmi import _native as Nt
    assert Nt.lib().pgmi_load_weight(e.ctx, name, src.data_ptr(), Nt.DTYPE_BF16, 1, None) == Nt.PGMI_E_STATE
    assert b"deactivate first" in Nt.lib().pgmi_last_error()
    want = run(S, fresh(S, "a"), 1)
    e.prepare()                                          # while active: derives from the slab as it is
    assert e.active_lora == "a" and same(run(S, e, 1), want) and same(run(S, e, 3), run(S, fresh(S, "a"), 3))
    e.set_lora(None)                                     # the copies were kept: the base comes back
    assert torch.equal(e.views[Q0 + ".weight"].view(torch.int16), S.base[Q0 + ".weight"].view(torch.int16))
    # prepare() while inactive, a base-weight change, then activation: merged onto the new base
    w = e.views[Q0 + ".weight"]
    try:
        e.prepare()
        w.mul_(2)                                        # exact in bf16
        e.set_lora("a")
        ref = fresh(S, "a", changes={Q0 + ".weight": S.base[Q0 + ".weight"] * 2}, key="a on 2 x q_proj")
        assert torch.equal(w.view(torch.int16), ref.views[Q0 + ".weight"].view(torch.int16))
        for B in (1, 3):
            assert same(run(S, e, B), run(S, ref, B)), B
        e.set_lora(None)
        assert torch.equal(w.view(torch.int16), (S.base[Q0 + ".weight"] * 2).view(torch.int16))
    finally:
        e.set_lora(None)
        w.copy_(S.base[Q0 + ".weight"])
        e.prepare()
    assert same(run(S, e, 1), S.base_out[1])


# ---------------------------------------------------------------- 8. the drop-in model
@torch.no_grad()
def test_drop_in_model(S):
    import modeling_gemma as MG
    import utils as U
    from pgmi import Engine, binding
    pcfg = MG.PaliGemmaConfig(**{k: v for k, v in CFG.items() if k not in ("bos_token_id", "eos_token_id")})
    model = U.build_model(pcfg, device="cuda")
    model.load_state_dict({n: t.clone() for n, t in S.base.items()}, strict=False)
    model.tie_weights()
    model.eval()
    assert model.pgmi_lookahead
    ids, px = S.inputs[1]
    L = ids.shape[1]

    def loop():
        """inference.py's greedy loop, 4 tokens: each step's last-row logits."""
        cur, mask, kv, out = ids, torch.ones_like(ids), MG.KVCache(), []
        for _ in range(NTOK):
            o = model(input_ids=cur, pixel_values=px, attention_mask=mask, kv_cache=kv)
            kv = o["kv_cache"]
            out.append(o["logits"][:, -1, :].clone())
            cur = torch.argmax(out[-1], dim=-1, keepdim=True)
            mask = torch.cat([mask, torch.ones((1, 1), device=ids.device, dtype=mask.dtype)], dim=-1)
        torch.cuda.synchronize()
        return out

    base = loop()
    model.pgmi_load_lora(S.path["a"], "a")
    model.pgmi_set_lora("a")
    got = loop()
    assert not torch.equal(got[0], base[0])
    # the Engine path under the same adapter (an engine of the binding's capacities)
    e = Engine(CFG, max_batch=binding.DEFAULT_MAX_BATCH, max_seq=binding.DEFAULT_MAX_SEQ)
    e.load_state_dict(S.base)
    e.prepare()
    e.load_lora(S.path["a"], "a")
    e.set_lora("a")
    kv = e.new_kv(1, L + NTOK + 1)
    feats = e.project(e.vision(px))
    want = [e.lm_forward(kv, 0, torch.arange(L)[None], ids=ids, image_feats=feats, logits_rows=1)[:, 0].clone()]
    for t in range(1, NTOK):
        cur = want[-1].argmax(-1)
        want.append(e.decode(cur, kv, L + t - 1, L + t, graph=True).clone())
    torch.cuda.synchronize()
    assert same(got, want)
    first = model.__dict__["_pgmi_bound"].engine
    model.pgmi_rebind()
    again = loop()
    second = model.__dict__["_pgmi_bound"].engine
    assert second is not first and second.active_lora == "a" and same(again, got)
    model.pgmi_set_lora(None)
    assert same(loop(), base)
    # an in-place update of a watched weight while an adapter is active is refused at the next prefill
    model.pgmi_set_lora("a")
    model.language_model.model.layers[0].self_attn.q_proj.weight.mul_(1)
    with pytest.raises(RuntimeError, match="pgmi_set_lora"):
        model(input_ids=ids, pixel_values=px, attention_mask=torch.ones_like(ids), kv_cache=MG.KVCache())
