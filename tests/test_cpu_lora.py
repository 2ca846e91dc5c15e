"""LoRA adapters on the host: the merge rule (csrc/lora.h through pgmi_lora_merge_host, pgmi.lora.merge_np and a
scalar transcription written here agree bit for bit), the peft checkpoint reader, and the C ABI's refusals, none
of which needs a device."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import weights as W

SHAPES = [(7, 24, 1), (256, 2048, 8), (1152, 1152, 16), (1152, 4304, 64), (33, 16384, 256)]
QP = "language_model.model.layers.0.self_attn.q_proj"


def bf16_bits(x):
    """fp32 -> bf16 bit patterns (RNE; finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def make_case(N, K, r, seed):
    g = np.random.default_rng(seed)
    Wb = bf16_bits(g.standard_normal((N, K), dtype=np.float32) * np.float32(0.05))
    A = g.standard_normal((r, K), dtype=np.float32) * np.float32(0.1)
    B = g.standard_normal((N, r), dtype=np.float32) * np.float32(0.1)
    return Wb, A, B, np.float32(16.0 / r)


def host_merge(Wb, A, B, s):
    from pgmi import _native as Nt
    out = np.empty_like(Wb)
    rc = Nt.lib().pgmi_lora_merge_host(Wb.ctypes.data, Wb.shape[0], Wb.shape[1], A.ctypes.data, B.ctypes.data,
                                       A.shape[0], float(s), out.ctypes.data)
    Nt.check(rc, "pgmi_lora_merge_host")
    return out


@pytest.mark.parametrize("N,K,r", SHAPES)
def test_host_rule_equals_numpy_rule(N, K, r):
    from pgmi import lora as LR
    Wb, A, B, s = make_case(N, K, r, 100 + r)
    got, ref = host_merge(Wb, A, B, s), LR.merge_np(Wb, A, B, s)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert int((got != Wb).sum()) > Wb.size // 2   # the adapter did change the weight


def test_numpy_rule_equals_scalar_transcription():
    from pgmi import lora as LR
    N, K, r = 5, 16, 3
    Wb, A, B, s = make_case(N, K, r, 7)
    Wb[0, 0], Wb[1, 1] = 0x0000, 0x8000   # zeros of both signs
    out = np.empty_like(Wb)
    f32 = np.float32
    for n in range(N):
        for k in range(K):
            acc = f32(0.0)
            for j in range(r):
                acc = f32(acc + f32(B[n, j] * A[j, k]))
            w = np.array([int(Wb[n, k]) << 16], np.uint32).view(np.float32)[0]
            v = f32(w + f32(acc * s))
            u = int(np.array([v], np.float32).view(np.uint32)[0])
            out[n, k] = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    assert np.array_equal(LR.merge_np(Wb, A, B, s), out)
    assert np.array_equal(host_merge(Wb, A, B, s), out)


def test_zero_B_returns_W_unchanged():
    from pgmi import lora as LR
    Wb, A, B, s = make_case(33, 64, 8, 9)
    Wb[0, :3] = [0x0000, 0x0001, 0x807F]   # a zero and denormals come back as they are
    B[:] = 0
    assert np.array_equal(LR.merge_np(Wb, A, B, s), Wb)
    assert np.array_equal(host_merge(Wb, A, B, s), Wb)
    # the one value the rule does not return: -0 + (+0) is +0 in IEEE arithmetic (the same number, another pattern)
    Wb[0, 3] = 0x8000
    for got in (LR.merge_np(Wb, A, B, s), host_merge(Wb, A, B, s)):
        assert got[0, 3] == 0x0000 and int((got != Wb).sum()) == 1


# ---------------------------------------------------------------- read_peft
def write_peft(dirpath, tensors, **cfg):
    from safetensors.numpy import save_file
    os.makedirs(dirpath, exist_ok=True)
    base = {"peft_type": "LORA", "r": 8, "lora_alpha": 16, "bias": "none", "use_dora": False, "use_rslora": False,
            "fan_in_fan_out": False, "alpha_pattern": {}, "target_modules": ["q_proj", "k_proj", "v_proj"]}
    base.update(cfg)
    with open(os.path.join(dirpath, "adapter_config.json"), "w") as f:
        json.dump(base, f)
    save_file({k: np.ascontiguousarray(v) for k, v in tensors.items()},
              os.path.join(dirpath, "adapter_model.safetensors"))
    return str(dirpath)


def factors(r=8, N=2048, K=2048, seed=0, dtype=np.float32):
    g = np.random.default_rng(seed)
    return (g.standard_normal((r, K), dtype=np.float32).astype(dtype),
            g.standard_normal((N, r), dtype=np.float32).astype(dtype))


def test_read_peft_names_and_scaling(tmp_path):
    from pgmi import lora as LR
    A, B = factors()
    A2, B2 = factors(r=4, N=1152, K=1152, seed=1, dtype=np.float16)
    VQ = "vision_tower.vision_model.encoder.layers.0.self_attn.out_proj"
    d = write_peft(tmp_path / "a", {f"base_model.model.{QP}.lora_A.weight": A, f"base_model.model.{QP}.lora_B.weight": B,
                                    f"base_model.model.{VQ}.lora_A.default.weight": A2,
                                    f"base_model.model.{VQ}.lora_B.default.weight": B2}, lora_alpha=32)
    ad = LR.read_peft(d)
    assert sorted(ad.targets) == sorted([QP + ".weight", VQ + ".weight"])
    a, b, s = ad.targets[QP + ".weight"]
    assert a.dtype == np.float32 and np.array_equal(a, A) and np.array_equal(b, B)
    assert s.dtype == np.float32 and s == np.float32(32 / 8)
    a2, b2, s2 = ad.targets[VQ + ".weight"]
    assert np.array_equal(a2, A2.astype(np.float32)) and np.array_equal(b2, B2.astype(np.float32))   # F16 widens exactly
    assert s2 == np.float32(32 / 4)   # r from the shapes
    # the file itself, with the config beside it
    assert sorted(LR.read_peft(os.path.join(d, "adapter_model.safetensors")).targets) == sorted(ad.targets)
    # rslora: alpha / sqrt(r), float64 then one rounding
    A3, B3 = factors(r=3)
    d = write_peft(tmp_path / "b", {f"base_model.model.{QP}.lora_A.weight": A3,
                                    f"base_model.model.{QP}.lora_B.weight": B3}, lora_alpha=7, use_rslora=True)
    assert LR.read_peft(d).targets[QP + ".weight"][2] == np.float32(7.0 / np.sqrt(np.float64(3)))
    assert LR.scaling_of(16, 8) == np.float32(2.0)


def test_read_peft_bf16_widens_exactly(tmp_path):
    import torch
    from safetensors.torch import save_file
    from pgmi import lora as LR
    A, B = (torch.from_numpy(x).to(torch.bfloat16) for x in factors())
    os.makedirs(tmp_path / "c")
    with open(tmp_path / "c" / "adapter_config.json", "w") as f:
        json.dump({"lora_alpha": 8, "r": 8}, f)
    save_file({f"base_model.model.{QP}.lora_A.weight": A, f"base_model.model.{QP}.lora_B.weight": B},
              str(tmp_path / "c" / "adapter_model.safetensors"))
    a, b, s = LR.read_peft(str(tmp_path / "c")).targets[QP + ".weight"]
    assert np.array_equal(a, A.float().numpy()) and np.array_equal(b, B.float().numpy()) and s == np.float32(1.0)


def test_read_peft_refusals(tmp_path):
    from pgmi import lora as LR
    A, B = factors()
    ka, kb = f"base_model.model.{QP}.lora_A.weight", f"base_model.model.{QP}.lora_B.weight"
    good = {ka: A, kb: B}
    E = "language_model.model.embed_tokens"
    cases = [
        (good, {"use_dora": True}, "use_dora"),
        (good, {"bias": "all"}, "bias"),
        (good, {"bias": "lora_only"}, "bias"),
        (good, {"fan_in_fan_out": True}, "fan_in_fan_out"),
        (good, {"alpha_pattern": {"q_proj": 4}}, "alpha_pattern"),
        ({**good, f"base_model.model.{E}.lora_embedding_A": np.zeros((8, 64), np.float32)}, {}, "lora_embedding_A"),
        ({**good, f"base_model.model.{QP}.lora_magnitude_vector": np.zeros(8, np.float32)}, {}, "lora_magnitude_vector"),
        ({**good, "base_model.model.language_model.model.norm.weight": np.zeros(2048, np.float32)}, {}, "norm.weight"),
        ({ka: A}, {}, ka),                                              # an A without its B
        ({kb: B}, {}, kb),
        ({ka: A, kb: factors(r=4)[1]}, {}, "mismatched ranks"),
        # targets that are not Linear slab weights
        ({f"base_model.model.{E}.lora_A.weight": A, f"base_model.model.{E}.lora_B.weight": B}, {}, "embed_tokens"),
        ({"base_model.model.vision_tower.vision_model.embeddings.patch_embedding.lora_A.weight": A,
          "base_model.model.vision_tower.vision_model.embeddings.patch_embedding.lora_B.weight": B}, {},
         "patch_embedding"),
    ]
    for i, (tensors, cfg, needle) in enumerate(cases):
        d = write_peft(tmp_path / f"r{i}", tensors, **cfg)
        with pytest.raises(ValueError, match=needle.replace(".", r"\.")):
            LR.read_peft(d)
    LR.read_peft(write_peft(tmp_path / "ok", good))   # and the plain one loads


# ---------------------------------------------------------------- the C ABI's refusals (before any device call)
@pytest.fixture(scope="module")
def ctx():
    from pgmi import _native as Nt
    from pgmi import config_dict
    d = config_dict(W.small_config(vision_layers=1, text_layers=1, vocab=64))
    c = Nt.PgmiConfig()
    for k, _ in Nt.PgmiConfig._fields_:
        if k not in ("max_batch", "max_seq", "max_kv"):
            setattr(c, k, d[k])
    c.max_batch, c.max_seq, c.max_kv = 1, 320, 64
    h = ctypes.c_void_p()
    Nt.check(Nt.lib().pgmi_create(0, ctypes.byref(c), ctypes.byref(h)), "pgmi_create")
    yield h
    Nt.lib().pgmi_destroy(h)


def test_abi_refusals(ctx):
    from pgmi import _native as Nt
    L = Nt.lib()
    i = ctypes.c_int(-5)
    assert L.pgmi_lora_create(None, ctypes.byref(i)) == Nt.PGMI_E_ARG
    assert L.pgmi_lora_create(ctx, None) == Nt.PGMI_E_ARG
    assert L.pgmi_lora_create(ctx, ctypes.byref(i)) == 0 and i.value == 0
    assert L.pgmi_lora_active(ctx) == -1 and L.pgmi_lora_active(None) == -1
    A, B = factors()
    sh = lambda *v: (ctypes.c_int64 * 2)(*v)   # noqa: E731
    name = (QP + ".weight").encode()

    def add(id_=0, nm=name, a=A.ctypes.data, b=B.ctypes.data, ash=(8, 2048), bsh=(2048, 8), adt=2, c=ctx):
        return L.pgmi_lora_add(c, id_, nm, a, adt, sh(*ash) if ash else None, b, 2, sh(*bsh) if bsh else None, 2.0, 0,
                               None)
    E = Nt.PGMI_E_ARG
    assert add(c=None) == E and add(nm=None) == E and add(a=None) == E and add(b=None) == E
    assert add(ash=None) == E and add(bsh=None) == E
    assert add(id_=1) == E and add(id_=-1) == E and add(id_=8) == E            # unknown ids
    assert add(adt=7) == E
    assert add(ash=(0, 2048), bsh=(2048, 0)) == E                               # r outside [1, 256]
    assert add(ash=(257, 2048), bsh=(2048, 257)) == E
    assert b"[1, 256]" in L.pgmi_last_error()
    assert add(ash=(8, 2040)) == E and add(bsh=(2047, 8)) == E and add(bsh=(2048, 4)) == E   # shapes
    for bad in ("language_model.model.embed_tokens.weight", "language_model.model.norm.weight",
                "vision_tower.vision_model.embeddings.patch_embedding.weight",
                "vision_tower.vision_model.embeddings.position_embedding.weight",
                "multi_modal_projector.linear.bias", "language_model.model.layers.0.input_layernorm.weight",
                "language_model.model.layers.7.self_attn.q_proj.weight", "no.such.weight"):
        assert add(nm=bad.encode()) == E, bad
    info = (ctypes.c_int64 * 3)()
    assert L.pgmi_lora_info(ctx, 0, info, 3) == 0 and list(info) == [0, 0, 0]   # nothing was added
    assert L.pgmi_lora_info(ctx, 0, info, 2) == E and L.pgmi_lora_info(ctx, 3, info, 3) == E
    assert L.pgmi_lora_info(ctx, 0, None, 3) == E
    assert L.pgmi_lora_set(ctx, 5, None) == E and L.pgmi_lora_set(ctx, -2, None) == E and L.pgmi_lora_set(None, 0, None) == E
    assert L.pgmi_lora_free(ctx, 5) == E and L.pgmi_lora_free(None, 0) == E
    assert L.pgmi_lora_free(ctx, 0) == 0 and L.pgmi_lora_free(ctx, 0) == E       # freed: the id is unknown again
    ids = []
    for _ in range(8):
        assert L.pgmi_lora_create(ctx, ctypes.byref(i)) == 0
        ids.append(i.value)
    assert ids == list(range(8))
    assert L.pgmi_lora_create(ctx, ctypes.byref(i)) == Nt.PGMI_E_STATE           # at most 8 per context
    for k in ids:
        assert L.pgmi_lora_free(ctx, k) == 0
    # the merge entries
    Wb = np.zeros((8, 16), np.uint16)
    a, b, o = np.zeros((2, 16), np.float32), np.zeros((8, 2), np.float32), np.zeros((8, 16), np.uint16)
    mh = L.pgmi_lora_merge_host
    assert mh(None, 8, 16, a.ctypes.data, b.ctypes.data, 2, 1.0, o.ctypes.data) == E
    assert mh(Wb.ctypes.data, 8, 16, a.ctypes.data, b.ctypes.data, 2, 1.0, None) == E
    assert mh(Wb.ctypes.data, 8, 16, a.ctypes.data, b.ctypes.data, 0, 1.0, o.ctypes.data) == E
    assert mh(Wb.ctypes.data, 8, 16, a.ctypes.data, b.ctypes.data, 257, 1.0, o.ctypes.data) == E
    op = L.pgmi_op_lora_merge   # refused before any launch: the pointers are never read
    assert op(ctx, None, 8, 16, 256, 256, 2, 1.0, 256, None) == E
    assert op(None, 256, 8, 16, 256, 256, 2, 1.0, 256, None) == E
    assert op(ctx, 256, 8, 16, 256, 256, 0, 1.0, 256, None) == E and op(ctx, 256, 8, 16, 256, 256, 257, 1.0, 256, None) == E
    assert op(ctx, 256, 8, 20, 256, 256, 2, 1.0, 256, None) == E and op(ctx, 256, 0, 16, 256, 256, 2, 1.0, 256, None) == E
    assert op(ctx, 256, 8, 16, 260, 256, 2, 1.0, 256, None) == E                 # alignment
