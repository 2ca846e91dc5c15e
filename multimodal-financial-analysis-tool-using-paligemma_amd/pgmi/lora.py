"""LoRA adapters: reading a peft checkpoint, and the merge rule stated in numpy (csrc/lora.h is the host and
device form).

What the reference's fine-tuning workflow leaves behind (a peft LoraConfig on q_proj / k_proj / v_proj) is an
adapter directory: adapter_config.json + adapter_model.safetensors.  read_peft turns one into the factors the
engine merges; Engine.load_lora / set_lora (pgmi/engine.py) do the rest on the device.

The rule, for a target W[N][K] (bf16, the pristine base), A[r][K], B[N][r] and a scale s, all fp32:

    acc = 0;  for j = 0 .. r-1:  acc = acc + (B[n][j] * A[j][k])     (fp32 multiply, then fp32 add: not fused)
    W'[n][k] = bf16_rne(fp32(W[n][k]) + acc * s)

It is not peft's bf16 merge() (which rounds B.A and the scaled delta to bf16 first): one rounding, from the base."""
from __future__ import annotations

import json
import math
import os
import re
import struct
from typing import Dict, NamedTuple, Tuple

import numpy as np

MAX_RANK = 256
# the Linear modules of the model: their 2-D weights are the only targets (csrc/engine_lora.hip lora_targetable)
LINEAR_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "out_proj", "gate_proj", "up_proj", "down_proj",
                  "mlp.fc1", "mlp.fc2", "multi_modal_projector.linear")

_KEY = re.compile(r"^base_model\.model\.(?P<module>.+)\.(?P<which>lora_[AB])(?:\.(?P<adapter>[^.]+))?\.weight$")


class Adapter(NamedTuple):
    """targets: slab weight name -> (A fp32 [r][K], B fp32 [N][r], scaling np.float32); config: the parsed
    adapter_config.json (empty for adapters built in memory)."""
    targets: Dict[str, Tuple[np.ndarray, np.ndarray, np.float32]]
    config: dict


def scaling_of(lora_alpha, r: int, use_rslora: bool = False) -> np.float32:
    """lora_alpha / r, or lora_alpha / sqrt(r) with rslora: computed in float64, rounded to fp32 once."""
    return np.float32(float(lora_alpha) / (math.sqrt(r) if use_rslora else float(r)))


def bf16_rne_np(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns, round to nearest even; a NaN becomes the quiet NaN of its sign (lora.h)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def merge_np(W: np.ndarray, A: np.ndarray, B: np.ndarray, scaling) -> np.ndarray:
    """The merge rule on bf16 bit patterns W (uint16 [N][K]); returns uint16 [N][K]."""
    W = np.asarray(W, np.uint16)
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    (N, K), r = W.shape, A.shape[0]
    if A.shape != (r, K) or B.shape != (N, r):
        raise ValueError(f"merge_np: W {W.shape} needs A (r, {K}) and B ({N}, r), got {A.shape} and {B.shape}")
    out = np.empty((N, K), np.uint16)
    rows = max(1, (1 << 17) // K)  # row blocks that stay in cache; every element's own order is the rule's
    acc = np.empty((rows, K), np.float32)
    tmp = np.empty((rows, K), np.float32)
    s = np.float32(scaling)
    with np.errstate(over="ignore", invalid="ignore"):
        for n0 in range(0, N, rows):
            n = min(rows, N - n0)
            a, t = acc[:n], tmp[:n]
            a.fill(0.0)
            for j in range(r):
                np.multiply(B[n0:n0 + n, j:j + 1], A[j:j + 1, :], out=t)
                np.add(a, t, out=a)
            np.multiply(a, s, out=t)
            base = (W[n0:n0 + n].astype(np.uint32) << 16).view(np.float32)
            out[n0:n0 + n] = bf16_rne_np(base + t)
    return out


def _check_config(cfg: dict) -> None:
    if cfg.get("use_dora"):
        raise ValueError("adapter_config.json: use_dora is set; DoRA adapters are not supported")
    if cfg.get("bias", "none") != "none":
        raise ValueError(f"adapter_config.json: bias = {cfg['bias']!r}; only bias = 'none' is supported")
    if cfg.get("fan_in_fan_out"):
        raise ValueError("adapter_config.json: fan_in_fan_out is set; transposed targets are not supported")
    if cfg.get("alpha_pattern"):
        raise ValueError("adapter_config.json: a non-empty alpha_pattern is not supported")
    if "lora_alpha" not in cfg:
        raise ValueError("adapter_config.json: lora_alpha is missing")


def _read_tensors(path: str) -> Dict[str, np.ndarray]:
    """Every tensor of a safetensors file as fp32 (BF16 / F16 / F32 widen exactly): through the safetensors
    library when it is importable, else through libpgmi's header reader."""
    try:
        from safetensors import safe_open
    except ImportError:
        safe_open = None
    out = {}
    if safe_open is not None:
        import torch
        with safe_open(path, framework="pt", device="cpu") as f:
            for k in f.keys():
                t = f.get_tensor(k)
                if t.dtype not in (torch.bfloat16, torch.float16, torch.float32):
                    raise ValueError(f"{k}: dtype {t.dtype} is not BF16 / F16 / F32")
                out[k] = t.float().numpy()
        return out
    from . import _native as N
    with open(path, "rb") as fh:
        data0 = 8 + struct.unpack("<Q", fh.read(8))[0]
        for name, dt, shape, b, e in N.safetensors_index(path):
            if dt not in (N.DTYPE_BF16, N.DTYPE_F16, N.DTYPE_F32):
                raise ValueError(f"{name}: dtype is not BF16 / F16 / F32")
            fh.seek(data0 + b)
            raw = fh.read(e - b)
            if dt == N.DTYPE_F32:
                v = np.frombuffer(raw, np.float32).copy()
            elif dt == N.DTYPE_F16:
                v = np.frombuffer(raw, np.float16).astype(np.float32)
            else:
                v = (np.frombuffer(raw, np.uint16).astype(np.uint32) << 16).view(np.float32)
            out[name] = v.reshape(shape)
    return out


def check_target_name(weight_name: str, key: str = "") -> None:
    if not weight_name.endswith(tuple(m + ".weight" for m in LINEAR_MODULES)):
        raise ValueError(f"{key or weight_name}: {weight_name} is not the weight of a Linear module "
                         f"(embeddings, the patch convolution, norms and biases are not LoRA targets)")


def read_peft(path: str) -> Adapter:
    """A peft LoRA checkpoint -- a directory with adapter_config.json and adapter_model.safetensors, or the
    safetensors file itself with the config beside it -- as an Adapter.  Keys
    base_model.model.<module>.lora_A.weight (or .lora_A.<adapter_name>.weight) map to the slab weight
    <module>.weight; each target's scaling is lora_alpha / r (/ sqrt(r) with use_rslora), r from its shapes.
    ValueError, naming the field or key: use_dora, bias != "none", fan_in_fan_out, a non-empty alpha_pattern,
    lora_embedding_* keys, any tensor that is neither lora_A nor lora_B, an A without its B (or the reverse),
    mismatched ranks, a rank outside [1, 256], a target that is not a Linear weight."""
    path = os.fspath(path)
    if os.path.isdir(path):
        cfg_path, st_path = os.path.join(path, "adapter_config.json"), os.path.join(path, "adapter_model.safetensors")
    else:
        cfg_path, st_path = os.path.join(os.path.dirname(path), "adapter_config.json"), path
    with open(cfg_path) as f:
        cfg = json.load(f)
    _check_config(cfg)
    halves: Dict[str, dict] = {}
    for key, t in _read_tensors(st_path).items():
        if "lora_embedding_" in key:
            raise ValueError(f"{key}: lora_embedding_* (LoRA on an embedding) is not supported")
        m = _KEY.match(key)
        if m is None:
            raise ValueError(f"{key}: neither a lora_A nor a lora_B tensor of base_model.model.<module>")
        name = m.group("module") + ".weight"
        check_target_name(name, key)
        if t.ndim != 2:
            raise ValueError(f"{key}: a LoRA factor is 2-D, got shape {tuple(t.shape)}")
        if m.group("which") in halves.setdefault(name, {}):
            raise ValueError(f"{key}: a second {m.group('which')} for {name} (several adapters in one file)")
        halves[name][m.group("which")] = (key, np.ascontiguousarray(t, np.float32))
    targets = {}
    for name, h in halves.items():
        if "lora_A" not in h or "lora_B" not in h:
            have = h.get("lora_A", h.get("lora_B"))[0]
            raise ValueError(f"{have}: {name} has a {'lora_A' if 'lora_A' in h else 'lora_B'} without its "
                             f"{'lora_B' if 'lora_A' in h else 'lora_A'}")
        (ka, A), (kb, B) = h["lora_A"], h["lora_B"]
        r = A.shape[0]
        if B.shape[1] != r:
            raise ValueError(f"{kb}: mismatched ranks, lora_A has r = {r} and lora_B r = {B.shape[1]}")
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"{ka}: rank {r} outside [1, {MAX_RANK}]")
        targets[name] = (A, B, scaling_of(cfg["lora_alpha"], r, bool(cfg.get("use_rslora"))))
    return Adapter(targets, cfg)
