"""Binds the drop-in nn.Module trees (modeling_gemma / modeling_siglip) to an Engine.

On the first forward on a GPU the module's parameters are copied into the engine's bf16
weight slab; bf16 parameters are then re-pointed at their slab views, so the model holds one
copy of the weights and later in-place updates (load_state_dict) land in the slab.  A cheap
fingerprint (storage pointers and version counters of a parameter sample, the sampled Parameter
objects kept from the first forward) detects .to(...) and in-place loads and rebuilds the engine;
replacing Parameter objects needs an explicit unbind (pgmi_rebind on the top-level modules).
At every prefill (full_check) the version counters of every parameter the sample cannot vouch for are
checked too: the weights engine.prepare() derives tensors from (the text layers' projections -> the
batched decode's fragment-major images, the patch embedding -> its padded copy) and any parameter that is
not a slab view (its in-place update never reaches the slab).  A change there re-copies those parameters,
drops the pending greedy lookahead and re-runs prepare() (round-6 verdict: an in-place update of an
unsampled weight left the derived images and a pending lookahead stale).
While a LoRA adapter is merged into the slab (Engine.set_lora) the parameters show the merged weights; the library's
merges and restores touch no version counter, so they never come here, and an update seen while one is active is
refused (_refuse_update_under_lora): the model deactivates first.
"""
from __future__ import annotations

import warnings
import weakref

import torch

from .engine import Engine

# capacities of engines built by the Python API (pgmi_config.max_batch / max_seq / max_kv)
DEFAULT_MAX_BATCH = 8
DEFAULT_MAX_SEQ = 1472

_DUMMY_TEXT = {"vocab_size": 8, "hidden_size": 2048, "intermediate_size": 16384, "num_hidden_layers": 0,
               "num_attention_heads": 8, "num_key_value_heads": 1, "head_dim": 256,
               "max_position_embeddings": 64, "rms_norm_eps": 1e-6, "rope_theta": 10000.0}
_DUMMY_VISION = {"hidden_size": 1152, "intermediate_size": 4304, "num_hidden_layers": 0,
                 "num_attention_heads": 16, "num_channels": 3, "image_size": 14, "patch_size": 14,
                 "layer_norm_eps": 1e-6}


def _device_of(module) -> torch.device:
    p = next(module.parameters(), None)
    if p is None or p.device.type != "cuda":
        raise RuntimeError(
            "libpgmi runs the PaliGemma path on an MI355X GPU only (no CPU fallback): move the model to the "
            "GPU with .to('cuda') first")
    return p.device


def _sample(module):
    """Every ~len/16-th parameter object plus the last (the fingerprint's witnesses)."""
    ps = list(module.parameters())
    return ps[:: max(1, len(ps) // 16)] + ps[-1:]


def _fingerprint_of(sample):
    return tuple((p.data_ptr(), p._version, p.dtype) for p in sample)


def _inv_fingerprint(inv_freq):
    return None if inv_freq is None else (inv_freq.data_ptr(), inv_freq._version, inv_freq.dtype)


# parameters engine.prepare() builds derived tensors from (csrc/engine_weights.hip pgmi_prepare): the text layers'
# projections (fragment-major images read by the batched decode) and the patch embedding (its padded copy)
_DERIVED = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
            "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")


def _watched(name: str, p, view) -> bool:
    """Checked at every prefill: a source of a derived tensor, or a parameter that is not a slab view."""
    if p.data_ptr() != view.data_ptr():
        return True
    if "patch_embedding.weight" in name:
        return True
    return "language_model.model.layers." in name and name.endswith(_DERIVED)


def _versions(watch):
    return [(p.data_ptr(), p._version) for p, _ in watch]


class _Bound:
    def __init__(self, engine, sample, inv_fp, watch):
        self.engine, self.sample, self.fp, self.inv_fp = engine, sample, _fingerprint_of(sample), inv_fp
        self.watch = watch  # [(parameter, slab view)] checked at every prefill
        self.wfp = _versions(watch)

    def refresh(self, inv_freq) -> None:
        """An in-place update of a watched parameter: copy what is not a slab view, drop the pending greedy
        lookahead (its logits came from the old weights), rebuild the derived tensors."""
        eng = self.engine
        _refuse_update_under_lora(eng)
        with torch.no_grad():
            for p, view in self.watch:
                if p.data_ptr() != view.data_ptr():
                    view.copy_(p.detach())
        la = eng.__dict__.get("_lookahead")
        if la is not None:
            la.pending = None
        eng.prepare(inv_freq=inv_freq)  # synchronises the device: a lookahead still running ends first
        self.wfp = _versions(self.watch)
        self.fp = _fingerprint_of(self.sample)


def _refuse_update_under_lora(eng) -> None:
    """A parameter changed in place (or moved) while a LoRA adapter is merged into the slab the parameters view:
    the update landed on merged weights, and the pristine copies no longer match any base.  (The library's own
    merges and restores write the slab without touching torch's version counters, so they never come here.)"""
    if eng.active_lora is not None:
        raise RuntimeError(
            f"a model weight was updated in place while the LoRA adapter {eng.active_lora!r} is active: the parameters "
            f"hold the merged weights.  Call pgmi_set_lora(None) before changing weights, then re-activate")


_warned_dtypes = set()


def bind(module, cfg: dict, prefix: str, inv_freq=None, full_check: bool = False) -> Engine:
    """Engine for `module` (parameters named prefix + local name in the slab).

    The binding is re-checked on every forward against a fingerprint of sampled parameters
    (storage pointer, in-place version, dtype): an in-place update (load_state_dict, copy_) re-binds.
    The sampled parameter objects are kept, so the check costs ~17 attribute reads instead of a
    walk of the module tree (~0.4-0.8 ms per decode step at the 3B shapes); replacing Parameter
    objects after the first forward needs unbind(module) (PaliGemmaForConditionalGeneration.pgmi_rebind).
    full_check (prefills): also compare the watched parameters' versions (module docstring), ~130 of them
    at the 3B shapes (~15 us).
    `cfg` may be a callable returning the config dict (built only when an engine is built).  A bound
    module's device is its sampled parameters' (a move to another device re-points them: the
    fingerprint changes), so the per-forward check walks no module tree."""
    b = module.__dict__.get("_pgmi_bound")
    inv_fp = _inv_fingerprint(inv_freq)
    if b is not None and b.fp == _fingerprint_of(b.sample) and b.sample[0].device == b.engine.device:
        if b.inv_fp != inv_fp:
            # the rotary inv_freq buffer changed (e.g. model.to(dtype) casts it, as the ablation's
            # run_inference does, ablation_study_fixed.py:182): rebuild the RoPE table from its values
            b.engine.prepare(inv_freq=inv_freq)
            b.inv_fp = inv_fp
        if full_check and _versions(b.watch) != b.wfp:
            b.refresh(inv_freq)
        return b.engine
    if b is not None:
        _refuse_update_under_lora(b.engine)
    dev = _device_of(module)
    if callable(cfg):
        cfg = cfg()
    eng = Engine(cfg, device=dev, max_batch=DEFAULT_MAX_BATCH, max_seq=DEFAULT_MAX_SEQ)
    watch = []
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.is_floating_point() and p.dtype != torch.bfloat16 and p.dtype not in _warned_dtypes:
                _warned_dtypes.add(p.dtype)
                warnings.warn(f"libpgmi computes in bf16: {p.dtype} parameters are rounded to bf16 "
                              f"(the reference's fp16 default, utils.py / ablation_study_fixed.py:330, is not "
                              f"reproduced)", stacklevel=3)
            full = prefix + name
            view = eng.views.get(full)
            if view is None:
                continue  # e.g. the tied lm_head (modeling_gemma.py:396-397)
            if tuple(p.shape) != tuple(view.shape):
                raise ValueError(f"{full}: shape {tuple(p.shape)} != {tuple(view.shape)}")
            view.copy_(p.detach())
            if p.dtype == torch.bfloat16 and p.device == dev:
                p.data = view
            if _watched(full, p, view):
                watch.append((p, view))
    eng.prepare(inv_freq=inv_freq)
    module.__dict__["_pgmi_bound"] = _Bound(eng, _sample(module), inv_fp, watch)
    return eng


def unbind(module):
    """Drop the engine binding: the next forward copies the (replaced) parameters into a new slab."""
    module.__dict__.pop("_pgmi_bound", None)


def set_owner(child, owner):
    """Let a submodule (vision tower, language model) run on its parent's engine."""
    child.__dict__["_pgmi_owner"] = weakref.ref(owner)


def owner_of(child):
    r = child.__dict__.get("_pgmi_owner")
    return r() if r is not None else None


def vision_cfg(vc) -> dict:
    v = {k: getattr(vc, k) for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                     "num_channels", "image_size", "patch_size", "layer_norm_eps")}
    return {"vision_config": v, "text_config": dict(_DUMMY_TEXT), "image_token_index": 7, "projection_dim": 2048,
            "pad_token_id": None}


def text_cfg(tc) -> dict:
    t = {k: getattr(tc, k) for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                     "num_attention_heads", "num_key_value_heads", "head_dim",
                                     "max_position_embeddings", "rms_norm_eps", "rope_theta")}
    return {"vision_config": dict(_DUMMY_VISION), "text_config": t, "image_token_index": -7,
            "projection_dim": 2048, "pad_token_id": getattr(tc, "pad_token_id", None)}


def vision_forward(transformer, pixel_values, prefix="vision_tower.vision_model."):
    """SiglipVisionTransformer.forward (modeling_siglip.py:236-244) through pgmi_vision."""
    owner = owner_of(transformer)
    if owner is not None:
        eng = owner._pgmi_engine(full_check=True)  # the tower reads the padded patch matrix (a derived tensor)
    else:
        eng = bind(transformer, vision_cfg(transformer.config), prefix, full_check=True)
    px = pixel_values
    if px.dtype not in (torch.float32, torch.bfloat16):
        px = px.float()
    return eng.vision(px)
