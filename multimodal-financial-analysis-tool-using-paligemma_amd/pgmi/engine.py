"""Engine: one libpgmi context on one GPU (weights slab, KV slabs, forward calls).

Device memory for the weights and the KV caches is torch-allocated (so the Python API can
expose the reference's parameter / cache tensors as views of it); the library owns its
workspaces.  Every compute call goes through libpgmi.so -- nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native as N
from . import prefix_np as PX
from . import ragged as R


def config_dict(cfg) -> dict:
    """Accept a PaliGemmaConfig (reference or drop-in) or an HF-style config.json dict."""
    if isinstance(cfg, dict):
        v, t = dict(cfg["vision_config"]), dict(cfg["text_config"])
        top = cfg
        get = top.get
    else:
        v = dict(vars(cfg.vision_config))
        t = dict(vars(cfg.text_config))
        top = vars(cfg)
        get = top.get
    pad = get("pad_token_id", None)
    return {
        "v_hidden": v.get("hidden_size", 768), "v_intermediate": v.get("intermediate_size", 3072),
        "v_layers": v.get("num_hidden_layers", 12), "v_heads": v.get("num_attention_heads", 12),
        "v_channels": v.get("num_channels", 3), "v_image": v.get("image_size", 224),
        "v_patch": v.get("patch_size", 16), "v_ln_eps": v.get("layer_norm_eps", 1e-6),
        "t_vocab": t["vocab_size"], "t_hidden": t["hidden_size"], "t_intermediate": t["intermediate_size"],
        "t_layers": t["num_hidden_layers"], "t_heads": t["num_attention_heads"],
        "t_kv_heads": t["num_key_value_heads"], "t_head_dim": t.get("head_dim", 256),
        "t_max_pos": t.get("max_position_embeddings", 8192), "t_rms_eps": t.get("rms_norm_eps", 1e-6),
        "t_rope_theta": t.get("rope_theta", 10000.0),
        "projection_dim": get("projection_dim", 2048), "image_token_index": get("image_token_index", 256000),
        "pad_token_id": -1 if pad is None else int(pad),
        "hidden_size": get("hidden_size", 2048),
    }


_KEEP = object()  # generate / score: no `adapter` argument -- whatever adapter is active stays


class Score(NamedTuple):
    """Engine.score's result: per-token log-probabilities (0 where ignored), each row's sum and live-token count,
    and the reference's loss (modeling_gemma.py:596-603)."""
    logprobs: torch.Tensor
    sums: torch.Tensor
    counts: torch.Tensor
    loss: torch.Tensor


class CandidateScores(NamedTuple):
    """Engine.score_candidates' result: each candidate's summed log-probability and token count, and its per-token
    log-probabilities (a list of 1-D tensors, one per candidate)."""
    sums: torch.Tensor
    counts: torch.Tensor
    logprobs: list


class Engine:
    # generate(): greedy steps per hipGraph launch (pgmi_decode_steps) for batches of GEN_MIN_BATCH rows or more.
    # Same box (tools/probes/multistep_probe.py): B = 8 step 1.279 -> 1.271 ms at 8-16 steps per launch, B = 1
    # 1.056 -> 1.060 ms (slower: B <= 2 keeps one launch per step)
    GEN_CHUNK = 8
    GEN_MIN_BATCH = 3

    # max_batch: sequences / images per call, 1..16 (16 rows fill the batched decode projections' MFMA tile: a B = 16
    # step costs 5 % more than a B = 8 one, tools/probes/batch16_probe.py); the default stays 8
    def __init__(self, cfg, device=None, max_batch: int = 8, max_seq: int = 1472, max_kv: Optional[int] = None):
        self.lib = N.lib()
        self.cfgd = config_dict(cfg)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        c = N.PgmiConfig()
        for k, _ in N.PgmiConfig._fields_:
            if k in ("max_batch", "max_seq", "max_kv"):
                continue
            setattr(c, k, self.cfgd[k])
        c.max_batch, c.max_seq = max_batch, max_seq
        c.max_kv = max_kv if max_kv else self.cfgd["t_max_pos"]
        self.max_batch, self.max_seq, self.max_kv = max_batch, max_seq, c.max_kv
        h = ctypes.c_void_p()
        N.check(self.lib.pgmi_create(self.device.index, ctypes.byref(c), ctypes.byref(h)), "pgmi_create")
        self.ctx = h
        nbytes = self.lib.pgmi_weights_bytes(self.ctx)
        self.slab = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        N.check(self.lib.pgmi_bind_weights(self.ctx, self.slab.data_ptr()), "pgmi_bind_weights")
        self.views = {}
        for i in range(self.lib.pgmi_weight_count(self.ctx)):
            name, off, shape, nd = ctypes.c_char_p(), ctypes.c_int64(), (ctypes.c_int64 * 4)(), ctypes.c_int()
            N.check(self.lib.pgmi_weight_info(self.ctx, i, ctypes.byref(name), ctypes.byref(off),
                                              ctypes.byref(shape), ctypes.byref(nd)))
            shp = tuple(shape[j] for j in range(nd.value))
            numel = math.prod(shp)
            self.views[name.value.decode()] = self.slab[off.value: off.value + 2 * numel].view(torch.bfloat16).view(shp)
        self.prepared = False
        self._logits_buf = {}
        self._gen_buf = {}  # generate(): per-batch-size step buffers
        self._lora = {}  # LoRA adapters: name -> id in the context (load_lora)
        self._lora_active = None  # the one merged into the slab now

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                # a greedy lookahead step (pgmi/lookahead.py) may still run on its side stream in this context's
                # workspace: it ends before the context's memory is released
                la = self.__dict__.get("_lookahead")
                if la is not None and la.last is not None:
                    la.last.synchronize()
                self.lib.pgmi_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def names(self):
        return list(self.views.keys())

    @torch.no_grad()
    def load_state_dict(self, sd: dict, strict: bool = True):
        self._no_lora("load_state_dict")
        missing = [n for n in self.views if n not in sd]
        if strict and missing:
            raise KeyError(f"missing weights: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for n, view in self.views.items():
            if n in sd:
                t = sd[n]
                if tuple(t.shape) != tuple(view.shape):
                    raise ValueError(f"{n}: shape {tuple(t.shape)} != {tuple(view.shape)}")
                view.copy_(t.to(device=self.device, dtype=torch.bfloat16))
        self.prepared = False

    def load_safetensors(self, path: str, strict: bool = True) -> int:
        """Native safetensors loading into the slab (pgmi_load_safetensors).
        `path` is a *.safetensors file or a directory of shards.  With strict, every slab weight
        must come from the files.  Returns the number of tensors loaded."""
        import glob
        import os
        self._no_lora("load_safetensors")
        files = sorted(glob.glob(os.path.join(path, "*.safetensors"))) if os.path.isdir(path) else [path]
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {path}")
        s = N.stream_handle(self.device)
        got = set()
        total = 0
        for f in files:
            nl, ns = ctypes.c_int(), ctypes.c_int()
            N.check(self.lib.pgmi_load_safetensors(self.ctx, f.encode(), ctypes.byref(nl), ctypes.byref(ns), s), f)
            total += nl.value
            got.update(e[0] for e in N.safetensors_index(f) if e[0] in self.views)
        missing = [n for n in self.views if n not in got]
        if strict and missing:
            raise KeyError(f"{len(missing)} weights missing from {path}: {missing[:4]}")
        self.prepared = False
        return total

    # ------------------------------------------------------------------ LoRA adapters
    def _no_lora(self, what: str) -> None:
        if self._lora_active is not None:
            raise RuntimeError(f"{what}: the LoRA adapter {self._lora_active!r} is merged into the weights; "
                               f"deactivate first (set_lora(None))")

    def load_lora(self, source, name: str) -> None:
        """Load a LoRA adapter under `name`: a peft directory / adapter_model.safetensors path (pgmi.lora.read_peft),
        a pgmi.lora.Adapter, or a dict slab weight name -> (A [r][K], B [N][r], scaling).  The factors go to the
        device as fp32 (pgmi_lora_add); nothing is merged until set_lora(name).  At most 8 adapters per engine."""
        import numpy as np
        from . import lora as LR
        if name is None or name in self._lora:
            raise ValueError(f"load_lora: adapter name {name!r} is " + ("taken" if name is not None else "required"))
        if isinstance(source, dict):
            targets = source
        elif isinstance(source, LR.Adapter):
            targets = source.targets
        else:
            targets = LR.read_peft(source).targets
        if not targets:
            raise ValueError("load_lora: the adapter has no targets")
        i = ctypes.c_int()
        N.check(self.lib.pgmi_lora_create(self.ctx, ctypes.byref(i)), "pgmi_lora_create")
        try:
            s = N.stream_handle(self.device)
            for wname, (A, B, scaling) in targets.items():
                A = np.ascontiguousarray(A.detach().float().cpu().numpy() if torch.is_tensor(A) else A, np.float32)
                B = np.ascontiguousarray(B.detach().float().cpu().numpy() if torch.is_tensor(B) else B, np.float32)
                if A.ndim != 2 or B.ndim != 2:
                    raise ValueError(f"{wname}: LoRA factors are 2-D")
                N.check(self.lib.pgmi_lora_add(self.ctx, i.value, wname.encode(), A.ctypes.data, N.DTYPE_F32,
                                               (ctypes.c_int64 * 2)(*A.shape), B.ctypes.data, N.DTYPE_F32,
                                               (ctypes.c_int64 * 2)(*B.shape), float(np.float32(scaling)), 0, s),
                        "pgmi_lora_add")
        except Exception:
            self.lib.pgmi_lora_free(self.ctx, i.value)
            raise
        self._lora[name] = i.value

    def set_lora(self, name: Optional[str]) -> None:
        """Merge the adapter `name` into the weight slab (None: back to the base model, bit for bit); the adapter
        active before is taken out first (pgmi_lora_set: synchronises the device).  Every later call -- prefill,
        decode, replayed graphs -- computes with the merged weights at no extra cost per token."""
        if name is not None and name not in self._lora:
            raise KeyError(f"set_lora: no adapter named {name!r} (loaded: {sorted(self._lora)})")
        if name == self._lora_active:
            return
        if self._lora_active is None and not self.prepared:
            self.prepare()  # the base was written since: the pristine copies are taken from it anew
        la = self.__dict__.get("_lookahead")
        if la is not None:  # a pending greedy lookahead's logits came from the outgoing weights
            la.pending = None
        N.check(self.lib.pgmi_lora_set(self.ctx, -1 if name is None else self._lora[name], self._s()), "pgmi_lora_set")
        self._lora_active = name

    @property
    def active_lora(self) -> Optional[str]:
        return self._lora_active

    def lora_info(self, name: str) -> dict:
        """targets, factor_bytes (resident fp32 factors) and pristine_bytes (base copies of its targets held now)."""
        v = (ctypes.c_int64 * 3)()
        N.check(self.lib.pgmi_lora_info(self.ctx, self._lora[name], v, 3), "pgmi_lora_info")
        return {"targets": v[0], "factor_bytes": v[1], "pristine_bytes": v[2]}

    def unload_lora(self, name: str) -> None:
        """Free an adapter's device memory; the active one must be deactivated first."""
        if name == self._lora_active:
            self._no_lora("unload_lora")
        N.check(self.lib.pgmi_lora_free(self.ctx, self._lora[name]), "pgmi_lora_free")
        del self._lora[name]

    def fill_synthetic(self, seed: int, policy):
        """Device-side deterministic init (oracle/wgen.c recipe); policy(name, shape) -> (scale, offset)."""
        self._no_lora("fill_synthetic")
        s = N.stream_handle(self.device)
        for n, view in self.views.items():
            scale, offset = policy(n, tuple(view.shape))
            key = self.lib.pgmi_synthetic_key(n.encode(), seed)
            N.check(self.lib.pgmi_fill_synthetic(self.ctx, n.encode(), key, scale, offset, s), n)
        self.prepared = False

    def prepare(self, inv_freq: Optional[torch.Tensor] = None, exact_table: bool = True):
        """RoPE tables from the module's inv_freq buffer (the reference's own values) and the
        padded patch matrix.  With exact_table the cos/sin table is computed by torch on the
        CPU exactly as GemmaRotaryEmbedding.forward does (modeling_gemma.py:168-185)."""
        hd, mp = self.cfgd["t_head_dim"], self.cfgd["t_max_pos"]
        if inv_freq is None:
            inv_freq = 1.0 / (self.cfgd["t_rope_theta"] ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
        inv = inv_freq.detach().float().cpu().contiguous()
        N.check(self.lib.pgmi_set_rope_inv_freq(self.ctx, inv.numpy().ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        if exact_table:
            pos = torch.arange(mp, dtype=torch.float32)
            freqs = (inv[None, :, None] @ pos[None, None, :]).transpose(1, 2)[0]  # (mp, hd/2) as :178
            cos = freqs.cos().to(torch.bfloat16).contiguous().view(torch.int16)
            sin = freqs.sin().to(torch.bfloat16).contiguous().view(torch.int16)
            N.check(self.lib.pgmi_set_rope_table(self.ctx, cos.data_ptr(), sin.data_ptr(), mp))
        N.check(self.lib.pgmi_prepare(self.ctx), "pgmi_prepare")
        self.prepared = True

    # ------------------------------------------------------------------ caches
    def new_kv(self, batch: int, max_tokens: Optional[int] = None) -> torch.Tensor:
        T = max_tokens or self.max_kv
        t = self.cfgd
        return torch.empty((t["t_layers"], 2, batch, T, t["t_kv_heads"] * t["t_head_dim"]),
                           dtype=torch.bfloat16, device=self.device)

    def scratch_kv(self, batch: int, tokens: int) -> torch.Tensor:
        """Cache for calls without a KVCache (kv_cache=None: the no-KV ablation mode)."""
        cur = getattr(self, "_scratch_kv", None)
        if cur is None or cur.shape[2] < batch or cur.shape[3] < tokens:
            cur = self.new_kv(max(batch, cur.shape[2] if cur is not None else 0),
                              max(tokens, cur.shape[3] if cur is not None else 0))
            self._scratch_kv = cur
        if cur.shape[2] != batch:
            return self.new_kv(batch, tokens)
        return cur

    def logits_buffer(self, batch: int) -> torch.Tensor:
        """Persistent decode logits buffer (a stable pointer lets the decode hipGraph be reused)."""
        buf = self._logits_buf.get(batch)
        if buf is None:
            buf = torch.empty((batch, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
            self._logits_buf[batch] = buf
        return buf

    # ------------------------------------------------------------------ forward pieces
    _stream_guard = None  # pgmi/lookahead.py: makes a call wait for a step still running on its side stream

    def _s(self):
        h = N.stream_handle(self.device)
        if self._stream_guard is not None:
            self._stream_guard(h)
        return h

    def _ready(self):
        if not self.prepared:
            self.prepare()

    def vision(self, pixel_values: torch.Tensor) -> torch.Tensor:
        self._ready()
        px = pixel_values.to(self.device)
        if px.dtype not in (torch.float32, torch.bfloat16):
            px = px.float()
        px = px.contiguous()
        B = px.shape[0]
        c = self.cfgd
        n = (c["v_image"] // c["v_patch"]) ** 2
        if tuple(px.shape[1:]) != (c["v_channels"], c["v_image"], c["v_image"]):
            raise ValueError(f"pixel_values shape {tuple(px.shape)} does not match the vision config")
        out = torch.empty((B, n, c["v_hidden"]), dtype=torch.bfloat16, device=self.device)
        dt = N.DTYPE_F32 if px.dtype == torch.float32 else N.DTYPE_BF16
        N.check(self.lib.pgmi_vision(self.ctx, px.data_ptr(), dt, B, out.data_ptr(), self._s()), "pgmi_vision")
        return out

    def preprocess(self, images, size: Optional[int] = None) -> torch.Tensor:
        """process_images (processing_paligemma.py:31-50) on the GPU: PIL-exact BICUBIC resize
        of each decoded RGB image (PIL image or uint8 HWC array), x/255, (x-0.5)/0.5, CHW.
        Returns pixel_values (B, 3, size, size) float32 on the device."""
        import numpy as np
        S = int(size or self.cfgd["v_image"])
        out = torch.empty((len(images), 3, S, S), dtype=torch.float32, device=self.device)
        for i, im in enumerate(images):
            arr = np.asarray(im.convert("RGB") if hasattr(im, "convert") else im, dtype=np.uint8)
            if arr.ndim != 3 or arr.shape[2] != 3:
                raise ValueError(f"expected an RGB image (H, W, 3), got {arr.shape}")
            src = torch.from_numpy(np.array(arr, dtype=np.uint8, order="C")).to(self.device)
            N.check(self.lib.pgmi_preprocess(self.ctx, src.data_ptr(), arr.shape[0], arr.shape[1], S, S,
                                             out[i].data_ptr(), self._s()), "pgmi_preprocess")
        return out

    def project(self, feats: torch.Tensor) -> torch.Tensor:
        self._ready()
        f = feats.to(self.device, torch.bfloat16).contiguous()
        rows = f.numel() // f.shape[-1]
        out = torch.empty(f.shape[:-1] + (self.cfgd["projection_dim"],), dtype=torch.bfloat16, device=self.device)
        N.check(self.lib.pgmi_project(self.ctx, f.data_ptr(), rows, out.data_ptr(), self._s()), "pgmi_project")
        return out

    def embed(self, ids: torch.Tensor) -> torch.Tensor:
        self._ready()
        i = ids.to(self.device, torch.int64).contiguous()
        out = torch.empty(tuple(i.shape) + (self.cfgd["t_hidden"],), dtype=torch.bfloat16, device=self.device)
        # (a plain lookup into a fresh tensor: no engine workspace, so no wait for a lookahead in flight)
        N.check(self.lib.pgmi_embed(self.ctx, i.data_ptr(), i.numel(), out.data_ptr(), N.stream_handle(self.device)),
                "pgmi_embed")
        return out

    def lm_forward(self, kv: torch.Tensor, kv_start: int, positions, ids=None, image_feats=None, embeds=None,
                   logits_rows: int = 0, lens=None, prefix_lens=None) -> torch.Tensor:
        """GemmaForCausalLM.forward over merged embeddings (see pgmi.h).  Returns fp32 logits
        (B, L, V) (logits_rows 0) or (B, 1, V): logits_rows 1 keeps every row's final hidden state
        for final_hidden / lazy all-row logits; 2 needs only the last row's, so the last layer's
        post-attention work runs for the last row alone (the KV cache is written for every row).

        lens (B ints, optional): a ragged batch -- row b's tokens are ids[b, :lens[b]], the rest of the
        row is right padding (pgmi_lm_forward_ragged): each row attends its own real tokens only, pad
        ids are never looked up, and logits_rows 1 / 2 return each row's logits at token lens[b] - 1.

        prefix_lens (B ints, optional): the prefix-LM form (pgmi_lm_forward_prefix; the rule is pgmi.prefix_np's).
        Token j of row b attends keys [0, kv_start + max(prefix_lens[b], j + 1)): its prefix from everywhere, the
        tokens after it causally.  Positions stay the caller's (prefix_np.prefix_positions for the reference's
        gap).  Token ids only; the call is eager (no prefill graph is looked up, captured or replayed)."""
        self._ready()
        if prefix_lens is not None and embeds is not None:
            raise ValueError("lm_forward: the prefix form (prefix_lens) takes token ids, not embeds")
        if lens is not None and embeds is not None:
            raise ValueError("lm_forward: a ragged batch (lens) takes token ids, not embeds")
        if embeds is not None:
            e = embeds.to(self.device, torch.bfloat16).contiguous()
            B, L = e.shape[0], e.shape[1]
            idp, imgp, nimg = None, None, 0
        else:
            ids = ids.to(self.device, torch.int64).contiguous()
            B, L = ids.shape
            e = None
            idp = ids.data_ptr()
            if image_feats is not None:
                image_feats = image_feats.to(self.device, torch.bfloat16).contiguous()
                imgp, nimg = image_feats.data_ptr(), image_feats.numel() // image_feats.shape[-1]
            else:
                imgp, nimg = None, 0
        pos = torch.as_tensor(positions, dtype=torch.int64).cpu()
        pos = torch.broadcast_to(pos.reshape(pos.shape[0] if pos.dim() > 1 else 1, -1), (B, L)).contiguous()
        V = self.cfgd["t_vocab"]
        out = torch.empty((B, L if logits_rows == 0 else 1, V), dtype=torch.float32, device=self.device)
        ln = None
        if lens is not None:
            ln = torch.as_tensor(lens).detach().to("cpu", torch.int32).reshape(-1).contiguous()
            if ln.numel() != B:
                raise ValueError(f"lens has {ln.numel()} entries for a batch of {B}")
        if prefix_lens is not None:
            pl = torch.as_tensor(prefix_lens).detach().to("cpu", torch.int32).reshape(-1).contiguous()
            if pl.numel() != B:
                raise ValueError(f"prefix_lens has {pl.numel()} entries for a batch of {B}")
            N.check(self.lib.pgmi_lm_forward_prefix(self.ctx, idp, imgp, nimg, B, L, pos.data_ptr(), N.ptr(ln),
                                                    pl.data_ptr(), kv.data_ptr(), kv.shape[2], kv.shape[3], kv_start,
                                                    out.data_ptr(), logits_rows, self._s()),
                    "pgmi_lm_forward_prefix")
            return out
        if ln is not None:
            N.check(self.lib.pgmi_lm_forward_ragged(self.ctx, idp, imgp, nimg, None, B, L, pos.data_ptr(),
                                                    ln.data_ptr(), kv.data_ptr(), kv.shape[2], kv.shape[3], kv_start,
                                                    out.data_ptr(), logits_rows, self._s()),
                    "pgmi_lm_forward_ragged")
            return out
        N.check(self.lib.pgmi_lm_forward(self.ctx, idp, imgp, nimg, N.ptr(e), B, L, pos.data_ptr(), kv.data_ptr(),
                                         kv.shape[2], kv.shape[3], kv_start, out.data_ptr(), logits_rows, self._s()),
                "pgmi_lm_forward")
        return out

    def final_hidden(self, rows: int) -> torch.Tensor:
        """The final RMSNorm output of the last lm_forward's rows (B*L, hidden) bf16 (a copy)."""
        out = torch.empty((rows, self.cfgd["t_hidden"]), dtype=torch.bfloat16, device=self.device)
        N.check(self.lib.pgmi_lm_final_hidden(self.ctx, out.data_ptr(), rows, self._s()), "pgmi_lm_final_hidden")
        return out

    def lm_head(self, normed: torch.Tensor) -> torch.Tensor:
        """lm_head + .float() (modeling_gemma.py:417-418) over final-normed rows -> (rows, V) fp32."""
        self._ready()
        x = normed.to(self.device, torch.bfloat16).reshape(-1, normed.shape[-1]).contiguous()
        out = torch.empty((x.shape[0], self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
        N.check(self.lib.pgmi_lm_head(self.ctx, x.data_ptr(), x.shape[0], out.data_ptr(), self._s()), "pgmi_lm_head")
        return out

    def lm_logprobs(self, normed: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
                    return_lse: bool = False):
        """Token log-probabilities of the reference's loss (modeling_gemma.py:596-603) over final-normed rows
        without the logits (pgmi_lm_logprobs): normed (..., hidden) bf16, labels (...) int64, already shifted.
        Returns fp32 (rows,): log_softmax(lm_head(normed))[label], 0 where the label is ignore_index, NaN for any
        other label outside the vocabulary; with return_lse also logsumexp per row."""
        self._ready()
        x = normed.to(self.device, torch.bfloat16).reshape(-1, normed.shape[-1]).contiguous()
        lb = labels.to(self.device, torch.int64).reshape(-1).contiguous()
        if lb.numel() != x.shape[0]:
            raise ValueError(f"need one label per row: {lb.numel()} != {x.shape[0]}")
        out = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        lse = torch.empty_like(out) if return_lse else None
        N.check(self.lib.pgmi_lm_logprobs(self.ctx, x.data_ptr(), x.shape[0], lb.data_ptr(), int(ignore_index),
                                          out.data_ptr(), N.ptr(lse), self._s()), "pgmi_lm_logprobs")
        return (out, lse) if return_lse else out

    def logprobs(self, logits: torch.Tensor, ids: torch.Tensor, ignore_index: int = -100, return_lse: bool = False):
        """log_softmax(logits)[id] per row of existing fp32 logits (..., V) (pgmi_logprobs; the rule of
        modeling_gemma.py:596-603): 0 where the id is ignore_index, NaN for any other id outside [0, V)."""
        x = logits.reshape(-1, logits.shape[-1]).to(self.device, torch.float32).contiguous()
        lb = ids.to(self.device, torch.int64).reshape(-1).contiguous()
        if lb.numel() != x.shape[0]:
            raise ValueError(f"need one id per row: {lb.numel()} != {x.shape[0]}")
        out = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        lse = torch.empty_like(out) if return_lse else None
        N.check(self.lib.pgmi_logprobs(self.ctx, x.data_ptr(), x.shape[0], x.shape[1], lb.data_ptr(), int(ignore_index),
                                       out.data_ptr(), N.ptr(lse), self._s()), "pgmi_logprobs")
        return (out, lse) if return_lse else out

    @torch.no_grad()
    def shifted_logprobs(self, hidden: torch.Tensor, shift_labels: torch.Tensor, live: Optional[torch.Tensor] = None,
                         ignore_index: int = -100):
        """The one place the shifted loss is taken from hidden rows (modeling_gemma.py:596-603): hidden (B * L,
        hidden) final-normed rows, shift_labels (B, L - 1) = labels[:, 1:], live (B, L - 1) bool (default: the
        labels that are not ignore_index).  Only the live rows go through the lm_head (one index_select, one host
        sync for their indices).  Returns (logprobs (B, L - 1) fp32 with 0 where not live, live, loss): loss =
        -mean over the live tokens in fp64, NaN when there is none."""
        shift = shift_labels.to(self.device, torch.int64)
        B, L1 = shift.shape
        L = L1 + 1
        if live is None:
            live = shift != ignore_index
        out = torch.zeros((B, L1), dtype=torch.float32, device=self.device)
        at = live.nonzero()  # the host sync
        if at.shape[0] == 0:
            return out, live, torch.full((), float("nan"), dtype=torch.float32, device=self.device)
        out[at[:, 0], at[:, 1]] = self.lm_logprobs(hidden.index_select(0, at[:, 0] * L + at[:, 1]),
                                                   shift[at[:, 0], at[:, 1]], ignore_index)
        return out, live, (-out.sum(dtype=torch.float64) / at.shape[0]).float()

    @torch.no_grad()
    def score(self, input_ids: torch.Tensor, pixel_values: Optional[torch.Tensor], labels: torch.Tensor,
              attention_mask: Optional[torch.Tensor] = None, ignore_index: int = -100, adapter=_KEEP,
              prefix_lens=None, image_feats: Optional[torch.Tensor] = None) -> "Score":
        """The reference's forward(labels=...) loss (modeling_gemma.py:596-603) per token, from one prefill:
        position j is scored against labels[:, j + 1], and only the rows whose shifted label is live go through
        the lm_head (one index_select on the final-normed rows, one host sync; no (B, L, V) tensor exists).

        attention_mask (B, L) of 0 / 1: a ragged batch as Engine.generate takes it; ids and labels are moved to
        the right-padded form and pad positions count as ignored whatever their label.  pixel_values None: a
        text-only prompt.  adapter: as generate's.  Returns Score(logprobs (B, L - 1) fp32 with 0 where ignored,
        sums (B,), counts (B,), loss = -mean over the live tokens, NaN when there is none).

        The default reproduces the reference's non-causal forward(labels=): every token attends every token, so a
        teacher-forced answer is scored with its own tokens in view -- score an answer with prefix_lens.
        prefix_lens (B ints): row b's first prefix_lens[b] real tokens (counted after right-padding, image tokens
        included) are the prompt, attended from everywhere; the tokens after them attend causally and take the
        positions the decode loop would give them (prefix_np.prefix_positions), so the log-probabilities are the
        ones generate(return_logprobs=True) reports for the same tokens.  Labels of positions < prefix_lens[b] stay
        the caller's business (mask them with ignore_index to score the answer alone).  image_feats: the projected
        features, in place of pixel_values (score_candidates runs the vision tower once)."""
        if image_feats is not None and pixel_values is not None:
            raise ValueError("score: pixel_values or image_feats, not both")
        if adapter is not _KEEP:
            self.set_lora(adapter)
        ids = input_ids.to(self.device, torch.int64)
        lab = labels.to(self.device, torch.int64)
        if tuple(lab.shape) != tuple(ids.shape):
            raise ValueError(f"labels {tuple(lab.shape)} do not match input_ids {tuple(ids.shape)}")
        lens = R.lengths_from_mask(attention_mask) if attention_mask is not None else None
        if lens is not None:
            ids, lens = R.right_pad(ids, attention_mask)
            lab, _ = R.right_pad(lab, attention_mask, pad_id=ignore_index)
        ids = ids.contiguous()
        B, L = ids.shape
        feats = self.project(self.vision(pixel_values)) if pixel_values is not None else image_feats
        kv = self.scratch_kv(B, L)
        if prefix_lens is None:
            self.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=1, lens=lens)
        else:
            pl = np.asarray(torch.as_tensor(prefix_lens).detach().cpu(), dtype=np.int64).reshape(-1)
            if pl.shape[0] != B:
                raise ValueError(f"prefix_lens has {pl.shape[0]} entries for a batch of {B}")
            self.lm_forward(kv, 0, torch.from_numpy(PX.prefix_positions(L, pl)), ids=ids, image_feats=feats,
                            logits_rows=1, lens=lens, prefix_lens=pl)
        hidden = self.final_hidden(B * L)
        shift = lab[:, 1:]
        live = shift != ignore_index
        if lens is not None:  # the scored token j + 1 must be a real one
            live &= (torch.arange(1, L, device=self.device)[None, :] < lens.to(self.device)[:, None])
        out, live, loss = self.shifted_logprobs(hidden, shift, live, ignore_index)
        return Score(out, out.sum(1), live.sum(1), loss)

    @torch.no_grad()
    def score_candidates(self, prompt_ids, pixel_values: Optional[torch.Tensor], candidates, adapter=_KEEP,
                         ignore_index: int = -100) -> "CandidateScores":
        """Rank candidate answers to one prompt: log p(candidate | image, prompt) for each of `candidates` (a list
        of non-empty token lists) after prompt_ids (L0 tokens, image tokens included; 1-D or (1, L0)) and
        pixel_values (one image, or None).  The vision tower and the projector run once and the features are
        repeated per row; the rows prompt + candidate go through score(prefix_lens=L0) in groups of at most
        max_batch, right-padded, with only the candidate's tokens labelled.  Returns CandidateScores(sums (C,) fp32,
        counts (C,), logprobs: a list of C fp32 tensors, one value per candidate token)."""
        if adapter is not _KEEP:
            self.set_lora(adapter)
        prompt = [int(t) for t in torch.as_tensor(prompt_ids).reshape(-1).tolist()]
        cands = [[int(t) for t in c] for c in candidates]
        L0 = len(prompt)
        if L0 < 1 or not cands or any(len(c) < 1 for c in cands):
            raise ValueError("score_candidates: a prompt and at least one candidate, none of them empty")
        feats = self.project(self.vision(pixel_values)) if pixel_values is not None else None
        if feats is not None and feats.shape[0] != 1:
            raise ValueError("score_candidates takes one image")
        sums, counts, per = [], [], []
        for c0 in range(0, len(cands), self.max_batch):
            grp = cands[c0:c0 + self.max_batch]
            B, L = len(grp), L0 + max(len(c) for c in grp)
            ids = torch.zeros((B, L), dtype=torch.int64)
            lab = torch.full((B, L), ignore_index, dtype=torch.int64)
            mask = torch.zeros((B, L), dtype=torch.int64)
            for b, c in enumerate(grp):
                ids[b, :L0 + len(c)] = torch.tensor(prompt + c)
                lab[b, L0:L0 + len(c)] = torch.tensor(c)
                mask[b, :L0 + len(c)] = 1
            sc = self.score(ids, None, lab, attention_mask=mask, ignore_index=ignore_index, prefix_lens=[L0] * B,
                            image_feats=feats.expand(B, -1, -1) if feats is not None else None)
            sums.append(sc.sums)
            counts.append(sc.counts)
            per += [sc.logprobs[b, L0 - 1:L0 - 1 + len(c)] for b, c in enumerate(grp)]
        return CandidateScores(torch.cat(sums), torch.cat(counts), per)

    def decode(self, ids: torch.Tensor, kv: torch.Tensor, kv_len: int, position: int, logits: torch.Tensor = None,
               next_ids: torch.Tensor = None, graph: bool = False) -> torch.Tensor:
        """One KV-cached decode step for B sequences; returns logits (B, V) fp32."""
        self._ready()
        if ids.dtype is not torch.int64 or ids.device != self.device or not ids.is_contiguous():
            ids = ids.to(self.device, torch.int64).contiguous()
        ids = ids.view(-1)
        B = ids.numel()
        if logits is None:
            logits = torch.empty((B, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
        N.check(self.lib.pgmi_decode(self.ctx, ids.data_ptr(), B, kv.data_ptr(), kv.shape[2], kv.shape[3], kv_len,
                                     position, logits.data_ptr(), N.ptr(next_ids), int(graph), self._s()),
                "pgmi_decode")
        return logits

    def decode_steps(self, ids: torch.Tensor, kv: torch.Tensor, kv_len: int, position: int, n_steps: int,
                     logits: torch.Tensor = None, tokens: torch.Tensor = None, graph: bool = False) -> torch.Tensor:
        """n_steps greedy decode steps back to back (pgmi_decode_steps): ids (device int64, B) is read by the
        first step and receives every step's argmax in place; tokens (int64 (n_steps, B), optional) records
        them.  Returns the last step's logits (B, V) fp32."""
        self._ready()
        if ids.dtype is not torch.int64 or ids.device != self.device or not ids.is_contiguous():
            raise ValueError("decode_steps: ids must be a contiguous int64 tensor on the engine's device (updated in place)")
        B = ids.numel()
        if logits is None:
            logits = torch.empty((B, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
        if tokens is not None and (tokens.dtype is not torch.int64 or tokens.device != self.device
                                   or not tokens.is_contiguous() or tokens.numel() < n_steps * B):
            raise ValueError("decode_steps: tokens must be a contiguous int64 (n_steps, B) tensor on the device")
        N.check(self.lib.pgmi_decode_steps(self.ctx, ids.data_ptr(), B, kv.data_ptr(), kv.shape[2], kv.shape[3], kv_len,
                                           position, int(n_steps), logits.data_ptr(), N.ptr(tokens), int(graph),
                                           self._s()), "pgmi_decode_steps")
        return logits

    def decode_ragged(self, ids: torch.Tensor, kv: torch.Tensor, kv_lens, positions, n_steps: int = 1,
                      logits: torch.Tensor = None, tokens: torch.Tensor = None, next_ids: torch.Tensor = None,
                      graph: bool = False) -> torch.Tensor:
        """n_steps decode steps for B rows of different lengths (pgmi_decode_ragged): at step t row b writes
        its K/V at row kv_lens[b] + t, attends keys [0, kv_lens[b] + t] and uses rotary position
        positions[b] + t.  kv_lens / positions: B host ints each.  n_steps > 1 feeds each step's argmax back
        through next_ids (default: ids, in place, which must then be a contiguous int64 device tensor);
        tokens (int64 (n_steps, B), optional) records them.  Returns the last step's logits (B, V) fp32."""
        self._ready()
        if ids.dtype is not torch.int64 or ids.device != self.device or not ids.is_contiguous():
            if n_steps > 1 and next_ids is None:
                raise ValueError("decode_ragged: ids must be a contiguous int64 tensor on the engine's device "
                                 "(updated in place when n_steps > 1)")
            ids = ids.to(self.device, torch.int64).contiguous()
        ids = ids.view(-1)
        B = ids.numel()
        kl = torch.as_tensor(kv_lens).detach().to("cpu", torch.int32).reshape(-1).contiguous()
        ps = torch.as_tensor(positions).detach().to("cpu", torch.int32).reshape(-1).contiguous()
        if kl.numel() != B or ps.numel() != B:
            raise ValueError(f"decode_ragged: kv_lens / positions need {B} entries each")
        if n_steps > 1 and next_ids is None:
            next_ids = ids
        if logits is None:
            logits = torch.empty((B, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
        if tokens is not None and (tokens.dtype is not torch.int64 or tokens.device != self.device
                                   or not tokens.is_contiguous() or tokens.numel() < n_steps * B):
            raise ValueError("decode_ragged: tokens must be a contiguous int64 (n_steps, B) tensor on the device")
        N.check(self.lib.pgmi_decode_ragged(self.ctx, ids.data_ptr(), B, kv.data_ptr(), kv.shape[2], kv.shape[3],
                                            kl.data_ptr(), ps.data_ptr(), int(n_steps), logits.data_ptr(),
                                            N.ptr(next_ids), N.ptr(tokens), int(graph), self._s()),
                "pgmi_decode_ragged")
        return logits

    def decode_embeds(self, embeds: torch.Tensor, kv: torch.Tensor, kv_len: int, position: int,
                      logits: torch.Tensor = None, graph: bool = False) -> torch.Tensor:
        """The decode step over already-merged input rows (B, hidden) bf16 -- a caller's merge for
        a q_len == 1 step (pgmi_decode_embeds); returns logits (B, V) fp32."""
        self._ready()
        e = embeds.to(self.device, torch.bfloat16).reshape(-1, self.cfgd["t_hidden"]).contiguous()
        B = e.shape[0]
        if logits is None:
            logits = torch.empty((B, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
        N.check(self.lib.pgmi_decode_embeds(self.ctx, e.data_ptr(), B, kv.data_ptr(), kv.shape[2], kv.shape[3], kv_len,
                                            position, logits.data_ptr(), None, int(graph), self._s()),
                "pgmi_decode_embeds")
        return logits

    _POS_DTYPES = {torch.bfloat16: 0, torch.float32: 2, torch.int64: 10, torch.int32: 11, torch.float64: 12}

    def decode_embeds_dev(self, embeds: torch.Tensor, kv: torch.Tensor, kv_len: int, position: torch.Tensor,
                          mask: torch.Tensor = None, logits: torch.Tensor = None, graph: bool = False,
                          next_ids: torch.Tensor = None) -> torch.Tensor:
        """decode_embeds for one sequence with its rotary position and additive mask left on the device
        (a merge's outputs, read by the step itself: no host sync).  position: one element; mask:
        kv_len + 1 additive values (bf16 or fp32; other float dtypes are promoted to fp32)."""
        self._ready()
        e = embeds.to(self.device, torch.bfloat16).reshape(-1, self.cfgd["t_hidden"]).contiguous()
        if e.shape[0] != 1:
            raise ValueError("decode_embeds_dev: one sequence per step")
        p = position.to(self.device).reshape(-1)[:1]
        if p.dtype not in self._POS_DTYPES:
            p = p.to(torch.float64)
        p = p.contiguous()
        mp, mdt = None, N.DTYPE_BF16
        if mask is not None:
            m = mask.to(self.device).reshape(-1)
            if m.numel() != kv_len + 1:
                raise ValueError(f"mask has {m.numel()} keys, the step attends {kv_len + 1}")
            if m.dtype not in (torch.bfloat16, torch.float32):
                m = m.float()
            mp = m.contiguous()
            mdt = N.DTYPE_F32 if mp.dtype == torch.float32 else N.DTYPE_BF16
        if logits is None:
            logits = torch.empty((1, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device)
        N.check(self.lib.pgmi_decode_embeds_dev(self.ctx, e.data_ptr(), 1, kv.data_ptr(), kv.shape[2], kv.shape[3],
                                                kv_len, p.data_ptr(), self._POS_DTYPES[p.dtype], N.ptr(mp), mdt,
                                                mp.numel() if mp is not None else 0, logits.data_ptr(),
                                                N.ptr(next_ids), int(graph), self._s()),
                "pgmi_decode_embeds_dev")
        return logits

    def set_prefill_graph(self, on: bool) -> None:
        """Replay captured hipGraphs for repeated vision / language-model calls with the same buffers."""
        N.check(self.lib.pgmi_set_prefill_graph(self.ctx, int(bool(on))), "pgmi_set_prefill_graph")

    def set_decode_staged_norm(self, on: int) -> None:
        """Batched decode RMSNorm form: 0 once per row (default), 1 staged per projection, -1 default."""
        N.check(self.lib.pgmi_set_decode_staged_norm(self.ctx, int(on)), "pgmi_set_decode_staged_norm")

    # The 13-bit weight images come in two forms with one C entry each: "" (row-major segments, batch 1-2) and
    # "_batched" (fragment-major segments, 3..16 rows).  The six public methods below name the form; these do the call.
    def _set_packed(self, form: str, mask: int) -> None:
        name = f"pgmi_set_decode_packed{form}"
        N.check(getattr(self.lib, name)(self.ctx, int(mask)), name)

    def _packed_info(self, form: str, n: int):
        name = f"pgmi_decode_packed{form}_info"
        v = (ctypes.c_int64 * n)()
        N.check(getattr(self.lib, name)(self.ctx, v, n), name)
        return v

    def _packed_tensor(self, form: str, kind: int, layer: int) -> bool:
        name = f"pgmi_decode_packed{form}_tensor"
        rc = getattr(self.lib, name)(self.ctx, int(kind), int(layer))
        if rc < 0:
            N.check(rc, name)
        return rc == 1

    def set_decode_packed(self, on: int) -> None:
        """Decode at batch 1-2 on the lossless 13-bit weight images: 0 off, a mask of kinds (1 gate|up, 2 down,
        4 lm_head; 7 all), -1 the default (all at B = 1, lm_head at B = 2).  Results are bit-identical either way (pgmi_set_decode_packed)."""
        self._set_packed("", on)

    def decode_packed_info(self) -> dict:
        """How the batch 1-2 decode step reads its 2 x layers + 1 streamed tensors now (pgmi_decode_packed_info)."""
        v = self._packed_info("", 9)
        return {"mask": v[0], "mask_b2": v[8], "packed": v[1], "raw": v[2], "packed_bytes": v[3], "raw_bytes": v[4],
                "alloc_failed": bool(v[5]), "mf_alloc_failed": bool(v[6]), "scanned": v[7]}

    def decode_packed_tensor(self, kind: int, layer: int = 0) -> bool:
        """Is the tensor of kind 1 gate|up / 2 down (of `layer`) / 4 lm_head read from its 13-bit image now?"""
        return self._packed_tensor("", kind, layer)

    def set_decode_packed_batched(self, mask: int) -> None:
        """Batched decode (3..16 rows) on the fragment-major 13-bit weight images: 0 off (the default), or a mask of
        kinds (1 gate|up, 2 down, 4 lm_head; 7 all).  Results are bit-identical either way
        (pgmi_set_decode_packed_batched)."""
        self._set_packed("_batched", mask)

    def decode_packed_batched_info(self) -> dict:
        """How the batched decode step reads its 2 x layers + 1 streamed tensors now
        (pgmi_decode_packed_batched_info)."""
        v = self._packed_info("_batched", 6)
        return {"mask": v[0], "scanned": v[1], "packed": v[2], "raw": v[3], "packed_bytes": v[4],
                "alloc_failed": bool(v[5])}

    def decode_packed_batched_tensor(self, kind: int, layer: int = 0) -> bool:
        """Is the tensor of kind 1 gate|up / 2 down (of `layer`) / 4 lm_head read from its fragment-major 13-bit
        image by the batched step now?"""
        return self._packed_tensor("_batched", kind, layer)

    def decode_kernel(self, which: int, layer: int, B: int) -> None:
        """One decode projection on the decode workspace (pgmi_decode_kernel): 1 o_proj, 2 gate|up, 3 down, 4 lm_head."""
        self._ready()
        N.check(self.lib.pgmi_decode_kernel(self.ctx, int(which), int(layer), int(B), self._s()), "pgmi_decode_kernel")

    def decode_stage(self, stage: int, layer: int, B: int, kv: torch.Tensor, kv_lens, positions, ids: torch.Tensor = None,
                     ragged: bool = False, mask: torch.Tensor = None) -> None:
        """One stage of the decode step through the step's own launch code (pgmi_debug_decode_stage: a test hook):
        0 entry, 1 q|k|v, 2 attention + o_proj, 3 gate|up, 4 down, 5 lm_head, on the workspace decode_buffer
        reads and writes.  kv_lens / positions: an int (lock-step) or B host ints (ragged, or lock-step, which
        reads the first).  mask (B = 1): kv_lens + 1 additive values, bf16 or fp32, on the device."""
        self._ready()
        kl = torch.as_tensor(kv_lens).detach().to("cpu", torch.int32).reshape(-1).contiguous()
        ps = torch.as_tensor(positions).detach().to("cpu", torch.int32).reshape(-1).contiguous()
        if kl.numel() < (B if ragged else 1) or ps.numel() < (B if ragged else 1):
            raise ValueError("decode_stage: kv_lens / positions need one entry (lock-step) or B (ragged)")
        if ids is not None:
            if ids.dtype is not torch.int64 or ids.device != self.device or not ids.is_contiguous() or ids.numel() < B:
                raise ValueError("decode_stage: ids must be a contiguous int64 tensor of B entries on the device")
        mdt = N.DTYPE_BF16
        if mask is not None:
            if mask.device != self.device or not mask.is_contiguous() or mask.dtype not in (torch.bfloat16,
                                                                                            torch.float32):
                raise ValueError("decode_stage: mask must be a contiguous bf16 / fp32 tensor on the device")
            if mask.numel() != int(kl[0]) + 1:
                raise ValueError(f"mask has {mask.numel()} keys, the step attends {int(kl[0]) + 1}")
            mdt = N.DTYPE_F32 if mask.dtype == torch.float32 else N.DTYPE_BF16
        N.check(self.lib.pgmi_debug_decode_stage(self.ctx, int(stage), int(layer), int(B), N.ptr(ids), kv.data_ptr(),
                                                 kv.shape[2], kv.shape[3], kl.data_ptr(), ps.data_ptr(),
                                                 int(bool(ragged)), N.ptr(mask), mdt, self._s()),
                "pgmi_debug_decode_stage")

    def decode_partials(self, t: torch.Tensor, write: bool = False) -> torch.Tensor:
        """Copy the flash-decoding partial records between the decode attention and o_proj (fp32 [max_batch * kv
        heads][chunks][16 * 256 + 32]) into the contiguous device tensor t, or (write) t into them
        (pgmi_debug_decode_partials: a test hook)."""
        self._ready()
        if t.device != self.device or not t.is_contiguous():
            raise ValueError("decode_partials: a contiguous tensor on the engine's device")
        N.check(self.lib.pgmi_debug_decode_partials(self.ctx, t.data_ptr(), t.numel() * t.element_size(),
                                                    int(bool(write)), self._s()), "pgmi_debug_decode_partials")
        return t

    def lane_reduce(self, op: int, rows: torch.Tensor):
        """The kernels' in-register cross-lane reductions on fp32 rows of 64 (pgmi_debug_lane_reduce: a test hook):
        every lane's result, fp32 [rows][64]; ops 2 and 6 (first max) return (values, int32 indices)."""
        if rows.dtype is not torch.float32 or rows.device != self.device or not rows.is_contiguous() or \
                rows.dim() != 2 or rows.shape[1] != 64:
            raise ValueError("lane_reduce: a contiguous fp32 [rows][64] tensor on the engine's device")
        pair = int(op) in (2, 6)
        out = torch.empty((2 if pair else 1, rows.shape[0], 64), dtype=torch.float32, device=self.device)
        N.check(self.lib.pgmi_debug_lane_reduce(self.ctx, int(op), rows.data_ptr(), rows.shape[0], out.data_ptr(),
                                                self._s()), "pgmi_debug_lane_reduce")
        return (out[0], out[1].view(torch.int32)) if pair else out[0]

    def decode_buffer(self, which: int, t: torch.Tensor, write: bool = False) -> torch.Tensor:
        """Copy the decode workspace's h (0) / act (1) / logits (2) / q (3) / attention output (4, B >= 3) / hn (5) /
        ssq (6) / next ids (7) rows into the contiguous device tensor t, or (write) t into the workspace
        (pgmi_debug_decode_buffer: a test hook)."""
        self._ready()
        if t.device != self.device or not t.is_contiguous():
            raise ValueError("decode_buffer: a contiguous tensor on the engine's device")
        N.check(self.lib.pgmi_debug_decode_buffer(self.ctx, int(which), t.data_ptr(), t.numel() * t.element_size(),
                                                  int(bool(write)), self._s()), "pgmi_debug_decode_buffer")
        return t

    def prefill_stage(self, stage: int, layer: int, group: int, kv: torch.Tensor, kv_start: int, positions,
                      logits: torch.Tensor, ids: torch.Tensor = None, image_feats: torch.Tensor = None,
                      embeds: torch.Tensor = None, B: int = None, L: int = None, logits_rows: int = 0,
                      lens=None) -> None:
        """One stage of the language-model prefill for one row group (batch rows 8 * group ..) through the prefill's
        own launch code (pgmi_debug_prefill_stage: a test hook): 0 entry (whole batch), 1 q|k|v + RoPE + KV append,
        2 attention, 3 o_proj + residual + norm, 4 gate|up, 5 down + residual + norm, 6 logits, 7 the last-row tail
        of logits_rows 2, on the workspace prefill_buffer reads and writes.  The arguments are lm_forward's: ids
        (B, L) int64 or embeds (B, L, hidden) bf16 on the device (else B and L), host positions, lens for a ragged
        batch, and the caller's fp32 logits tensor."""
        self._ready()
        for t in (ids, image_feats, embeds, logits):
            if t is not None and (t.device != self.device or not t.is_contiguous()):
                raise ValueError("prefill_stage: contiguous tensors on the engine's device")
        if ids is not None:
            B, L = ids.shape
        elif embeds is not None:
            B, L = embeds.shape[0], embeds.shape[1]
        if B is None or L is None:
            raise ValueError("prefill_stage: ids, embeds or B and L")
        nimg = 0 if image_feats is None else image_feats.numel() // image_feats.shape[-1]
        pos = torch.as_tensor(positions, dtype=torch.int64).cpu()
        pos = torch.broadcast_to(pos.reshape(pos.shape[0] if pos.dim() > 1 else 1, -1), (B, L)).contiguous()
        ln = None
        if lens is not None:
            ln = torch.as_tensor(lens).detach().to("cpu", torch.int32).reshape(-1).contiguous()
            if ln.numel() != B:
                raise ValueError(f"lens has {ln.numel()} entries for a batch of {B}")
        rows = B * (L if logits_rows == 0 else 1)
        if logits.dtype is not torch.float32 or logits.numel() < rows * self.cfgd["t_vocab"]:
            raise ValueError("prefill_stage: logits must be fp32 with room for the call's rows")
        N.check(self.lib.pgmi_debug_prefill_stage(self.ctx, int(stage), int(layer), int(group), N.ptr(ids),
                                                  N.ptr(image_feats), nimg, N.ptr(embeds), int(B), int(L),
                                                  pos.data_ptr(), N.ptr(ln), kv.data_ptr(), kv.shape[2], kv.shape[3],
                                                  int(kv_start), logits.data_ptr(), int(logits_rows), self._s()),
                "pgmi_debug_prefill_stage")

    def prefill_buffer(self, which: int, t: torch.Tensor, write: bool = False) -> torch.Tensor:
        """Copy the first rows of the prefill workspace's Hs (0) / Tn (1) / QKV (2) / Qr (3) / AO (4) / ACT (5) /
        lastrows (6) / dAO (7) into the contiguous device tensor t, or (write) t into the workspace
        (pgmi_debug_prefill_buffer: a test hook)."""
        self._ready()
        if t.device != self.device or not t.is_contiguous():
            raise ValueError("prefill_buffer: a contiguous tensor on the engine's device")
        N.check(self.lib.pgmi_debug_prefill_buffer(self.ctx, int(which), t.data_ptr(), t.numel() * t.element_size(),
                                                   int(bool(write)), self._s()), "pgmi_debug_prefill_buffer")
        return t

    def argmax(self, logits: torch.Tensor) -> torch.Tensor:
        l2 = logits.reshape(-1, logits.shape[-1]).contiguous()
        out = torch.empty(l2.shape[0], dtype=torch.int64, device=self.device)
        N.check(self.lib.pgmi_argmax(self.ctx, l2.data_ptr(), l2.shape[0], l2.shape[1], out.data_ptr(), self._s()))
        return out

    def sample_top_p(self, x: torch.Tensor, top_p: float, temperature: Optional[float] = None,
                     u: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                     return_kept_mass: bool = False):
        """Nucleus sampling on the device (inference.py:15-24).
        x (..., V) fp32: logits when `temperature` > 0 (softmax(x / T) of inference.py:65 is
        fused), else probabilities (the reference _sample_top_p's input).  u: uniforms in [0, 1)
        per row (default: torch.rand on the device with `generator`).  Returns int64 (rows,)."""
        x2 = x.reshape(-1, x.shape[-1]).to(self.device, torch.float32).contiguous()
        rows, V = x2.shape
        if u is None:
            u = torch.rand(rows, device=self.device, generator=generator)
        u = u.to(self.device, torch.float32).reshape(-1).contiguous()
        if u.numel() != rows:
            raise ValueError(f"need one uniform per row: {u.numel()} != {rows}")
        out = torch.empty(rows, dtype=torch.int64, device=self.device)
        kept = torch.empty(rows, dtype=torch.float32, device=self.device) if return_kept_mass else None
        T = float(temperature) if temperature is not None and temperature > 0 else 0.0
        N.check(self.lib.pgmi_sample_top_p(self.ctx, x2.data_ptr(), rows, V, T, float(top_p), u.data_ptr(),
                                           out.data_ptr(), N.ptr(kept), self._s()), "pgmi_sample_top_p")
        return (out, kept) if return_kept_mass else out

    # ------------------------------------------------------------------ batched greedy driver
    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, pixel_values: torch.Tensor, n_tokens: int, graph: bool = True,
                 kv: torch.Tensor = None, do_sample: bool = False, temperature: float = 0.8, top_p: float = 0.9,
                 generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, sync_every: int = 16, return_lengths: bool = False,
                 attention_mask: Optional[torch.Tensor] = None, return_logprobs: bool = False, adapter=_KEEP):
        """Batched generation: prefill, then n_tokens-1 decode steps
        with the next token picked on the device -- greedy argmax, or with do_sample the
        temperature + top-p draw of inference.py:64-66 -- and no host sync per token.
        Positions follow inference.py's semantics (first decode position = L + 1,
        modeling_gemma.py:526).

        eos_token_id: the stop token of inference.py:51,70-71, applied per row on the device
        (pgmi_eos_update): a row keeps its eos and emits pad_token_id (default: eos) after it.
        The loop ends early once every row has stopped, checked every `sync_every` steps (one
        host read per check instead of the reference's `.item()` per token); the result is
        trimmed to the longest row.  return_lengths: also return int64 (B,) tokens per row up
        to and including its eos (the length of the reference's generated_tokens).

        attention_mask (B, L) of 0 / 1, optional: a batch of different prompts as the processor pads it
        (padding="longest", left or right).  Each row then runs with its own length -- prefill over its
        real tokens, decode at its own KV row and rotary position (pgmi_lm_forward_ragged /
        pgmi_decode_ragged) -- and generates what it would alone.  No mask, or all ones: the lock-step
        path.  kv defaults to new_kv(B, L + n_tokens + 1) either way.

        return_logprobs: also return fp32 (B, n_tokens) (last in the returned tuple): the log-probability of each
        emitted token under softmax of the raw step logits (pgmi_logprobs) -- no temperature and no top-p
        renormalisation, whatever the sampling settings -- and 0 for the pad emitted after a row's eos.  The
        loop then runs one launch per step, as do_sample does; the tokens are the same.

        adapter: the name of a loaded LoRA adapter to generate under, or None for the base model; the engine
        switches first when it is not the active one (set_lora).  Left out: whatever is active stays."""
        if adapter is not _KEEP:
            self.set_lora(adapter)
        ids = input_ids.to(self.device, torch.int64)
        lens = R.lengths_from_mask(attention_mask) if attention_mask is not None else None
        if lens is not None:
            ids, lens = R.right_pad(ids, attention_mask)
            ids = ids.contiguous()
        B, L = ids.shape
        if kv is None:
            kv = self.new_kv(B, L + n_tokens + 1)
        feats = self.project(self.vision(pixel_values))
        logits = self.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=2,
                                 lens=lens)
        toks = torch.empty((B, n_tokens), dtype=torch.int64, device=self.device)
        if do_sample:
            us = torch.rand((n_tokens, B), device=self.device, generator=generator)
            toks[:, 0] = self.sample_top_p(logits[:, 0], top_p, temperature, u=us[0])
        else:
            toks[:, 0] = self.argmax(logits[:, 0])
        if return_logprobs:
            lps = torch.zeros((B, n_tokens), dtype=torch.float32, device=self.device)
            lps[:, 0] = self.logprobs(logits[:, 0], toks[:, 0])
        # per-B persistent buffers (step logits, fed-back ids, sampled step's argmax, chunk record): stable
        # pointers, so repeated generate calls on the same cache replay the decode graphs they captured
        bufs = self._gen_buf.get(B)
        if bufs is None:
            bufs = (torch.empty((B, self.cfgd["t_vocab"]), dtype=torch.float32, device=self.device),
                    torch.empty(B, dtype=torch.int64, device=self.device),
                    torch.empty(B, dtype=torch.int64, device=self.device),
                    torch.empty((self.GEN_CHUNK, B), dtype=torch.int64, device=self.device))
            self._gen_buf[B] = bufs
        step_logits, cur, nxt, rec = bufs
        cur.copy_(toks[:, 0])
        # step(t, next_ids) / step(t, None, n, rec): the decode step(s) producing token t (.. t + n - 1) from `cur`
        # -- all the two forms differ in after the prefill (lock-step: one KV row and position; ragged: a row's own)
        if lens is None:
            def step(t, next_ids, n=1, tokens=None):
                if tokens is not None:  # pgmi_decode_steps: the argmax is fed back in place
                    self.decode_steps(cur, kv, L + t - 1, L + t, n, logits=step_logits, tokens=tokens, graph=graph)
                else:
                    self.decode(cur, kv, L + t - 1, L + t, logits=step_logits, next_ids=next_ids, graph=graph)
        else:
            lens = lens.to(torch.int32)

            def step(t, next_ids, n=1, tokens=None):
                self.decode_ragged(cur, kv, lens + (t - 1), lens + t, n, logits=step_logits, tokens=tokens,
                                   next_ids=next_ids, graph=graph)
        stop = eos_token_id is not None
        if stop:
            pad = int(eos_token_id if pad_token_id is None else pad_token_id)
            finished = torch.zeros(B, dtype=torch.int32, device=self.device)
            alive = torch.empty(1, dtype=torch.int32, device=self.device)
            self._eos_update(cur, finished, int(eos_token_id), pad, alive)
            toks[:, 0] = cur
        n_done = n_tokens
        if not do_sample and not stop and not return_logprobs and graph and n_tokens > 1 and B >= self.GEN_MIN_BATCH:
            # greedy without a stop token: GEN_CHUNK steps per hipGraph launch (pgmi_decode_steps / _ragged), the
            # argmax fed back in place and every step's token kept in a device record
            t = 1
            while t < n_tokens:
                n = min(self.GEN_CHUNK, n_tokens - t)
                step(t, None, n, rec)
                toks[:, t:t + n] = rec[:n].t()
                t += n
        else:
            for t in range(1, n_tokens):
                if stop and (t - 1) % max(1, sync_every) == 0 and int(alive.item()) == 0:
                    n_done = t
                    break
                if do_sample:
                    step(t, nxt)
                    cur.copy_(self.sample_top_p(step_logits, top_p, temperature, u=us[t]))
                else:  # greedy: the argmax is fed back in place (next_ids == ids)
                    step(t, cur)
                if return_logprobs:  # of the token the step picked; rows that stopped earlier emit pad: 0
                    lp = self.logprobs(step_logits, cur)
                    lps[:, t] = lp.masked_fill_(finished != 0, 0.0) if stop else lp
                if stop:
                    self._eos_update(cur, finished, int(eos_token_id), pad, alive)
                toks[:, t] = cur
        if not stop:
            ret = (toks, torch.full((B,), n_tokens, dtype=torch.int64, device=self.device)) if return_lengths else (toks,)
        else:
            toks = toks[:, :n_done]
            hit = toks == int(eos_token_id)
            first = torch.where(hit.any(1), hit.int().argmax(1) + 1,
                                torch.full_like(hit[:, 0], n_done, dtype=torch.int64))
            toks = toks[:, :int(first.max().item())].contiguous()
            ret = (toks, first.to(torch.int64)) if return_lengths else (toks,)
        if return_logprobs:
            ret = ret + (lps[:, :toks.shape[1]].contiguous(),)
        return ret if len(ret) > 1 else ret[0]

    def _eos_update(self, next_ids: torch.Tensor, finished: torch.Tensor, eos: int, pad: int,
                    n_alive: Optional[torch.Tensor]) -> None:
        N.check(self.lib.pgmi_eos_update(self.ctx, next_ids.data_ptr(), finished.data_ptr(), next_ids.numel(), eos, pad,
                                         n_alive.data_ptr() if n_alive is not None else None, self._s()),
                "pgmi_eos_update")
