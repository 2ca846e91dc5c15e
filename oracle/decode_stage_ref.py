"""oracle/decode_stage_ref.py -- TEST INFRASTRUCTURE ONLY.

The decode step cut at the six points of pgmi_debug_decode_stage (include/pgmi.h), each stage as two numpy
functions of the same inputs:

  truth_stageN  float64 throughout: the only roundings are the bf16 inputs and weights as given (the rotary
                cos/sin table counts as a weight: it is a bf16 table on both sides).
  ref_stageN    the reference's arithmetic -- fp32 accumulation, bf16 where modeling_gemma.py rounds -- built
                from oracle/paligemma_np.py's functions, one row at a time in the shapes paligemma_decode gives
                them for B = 1, so that the chained stages equal that oracle bit for bit
                (tests/test_cpu_decode_stage_refs.py).

Arrays are float32 holding bf16 values (truth: float64).  Rows are batch rows: h, hn [B][hidden], q
[B][heads * head_dim], k, v [B][kv_heads * head_dim], act [B][intermediate], logits [B][vocab].  The KV slab is
[layer][K|V][kv_batch][token][kv_heads * head_dim] (Engine.new_kv); a row of length kv_len has its new K/V written
at token kv_len and attends tokens [0, kv_len].
"""
from __future__ import annotations

import math

import numpy as np

from . import paligemma_np as O

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------- shared pieces
def dims(cfg):
    t = cfg["text_config"]
    return dict(H=t["hidden_size"], I=t["intermediate_size"], NH=t["num_attention_heads"],
                NKV=t["num_key_value_heads"], HD=t.get("head_dim", 256), V=t["vocab_size"],
                L=t["num_hidden_layers"], eps=t.get("rms_norm_eps", 1e-6),
                max_pos=t.get("max_position_embeddings", 8192), theta=t.get("rope_theta", 10000.0))


def normalizer(cfg) -> np.float32:
    """GemmaModel's embedding normalizer, bf16(sqrt(hidden)) (modeling_gemma.py:367)."""
    return O.bf16(np.array([math.sqrt(cfg["text_config"]["hidden_size"])], F32))[0]


def rope_rows(cfg, positions):
    """cos, sin [B][head_dim] (bf16 values) of each row's position, clamped to the table
    (GemmaRotaryEmbedding.forward, modeling_gemma.py:155-185)."""
    d = dims(cfg)
    return O.rope_cos_sin(np.asarray(positions).reshape(-1), O.inv_freq(d["HD"], d["theta"]), d["max_pos"])


def embed_rows(P, cfg, ids):
    """Embedding rows of the merge for text-only ids: pad-id rows are zero (modeling_gemma.py:468-537)."""
    return O.merge(P, cfg, None, np.asarray(ids).reshape(-1, 1))[:, 0]


def new_kv(cfg, kv_batch, kv_max, fill=np.nan):
    d = dims(cfg)
    return np.full((d["L"], 2, kv_batch, kv_max, d["NKV"] * d["HD"]), fill, F32)


def kv_append(kv, layer, kv_lens, k, v):
    """Write row b's new K/V at token kv_lens[b] of batch row b (in place)."""
    for b, n in enumerate(np.asarray(kv_lens).reshape(-1)):
        kv[layer, 0, b, int(n)] = k[b]
        kv[layer, 1, b, int(n)] = v[b]
    return kv


def _lp(i):
    return f"language_model.model.layers.{i}."


def _rows(fn, *xs):
    """fn over one row at a time, each as (1, 1, D): the shapes the oracle's B = 1 decode step computes in."""
    return np.concatenate([fn(*[x[b:b + 1, None, :] for x in xs])[:, 0] for b in range(xs[0].shape[0])], axis=0)


def _rms64(x, w, eps):
    x = x.astype(F64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * (1.0 + w.astype(F64))


def _gelu64(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _lin64(x, w):
    return x.astype(F64) @ w.T.astype(F64)


# ---------------------------------------------------------------- stage 0: embedding x normalizer (+ layer 0's input norm)
def ref_stage0(P, cfg, ids):
    """-> h, hn: h = bf16(E[ids] x bf16(sqrt(hidden))) with pad rows zero (modeling_gemma.py:367-368), hn = layer
    0's input RMSNorm of it (what the unstaged B >= 3 form hands to q|k|v)."""
    h = O.bf16(embed_rows(P, cfg, ids) * normalizer(cfg))
    return h, O.rms_norm(h, P[_lp(0) + "input_layernorm.weight"], dims(cfg)["eps"])


def truth_stage0(P, cfg, ids):
    h = embed_rows(P, cfg, ids).astype(F64) * F64(normalizer(cfg))
    return h, _rms64(h, P[_lp(0) + "input_layernorm.weight"], dims(cfg)["eps"])


# ---------------------------------------------------------------- stage 1: input norm, q|k|v, RoPE
def ref_stage1(P, cfg, layer, h, positions, hn=None):
    """-> q, k, v rows (k, v: the rows appended to the cache).  hn: the already normed rows (else h is normed
    here); positions: one rotary position per row."""
    d = dims(cfg)
    pre = _lp(layer)
    x = O.rms_norm(h, P[pre + "input_layernorm.weight"], d["eps"]) if hn is None else hn
    q = _rows(lambda r: O.linear(r, P[pre + "self_attn.q_proj.weight"]), x)
    k = _rows(lambda r: O.linear(r, P[pre + "self_attn.k_proj.weight"]), x)
    v = _rows(lambda r: O.linear(r, P[pre + "self_attn.v_proj.weight"]), x)
    cos, sin = rope_rows(cfg, positions)
    B = x.shape[0]
    q = O.apply_rope(q.reshape(B, d["NH"], d["HD"]), cos[:, None], sin[:, None]).reshape(B, -1)
    k = O.apply_rope(k.reshape(B, d["NKV"], d["HD"]), cos[:, None], sin[:, None]).reshape(B, -1)
    return q, k, v


def truth_stage1(P, cfg, layer, h, positions, hn=None):
    d = dims(cfg)
    pre = _lp(layer)
    x = _rms64(h, P[pre + "input_layernorm.weight"], d["eps"]) if hn is None else hn.astype(F64)
    q = _lin64(x, P[pre + "self_attn.q_proj.weight"])
    k = _lin64(x, P[pre + "self_attn.k_proj.weight"])
    v = _lin64(x, P[pre + "self_attn.v_proj.weight"])
    cos, sin = (t.astype(F64)[:, None] for t in rope_rows(cfg, positions))
    B = x.shape[0]
    rot = lambda y: y * cos + O.rotate_half(y) * sin  # noqa: E731
    return rot(q.reshape(B, d["NH"], d["HD"])).reshape(B, -1), rot(k.reshape(B, d["NKV"], d["HD"])).reshape(B, -1), v


# ---------------------------------------------------------------- stage 2: attention, o_proj, residual
def _heads(kv_slab_row, n, NKV, HD, rep, dt):
    """Tokens [0, n) of one batch row's K or V as (1, heads, n, head_dim) (repeat_kv, modeling_gemma.py:136-141)."""
    x = kv_slab_row[:n].astype(dt).reshape(1, n, NKV, HD).transpose(0, 2, 1, 3)
    return np.repeat(x, rep, axis=1)


def ref_stage2(P, cfg, layer, q, kv, kv_lens, h, masks=None, mask_round=True):
    """-> h_new, ao: row b attends tokens [0, kv_lens[b]] of batch row b of `kv` (its own K/V already appended),
    ao = the attention output rows before o_proj, h_new = bf16(o_proj(ao) + h) (modeling_gemma.py:266-291,
    :318-322).  masks: per row None or kv_lens[b] + 1 additive values; mask_round: the sum is rounded to bf16
    (a bf16 mask, modeling_gemma.py:269) or left in fp32 (an fp32 mask)."""
    d = dims(cfg)
    NH, NKV, HD = d["NH"], d["NKV"], d["HD"]
    ao = np.zeros_like(q)
    for b, n in enumerate(np.asarray(kv_lens).reshape(-1)[:q.shape[0]]):
        n = int(n) + 1
        k = _heads(kv[layer, 0, b], n, NKV, HD, NH // NKV, F32)
        v = _heads(kv[layer, 1, b], n, NKV, HD, NH // NKV, F32)
        qb = q[b].reshape(1, 1, NH, HD).transpose(0, 2, 1, 3)
        s = O.bf16(np.matmul(qb, k.transpose(0, 1, 3, 2)))
        s = O.bf16(s / F32(math.sqrt(HD)))
        if masks is not None and masks[b] is not None:
            s = s + np.asarray(masks[b], F32).reshape(1, 1, 1, n)
            if mask_round:
                s = O.bf16(s)
        p = O.bf16(O.softmax_f32(s))
        o = O.bf16(np.matmul(p, v))
        ao[b] = o.transpose(0, 2, 1, 3).reshape(NH * HD)
    x = _rows(lambda r: O.linear(r, P[_lp(layer) + "self_attn.o_proj.weight"]), ao)
    return O.bf16(x + h), ao


def truth_stage2(P, cfg, layer, q, kv, kv_lens, h, masks=None, mask_round=True):
    d = dims(cfg)
    NH, NKV, HD = d["NH"], d["NKV"], d["HD"]
    ao = np.zeros(q.shape, F64)
    for b, n in enumerate(np.asarray(kv_lens).reshape(-1)[:q.shape[0]]):
        n = int(n) + 1
        k = _heads(kv[layer, 0, b], n, NKV, HD, NH // NKV, F64)
        v = _heads(kv[layer, 1, b], n, NKV, HD, NH // NKV, F64)
        qb = q[b].astype(F64).reshape(1, 1, NH, HD).transpose(0, 2, 1, 3)
        s = np.matmul(qb, k.transpose(0, 1, 3, 2)) / math.sqrt(HD)
        if masks is not None and masks[b] is not None:
            s = s + np.asarray(masks[b], F64).reshape(1, 1, 1, n)
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        p = e / e.sum(axis=-1, keepdims=True)
        ao[b] = np.matmul(p, v).transpose(0, 2, 1, 3).reshape(NH * HD)
    return _lin64(ao, P[_lp(layer) + "self_attn.o_proj.weight"]) + h.astype(F64), ao


# ---------------------------------------------------------------- stage 3: post-attention norm, gate|up, GeGLU
def ref_stage3(P, cfg, layer, h):
    """-> act = bf16(gelu_tanh(gate(x)) * up(x)), x = the post-attention RMSNorm of h (modeling_gemma.py:133-134)."""
    pre = _lp(layer)
    x = O.rms_norm(h, P[pre + "post_attention_layernorm.weight"], dims(cfg)["eps"])
    g = _rows(lambda r: O.gelu_tanh(O.linear(r, P[pre + "mlp.gate_proj.weight"])), x)
    u = _rows(lambda r: O.linear(r, P[pre + "mlp.up_proj.weight"]), x)
    return O.bf16(g * u)


def truth_stage3(P, cfg, layer, h):
    pre = _lp(layer)
    x = _rms64(h, P[pre + "post_attention_layernorm.weight"], dims(cfg)["eps"])
    return _gelu64(_lin64(x, P[pre + "mlp.gate_proj.weight"])) * _lin64(x, P[pre + "mlp.up_proj.weight"])


# ---------------------------------------------------------------- stage 4: down, residual (+ the next layer's input norm)
def ref_stage4(P, cfg, layer, act, h):
    """-> h_new = bf16(down(act) + h), hn = the next layer's input RMSNorm of h_new (None on the last layer)."""
    d = dims(cfg)
    x = _rows(lambda r: O.linear(r, P[_lp(layer) + "mlp.down_proj.weight"]), act)
    hn_ = O.bf16(x + h)
    nxt = O.rms_norm(hn_, P[_lp(layer + 1) + "input_layernorm.weight"], d["eps"]) if layer + 1 < d["L"] else None
    return hn_, nxt


def truth_stage4(P, cfg, layer, act, h):
    d = dims(cfg)
    hn_ = _lin64(act, P[_lp(layer) + "mlp.down_proj.weight"]) + h.astype(F64)
    nxt = _rms64(hn_, P[_lp(layer + 1) + "input_layernorm.weight"], d["eps"]) if layer + 1 < d["L"] else None
    return hn_, nxt


# ---------------------------------------------------------------- stage 5: final norm, lm_head, argmax
def ref_stage5(P, cfg, h):
    """-> logits, next ids (the first maximum, torch.argmax / inference.py:68); the head is tied to the embedding."""
    x = O.rms_norm(h, P["language_model.model.norm.weight"], dims(cfg)["eps"])
    lg = _rows(lambda r: O.linear(r, P["language_model.model.embed_tokens.weight"]), x)
    return lg, np.argmax(lg, axis=-1)


def truth_stage5(P, cfg, h):
    x = _rms64(h, P["language_model.model.norm.weight"], dims(cfg)["eps"])
    lg = _lin64(x, P["language_model.model.embed_tokens.weight"])
    return lg, np.argmax(lg, axis=-1)


# ---------------------------------------------------------------- the chained step
def ref_decode(P, cfg, ids, kv, kv_lens, positions):
    """Stages 0..5 chained over every layer: one decode step for B rows; `kv` receives the new rows.  -> logits,
    next ids."""
    d = dims(cfg)
    h, _ = ref_stage0(P, cfg, ids)
    for i in range(d["L"]):
        q, k, v = ref_stage1(P, cfg, i, h, positions)
        kv_append(kv, i, kv_lens, k, v)
        h, _ = ref_stage2(P, cfg, i, q, kv, kv_lens, h)
        act = ref_stage3(P, cfg, i, h)
        h, _ = ref_stage4(P, cfg, i, act, h)
    return ref_stage5(P, cfg, h)


# ---------------------------------------------------------------- the acceptance measures (per row)
def rel_l2_rows(x, t):
    x, t = np.asarray(x, F64), np.asarray(t, F64)
    return np.linalg.norm(x - t, axis=-1) / np.maximum(np.linalg.norm(t, axis=-1), 1e-300)


def d_rows(x, t):
    """max_i |x_i - t_i| / (|t_i| + s), s the rms of the truth row."""
    x, t = np.asarray(x, F64), np.asarray(t, F64)
    s = np.sqrt((t * t).mean(axis=-1, keepdims=True))
    return (np.abs(x - t) / (np.abs(t) + s + 1e-300)).max(axis=-1)


def bias_rows(x, t):
    """(mean_i sign(t_i) (x_i - t_i) / (|t_i| + s), its standard error under zero-mean errors): round-to-nearest
    leaves the mean at zero within the error, truncation pulls every element towards zero (about half a bf16 ulp)."""
    x, t = np.asarray(x, F64), np.asarray(t, F64)
    s = np.sqrt((t * t).mean(axis=-1, keepdims=True))
    e = np.sign(t) * (x - t) / (np.abs(t) + s + 1e-300)
    return e.mean(axis=-1), np.sqrt((e * e).mean(axis=-1) / e.shape[-1])


def ulp_frac(a, b, ulps=1):
    """Fraction of elements of a within `ulps` bf16 ulps of b (tests/test_gpu_ops.py's measure)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    sp = np.abs(b) * F32(2.0 ** -7) + F32(1e-30)
    return float((np.abs(a - b) <= ulps * sp).mean())
