"""oracle/prefill_stage_ref.py -- TEST INFRASTRUCTURE ONLY.

The language-model prefill cut at the stages of pgmi_debug_prefill_stage (include/pgmi.h), each stage as two numpy
functions of the same inputs:

  truth_stageN  float64 throughout: the only roundings are the bf16 inputs and weights as given (the rotary
                cos/sin table counts as a weight: it is a bf16 table on both sides).
  ref_stageN    the reference's arithmetic -- fp32 accumulation, bf16 where modeling_gemma.py rounds -- built from
                oracle/paligemma_np.py's functions, one sequence at a time in the shapes gemma_forward gives them
                for that sequence alone ((1, n, D) with n its real tokens; a ragged row's pad slots as a second
                piece), so that the chained stages equal that oracle bit for bit
                (tests/test_cpu_prefill_stage_refs.py).

Arrays are float32 holding bf16 values (truth: float64), [B][L][D]: hs, tn [..][hidden], q, ao [..][heads *
head_dim], k, v [..][kv_heads * head_dim], act [..][intermediate], logits [..][vocab].  The KV slab is
[layer][K|V][kv_batch][token][kv_heads * head_dim] (Engine.new_kv); a call at kv_start writes slot l of batch row b
at token kv_start + l, and every query row of b attends tokens [0, kv_start + n_b), n_b = lens[b] for a ragged
batch (its real tokens; the pad slots' rows are computed like any other row and attend the same keys), else L.
"""
from __future__ import annotations

import math

import numpy as np

from . import paligemma_np as O
from .decode_stage_ref import (F32, F64, _gelu64, _lin64, _lp, _rms64, bias_rows, d_rows, dims,  # noqa: F401
                               normalizer, rel_l2_rows, rope_rows, ulp_frac)


# ---------------------------------------------------------------- shared pieces
def _lens(lens, B, L):
    return [L] * B if lens is None else [int(n) for n in np.asarray(lens).reshape(-1)[:B]]


def _seq(fn, lens, *xs):
    """fn over one sequence at a time: its real tokens as (1, n, D), then (ragged) its pad slots as (1, L - n, D)."""
    B, L = xs[0].shape[:2]
    out = []
    for b, n in enumerate(_lens(lens, B, L)):
        parts = [fn(*[x[b:b + 1, :n] for x in xs])]
        if n < L:
            parts.append(fn(*[x[b:b + 1, n:] for x in xs]))
        out.append(np.concatenate(parts, axis=1))
    return np.concatenate(out, axis=0)


def merged_ids(cfg, ids, lens):
    """The ids the merge sees: a ragged row's pad slots hold the pad id whatever the caller left there."""
    ids = np.array(ids, dtype=np.int64, copy=True)
    if lens is not None:
        for b, n in enumerate(_lens(lens, *ids.shape)):
            ids[b, n:] = cfg.get("pad_token_id", 0)
    return ids


def kv_write(kv, layer, kv_start, k, v):
    """Write the call's K/V rows (every slot, pad slots included) at tokens kv_start .. of batch rows 0 .. (in place)."""
    B, L = k.shape[:2]
    kv[layer, 0, :B, kv_start:kv_start + L] = k
    kv[layer, 1, :B, kv_start:kv_start + L] = v
    return kv


def _next_norm(cfg, layer):
    return _lp(layer + 1) + "input_layernorm.weight" if layer + 1 < dims(cfg)["L"] else "language_model.model.norm.weight"


# ---------------------------------------------------------------- stage 0: merge x normalizer, layer 0's input norm
def ref_stage0(P, cfg, ids=None, feats=None, lens=None, embeds=None):
    """-> hs, tn.  ids (B, L) with feats (rows, hidden) the projected image rows in masked_scatter order (the k-th
    <image> token takes row k; modeling_gemma.py:468-537), or embeds (B, L, hidden) given rows.  hs = bf16(rows x
    bf16(sqrt(hidden))) (:367-368), tn = layer 0's input RMSNorm of it."""
    if embeds is None:
        f = None if feats is None else np.asarray(feats, F32)[None]
        embeds = O.merge(P, cfg, f, merged_ids(cfg, ids, lens))
    hs = O.bf16(embeds * normalizer(cfg))
    return hs, O.rms_norm(hs, P[_lp(0) + "input_layernorm.weight"], dims(cfg)["eps"])


def truth_stage0(P, cfg, ids=None, feats=None, lens=None, embeds=None):
    if embeds is None:
        ids = merged_ids(cfg, ids, lens)
        E = P["language_model.model.embed_tokens.weight"]
        pad = cfg.get("pad_token_id", 0)
        img = ids == cfg["image_token_index"]
        embeds = np.where(((ids != pad) & ~img)[..., None], E[ids].astype(F64), 0.0)
        if feats is not None and img.any():
            embeds[img] = (np.asarray(feats, F64) / math.sqrt(cfg["hidden_size"]))[: int(img.sum())]
    hs = np.asarray(embeds, F64) * F64(normalizer(cfg))
    return hs, _rms64(hs, P[_lp(0) + "input_layernorm.weight"], dims(cfg)["eps"])


# ---------------------------------------------------------------- stage 1: q|k|v, RoPE (the rows the cache receives)
def ref_stage1(P, cfg, layer, tn, positions, lens=None):
    """-> q, k, v of every slot; positions (B, L)."""
    d = dims(cfg)
    pre = _lp(layer) + "self_attn."
    NH, NKV, HD = d["NH"], d["NKV"], d["HD"]
    invf = O.inv_freq(HD, d["theta"])
    pos = np.asarray(positions).reshape(tn.shape[:2])[..., None].astype(F32)

    def one(x, p):
        n = x.shape[1]
        cos, sin = O.rope_cos_sin(p[..., 0], invf, d["max_pos"])
        cos, sin = cos[:, None], sin[:, None]
        q = O.linear(x, P[pre + "q_proj.weight"]).reshape(1, n, NH, HD).transpose(0, 2, 1, 3)
        k = O.linear(x, P[pre + "k_proj.weight"]).reshape(1, n, NKV, HD).transpose(0, 2, 1, 3)
        v = O.linear(x, P[pre + "v_proj.weight"])
        q = O.apply_rope(q, cos, sin).transpose(0, 2, 1, 3).reshape(1, n, NH * HD)
        k = O.apply_rope(k, cos, sin).transpose(0, 2, 1, 3).reshape(1, n, NKV * HD)
        return np.concatenate([q, k, v], axis=-1)

    qkv = _seq(one, lens, tn, pos)
    return qkv[..., :NH * HD], qkv[..., NH * HD:(NH + NKV) * HD], qkv[..., (NH + NKV) * HD:]


def truth_stage1(P, cfg, layer, tn, positions, lens=None):
    d = dims(cfg)
    pre = _lp(layer) + "self_attn."
    NH, NKV, HD = d["NH"], d["NKV"], d["HD"]
    B, L = tn.shape[:2]
    cos, sin = (t.astype(F64).reshape(B, L, 1, HD) for t in rope_rows(cfg, positions))
    rot = lambda y: y * cos + O.rotate_half(y) * sin  # noqa: E731
    q = rot(_lin64(tn, P[pre + "q_proj.weight"]).reshape(B, L, NH, HD)).reshape(B, L, -1)
    k = rot(_lin64(tn, P[pre + "k_proj.weight"]).reshape(B, L, NKV, HD)).reshape(B, L, -1)
    return q, k, _lin64(tn, P[pre + "v_proj.weight"])


# ---------------------------------------------------------------- stage 2: attention
def _heads(row, n, NKV, HD, rep, dt):
    """Tokens [0, n) of one batch row's K or V as (1, heads, n, head_dim) (repeat_kv, modeling_gemma.py:136-141)."""
    x = row[:n].astype(dt).reshape(1, n, NKV, HD).transpose(0, 2, 1, 3)
    return np.repeat(x, rep, axis=1)


def ref_stage2(P, cfg, layer, q, kv, kv_start, lens=None, L=None, less=None):
    """-> ao: every query row of batch row b over tokens [0, kv_start + n_b) of `kv` (its own rows already written;
    modeling_gemma.py:266-277, no mask: the prefix attends itself in full, :506-507).  L: the call's slots per row
    where q holds fewer (stage 7's single row).  less: {(b, l): k} -- that query row attends k keys fewer (a mutant)."""
    d = dims(cfg)
    NH, NKV, HD = d["NH"], d["NKV"], d["HD"]
    B, Lq = q.shape[:2]
    keys = [kv_start + n for n in _lens(lens, B, L or Lq)]
    ao = np.zeros(q.shape, F32)
    for b in range(B):
        def one(x, b=b, n=keys[b]):
            k = _heads(kv[layer, 0, b], n, NKV, HD, NH // NKV, F32)
            v = _heads(kv[layer, 1, b], n, NKV, HD, NH // NKV, F32)
            qb = x.reshape(1, x.shape[1], NH, HD).transpose(0, 2, 1, 3)
            s = O.bf16(np.matmul(qb, k.transpose(0, 1, 3, 2)))
            s = O.bf16(s / F32(math.sqrt(HD)))
            p = O.bf16(O.softmax_f32(s))
            o = O.bf16(np.matmul(p, v))
            return o.transpose(0, 2, 1, 3).reshape(1, x.shape[1], NH * HD)
        ao[b:b + 1] = _seq(one, None if lens is None or L is not None else [_lens(lens, B, Lq)[b]], q[b:b + 1])
        for (bb, l), cut in (less or {}).items():
            if bb == b:
                ao[b, l] = one(q[b:b + 1, l:l + 1], n=keys[b] - cut)[0, 0]
    return ao


def truth_stage2(P, cfg, layer, q, kv, kv_start, lens=None, L=None):
    d = dims(cfg)
    NH, NKV, HD = d["NH"], d["NKV"], d["HD"]
    B, Lq = q.shape[:2]
    ao = np.zeros(q.shape, F64)
    for b, n in enumerate(_lens(lens, B, L or Lq)):
        n += kv_start
        k = _heads(kv[layer, 0, b], n, NKV, HD, NH // NKV, F64)
        v = _heads(kv[layer, 1, b], n, NKV, HD, NH // NKV, F64)
        qb = q[b].astype(F64).reshape(1, Lq, NH, HD).transpose(0, 2, 1, 3)
        s = np.matmul(qb, k.transpose(0, 1, 3, 2)) / math.sqrt(HD)
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        ao[b] = np.matmul(e / e.sum(axis=-1, keepdims=True), v).transpose(0, 2, 1, 3).reshape(Lq, NH * HD)
    return ao


# ---------------------------------------------------------------- stage 3: o_proj, residual, post-attention norm
def ref_stage3(P, cfg, layer, ao, hs, lens=None):
    """-> hs_new = bf16(o_proj(ao) + hs), tn = its post-attention RMSNorm (modeling_gemma.py:291, :318-322)."""
    x = _seq(lambda r: O.linear(r, P[_lp(layer) + "self_attn.o_proj.weight"]), lens, ao)
    h = O.bf16(x + hs)
    return h, O.rms_norm(h, P[_lp(layer) + "post_attention_layernorm.weight"], dims(cfg)["eps"])


def truth_stage3(P, cfg, layer, ao, hs, lens=None):
    h = _lin64(ao, P[_lp(layer) + "self_attn.o_proj.weight"]) + np.asarray(hs, F64)
    return h, _rms64(h, P[_lp(layer) + "post_attention_layernorm.weight"], dims(cfg)["eps"])


# ---------------------------------------------------------------- stage 4: gate|up, GeGLU
def ref_stage4(P, cfg, layer, tn, lens=None):
    """-> act = bf16(gelu_tanh(gate(tn)) * up(tn)) (modeling_gemma.py:133-134)."""
    pre = _lp(layer) + "mlp."
    g = _seq(lambda r: O.gelu_tanh(O.linear(r, P[pre + "gate_proj.weight"])), lens, tn)
    u = _seq(lambda r: O.linear(r, P[pre + "up_proj.weight"]), lens, tn)
    return O.bf16(g * u)


def truth_stage4(P, cfg, layer, tn, lens=None):
    pre = _lp(layer) + "mlp."
    return _gelu64(_lin64(tn, P[pre + "gate_proj.weight"])) * _lin64(tn, P[pre + "up_proj.weight"])


# ---------------------------------------------------------------- stage 5: down, residual, the next norm
def ref_stage5(P, cfg, layer, act, hs, lens=None):
    """-> hs_new = bf16(down(act) + hs), tn = the next layer's input RMSNorm of it (the final norm after the last)."""
    x = _seq(lambda r: O.linear(r, P[_lp(layer) + "mlp.down_proj.weight"]), lens, act)
    h = O.bf16(x + hs)
    return h, O.rms_norm(h, P[_next_norm(cfg, layer)], dims(cfg)["eps"])


def truth_stage5(P, cfg, layer, act, hs, lens=None):
    h = _lin64(act, P[_lp(layer) + "mlp.down_proj.weight"]) + np.asarray(hs, F64)
    return h, _rms64(h, P[_next_norm(cfg, layer)], dims(cfg)["eps"])


# ---------------------------------------------------------------- stage 6: the logits
def last_rows(x, lens=None, at=None):
    """[B][1][D]: each sequence's last real row (lens[b] - 1; lock-step: L - 1), or row `at` of every sequence."""
    B, L = x.shape[:2]
    idx = [n - 1 for n in _lens(lens, B, L)] if at is None else [at] * B
    return np.stack([x[b, i:i + 1] for b, i in enumerate(idx)])


def ref_stage6(P, cfg, tn, hs, logits_rows, lens=None, lastrows=None, at=None):
    """-> logits, lastrows.  logits_rows 0: lm_head of every row of tn (the final norm, modeling_gemma.py:379,
    :417-418; the head is tied to the embedding).  1: the final norm + lm_head of each sequence's last row of hs.
    2: the same of the given lastrows (stage 7's)."""
    E = P["language_model.model.embed_tokens.weight"]
    if logits_rows == 0:
        return _seq(lambda r: O.linear(r, E), lens, tn), None
    if logits_rows == 1:
        lastrows = last_rows(hs, lens, at)
    x = O.rms_norm(lastrows, P["language_model.model.norm.weight"], dims(cfg)["eps"])
    return _seq(lambda r: O.linear(r, E), None, x), lastrows


def truth_stage6(P, cfg, tn, hs, logits_rows, lens=None, lastrows=None, at=None):
    E = P["language_model.model.embed_tokens.weight"]
    if logits_rows == 0:
        return _lin64(tn, E), None
    if logits_rows == 1:
        lastrows = last_rows(hs, lens, at)
    return _lin64(_rms64(lastrows, P["language_model.model.norm.weight"], dims(cfg)["eps"]), E), lastrows


# ---------------------------------------------------------------- stage 7: the last layer for the last row alone
def ref_stage7(P, cfg, layer, q, kv, kv_start, hs):
    """-> lastrows [B][1][hidden]: stages 2 .. 5 of `layer` for the last slot of each sequence (q [B][L][..] as
    stage 1 left it, hs the hidden state entering the layer) without the closing norm (stage 6 applies it)."""
    L = q.shape[1]
    ao = ref_stage2(P, cfg, layer, q[:, L - 1:], kv, kv_start, L=L)
    h, tn = ref_stage3(P, cfg, layer, ao, hs[:, L - 1:])
    act = ref_stage4(P, cfg, layer, tn)
    x = _seq(lambda r: O.linear(r, P[_lp(layer) + "mlp.down_proj.weight"]), None, act)
    return O.bf16(x + h), ao


def truth_stage7(P, cfg, layer, q, kv, kv_start, hs):
    L = q.shape[1]
    ao = truth_stage2(P, cfg, layer, q[:, L - 1:], kv, kv_start, L=L)
    h, tn = truth_stage3(P, cfg, layer, ao, hs[:, L - 1:])
    act = truth_stage4(P, cfg, layer, tn)
    return _lin64(act, P[_lp(layer) + "mlp.down_proj.weight"]) + h, ao


# ---------------------------------------------------------------- the chained prefill
def ref_prefill(P, cfg, kv, kv_start, positions, ids=None, feats=None, lens=None, embeds=None, logits_rows=0):
    """Stages 0 .. 6 chained over every layer; `kv` receives the call's rows.  -> logits."""
    hs, tn = ref_stage0(P, cfg, ids, feats, lens, embeds)
    for i in range(dims(cfg)["L"]):
        q, k, v = ref_stage1(P, cfg, i, tn, positions, lens)
        kv_write(kv, i, kv_start, k, v)
        ao = ref_stage2(P, cfg, i, q, kv, kv_start, lens)
        hs, tn = ref_stage3(P, cfg, i, ao, hs, lens)
        act = ref_stage4(P, cfg, i, tn, lens)
        hs, tn = ref_stage5(P, cfg, i, act, hs, lens)
    return ref_stage6(P, cfg, tn, hs, logits_rows, lens)[0]
