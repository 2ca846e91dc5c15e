"""The prefix-LM attention cases shared by tests/test_cpu_prefix.py (reference against float64 truth, no GPU) and
tests/test_gpu_prefix.py (pgmi_op_attention_prefix against both): the case table, seeded inputs built like
prefill_stage_cases.attn_inputs, and the cached R / T pair.  Query j of batch row b attends keys
[0, min(kv_start + lens[b], kv_start + max(prefix[b], j + 1))) (pgmi.prefix_np).  The acceptance conditions are the
decode suite's (decode_stage_cases.check with ulp=False), unchanged."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

import decode_stage_cases as DC
from oracle import paligemma_np as O
from pgmi import prefix_np as PX

NH, NKV, HD = 8, 1, 256
QD, KD = NH * HD, NKV * HD

Case = namedtuple("Case", "B Lq kv_start lens prefix")

CASES = {
    "causal40": Case(1, 40, 0, None, (0,)),                  # rows with 1 .. 40 keys, across the 32-key tile
    "p33of72": Case(1, 72, 0, None, (33,)),                  # 9 workgroups, bounds differ per workgroup
    "ragged": Case(3, 40, 0, (1, 40, 23), (1, 17, 23)),      # two all-prefix rows beside a causal one
    "cached": Case(2, 17, 47, None, (0, 5)),                 # cached keys visible from every query
    "cached500": Case(1, 17, 500, None, (0,)),               # 517 keys in 17 tiles, one key range: the last tile masked
    # 1,020 keys in 32 tiles: the launcher splits them into two ranges of 16 tiles (asserted by the GPU test: a
    # split needs >= 32 tiles), range 1 from key 512.  Query j attends 501 + j keys: the first workgroup (j <= 7,
    # bound 508) does no tile of range 1 at all; in the second (j = 8 .. 15, bound 516) range 1 is one tile in which
    # j = 8 .. 11 have no key while j = 12 .. 15 do; every partial goes through k_attn_fs_combine
    "split1020": Case(1, 520, 500, None, (0,)),
}
SPLITS = {"split1020": 2}                                    # key ranges per case (default 1)


def real(name):
    c = CASES[name]
    return [c.Lq] * c.B if c.lens is None else list(c.lens)


def limits(name):
    c = CASES[name]
    return PX.prefix_limits(c.Lq, c.kv_start, c.lens, c.prefix)


def _rng(*key):
    return np.random.default_rng([20253, *key])


def _randn(rng, *shape):
    return O.bf16(rng.standard_normal(shape).astype(np.float32))


@lru_cache(maxsize=None)
def inputs(name):
    """-> q [B][Lq][QD], k and v [B][kv_start + Lq][KD]: seeded bf16 values at tokens [0, kv_start + n_b) of batch row
    b and NaN behind them (no query of the row may read those).  As in prefill_stage_cases.attn_inputs the last real
    key of each row is planted dominant in head 0 (+ 8 u on a query's head 0, - 32 u on every other key, along one
    unit direction u) -- for the queries that see that key, the row's last and its pad slots: one of them that attends
    a key too few loses head 0 altogether.  The other queries carry no plant: all their keys would sit 16 lower, where
    bf16 rounds a score by up to 2^-4, and the reference alone was at rel-L2 1.3e-2 .. 1.6e-2, d 0.07 .. 0.12, past
    CAP_REL and CAP_D.  Their head 0 has its component along u taken out instead (up to bf16 rounding), so the keys'
    - 32 u does not reach their scores: left in, a component of 2 .. 3 put every score of the row at 4 .. 6, rounded
    by up to 2^-6, and the reference alone at rel-L2 1.05e-2."""
    c = CASES[name]
    rng = _rng(list(CASES).index(name))
    q = _randn(rng, c.B, c.Lq, QD)
    u = rng.standard_normal(KD).astype(np.float32)
    u /= np.linalg.norm(u)
    sees_last = limits(name) == c.kv_start + np.asarray(real(name))[:, None]
    q0 = q[:, :, :KD]
    q[:, :, :KD] = O.bf16(np.where(sees_last[:, :, None], q0 + np.float32(8.0) * u, q0 - (q0 @ u)[:, :, None] * u))
    k = np.full((c.B, c.kv_start + c.Lq, KD), np.nan, np.float32)
    v = k.copy()
    for b, n in enumerate(real(name)):
        n += c.kv_start
        k[b, :n], v[b, :n] = _randn(rng, n, KD), _randn(rng, n, KD)
        k[b, :n - 1] = O.bf16(k[b, :n - 1] - np.float32(32.0) * u)
    return q, k, v


def _heads(x, n, dt):
    """Tokens [0, n) of one batch row's K or V as (1, heads, n, head_dim) (repeat_kv, modeling_gemma.py:136-141)."""
    return np.repeat(x[:n].astype(dt).reshape(1, n, NKV, HD).transpose(0, 2, 1, 3), NH // NKV, axis=1)


@lru_cache(maxsize=None)
def ref(name):
    """-> R, T [B][Lq][QD].  R: the oracle's arithmetic (gemma_attention, modeling_gemma.py:266-277) with the additive
    prefix mask -- s = bf16(q.k), bf16(s / sqrt(hd)), bf16(s + mask), p = bf16(softmax_fp32(s)), o = bf16(p.v) -- one
    sequence at a time over its own real keys.  T: float64 on the same bf16 inputs."""
    c = CASES[name]
    q, k, v = inputs(name)
    mask = PX.prefix_mask(c.Lq, c.kv_start, c.lens, c.prefix)
    R, T = np.zeros(q.shape, np.float32), np.zeros(q.shape, np.float64)
    for b, n in enumerate(real(name)):
        n += c.kv_start
        m = mask[b:b + 1, :, :, :n]
        qb = q[b].reshape(1, c.Lq, NH, HD).transpose(0, 2, 1, 3)
        kk, vv = _heads(k[b], n, np.float32), _heads(v[b], n, np.float32)
        s = O.bf16(np.matmul(qb, kk.transpose(0, 1, 3, 2)))
        s = O.bf16(s / np.float32(math.sqrt(HD)))
        s = O.bf16(s + m)
        o = O.bf16(np.matmul(O.bf16(O.softmax_f32(s)), vv))
        R[b] = o.transpose(0, 2, 1, 3).reshape(c.Lq, QD)
        s = np.matmul(qb.astype(np.float64), _heads(k[b], n, np.float64).transpose(0, 1, 3, 2)) / math.sqrt(HD) + m
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        o = np.matmul(e / e.sum(axis=-1, keepdims=True), _heads(v[b], n, np.float64))
        T[b] = o.transpose(0, 2, 1, 3).reshape(c.Lq, QD)
    return R, T


def rows2(x):
    return np.asarray(x).reshape(-1, np.asarray(x).shape[-1])


def check(name, G):
    """decode_stage_cases.check(name, G, R, T, ulp=False), row by row."""
    R, T = ref(name)
    DC.check(f"prefix attention {name}", rows2(G), rows2(R), rows2(T), ulp=False)


# ---------------------------------------------------------------- model level: the masked oracle, one row at a time
SEED = 1234
STEP_FLOOR_FACTOR = 1.45       # tests_helpers.STEP_FLOOR_FACTOR: rel-L2 <= max(2e-2, 1.45 x the reference's own error)


@lru_cache(maxsize=None)
def text_model():
    """The 2+2-layer full-width config and the language model's seeded weights (text only)."""
    from oracle import weights as W
    cfg = W.small_config()
    P = W.synthetic_state_dict_f32(cfg, SEED)
    return cfg, {n: v for n, v in P.items() if n.startswith("language_model")}


def text_row(n, seed):
    """n random text ids in [3, vocab - 1), the first one <bos> = 2."""
    cfg, _ = text_model()
    ids = np.random.default_rng([77, seed]).integers(3, cfg["text_config"]["vocab_size"] - 1, n).astype(np.int64)
    ids[0] = 2
    assert not (ids == cfg["image_token_index"]).any()
    return ids


def rel_rows(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-30)


def step_bound(floor):
    return np.maximum(2e-2, STEP_FLOOR_FACTOR * np.asarray(floor))


def oracle_pass(row, prefix, masked=True):
    """One pass of the oracle over one unpadded row at B = 1: gemma_forward with prefix_mask and prefix_positions
    (masked), or the reference's zero mask at positions 0 .. L - 1 (today's prefill).  -> logits [L][V] in bf16
    arithmetic, the same in fp32 (O.fp32_truth), and the bf16 run's cache (k, v per layer, [1][heads][L][hd])."""
    cfg, P = text_model()
    L = len(row)
    emb = O.merge(P, cfg, None, np.asarray(row)[None])
    mask = PX.prefix_mask(L, 0, None, [prefix]) if masked else None
    pos = PX.prefix_positions(L, [prefix]) if masked else np.arange(L)[None]
    kv = O.KV()
    ref = O.gemma_forward(P, cfg, emb, pos, kv, mask=mask)[0]
    with O.fp32_truth():
        tru = O.gemma_forward(P, cfg, emb, pos, O.KV(), mask=mask)[0]
    return ref, tru, (kv.k, kv.v)


def oracle_stepwise(row, prefix):
    """A prefix-token prefill, then len(row) - prefix paligemma_decode steps fed the row's own tokens.  -> the
    len(row) - prefix + 1 step logits [..][V] in bf16 arithmetic and in fp32: row t is one pass's row prefix - 1 + t."""
    cfg, P = text_model()
    out = []
    for truth in (False, True):
        ctx = O.fp32_truth() if truth else None
        if ctx:
            ctx.__enter__()
        try:
            kv = O.KV()
            emb = O.merge(P, cfg, None, np.asarray(row[:prefix])[None])
            lg = [O.gemma_forward(P, cfg, emb, np.arange(prefix)[None], kv, all_logits=False)[0, -1]]
            for t in range(prefix, len(row)):
                lg.append(O.paligemma_decode(P, cfg, np.asarray(row[t:t + 1]), kv, t + 1)[0, -1])
        finally:
            if ctx:
                ctx.__exit__()
        out.append(np.stack(lg))
    return out[0], out[1]
