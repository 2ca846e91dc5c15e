"""The prefill-stage cases shared by tests/test_cpu_prefill_stage_refs.py (reference against float64 truth, no GPU)
and tests/test_gpu_prefill_stages.py (kernels against both): the case list, seeded inputs of every stage (a stage's
inputs never come from the stage before it) and the cached references.  The acceptance conditions are the decode
suite's (decode_stage_cases.check / check_norm / reference_distances, CAP_REL, CAP_D, BIAS_SE), unchanged."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import decode_stage_cases as DC
from decode_stage_cases import (BIAS_SE, CAP_D, CAP_REL, FIGURES, check_norm, model,  # noqa: F401
                                reference_distances)
from oracle import paligemma_np as O
from oracle import prefill_stage_ref as R

SEED, V, MAX_BATCH, MAX_SEQ, KV_MAX = DC.SEED, DC.V, DC.MAX_BATCH, 320, DC.KV_MAX
KV_BATCH = DC.KV_BATCH                       # 17 > every B: a wrong batch stride lands in a visible row
H, I, QD, KD = DC.H, DC.I, DC.QD, DC.KD
GROUP = 8                                    # csrc/engine_ctx.h kPrefillGroup
MAX_POS = DC.MAX_POS

Case = namedtuple("Case", "B L kv_start lens pos kv_max")


def _case(B, L, kv_start=0, lens=None, shift=0, base=None, kv_max=KV_MAX):
    """positions: kv_start + slot, batch row b shifted by b * shift; base: the first position of row 0 instead."""
    first = kv_start if base is None else base
    pos = first + np.arange(L)[None, :] + shift * np.arange(B)[:, None]
    return Case(B, L, kv_start, lens, pos.astype(np.int64), kv_max)


CASES = {
    # the table plans of M = 288: fused RoPE epilogue, o_proj split 4, R288w, down split 8; attention variant 82
    "A": _case(1, 288),
    "B": _case(1, 1),                                     # one row, one key
    "C": _case(1, 33),                                    # an M tail past 32 under the fallback plans
    "D": _case(2, 17, 47, shift=9),                       # continuation: Lk = 64 > Lq, row 1's positions shifted
    "Dmax": _case(2, 17, 47, shift=-30, base=8175),       # positions up to 8191, the table's last row
    "E": _case(3, 40, 0, lens=(1, 40, 23)),               # ragged
    "F": _case(9, 8),                                     # a second row group holding one row
    "Fr": _case(9, 8, 0, lens=(8, 1, 5, 8, 3, 8, 2, 7, 4)),
    "G": _case(1, 17, 500),                               # Lk = 517 >= 512: the key-split attention (stages 1, 2)
    # stage 7 only (the last-row tail of logits_rows 2): B = 3 (the MFMA o_proj GEMV), and both B past the config's
    # max_kv on a longer slab (the prefill attention kernel + gemv_res instead of flash-decoding)
    "T3": _case(3, 17, 47, shift=3),
    "X1": _case(1, 17, 1010, kv_max=1040),
    "X3": _case(3, 17, 1010, shift=2, base=1010, kv_max=1040),
}
STAGE_CASES = ("A", "B", "C", "D", "E", "F", "Fr")       # every stage; G: stages 1 and 2; Dmax: stage 1
TAIL_CASES = ("C", "D", "T3", "F", "X1", "X3")            # stage 7
CHAIN_CASES = ("B", "C", "D", "E", "F", "Fr")
# layer per stage (both layers are covered: stage 5 closes with the next input norm on 0, the final norm on 1)
LAYER = {1: 1, 2: 0, 3: 0, 4: 1, 5: 0, 7: 1}
# case C's forced plans (pgmi_tune_gemm_shape; M, N, K, dual, cfg, split): the M = 288 table's four configurations
C_TABLE_PLANS = ((33, 2560, 2048, 0, 32, 1), (33, 2048, 2048, 0, 34, 4), (33, 16384, 2048, 1, 38, 1),
                 (33, 2048, 16384, 0, 31, 8))
C_SPLIT_QKV = ((33, 2560, 2048, 0, 11, 2),)               # q|k|v split: the fused path refused, slabs to rope_kv_append
C_PLAIN_QKV = ((33, 2560, 2048, 0, 11, 1),)               # a tile without the RoPE epilogue, unsplit


def groups(c):
    return [(g, g * GROUP, min(GROUP, c.B - g * GROUP)) for g in range((c.B + GROUP - 1) // GROUP)]


def rows2(x):
    """[B][L][D] -> [B * L][D] (check() compares row by row)."""
    return np.asarray(x).reshape(-1, np.asarray(x).shape[-1])


def check(name, G, Rr, T, **kw):
    DC.check(name, rows2(G), rows2(Rr), rows2(T), **kw)


def _rng(*key):
    return np.random.default_rng([20252, *key])


def _key(name):
    return list(CASES).index(name)


def _randn(rng, *shape, scale=1.0):
    return O.bf16(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


# ---------------------------------------------------------------- seeded inputs
@lru_cache(maxsize=None)
def ids_feats(name):
    """ids (B, L) and the projected image rows: every row of L >= 4 opens with 1 .. 3 <image> tokens (the k-th of
    the batch takes image row k), row 0 holds the pad id once, and a ragged row's pad slots hold <image> tokens the
    merge must neither count nor look up.  Two image rows more than the tokens take."""
    cfg, _ = model()
    c = CASES[name]
    rng = _rng(1, _key(name))
    ids = rng.integers(3, V - 64, (c.B, c.L)).astype(np.int64)
    n_img = 0
    for b in range(c.B):
        n = c.L if c.lens is None else c.lens[b]
        k = min(1 + b % 3, n - 1) if c.L >= 4 else 0
        ids[b, :k] = cfg["image_token_index"]
        ids[b, n:] = cfg["image_token_index"]
        n_img += k
    if c.L >= 4 and (c.lens is None or c.lens[0] == c.L):
        ids[0, c.L // 2] = cfg.get("pad_token_id", 0)
    return ids, _randn(rng, n_img + 2, H)


@lru_cache(maxsize=None)
def rows(name, what):
    """Seeded rows [B][L][..]: 'tn' normed rows, 'hs' hidden rows (row scale 0.5 .. 3), 'ao', 'act', 'q'."""
    c = CASES[name]
    rng = _rng(2, _key(name), ("tn", "hs", "ao", "act", "q", "emb").index(what))
    if what == "hs":
        sc = np.linspace(0.5, 3.0, c.B * c.L, dtype=np.float32).reshape(c.B, c.L, 1)
        return O.bf16(_randn(rng, c.B, c.L, H) * sc)
    width, scale = {"tn": (H, 1.0), "ao": (H, 0.5), "act": (I, 0.25), "q": (QD, 1.0), "emb": (H, 0.05)}[what]
    return _randn(rng, c.B, c.L, width, scale=scale)


def real(name):
    c = CASES[name]
    return [c.L] * c.B if c.lens is None else list(c.lens)


@lru_cache(maxsize=None)
def attn_inputs(name, layer):
    """-> q [B][L][QD] and a NaN slab [2][2][B][kv_start + L][KD] (the GPU test copies it into its own) holding seeded
    K/V at batch row b, tokens [0, kv_start + n_b) of `layer`.  The last real key of each row is planted dominant in
    head 0: every query's head 0 carries + 8 u and every OTHER key - 32 u along one unit direction u, so in head 0
    every other score sits 8 x 32 / 16 = 16 below the last key's (e^-16 x 517 keys: its weight rounds to 1.0 in bf16)
    and a row attending one key too few loses head 0 altogether; in the other heads the shift is common to those
    keys up to about +- 2.  Two weaker plants were tried first and are recorded here because both were changed
    for what the REFERENCE does, by the number formats alone:
      * + 3.5 on the last key's own score put the reference alone past CAP_REL at cases A and G (rel-L2 7.9e-3 ..
        8.7e-3): bf16 rounds a score of 4 .. 8 by up to 2^-7, and all of it lands in the dominant weight.  So the
        plant lowers the other scores instead and the dominant one stays near zero.
      * - 6 on the other scores left the last key 0.3 .. 0.45 of head 0 at 288 / 517 keys, and head 0 most of the
        row's norm.  The row's error is then ONE bf16 rounding of ONE weight -- the reference's of the normalised p,
        the kernel's of the unnormalised e (the allowed deviation) -- two independent errors uniform in +- 2^-9,
        whose ratio passes 1.5 at one row in three however exact the implementation.  On the MI355X the kernel and
        the reference had the same mean error in head 0 (1.51e-2 both, case A), the kernel's worst row was below the
        reference's (5.98e-3 against 6.30e-3), and 5 of 288 rows (A) and 1 of 17 (G) passed 1.5 x (worst 1.84 x).
        With a weight that rounds to 1.0 on both sides (the decode suite's every-key-but-one mask has the same
        property) no single rounding carries a row."""
    c = CASES[name]
    rng = _rng(3, _key(name))
    q = rows(name, "q").copy()
    u = rng.standard_normal(KD).astype(np.float32)
    u /= np.linalg.norm(u)
    q[:, :, :KD] = O.bf16(q[:, :, :KD] + np.float32(8.0) * u)
    kv = np.full((2, 2, c.B, c.kv_start + c.L, KD), np.nan, np.float32)
    for b, n in enumerate(real(name)):
        n += c.kv_start
        kv[layer, :, b, :n] = _randn(rng, 2, n, KD)
        kv[layer, 0, b, :n - 1] = O.bf16(kv[layer, 0, b, :n - 1] - np.float32(32.0) * u)
    return q, kv


# ---------------------------------------------------------------- cached references: -> (R..., T...)
@lru_cache(maxsize=None)
def stage0_ref(name, embeds=False):
    cfg, P = model()
    c = CASES[name]
    if embeds:
        kw = dict(embeds=rows(name, "emb"))
    else:
        ids, feats = ids_feats(name)
        kw = dict(ids=ids, feats=feats, lens=c.lens)
    return R.ref_stage0(P, cfg, **kw), R.truth_stage0(P, cfg, **kw)


@lru_cache(maxsize=None)
def stage1_ref(name, layer=LAYER[1]):
    cfg, P = model()
    c = CASES[name]
    a = (P, cfg, layer, rows(name, "tn"), c.pos, c.lens)
    return R.ref_stage1(*a), R.truth_stage1(*a)


@lru_cache(maxsize=None)
def stage2_ref(name, layer=LAYER[2]):
    cfg, P = model()
    c = CASES[name]
    q, kv = attn_inputs(name, layer)
    return (R.ref_stage2(P, cfg, layer, q, kv, c.kv_start, c.lens),
            R.truth_stage2(P, cfg, layer, q, kv, c.kv_start, c.lens))


@lru_cache(maxsize=None)
def stage3_ref(name, layer=LAYER[3]):
    cfg, P = model()
    a = (P, cfg, layer, rows(name, "ao"), rows(name, "hs"), CASES[name].lens)
    return R.ref_stage3(*a), R.truth_stage3(*a)


@lru_cache(maxsize=None)
def stage4_ref(name, layer=LAYER[4]):
    cfg, P = model()
    a = (P, cfg, layer, rows(name, "tn"), CASES[name].lens)
    return R.ref_stage4(*a), R.truth_stage4(*a)


@lru_cache(maxsize=None)
def stage5_ref(name, layer):
    cfg, P = model()
    a = (P, cfg, layer, rows(name, "act"), rows(name, "hs"), CASES[name].lens)
    return R.ref_stage5(*a), R.truth_stage5(*a)


@lru_cache(maxsize=None)
def stage6_ref(name, logits_rows):
    """Logits of the seeded tn (logits_rows 0) or of the last real rows of the seeded hs (1)."""
    cfg, P = model()
    a = (P, cfg, rows(name, "tn"), rows(name, "hs"), logits_rows, CASES[name].lens)
    return R.ref_stage6(*a), R.truth_stage6(*a)


@lru_cache(maxsize=None)
def stage7_ref(name, layer=LAYER[7]):
    """-> (R lastrows, R ao, R logits), (T ...): the tail from the seeded q / slab / hs, and stage 6 of its rows."""
    cfg, P = model()
    c = CASES[name]
    q, kv = attn_inputs(name, layer)
    hs = rows(name, "hs")
    Rl, Ra = R.ref_stage7(P, cfg, layer, q, kv, c.kv_start, hs)
    Tl, Ta = R.truth_stage7(P, cfg, layer, q, kv, c.kv_start, hs)
    Rg = R.ref_stage6(P, cfg, None, None, 2, lastrows=Rl)[0]
    Tg = R.truth_stage6(P, cfg, None, None, 2, lastrows=Tl)[0]
    return (Rl, Ra, Rg), (Tl, Ta, Tg)


@lru_cache(maxsize=None)
def prior_kv(name):
    """The slab a chained case starts from: NaN, and for a continuation (kv_start > 0) the reference's own K/V rows of
    kv_start earlier tokens per row (a reference prefill of seeded ids at positions 0 ..)."""
    cfg, P = model()
    c = CASES[name]
    kv = np.full((2, 2, c.B, c.kv_start + c.L, KD), np.nan, np.float32)   # (the GPU test copies it into its own)
    if c.kv_start:
        ids = _rng(4, _key(name)).integers(3, V - 64, (c.B, c.kv_start)).astype(np.int64)
        pos = np.broadcast_to(np.arange(c.kv_start), ids.shape)
        R.ref_prefill(P, cfg, kv, 0, pos, ids=ids, logits_rows=1)
    return kv
