"""The decode-stage cases shared by tests/test_cpu_decode_stage_refs.py (reference against float64 truth, no GPU)
and tests/test_gpu_decode_stages.py (kernels against both): seeded inputs, the case lists, the cached references
and the acceptance conditions.  A row's inputs do not depend on the batch it runs in, so every reference is
computed once for 16 rows and a batch of B compares its first B rows."""
from functools import lru_cache

import numpy as np

from oracle import decode_stage_ref as D
from oracle import paligemma_np as O
from oracle import weights as W

SEED, V, MAX_BATCH, KV_MAX = 1234, 1000, 16, 1024
KV_BATCH = MAX_BATCH + 1                       # > B: a wrong batch stride lands in a visible row
BATCHES = (1, 2, 3, 4, 5, 8, 9, 13, 16)        # launch_gemv's switch points and the MFMA tile's
H, I, QD, KD = 2048, 16384, 2048, 256
# attended key counts kv_len + 1: the wave's 16-key group, the 32-row V half, the 64-key chunk, the combine's
# 12-chunk register limit (768), the engine's max_chunks (1024)
LKS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 767, 768, 769, 1024)
LOCK_LKS = (2, 17, 33, 64, 65, 768, 769, 1024)
LOCK_BS = (1, 2, 4, 8, 16)
RAGGED16 = (769, 1, 64, 2, 1024, 15, 33, 16, 768, 17, 65, 31, 129, 32, 767, 63)   # sixteen different counts
RAGGED2 = (769, 40)
MASK_LK = 200                                  # chunks of 64, 64, 64 and 8 keys
MASKS = ("random", "chunk", "one")


@lru_cache(maxsize=None)
def model():
    cfg = W.small_config(vision_layers=1, text_layers=2, vocab=V)
    return cfg, W.synthetic_state_dict_f32(cfg, SEED)


def _rng(*key):
    return np.random.default_rng([20251, *key])


def _randn(rng, *shape, scale=1.0):
    return O.bf16(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


@lru_cache(maxsize=None)
def h_rows():
    """16 hidden rows, row scale 0.5 .. 3."""
    return O.bf16(_randn(_rng(1), MAX_BATCH, H) * np.linspace(0.5, 3.0, MAX_BATCH, dtype=np.float32)[:, None])


@lru_cache(maxsize=None)
def act_rows():
    return _randn(_rng(2), MAX_BATCH, I, scale=0.25)


def ssq_of(h):
    """The 16-column partial sums of squares of bf16 rows (what o_proj's epilogue hands to gate|up)."""
    h = np.asarray(h, np.float64)
    return (h * h).reshape(h.shape[0], -1, 16).sum(-1)


# ---------------------------------------------------------------- stage 0 / 1
MAX_POS = 8192
# (name, layer, kv_lens[16], positions[16], ragged): positions 0, 1, kv_len + 1, max_pos - 1; the ragged call has a
# different kv_len per row, positions that are not kv_len + 1, one at max_pos - 1 and one past the table (the clamp)
QKV_CASES = (
    ("pos0", 0, (5,) * 16, (0,) * 16, False),
    ("pos1", 1, (0,) * 16, (1,) * 16, False),
    ("next", 0, (40,) * 16, (41,) * 16, False),
    ("last", 1, (KV_MAX - 1,) * 16, (MAX_POS - 1,) * 16, False),
    ("ragged", 1, tuple((61 * b + 7) % 1023 for b in range(16)),
     tuple([3 * b + 2 for b in range(14)] + [MAX_POS - 1, MAX_POS + 5]), True),
)


@lru_cache(maxsize=None)
def norm_ref(layer):
    """Layer `layer`'s input RMSNorm of h_rows: reference and truth."""
    cfg, P = model()
    w = P[f"language_model.model.layers.{layer}.input_layernorm.weight"]
    return O.rms_norm(h_rows(), w, D.dims(cfg)["eps"]), D._rms64(h_rows(), w, D.dims(cfg)["eps"])


@lru_cache(maxsize=None)
def qkv_ref(case):
    """-> (Rq, Rk, Rv), (Tq, Tk, Tv) for the 16 rows of QKV_CASES[case]."""
    cfg, P = model()
    _, layer, _, pos, _ = QKV_CASES[case]
    return D.ref_stage1(P, cfg, layer, h_rows(), pos), D.truth_stage1(P, cfg, layer, h_rows(), pos)


@lru_cache(maxsize=None)
def ids_rows():
    """17 token ids: vocab - 1 first, the pad id second, none of them the image token."""
    cfg, _ = model()
    ids = _rng(3).integers(3, V - 64, 17)
    ids[0], ids[1] = V - 1, cfg.get("pad_token_id", 0)
    return ids.astype(np.int64)


# ---------------------------------------------------------------- stage 2
@lru_cache(maxsize=None)
def attn_row(Lk, b):
    """Row b's inputs for Lk attended keys: q, K [Lk][256], V [Lk][256], h."""
    r = _rng(4, Lk, b)
    return _randn(r, QD), _randn(r, Lk, KD), _randn(r, Lk, KD), _randn(r, H, scale=0.5 + 0.15 * b)


@lru_cache(maxsize=None)
def mask_row(kind):
    """An additive mask over MASK_LK keys (bf16 values): random finite; one whole 64-key chunk at -inf; every key
    but one at -inf.  (Finite values of scale 1: at scale 2 the bf16 rounding of s + mask, an absolute error in the
    exponent that grows with |s + mask|, put the reference alone at rel-L2 8.1e-3, past CAP_REL.)"""
    m = _randn(_rng(5), MASK_LK, scale=1.0)
    if kind == "chunk":
        m[64:128] = -np.inf
    elif kind == "one":
        keep = m[77]
        m[:] = -np.inf
        m[77] = keep
    return m


@lru_cache(maxsize=None)
def attn_ref(Lk, b, layer, zero_h=False, mask=None, mask_round=True):
    """-> dict Rh, Ra, Th, Ta: stage 2's h and attention output for one row, reference and truth."""
    cfg, P = model()
    q, K, Vv, h = attn_row(Lk, b)
    if zero_h:
        h = np.zeros_like(h)
    kv = np.zeros((2, 2, 1, Lk, KD), np.float32)
    kv[layer, 0, 0], kv[layer, 1, 0] = K, Vv
    masks = None if mask is None else [mask_row(mask)]
    Rh, Ra = D.ref_stage2(P, cfg, layer, q[None], kv, [Lk - 1], h[None], masks, mask_round)
    Th, Ta = D.truth_stage2(P, cfg, layer, q[None], kv, [Lk - 1], h[None], masks, mask_round)
    return dict(Rh=Rh[0], Ra=Ra[0], Th=Th[0], Ta=Ta[0])


# ---------------------------------------------------------------- stage 3, 4, 5
@lru_cache(maxsize=None)
def geglu_ref(layer):
    cfg, P = model()
    return D.ref_stage3(P, cfg, layer, h_rows()), D.truth_stage3(P, cfg, layer, h_rows())


@lru_cache(maxsize=None)
def down_ref(layer):
    """-> (Rh, Rhn), (Th, Thn); hn is None on the last layer."""
    cfg, P = model()
    return D.ref_stage4(P, cfg, layer, act_rows(), h_rows()), D.truth_stage4(P, cfg, layer, act_rows(), h_rows())


@lru_cache(maxsize=None)
def logits_ref():
    cfg, P = model()
    return D.ref_stage5(P, cfg, h_rows()), D.truth_stage5(P, cfg, h_rows())


@lru_cache(maxsize=None)
def tie_rows():
    """16 rows whose final norm points along embedding row 5: with row 5 copied into row 997 that pair is the
    maximum of the logits (Cauchy-Schwarz), and an exact tie."""
    cfg, P = model()
    e = P["language_model.model.embed_tokens.weight"][5].astype(np.float32)
    w = P["language_model.model.norm.weight"].astype(np.float32)
    base = e / (1.0 + w) * 60.0
    return O.bf16(base[None] * np.linspace(1.0, 3.0, MAX_BATCH, dtype=np.float32)[:, None]
                  + _randn(_rng(6), MAX_BATCH, H, scale=0.02))


# ---------------------------------------------------------------- the acceptance conditions
# Caps on the reference's own distance from the truth, for the thresholds below to mean something.  One bf16
# rounding moves an element by at most 2^-9 of itself; a stage rounds its output two to five times and reads
# inputs rounded once, so rel-L2 stays within a few 2^-9 (cap 2^-7) and d = max |x - t| / (|t| + rms t) stays an
# order below the 0.5 a misplaced, stale or swapped element gives: cap 0.05, so that 3 d(R) <= 0.15.
CAP_REL, CAP_D = 2.0 ** -7, 0.05
# The aggregate and per-element conditions see truncation in an epilogue at some rows only (measured on the CPU:
# rel-L2 1.2 .. 1.6 x the reference's, every element within 1 ulp), so a third one sees it at every row:
# round-to-nearest errors have zero mean, so the signed mean error of a row of n elements stays within a few
# standard errors (the reference's rms error / sqrt(n)) of zero, while truncation shifts it by about half an ulp
# (7e-4 .. 1.2e-3 here, 8 to 20 standard errors).  It applies to the GEMV epilogues (q, K, V, act, h, hn,
# logits).  Six standard errors: 2e-9 per row, under 1e-4 over the 2e4 rows the GPU file compares.
BIAS_SE = 6.0
FIGURES = {}


def reference_distances(name, R, T):
    """The reference's rel-L2 and d against the truth, worst row; recorded under `name`."""
    R, T = np.atleast_2d(R), np.atleast_2d(T)
    rel, d = float(D.rel_l2_rows(R, T).max()), float(D.d_rows(R, T).max())
    FIGURES[name] = (rel, d)
    return rel, d


def check(name, G, R, T, ulp=True, bias=None):
    """The conditions of a compared tensor, row by row: rel_l2(G, T) <= 1.5 rel_l2(R, T), d(G) <= 3 d(R), (ulp) at
    least 99 % of the elements within 1 bf16 ulp of R, and (bias; default: as ulp) the signed mean error within
    BIAS_SE standard errors of zero -- not for attention outputs, where one rounded probability moves all 256
    elements of a head together.  Prints each figure before it asserts."""
    G, R, T = np.atleast_2d(np.asarray(G, np.float32)), np.atleast_2d(R), np.atleast_2d(T)
    assert np.isfinite(G).all(), f"{name}: a non-finite output"
    rg, rr = D.rel_l2_rows(G, T), D.rel_l2_rows(R, T)
    dg, dr = D.d_rows(G, T), D.d_rows(R, T)
    frac = D.ulp_frac(G, R, 1) if ulp else 1.0
    i, j = int(np.argmax(rg - 1.5 * rr)), int(np.argmax(dg - 3 * dr))
    print(f"{name}: rel_l2 G {rg[i]:.3e} R {rr[i]:.3e} (row {i}); d G {dg[j]:.3e} R {dr[j]:.3e} (row {j}); "
          f"within 1 ulp of R {frac:.4f}")
    assert (rg <= 1.5 * rr).all(), f"{name}: rel_l2(G, T) {rg[i]:.3e} > 1.5 x rel_l2(R, T) {rr[i]:.3e} at row {i}"
    assert (dg <= 3 * dr).all(), f"{name}: d(G) {dg[j]:.3e} > 3 x d(R) {dr[j]:.3e} at row {j}"
    assert frac >= 0.99, f"{name}: {frac:.4f} of the elements within 1 bf16 ulp of the reference"
    if not (ulp if bias is None else bias):
        return
    bg, se = D.bias_rows(G, T)[0], D.bias_rows(R, T)[1]
    k = int(np.argmax(np.abs(bg) - BIAS_SE * se))
    assert (np.abs(bg) <= BIAS_SE * se).all(), (
        f"{name}: signed mean error {bg[k]:.3e} at row {k}, past {BIAS_SE} standard errors ({se[k]:.3e}) of a "
        f"zero-mean rounding error: truncation?")


def check_norm(name, G, R):
    """An elementwise norm output: within 2 bf16 ulp of R everywhere."""
    assert D.ulp_frac(np.asarray(G, np.float32), R, 2) == 1.0, f"{name}: an element more than 2 ulp off"
