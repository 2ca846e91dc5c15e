"""Rows and numpy fp32 emulations for the in-register cross-lane reductions (csrc/common.h; the hook is
pgmi_debug_lane_reduce).  A reduction over the 64 lanes of a wave is the xor butterfly
v[l] = op(v[l], v[l ^ o]) for o in a fixed order, every lane holding a result; the emulation is that
definition, in numpy float32 (IEEE round-to-nearest-even adds, as the GPU's).

Rows hold no NaN and never +inf with -inf (an invalid sum's NaN sign differs between hosts and the GPU), and no
+0.0 beside -0.0 as the only maxima (fmaxf of the two is either)."""
import numpy as np

SEED = 20261021
LANES = np.arange(64)
DESC = (32, 16, 8, 4, 2, 1)
ASC = (1, 2, 4, 8, 16, 32)
ROW16_ASC = (1, 2, 4, 8)
QUARTERS = (16, 32)

# op id of pgmi_debug_lane_reduce -> (kind, xor offsets in order)
OPS = {
    0: ("sum", DESC),
    1: ("max", DESC),
    2: ("first_max", DESC),
    3: ("sum", ROW16_ASC),
    4: ("sum", ASC),
    5: ("sum", QUARTERS),
    6: ("first_max", ROW16_ASC),
    7: ("max", ROW16_ASC),
}


def random_rows(n=1024):
    """standard normal x 2^U[-12, 12]: magnitudes spread over 24 binades, so a sum's bits depend on its order"""
    g = np.random.default_rng(SEED)
    x = g.standard_normal((n, 64)) * np.exp2(g.uniform(-12.0, 12.0, (n, 64)))
    return np.ascontiguousarray(x, np.float32)


def special_rows():
    """12 rows (three workgroups): infinities, -0.0, denormals, equal maxima at different lanes"""
    g = np.random.default_rng(SEED + 1)
    base = g.standard_normal((12, 64)).astype(np.float32)
    r = base.copy()
    r[0, 17] = np.inf                                   # one +inf
    r[1, [3, 40]] = np.inf                              # two +inf, one per half
    r[2, 62] = -np.inf                                  # one -inf
    r[3, :] = -np.inf                                   # all -inf (a fully masked score row)
    r[4, :] = -0.0                                      # all -0.0: sum and max stay -0.0
    r[5] = -np.abs(base[5]); r[5, [0, 9, 33]] = -0.0     # -0.0 the maximum among negatives, three times
    r[6, :] = -0.0; r[6, 0::2] = base[6, 0::2]; r[6, 1::2] = -base[6, 0::2]   # x, -x pairs cancel to +0.0
    r[7] = (g.integers(-(1 << 20), 1 << 20, 64) * np.float64(2.0 ** -149)).astype(np.float32)   # denormals only
    r[8, 0::3] = r[7, 0::3]                             # denormals beside normal values
    r[9] = -np.abs(base[9]); r[9, [5, 37, 63]] = 2.5     # equal maxima at lanes 5, 37, 63
    r[10, :] = 1.25                                     # all equal
    r[11] = -np.abs(base[11]); r[11, 63] = 3.0; r[11, 48] = 3.0; r[11, 15] = 3.0 - 2.0 ** -22   # a near miss lower
    assert not np.isnan(r).any()
    return np.ascontiguousarray(r, np.float32)


def xor_tree(x, kind, offsets):
    """every lane's result of the butterfly over `offsets`; kind first_max -> (values, int32 indices)"""
    v = np.array(x, np.float32, copy=True)
    if kind == "first_max":
        ix = np.broadcast_to(LANES.astype(np.int32), v.shape).copy()
        for o in offsets:
            v2, i2 = v[:, LANES ^ o], ix[:, LANES ^ o]
            take = (v2 > v) | ((v2 == v) & (i2 < ix))
            v, ix = np.where(take, v2, v), np.where(take, i2, ix)
        return v, ix
    for o in offsets:
        p = v[:, LANES ^ o]
        v = (v + p).astype(np.float32) if kind == "sum" else np.maximum(v, p)
    return v


def sequential_sum(x):
    s = np.zeros(x.shape[0], np.float32)
    for l in range(64):
        s = (s + x[:, l]).astype(np.float32)
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)
