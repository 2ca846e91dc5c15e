"""Inputs of tests/test_cpu_logits.py: the row families, history words, bias row and parameter settings on which
pgmi_logits_process_host and pgmi/logits_np.py are held bit for bit equal -- kept apart from the test so that a
device implementation (left out so far) is held to the same family.  Everything is generated
from seeds; nothing here computes the rule."""
import ctypes

import numpy as np

VS = (77, 2049, 4096, 257216, 300001)
ROWS = (1, 3, 16)
N_FAMILIES = 7


def ks(V):
    return (1, 2, 50, V - 1, V, V + 5)


def kth_largest(row, k):
    return np.partition(row, len(row) - k)[len(row) - k]


def family_row(fam, V, k, rng):
    """One fp32 row of family `fam`; k: the top-k the case runs with (the planted-tie family aims at it)."""
    base = (rng.standard_normal(V) * 3.0).astype(np.float32)
    if fam == 0:    # N(0, 3)
        return base
    if fam == 1:    # all negative
        return (-np.abs(base) - np.float32(0.125)).astype(np.float32)
    if fam == 2:    # all in [1, 2): one exponent, so one histogram bin holds the whole row
        return (1.0 + rng.random(V)).astype(np.float32).clip(1.0, np.nextafter(np.float32(2), np.float32(0)))
    if fam == 3:    # all equal
        return np.full(V, 0.75, np.float32)
    if fam == 4:    # zeros of both signs among a few other values
        return rng.choice(np.array([0.0, -0.0, 1.5, -2.0], np.float32), size=V, p=[0.4, 0.4, 0.1, 0.1])
    if fam == 5:    # -inf entries
        base[rng.random(V) < 0.2] = -np.inf
        return base
    # planted ties at the k-th value: at index 0, at V - 1, and on both sides of a slice boundary
    kk = k if 1 <= k < V else max(1, V // 2)
    t = kth_largest(base, kk)
    for i in (0, V - 1, 2047, 2048):
        if i < V:
            base[i] = t  # never raises the count above t, so t stays the kk-th largest value
    return base


def rows_of(V, rows, k, seed):
    rng = np.random.default_rng([V, rows, k, seed])
    return np.stack([family_row((r + seed) % N_FAMILIES, V, k, rng) for r in range(rows)])


def history_words(V, rows, seed):
    """n_out in 0..5 and a random prompt bit: both signs of x meet seen and unseen words of both kinds."""
    rng = np.random.default_rng([V, rows, seed, 1])
    n_out = rng.integers(0, 6, (rows, V)).astype(np.uint32)
    return n_out | (rng.integers(0, 2, (rows, V)).astype(np.uint32) << np.uint32(31))


def bias_row(V, seed):
    """Mostly zero, a tenth finite, a twentieth banned."""
    rng = np.random.default_rng([V, seed, 2])
    b = np.zeros(V, np.float32)
    r = rng.random(V)
    b[r < 0.10] = rng.standard_normal(int((r < 0.10).sum())).astype(np.float32)
    b[r > 0.95] = -np.inf
    return b


# parameter settings: (name, penalties on, bias on, min_p, temperature, suppress on)
SETTINGS = (
    ("penalties+bias", True, True, 0.0, 1.0, False),
    ("top-k alone", False, False, 0.0, 1.0, False),
    ("min-p", True, False, 0.05, 0.8, False),
    ("suppress+bias", False, True, 0.02, 1.3, True),
)


def case(V, rows, k, seed, setting):
    """-> dict(x, h, bias, emitted, kw) with kw the rule's scalar parameters (numpy names)."""
    from pgmi import logits_np as LN
    _, pen, has_bias, min_p, T, sup = setting
    x = rows_of(V, rows, k, seed)
    kw = dict(rp=1.3 if pen else 1.0, pp=0.4 if pen else 0.0, fp=0.2 if pen else 0.0, top_k=k,
              delta=LN.min_p_delta(min_p, T), suppress_id=(V // 3 if sup else -1), min_new_tokens=(3 if sup else 0))
    emitted = (np.arange(rows, dtype=np.int32) % 5) if sup else None  # rows below and at / past the minimum
    return dict(x=x, h=history_words(V, rows, seed) if pen else None, bias=bias_row(V, seed) if has_bias else None,
                emitted=emitted, kw=kw)


def iter_cases(V):
    """(rows, k, setting name, case) over the family.  Up to V = 4096 every (rows, k, setting); at the two large
    vocabularies every k at 16 rows (each row another family) with penalties + bias, every setting at k = 50, and
    two of the k at 1 and at 3 rows -- the host's sort of a 300,001-entry row is what a test's seconds go to."""
    big = V > 4096
    for rows in ROWS:
        for seed, k in enumerate(ks(V)):
            if big and rows != 16 and seed % 3 != rows % 3:
                continue
            for setting in (SETTINGS if (not big or seed == 2) else SETTINGS[:1]):
                yield rows, k, setting[0], case(V, rows, k, seed, setting)


def host_process(x, h=None, bias=None, emitted=None, *, rp=1.0, pp=0.0, fp=0.0, top_k=0, delta=-np.inf,
                 suppress_id=-1, min_new_tokens=0, expect=0):
    """pgmi_logits_process_host on numpy arrays -> y; expect: the return code the call must give."""
    from pgmi import _native as N
    x = np.ascontiguousarray(x, np.float32)
    rows, V = x.shape
    p = N.PgmiLogitsParams(rp, pp, fp, int(top_k), delta, int(suppress_id), int(min_new_tokens))
    y = np.empty_like(x)
    keep =[None if a is None else np.ascontiguousarray(a, dt)
            for a, dt in ((h, np.uint32), (bias, np.float32), (emitted, np.int32))]
    rc = N.lib().pgmi_logits_process_host(x.ctypes.data_as(ctypes.c_void_p), rows, V,
                                          *(None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in keep[:2]),
                                          ctypes.byref(p),
                                          None if keep[2] is None else keep[2].ctypes.data_as(ctypes.c_void_p),
                                          y.ctypes.data_as(ctypes.c_void_p))
    assert rc == expect, (rc, N.lib().pgmi_last_error())
    return y


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))
