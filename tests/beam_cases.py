"""Inputs of tests/test_cpu_beam.py: the logits rows, running scores and stop tokens on which pgmi_beam_step_host and
pgmi/beam_np.py are held bit for bit equal -- kept apart from the test so that a device step (left
out so far) is held to the same family -- and the host rule's ctypes wrapper.  Everything is generated from seeds."""
import ctypes

import numpy as np

GKS = ((1, 1), (1, 2), (1, 4), (2, 3), (4, 4), (2, 8), (1, 16))
SLICE = 2048  # the device's first pass works on slices of this many elements
FAMILIES = ("normal", "all equal", "identical rows", "-inf entries", "top C in one slice", "one per slice",
            "slice boundaries")
EOS_MODES = ("none", "rank 0", "rank in [K, 2K)", "every row")
LAYOUT_NAMES = ("den", "run", "heur", "frozen", "pool_score", "pool_valid", "pool_step", "pool_parent", "pool_token",
                "hist_parent", "hist_token", "state_words", "total_words", "nb")


def rows_for(fam, V, G, K, rows_in, rng):
    """fp32 (G * rows_in, V) of family `fam`, and the running scores fp32 (G * K)."""
    C = 2 * K
    rows = G * rows_in
    x = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    run = (-np.abs(rng.standard_normal(G * K)) * 2.0).astype(np.float32)
    run[::K] = 0.0
    if fam == 1:
        x[:] = np.float32(0.75)
    elif fam == 2:    # one row and one running score per group: only the row index can order the candidates
        for g in range(G):
            x[g * rows_in:(g + 1) * rows_in] = x[g * rows_in]
            run[g * K:(g + 1) * K] = run[g * K + K - 1]
    elif fam == 3:
        x[rng.random((rows, V)) < 0.3] = -np.inf
        x[:, :2][x[:, :2] == 0] = -0.0
    elif fam >= 4:    # C + 2 large values, in equal pairs, at chosen places
        n_sl = (V + SLICE - 1) // SLICE
        for r in range(rows):
            if fam == 4:
                s0 = int(rng.integers(0, n_sl))
                lo, hi = s0 * SLICE, min(V, (s0 + 1) * SLICE)
                at = rng.choice(np.arange(lo, hi), size=min(C + 2, hi - lo), replace=False)
            elif fam == 5:
                at = np.array([(j % n_sl) * SLICE + (j // n_sl) * 7 + int(rng.integers(0, 5)) for j in range(C + 2)])
            else:
                at = np.array([0, V - 1] + [b + d for b in range(SLICE, V, SLICE) for d in (-1, 0)][:C])
            at = np.unique(at[(at >= 0) & (at < V)])
            rng.shuffle(at)
            x[r, at] = (20.0 + (np.arange(len(at)) // 2)).astype(np.float32)
    return x, run


def pick_eos(mode, x, run, G, K, rows_in):
    """The stop token of an eos mode; x may be edited (mode 3 plants the token on top of every row)."""
    from pgmi import beam_np as BN
    if mode == 0:
        return -1
    if mode == 3:
        e = x.shape[1] // 2
        x[:, e] = np.where(np.isfinite(x.max(1)), x.max(1), 0) + np.float32(1.0)
        return e
    st = BN.BeamState(G, K, 4)  # the candidates' order without a stop token (t = 0 of 4: nothing hits)
    st.run[:] = run
    BN.beam_step_np(st, x, rows_in, 0)
    # with no hit the running beams are candidates 0 .. K - 1; rank in [K, 2K) is whatever follows in a second pick
    if mode == 1:
        return int(st.hist_token[0, 0])
    st2 = BN.BeamState(G, K, 4, eos=int(st.hist_token[0, 0]))
    st2.run[:] = run
    BN.beam_step_np(st2, x, rows_in, 0)
    return int(st2.hist_token[0, K - 1])  # candidate K or later of the first order


VS = (0, 77, 2049, 4099, 257216)  # 0: V = 2K, the smallest the rule takes


def iter_cases(V):
    """(name, G, K, rows_in, x, run, eos) over the family; V = 0 stands for V = 2K.  Up to V = 4099 every (G, K),
    rows_in, family and stop-token mode; at 257,216 every (G, K) and rows_in with the family and the mode rotating --
    sixteen rows of a quarter of a million entries are what a test's seconds go to."""
    big = V > 4099
    n = 0
    for G, K in GKS:
        Vv = 2 * K if V == 0 else V
        if Vv < 2 * K:
            continue
        for rows_in in ((1, K) if K > 1 else (1,)):
            for fam in range(len(FAMILIES)):
                for mode in range(len(EOS_MODES)):
                    n += 1
                    if big and (n % 9) != 0 and not (fam == 0 and mode == 0):
                        continue
                    rng = np.random.default_rng([Vv, G, K, rows_in, fam, mode])
                    x, run = rows_for(fam, Vv, G, K, rows_in, rng)
                    eos = pick_eos(mode, x, run, G, K, rows_in)
                    yield f"{FAMILIES[fam]} / eos {EOS_MODES[mode]}", G, K, rows_in, x, run, eos


def layout(G, K, n_tokens, V):
    from pgmi import _native as N
    out = (ctypes.c_int64 * 14)()
    N.check(N.lib().pgmi_beam_state_layout(G, K, n_tokens, V, out, 14), "pgmi_beam_state_layout")
    return dict(zip(LAYOUT_NAMES, (int(v) for v in out)))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostBeam:
    """pgmi_beam_reset_host / pgmi_beam_step_host on a numpy blob."""

    def __init__(self, G, K, n_tokens, V, eos=-1, early=False, den=None, length_penalty=1.0):
        from pgmi import _native as N
        from pgmi import beam_np as BN
        self.N, self.BN = N, BN
        self.G, self.K, self.n_tokens, self.V, self.eos, self.early = G, K, n_tokens, V, eos, early
        self.lay = layout(G, K, n_tokens, V)
        self.words = np.zeros(self.lay["state_words"], np.int32)
        self.den = BN.den_table(n_tokens, length_penalty) if den is None else np.ascontiguousarray(den, np.float32)
        N.check(N.lib().pgmi_beam_reset_host(_p(self.words), G, K, n_tokens, V, eos, int(early), _p(self.den)),
                "pgmi_beam_reset_host")

    def set_run(self, run):
        o = self.lay["run"]
        self.words[o:o + self.G * self.K] = np.ascontiguousarray(run, np.float32).view(np.int32)

    def step(self, logits, rows_in, t, lse=None, expect=0):
        x = np.ascontiguousarray(logits, np.float32)
        ids = np.full(self.G * self.K, -7, np.int64)
        par = np.full(self.G * self.K, -7, np.int32)
        n_open = np.zeros(1, np.int32)
        lse_out = np.zeros(x.shape[0], np.float32)
        lse = None if lse is None else np.ascontiguousarray(lse, np.float32)
        rc = self.N.lib().pgmi_beam_step_host(_p(self.words), _p(x), rows_in, t, _p(lse), _p(ids), _p(par), _p(n_open),
                                              _p(lse_out))
        assert rc == expect, (rc, self.N.lib().pgmi_last_error())
        return ids, par, int(n_open[0]), lse_out

    def state(self):
        return self.BN.BeamState.from_words(self.words, self.lay, self.G, self.K, self.n_tokens, self.eos, self.early)


def same_state(a, b):
    """Every field of two BeamStates, bit for bit; returns the first field that differs, or None."""
    for name in ("den",) + a.FIELDS:
        u, v = getattr(a, name), getattr(b, name)
        if u.shape != v.shape or not np.array_equal(u.view(np.int32), v.view(np.int32)):
            return name
    return None
