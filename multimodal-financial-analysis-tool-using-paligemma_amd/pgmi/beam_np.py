"""The beam-search rule of csrc/beam_rule.h in numpy -- the second statement of the rule, held
bit for bit equal to pgmi_beam_step_host by tests/test_cpu_beam.py, and equal to transformers' _beam_search
(do_sample=False, one stop token, early_stopping in {False, True}) on a small model.

G groups (prompts) of K beams, C = 2K candidates per step, steps t = 0 .. n_tokens - 1; t = 0 picks from the
prefill's logits (one row per group).  For input row r of a group, lse_r = fp32 log-sum-exp of the row (an input of
the rule: the caller's, or float64 rounded once) and run_r its running score (0 after a reset):
  score     s = fp32(fp32(x - lse_r) + run_r), x's -0 taken as +0
  order     in a row (x descending, token ascending); in a group (s descending, row ascending, in-row rank
            ascending); the first C are the step's candidates
  hit_j     token_j == eos, or t == n_tokens - 1
  running   the first K candidates with hit = 0 (on the last step: the first K candidates), each (parent row, token, s)
  pool      K slots per group; unless the group is frozen a candidate with hit_j and j < K enters with
            fp32(s / den[t + 1]), den[n] = fp32(float64(n) ** length_penalty); the best K of old and new stay: score
            descending, old before new, then candidate rank; empty slots lose to everything
  freeze    heur &= fp32(run_best / den[t + 1]) > worst (the smallest score of a full pool, else -inf); frozen once
            heur is false, and with early_stopping once the pool is full; a frozen group's pool never changes
  history   parent[t][row], token[t][row] of the running beams; pool slots (step, parent row, token) point into it
            and backtrack_np walks them back."""
from __future__ import annotations

import numpy as np

NEG_INF = np.float32(-np.inf)


def den_table(n_tokens: int, length_penalty: float) -> np.ndarray:
    """den[n] = fp32(float64(n) ** length_penalty), n = 0 .. n_tokens (den[0] is never read)."""
    d = np.ones(n_tokens + 1, dtype=np.float64)
    for n in range(1, n_tokens + 1):
        d[n] = float(n) ** float(length_penalty)
    return d.astype(np.float32)


class BeamState:
    """The state of a search: what pgmi_beam_reset writes, as arrays."""

    def __init__(self, G: int, K: int, n_tokens: int, eos=None, length_penalty: float = 1.0,
                 early_stopping: bool = False, den=None):
        if G < 1 or K < 1 or n_tokens < 1:
            raise ValueError("beam: G, K and n_tokens must be >= 1")
        self.G, self.K, self.n_tokens = G, K, n_tokens
        self.eos = -1 if eos is None else int(eos)
        self.early = bool(early_stopping)
        self.den = den_table(n_tokens, length_penalty) if den is None else np.asarray(den, np.float32)
        GK = G * K
        self.run = np.zeros(GK, np.float32)
        self.heur = np.ones(G, np.int32)
        self.frozen = np.zeros(G, np.int32)
        self.pool_score = np.full(GK, NEG_INF, np.float32)
        self.pool_valid = np.zeros(GK, np.int32)
        self.pool_step = np.zeros(GK, np.int32)
        self.pool_parent = np.zeros(GK, np.int32)
        self.pool_token = np.zeros(GK, np.int32)
        self.hist_parent = np.full((n_tokens, GK), -1, np.int32)
        self.hist_token = np.full((n_tokens, GK), -1, np.int32)

    FIELDS = ("run", "heur", "frozen", "pool_score", "pool_valid", "pool_step", "pool_parent", "pool_token",
              "hist_parent", "hist_token")

    @classmethod
    def from_words(cls, words, offsets: dict, G: int, K: int, n_tokens: int, eos=None, early_stopping=False):
        """The state held in a blob of 4-byte words (pgmi_beam_state_layout's offsets by field name)."""
        w = np.ascontiguousarray(words).view(np.int32)
        st = cls(G, K, n_tokens, eos, 1.0, early_stopping, den=w[offsets["den"]: offsets["den"] + n_tokens + 1]
                 .view(np.float32).copy())
        GK = G * K
        for name in cls.FIELDS:
            n = {"heur": G, "frozen": G, "hist_parent": n_tokens * GK, "hist_token": n_tokens * GK}.get(name, GK)
            a = w[offsets[name]: offsets[name] + n].copy()
            if name in ("run", "pool_score"):
                a = a.view(np.float32)
            setattr(st, name, a.reshape(n_tokens, GK) if name.startswith("hist") else a)
        return st


def lse_np(logits) -> np.ndarray:
    """Each row's log-sum-exp in float64, rounded once to fp32."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        m = x.max(1)
        ms = np.where(np.isfinite(m), m, 0.0)
        return (m + np.log(np.exp(x - ms[:, None]).sum(1))).astype(np.float32)


def _row_top(x, C):
    """The row's first C token indices by (x descending, token ascending)."""
    V = x.shape[0]
    if V > 4 * C:
        kth = np.partition(x, V - C)[V - C]
        idx = np.nonzero(x >= kth)[0]  # everything tied at the C-th value is kept for the order to decide
        if idx.size < C:               # (a row with NaN: outside the rule)
            idx = np.arange(V)
    else:
        idx = np.arange(V)
    order = np.lexsort((idx, -x[idx]))
    return idx[order[:C]]


def beam_step_np(st: BeamState, logits, rows_in: int, t: int, lse=None):
    """One step on st (updated in place).  logits fp32 (G * rows_in, V), rows_in 1 or K.  Returns (next_ids int64
    (G * K), parent int32 (G * K), n_open, lse fp32 (G * rows_in))."""
    G, K = st.G, st.K
    C = 2 * K
    x = np.asarray(logits, np.float32)
    if x.ndim != 2 or x.shape[0] != G * rows_in or rows_in not in (1, K):
        raise ValueError("beam_step: logits are (G * rows_in, V) with rows_in 1 or K")
    V = x.shape[1]
    if V < C:
        raise ValueError("beam_step: V >= 2K")
    if not 0 <= t < st.n_tokens:
        raise ValueError("beam_step: step outside [0, n_tokens)")
    x = np.where(x == 0, np.float32(0), x)  # -0 -> +0
    lse = lse_np(x) if lse is None else np.asarray(lse, np.float32).reshape(-1)
    last = t == st.n_tokens - 1
    d = st.den[t + 1]
    next_ids = np.zeros(G * K, np.int64)
    parent = np.zeros(G * K, np.int32)
    for g in range(G):
        o = g * K
        s_all, row_all, rank_all, tok_all = [], [], [], []
        for r in range(rows_in):
            xr = x[g * rows_in + r]
            tok = _row_top(xr, C)
            with np.errstate(all="ignore"):
                s = ((xr[tok] - lse[g * rows_in + r]).astype(np.float32) + st.run[o + r]).astype(np.float32)
            s_all.append(s)
            row_all.append(np.full(C, r))
            rank_all.append(np.arange(C))
            tok_all.append(tok)
        s_all, row_all = np.concatenate(s_all), np.concatenate(row_all)
        rank_all, tok_all = np.concatenate(rank_all), np.concatenate(tok_all)
        first = np.lexsort((rank_all, row_all, -s_all))[:C]
        cs, crow, ct = s_all[first], row_all[first], tok_all[first]
        hit = np.full(C, True) if last else ct == st.eos
        keep = np.concatenate([np.nonzero(~hit)[0], np.nonzero(hit)[0]])[:K]  # (hits only on the last step)
        st.run[o:o + K] = cs[keep]
        next_ids[o:o + K] = ct[keep]
        parent[o:o + K] = o + crow[keep]
        st.hist_parent[t, o:o + K] = o + crow[keep]
        st.hist_token[t, o:o + K] = ct[keep]
        if not st.frozen[g]:
            merged = [(st.pool_score[o + i], st.pool_step[o + i], st.pool_parent[o + i], st.pool_token[o + i])
                      for i in range(K) if st.pool_valid[o + i]]
            with np.errstate(all="ignore"):
                merged += [(np.float32(cs[j] / d), t, o + crow[j], ct[j]) for j in range(K) if hit[j]]
            merged = sorted(merged, key=lambda e: -e[0])[:K]  # stable: old before new, then candidate rank
            for i, e in enumerate(merged):
                st.pool_score[o + i], st.pool_step[o + i], st.pool_parent[o + i], st.pool_token[o + i] = e
                st.pool_valid[o + i] = 1
        full = bool(st.pool_valid[o:o + K].all())
        worst = st.pool_score[o:o + K].min() if full else NEG_INF
        with np.errstate(all="ignore"):
            if not np.float32(st.run[o] / d) > worst:
                st.heur[g] = 0
        if not st.heur[g] or (st.early and full):
            st.frozen[g] = 1
    return next_ids, parent, int((st.frozen == 0).sum()), lse


def backtrack_np(st: BeamState, num_return_sequences: int = 1, pad=None):
    """The pool's first R hypotheses of every group: (sequences int64 (G, R, n) padded with `pad` (default: eos, or 0
    without one) after each hypothesis' last token, scores fp32 (G, R) descending, lengths int64 (G, R) counting the
    eos), n the longest returned hypothesis."""
    G, K, R = st.G, st.K, num_return_sequences
    if not 1 <= R <= K:
        raise ValueError("backtrack: 1 <= num_return_sequences <= K")
    if pad is None:
        pad = st.eos if st.eos >= 0 else 0
    seqs = np.full((G, R, st.n_tokens), int(pad), np.int64)
    scores = np.full((G, R), NEG_INF, np.float32)
    lengths = np.zeros((G, R), np.int64)
    for g in range(G):
        for i in range(R):
            slot = g * K + i
            if not st.pool_valid[slot]:
                continue
            step, row = int(st.pool_step[slot]), int(st.pool_parent[slot])
            seqs[g, i, step] = st.pool_token[slot]
            for u in range(step - 1, -1, -1):
                seqs[g, i, u] = st.hist_token[u, row]
                row = int(st.hist_parent[u, row])
            scores[g, i] = st.pool_score[slot]
            lengths[g, i] = step + 1
    return seqs[:, :, :max(1, int(lengths.max()))], scores, lengths


def beam_search_np(step_logits_fn, G: int, K: int, n_tokens: int, eos=None, length_penalty: float = 1.0,
                   early_stopping: bool = False, num_return_sequences: int = 1, pad=None, step_fn=beam_step_np):
    """A whole search.  step_logits_fn(t, ids, parent) returns the logits step t picks from: at t = 0 (ids and parent
    None) the prefill's (G, V); later (G * K, V) for the beams `ids` int64 (G * K), each continuing the row
    parent[b] of the step before -- the callback reorders whatever cache it keeps.  Ends after n_tokens steps, or
    once every group is frozen.  Returns backtrack_np's triple and the final state."""
    st = BeamState(G, K, n_tokens, eos, length_penalty, early_stopping)
    ids = parent = None
    for t in range(n_tokens):
        logits = step_logits_fn(t, ids, parent)
        ids, parent, n_open, _ = step_fn(st, logits, 1 if t == 0 else K, t)
        if n_open == 0:
            break
    return backtrack_np(st, num_return_sequences, pad) + (st,)
