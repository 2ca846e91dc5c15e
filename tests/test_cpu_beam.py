"""The beam-search rule (csrc/beam_rule.h) without a GPU:

1. pgmi_beam_step_host (the C statement, compiled from the header a device step is to use) equals pgmi/beam_np.py (the numpy
   statement) bit for bit over the family of tests/beam_cases.py -- next ids, parents, running scores, pool, flags,
   history -- and over consecutive steps with length_penalty in {0, 1, 2} and both early_stopping values.
2. beam_search_np equals transformers' generate(num_beams=K, do_sample=False) on a small random Gemma: sequences
   equal, sequences_scores within (t + 4) * 2^-23 * max(1, |score|) for a hypothesis of t steps (one fp32 rounding
   per step and the log-softmax's own).  The seeds are fixed so that a float64 restatement of the rule sees no
   decision closer than 1e-3; the test asserts that margin.
3. A group's result is the same alone and inside a batch; every refused argument is refused."""
import ctypes

import numpy as np
import pytest

import beam_cases as C
from pgmi import beam_np as BN


def _np_state(G, K, n_tokens, eos, early=False, length_penalty=1.0, run=None):
    st = BN.BeamState(G, K, n_tokens, eos, length_penalty, early)
    if run is not None:
        st.run[:] = run
    return st


@pytest.mark.parametrize("V", C.VS)
def test_host_rule_equals_numpy_rule(V):
    n = 0
    for name, G, K, rows_in, x, run, eos in C.iter_cases(V):
        what = (V, G, K, rows_in, name)
        lse = BN.lse_np(x)
        for t, n_tokens in ((0, 3), (2, 3)):  # a middle step, and the last one
            hb = C.HostBeam(G, K, n_tokens, x.shape[1], eos)
            hb.set_run(run)
            st = _np_state(G, K, n_tokens, eos, run=run)
            ids, par, n_open, _ = hb.step(x, rows_in, t, lse)
            ids2, par2, n_open2, _ = BN.beam_step_np(st, x, rows_in, t, lse)
            assert np.array_equal(ids, ids2) and np.array_equal(par, par2) and n_open == n_open2, what
            assert C.same_state(hb.state(), st) is None, (what, C.same_state(hb.state(), st))
            assert ids.min() >= 0 and ids.max() < x.shape[1] and par.min() >= 0 and par.max() < G * K, what
            assert all(par[b] // K == b // K for b in range(G * K)), what  # a parent is a row of the same group
            if t == 2:  # the last step finishes the first K candidates: the pool is full, and they run on
                assert st.pool_valid.all() and (st.pool_step == 2).all(), what
                assert np.array_equal(st.pool_token, ids) and np.array_equal(st.pool_parent, par), what
            elif eos < 0:
                assert not st.pool_valid.any(), what
        n += 1
    assert n >= 14


def test_host_lse_is_the_float64_one():
    """Without an lse the host takes its own: fp64, rounded once -- within one fp32 ulp of numpy's (the two sum in
    another order), and the step it drives equals the numpy step given the same lse."""
    for V, G, K in ((77, 2, 3), (4099, 1, 4), (257216, 1, 2)):
        x = (np.random.default_rng(V).standard_normal((G * K, V)) * 3).astype(np.float32)
        x[0, ::3] = -np.inf
        hb = C.HostBeam(G, K, 4, V)
        ids, par, _, lse = hb.step(x, K, 1)
        want = BN.lse_np(x)
        assert np.all(np.abs(lse - want) <= 2.0 ** -23 * np.maximum(1, np.abs(want)))
        st = _np_state(G, K, 4, -1)
        ids2, par2, _, _ = BN.beam_step_np(st, x, K, 1, lse)
        assert np.array_equal(ids, ids2) and np.array_equal(par, par2) and C.same_state(hb.state(), st) is None


def _eos_heavy_logits(rng, rows, V, eos):
    x = (rng.standard_normal((rows, V)) * 2).astype(np.float32)
    x[:, eos] += np.float32(5.0)  # the stop token is at or near the top of most rows
    return x


@pytest.mark.parametrize("early", (False, True))
@pytest.mark.parametrize("length_penalty", (0.0, 1.0, 2.0))
def test_pool_merge_and_freeze_over_steps(length_penalty, early):
    V, n_tokens, eos = 77, 9, 5
    seen_frozen = seen_pool = 0
    for G, K in ((1, 1), (1, 4), (2, 3), (4, 4), (1, 16)):
        rng = np.random.default_rng([G, K, int(length_penalty), int(early)])
        hb = C.HostBeam(G, K, n_tokens, V, eos, early, length_penalty=length_penalty)
        st = _np_state(G, K, n_tokens, eos, early, length_penalty)
        for t in range(n_tokens):
            x = _eos_heavy_logits(rng, G * (1 if t == 0 else K), V, eos)
            lse = BN.lse_np(x)
            before = hb.state()
            ids, par, n_open, _ = hb.step(x, 1 if t == 0 else K, t, lse)
            ids2, par2, n_open2, _ = BN.beam_step_np(st, x, 1 if t == 0 else K, t, lse)
            after = hb.state()
            assert np.array_equal(ids, ids2) and np.array_equal(par, par2) and n_open == n_open2, (G, K, t)
            assert C.same_state(after, st) is None, (G, K, t, C.same_state(after, st))
            assert n_open == int((after.frozen == 0).sum())
            for g in range(G):
                sl = slice(g * K, (g + 1) * K)
                if before.frozen[g]:  # a frozen group's pool and flags stay as they were
                    seen_frozen += 1
                    assert after.frozen[g] == 1
                    for f in ("pool_score", "pool_valid", "pool_step", "pool_parent", "pool_token"):
                        assert np.array_equal(getattr(before, f)[sl].view(np.int32), getattr(after, f)[sl].view(np.int32))
                sc, va = after.pool_score[sl], after.pool_valid[sl]
                assert np.all(va[:-1] >= va[1:]) and np.all(sc[:-1][va[1:] == 1] >= sc[1:][va[1:] == 1])
                seen_pool += int(va.sum() > 0 and t < n_tokens - 1)
                if early and va.all():
                    assert after.frozen[g] == 1
        assert st.pool_valid.all()  # the last step fills what the stop token left open
        assert np.all(st.hist_parent >= 0) and np.all(st.hist_token >= 0)
    assert seen_frozen > 0 and seen_pool > 0


def test_a_group_is_the_same_alone_and_in_a_batch():
    V, K, n_tokens, eos = 2049, 3, 5, 11
    rng = np.random.default_rng(7)
    steps = [_eos_heavy_logits(rng, 3 * (1 if t == 0 else K), V, eos) for t in range(n_tokens)]
    both = _np_state(3, K, n_tokens, eos, length_penalty=2.0)
    alone = [_np_state(1, K, n_tokens, eos, length_penalty=2.0) for _ in range(3)]
    for t, x in enumerate(steps):
        r = 1 if t == 0 else K
        ids, par, _, _ = BN.beam_step_np(both, x, r, t)
        for g in range(3):
            ids1, par1, _, _ = BN.beam_step_np(alone[g], x[g * r:(g + 1) * r], r, t)
            assert np.array_equal(ids[g * K:(g + 1) * K], ids1) and np.array_equal(par[g * K:(g + 1) * K] - g * K, par1)
    seqs, scores, lengths = BN.backtrack_np(both, K)
    for g in range(3):
        s1, sc1, l1 = BN.backtrack_np(alone[g], K)
        n = s1.shape[2]
        assert np.array_equal(seqs[g, :, :n], s1[0]) and np.all(seqs[g, :, n:] == eos)
        assert np.array_equal(scores[g].view(np.int32), sc1[0].view(np.int32)) and np.array_equal(lengths[g], l1[0])
        assert np.all(scores[g][:-1] >= scores[g][1:])


def test_refused_arguments():
    from pgmi import _native as N
    L = N.lib()
    den = np.ones(8, np.float32)
    buf = np.zeros(1 << 16, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # (G, K, n_tokens, V, eos): K outside 1..16, G * K > 16, no tokens, V < 2K, eos outside the vocabulary
    for G, K, n, V, eos in ((1, 0, 4, 64, -1), (1, 17, 4, 64, -1), (3, 6, 4, 64, -1), (0, 2, 4, 64, -1),
                            (1, 2, 0, 64, -1), (1, 4, 4, 7, -1), (1, 2, 4, 64, 64), (1, 2, 4, 64, -2)):
        assert L.pgmi_beam_reset_host(p(buf), G, K, n, V, eos, 0, p(den)) == N.PGMI_E_ARG, (G, K, n, V, eos)
        if eos == -1:
            assert L.pgmi_beam_state_bytes(G, K, n, V) == -1
            assert L.pgmi_beam_state_layout(G, K, n, V, (ctypes.c_int64 * 14)(), 14) == N.PGMI_E_ARG
    assert L.pgmi_beam_state_bytes(4, 4, 64, 257216) > 0
    assert L.pgmi_beam_reset_host(None, 1, 2, 4, 64, -1, 0, p(den)) == N.PGMI_E_ARG
    assert L.pgmi_beam_reset_host(p(buf), 1, 2, 4, 64, -1, 0, None) == N.PGMI_E_ARG
    hb = C.HostBeam(2, 3, 4, 64)
    x = np.zeros((6, 64), np.float32)
    hb.step(x, 2, 1, expect=N.PGMI_E_ARG)      # rows_in is 1 or K
    hb.step(x, 3, 4, expect=N.PGMI_E_ARG)      # step outside [0, n_tokens)
    hb.step(x, 3, -1, expect=N.PGMI_E_ARG)
    ids, par = np.zeros(6, np.int64), np.zeros(6, np.int32)
    assert L.pgmi_beam_step_host(p(hb.words), None, 3, 1, None, p(ids), p(par), None, None) == N.PGMI_E_ARG
    assert L.pgmi_beam_step_host(p(hb.words), p(x), 3, 1, None, None, p(par), None, None) == N.PGMI_E_ARG
    assert L.pgmi_beam_step_host(p(np.zeros(64, np.int32)), p(x), 3, 1, None, p(ids), p(par), None, None) == \
        N.PGMI_E_ARG  # a state that was never reset
    st = BN.BeamState(2, 3, 4)
    for bad in (dict(rows_in=2, t=1), dict(rows_in=3, t=4), dict(rows_in=3, t=-1)):
        with pytest.raises(ValueError):
            BN.beam_step_np(st, x, **bad)
    with pytest.raises(ValueError):
        BN.beam_step_np(BN.BeamState(1, 4, 4), np.zeros((4, 7), np.float32), 4, 1)  # V < 2K
    with pytest.raises(ValueError):
        BN.backtrack_np(st, 4)  # more sequences than beams
    with pytest.raises(ValueError):
        BN.BeamState(1, 0, 4)


# ---------------------------------------------------------------- against transformers' beam search
HF_VOCAB, HF_PROMPT, HF_TOKENS = 97, 5, 7
# chosen by a search over seeds for the smallest float64 margin below (1.1e-3 over all 120 settings); the first stop
# token ends hypotheses of this model early, the second is never among its candidates
HF_MODEL_SEED, HF_PROMPT_SEED = 0, 2
HF_EOS_EMITTED, HF_EOS_NEVER = 33, 96
MARGIN = 1e-3


def _tiny_gemma(seed):
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    cfg = tf.GemmaConfig(vocab_size=HF_VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                         num_attention_heads=2, num_key_value_heads=1, head_dim=16, max_position_embeddings=64,
                         pad_token_id=0, eos_token_id=None, bos_token_id=None, attn_implementation="eager")
    model = tf.GemmaForCausalLM(cfg).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():  # a spread of logits a default initialisation does not give
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if "norm" in name else 0.45))
    return torch, model


def _prompts(G):
    return np.random.default_rng([HF_PROMPT_SEED, G]).integers(1, HF_VOCAB, (G, HF_PROMPT))


class _ModelSteps:
    """beam_search_np's callback on the transformers model, run as generate runs it: the prompt expanded to G * K
    rows and prefilled once, then one cached token per step after cache.reorder_cache(parent)."""

    def __init__(self, torch, model, prompts, K):
        self.torch, self.model, self.K = torch, model, K
        self.ids = torch.from_numpy(np.repeat(prompts, K, axis=0))
        self.cache = None

    def __call__(self, t, ids, parent):
        torch = self.torch
        with torch.no_grad():
            if t == 0:
                out = self.model(input_ids=self.ids, attention_mask=torch.ones_like(self.ids), use_cache=True)
                self.cache = out.past_key_values
                return out.logits[::self.K, -1].float().numpy()
            par = torch.from_numpy(parent.astype(np.int64))
            self.cache.reorder_cache(par)
            self.ids = torch.cat([self.ids[par], torch.from_numpy(ids)[:, None]], 1)
            out = self.model(input_ids=self.ids[:, -1:], attention_mask=torch.ones_like(self.ids),
                             past_key_values=self.cache, use_cache=True)
            return out.logits[:, -1].float().numpy()


class _Margins:
    """beam_step_np, and beside it the smallest float64 gap at any of the step's decisions: candidate j against
    j + 1 for j < C (the C-th against the first left out included), neighbours in the pool's merge, and the
    freeze's comparison."""

    def __init__(self):
        self.least = np.inf

    def __call__(self, st, logits, rows_in, t, lse=None):
        G, K = st.G, st.K
        Cn = 2 * K
        x = np.asarray(logits, np.float64)
        lp = x - (x.max(1, keepdims=True) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)))
        d = float(st.den[t + 1])
        frozen = st.frozen.copy()
        pool = [[float(st.pool_score[g * K + i]) for i in range(K) if st.pool_valid[g * K + i]] for g in range(G)]
        for g in range(G):
            s = (lp[g * rows_in:(g + 1) * rows_in] + st.run[g * K:g * K + rows_in, None].astype(np.float64)).ravel()
            top = np.sort(s)[::-1][:Cn + 1]
            self.least = min(self.least, float(np.min(top[:-1] - top[1:])))
        out = BN.beam_step_np(st, logits, rows_in, t, lse)
        for g in range(G):
            if frozen[g]:
                continue
            now = np.sort(np.array([float(st.pool_score[g * K + i]) for i in range(K) if st.pool_valid[g * K + i]]
                                   + pool[g]))  # old and new entries: duplicates are the old ones kept
            gaps = np.diff(np.unique(now))
            if gaps.size:
                self.least = min(self.least, float(gaps.min()))
            if st.pool_valid[g * K:(g + 1) * K].all() and t < st.n_tokens - 1:  # (nothing follows the last step)
                self.least = min(self.least, abs(float(st.run[g * K]) / d - float(st.pool_score[g * K + K - 1])))
        return out


def _hf_case(torch, model, G, K, eos, length_penalty, early, R):
    prompts = _prompts(G)
    mon = _Margins()
    seqs, scores, lengths, st = BN.beam_search_np(_ModelSteps(torch, model, prompts, K), G, K, HF_TOKENS, eos,
                                                  length_penalty, early, R, pad=1, step_fn=mon)
    with torch.no_grad():
        out = model.generate(torch.from_numpy(prompts), attention_mask=torch.ones(prompts.shape, dtype=torch.long),
                             num_beams=K, do_sample=False, max_new_tokens=HF_TOKENS, eos_token_id=eos,
                             pad_token_id=1, length_penalty=length_penalty, early_stopping=early,
                             num_return_sequences=R, return_dict_in_generate=True, output_scores=True)
    if K == 1:  # greedy search in transformers: the tokens only
        hs, hsc = out.sequences[:, HF_PROMPT:].numpy().reshape(G, 1, -1), None
    else:
        hs = out.sequences[:, HF_PROMPT:].numpy().reshape(G, R, -1)
        hsc = out.sequences_scores.numpy().reshape(G, R)
    return seqs, scores, lengths, st, hs, hsc, mon.least


def _hf_settings():
    for K in (1, 2, 4):
        for G in (1, 2):
            for lp in (0.0, 1.0, 2.0):
                for early in (False, True):
                    for R in sorted({1, K}):
                        for eos in (HF_EOS_EMITTED, HF_EOS_NEVER):
                            yield K, G, lp, early, R, eos


def test_numpy_search_equals_transformers_beam_search():
    torch, model = _tiny_gemma(HF_MODEL_SEED)
    stopped = 0
    for K, G, lp, early, R, eos in _hf_settings():
        what = (K, G, lp, early, R, eos)
        seqs, scores, lengths, st, hs, hsc, least = _hf_case(torch, model, G, K, eos, lp, early, R)
        assert least >= MARGIN, (what, least)
        n = seqs.shape[2]
        if K == 1:
            # greedy stops at its eos; the one beam's best hypothesis is that sequence unless an earlier, shorter
            # one scored higher, which the margins of a single beam exclude: a one-slot pool takes the first eos
            hl = np.array([[(list(r).index(eos) + 1) if eos in list(r) else len(r) for r in g] for g in hs])
            n = int(hl.max())
            assert np.array_equal(lengths, hl) and np.array_equal(seqs[:, :, :n], hs[:, :, :n]), what
            continue
        assert hs.shape[2] == n and np.array_equal(seqs, hs), (what, seqs, hs)
        tol = (lengths + 4) * 2.0 ** -23 * np.maximum(1.0, np.abs(hsc))
        assert np.all(np.abs(scores.astype(np.float64) - hsc) <= tol), (what, scores, hsc)
        assert np.all(scores[:, :-1] >= scores[:, 1:])
        stopped += int((lengths < HF_TOKENS).any())
        if eos == HF_EOS_NEVER:
            assert (lengths == HF_TOKENS).all() and not (seqs == eos).any(), what
    assert stopped > 0  # the emitted stop token ended hypotheses early
