"""Batches of 9..16 sequences per context: the batch rows fill the 16-row M side of the decode projections' MFMA
tile (kernels_gemv_mfma.hip), and every layer above it -- per-row step records, ragged prefill, generate --
holds 16 rows.

Two kinds of check, on the 2+2-layer full-width config with synthetic weights (seed 1234):
  * against the numpy oracle run on each row ALONE at B = 1 (bf16, and its fp32 truth as the floor): the rules of
    tests/test_gpu_ragged.py -- check_model_parity, |delta| <= 0.25 on the reference's top-8, argmax equal where
    the reference's top-2 margin exceeds 0.25;
  * bit identity: no reduction in the batched decode kernels involves the batch size, so a row computes the same
    bits in a batch of 16 as in a batch of 8 (same K splits, same combine order).
The oracle runs once per module (two sets of 16 rows: equal lengths of 33, and sixteen ragged lengths)."""
import numpy as np
import pytest
import torch

from oracle import paligemma_np as O
from oracle import weights as W
from tests_helpers import check_model_parity

pytestmark = pytest.mark.gpu
SEED = 1234
TEXT_SEED = 5
B16 = 16
L33 = 33
N_STEPS = 5
LENS8 = [1, 31, 32, 33, 63, 64, 65, 97]
# LENS8 plus eight more on both sides of the 32-key tile and of the 64-key chunk
LENS16 = LENS8 + [30, 34, 29, 35, 62, 66, 61, 67]
RAG_STEPS = 2                              # the rows of 63 and 62 tokens cross 64 keys on decode step 1 / 2


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.small_config(), max_batch=B16, max_seq=128, max_kv=256)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    yield e
    del e
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def P_text():
    P = W.synthetic_state_dict_f32(W.small_config(), SEED)
    return {n: v for n, v in P.items() if n.startswith("language_model")}


def text_rows(lens, seed=TEXT_SEED):
    """Random text prompts (ids in [3, vocab - 1), ids[:, 0] = 2), one per length."""
    cfg = W.small_config()
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, cfg["text_config"]["vocab_size"] - 1, size=(len(lens), max(lens))).astype(np.int64)
    ids[:, 0] = 2
    assert not (ids == cfg["image_token_index"]).any()   # text only: no row asks for an image feature
    return [ids[b, :n].copy() for b, n in enumerate(lens)]


def padded(rows, pad):
    ids = np.full((len(rows), max(len(r) for r in rows)), pad, dtype=np.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = r
    return torch.from_numpy(ids).cuda()


def oracle_row(P, row, steps):
    """The oracle on one unpadded row at B = 1: prefill, then `steps` decode steps along its own greedy
    tokens; the same tokens through the fp32 truth.  Returns (logits bf16 [steps + 1][V], truth, the
    tokens fed [steps])."""
    cfg = W.small_config()
    ids = row[None]
    L = ids.shape[1]
    emb = O.merge(P, cfg, None, ids)
    pos = np.arange(L)[None]
    okv, fkv = O.KV(), O.KV()
    ref = O.gemma_forward(P, cfg, emb, pos, okv, all_logits=False)[:, -1]
    with O.fp32_truth():
        tru = O.gemma_forward(P, cfg, emb, pos, fkv, all_logits=False)[:, -1]
    refs, trus, toks = [ref[0]], [tru[0]], []
    for t in range(steps):
        nxt = ref.argmax(-1)
        toks.append(int(nxt[0]))
        ref = O.paligemma_decode(P, cfg, nxt, okv, L + 1 + t)[:, -1]
        with O.fp32_truth():
            tru = O.paligemma_decode(P, cfg, nxt, fkv, L + 1 + t)[:, -1]
        refs.append(ref[0])
        trus.append(tru[0])
    return np.stack(refs), np.stack(trus), toks


def top8_and_argmax(got, ref, where):
    top = np.argsort(ref)[-8:]
    assert np.abs(got[top] - ref[top]).max() <= 0.25, where
    s = np.sort(ref)
    if s[-1] - s[-2] > 0.25:
        assert int(got.argmax()) == int(ref.argmax()), where


def check_rows(label, hist, refs, lens):
    """hist: our logits per step, each (B, V); refs[b] = oracle_row of row b."""
    for b in range(hist[0].shape[0]):
        ours = np.stack([h[b] for h in hist])
        for t in range(len(hist)):
            top8_and_argmax(ours[t], refs[b][0][t], (label, b, t))
        check_model_parity(f"batch16/{label}/row{b}_len{lens[b]}", ours, refs[b][0][:len(hist)], refs[b][1][:len(hist)])


@pytest.fixture(scope="module")
def lock16(P_text):
    """Sixteen prompts of 33 tokens and each one's oracle run (prefill + 5 decode steps), computed once."""
    rows = text_rows([L33] * B16)
    return rows, [oracle_row(P_text, r, N_STEPS) for r in rows]


@pytest.fixture(scope="module")
def rag16(P_text):
    """Sixteen prompts of LENS16 tokens and each one's oracle run (prefill + RAG_STEPS decode steps)."""
    rows = text_rows(LENS16, TEXT_SEED + 1)
    return rows, [oracle_row(P_text, r, RAG_STEPS) for r in rows]


@pytest.fixture(scope="module")
def prefilled16(eng, lock16):
    """The 16 equal-length rows after one prefill: (ids, the cache, each row's first greedy token).  Left unchanged."""
    rows, _ = lock16
    ids = padded(rows, 0)
    kv = eng.new_kv(B16, 64)
    lg = eng.lm_forward(kv, 0, torch.arange(L33).expand(B16, L33), ids=ids, logits_rows=1)[:, 0]
    first = eng.argmax(lg).clone()
    torch.cuda.synchronize()
    return ids, kv, first


# ---------------------------------------------------------------- 1. lock-step rows against the oracle
@pytest.mark.parametrize("B", [9, 13, 16])   # first row of the C tile's upper half / a partly filled quad / the full tile
def test_lock_step_rows_vs_oracle(eng, lock16, B):
    rows, refs = lock16
    ids = padded(rows[:B], 0)
    kv = eng.new_kv(B, 64)
    got = eng.lm_forward(kv, 0, torch.arange(L33).expand(B, L33), ids=ids, logits_rows=1)[:, 0]
    hist = [got.cpu().numpy()]
    logits = torch.empty((B, eng.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")
    for t in range(N_STEPS):                    # teacher-forced on each row's own oracle-greedy tokens
        nxt = torch.tensor([refs[b][2][t] for b in range(B)], dtype=torch.int64, device="cuda")
        hist.append(eng.decode(nxt, kv, L33 + t, L33 + t + 1, logits=logits, graph=t > 0).cpu().numpy())
    check_rows(f"lock_B{B}", hist, refs, [L33] * B)


# ---------------------------------------------------------------- 2. a row does not depend on its batch
def _decode_runs(eng, kv0, first, n):
    """pgmi_decode and an n-step pgmi_decode_steps on a copy of kv0, three calls each with graph=True (the eager
    call, the capturing call, a replay), the cache restored before every call.  Returns per call (logits, tokens
    [steps][B], the K/V rows the call wrote)."""
    B, V = first.numel(), eng.cfgd["t_vocab"]
    kv = kv0.clone()
    lg = torch.empty((B, V), dtype=torch.float32, device="cuda")
    nx = torch.empty(B, dtype=torch.int64, device="cuda")
    cur = torch.empty(B, dtype=torch.int64, device="cuda")
    rec = torch.empty((n, B), dtype=torch.int64, device="cuda")
    out = []
    for _ in range(3):
        kv.copy_(kv0)
        lg.fill_(float("nan"))
        nx.fill_(-1)
        eng.decode(first, kv, L33, L33 + 1, logits=lg, next_ids=nx, graph=True)
        torch.cuda.synchronize()
        out.append((lg.clone(), nx.clone()[None], kv[:, :, :, L33:L33 + 1].clone()))
    for _ in range(3):
        kv.copy_(kv0)
        lg.fill_(float("nan"))
        rec.fill_(-1)
        cur.copy_(first)
        eng.decode_steps(cur, kv, L33, L33 + 1, n, logits=lg, tokens=rec, graph=True)
        torch.cuda.synchronize()
        assert torch.equal(cur, rec[-1])
        out.append((lg.clone(), rec.clone(), kv[:, :, :, L33:L33 + n].clone()))
    return out


@pytest.mark.parametrize("staged", [0, 1])     # both RMSNorm forms of the batched step
def test_row_does_not_depend_on_its_batch(eng, prefilled16, staged):
    """The 16-row step against the same rows as two 8-row steps, through one engine: the prefill ran once (the
    8-row caches are copies of the 16-row cache's rows), so only the decode differs.  Logits, argmax tokens
    and the written K/V rows are bit-identical."""
    _, kv16, first = prefilled16
    eng.set_decode_staged_norm(staged)
    try:
        full = _decode_runs(eng, kv16, first, N_STEPS)
        lo = _decode_runs(eng, kv16[:, :, :8].contiguous(), first[:8].clone(), N_STEPS)
        hi = _decode_runs(eng, kv16[:, :, 8:].contiguous(), first[8:].clone(), N_STEPS)
    finally:
        eng.set_decode_staged_norm(-1)
    for i, (f, a, b) in enumerate(zip(full, lo, hi)):
        assert torch.isfinite(f[0]).all(), i
        assert torch.equal(f[0], torch.cat([a[0], b[0]], 0)), (staged, i, "logits")
        assert torch.equal(f[1], torch.cat([a[1], b[1]], 1)), (staged, i, "tokens")
        assert torch.equal(f[2], torch.cat([a[2], b[2]], 2)), (staged, i, "kv rows")
    # the three decode calls agree with each other, and so do the three decode_steps calls
    for j in (1, 2, 4, 5):
        k = 0 if j < 3 else 3
        assert all(torch.equal(full[j][q], full[k][q]) for q in range(3)), j


# ---------------------------------------------------------------- 3. ragged at 16 rows
@pytest.fixture(scope="module")
def ragged_prefilled(eng, rag16):
    rows, refs = rag16
    ids = padded(rows, 0)
    Lmax = max(LENS16)
    kv = eng.new_kv(B16, 128)
    got = eng.lm_forward(kv, 0, torch.arange(Lmax).expand(B16, Lmax), ids=ids, logits_rows=1, lens=LENS16)[:, 0]
    torch.cuda.synchronize()
    return ids, kv, got.clone()


def test_ragged_16_rows_vs_oracle(eng, rag16, ragged_prefilled):
    _, refs = rag16
    _, kv0, got = ragged_prefilled
    kv = kv0.clone()
    logits = torch.empty((B16, eng.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")
    ln = torch.tensor(LENS16, dtype=torch.int32)
    assert any(n <= 64 < n + RAG_STEPS for n in LENS16)   # a row crosses the 64-key chunk boundary while decoding
    hist = [got.cpu().numpy()]
    for t in range(RAG_STEPS):
        nxt = torch.tensor([refs[b][2][t] for b in range(B16)], dtype=torch.int64, device="cuda")
        hist.append(eng.decode_ragged(nxt, kv, ln + t, ln + t + 1, logits=logits, graph=t > 0).cpu().numpy())
    check_rows("ragged", hist, refs, LENS16)


@pytest.mark.parametrize("graph", [False, True])
def test_equal_lengths_ragged_equals_lock_step_at_16(eng, prefilled16, graph):
    _, kv0, first = prefilled16
    n, V = N_STEPS, eng.cfgd["t_vocab"]
    ln = torch.tensor([L33] * B16, dtype=torch.int32)
    kv1, cur1 = kv0.clone(), first.clone()
    lg1 = torch.empty((B16, V), dtype=torch.float32, device="cuda")
    ref = []
    for t in range(n):
        eng.decode(cur1, kv1, L33 + t, L33 + t + 1, logits=lg1, next_ids=cur1, graph=graph)
        ref.append(cur1.clone())
    ref = torch.stack(ref)
    kv2, cur2 = kv0.clone(), first.clone()
    lg2 = torch.full((B16, V), float("nan"), dtype=torch.float32, device="cuda")
    got = []
    for t in range(n):
        eng.decode_ragged(cur2, kv2, ln + t, ln + t + 1, logits=lg2, next_ids=cur2, graph=graph)
        got.append(cur2.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), ref)
    assert torch.equal(lg2, lg1)
    assert torch.equal(kv2[:, :, :, :L33 + n], kv1[:, :, :, :L33 + n])
    # one n-step ragged call against pgmi_decode_steps
    kv3, cur3 = kv0.clone(), first.clone()
    rec3 = torch.empty((n, B16), dtype=torch.int64, device="cuda")
    lg3 = torch.empty((B16, V), dtype=torch.float32, device="cuda")
    eng.decode_steps(cur3, kv3, L33, L33 + 1, n, logits=lg3, tokens=rec3, graph=graph)
    kv4, cur4 = kv0.clone(), first.clone()
    rec4 = torch.full((n, B16), -1, dtype=torch.int64, device="cuda")
    lg4 = torch.full((B16, V), float("nan"), dtype=torch.float32, device="cuda")
    eng.decode_ragged(cur4, kv4, ln, ln + 1, n, logits=lg4, tokens=rec4, graph=graph)
    torch.cuda.synchronize()
    assert torch.equal(rec3, ref) and torch.equal(rec4, ref)
    assert torch.equal(lg4, lg3) and torch.equal(lg3, lg1)
    assert torch.equal(kv4[:, :, :, :L33 + n], kv3[:, :, :, :L33 + n])


# ---------------------------------------------------------------- 4. nothing past a row's length is read
def test_kv_past_a_rows_length_is_never_read_at_16(eng, rag16, ragged_prefilled):
    _, refs = rag16
    _, kv0, _ = ragged_prefilled
    nan16 = torch.tensor([0x7FC0], dtype=torch.int16).view(torch.bfloat16).item()
    outs = []
    for fill in (nan16, 0.0):
        kv = kv0.clone()
        for b, n in enumerate(LENS16):
            kv[:, :, b, n:] = fill
        if fill != 0.0:
            assert torch.isnan(kv[:, :, 0, LENS16[0]:].float()).all()
        cur = torch.tensor([refs[b][2][0] for b in range(B16)], dtype=torch.int64, device="cuda")
        logits = torch.empty((B16, eng.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")
        ln = torch.tensor(LENS16, dtype=torch.int32)
        steps = []
        for t in range(3):
            eng.decode_ragged(cur, kv, ln + t, ln + t + 1, logits=logits, next_ids=cur, graph=False)
            steps.append(logits.clone())
        torch.cuda.synchronize()
        outs.append(torch.stack(steps))
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- 5. generate at 16 rows
def _pixels(n, seed=0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(O.bf16(rng.uniform(-1, 1, (n, 3, 224, 224)).astype(np.float32))).cuda()


def test_generate_16_rows_greedy_and_eos(eng, prefilled16):
    """generate() includes the prefill.  The engine runs a prefill of more than 8 rows as row groups of 8, each at
    the 8-row call's GEMM shapes, and the decode steps do not depend on the batch, so the 16-row run equals its two
    halves bit for bit."""
    ids, _, _ = prefilled16
    px = _pixels(B16)
    n = 12                                           # a chunk of 8 steps per launch, then one of 3
    g = eng.generate(ids, px, n, graph=True)
    s = eng.generate(ids, px, n, graph=False)
    lo = eng.generate(ids[:8].contiguous(), px[:8], n, graph=True)
    hi = eng.generate(ids[8:].contiguous(), px[8:], n, graph=True)
    assert g.shape == (B16, n)
    assert torch.equal(g, s)                         # 8 steps per launch == one launch per step
    assert torch.equal(g, torch.cat([lo, hi], 0))    # == the two halves of 8
    # a stop token that some row emits: rows, lengths and trimming as the halves'
    eos, pad = int(g[0, 2]), -7
    kw = dict(eos_token_id=eos, pad_token_id=pad, sync_every=2, return_lengths=True)
    t16, l16 = eng.generate(ids, px, n, graph=True, **kw)
    ta, la = eng.generate(ids[:8].contiguous(), px[:8], n, graph=True, **kw)
    tb, lb = eng.generate(ids[8:].contiguous(), px[8:], n, graph=True, **kw)
    assert int(l16[0]) <= 3
    assert torch.equal(l16, torch.cat([la, lb]))
    assert t16.shape[1] == max(ta.shape[1], tb.shape[1]) == int(l16.max())
    for half, r0 in ((ta, 0), (tb, 8)):
        w = half.shape[1]
        assert torch.equal(t16[r0:r0 + 8, :w], half)
        assert (t16[r0:r0 + 8, w:] == pad).all()
    gn = g.cpu().numpy()
    for r in range(B16):                             # and as the free-running tokens up to each row's eos
        k = int(l16[r])
        assert np.array_equal(t16[r, :k].cpu().numpy(), gn[r, :k]), r
        assert (t16[r, k:] == pad).all(), r


# Text seeds of the ragged generate test, one per row of LENS16 (row b: default_rng(seed).integers(3, vocab - 1, n),
# <bos> first where n > 1).  Random text mostly gives near-ties (the oracle's top-2 margin is under 0.25 on 47 of
# the 64 first steps of rag16's prompts), so each seed is one found by trying 1000 b, 1000 b + 1, ... on the oracle
# (CPU, the row alone, bf16) until its top-2 margin is at least 0.40 on each of the first four greedy steps (0.42 ..
# 1.3 on these).  The one-token row is a token of its own, not <bos>: <bos> alone is a near-tie (margin 0.03).
GEN_SEEDS16 = [38, 1005, 2804, 3154, 4061, 5110, 6046, 7808, 8043, 9180, 10008, 11058, 12226, 13290, 14043, 15016]
GEN_FLOOR = 4      # tokens of every row that must be compared (tests/test_gpu_ragged.py's floor)


def gen_rows16():
    cfg = W.small_config()
    rows = []
    for n, seed in zip(LENS16, GEN_SEEDS16):
        r = np.random.default_rng(seed).integers(3, cfg["text_config"]["vocab_size"] - 1, size=n).astype(np.int64)
        if n > 1:
            r[0] = 2
        assert not (r == cfg["image_token_index"]).any()
        rows.append(r)
    return rows


def test_generate_16_ragged_rows_equal_their_own_batch_of_one(eng):
    """generate(attention_mask=...) over sixteen ragged prompts: every row generates what it generates alone.  A
    batch of one runs the v_dot2 GEMVs, not the MFMA projections (another accumulation order), so -- as
    test_generate_with_padded_mask -- the prompts are chosen for decisive margins (GEN_SEEDS16), a row is compared
    up to its first step whose top-2 margin on the single row's own logits is under 0.25, and every row must be
    compared on at least GEN_FLOOR of its 6 tokens.  The 8-steps-per-launch graphs against one launch per step are
    bit-identical on every step."""
    rows = gen_rows16()
    ids = padded(rows, 0)
    px = _pixels(B16)
    Lmax, n = max(LENS16), 6
    mask = torch.zeros((B16, Lmax), dtype=torch.int64)
    for b, ln in enumerate(LENS16):
        mask[b, :ln] = 1
    got = eng.generate(ids, px, n, graph=True, attention_mask=mask)
    assert got.shape == (B16, n)
    assert torch.equal(got, eng.generate(ids, px, n, graph=False, attention_mask=mask))
    got = got.cpu().numpy()
    for b, ln in enumerate(LENS16):
        one_ids, one_px = ids[b:b + 1, :ln].contiguous(), px[b:b + 1]
        want = eng.generate(one_ids, one_px, n, graph=True).cpu().numpy()[0]
        # the single row's top-2 margins along its own tokens (a teacher-forced pass)
        kv1 = eng.new_kv(1, ln + n + 1)
        lg = eng.lm_forward(kv1, 0, torch.arange(ln)[None], ids=one_ids, logits_rows=2)[:, 0]
        margins = []
        for t in range(n):
            top2 = lg[0].topk(2).values
            margins.append(float(top2[0] - top2[1]))
            if t + 1 < n:
                lg = eng.decode(torch.tensor([int(want[t])], device="cuda"), kv1, ln + t, ln + t + 1)
        low = [t for t, m in enumerate(margins) if m < 0.25]
        upto = low[0] if low else n
        print(f"batch16 ragged generate row {b} len {ln}: margins {[round(m, 3) for m in margins]} compared {upto}")
        assert upto >= GEN_FLOOR, (b, margins)
        assert np.array_equal(got[b, :upto], want[:upto]), (b, got[b], want, margins)


# ---------------------------------------------------------------- 6. sampling plumbing at 16 rows
def test_sampling_with_top_p_zero_is_greedy_at_16(eng, prefilled16):
    """do_sample with top_p = 0 keeps only the first sorted token (inference.py:19: `0 - 0 > p` is false for it
    alone), so the sampled tokens are greedy's wherever the step's top-2 logit margin is non-zero."""
    ids, _, _ = prefilled16
    px = _pixels(B16)
    n = 6
    greedy = eng.generate(ids, px, n, graph=False)
    samp = eng.generate(ids, px, n, graph=False, do_sample=True, top_p=0.0, temperature=0.8,
                        generator=torch.Generator("cuda").manual_seed(11))
    if torch.equal(samp, greedy):
        return
    # a row that differs: its first differing step must be an exact tie of the top two logits (the step's logits
    # along the greedy tokens, recomputed teacher-forced)
    kv = eng.new_kv(B16, L33 + n + 1)
    lg = eng.lm_forward(kv, 0, torch.arange(L33).expand(B16, L33), ids=ids, logits_rows=2)[:, 0]
    margins = []
    for t in range(n):
        top2 = lg.topk(2, dim=-1).values
        margins.append((top2[:, 0] - top2[:, 1]).cpu().numpy())
        if t + 1 < n:
            lg = eng.decode(greedy[:, t].contiguous(), kv, L33 + t, L33 + t + 1)
    margins = np.stack(margins, 1)
    gn, sn = greedy.cpu().numpy(), samp.cpu().numpy()
    for r in range(B16):
        d = np.nonzero(gn[r] != sn[r])[0]
        if len(d):
            assert margins[r, d[0]] == 0.0, (r, int(d[0]), gn[r], sn[r], margins[r])


# ---------------------------------------------------------------- 7. prefill at 16 images
def test_prefill_16_images_equals_two_batches_of_8():
    """vision -> project -> lm_forward(logits_rows=1) for 16 distinct images in one batch against the same rows as
    two batches of 8, held to the project's bound for "same values, another accumulation order"
    (test_last_row_only_final_layer): same argmax, rel-L2 < 1e-2.  An engine of its own: a prompt with a
    whole image's 256 tokens needs max_seq >= 272.

    The engine runs the vision tower, the projector and the language-model layers of more than 8 images as row
    groups of 8 through the 8-image plans, so the two runs are the same kernels on the same rows; as one M = 4,096 /
    4,352 batch on the generic plans the logits sat 1.5e-2 .. 2.5e-2 apart (equal argmax, features 6e-3 apart)."""
    from pgmi import Engine
    cfg = W.small_config()
    e = Engine(cfg, max_batch=B16, max_seq=272, max_kv=288)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    n_img, L = W.num_image_tokens(cfg), 272
    rng = np.random.default_rng(7)
    text = rng.integers(3, 16000, size=(B16, L - n_img - 1)).astype(np.int64)
    ids = np.concatenate([np.full((B16, n_img), cfg["image_token_index"], np.int64), np.full((B16, 1), 2, np.int64),
                          text], 1)
    ids = torch.from_numpy(ids).cuda()
    px = _pixels(B16, seed=3)

    def run(r0, r1):
        B = r1 - r0
        feats = e.project(e.vision(px[r0:r1].contiguous()))
        kv = e.new_kv(B, 288)
        lg = e.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids[r0:r1].contiguous(), image_feats=feats,
                          logits_rows=1)[:, 0]
        torch.cuda.synchronize()
        return feats.float().cpu().numpy(), lg.cpu().numpy()

    f16, l16 = run(0, 16)
    fa, la = run(0, 8)
    fb, lb = run(8, 16)
    f8, l8 = np.concatenate([fa, fb]), np.concatenate([la, lb])
    assert np.isfinite(l16).all()
    print("batch16 prefill16 rel-L2 per row, features: " + " ".join(f"{rel_l2(f16[b], f8[b]):.2e}" for b in range(B16)))
    print("batch16 prefill16 rel-L2 per row, logits:   " + " ".join(f"{rel_l2(l16[b], l8[b]):.2e}" for b in range(B16)))
    print("batch16 prefill16 argmax equal per row:     " + " ".join(str(int(l16[b].argmax() == l8[b].argmax())) for b in range(B16)))
    for b in range(B16):
        assert rel_l2(f16[b], f8[b]) < 1e-2, b
        assert rel_l2(l16[b], l8[b]) < 1e-2, (b, rel_l2(l16[b], l8[b]))
        assert int(l16[b].argmax()) == int(l8[b].argmax()), b
    assert len({int(x.argmax()) for x in l16}) > 1       # distinct images and prompts: not one answer for all
    del e
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 8. capacity
def test_17_rows_are_refused(eng):
    V = eng.cfgd["t_vocab"]
    ids17 = torch.full((17,), 5, dtype=torch.int64, device="cuda")
    kv17 = eng.new_kv(17, 64)
    with pytest.raises(ValueError):
        eng.decode(ids17, kv17, 8, 9)
    with pytest.raises(ValueError):
        eng.decode_ragged(ids17, kv17, [8] * 17, [9] * 17)
    with pytest.raises(ValueError):
        eng.lm_forward(kv17, 0, torch.arange(8).expand(17, 8), ids=ids17[:, None].expand(17, 8).contiguous(),
                       logits_rows=1)
    with pytest.raises(ValueError):
        eng.generate(ids17[:, None].expand(17, 8).contiguous(), _pixels(17), 2)
    # 16 rows pass the same calls
    kv = eng.new_kv(B16, 64)
    lg = eng.lm_forward(kv, 0, torch.arange(8).expand(B16, 8), ids=ids17[:16, None].expand(16, 8).contiguous(),
                        logits_rows=1)
    assert lg.shape == (B16, 1, V) and torch.isfinite(lg).all()


@pytest.mark.parametrize("K,N", [(2048, 2048), (2048, 1000), (16384, 2048), (16384, 520)])
def test_op_gemv_res_16_rows_equal_two_calls_of_8(eng, K, N):
    from pgmi import _native as NN
    rng = np.random.default_rng(K + N)
    x = torch.from_numpy(rng.standard_normal((B16, K)).astype(np.float32)).cuda().to(torch.bfloat16)
    w = torch.from_numpy((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)).cuda().to(torch.bfloat16)
    h = torch.from_numpy(rng.standard_normal((B16, N)).astype(np.float32)).cuda().to(torch.bfloat16)
    h16, h8 = h.clone(), h.clone()
    NN.check(eng.lib.pgmi_op_gemv_res(eng.ctx, x.data_ptr(), w.data_ptr(), B16, N, K, h16.data_ptr(), NN.stream_handle()))
    for r0 in (0, 8):
        NN.check(eng.lib.pgmi_op_gemv_res(eng.ctx, x[r0:].data_ptr(), w.data_ptr(), 8, N, K, h8[r0:].data_ptr(),
                                          NN.stream_handle()))
    torch.cuda.synchronize()
    assert torch.equal(h16, h8)
    ref = ((x.float() @ w.float().T).to(torch.bfloat16).float() + h.float()).to(torch.bfloat16).float()
    assert rel_l2(h16.float().cpu().numpy(), ref.cpu().numpy()) < 2e-3   # test_gemv_res's bound, same rounding points
    with pytest.raises(ValueError):
        NN.check(eng.lib.pgmi_op_gemv_res(eng.ctx, x.data_ptr(), w.data_ptr(), 17, N, K, h16.data_ptr(),
                                          NN.stream_handle()))


# ---------------------------------------------------------------- 9. graph cache
def test_repeated_generate_at_16_does_not_grow_the_graph_cache(eng, prefilled16):
    ids, _, _ = prefilled16
    px = _pixels(B16)
    n = 12
    kv = eng.new_kv(B16, L33 + n + 1)
    eng.set_decode_staged_norm(-1)                   # an empty decode cache to start from (it is bounded at 64 keys)
    assert eng.lib.pgmi_graph_count(eng.ctx, 1) == 0
    counts, toks = [], []
    for _ in range(4):
        toks.append(eng.generate(ids, px, n, graph=True, kv=kv))
        counts.append(eng.lib.pgmi_graph_count(eng.ctx, 1))
    assert counts[1] == counts[2] == counts[3], counts
    assert all(torch.equal(t, toks[0]) for t in toks[1:])
