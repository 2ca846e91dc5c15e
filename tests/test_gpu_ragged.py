"""Ragged batches (pgmi_lm_forward_ragged / pgmi_decode_ragged / Engine.generate(attention_mask=...)):
every row of a right-padded batch computes what it would compute alone.  The reference for a row is the
oracle run on that row alone, unpadded, at B = 1 (bf16, and its fp32 truth as the floor); the 2+2-layer
full-width config and the rules of tests/test_gpu_model_small.py throughout."""
import os

import numpy as np
import pytest
import torch

from oracle import paligemma_np as O
from oracle import weights as W
from tests_helpers import check_model_parity

pytestmark = pytest.mark.gpu
SEED = 1234
TEXT_SEED = 5
LENS8 = [1, 31, 32, 33, 63, 64, 65, 97]   # both sides of the 32-key tile and of the 64-key chunk, one token
IMG_LENS = [288, 270, 259]
GEN_TEXT_SEEDS = [33, 54, 31]             # test 9's text tokens, per row (margins checked on the oracle, see there)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "small_bf16.npz"))


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.small_config(), max_batch=8, max_seq=1024, max_kv=1024)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    return e


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
    return [ids[b, :n].copy() for b, n in enumerate(lens)]


def padded(rows, pad):
    ids = np.full((len(rows), max(len(r) for r in rows)), pad, dtype=np.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = r
    return torch.from_numpy(ids).cuda()


def oracle_row(P, row, steps):
    """The oracle on one unpadded row at B = 1: prefill, then `steps` decode steps along its own greedy
    tokens; the same tokens through the fp32 truth.  Returns (logits bf16 [steps + 1][V], truth, the
    tokens fed [steps], the bf16 run's KV after the prefill (k, v per layer))."""
    cfg = W.small_config()
    ids = row[None]
    L = ids.shape[1]
    emb = O.merge(P, cfg, None, ids)
    pos = np.arange(L)[None]
    okv, fkv = O.KV(), O.KV()
    ref = O.gemma_forward(P, cfg, emb, pos, okv, all_logits=False)[:, -1]
    with O.fp32_truth():
        tru = O.gemma_forward(P, cfg, emb, pos, fkv, all_logits=False)[:, -1]
    kv0 = ([k.copy() for k in okv.k], [v.copy() for v in okv.v])
    refs, trus, toks = [ref[0]], [tru[0]], []
    for t in range(steps):
        nxt = ref.argmax(-1)
        toks.append(int(nxt[0]))
        ref = O.paligemma_decode(P, cfg, nxt, okv, L + 1 + t)[:, -1]
        with O.fp32_truth():
            tru = O.paligemma_decode(P, cfg, nxt, fkv, L + 1 + t)[:, -1]
        refs.append(ref[0])
        trus.append(tru[0])
    return np.stack(refs), np.stack(trus), toks, kv0


def top8_and_argmax(got, ref, where):
    top = np.argsort(ref)[-8:]
    assert np.abs(got[top] - ref[top]).max() <= 0.25, where
    s = np.sort(ref)
    if s[-1] - s[-2] > 0.25:
        assert int(got.argmax()) == int(ref.argmax()), where


@pytest.fixture(scope="module")
def prefill8(P_text):
    """Test 2's rows and their oracle runs (computed once, left unchanged)."""
    rows = text_rows(LENS8)
    return rows, [oracle_row(P_text, r, 0) for r in rows]


# ---------------------------------------------------------------- 2. ragged prefill vs the oracle
def test_ragged_prefill_vs_oracle(eng, prefill8):
    rows, refs = prefill8
    B, Lmax = len(rows), max(LENS8)
    ids = padded(rows, 0)
    pos = torch.arange(Lmax).expand(B, Lmax)
    kv = eng.new_kv(B, 128)
    lg = eng.lm_forward(kv, 0, pos, ids=ids, logits_rows=1, lens=LENS8)[:, 0]
    kv2 = eng.new_kv(B, 128)
    lg2 = eng.lm_forward(kv2, 0, pos, ids=ids, logits_rows=2, lens=LENS8)[:, 0]
    torch.cuda.synchronize()
    g, g2 = lg.cpu().numpy(), lg2.cpu().numpy()
    for b, n in enumerate(LENS8):
        ref, tru, _, (ok, ov) = refs[b]
        check_model_parity(f"ragged/prefill8/row{b}_len{n}", g[b], ref[0], tru[0])
        top8_and_argmax(g[b], ref[0], (b, n))
        # K/V rows [0, lens[b]) of layer 0 and of the last layer against the oracle's cache
        assert rel_l2(kv[0, 0, b, :n].float().cpu().numpy(), ok[0][0, 0]) < 1e-2, (b, n)
        assert rel_l2(kv[0, 1, b, :n].float().cpu().numpy(), ov[0][0, 0]) < 1e-2, (b, n)
        assert rel_l2(kv[-1, 0, b, :n].float().cpu().numpy(), ok[-1][0, 0]) < 3e-2, (b, n)
        assert rel_l2(kv[-1, 1, b, :n].float().cpu().numpy(), ov[-1][0, 0]) < 3e-2, (b, n)
        # logits_rows 2 against logits_rows 1 (test_last_row_only_final_layer's bounds)
        assert int(g2[b].argmax()) == int(g[b].argmax()), (b, n)
        assert rel_l2(g2[b], g[b]) < 1e-2, (b, n)
    assert torch.isfinite(kv[:, :, :, :Lmax].float()).all()   # pad slots: unspecified but finite


# ---------------------------------------------------------------- 3. pad independence
def test_pad_ids_and_graph_replay_do_not_matter(eng, prefill8):
    """Pad slots filled with token 5, then with token 9 (both valid ids): logits and the K/V rows
    [0, lens[b]) are bit-identical, on the eager call, the capturing call and the replays."""
    from pgmi import _native as N
    rows, _ = prefill8
    B, Lmax = len(rows), max(LENS8)
    ids = padded(rows, 5)
    ids9 = padded(rows, 9)
    pos = torch.arange(Lmax).expand(B, Lmax).contiguous()
    lens = torch.tensor(LENS8, dtype=torch.int32)
    kv = eng.new_kv(B, 128)
    logits = torch.empty((B, 1, eng.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")

    def run():
        kv.fill_(float("nan"))        # nothing a call returns may come from an earlier call's cache
        logits.fill_(float("nan"))
        N.check(eng.lib.pgmi_lm_forward_ragged(eng.ctx, ids.data_ptr(), None, 0, None, B, Lmax, pos.data_ptr(),
                                               lens.data_ptr(), kv.data_ptr(), B, kv.shape[3], 0, logits.data_ptr(),
                                               1, eng._s()))
        torch.cuda.synchronize()
        return logits[:, 0].clone(), [kv[:, :, b, :n].clone() for b, n in enumerate(LENS8)]

    want_l, want_kv = run()           # eager (first call with these buffers)
    assert torch.isfinite(want_l).all()
    for i in range(4):                # capture, replay; then the pads changed in place: replay, replay
        if i == 2:
            ids.copy_(ids9)
        got_l, got_kv = run()
        assert torch.equal(got_l, want_l), i
        for b in range(B):
            assert torch.equal(got_kv[b], want_kv[b]), (i, b)


# ---------------------------------------------------------------- 4. ragged prefill with images
def image_batch(gold, text_seeds=None):
    """gold["ids"] (256 <image> tokens + 32 text tokens) truncated to 288 / 270 / 259 tokens, with the
    image, its horizontal flip and its vertical flip; text_seeds: row b's text tokens after <bos> are
    random ones drawn with text_seeds[b] instead."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2)]).contiguous()
    base = gold["ids"][0]
    rows = []
    for b, n in enumerate(IMG_LENS):
        r = base[:n].copy()
        if text_seeds is not None:
            cfg = W.small_config()
            rng = np.random.default_rng(text_seeds[b])
            text = rng.integers(3, cfg["text_config"]["vocab_size"] - 1, size=(3, 31)).astype(np.int64)
            r[257:n] = text[b, :n - 257]
        rows.append(r)
    return rows, pxs


@pytest.fixture(scope="module")
def truth_last(gold):
    P = W.synthetic_state_dict_f32(W.small_config(), SEED)
    with O.fp32_truth():
        lg, _ = O.paligemma_prefill(P, W.small_config(), gold["ids"], O.from_bits(gold["pixels_bits"]),
                                    all_logits=False)
    return lg[:, -1]


def test_ragged_prefill_with_images(eng, gold, truth_last):
    rows, pxs = image_batch(gold)
    B, Lmax = 3, max(IMG_LENS)
    ids = padded(rows, 0)
    feats = eng.project(eng.vision(pxs))
    kv = eng.new_kv(B, Lmax + 8)
    got = eng.lm_forward(kv, 0, torch.arange(Lmax).expand(B, Lmax), ids=ids, image_feats=feats, logits_rows=1,
                         lens=IMG_LENS)[:, 0].cpu().numpy()
    for b, n in enumerate(IMG_LENS):
        kv1 = eng.new_kv(1, Lmax + 8)
        one = eng.lm_forward(kv1, 0, torch.arange(n)[None], ids=ids[b:b + 1, :n].contiguous(),
                             image_feats=eng.project(eng.vision(pxs[b:b + 1])), logits_rows=1)[0, 0].cpu().numpy()
        assert rel_l2(got[b], one) < 3e-2, b
        top8_and_argmax(got[b], one, b)
    check_model_parity("ragged/prefill_images/row0", got[:1], gold["prefill_logits_last"], truth_last)


# ---------------------------------------------------------------- 5 / 6 / 8. ragged decode vs the oracle
def ragged_decode_vs_oracle(e, P, lens, steps, label, kv_tokens):
    rows = text_rows(lens)
    refs = [oracle_row(P, r, steps) for r in rows]
    B, Lmax = len(rows), max(lens)
    ids = padded(rows, 0)
    kv = e.new_kv(B, kv_tokens)
    got = e.lm_forward(kv, 0, torch.arange(Lmax).expand(B, Lmax), ids=ids, logits_rows=1, lens=lens)[:, 0]
    kv_after_prefill = kv.clone()
    logits = torch.empty((B, e.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int32)
    hist = [got.cpu().numpy()]
    for t in range(steps):                      # teacher-forced on each row's own oracle-greedy tokens
        nxt = torch.tensor([refs[b][2][t] for b in range(B)], dtype=torch.int64, device="cuda")
        hist.append(e.decode_ragged(nxt, kv, ln + t, ln + t + 1, logits=logits, graph=t > 0).cpu().numpy())
    for b in range(B):
        ours = np.stack([h[b] for h in hist])
        for t in range(steps + 1):
            top8_and_argmax(ours[t], refs[b][0][t], (label, b, t))
        check_model_parity(f"ragged/{label}/row{b}_len{lens[b]}", ours, refs[b][0], refs[b][1])
    return kv_after_prefill, refs


@pytest.fixture(scope="module")
def decode4(eng, P_text):
    """Test 5 at B = 4 (the MFMA projections): its cache after the prefill serves test 8."""
    lens = [62, 63, 64, 5]
    kv0, refs = ragged_decode_vs_oracle(eng, P_text, lens, 4, "decode_B4", 80)
    return lens, kv0, refs


def test_ragged_decode_vs_oracle_B2(eng, P_text):
    ragged_decode_vs_oracle(eng, P_text, [62, 5], 4, "decode_B2", 80)


def test_ragged_decode_vs_oracle_B4(decode4):
    assert decode4 is not None   # the comparison runs (and asserts) in the fixture; test 8 reuses its cache


@pytest.mark.parametrize("lens", [[766, 40], [766, 40, 767, 700]])
def test_ragged_decode_two_pass_combine_boundary(P_text, lens):
    """One row crosses 768 keys (more than 12 chunks: the combine's two-pass form) while its neighbour stays
    short."""
    from pgmi import Engine
    e = Engine(W.small_config(), max_batch=len(lens), max_seq=768, max_kv=832)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    ragged_decode_vs_oracle(e, P_text, lens, 4, f"decode_768_B{len(lens)}", 832)
    del e
    torch.cuda.empty_cache()


def test_kv_past_a_rows_length_is_never_read(eng, decode4):
    lens, kv0, refs = decode4
    B = len(lens)
    nan16 = torch.tensor([0x7FC0], dtype=torch.int16).view(torch.bfloat16).item()
    outs = []
    for fill in (nan16, 0.0):
        kv = kv0.clone()
        for b, n in enumerate(lens):
            kv[:, :, b, n:] = fill
        if fill != 0.0:
            assert torch.isnan(kv[:, :, 0, lens[0]:].float()).all()
        cur = torch.tensor([refs[b][2][0] for b in range(B)], dtype=torch.int64, device="cuda")
        logits = torch.empty((B, eng.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")
        ln = torch.tensor(lens, dtype=torch.int32)
        steps = []
        for t in range(3):
            eng.decode_ragged(cur, kv, ln + t, ln + t + 1, logits=logits, next_ids=cur, graph=False)
            steps.append(logits.clone())
        torch.cuda.synchronize()
        outs.append(torch.stack(steps))
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- 7. equal lengths == lock-step, bit for bit
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("graph", [False, True])
def test_equal_lengths_equal_lock_step(eng, gold, B, graph):
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2)])[:B].contiguous()
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L, n, V = ids.shape[1], 5, eng.cfgd["t_vocab"]
    feats = eng.project(eng.vision(pxs))
    pos = torch.arange(L).expand(B, L)
    kv0 = eng.new_kv(B, L + n + 1)
    l_lock = eng.lm_forward(kv0, 0, pos, ids=ids, image_feats=feats, logits_rows=1)[:, 0]
    first = eng.argmax(l_lock)
    # ragged prefill with equal lengths (the attention variant may differ: accumulation order)
    kvr = eng.new_kv(B, L + n + 1)
    l_rag = eng.lm_forward(kvr, 0, pos, ids=ids, image_feats=feats, logits_rows=1, lens=[L] * B)[:, 0]
    for b in range(B):
        assert rel_l2(l_rag[b].cpu().numpy(), l_lock[b].cpu().numpy()) < 1e-3, b
    # lock-step decode
    kv1 = kv0.clone()
    cur = first.clone()
    lg1 = torch.empty((B, V), dtype=torch.float32, device="cuda")
    ref = []
    for t in range(n):
        eng.decode(cur, kv1, L + t, L + t + 1, logits=lg1, next_ids=cur, graph=graph)
        ref.append(cur.clone())
    ref = torch.stack(ref)
    ln = torch.tensor([L] * B, dtype=torch.int32)
    # five 1-step ragged calls (graph=True: eager, capture, replays)
    kv2 = kv0.clone()
    cur2 = first.clone()
    lg2 = torch.full((B, V), float("nan"), dtype=torch.float32, device="cuda")
    got = []
    for t in range(n):
        eng.decode_ragged(cur2, kv2, ln + t, ln + t + 1, logits=lg2, next_ids=cur2, graph=graph)
        got.append(cur2.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), ref)
    assert torch.equal(lg2, lg1)
    assert torch.equal(kv2[:, :, :, :L + n], kv1[:, :, :, :L + n])
    # one 5-step ragged call, three times (graph=True: eager, capture, replay)
    kv3 = kv0.clone()
    cur3 = torch.empty_like(first)
    rec = torch.empty((n, B), dtype=torch.int64, device="cuda")
    lg3 = torch.empty((B, V), dtype=torch.float32, device="cuda")
    for rep in range(3):
        cur3.copy_(first)
        rec.fill_(-1)
        lg3.fill_(float("nan"))
        eng.decode_ragged(cur3, kv3, ln, ln + 1, n, logits=lg3, tokens=rec, graph=graph)
        torch.cuda.synchronize()
        assert torch.equal(rec, ref), rep
        assert torch.equal(cur3, ref[-1]) and torch.equal(lg3, lg1), rep
        assert torch.equal(kv3[:, :, :, :L + n], kv1[:, :, :, :L + n]), rep


# ---------------------------------------------------------------- 9. generate with a padded mask
@pytest.mark.parametrize("graph", [False, True])
def test_generate_with_padded_mask(eng, gold, graph):
    """Prompts: test 4's lengths and pixels with random text tokens (GEN_TEXT_SEEDS, one seed per row).
    gold["ids"]' own text gives the oracle (O.greedy_generate on the CPU, each row alone) top-2 margins of
    0.016 / 0.0 / 0.125 at step 0, so no step could be compared; with these seeds its margins are
    0.50 0.80 0.89 0.53 | 0.24 ... (row 0: four steps), >= 0.45 on all eight (row 1) and >= 0.39 on
    all eight (row 2)."""
    rows, pxs = image_batch(gold, GEN_TEXT_SEEDS)
    B, Lmax, n = 3, max(IMG_LENS), 8
    ids = padded(rows, 0)
    mask = torch.zeros((B, Lmax), dtype=torch.int64)
    for b, ln in enumerate(IMG_LENS):
        mask[b, :ln] = 1
    got = eng.generate(ids, pxs, n, graph=graph, attention_mask=mask)
    assert got.shape == (B, n)
    got = got.cpu().numpy()
    for b, ln in enumerate(IMG_LENS):
        one_ids, one_px = ids[b:b + 1, :ln].contiguous(), pxs[b:b + 1]
        want = eng.generate(one_ids, one_px, n, graph=graph).cpu().numpy()[0]
        # the single row's top-2 margins along its own tokens (a teacher-forced pass)
        kv1 = eng.new_kv(1, ln + n + 1)
        lg = eng.lm_forward(kv1, 0, torch.arange(ln)[None], ids=one_ids, image_feats=eng.project(eng.vision(one_px)),
                            logits_rows=2)[:, 0]
        margins = []
        for t in range(n):
            top2 = lg[0].topk(2).values
            margins.append(float(top2[0] - top2[1]))
            if t + 1 < n:
                lg = eng.decode(torch.tensor([int(want[t])], device="cuda"), kv1, ln + t, ln + t + 1)
        low = [t for t, m in enumerate(margins) if m < 0.25]
        upto = low[0] if low else n
        assert upto >= 4, (b, margins)              # every row is compared on at least 4 of its 8 steps
        assert np.array_equal(got[b, :upto], want[:upto]), (b, got[b], want, margins)
    # the left-padded form of the same batch gives the same tokens
    ids_l = torch.full_like(ids, 7)
    mask_l = torch.zeros_like(mask)
    for b, ln in enumerate(IMG_LENS):
        ids_l[b, Lmax - ln:] = ids[b, :ln]
        mask_l[b, Lmax - ln:] = 1
    got_l = eng.generate(ids_l, pxs, n, graph=graph, attention_mask=mask_l)
    assert torch.equal(got_l.cpu(), torch.from_numpy(got))
    # eos = row 0's 4th free-running token: test_eos_stops_each_row's rules
    eos, pad = int(got[0, 3]), -7
    e_toks, e_lens = eng.generate(ids, pxs, n, graph=graph, attention_mask=mask, eos_token_id=eos, pad_token_id=pad,
                                  sync_every=2, return_lengths=True)
    e_toks, e_lens = e_toks.cpu().numpy(), e_lens.cpu().numpy()
    want_len = []
    for r in range(B):
        hits = np.nonzero(got[r] == eos)[0]
        want_len.append(int(hits[0]) + 1 if len(hits) else n)
    assert list(e_lens) == want_len, (e_lens, want_len, got)
    assert e_toks.shape == (B, max(want_len))
    for r in range(B):
        k = want_len[r]
        assert np.array_equal(e_toks[r, :k], got[r, :k]), (r, e_toks[r], got[r])
        assert (e_toks[r, k:] == pad).all(), (r, e_toks[r])
    # sampling with an all-ones mask is today's path, bit for bit
    full = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    s0 = eng.generate(full, pxs, n, graph=graph, do_sample=True, generator=torch.Generator("cuda").manual_seed(3))
    s1 = eng.generate(full, pxs, n, graph=graph, do_sample=True, generator=torch.Generator("cuda").manual_seed(3),
                      attention_mask=torch.ones_like(full))
    assert torch.equal(s0, s1)


# ---------------------------------------------------------------- 10. argument checks
def test_argument_checks(eng, gold):
    rows = text_rows([8, 5])
    ids = padded(rows, 0)
    pos = torch.arange(8).expand(2, 8)
    kv = eng.new_kv(2, 16)
    with pytest.raises(ValueError):
        eng.lm_forward(kv, 0, pos, ids=ids, logits_rows=1, lens=[8, 0])
    with pytest.raises(ValueError):
        eng.lm_forward(kv, 0, pos, ids=ids, logits_rows=1, lens=[9, 5])
    eng.lm_forward(kv, 0, pos, ids=ids, logits_rows=1, lens=[8, 5])
    cur = torch.tensor([3, 4], dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):     # row 0: kv_lens + n_steps = 17 > kv_max = 16
        eng.decode_ragged(cur, kv, [14, 5], [15, 6], 3)
    with pytest.raises(ValueError):     # a single step at the cache's end
        eng.decode_ragged(cur, kv, [16, 5], [17, 6])
    eng.decode_ragged(cur, kv, [14, 5], [15, 6], 2)
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    gids = torch.from_numpy(gold["ids"]).cuda()
    hole = torch.ones_like(gids)
    hole[0, 270] = 0
    with pytest.raises(ValueError):
        eng.generate(gids, px, 2, attention_mask=hole)
