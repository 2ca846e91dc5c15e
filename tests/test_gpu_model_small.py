"""Model-level parity on the 2+2-layer full-width config: libpgmi (Engine) vs the golden
vectors captured from the reference modules (tests/golden/small_bf16.npz) and vs the oracle
run here on the same synthetic weights."""
import os

import numpy as np
import pytest
import torch

from oracle import paligemma_np as O
from oracle import weights as W
from tests_helpers import check_model_parity, logit_stats

pytestmark = pytest.mark.gpu
SEED = 1234


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "small_bf16.npz"))


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    cfg = W.small_config()
    e = Engine(cfg, max_batch=8, max_seq=640, max_kv=1024)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    return e


@pytest.fixture(scope="module")
def truth_last(gold):
    """The oracle with every bf16 rounding point removed (O.fp32_truth: the reference in fp32 on the
    same bf16-valued weights) -- the floor of the SURVEY sec.8c rule on this configuration."""
    P = W.synthetic_state_dict_f32(W.small_config(), SEED)
    with O.fp32_truth():
        lg, _ = O.paligemma_prefill(P, W.small_config(), gold["ids"], O.from_bits(gold["pixels_bits"]),
                                    all_logits=False)
    return lg[:, -1]


def tap(gold, name):
    return O.from_bits(gold["tap_" + name])


def test_vision_tower(eng, gold):
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    feats = eng.vision(px).float().cpu().numpy()
    assert rel_l2(feats[:, ::8], tap(gold, "vision_out")) < 1e-2
    proj = eng.project(eng.vision(px)).float().cpu().numpy()
    assert rel_l2(proj[:, ::8], tap(gold, "image_features")) < 1.5e-2


def test_prefill_logits(eng, gold, truth_last):
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    ids = torch.from_numpy(gold["ids"]).cuda()
    L = ids.shape[1]
    kv = eng.new_kv(1, 1024)
    feats = eng.project(eng.vision(px))
    logits = eng.lm_forward(kv, 0, torch.arange(L)[None], ids=ids, image_feats=feats, logits_rows=0)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    ref_last = gold["prefill_logits_last"]
    # SURVEY sec.8c per-step rule against the reference bf16, with its own error vs fp32 as floor
    check_model_parity("small/prefill_last", lg[:, -1], ref_last, truth_last)
    # every 32nd row (no fp32 truth for the other rows: the last row's floor is what 3e-2 covers)
    st = logit_stats("small/prefill_rows", lg[0, ::32], O.from_bits(gold["prefill_logits_rows"])[0])
    assert st["rel_vs_ref_bf16_max"] < 3e-2
    # last-row-only mode (decode GEMV kernel) gives the same numbers up to reassociation
    kv2 = eng.new_kv(1, 1024)
    last = eng.lm_forward(kv2, 0, torch.arange(L)[None], ids=ids, image_feats=feats, logits_rows=1)
    assert rel_l2(last.cpu().numpy()[:, 0], lg[:, -1]) < 1e-3  # GEMV vs GEMM accumulation order
    # KV cache rows vs the reference's KVCache (layer 0 and last; every 4th row)
    k0 = kv[0, 0, 0, :L].float().cpu().numpy()[::4]
    assert rel_l2(k0, O.from_bits(gold["k0"])[0, 0]) < 1e-2
    vl = kv[-1, 1, 0, :L].float().cpu().numpy()[::4]
    assert rel_l2(vl, O.from_bits(gold["v_last"])[0, 0]) < 3e-2


@pytest.mark.parametrize("B", [1, 3])
def test_last_row_only_final_layer(eng, gold, B):
    """logits_rows 2 (the generate loop's prefill): every row's K/V is written exactly as in the
    all-row pass (bit-identical cache), the last layer's attention / o_proj / MLP / final norm run
    for the last row alone on the decode GEMVs, so the last-row logits match logits_rows 1 up to
    accumulation order; the other rows' final hidden states are not kept (final_hidden refuses)."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2)])[:B].contiguous()
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    feats = eng.project(eng.vision(pxs))
    pos = torch.arange(L).expand(B, L)
    kv1, kv2 = eng.new_kv(B, 1024), eng.new_kv(B, 1024)
    l1 = eng.lm_forward(kv1, 0, pos, ids=ids, image_feats=feats, logits_rows=1)[:, 0]
    h1 = eng.final_hidden(B * L)
    l2 = eng.lm_forward(kv2, 0, pos, ids=ids, image_feats=feats, logits_rows=2)[:, 0]
    torch.cuda.synchronize()
    assert torch.equal(kv1[:, :, :, :L], kv2[:, :, :, :L])
    for b in range(B):
        # one layer (of this model's two) on the decode kernels: GEMV-vs-GEMM accumulation order,
        # flash-decoding's chunk-local bf16 p, then bf16 rounding of the residual
        # stream (measured 1.9e-3 at B = 1, 5.1e-3 at B = 3 on the MFMA GEMVs)
        assert rel_l2(l2[b].cpu().numpy(), l1[b].cpu().numpy()) < 1e-2
        assert int(l2[b].argmax()) == int(l1[b].argmax())
    assert torch.isfinite(h1).all()
    with pytest.raises(AssertionError):
        eng.final_hidden(B * L)
    if B == 1:
        assert rel_l2(l2[0].cpu().numpy(), gold["prefill_logits_last"]) < 3e-2
    with pytest.raises(ValueError):
        eng.lm_forward(kv2, 0, pos, ids=ids, image_feats=feats, logits_rows=3)


@pytest.mark.parametrize("B", [1, 3])
def test_prefill_graph_replay_matches_eager(eng, gold, B):
    """The prefill hipGraphs (vision tower, language-model forward; engine_graph.h run_graphed): the
    first call with a given buffer set runs eagerly, the second captures, later ones replay.
    Every call of the sequence -- eager, capture, replay, replay after the inputs changed in
    place -- is bit-identical to an eager run with graphs switched off, and the replayed logits
    still meet the reference's golden (the graph reads its buffers, not a baked copy)."""
    from pgmi import _native as N
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2)])[:B].contiguous().float()
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    c = eng.cfgd
    n_img = (c["v_image"] // c["v_patch"]) ** 2
    pos = torch.arange(L).expand(B, L).contiguous()             # host positions (copied per call)
    kv = eng.new_kv(B, 1024)
    # fixed buffers: the graph key is every pointer the call reads or writes (engine_graph.h run_graphed)
    vout = torch.empty((B, n_img, c["v_hidden"]), dtype=torch.bfloat16, device="cuda")
    feats = torch.empty((B, n_img, c["projection_dim"]), dtype=torch.bfloat16, device="cuda")
    logits = torch.empty((B, 1, c["t_vocab"]), dtype=torch.float32, device="cuda")
    lib, s = eng.lib, eng._s()

    def run():
        N.check(lib.pgmi_vision(eng.ctx, pxs.data_ptr(), N.DTYPE_F32, B, vout.data_ptr(), s))
        N.check(lib.pgmi_project(eng.ctx, vout.data_ptr(), B * n_img, feats.data_ptr(), s))
        N.check(lib.pgmi_lm_forward(eng.ctx, ids.data_ptr(), feats.data_ptr(), B * n_img, None, B, L, pos.data_ptr(),
                                    kv.data_ptr(), B, kv.shape[3], 0, logits.data_ptr(), 1, s))
        return logits[:, 0].clone()

    try:
        eng.set_prefill_graph(False)
        want = run()
        want_feats = feats.clone()
        eng.set_prefill_graph(True)
        for i in range(4):                                  # eager, capture, replay, replay
            got = run()
            torch.cuda.synchronize()
            assert torch.equal(feats, want_feats), i
            assert torch.equal(got, want), i
        # inputs changed in place: the replay follows them (eager run of the flipped batch)
        pxs.copy_(pxs.flip(-1))
        got = run()
        eng.set_prefill_graph(False)
        want2 = run()
        assert torch.equal(got, want2)
        assert not torch.equal(want2, want)
    finally:
        eng.set_prefill_graph(True)
    if B == 1:
        assert rel_l2(want.cpu().numpy(), gold["prefill_logits_last"]) < 3e-2


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_tokens(eng, gold, graph):
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    ids = torch.from_numpy(gold["ids"]).cuda()
    toks = eng.generate(ids, px, 16, graph=graph).cpu().numpy()
    ref = gold["greedy_tokens"].reshape(1, -1)
    # margins of the reference's own greedy choices: a step whose top-2 margin is below
    # 0.25 may legitimately flip under bf16 reassociation
    rl = O.from_bits(gold["greedy_logits"])
    s = np.sort(rl, -1)
    margin = s[:, -1] - s[:, -2]
    first_diff = int(np.argmax(toks[0] != ref[0])) if (toks[0] != ref[0]).any() else None
    if first_diff is not None:
        assert margin[first_diff] < 0.25, (toks, ref, margin)


def test_batched_decode_matches_single(eng, gold):
    """B=3 lock-step decode (new capability): each row equals the B=1 run of that image."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2)])
    ids = torch.from_numpy(gold["ids"]).cuda().expand(3, -1).contiguous()
    tb = eng.generate(ids, pxs, 6, graph=False).cpu().numpy()
    for i in range(3):
        t1 = eng.generate(ids[i:i + 1], pxs[i:i + 1], 6, graph=False).cpu().numpy()
        assert np.array_equal(tb[i], t1[0]), (i, tb[i], t1[0])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("graph", [False, True])
def test_decode_steps_equal_single_steps(eng, gold, B, graph):
    """pgmi_decode_steps (n greedy steps per call, one hipGraph launch at graph=True; Engine.generate's greedy
    loop) runs pgmi_decode's step kernel for kernel: its token record, the ids fed back in place, the last
    step's logits and the KV rows equal n single-step calls bit for bit -- on the eager first call, the
    capturing second and a replay."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    base = px[0]
    pxs = torch.stack([base, base.flip(-1), base.flip(-2)][:B])
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    n = 5
    feats = eng.project(eng.vision(pxs))
    V = eng.cfgd["t_vocab"]

    def prefill(kv):
        lg = eng.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=1)[:, 0]
        return eng.argmax(lg)

    kv1 = eng.new_kv(B, L + n + 1)
    first = prefill(kv1)
    cur = first.clone()
    lg1 = torch.empty((B, V), dtype=torch.float32, device="cuda")
    ref = []
    for t in range(n):
        eng.decode(cur, kv1, L + t, L + t + 1, logits=lg1, next_ids=cur, graph=graph)
        ref.append(cur.clone())
    ref = torch.stack(ref)
    kv2 = eng.new_kv(B, L + n + 1)
    prefill(kv2)
    cur2 = torch.empty_like(first)
    rec = torch.empty((n, B), dtype=torch.int64, device="cuda")
    lg2 = torch.empty((B, V), dtype=torch.float32, device="cuda")
    for rep in range(3):
        cur2.copy_(first)
        rec.fill_(-1)
        lg2.fill_(float("nan"))
        eng.decode_steps(cur2, kv2, L, L + 1, n, logits=lg2, tokens=rec, graph=graph)
        torch.cuda.synchronize()
        assert torch.equal(rec, ref), (rep, rec, ref)
        assert torch.equal(cur2, ref[-1]) and torch.equal(lg2, lg1), rep
        assert torch.equal(kv2[:, :, :, :L + n], kv1[:, :, :, :L + n]), rep
    with pytest.raises(ValueError):  # the n steps' KV rows must fit the cache
        eng.decode_steps(cur2, kv2, L, L + 1, n + 2, logits=lg2, graph=graph)


@pytest.mark.parametrize("B", [2, 8])
def test_batched_decode_logits_match_single(eng, gold, B):
    """B lock-step sequences (BASELINE configs[3]: 8 images per GPU; B >= 3 runs the MFMA decode
    projections of kernels_gemv_mfma.hip): teacher-forced on each row's own B=1 tokens, every
    step's logits match that row's B=1 logits (rel-L2 <= 3e-2, the model-level bound used against
    the reference goldens: B rows change the prefill GEMM plans, hence the accumulation order;
    |d| <= 0.25 at the top-8) and the greedy pick agrees wherever the B=1 top-2 margin exceeds 0.25."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    base = px[0]
    pxs = torch.stack([base, base.flip(-1), base.flip(-2), base.flip(-1).flip(-2), base.roll(7, -1),
                       base.roll(11, -2), -base, base * 0.5][:B])
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    n = 6
    kvb = eng.new_kv(B, L + n + 1)
    lb = eng.lm_forward(kvb, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=eng.project(eng.vision(pxs)),
                        logits_rows=1)[:, 0]
    singles = []
    for i in range(B):
        kv1 = eng.new_kv(1, L + n + 1)
        l1 = eng.lm_forward(kv1, 0, torch.arange(L)[None], ids=ids[i:i + 1],
                            image_feats=eng.project(eng.vision(pxs[i:i + 1])), logits_rows=1)[:, 0]
        steps = [l1.clone()]
        tok = l1.argmax(-1)
        toks = [tok]
        for t in range(1, n):
            l1 = eng.decode(tok, kv1, L + t - 1, L + t).clone()
            steps.append(l1)
            tok = l1.argmax(-1)
            toks.append(tok)
        singles.append((torch.cat(steps), torch.cat(toks)))
    for t in range(n):
        ref = torch.stack([s[0][t] for s in singles])
        got = lb if t == 0 else eng.decode(torch.stack([s[1][t - 1] for s in singles]), kvb, L + t - 1, L + t).clone()
        for i in range(B):
            r, gq = ref[i].cpu().numpy(), got[i].cpu().numpy()
            assert rel_l2(gq, r) < 3e-2, (t, i)
            top = np.argsort(r)[-8:]
            assert np.abs(gq[top] - r[top]).max() <= 0.25, (t, i)
            srt = np.sort(r)
            if srt[-1] - srt[-2] > 0.25:
                assert int(gq.argmax()) == int(r.argmax()), (t, i)


def test_eos_stops_each_row(eng, gold):
    """Stop token (inference.py:51,70-71) per row on the device: a row keeps its first eos and
    emits pad after it; lengths = tokens up to and including eos; the loop ends once every row
    has stopped and the result is trimmed to the longest row."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2)])
    ids = torch.from_numpy(gold["ids"]).cuda().expand(3, -1).contiguous()
    n = 12
    free = eng.generate(ids, pxs, n, graph=True).cpu().numpy()
    eos = int(free[0, 3])
    pad = -7
    got, lens = eng.generate(ids, pxs, n, graph=True, eos_token_id=eos, pad_token_id=pad, sync_every=2,
                             return_lengths=True)
    got, lens = got.cpu().numpy(), lens.cpu().numpy()
    want_len = []
    for r in range(3):
        hits = np.nonzero(free[r] == eos)[0]
        want_len.append(int(hits[0]) + 1 if len(hits) else n)
    assert list(lens) == want_len, (lens, want_len, free)
    assert got.shape == (3, max(want_len))
    for r in range(3):
        k = want_len[r]
        assert np.array_equal(got[r, :k], free[r, :k]), (r, got[r], free[r])
        assert (got[r, k:] == pad).all(), (r, got[r])
    # a B=1 run matches the reference loop exactly: generated tokens end at (and include) eos
    one = eng.generate(ids[:1], pxs[:1], n, graph=True, eos_token_id=eos).cpu().numpy()
    assert np.array_equal(one[0], free[0, :want_len[0]])


def test_eos_update_kernel(eng):
    """pgmi_eos_update against a host restatement on ragged rows (B = 300 > one workgroup's lanes)."""
    g = torch.Generator().manual_seed(5)
    B, eos, pad = 300, 1, 0
    nxt = torch.randint(0, 4, (B,), generator=g)
    fin = (torch.rand(B, generator=g) < 0.3).to(torch.int32)
    want_n = torch.where(fin.bool(), torch.full_like(nxt, pad), nxt)
    want_f = fin | (nxt == eos).to(torch.int32)
    want_alive = int(((fin == 0) & (nxt != eos)).sum())
    nd, fd = nxt.cuda(), fin.cuda()
    alive = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    eng._eos_update(nd, fd, eos, pad, alive)
    torch.cuda.synchronize()
    assert torch.equal(nd.cpu(), want_n)
    assert torch.equal(fd.cpu(), want_f)
    assert int(alive.item()) == want_alive


@pytest.mark.parametrize("B", [1, 4])
def test_inplace_feedback_matches_staged(eng, gold, B):
    """pgmi_decode with next_ids == ids (graph reads and overwrites the caller's buffer, no
    staging copy) produces the same tokens and logits as the staged form."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2), px[0].flip(-1).flip(-2)])[:B].contiguous()
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    feats = eng.project(eng.vision(pxs))
    runs = []
    for inplace in (False, True):
        kv = eng.new_kv(B, 1024)
        lg = eng.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=1)
        cur = eng.argmax(lg[:, 0])
        nxt = torch.empty_like(cur)
        logits = torch.empty((B, eng.cfgd["t_vocab"]), dtype=torch.float32, device="cuda")
        seq = []
        for t in range(1, 7):
            if inplace:
                eng.decode(cur, kv, L + t - 1, L + t, logits=logits, next_ids=cur, graph=True)
            else:
                eng.decode(cur, kv, L + t - 1, L + t, logits=logits, next_ids=nxt, graph=True)
                cur.copy_(nxt)
            seq.append(cur.clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(seq, 1).cpu(), logits.cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    # the argmax folded into lm_head's last workgroup == torch.argmax of the returned logits
    assert torch.equal(runs[1][0][:, -1], runs[1][1].argmax(-1))


@pytest.mark.parametrize("B", [1, 4])
def test_decode_past_768_keys_vs_oracle(B):
    """KV length past 768 keys: batch-1 decode switches the o_proj prologue's attention combine to
    its two-pass form (gemv_body.h, > 12 chunks of 64 keys); B >= 3 decodes on the MFMA path with
    the k_attn_combine kernel.  A ~1000-token text prompt is prefilled, then 4 decode steps are
    teacher-forced along the oracle's greedy tokens and compared row by row (same rules as the
    other model-level tests: the per-step rel-L2 rule against the oracle bf16 with the oracle's fp32
    truth as floor, |delta| <= 0.25 at the oracle's top-8, argmax where the oracle's top-2 margin
    exceeds 0.25)."""
    from pgmi import Engine
    cfg = W.small_config()
    L, steps = 1000, 4
    e = Engine(cfg, max_batch=B, max_seq=L, max_kv=L + 64)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    rng = np.random.default_rng(5)
    ids = rng.integers(3, cfg["text_config"]["vocab_size"] - 1, size=(B, L)).astype(np.int64)
    ids[:, 0] = 2
    P = W.synthetic_state_dict_f32(cfg, SEED)
    P = {n: v for n, v in P.items() if n.startswith("language_model")}
    emb = O.merge(P, cfg, None, ids)
    okv = O.KV()
    ref = O.gemma_forward(P, cfg, emb, np.broadcast_to(np.arange(L), (B, L)), okv, all_logits=False)[:, -1]
    # the fp32 truth along the same (oracle-bf16 greedy) tokens: the floor of the per-step rule
    fkv = O.KV()
    with O.fp32_truth():
        tru = O.gemma_forward(P, cfg, emb, np.broadcast_to(np.arange(L), (B, L)), fkv, all_logits=False)[:, -1]
    kv = e.new_kv(B, L + 64)
    got = e.lm_forward(kv, 0, torch.arange(L)[None], ids=torch.from_numpy(ids).cuda(), logits_rows=1)[:, 0]
    logits = torch.empty((B, cfg["text_config"]["vocab_size"]), dtype=torch.float32, device="cuda")
    hist = []
    for t in range(steps + 1):
        g = got.cpu().numpy()
        hist.append((g, ref, tru))
        for b in range(B):
            top = np.argsort(ref[b])[-8:]
            assert np.abs(g[b][top] - ref[b][top]).max() <= 0.25, (t, b)
            s = np.sort(ref[b])
            if s[-1] - s[-2] > 0.25:
                assert int(g[b].argmax()) == int(ref[b].argmax()), (t, b)
        if t == steps:
            break
        nxt = ref.argmax(-1)                               # teacher-forced on the oracle's tokens
        ref = O.paligemma_decode(P, cfg, nxt, okv, L + 1 + t)[:, -1]
        with O.fp32_truth():
            tru = O.paligemma_decode(P, cfg, nxt, fkv, L + 1 + t)[:, -1]
        got = e.decode(torch.from_numpy(nxt).cuda(), kv, L + t, L + 1 + t, logits=logits, graph=t > 0).clone()
    for b in range(B):
        check_model_parity(f"small/decode_past_768_B{B}/row{b}", np.stack([h[0][b] for h in hist]),
                           np.stack([h[1][b] for h in hist]), np.stack([h[2][b] for h in hist]))
    del e
    torch.cuda.empty_cache()


def test_rccl_weight_broadcast_single_rank(eng):
    """pgmi_comm_unique_id / pgmi_comm_init / pgmi_broadcast_weights (the replicas' load-time RCCL
    broadcast through the C ABI) on a one-rank communicator: the slab comes back unchanged."""
    import ctypes
    from pgmi import _native as N
    lib = eng.lib
    uid = (ctypes.c_uint8 * 128)()
    N.check(lib.pgmi_comm_unique_id(uid))
    comm = ctypes.c_void_p()
    N.check(lib.pgmi_comm_init(eng.device.index, 1, 0, uid, ctypes.byref(comm)))
    before = eng.slab[::4099].clone()
    try:
        N.check(lib.pgmi_broadcast_weights(eng.ctx, comm, 0, eng._s()))
        torch.cuda.synchronize()
    finally:
        N.check(lib.pgmi_comm_destroy(comm))
    assert torch.equal(eng.slab[::4099], before)
    eng.prepare()


@pytest.mark.parametrize("mask_dtype", ["bf16", "fp32"])
def test_decode_embeds_dev_position_and_mask(eng, gold, mask_dtype):
    """pgmi_decode_embeds_dev (the ablation harness's q_len == 1 steps without a host read): the
    rotary position and the additive mask are read on the device.  A zero mask gives exactly the
    host-position step's logits; a mask hiding the first 40 keys matches the oracle with the same
    additive mask (modeling_gemma.py:269; bf16 mask: score + mask rounded to bf16, fp32 mask: added
    in fp32)."""
    cfg = W.small_config()
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    ids = torch.from_numpy(gold["ids"]).cuda()
    L = ids.shape[1]
    feats = eng.project(eng.vision(px))
    kv = eng.new_kv(1, 1024)
    eng.lm_forward(kv, 0, torch.arange(L)[None], ids=ids, image_feats=feats, logits_rows=1)
    tok = 108
    row = eng.embed(torch.tensor([[tok]], device="cuda"))[:, 0]
    host = eng.decode_embeds(row, kv, L, L + 1, graph=False).clone()
    dt = torch.bfloat16 if mask_dtype == "bf16" else torch.float32
    pos = torch.tensor([[float(L + 1)]], device="cuda")
    zero = torch.zeros((1, 1, 1, L + 1), dtype=dt, device="cuda")
    dev = eng.decode_embeds_dev(row, kv, L, pos, zero, graph=False).clone()
    assert torch.equal(host, dev)
    m = torch.zeros((1, 1, 1, L + 1), dtype=torch.float32)
    m[..., :40] = -1e4
    got = eng.decode_embeds_dev(row, kv, L, pos, m.to("cuda", dt), graph=False).clone().cpu().numpy()[0]
    # the oracle over the same prompt, then the one-token step with the same additive mask
    P = W.synthetic_state_dict_f32(cfg, SEED)
    _, okv = O.paligemma_prefill(P, cfg, gold["ids"], O.from_bits(gold["pixels_bits"]), all_logits=False)
    emb = O.merge(P, cfg, None, np.array([[tok]]))
    # (unmasked keys add an exact 0 in either dtype; masked ones vanish from the softmax in both, so the
    # oracle's bf16 add is the reference for both mask dtypes)
    ref = O.gemma_forward(P, cfg, emb, np.full((1, 1), L + 1), okv, mask=O.bf16(m.numpy()))[0, -1]
    assert rel_l2(got, ref) < 3e-2, rel_l2(got, ref)
    top = np.argsort(ref)[-8:]
    assert np.abs(got[top] - ref[top]).max() <= 0.25
    assert rel_l2(got, host.cpu().numpy()[0]) > 1e-3  # the mask changed the step


@torch.no_grad()
def test_prefill_probe_kernel_events(eng, gold):
    """pgmi_prefill_probe (bench.py's in-situ GEMM timing): every layer's gate|up and down GEMM kernel takes
    its own start / stop events; the probed (eager) forward returns the same logits as the unprobed one,
    every time is positive and below a bound, and switching the probe off restores the graphs.  logits_rows 1
    (every layer's MLP on every row, as bench.py probes it): with 2 the last layer's MLP runs for the last row
    on the decode GEMVs, so it has no GEMM to time and pgmi_prefill_probe_times reports an error."""
    import ctypes

    from pgmi import _native as N
    ids = torch.from_numpy(gold["ids"]).cuda()
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    feats = eng.project(eng.vision(px))
    L = ids.shape[1]
    kv = eng.new_kv(1, 512)
    pos = torch.arange(L)[None]
    ref = eng.lm_forward(kv, 0, pos, ids=ids, image_feats=feats, logits_rows=1).clone()
    nl = W.small_config()["text_config"]["num_hidden_layers"]
    us = (ctypes.c_float * (2 * nl))()
    N.check(eng.lib.pgmi_prefill_probe(eng.ctx, 1))
    try:
        out = eng.lm_forward(kv, 0, pos, ids=ids, image_feats=feats, logits_rows=1).clone()
        torch.cuda.synchronize()
        N.check(eng.lib.pgmi_prefill_probe_times(eng.ctx, us, 2 * nl))
    finally:
        N.check(eng.lib.pgmi_prefill_probe(eng.ctx, 0))
    assert torch.equal(out, ref)
    t = list(us)
    assert all(1.0 < v < 5000.0 for v in t), t
    again = eng.lm_forward(kv, 0, pos, ids=ids, image_feats=feats, logits_rows=1)
    assert torch.equal(again, ref)


# ---------------------------------------------------------------- the two graph caches (pgmi_graph_count)
GRAPH_CACHE_MAX = 64  # include/pgmi.h PGMI_GRAPH_CACHE_MAX


def graph_count(eng, which):
    """Keys in the context's prefill (0) or decode (1) graph cache."""
    return eng.lib.pgmi_graph_count(eng.ctx, which)


def _prefilled(eng, gold, B, kv):
    """Prefill kv with B copies of the golden prompt (flipped images); returns (L, first tokens)."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2), px[0].flip(-1).flip(-2)])[:B].contiguous()
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    lg = eng.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=eng.project(eng.vision(pxs)),
                        logits_rows=1)
    return L, eng.argmax(lg[:, 0]), ids, pxs


def test_decode_graph_cache_is_bounded(eng, gold):
    """The decode graph cache holds at most PGMI_GRAPH_CACHE_MAX keys: 70 distinct logits buffers (70 keys, each
    called twice: eager, then capture + launch) never leave more than 64 entries behind, and a step run through
    a cache that was dropped on the way still returns the eager step's logits bit for bit."""
    eng.set_decode_staged_norm(-1)  # an empty decode cache to start from
    assert graph_count(eng, 1) == 0
    kv = eng.new_kv(1, 512)
    L, cur, _, _ = _prefilled(eng, gold, 1, kv)
    V = eng.cfgd["t_vocab"]
    bufs = [torch.empty((1, V), dtype=torch.float32, device="cuda") for _ in range(70)]  # all alive: 70 addresses
    assert len({b.data_ptr() for b in bufs}) == 70
    counts = []
    for b in bufs:
        for _ in range(2):
            eng.decode(cur, kv, L, L + 1, logits=b, graph=True)
            counts.append(graph_count(eng, 1))
    torch.cuda.synchronize()
    assert max(counts) <= GRAPH_CACHE_MAX, counts
    assert max(counts) == GRAPH_CACHE_MAX and counts[-1] < GRAPH_CACHE_MAX, counts  # filled, then dropped
    want = eng.decode(cur, kv, L, L + 1, graph=False)
    torch.cuda.synchronize()
    assert torch.equal(bufs[-1], want)
    assert torch.equal(bufs[0], want)


@pytest.mark.parametrize("B,n_tokens", [(4, 10), (1, 6)])
def test_repeated_generate_replays_its_graphs(eng, gold, B, n_tokens):
    """Lock-step generate keeps its step buffers per batch size, so calls on the same cache replay the decode
    graphs they captured instead of capturing new ones: B = 4 runs two chunks of the multi-step path (8 steps,
    then 1), B = 1 the single-step path.  Every call returns the eager loop's tokens."""
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    pxs = torch.stack([px[0], px[0].flip(-1), px[0].flip(-2), px[0].flip(-1).flip(-2)])[:B].contiguous()
    ids = torch.from_numpy(gold["ids"]).cuda().expand(B, -1).contiguous()
    kv = eng.new_kv(B, ids.shape[1] + n_tokens + 1)
    want = eng.generate(ids, pxs, n_tokens, graph=False, kv=kv)
    got, counts = [], []
    for _ in range(3):
        got.append(eng.generate(ids, pxs, n_tokens, graph=True, kv=kv))
        counts.append(graph_count(eng, 1))
    torch.cuda.synchronize()
    assert counts[2] == counts[1], counts
    for i, g in enumerate(got):
        assert torch.equal(g, want), (i, g, want)


def test_graph_caches_clear_selectively(eng, gold):
    """pgmi_set_prefill_graph drops the prefill graphs only, pgmi_set_decode_staged_norm the decode graphs only,
    pgmi_prepare both."""
    from pgmi import _native as N
    c = eng.cfgd
    n_img = (c["v_image"] // c["v_patch"]) ** 2
    kv = eng.new_kv(1, 512)
    L, cur, ids, pxs = _prefilled(eng, gold, 1, kv)
    pos = torch.arange(L)[None].contiguous()
    feats = eng.project(eng.vision(pxs))
    # fixed buffers: the prefill key is every pointer the call reads or writes
    logits = torch.empty((1, 1, c["t_vocab"]), dtype=torch.float32, device="cuda")
    step_logits = eng.logits_buffer(1)

    def prefill_pair():
        for _ in range(2):
            N.check(eng.lib.pgmi_lm_forward(eng.ctx, ids.data_ptr(), feats.data_ptr(), n_img, None, 1, L,
                                            pos.data_ptr(), kv.data_ptr(), 1, kv.shape[3], 0, logits.data_ptr(), 1,
                                            eng._s()))

    def decode_pair():
        for _ in range(2):
            eng.decode(cur, kv, L, L + 1, logits=step_logits, graph=True)

    prefill_pair()
    decode_pair()
    n0, n1 = graph_count(eng, 0), graph_count(eng, 1)
    assert n0 > 0 and n1 > 0
    eng.set_prefill_graph(True)
    assert (graph_count(eng, 0), graph_count(eng, 1)) == (0, n1)
    prefill_pair()
    n0 = graph_count(eng, 0)
    assert n0 > 0
    eng.set_decode_staged_norm(-1)
    assert (graph_count(eng, 0), graph_count(eng, 1)) == (n0, 0)
    decode_pair()
    assert graph_count(eng, 1) > 0
    eng.prepare()
    assert (graph_count(eng, 0), graph_count(eng, 1)) == (0, 0)


def test_tune_call_makes_a_new_prefill_key(eng, gold):
    """A pgmi_tune_* call changes which kernels a prefill body launches: the tuning epoch is part of the prefill
    key, so the next call runs eagerly under a new key instead of replaying the graph of the other plan."""
    from pgmi import _native as N
    c = eng.cfgd
    n_img = (c["v_image"] // c["v_patch"]) ** 2
    kv = eng.new_kv(1, 512)
    L, cur, ids, pxs = _prefilled(eng, gold, 1, kv)
    pos = torch.arange(L)[None].contiguous()
    feats = eng.project(eng.vision(pxs))
    logits = torch.empty((1, 1, c["t_vocab"]), dtype=torch.float32, device="cuda")

    def prefill():
        N.check(eng.lib.pgmi_lm_forward(eng.ctx, ids.data_ptr(), feats.data_ptr(), n_img, None, 1, L, pos.data_ptr(),
                                        kv.data_ptr(), 1, kv.shape[3], 0, logits.data_ptr(), 1, eng._s()))

    prefill()
    prefill()
    n = graph_count(eng, 0)
    assert 0 < n <= 64
    try:
        N.check(eng.lib.pgmi_tune_attention(0))
        prefill()
        assert graph_count(eng, 0) == n + 1 <= 64
    finally:
        N.check(eng.lib.pgmi_tune_attention(-1))
    prefill()
    assert graph_count(eng, 0) == n + 2 <= 64
    torch.cuda.synchronize()
