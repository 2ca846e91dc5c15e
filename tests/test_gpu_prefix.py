"""The prefix-LM prefill on the MI355X (pgmi_lm_forward_prefix, pgmi_op_attention_prefix, Engine.score(prefix_lens=),
Engine.score_candidates): the attention kernel's per-query key limits against the oracle's masked arithmetic and a
float64 truth (tests/prefix_cases.py), the model against the masked oracle, one pass against a prefill and decode
steps on the engine itself, and scoring against generate's own log-probabilities.  The 2+2-layer full-width config and
the rules of tests/test_gpu_model_small.py and tests/test_gpu_logprobs.py throughout."""
import os

import numpy as np
import pytest
import torch

import prefix_cases as PC
from oracle import paligemma_np as O
from oracle import weights as W
from pgmi import prefix_np as PX
from pgmi.scoring import logprobs_np
from tests_helpers import check_model_parity

pytestmark = pytest.mark.gpu
IGN = -100


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.small_config(), max_batch=16, max_seq=320, max_kv=1024)
    e.fill_synthetic(PC.SEED, W.init_policy)
    e.prepare()
    return e


def graph_count(eng):
    return eng.lib.pgmi_graph_count(eng.ctx, 0)


def bf16_cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def padded(rows, pad=0):
    ids = np.full((len(rows), max(len(r) for r in rows)), pad, dtype=np.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = r
    return torch.from_numpy(ids).cuda()


# ---------------------------------------------------------------- 4. the kernel
@pytest.mark.parametrize("name", list(PC.CASES))
def test_attention_prefix_kernel(eng, name):
    from pgmi import _native as N
    c = PC.CASES[name]
    q, k, v = PC.inputs(name)              # K/V behind each row's keys: NaN -- no query may read them
    Lk = c.kv_start + c.Lq
    rows, tail = c.B * c.Lq, 4
    dq, dk, dv = bf16_cuda(q), bf16_cuda(k), bf16_cuda(v)
    out = torch.full((rows + tail, PC.QD), 7.0, dtype=torch.bfloat16, device="cuda")
    klen = None if c.lens is None else torch.tensor([c.kv_start + n for n in c.lens], dtype=torch.int32)
    pfx = torch.tensor(c.prefix, dtype=torch.int32)
    # the key ranges this call is split into: the case aimed at the partials and their combine must have two
    assert eng.lib.pgmi_op_attention_prefix_splits(eng.ctx, c.B, c.Lq, PC.NH, PC.NKV, c.kv_start) == \
        PC.SPLITS.get(name, 1)
    N.check(eng.lib.pgmi_op_attention_prefix(eng.ctx, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), out.data_ptr(), c.B,
                                             c.Lq, Lk, PC.NH, PC.NKV, PC.HD, 0, 1.0 / 16.0, c.kv_start,
                                             None if klen is None else klen.data_ptr(), pfx.data_ptr(), eng._s()),
            "pgmi_op_attention_prefix")
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    assert np.all(got[rows:] == 7.0), "rows past the outputs were written"
    G = got[:rows].reshape(c.B, c.Lq, PC.QD)
    assert np.isfinite(G).all(), "a non-finite output: a key past a row's limit was read"
    PC.check(name, G)


# ---------------------------------------------------------------- 5. all-prefix is today's path
def test_all_prefix_is_todays_prefill(eng):
    lens = [1, 40, 23, 33]
    rows = [PC.text_row(n, 50 + n) for n in lens]
    B, L = len(rows), max(lens)
    ids = padded(rows)
    pos = torch.arange(L).expand(B, L)
    n0 = graph_count(eng)

    def run(**kw):
        kv = eng.new_kv(B, 64)
        kv.fill_(float("nan"))
        lg = eng.lm_forward(kv, 0, pos, ids=ids, logits_rows=0, **kw)
        torch.cuda.synchronize()
        return lg, kv

    want, wkv = run(lens=lens)
    n1 = graph_count(eng)
    got, gkv = run(lens=lens, prefix_lens=lens)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n], want[b, :n]), b
        assert torch.equal(gkv[:, :, b, :n], wkv[:, :, b, :n]), b
    want, wkv = run()                       # lock-step
    n2 = graph_count(eng)
    got, gkv = run(prefix_lens=[L] * B)
    assert torch.equal(got, want) and torch.equal(gkv[:, :, :, :L], wkv[:, :, :, :L])
    last = eng.lm_forward(eng.new_kv(B, 64), 0, pos, ids=ids, logits_rows=2, prefix_lens=[L] * B)
    assert torch.equal(last[:, 0], eng.lm_forward(eng.new_kv(B, 64), 0, pos, ids=ids, logits_rows=2)[:, 0])
    n3 = graph_count(eng)
    # the prefix calls neither looked a key up nor left one: only the three plain calls did
    assert (n1 - n0, n2 - n1, n3 - n2) == (1, 1, 1), (n0, n1, n2, n3)
    eng.lm_forward(eng.new_kv(B, 64), 0, pos, ids=ids, logits_rows=0, lens=lens, prefix_lens=[0, 17, 23, 5])
    assert graph_count(eng) == n3


# ---------------------------------------------------------------- 6. the model against the masked oracle
def model_vs_oracle(eng, label, rows, prefix, lens):
    B, L = len(rows), max(len(r) for r in rows)
    kv = eng.new_kv(B, L + 3)
    lg = eng.lm_forward(kv, 0, torch.from_numpy(PX.prefix_positions(L, prefix)), ids=padded(rows), logits_rows=0,
                        lens=lens, prefix_lens=prefix)
    torch.cuda.synchronize()
    g = lg.cpu().numpy()
    for b, (row, p) in enumerate(zip(rows, prefix)):
        n = len(row)
        ref, tru, (ok, ov) = PC.oracle_pass(row, p)
        lo = max(p - 1, 0)
        check_model_parity(f"prefix/{label}/row{b}_P{p}_n{n - p}", g[b, lo:n], ref[lo:], tru[lo:])
        assert rel_l2(kv[0, 0, b, :n].float().cpu().numpy(), ok[0][0, 0]) < 1e-2, (b, n)
        assert rel_l2(kv[0, 1, b, :n].float().cpu().numpy(), ov[0][0, 0]) < 1e-2, (b, n)
        assert rel_l2(kv[-1, 0, b, :n].float().cpu().numpy(), ok[-1][0, 0]) < 3e-2, (b, n)
        assert rel_l2(kv[-1, 1, b, :n].float().cpu().numpy(), ov[-1][0, 0]) < 3e-2, (b, n)


def test_model_ragged_vs_masked_oracle(eng):
    pn = [(33, 8), (64, 1), (31, 2)]
    rows = [PC.text_row(p + n, 100 * p + n) for p, n in pn]
    model_vs_oracle(eng, "ragged", rows, [p for p, _ in pn], [p + n for p, n in pn])


def test_model_second_row_group_vs_masked_oracle(eng):
    rows = [PC.text_row(8, 200 + b) for b in range(9)]
    model_vs_oracle(eng, "nine", rows, [3] * 9, None)


# ---------------------------------------------------------------- 7. one pass = stepwise, on the engine itself
def test_one_pass_is_stepwise_on_the_engine(eng):
    P, n = 33, 8
    row = PC.text_row(P + n + 1, 100 * P + n)           # the last token feeds the further step
    ids = torch.from_numpy(row)[None].cuda()
    ref, tru, _ = PC.oracle_pass(row, P)
    bound = PC.step_bound(PC.rel_rows(ref, tru))[P - 1:]   # rows P - 1 .. P + n: the floor from the oracle
    kv_s = eng.new_kv(1, 64)
    steps = [eng.lm_forward(kv_s, 0, torch.arange(P)[None], ids=ids[:, :P].contiguous(), logits_rows=1)[0, 0]]
    for t in range(n):
        steps.append(eng.decode(ids[:, P + t].contiguous(), kv_s, P + t, P + t + 1).clone()[0])
    kv_o = eng.new_kv(1, 64)
    L = P + n
    one = eng.lm_forward(kv_o, 0, torch.from_numpy(PX.prefix_positions(L, [P])), ids=ids[:, :L].contiguous(),
                         logits_rows=0, prefix_lens=[P])[0, P - 1:]
    # the last-row form of the same causal call: the last row attends every key either way (lm_last_row_tail), so
    # its logits are those of row L - 1 within test_last_row_only_final_layer's bounds, and the cache is the same
    kv_l = eng.new_kv(1, 64)
    last = eng.lm_forward(kv_l, 0, torch.from_numpy(PX.prefix_positions(L, [P])), ids=ids[:, :L].contiguous(),
                          logits_rows=2, prefix_lens=[P])[0, 0]
    assert int(last.argmax()) == int(one[-1].argmax())
    assert rel_l2(last.cpu().numpy(), one[-1].cpu().numpy()) < 1e-2
    assert torch.equal(kv_l[:, :, :, :L], kv_o[:, :, :, :L])
    steps.append(eng.decode(ids[:, L].contiguous(), kv_s, L, L + 1).clone()[0])
    further = eng.decode(ids[:, L].contiguous(), kv_o, L, L + 1).clone()[0]
    torch.cuda.synchronize()
    s = torch.stack(steps).cpu().numpy()
    g = np.concatenate([one.cpu().numpy(), further.cpu().numpy()[None]])
    r = PC.rel_rows(g, s)
    print(f"prefix one pass vs stepwise (engine): rel-L2 {r.min():.2e} .. {r.max():.2e}, bounds {bound.min():.2e} .. "
          f"{bound.max():.2e}")
    assert r.shape == bound.shape == (n + 2,)
    assert (r <= bound).all(), (r, bound)


# ---------------------------------------------------------------- 8 / 9. scoring
N_GEN = 8


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "small_bf16.npz"))


@pytest.fixture(scope="module")
def image_oracle(gold):
    """The golden image's projected features from the oracle, bf16 and fp32 (once), and the weights."""
    cfg = W.small_config()
    P = W.synthetic_state_dict_f32(cfg, PC.SEED)
    px = O.from_bits(gold["pixels_bits"])
    feats = O.project(P, O.siglip_vision(P, cfg, px))
    with O.fp32_truth():
        feats32 = O.project(P, O.siglip_vision(P, cfg, px))
    return cfg, P, feats, feats32


def oracle_answer_logprobs(image_oracle, row, p):
    """The masked oracle over one row (image prompt of p tokens, then the answer) -> the answer tokens' log-
    probabilities, bf16 and fp32."""
    cfg, P, feats, feats32 = image_oracle
    L = len(row)
    mask, pos = PX.prefix_mask(L, 0, None, [p]), PX.prefix_positions(L, [p])
    lab = np.asarray(row[p:])[None]
    ref = O.gemma_forward(P, cfg, O.merge(P, cfg, feats, row[None]), pos, O.KV(), mask=mask)
    with O.fp32_truth():
        tru = O.gemma_forward(P, cfg, O.merge(P, cfg, feats32, row[None]), pos, O.KV(), mask=mask)
    return logprobs_np(ref[:, p - 1:L - 1], lab, IGN)[0], logprobs_np(tru[:, p - 1:L - 1], lab, IGN)[0]


@pytest.fixture(scope="module")
def generated(eng, gold):
    """Two prompts over the golden image (the golden text, and random text) and the 8 tokens generate emits."""
    base = gold["ids"][0].astype(np.int64)
    other = base.copy()
    other[257:] = PC.text_row(len(base) - 257, 9)
    ids = torch.from_numpy(np.stack([base, other])).cuda()
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda().expand(2, -1, -1, -1).contiguous()
    toks, lps = eng.generate(ids, px, N_GEN, return_logprobs=True)
    return ids, px, toks, lps.cpu().numpy()


@pytest.fixture(scope="module")
def answer_floor(image_oracle, generated):
    """Per row: the masked oracle's log-probabilities of the emitted tokens, bf16 and fp32."""
    ids, _, toks, _ = generated
    full = torch.cat([ids, toks], 1).cpu().numpy()
    return [oracle_answer_logprobs(image_oracle, full[b], ids.shape[1]) for b in range(2)]


def test_score_prefix_on_generated_tokens(eng, generated, answer_floor):
    ids, px, toks, gen_lp = generated
    B, L0 = ids.shape
    full = torch.cat([ids, toks], 1)
    lab = torch.full_like(full, IGN)
    lab[:, L0:] = toks
    sc = eng.score(full, px, lab, prefix_lens=[L0] * B)
    ours = sc.logprobs[:, L0 - 1:].cpu().numpy()
    plain = eng.score(full, px, lab).logprobs[:, L0 - 1:].cpu().numpy()
    assert ours.shape == (B, N_GEN) and np.array_equal(sc.counts.cpu().numpy(), [N_GEN] * B)
    assert not sc.logprobs[:, :L0 - 1].any()
    ref = np.stack([r for r, _ in answer_floor])
    tru = np.stack([t for _, t in answer_floor])
    er = float(np.abs(ref - tru).mean())
    eo, eg, ep = (float(np.abs(x - y).mean()) for x, y in ((ours, tru), (ours, gen_lp), (plain, tru)))
    epg = float(np.abs(plain - gen_lp).mean())
    print(f"prefix score: ours vs truth {eo:.4e}, oracle bf16 vs truth {er:.4e}, ours vs generate's {eg:.4e}, "
          f"without prefix_lens vs truth {ep:.4e}, vs generate's {epg:.4e}")
    assert eo <= 1.5 * er, (eo, er)
    assert eg <= 3 * er, (eg, er)
    assert ep > 3 * er and epg > 3 * er, (ep, epg, er)     # today's non-causal score sees the answer


CAND_SEED = 1            # the oracle's fp32 gap between the two 5-token candidates: 2.45 nats (seed 3: 0.21)


def test_score_candidates(eng, generated, answer_floor, image_oracle):
    ids, px, _, _ = generated
    prompt = ids[0]
    L0 = prompt.shape[0]
    rng = np.random.default_rng([78, CAND_SEED])
    V = eng.cfgd["t_vocab"]
    cands = [[int(t) for t in rng.integers(3, V - 65, n)] for n in (1, 2, 5, 5)]
    cs = eng.score_candidates(prompt, px[:1], cands)
    er = float(np.mean([np.abs(r - t).mean() for r, t in answer_floor]))
    assert cs.sums.shape == (4,) and [int(x) for x in cs.counts.cpu()] == [1, 2, 5, 5]
    for i, c in enumerate(cands):
        row = torch.cat([prompt, torch.tensor(c, device=prompt.device)])[None]
        lab = torch.full_like(row, IGN)
        lab[:, L0:] = row[:, L0:]
        one = eng.score(row, px[:1], lab, prefix_lens=[L0])
        a, b = cs.logprobs[i].cpu().numpy(), one.logprobs[0, L0 - 1:].cpu().numpy()
        assert a.shape == b.shape == (len(c),)
        assert float(np.abs(a - b).mean()) <= 3 * er, (i, a, b, er)
        assert abs(float(cs.sums[i]) - float(a.sum())) <= 1e-4 * abs(float(a.sum()))
    # the two 5-token candidates: ranked as the oracle's fp32 ranks them (its gap asserted: > 0.25 nats)
    t2, t3 = (oracle_answer_logprobs(image_oracle, np.concatenate([prompt.cpu().numpy(), c]), L0)[1].sum()
              for c in cands[2:])
    assert abs(t2 - t3) > 0.25, (t2, t3)
    assert (float(cs.sums[2]) > float(cs.sums[3])) == (t2 > t3), (cs.sums, t2, t3)


# ---------------------------------------------------------------- 10. refusals
def test_refusals(eng):
    from pgmi import _native as N
    rows = [PC.text_row(n, 60 + n) for n in (5, 3)]
    ids = padded(rows)
    pos = torch.arange(5).expand(2, 5)
    kv = eng.new_kv(2, 16)
    for lens, pfx in (([5, 3], [-1, 0]), ([5, 3], [5, 4]), (None, [6, 0]), (None, [0, -2])):
        with pytest.raises(ValueError):
            eng.lm_forward(kv, 0, pos, ids=ids, lens=lens, prefix_lens=pfx)
    # a refused prefix length leaves the last call's final hidden rows valid (it is refused before anything is written)
    eng.lm_forward(kv, 0, pos, ids=ids, logits_rows=1)
    want = eng.final_hidden(10)
    with pytest.raises(ValueError):
        eng.lm_forward(kv, 0, pos, ids=ids, prefix_lens=[6, 0])
    assert torch.equal(eng.final_hidden(10), want)
    with pytest.raises(ValueError):
        eng.lm_forward(kv, 0, pos, ids=ids, prefix_lens=[0])                   # one entry for two rows
    with pytest.raises(ValueError):
        eng.lm_forward(kv, 0, pos, embeds=torch.zeros(2, 5, 2048), prefix_lens=[0, 0])
    V = eng.cfgd["t_vocab"]
    out = torch.empty((2, 5, V), dtype=torch.float32, device="cuda")
    p32 = torch.zeros(2, dtype=torch.int32)
    posc = pos.contiguous()

    def call(idp, posp, pfxp, kvp, outp, B=2):
        return eng.lib.pgmi_lm_forward_prefix(eng.ctx, idp, None, 0, B, 5, posp, None, pfxp, kvp, 2, 16, 0, outp, 0,
                                              eng._s())
    ok = (ids.data_ptr(), posc.data_ptr(), p32.data_ptr(), kv.data_ptr(), out.data_ptr())
    for i in range(5):                                                          # each array null in turn
        args = list(ok)
        args[i] = None
        assert call(*args) == N.PGMI_E_ARG, i
    assert call(*ok, B=3) == N.PGMI_E_ARG                                       # more rows than the cache holds
    big = padded([PC.text_row(4, b) for b in range(17)])
    with pytest.raises(ValueError):                                          # B over the context's capacity
        eng.lm_forward(eng.new_kv(17, 8), 0, torch.arange(4).expand(17, 4), ids=big, prefix_lens=[0] * 17)
    # the op: a prefix past a row's keys, a key count outside the new rows, a head dim the form does not have
    q = torch.zeros((1, 4, PC.NH, PC.HD), dtype=torch.bfloat16, device="cuda")
    kk = torch.zeros((1, 4, 1, PC.HD), dtype=torch.bfloat16, device="cuda")
    o = torch.empty_like(q)

    def op(pfx, klen=None, hd=PC.HD):
        p = torch.tensor([pfx], dtype=torch.int32)
        kl = None if klen is None else torch.tensor([klen], dtype=torch.int32)
        return eng.lib.pgmi_op_attention_prefix(eng.ctx, q.data_ptr(), kk.data_ptr(), kk.data_ptr(), o.data_ptr(), 1, 4,
                                                4, PC.NH, 1, hd, 0, 1.0 / 16.0, 0, None if kl is None else kl.data_ptr(),
                                                p.data_ptr(), eng._s())
    assert op(5) == N.PGMI_E_ARG and op(-1) == N.PGMI_E_ARG and op(3, klen=2) == N.PGMI_E_ARG
    assert op(0, klen=5) == N.PGMI_E_ARG and op(0, klen=0) == N.PGMI_E_ARG and op(0, hd=72) == N.PGMI_E_ARG
    assert op(2) == 0
    torch.cuda.synchronize()
