"""Token log-probabilities and the loss without the logits (modeling_gemma.py:596-603): the fused lm_head kernel
(EPI_LSE), the row kernel on existing logits, Engine.score / generate(return_logprobs) and the drop-in model's
pgmi_fused_loss, each held to pgmi/scoring.py's float64 rule.

The log-sum-exp tolerance is (d + 4) * 2^-23 * max(1, |lse|), d the longest chain of fp32 additions one term
exp(x - m) passes through on its way into the sum (everything after it is fp64):
  * fused kernel (csrc/kernels_gemm.hip, lse_wave / lse_merge): in-lane over a wave's TN <= 4 column tiles (3),
    four xor-shuffles over lane & 15 (4), the WN <= 4 waves of a row in LDS (3): d = 10; the column tiles are
    merged in fp64 (k_lse_combine).
  * row kernel (csrc/kernels_misc.hip, k_logprob_part): a thread's ceil(slice / 256) elements in index order
    (slice <= 2048 for rows * 8 <= 1024: 7), six xor-shuffles (6), the four waves (3): d = 16; the slices are
    merged in fp64 (k_logprob_finish).
Both stay far below the 2e-4 cap (2,010 sequential fp32 adds).

logprob is the fp32 difference logit[label] - lse of the ROUNDED lse, so the label's logit is recovered exactly
as the bf16 value nearest logprob + lse only when it is not tiny beside lse; the tests check the identity itself
instead, bit for bit: logprob == fp32(GEMM's logit[label]) - lse as one fp32 subtraction."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import paligemma_np as O
from oracle import weights as W
from pgmi.scoring import logprobs_np, logsumexp_np, loss_from_logprobs_np, shifted_loss_np

pytestmark = pytest.mark.gpu
SEED = 1234
IGN = -100
K = 2048
D_FUSED, D_ROWS = 10, 16
CAP = 2e-4


def lse_tol(d, lse):
    t = (d + 4) * 2.0 ** -23 * np.maximum(1.0, np.abs(lse))
    assert np.all(t <= CAP)
    return t


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.small_config(), max_batch=8, max_seq=320, max_kv=512)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    yield e
    del e
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def P():
    return W.synthetic_state_dict_f32(W.small_config(), SEED)


# ---------------------------------------------------------------- 1. the fused kernel against the GEMM it mirrors
_mats = {}


def _matrix(V):
    """W[V][K] (logits of std 3) and 300 normed rows, bf16, on the device; made once per V."""
    if V not in _mats:
        g = torch.Generator().manual_seed(V)
        Wt = (torch.randn((V, K), generator=g) * (3.0 / K ** 0.5)).to(torch.bfloat16).cuda()
        A = torch.randn((300, K), generator=g).to(torch.bfloat16).cuda()
        _mats[V] = (A, Wt)
    return _mats[V]


def _gemm_f32(eng, A, Wt):
    from pgmi import _native as N
    out = torch.empty((A.shape[0], Wt.shape[0]), dtype=torch.float32, device="cuda")
    N.check(eng.lib.pgmi_op_gemm(eng.ctx, A.data_ptr(), Wt.data_ptr(), A.shape[0], Wt.shape[0], A.shape[1], 6, None,
                                 None, out.data_ptr(), N.stream_handle()))
    return out


def _op_lm_logprobs(eng, A, Wt, labels):
    from pgmi import _native as N
    rows = A.shape[0]
    lb = torch.as_tensor(labels, dtype=torch.int64).cuda()
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda")
    lse = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda")
    N.check(eng.lib.pgmi_op_lm_logprobs(eng.ctx, A.data_ptr(), Wt.data_ptr(), rows, Wt.shape[0], A.shape[1],
                                        lb.data_ptr(), IGN, lp.data_ptr(), lse.data_ptr(), N.stream_handle()),
            "pgmi_op_lm_logprobs")
    torch.cuda.synchronize()
    return lp.cpu().numpy(), lse.cpu().numpy()


def _check_against_logits(G, labels, lp, lse, d):
    """lp / lse of one call against the logits G (rows, V) the GEMM wrote."""
    V = G.shape[1]
    labels = np.asarray(labels)
    ref = logsumexp_np(G)
    err = np.abs(lse.astype(np.float64) - ref)
    print("lse max err", float(err.max()), "tol", float(lse_tol(d, ref).min()))
    assert np.all(err <= lse_tol(d, ref)), (err.max(), lse_tol(d, ref).min())
    for r, l in enumerate(labels):
        if l == IGN:
            assert bits(lp[r]) == bits(0.0), (r, lp[r])
        elif l < 0 or l >= V:
            assert np.isnan(lp[r]), (r, lp[r])
        else:  # the label's logit is the GEMM's, bit for bit: one fp32 subtraction from the returned lse
            assert bits(lp[r]) == bits(np.float32(G[r, l]) - np.float32(lse[r])), (r, l, lp[r], G[r, l], lse[r])
    want = logprobs_np(G, labels, IGN)
    live = np.isfinite(want) & (labels != IGN)
    assert np.all(np.abs(lp[live] - want[live]) <= lse_tol(d, ref)[live] + 2.0 ** -23 * np.maximum(1, np.abs(want[live])))


def _special_labels(V):
    # column 0, the last column, both sides of the 64- and 128-column tile boundaries, ignored, one label >= V
    return [0, V - 1, 63, 64, 127, 128, IGN, V, V - 2, 65, 129, -1]


@pytest.mark.parametrize("V", [1000, 16384])
@pytest.mark.parametrize("rows", [1, 5, 16, 17, 130])
def test_fused_kernel_matches_gemm(eng, rows, V):
    from pgmi import _native as N
    A, Wt = _matrix(V)
    A = A[:rows].contiguous()
    G = _gemm_f32(eng, A, Wt).cpu().numpy()
    sp = _special_labels(V)
    rng = np.random.default_rng(rows + V)
    first = None
    for off in range(0, len(sp), rows):   # every special label is used at every row count
        labels = [sp[(off + r) % len(sp)] if r < len(sp) else int(rng.integers(0, V)) for r in range(rows)]
        lp, lse = _op_lm_logprobs(eng, A, Wt, labels)
        _check_against_logits(G, labels, lp, lse, D_FUSED)
        first = first or (labels, lp, lse)
    labels, lp, lse = first
    lp2, lse2 = _op_lm_logprobs(eng, A, Wt, labels)          # a second call: the same bits
    assert np.array_equal(bits(lp), bits(lp2)) and np.array_equal(bits(lse), bits(lse2))
    # the shape's own configuration with a forced K split: this epilogue never splits
    cfg, bm, bn, split = (ctypes.c_int() for _ in range(4))
    assert eng.lib.pgmi_debug_gemm_plan(rows, V, K, 0, ctypes.byref(cfg), ctypes.byref(bm), ctypes.byref(bn),
                                        ctypes.byref(split)) == 0
    assert split.value == 1   # the GEMM above ran unsplit: its logits are the ones the epilogue reduces
    try:
        assert eng.lib.pgmi_tune_gemm(cfg.value, 4) == 0
        lp3, lse3 = _op_lm_logprobs(eng, A, Wt, labels)
        if rows == 17:        # a forced configuration without this epilogue (the 8-phase E256) is refused
            assert eng.lib.pgmi_tune_gemm(36, 1) == 0
            with pytest.raises(ValueError):
                _op_lm_logprobs(eng, A, Wt, labels)
    finally:
        assert eng.lib.pgmi_tune_gemm(-1, 0) == 0
    assert np.array_equal(bits(lp), bits(lp3)) and np.array_equal(bits(lse), bits(lse3))
    if rows == 5 and V == 1000:   # the tied-embedding entry and its wrapper: same kernel on the engine's E
        E = eng.views["language_model.model.embed_tokens.weight"]
        An = torch.randn((5, K), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
        lb = torch.tensor([0, E.shape[0] - 1, IGN, E.shape[0], 77])
        lp_e, lse_e = eng.lm_logprobs(An, lb, return_lse=True)
        torch.cuda.synchronize()
        _check_against_logits(eng.lm_head(An).cpu().numpy(), lb.numpy(), lp_e.cpu().numpy(), lse_e.cpu().numpy(),
                              D_FUSED)


# every configuration with an EPI_LSE instance (csrc/kernels_gemm.hip lse_has): id -> (name, BM, BN, waves per row)
LSE_CFGS = {11: ("P128w", 128, 128, 2), 14: ("P64x64", 64, 64, 2), 22: ("Q256w", 256, 128, 4),
            31: ("W288n", 288, 64, 4), 32: ("W64x64", 64, 64, 2), 34: ("W128x128", 128, 128, 4)}


@pytest.mark.parametrize("cfg", sorted(LSE_CFGS))
def test_fused_kernel_every_instance(eng, cfg):
    """Each of the six instances forced (pgmi_tune_gemm(id, 1)), against pgmi_op_gemm(epi 6) under the same forced
    configuration: both kernel families, the loader waves' share of the epilogue (k_gemm_w), two and four waves
    per row in the LDS merge, one to four column tiles per wave.  rows 17 and 130 leave a row-tile tail in every
    BM; 300 gives BM 256 and 288 a full tile plus a tail.  V = 1000 leaves a column tail in every BN."""
    name, BM, BN, _ = LSE_CFGS[cfg]
    plan = [ctypes.c_int() for _ in range(4)]
    try:
        assert eng.lib.pgmi_tune_gemm(cfg, 1) == 0
        assert eng.lib.pgmi_debug_gemm_plan(300, 1000, K, 0, *[ctypes.byref(p) for p in plan]) == 0
        assert [p.value for p in plan] == [cfg, BM, BN, 1], name
        for V in (1000, 16384):
            A300, Wt = _matrix(V)
            sp = _special_labels(V)
            for rows in (17, 130, 300):
                A = A300[:rows].contiguous()
                G = _gemm_f32(eng, A, Wt).cpu().numpy()
                rng = np.random.default_rng(rows + V + cfg)
                labels = [sp[r] if r < len(sp) else int(rng.integers(0, V)) for r in range(rows)]
                labels[-1] = V - 1            # the last row of the row-tile tail, the last column of the column tail
                lp, lse = _op_lm_logprobs(eng, A, Wt, labels)
                _check_against_logits(G, labels, lp, lse, D_FUSED)
                lp2, lse2 = _op_lm_logprobs(eng, A, Wt, labels)
                assert np.array_equal(bits(lp), bits(lp2)) and np.array_equal(bits(lse), bits(lse2)), (name, rows, V)
    finally:
        assert eng.lib.pgmi_tune_gemm(-1, 0) == 0


@pytest.mark.slow
@pytest.mark.parametrize("rows", [16, 288])
def test_fused_kernel_production_vocab(eng, rows):
    """V = 257216 = 2009 * 128 + 64: the production vocabulary, whose last column tile is half empty."""
    V = 257216
    g = torch.Generator(device="cuda").manual_seed(rows)
    Wt = (torch.randn((V, K), generator=g, device="cuda") * (3.0 / K ** 0.5)).to(torch.bfloat16)
    A = torch.randn((rows, K), generator=g, device="cuda").to(torch.bfloat16)
    G = _gemm_f32(eng, A, Wt).cpu().numpy()
    sp = [0, V - 1, 63, 64, 127, 128, IGN, V, V - 64, V - 65, 257151, 257152]
    rng = np.random.default_rng(rows)
    labels = [sp[r] if r < len(sp) else int(rng.integers(0, V)) for r in range(rows)]
    lp, lse = _op_lm_logprobs(eng, A, Wt, labels)
    _check_against_logits(G, labels, lp, lse, D_FUSED)
    lp2, lse2 = _op_lm_logprobs(eng, A, Wt, labels)
    assert np.array_equal(bits(lp), bits(lp2)) and np.array_equal(bits(lse), bits(lse2))


# ---------------------------------------------------------------- 2. the row kernel
@pytest.mark.parametrize("V", [1000, 16384])
@pytest.mark.parametrize("rows", [1, 3, 16])
def test_row_kernel(eng, rows, V):
    rng = np.random.default_rng(rows * 3 + V)
    x = (rng.standard_normal((rows, V)) * 4).astype(np.float32)
    ids = rng.integers(0, V, rows)
    ids[0] = V - 1
    if rows >= 3:
        ids[1], ids[2] = IGN, V
    if rows == 16:
        x[4, ::3] = -np.inf          # a row with -inf entries (a live id among the finite ones)
        ids[4] = 1
        x[5, :] = np.float32(2.5)    # a constant row: lse = 2.5 + log V
        ids[6] = 0
    lp, lse = eng.logprobs(torch.from_numpy(x).cuda(), torch.from_numpy(ids).cuda(), return_lse=True)
    torch.cuda.synchronize()
    lp, lse = lp.cpu().numpy(), lse.cpu().numpy()
    _check_against_logits(x, ids, lp, lse, D_ROWS)
    if rows == 16:
        assert abs(float(lse[5]) - (2.5 + np.log(V))) <= lse_tol(D_ROWS, lse[5])
    lp2, lse2 = eng.logprobs(torch.from_numpy(x).cuda(), torch.from_numpy(ids).cuda(), return_lse=True)
    assert np.array_equal(bits(lp), bits(lp2.cpu().numpy())) and np.array_equal(bits(lse), bits(lse2.cpu().numpy()))


# ---------------------------------------------------------------- 3. Engine.score against the oracle
LENS = [2, 33, 64, 65, 97]       # 1 + 1: the shortest row with a scored position


def text_rows(lens, seed):
    """Random text prompts as tests/test_gpu_batch16.py builds them (ids in [3, vocab - 1), ids[:, 0] = 2)."""
    cfg = W.small_config()
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, cfg["text_config"]["vocab_size"] - 1, size=(len(lens), max(lens))).astype(np.int64)
    ids[:, 0] = 2
    assert not (ids == cfg["image_token_index"]).any()
    return [ids[b, :n].copy() for b, n in enumerate(lens)]


def row_labels(rows, seed):
    """Per row: random labels, the first quarter of the row and every seventh position ignored; the last label
    always live (the 2-token row's only scored position)."""
    rng = np.random.default_rng(seed)
    V = W.small_config()["text_config"]["vocab_size"]
    out = []
    for r in rows:
        lb = rng.integers(0, V, len(r)).astype(np.int64)
        lb[:len(r) // 4] = IGN
        lb[::7] = IGN
        lb[-1] = int(rng.integers(0, V))
        out.append(lb)
    return out


def oracle_logprobs(P, ids_row, labels_row, pixels=None):
    """The oracle (bf16) and its fp32 truth on one row alone, all logits -> shifted per-token log-probabilities."""
    cfg = W.small_config()
    ids = ids_row[None]
    sl = labels_row[None, 1:]
    if pixels is None:
        Pt = {n: v for n, v in P.items() if n.startswith("language_model")}
        emb = O.merge(Pt, cfg, None, ids)
        pos = np.arange(ids.shape[1])[None]
        ref = O.gemma_forward(Pt, cfg, emb, pos, O.KV(), all_logits=True)
        with O.fp32_truth():
            tru = O.gemma_forward(Pt, cfg, emb, pos, O.KV(), all_logits=True)
    else:
        ref, _ = O.paligemma_prefill(P, cfg, ids, pixels, all_logits=True)
        with O.fp32_truth():
            tru, _ = O.paligemma_prefill(P, cfg, ids, pixels, all_logits=True)
    return logprobs_np(ref[:, :-1], sl, IGN)[0], logprobs_np(tru[:, :-1], sl, IGN)[0]


def pad2(rows, pad):
    out = np.full((len(rows), max(len(r) for r in rows)), pad, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


@pytest.fixture(scope="module")
def scored(P):
    """The five ragged rows and two rows of 33, their labels and each row's oracle log-probabilities (once)."""
    rows = text_rows(LENS + [33, 33], 11)
    labels = row_labels(rows, 12)
    return rows, labels, [oracle_logprobs(P, r, l) for r, l in zip(rows, labels)]


def _floor_rule(label, ours, refs, labels):
    """SURVEY sec.8c's rule on log-probabilities: our mean |logprob - truth| over the live tokens <= 1.5 x the
    oracle bf16's own; both measured here."""
    eo, er = [], []
    for b, (ref, tru) in enumerate(refs):
        live = labels[b][1:] != IGN
        n = len(ref)
        eo.append(np.abs(ours[b][:n][live] - tru[live]))
        er.append(np.abs(ref[live] - tru[live]))
    eo, er = np.concatenate(eo), np.concatenate(er)
    print(f"score-parity {label}: ours vs truth {eo.mean():.4e}, oracle bf16 vs truth {er.mean():.4e}, n = {len(eo)}")
    assert eo.mean() <= 1.5 * er.mean(), (label, eo.mean(), er.mean())


def _check_score(sc, labels_padded):
    """labels_padded: IGN under the pad positions.  loss against the float64 rule on our own per-token values."""
    lp = sc.logprobs.cpu().numpy()
    sl = labels_padded[:, 1:]
    live = sl != IGN
    want = loss_from_logprobs_np(lp, sl, IGN)
    assert abs(float(sc.loss) - want) <= 1e-6 * abs(want), (float(sc.loss), want)
    assert np.all(lp[~live] == 0) and np.all(lp[live] < 0)
    assert np.array_equal(sc.counts.cpu().numpy(), live.sum(1))
    np.testing.assert_allclose(sc.sums.cpu().numpy(), lp.sum(1), rtol=1e-5)
    return lp


def test_score_lock_step(eng, scored):
    rows, labels, refs = scored
    ids, lab = pad2(rows[5:], 0), pad2(labels[5:], IGN)
    sc = eng.score(torch.from_numpy(ids), None, torch.from_numpy(lab))
    lp = _check_score(sc, lab)
    assert lp.shape == (2, 32) and np.all(lp[lab[:, 1:] == IGN] == 0)
    _floor_rule("lock-step 2 x 33", lp, refs[5:], labels[5:])


def test_score_ragged(eng, scored):
    rows, labels, refs = scored
    rows, labels, refs = rows[:5], labels[:5], refs[:5]
    ids, lab = pad2(rows, 0), pad2(labels, IGN)
    mask = (np.arange(ids.shape[1])[None] < np.array(LENS)[:, None]).astype(np.int64)
    sc = eng.score(torch.from_numpy(ids), None, torch.from_numpy(lab), attention_mask=torch.from_numpy(mask))
    lp = _check_score(sc, lab)
    assert lp.shape == (5, 96)
    assert np.array_equal(sc.counts.cpu().numpy(), [(l[1:] != IGN).sum() for l in labels])
    _floor_rule("ragged " + str(LENS), lp, refs, labels)
    # labels under the pad positions, and further positions ignored, change no live value (bit for bit).  The
    # reduction order is the GEMM configuration's: both calls keep more than 64 live rows, the one regime this
    # vocabulary's plans have above it (the production vocabulary has a single plan for every row count)
    V = eng.cfgd["t_vocab"]
    lab2 = lab.copy()
    lab2[mask == 0] = np.random.default_rng(1).integers(0, V, int((mask == 0).sum()))
    more = np.zeros_like(lab2, dtype=bool)
    more[:, 40:60] = True
    lab2[more & (mask == 1)] = IGN
    sc2 = eng.score(torch.from_numpy(ids), None, torch.from_numpy(lab2), attention_mask=torch.from_numpy(mask))
    lp2 = sc2.logprobs.cpu().numpy()
    still = (lab2[:, 1:] != IGN) & (mask[:, 1:] == 1)
    assert still.sum() > 64 and still.sum() < (lp != 0).sum()
    assert np.array_equal(bits(lp2[still]), bits(lp[still])) and np.all(lp2[~still] == 0)
    # a left-padded mask scores the same tokens (returned in the right-padded layout)
    L = ids.shape[1]
    idl, lbl, ml = np.zeros_like(ids), np.full_like(lab, IGN), np.zeros_like(mask)
    for b, n in enumerate(LENS):
        idl[b, L - n:], lbl[b, L - n:], ml[b, L - n:] = ids[b, :n], lab[b, :n], 1
    sc3 = eng.score(torch.from_numpy(idl), None, torch.from_numpy(lbl), attention_mask=torch.from_numpy(ml))
    assert np.array_equal(bits(sc3.logprobs.cpu().numpy()), bits(lp))
    # nothing live: NaN, as torch gives
    sc4 = eng.score(torch.from_numpy(ids), None, torch.full_like(torch.from_numpy(lab), IGN),
                    attention_mask=torch.from_numpy(mask))
    assert np.isnan(float(sc4.loss)) and not sc4.logprobs.any() and not sc4.counts.any()


def test_score_image_prompt(eng, P, golden_dir):
    gold = np.load(os.path.join(golden_dir, "small_bf16.npz"))
    ids, px = gold["ids"].astype(np.int64), O.from_bits(gold["pixels_bits"])
    L = ids.shape[1]
    assert L <= 320 and (ids == W.small_config()["image_token_index"]).any()
    rng = np.random.default_rng(3)
    lab = np.full((1, L), IGN, dtype=np.int64)   # the image and most of the prompt masked: the last 8 labels live
    lab[0, -8:] = rng.integers(0, eng.cfgd["t_vocab"], 8)
    ref = oracle_logprobs(P, ids[0], lab[0], pixels=px)
    sc = eng.score(torch.from_numpy(ids), torch.from_numpy(px).cuda(), torch.from_numpy(lab))
    lp = _check_score(sc, lab)
    assert int(sc.counts[0]) == 8
    _floor_rule("image prompt", lp, [ref], [lab[0]])


def test_score_vs_reference_loss(eng, golden_dir):
    """tests/golden/small_loss.npz (make_golden_loss.py): the reference model's own forward(labels=...) in bf16 and
    fp32 on this configuration; Engine.score is held to it under the same 1.5 x rule, and its loss likewise."""
    g = np.load(os.path.join(golden_dir, "small_loss.npz"))
    gold = np.load(os.path.join(golden_dir, "small_bf16.npz"))
    assert np.array_equal(g["ids"], gold["ids"])
    px = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    sc = eng.score(torch.from_numpy(g["ids"]), px, torch.from_numpy(g["labels"]))
    lp = _check_score(sc, g["labels"])
    _floor_rule("reference loss", lp, [(g["logprobs_bf16"][0], g["logprobs_fp32"][0])], [g["labels"][0]])
    e_ours, e_ref = abs(float(sc.loss) - float(g["loss_fp32"])), abs(float(g["loss_bf16"]) - float(g["loss_fp32"]))
    print(f"loss: ours {float(sc.loss):.6f}, reference bf16 {float(g['loss_bf16']):.6f}, fp32 {float(g['loss_fp32']):.6f}")
    # the loss is a mean of 30 signed errors, so the reference's own |loss error| can land near zero by
    # cancellation: the bound is 1.5 x its mean per-token error (what _floor_rule measures), which bounds both
    live = g["labels"][0, 1:] != IGN
    per_tok = float(np.abs(g["logprobs_bf16"][0][live] - g["logprobs_fp32"][0][live]).mean())
    assert e_ours <= 1.5 * max(e_ref, per_tok), (e_ours, e_ref, per_tok)


# ---------------------------------------------------------------- 4. only live rows are multiplied
def test_score_multiplies_live_rows_only(eng, scored):
    rows, labels, _ = scored
    ids = torch.from_numpy(rows[4][None]).cuda()                  # the 97-token row
    full = labels[4].copy()
    full[1:] = np.where(full[1:] == IGN, 5, full[1:])             # all 96 positions live
    last4 = np.full_like(full, IGN)
    last4[-4:] = full[-4:]
    V = eng.cfgd["t_vocab"]
    all_rows = eng.score(ids, None, torch.from_numpy(full[None]).cuda()).logprobs.cpu().numpy()
    lab = torch.from_numpy(last4[None]).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sc = eng.score(ids, None, lab)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("score memory growth", growth, "bytes; one (97, V) fp32 tensor:", 97 * V * 4)
    assert growth < 97 * V * 4
    lp = sc.logprobs.cpu().numpy()
    assert int(sc.counts[0]) == 4 and not lp[0, :-4].any()
    # 4 rows and 96 rows take different tile configurations: each within test 1's tolerance of the float64 value
    # of the same logits, so within twice that of each other -- not bit for bit
    lg = eng.lm_forward(eng.new_kv(1, 128), 0, torch.arange(97)[None], ids=ids, logits_rows=0)[0, -5:-1]
    tol = 2 * lse_tol(D_FUSED, logsumexp_np(lg.cpu().numpy())) + 2.0 ** -23 * np.maximum(1, np.abs(lp[0, -4:]))
    assert np.all(np.abs(lp[0, -4:] - all_rows[0, -4:]) <= tol), (lp[0, -4:], all_rows[0, -4:])


# ---------------------------------------------------------------- 5. the drop-in model
@torch.no_grad()
def test_dropin_fused_loss(scored):
    import modeling_gemma as MG
    import utils as U
    from pgmi.lazy_logits import LazyLogits
    cfg = W.small_config()
    pcfg = MG.PaliGemmaConfig(**{k: v for k, v in cfg.items() if k not in ("bos_token_id", "eos_token_id")})
    m = U.build_model(pcfg, device="cuda")
    m.tie_weights()
    e = m._pgmi_engine()
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    m.eval()
    rows, labels, _ = scored
    ids = torch.from_numpy(pad2(rows[5:], 0)).cuda()
    lab = torch.from_numpy(pad2(labels[5:], IGN)).cuda()
    assert pcfg.ignore_index == IGN
    try:
        off = m(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab)
        full = off["logits"].materialize()
        # flag off: torch's loss on the materialised tensor, exactly
        want = torch.nn.CrossEntropyLoss(ignore_index=IGN)(full[:, :-1].reshape(-1, full.shape[-1]),
                                                           lab[:, 1:].reshape(-1))
        assert torch.equal(off["loss"], want)
        m.pgmi_fused_loss = True
        on = m(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab)
        assert isinstance(on["logits"], LazyLogits) and not on["logits"].is_materialized
        # the fused loss is held to the float64 loss of the logits it reduces: pgmi_lm_head on the same live hidden
        # rows, a GEMM whose plan is asserted unsplit (the materialised tensor's 66-row GEMM may split K at this
        # vocabulary, and a label logit one bf16 step away would pass the bound only by luck).  The bound is the
        # kernel's log-sum-exp tolerance plus the fp32 rounding of each log-probability: test 1's, through a mean
        sl = lab[:, 1:]
        at = (sl != IGN).nonzero()
        Lm = ids.shape[1]
        live_rows = e.final_hidden(ids.shape[0] * Lm).index_select(0, at[:, 0] * Lm + at[:, 1])
        plan = [ctypes.c_int() for _ in range(4)]
        assert e.lib.pgmi_debug_gemm_plan(live_rows.shape[0], full.shape[-1], K, 0, *[ctypes.byref(q) for q in plan]) == 0
        assert plan[3].value == 1, [q.value for q in plan]
        live_logits = e.lm_head(live_rows).cpu().numpy()
        live_labels = sl[at[:, 0], at[:, 1]].cpu().numpy()
        truth = loss_from_logprobs_np(logprobs_np(live_logits, live_labels, IGN), live_labels, IGN)
        print("float64 loss of the materialised tensor:", shifted_loss_np(full.cpu().numpy(), lab.cpu().numpy(), IGN))
        lse_max = float(np.abs(logsumexp_np(live_logits)).max())
        bound = float(lse_tol(D_FUSED, lse_max)) + 2.0 ** -23 * max(1.0, abs(truth))
        print("fused loss", float(on["loss"]), "torch", float(off["loss"]), "float64", truth, "bound", bound)
        assert abs(float(on["loss"]) - truth) <= bound
        # "all" returns a plain tensor: the torch path runs whatever the switch says
        m.pgmi_prefill_logits = "all"
        allr = m(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab)
        assert isinstance(allr["logits"], torch.Tensor)
        assert torch.equal(allr["loss"], off["loss"])   # the last row, the only one that differs, is never scored
    finally:
        del m, e
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 6. generate(return_logprobs=True)
@torch.no_grad()
def test_generate_logprobs(eng, golden_dir):
    gold = np.load(os.path.join(golden_dir, "small_bf16.npz"))
    px0 = torch.from_numpy(O.from_bits(gold["pixels_bits"])).cuda()
    B, n = 3, 5
    px = torch.stack([px0[0], px0[0].flip(-1), px0[0].flip(-2)]).contiguous()
    ids = torch.from_numpy(gold["ids"].astype(np.int64)).cuda().expand(B, -1).contiguous()
    L = ids.shape[1]
    toks = eng.generate(ids, px, n)
    toks_l, lps = eng.generate(ids, px, n, return_logprobs=True)
    assert torch.equal(toks, toks_l) and lps.shape == (B, n) and lps.dtype == torch.float32
    # each value against the step's own logits: the same prefill (last row on the decode kernels) and decode
    # steps, teacher-forced on the emitted tokens
    kv = eng.new_kv(B, L + n + 1)
    feats = eng.project(eng.vision(px))
    lg = eng.lm_forward(kv, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=2)[:, 0]
    hist = [lg.cpu().numpy()]
    for t in range(1, n):
        hist.append(eng.decode(toks[:, t - 1].contiguous(), kv, L + t - 1, L + t, graph=True).cpu().numpy())
    got = lps.cpu().numpy()
    tk = toks.cpu().numpy()
    for t in range(n):
        want = logprobs_np(hist[t], tk[:, t], IGN)
        tol = lse_tol(D_ROWS, logsumexp_np(hist[t])) + 2.0 ** -23 * np.maximum(1, np.abs(want))
        assert np.all(np.abs(got[:, t] - want) <= tol), (t, got[:, t], want)
    assert np.all(got < 0)
    # with a stop token: the same tokens, and 0 after a row's eos (row 0 stops at its second token)
    eos = int(tk[0, 1])
    te, le = eng.generate(ids, px, n, eos_token_id=eos, return_lengths=True)
    te2, le2, lpe = eng.generate(ids, px, n, eos_token_id=eos, return_lengths=True, return_logprobs=True)
    assert torch.equal(te, te2) and torch.equal(le, le2) and lpe.shape == te.shape
    lpe, le = lpe.cpu().numpy(), le.cpu().numpy()
    assert le[0] == 2 or tk[0, 0] == eos
    for b in range(B):
        assert np.array_equal(bits(lpe[b, :le[b]]), bits(got[b, :le[b]])) and not lpe[b, le[b]:].any()
    # sampling under a fixed generator: the same tokens; the values are those of the raw logits (no temperature)
    gen = torch.Generator(device="cuda")
    ts = eng.generate(ids, px, n, do_sample=True, generator=gen.manual_seed(7))
    ts2, lpsamp = eng.generate(ids, px, n, do_sample=True, generator=gen.manual_seed(7), return_logprobs=True)
    assert torch.equal(ts, ts2)
    # every step, teacher-forced on the sampled tokens: sample_top_p reads the step's logits just before
    # Engine.logprobs does, and must leave them as they were
    kv2 = eng.new_kv(B, L + n + 1)
    hs = [eng.lm_forward(kv2, 0, torch.arange(L).expand(B, L), ids=ids, image_feats=feats, logits_rows=2)[:, 0]
          .cpu().numpy()]
    for t in range(1, n):
        hs.append(eng.decode(ts[:, t - 1].contiguous(), kv2, L + t - 1, L + t, graph=True).cpu().numpy())
    gs, tsn = lpsamp.cpu().numpy(), ts.cpu().numpy()
    for t in range(n):
        want = logprobs_np(hs[t], tsn[:, t], IGN)
        tol = lse_tol(D_ROWS, logsumexp_np(hs[t])) + 2.0 ** -23 * np.maximum(1, np.abs(want))
        assert np.all(np.abs(gs[:, t] - want) <= tol), (t, gs[:, t], want)
