"""The prefill-stage references (oracle/prefill_stage_ref.py), no GPU.

1. Chained over the layers, ref_stage0..6 equal the oracle the rest of the suite trusts (O.merge + O.gemma_forward,
   each sequence run alone on its real tokens) bit for bit in logits (every row, and the last row) and K/V rows, on
   the cases of tests/prefill_stage_cases.py: the ragged rows and the kv_start > 0 continuation included.
2. On every case and compared tensor of tests/test_gpu_prefill_stages.py the reference alone stays inside the caps
   the decode suite fixed (decode_stage_cases.CAP_REL = 2^-7, CAP_D = 0.05), and its GEMM epilogues keep their signed
   mean error within BIAS_SE standard errors.  One input was changed for a cap: the dominant last key of stage 2 is
   planted by lowering every other key's score in head 0, not by raising its own (prefill_stage_cases.attn_inputs:
   with its own score at 4 .. 8 the reference alone reached rel-L2 7.9e-3 .. 8.7e-3 at cases A and G), and by
   enough that its weight rounds to 1.0 (the same docstring says why).
3. Seven faults injected into the reference on the CPU are each rejected by the conditions the GPU file applies to
   that tensor: bf16 truncation (stages 1, 3, 4, 5), a RoPE position off by one, a dropped split-K slab (3, 5), a
   row attending one key too few, K/V rows one slot late, image row k + 1 at the k-th <image> token, a ragged
   row's logits taken at L - 1.  No condition had to be added.

Measured reference distances, worst row over the cases (R against T; d = max |x - t| / (|t| + rms t); `pytest -s`
prints every case's):

    tensor                                        rel_l2(R, T)        d(R)
    stage 0 hs, from ids / from given rows        1.6e-3 .. 2.0e-3    1.9e-3 .. 4.1e-3   (G must equal R bit for bit)
    stage 0 tn (layer 0's input norm)             2.2e-3 .. 2.6e-3    3.8e-3 .. 6.0e-3
    stage 1 q                                     1.7e-3 .. 3.0e-3    2.4e-3 .. 1.4e-2   (least: case B, position 0)
    stage 1 k                                     1.6e-3 .. 3.4e-3    2.1e-3 .. 9.8e-3
    stage 1 v                                     1.7e-3 .. 2.0e-3    2.3e-3 .. 3.0e-3
    stage 2 ao                                    0 (one key) .. 5.5e-3   0 .. 2.8e-2
    stage 3 hs / tn                               2.4e-3 .. 2.5e-3 / 2.9e-3 .. 3.1e-3     4.7e-3 .. 5.4e-3 / 5.2e-3 .. 6.9e-3
    stage 4 act                                   3.5e-3 .. 3.7e-3    8.5e-3 .. 1.1e-2
    stage 5 hs / tn, layer 0 and 1                2.3e-3 .. 2.4e-3 / 2.8e-3 .. 3.0e-3     3.8e-3 .. 6.0e-3 / 4.8e-3 .. 6.9e-3
    stage 6 logits, every row / last rows         1.6e-3 .. 1.8e-3 / 2.3e-3 .. 2.4e-3     2.4e-3 .. 2.9e-3 / 4.3e-3 .. 5.4e-3
    stage 7 ao / lastrows / its logits            up to 4.7e-3 / 6.6e-3 / 7.4e-3          up to 2.0e-2 / 1.9e-2 / 2.3e-2
"""
import numpy as np
import pytest

import prefill_stage_cases as C
from oracle import paligemma_np as O
from oracle import prefill_stage_ref as R


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _inside(name, Rr, T, bias=True):
    Rr, T = C.rows2(Rr), C.rows2(T)
    rel, d = C.reference_distances(name, Rr, T)
    print(f"{name:40s} rel_l2(R, T) {rel:.3e}  d(R) {d:.3e}")
    assert rel <= C.CAP_REL and d <= C.CAP_D, (name, rel, d)
    if bias:   # (not attention outputs: one rounded probability moves all 256 elements of a head together)
        b, se = R.bias_rows(Rr, T)
        assert (np.abs(b) <= C.BIAS_SE * se).all(), (name, b, se)


def _live(x):
    return np.abs(C.rows2(x)).sum(-1) > 0


# ---------------------------------------------------------------- 1. the chain is the oracle
def _oracle_row(P, cfg, emb, pos, prior, b, n, all_logits):
    """O.gemma_forward for batch row b alone on its n real tokens, its cache holding the prior rows."""
    kv = O.KV()
    if prior is not None:
        for i in range(R.dims(cfg)["L"]):
            kv.update(prior[i, 0, b][None, None].copy(), prior[i, 1, b][None, None].copy(), i)
    lg = O.gemma_forward(P, cfg, emb[b:b + 1, :n], pos[b:b + 1, :n], kv, all_logits=all_logits)
    return lg[0], [k[0, 0] for k in kv.k], [v[0, 0] for v in kv.v]


@pytest.mark.parametrize("name", ("A",) + C.CHAIN_CASES)
def test_chained_references_equal_the_oracle(name):
    cfg, P = C.model()
    c = C.CASES[name]
    ids, feats = C.ids_feats(name)
    emb = O.merge(P, cfg, feats[None], R.merged_ids(cfg, ids, c.lens))
    prior = C.prior_kv(name)
    for logits_rows in ((0,) if name == "A" else (0, 1)):
        kv = prior.copy()
        lg = R.ref_prefill(P, cfg, kv, c.kv_start, c.pos, ids=ids, feats=feats, lens=c.lens, logits_rows=logits_rows)
        for b, n in enumerate(C.real(name)):
            want, Ks, Vs = _oracle_row(P, cfg, emb, c.pos, prior[:, :, :, :c.kv_start] if c.kv_start else None, b, n,
                                       logits_rows == 0)
            got = lg[b, :n] if logits_rows == 0 else lg[b]
            assert np.array_equal(_bits(got), _bits(want)), (name, logits_rows, b)
            for i in range(R.dims(cfg)["L"]):
                assert np.array_equal(_bits(kv[i, 0, b, :c.kv_start + n]), _bits(Ks[i])), (name, b, i)
                assert np.array_equal(_bits(kv[i, 1, b, :c.kv_start + n]), _bits(Vs[i])), (name, b, i)
            assert np.isfinite(kv[:, :, b]).all()       # every slot of the row is written, pad slots included


def test_lock_step_batch_equals_the_batched_oracle():
    """Case F as one (9, 8) call of the oracle: the rows do not depend on the batch they came in."""
    cfg, P = C.model()
    c = C.CASES["F"]
    ids, feats = C.ids_feats("F")
    kv = C.prior_kv("F").copy()
    lg = R.ref_prefill(P, cfg, kv, 0, c.pos, ids=ids, feats=feats)
    okv = O.KV()
    want = O.gemma_forward(P, cfg, O.merge(P, cfg, feats[None], ids), c.pos, okv)
    assert np.array_equal(_bits(lg), _bits(want))
    for i in range(2):
        assert np.array_equal(_bits(kv[i, 0, :, :c.L]), _bits(okv.k[i][:, 0]))
        assert np.array_equal(_bits(kv[i, 1, :, :c.L]), _bits(okv.v[i][:, 0]))


def test_merge_pad_slots_and_image_order():
    cfg, P = C.model()
    ids, feats = C.ids_feats("E")
    (hs, _), _ = C.stage0_ref("E")
    lens = C.CASES["E"].lens
    for b, n in enumerate(lens):
        assert not hs[b, n:].any()                       # pad slots are zero rows whatever id they hold
    # rows 1 and 2 open with 2 and 3 <image> tokens (row 0 has one real token, no image): image rows 0 .. 4 in order
    sc = O.bf16(O.bf16(feats / np.float32(cfg["hidden_size"] ** 0.5)) * R.normalizer(cfg))
    assert np.array_equal(hs[1, :2], sc[0:2]) and np.array_equal(hs[2, :3], sc[2:5])


# ---------------------------------------------------------------- 2. the reference inside its caps, case by case
@pytest.mark.parametrize("name", C.STAGE_CASES)
def test_stage0(name):
    (Rh, Rn), (Th, Tn) = C.stage0_ref(name)
    live = _live(Rh)
    assert np.array_equal(live, _live(Th))
    _inside(f"stage0 {name} hs", C.rows2(Rh)[live], C.rows2(Th)[live], bias=False)
    _inside(f"stage0 {name} tn", C.rows2(Rn)[live], C.rows2(Tn)[live], bias=False)
    assert not C.rows2(Rn)[~live].any() and not C.rows2(Tn)[~live].any()
    if C.CASES[name].lens is None:
        (Rh, Rn), (Th, Tn) = C.stage0_ref(name, embeds=True)
        _inside(f"stage0 {name} embeds hs", Rh, Th, bias=False)
        _inside(f"stage0 {name} embeds tn", Rn, Tn, bias=False)


@pytest.mark.parametrize("name", C.STAGE_CASES + ("G", "Dmax"))
def test_stage1(name):
    Rr, T = C.stage1_ref(name)
    for nm, r, t in zip("qkv", Rr, T):
        _inside(f"stage1 {name} {nm}", r, t)


@pytest.mark.parametrize("name", C.STAGE_CASES + ("G",))
def test_stage2(name):
    Rr, T = C.stage2_ref(name)
    _inside(f"stage2 {name} ao", Rr, T, bias=False)


@pytest.mark.parametrize("name", C.STAGE_CASES)
def test_stage3_4_5_6(name):
    (Rh, Rn), (Th, Tn) = C.stage3_ref(name)
    _inside(f"stage3 {name} hs", Rh, Th)
    _inside(f"stage3 {name} tn", Rn, Tn, bias=False)
    _inside(f"stage4 {name} act", *C.stage4_ref(name))
    for layer in ((0,) if name == "A" else (0, 1)):
        (Rh, Rn), (Th, Tn) = C.stage5_ref(name, layer)
        _inside(f"stage5 {name} layer {layer} hs", Rh, Th)
        _inside(f"stage5 {name} layer {layer} tn", Rn, Tn, bias=False)
    for logits_rows in (0, 1):
        (Rl, _), (Tl, _) = C.stage6_ref(name, logits_rows)
        _inside(f"stage6 {name} logits_rows {logits_rows}", Rl, Tl)


@pytest.mark.parametrize("name", C.TAIL_CASES)
def test_stage7(name):
    (Rl, Ra, Rg), (Tl, Ta, Tg) = C.stage7_ref(name)
    _inside(f"stage7 {name} lastrows", Rl, Tl, bias=False)
    _inside(f"stage7 {name} ao", Ra, Ta, bias=False)
    _inside(f"stage7 {name} logits", Rg, Tg, bias=False)


# ---------------------------------------------------------------- 3. the conditions reject the seven mutants
def _trunc(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _caught(name, G, Rr, T, **kw):
    with pytest.raises(AssertionError):
        C.check(name, G, Rr, T, **kw)


def _w(layer, what):
    return C.model()[1][f"language_model.model.layers.{layer}.{what}.weight"]


def test_mutant_i_truncation():
    cfg, P = C.model()
    name = "C"
    # stage 1: v truncated after the projection, k after the rotary sum
    layer = C.LAYER[1]
    (Rq, Rk, Rv), (Tq, Tk, Tv) = C.stage1_ref(name)
    tn = C.rows(name, "tn")
    C.check("the reference itself", Rv, Rv, Tv)
    _caught("v truncates", _trunc(tn @ _w(layer, "self_attn.v_proj").T), Rv, Tv)
    k = O.linear(tn, _w(layer, "self_attn.k_proj"))
    cos, sin = R.rope_rows(cfg, C.CASES[name].pos)
    cos, sin = cos.reshape(1, -1, C.KD), sin.reshape(1, -1, C.KD)
    _caught("k's rotary sum truncates", _trunc(O.bf16(k * cos) + O.bf16(O.rotate_half(k) * sin)), Rk, Tk)
    # stage 3 / 5: the residual sum truncated
    (Rh, _), (Th, _) = C.stage3_ref(name)
    x = O.linear(C.rows(name, "ao"), _w(C.LAYER[3], "self_attn.o_proj"))
    _caught("o_proj's residual sum truncates", _trunc(x + C.rows(name, "hs")), Rh, Th)
    (Rh, _), (Th, _) = C.stage5_ref(name, 0)
    x = O.linear(C.rows(name, "act"), _w(0, "mlp.down_proj"))
    _caught("down's residual sum truncates", _trunc(x + C.rows(name, "hs")), Rh, Th)
    # stage 4: the GeGLU product truncated
    Ra, Ta = C.stage4_ref(name)
    g = O.gelu_tanh(O.linear(tn, _w(C.LAYER[4], "mlp.gate_proj")))
    _caught("GeGLU's product truncates", _trunc(g * O.linear(tn, _w(C.LAYER[4], "mlp.up_proj"))), Ra, Ta)


@pytest.mark.parametrize("name", ("D", "Dmax"))
def test_mutant_ii_rope_position_off_by_one(name):
    cfg, P = C.model()
    c = C.CASES[name]
    (Rq, Rk, _), (Tq, Tk, _) = C.stage1_ref(name)
    pos = c.pos.copy()
    pos[1, 3] += 1
    Gq, Gk, _ = R.ref_stage1(P, cfg, C.LAYER[1], C.rows(name, "tn")[1:2, 3:4], pos[1:2, 3:4])
    for nm, G1, Rr, T in (("q", Gq, Rq, Tq), ("k", Gk, Rk, Tk)):
        G = Rr.copy()
        G[1, 3] = G1[0, 0]
        _caught(f"{name} {nm}: one row's position + 1", G, Rr, T)


def test_mutant_iii_dropped_split_k_slab():
    name = "C"
    for stage, what, w, K, split in ((3, "ao", _w(C.LAYER[3], "self_attn.o_proj"), C.H, 4),
                                     (5, "act", _w(0, "mlp.down_proj"), C.I, 8)):
        (Rh, Rn), (Th, Tn) = C.stage3_ref(name) if stage == 3 else C.stage5_ref(name, 0)
        keep = np.ones(K, bool)
        keep[K // split:2 * (K // split)] = False
        G = O.bf16(O.bf16(C.rows(name, what)[..., keep] @ w[:, keep].T) + C.rows(name, "hs"))
        _caught(f"stage {stage}: slab 1 of {split} dropped", G, Rh, Th)


@pytest.mark.parametrize("name,row", (("D", (1, 16)), ("E", (2, 5)), ("A", (0, 100)), ("G", (0, 0))))
def test_mutant_iv_one_key_too_few(name, row):
    cfg, P = C.model()
    c = C.CASES[name]
    Rr, T = C.stage2_ref(name)
    q, kv = C.attn_inputs(name, C.LAYER[2])
    b, l = row
    G = Rr.copy()
    G[b, l] = R.ref_stage2(P, cfg, C.LAYER[2], q[b:b + 1, l:l + 1], kv[:, :, b:b + 1], c.kv_start,
                           None if c.lens is None else [c.lens[b]], L=c.L, less={(0, 0): 1})[0, 0]
    assert not np.array_equal(G, Rr)
    _caught(f"{name}: row {row} attends one key too few", G, Rr, T, ulp=False)


def test_mutant_v_kv_rows_one_slot_late():
    (_, Rk, Rv), (_, Tk, Tv) = C.stage1_ref("D")
    for nm, Rr, T in (("K", Rk, Tk), ("V", Rv, Tv)):
        G = np.roll(Rr, 1, axis=1)       # slot l holds row l - 1's; slot 0 what the late write left: stale content
        G[:, 0] = 1.0
        _caught(f"{nm} rows one slot late", G, Rr, T)


def test_mutant_vi_image_row_off_by_one():
    cfg, P = C.model()
    ids, feats = C.ids_feats("E")
    (Rh, Rn), (Th, Tn) = C.stage0_ref("E")
    Gh, Gn = R.ref_stage0(P, cfg, ids, feats[1:], C.CASES["E"].lens)
    assert not np.array_equal(Gh, Rh)                    # stage 0's condition: bit for bit
    live = _live(Rh)
    _caught("image row k + 1 at the k-th image token", C.rows2(Gn)[live], C.rows2(Rn)[live], C.rows2(Tn)[live])


@pytest.mark.parametrize("name", ("E", "Fr"))
def test_mutant_vii_ragged_logits_at_the_last_slot(name):
    cfg, P = C.model()
    (Rl, _), (Tl, _) = C.stage6_ref(name, 1)
    G, _ = R.ref_stage6(P, cfg, None, C.rows(name, "hs"), 1, lens=None)
    _caught("logits of slot L - 1", G, Rl, Tl, ulp=False, bias=True)
