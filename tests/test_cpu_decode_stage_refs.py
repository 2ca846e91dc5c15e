"""The decode-stage references (oracle/decode_stage_ref.py), no GPU.

1. Chained, ref_stage0..5 equal the oracle the rest of the suite trusts (O.paligemma_decode) bit for bit: B = 1, and
   two rows run separately, on the 2-text-layer full-width config with a vocabulary of 1,000.
2. On every case tests/test_gpu_decode_stages.py runs (tests/decode_stage_cases.py), the reference alone stays
   inside the caps that make the GPU test's thresholds (1.5 x its rel-L2, 3 x its d against the float64 truth)
   meaningful: rel-L2 <= 2^-7, d <= 0.05 and a signed mean error within 6 standard errors of zero
   (decode_stage_cases.CAP_*, BIAS_SE, with the reasoning); the fixed ulp conditions are stated against the
   reference itself.  One input was changed for a cap: the finite mask values have scale 1, not 2 (mask_row).
3. The conditions reject the faults they are there for, injected into the reference on the CPU: truncation in an
   epilogue, a swapped pair of columns, a stale element.

Measured reference distances, worst row of each case (R against T; d = max |x - t| / (|t| + rms t)):

    tensor                                   rel_l2(R, T)        d(R)
    stage 0 h (embedding x normalizer)       1.6e-3              1.9e-3
    stage 0 hn; input norm, layer 0 / 1      2.3e-3; 1.7e-3      3.8e-3; 2.6e-3 .. 2.7e-3
    stage 1 q, five position cases           2.4e-3 .. 3.4e-3    6.1e-3 .. 1.1e-2
    stage 1 k                                2.6e-3 .. 3.6e-3    5.0e-3 .. 8.3e-3
    stage 1 v                                2.6e-3              5.3e-3 .. 6.0e-3
    stage 2 h with the residual, every Lk    1.7e-3 .. 4.7e-3    2.5e-3 .. 1.2e-2
    stage 2 h on a zero h, every Lk          1.7e-3 .. 7.5e-3    2.4e-3 .. 2.2e-2   (worst: Lk 768, row 1)
    stage 2 attention output, every Lk       0 (Lk 1) .. 7.4e-3  0 .. 2.5e-2
    stage 2 random or chunk mask, h / ao     3.4e-3 .. 5.5e-3    7.1e-3 .. 1.6e-2
    stage 2 every key but one masked         ao 0 (exact); h 1.7e-3 .. 2.4e-3, d 2.4e-3 .. 4.1e-3
    stage 3 act                              4.3e-3              2.1e-2
    stage 4 h, layer 0 / 1                   2.3e-3 / 2.4e-3     4.6e-3 / 4.4e-3
    stage 4 hn (layer 1's input norm)        2.9e-3              5.6e-3
    stage 5 logits                           2.5e-3              5.7e-3

(`pytest -s` prints every case's figures.)
"""
import numpy as np
import pytest

import decode_stage_cases as C
from oracle import decode_stage_ref as D
from oracle import paligemma_np as O


def _inside(name, R, T, bias=True):
    rel, d = C.reference_distances(name, R, T)
    print(f"{name:34s} rel_l2(R, T) {rel:.3e}  d(R) {d:.3e}")
    assert rel <= C.CAP_REL and d <= C.CAP_D, (name, rel, d)
    if bias:   # (not attention outputs: one rounded probability moves all 256 elements of a head together)
        b, se = D.bias_rows(np.atleast_2d(R), np.atleast_2d(T))
        assert (np.abs(b) <= C.BIAS_SE * se).all(), (name, b, se)


# ---------------------------------------------------------------- 1. the chain is the oracle
def _oracle_step(P, cfg, ids, K, Vv, kv_len, position):
    """O.paligemma_decode for one row whose cache holds kv_len tokens per layer."""
    d = D.dims(cfg)
    kv = O.KV()
    for i in range(d["L"]):
        kv.update(K[i][None, None].copy(), Vv[i][None, None].copy(), i)   # (1, kv heads, tokens, head_dim)
    lg = O.paligemma_decode(P, cfg, np.array([ids]), kv, position)
    return lg[0, 0], [k[0, 0] for k in kv.k], [v[0, 0] for v in kv.v]


@pytest.mark.parametrize("rows", [1, 2])
def test_chained_references_equal_the_oracle(rows):
    cfg, P = C.model()
    d = D.dims(cfg)
    rng = np.random.default_rng(9)
    lens = [37, 12][:rows]
    pos = [38, 13][:rows]
    ids = [int(C.ids_rows()[3]), int(C.ids_rows()[0])][:rows]
    kv = D.new_kv(cfg, rows, 64)
    for b in range(rows):
        kv[:, :, b, :lens[b]] = O.bf16(rng.standard_normal((d["L"], 2, lens[b], 256)).astype(np.float32))
    kv0 = kv.copy()
    lg, nxt = D.ref_decode(P, cfg, ids, kv, lens, pos)
    for b in range(rows):
        want, Ks, Vs = _oracle_step(P, cfg, ids[b], kv0[:, 0, b, :lens[b]], kv0[:, 1, b, :lens[b]], lens[b], pos[b])
        assert np.array_equal(lg[b].view(np.uint32), want.view(np.uint32))
        assert nxt[b] == int(np.argmax(want))
        for i in range(d["L"]):
            assert np.array_equal(kv[i, 0, b, :lens[b] + 1].view(np.uint32), Ks[i].view(np.uint32))
            assert np.array_equal(kv[i, 1, b, :lens[b] + 1].view(np.uint32), Vs[i].view(np.uint32))
        assert np.isnan(kv[:, :, b, lens[b] + 1:]).all()          # nothing past the appended row


def test_pad_id_row_embeds_to_zero_and_normalizer_is_bf16():
    cfg, P = C.model()
    h, _ = D.ref_stage0(P, cfg, C.ids_rows()[:3])
    assert float(D.normalizer(cfg)) == 45.25
    assert not h[1].any() and h[0].any()
    E = P["language_model.model.embed_tokens.weight"]
    assert np.array_equal(h[0], O.bf16(E[C.V - 1] * np.float32(45.25)))


def test_rope_rows_clamp_to_the_table():
    cfg, _ = C.model()
    c, s = D.rope_rows(cfg, [C.MAX_POS - 1, C.MAX_POS + 5, -3, 0])
    assert np.array_equal(c[0], c[1]) and np.array_equal(s[0], s[1])
    assert np.array_equal(c[2], c[3]) and np.array_equal(s[2], s[3])


# ---------------------------------------------------------------- 2. the reference inside its caps, case by case
def test_stage0_and_norm():
    cfg, P = C.model()
    (Rh, Rn), (Th, Tn) = D.ref_stage0(P, cfg, C.ids_rows()[:16]), D.truth_stage0(P, cfg, C.ids_rows()[:16])
    _inside("stage0 h", Rh, Th)
    _inside("stage0 hn", np.delete(Rn, 1, 0), np.delete(Tn, 1, 0))     # (the pad row is zero on both sides)
    assert not Rn[1].any() and not Tn[1].any()
    for layer in (0, 1):
        _inside(f"input norm layer {layer}", *C.norm_ref(layer))


@pytest.mark.parametrize("case", range(len(C.QKV_CASES)))
def test_stage1(case):
    R, T = C.qkv_ref(case)
    for nm, r, t in zip("qkv", R, T):
        _inside(f"stage1 {C.QKV_CASES[case][0]} {nm}", r, t)


@pytest.mark.parametrize("zero_h", [False, True])
def test_stage2_key_counts(zero_h):
    """Every count (row 0, layer 0), the rows the lock-step and ragged calls add, with and without the residual."""
    todo = [(Lk, 0, 0) for Lk in C.LKS]
    todo += [(Lk, b, 0) for Lk in C.LOCK_LKS for b in (1, 3, 7, 15)]
    todo += [(Lk, b, 1) for b, Lk in enumerate(C.RAGGED16)] + [(Lk, b, 1) for b, Lk in enumerate(C.RAGGED2)]
    for Lk, b, layer in todo:
        r = C.attn_ref(Lk, b, layer, zero_h)
        _inside(f"stage2 Lk {Lk} row {b} layer {layer} zero_h {int(zero_h)} h", r["Rh"], r["Th"], bias=False)
        _inside(f"stage2 Lk {Lk} row {b} layer {layer} ao", r["Ra"], r["Ta"], bias=False)


@pytest.mark.parametrize("kind", C.MASKS)
@pytest.mark.parametrize("mask_round", [True, False])
def test_stage2_masks(kind, mask_round):
    for zero_h in (False, True):
        r = C.attn_ref(C.MASK_LK, 0, 0, zero_h, kind, mask_round)
        assert np.isfinite(r["Rh"]).all() and np.isfinite(r["Th"]).all()
        _inside(f"stage2 mask {kind} round {int(mask_round)} zero_h {int(zero_h)} h", r["Rh"], r["Th"], bias=False)
        _inside(f"stage2 mask {kind} round {int(mask_round)} ao", r["Ra"], r["Ta"], bias=False)


def test_stage3():
    _inside("stage3 act layer 0", *C.geglu_ref(0))


@pytest.mark.parametrize("layer", [0, 1])
def test_stage4(layer):
    (Rh, Rn), (Th, Tn) = C.down_ref(layer)
    _inside(f"stage4 h layer {layer}", Rh, Th)
    if layer == 0:
        _inside("stage4 hn layer 0", Rn, Tn)
    else:
        assert Rn is None and Tn is None


def test_stage5():
    (Rl, Ri), (Tl, Ti) = C.logits_ref()
    _inside("stage5 logits", Rl, Tl)
    # the tie rows: with embedding row 5 also in row 997, that pair is the maximum of every row
    cfg, P = C.model()
    P2 = dict(P)
    E = P["language_model.model.embed_tokens.weight"].copy()
    E[997] = E[5]
    P2["language_model.model.embed_tokens.weight"] = E
    lg, nxt = D.ref_stage5(P2, cfg, C.tie_rows())
    assert (nxt == 5).all() and np.array_equal(lg[:, 5], lg[:, 997])
    assert (np.delete(lg, [5, 997], axis=1).max(-1) < lg[:, 5] - 0.5).all()


# ---------------------------------------------------------------- 3. the conditions reject known faults
def _trunc(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def test_conditions_reject_injected_faults():
    cfg, P = C.model()
    (Rh, _), (Th, _) = C.down_ref(0)
    C.check("the reference itself", Rh, Rh, Th)
    x = O.bf16(C.act_rows() @ P["language_model.model.layers.0.mlp.down_proj.weight"].T)
    # truncation: the aggregate condition sees it at some rows only (1.2 .. 1.6 x the reference's rel-L2), the
    # signed mean error at every row
    for name, G, R, T in (
            ("down's epilogue truncates", _trunc(x + C.h_rows()), Rh, Th),
            ("v truncates", _trunc(C.norm_ref(0)[0] @ P["language_model.model.layers.0.self_attn.v_proj.weight"].T),
             *[r[2] for r in C.qkv_ref(2)])):
        with pytest.raises(AssertionError, match="rel_l2|truncation"):
            C.check(name, G, R, T)
        ratio = D.rel_l2_rows(G, T) / D.rel_l2_rows(R, T)
        assert ratio.min() < 1.5, "the aggregate condition alone would do"
        b, se = D.bias_rows(G, T)[0], D.bias_rows(R, T)[1]
        assert (np.abs(b) > C.BIAS_SE * se).all(), (name, b, se)
    G = Rh.copy()
    G[:, [100, 101]] = G[:, [101, 100]]
    with pytest.raises(AssertionError, match="rel_l2"):
        C.check("two columns swapped", G, Rh, Th)
    assert (D.d_rows(G, Th) > 3 * D.d_rows(Rh, Th)).all()
    G = Rh.copy()
    G[3, 777] = C.h_rows()[3, 777]
    with pytest.raises(AssertionError, match="row 3"):
        C.check("one stale element", G, Rh, Th)
    assert D.d_rows(G, Th)[3] > 3 * D.d_rows(Rh, Th)[3]
