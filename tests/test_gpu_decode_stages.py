"""The decode step, one stage at a time (pgmi_debug_decode_stage: the step's own launch code, stopped after each
stage) against oracle/decode_stage_ref.py: R = the reference's arithmetic (fp32 accumulation, bf16 where
modeling_gemma.py rounds), T = float64 truth of the same bf16 inputs and weights.  Engine: the 2-text-layer
full-width config, vocabulary 1,000 (a partial lm_head row group), max_batch 16, max_kv 1024, synthetic weights.

Per compared tensor, row by row (decode_stage_cases.check): rel_l2(G, T) <= 1.5 rel_l2(R, T); d(G) <= 3 d(R) with
d(X) = max |X - T| / (|T| + rms T); q, K, V, act, h, hn at least 99 % within 1 bf16 ulp of R; elementwise norm
outputs within 2 ulp of R everywhere; GEMV epilogues also keep their signed mean error within six standard errors
of zero (truncation: decode_stage_cases.BIAS_SE).  Attention outputs (ao, stage 2's h) are judged against T only: the kernel
rounds the chunk-local unnormalised e to bf16 where the reference rounds the normalised p.
No threshold comes from the kernel's output.

The reference's own distances (tests/test_cpu_decode_stage_refs.py measures them; worst row of each case), i.e.
what the thresholds are 1.5 x and 3 x of:

    tensor                                   rel_l2(R, T)        d(R)
    stage 0 h (embedding x normalizer)       1.6e-3              1.9e-3     (G must equal R bit for bit)
    input norm, layer 0 / 1                  1.7e-3              2.6e-3 .. 2.7e-3
    stage 1 q, five position cases           2.4e-3 .. 3.4e-3    6.1e-3 .. 1.1e-2
    stage 1 k                                2.6e-3 .. 3.6e-3    5.0e-3 .. 8.3e-3
    stage 1 v                                2.6e-3              5.3e-3 .. 6.0e-3
    stage 2 h / ao, no mask, every Lk        up to 5.4e-3        up to 2.2e-2   (Lk 1: ao exact, h 1.7e-3)
    stage 2 h / ao, random or chunk mask     3.4e-3 .. 5.5e-3    7.1e-3 .. 1.6e-2
    stage 2 all keys but one masked          ao 0 (exact), h 1.7e-3 .. 2.4e-3, d 2.4e-3 .. 4.1e-3
    stage 3 act                              4.3e-3              2.1e-2
    stage 4 h, layer 0 / 1                   2.3e-3 / 2.4e-3     4.6e-3 / 4.4e-3
    stage 4 hn (layer 1's input norm)        2.9e-3              5.6e-3
    stage 5 logits                           2.5e-3              5.7e-3

Every row at or past kv_len + 1 of the KV slab holds bf16 NaNs, and every output must be finite: nothing past a
row's length reaches a result."""
import numpy as np
import pytest
import torch

import decode_stage_cases as C
from oracle import decode_stage_ref as D
from oracle import paligemma_np as O
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BITS = 0x7FC1   # a bf16 NaN bit pattern
STAGED, PACKED = (0, 1), (7, 0)


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    cfg, _ = C.model()
    e = Engine(cfg, max_batch=C.MAX_BATCH, max_seq=64, max_kv=C.KV_MAX)
    e.fill_synthetic(C.SEED, W.init_policy)
    e.prepare()
    yield e
    e.set_decode_staged_norm(-1)
    e.set_decode_packed(-1)


def bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(DEV)


def f32(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16)


def forms(B):
    """The settings a batch runs under: both norm forms at B >= 3, packed on and off at B <= 2."""
    return [("staged", s) for s in STAGED] if B >= 3 else [("packed", p) for p in PACKED]


def set_form(eng, form):
    if form[0] == "staged":
        eng.set_decode_staged_norm(form[1])
    else:
        eng.set_decode_packed(form[1])


def unstaged(B, form):
    return B >= 3 and form == ("staged", 0)


def put(eng, which, x, dtype=torch.bfloat16):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV).contiguous()
    eng.decode_buffer(which, t, write=True)


def get(eng, which, rows, cols, dtype=torch.bfloat16):
    t = eng.decode_buffer(which, torch.empty((rows, cols), dtype=dtype, device=DEV))
    torch.cuda.synchronize()
    return t


def nan_slab(eng):
    kv = eng.new_kv(C.KV_BATCH, C.KV_MAX)
    kv.view(torch.int16).fill_(NAN_BITS)
    return kv


@pytest.fixture(scope="module")
def sentinel(eng):
    """A slab of seeded finite bf16 bit patterns (mid-range exponents); tests run on clones of it."""
    kv = eng.new_kv(C.KV_BATCH, C.KV_MAX)
    g = torch.Generator().manual_seed(5)
    r = torch.randint(0, 1 << 13, tuple(kv.shape[1:]), generator=g, dtype=torch.int32)
    pat = ((r & 0x1000) << 3) | (0x3C00 + (r & 0x07FF))         # sign, exponent 120..135, mantissa
    pat = torch.where(pat >= 0x8000, pat - 0x10000, pat).to(torch.int16).to(DEV)
    kv.view(torch.int16).copy_(pat[None].expand(kv.shape[0], *pat.shape))
    return kv


# ---------------------------------------------------------------- stage 0
@pytest.mark.parametrize("B", C.BATCHES)
def test_stage0_embedding_and_input_norm(eng, B):
    cfg, P = C.model()
    kv = nan_slab(eng)
    for first in (0, 1):   # rows 0.. (vocab - 1 first, then the pad id) and rows 1.. (the pad id first)
        ids_np = C.ids_rows()[first:first + B]
        (Rh, Rn), (Th, Tn) = D.ref_stage0(P, cfg, ids_np), D.truth_stage0(P, cfg, ids_np)
        ids = torch.from_numpy(ids_np).to(DEV)
        for form in forms(B):
            set_form(eng, form)
            put(eng, 0, np.full((B, C.H), 7.0, np.float32))
            put(eng, 5, np.full((B, C.H), 7.0, np.float32))
            eng.decode_stage(0, 0, B, kv, 0, 1, ids=ids)
            h, hn = f32(get(eng, 0, B, C.H)), f32(get(eng, 5, B, C.H))
            if B <= 2:   # the fold: layer 0's q|k|v embeds, the entry does nothing
                assert (h == 7.0).all() and (hn == 7.0).all()
                continue
            assert np.array_equal(h, Rh)                  # one exact product, one rounding: bit for bit
            if unstaged(B, form):
                live = np.abs(Rh).sum(-1) > 0             # (a pad row is zero: its norm is zero on every side)
                C.check(f"stage0 hn B{B}", hn[live], Rn[live], Tn[live])
                C.check_norm(f"stage0 hn B{B}", hn, Rn)
                assert not hn[~live].any()
            else:
                assert (hn == 7.0).all()                  # the staged form never writes hn


# ---------------------------------------------------------------- stage 1
def _run_qkv(eng, B, form, case, kv0, ids=None, h=None):
    """Stage 1 of QKV_CASES[case] on a copy of the slab kv0 -> q, the slab."""
    _, layer, lens, pos, ragged = C.QKV_CASES[case]
    kv = kv0.clone()
    if h is not None:
        put(eng, 0, h[:B])
        if unstaged(B, form):   # the unstaged q|k|v reads the rows stage 4 (or the entry) normed
            put(eng, 5, C.norm_ref(layer)[0][:B])
    put(eng, 3, np.full((B, C.QD), 7.0, np.float32))
    eng.decode_stage(1, layer, B, kv, lens[:B], pos[:B], ids=ids, ragged=ragged)
    return get(eng, 3, B, C.QD), kv


def _check_slab(kv, kv0, layer, lens, B, Rk, Rv, Tk, Tv, name):
    """Rows kv_lens[b] of `layer` hold the new K / V; every other element of the slab is bit-unchanged."""
    rows = torch.tensor(lens[:B], device=DEV)
    bs = torch.arange(B, device=DEV)
    C.check(name + " K", f32(kv[layer, 0, bs, rows]), Rk[:B], Tk[:B])
    C.check(name + " V", f32(kv[layer, 1, bs, rows]), Rv[:B], Tv[:B])
    back = kv.clone()
    back[layer, :, bs, rows] = kv0[layer, :, bs, rows]
    assert torch.equal(bits(back), bits(kv0)), name + ": an element outside the appended rows changed"


@pytest.mark.parametrize("case", range(len(C.QKV_CASES)), ids=[c[0] for c in C.QKV_CASES])
@pytest.mark.parametrize("B", C.BATCHES)
def test_stage1_qkv(eng, sentinel, B, case):
    name, layer, lens, pos, ragged = C.QKV_CASES[case]
    (Rq, Rk, Rv), (Tq, Tk, Tv) = C.qkv_ref(case)
    kv0 = sentinel
    for form in forms(B):
        set_form(eng, form)
        q, kv = _run_qkv(eng, B, form, case, kv0, h=C.h_rows())
        C.check(f"stage1 {name} B{B} {form} q", f32(q), Rq[:B], Tq[:B])
        use = lens if ragged else (lens[0],) * 16
        _check_slab(kv, kv0, layer, use, B, Rk, Rv, Tk, Tv, f"stage1 {name} B{B} {form}")


@pytest.mark.parametrize("B", C.BATCHES)
def test_stage1_layer0_from_ids_equals_explicit_rows(eng, sentinel, B):
    """Layer 0 fed ids (B <= 2: the embedding folded into q|k|v) against the same stage fed the embedded, scaled
    rows: q and the slab bit for bit, and h holds the scaled rows afterwards."""
    cfg, P = C.model()
    kv0 = sentinel
    case = 2   # layer 0, kv_len 40, position 41
    for first in (0, 1):
        ids_np = C.ids_rows()[first:first + B]
        Rh, _ = D.ref_stage0(P, cfg, ids_np)
        ids = torch.from_numpy(ids_np).to(DEV)
        for form in forms(B):
            set_form(eng, form)
            put(eng, 0, np.full((B, C.H), 7.0, np.float32))
            kv = kv0.clone()
            eng.decode_stage(0, 0, B, kv, 40, 41, ids=ids)
            eng.decode_stage(1, 0, B, kv, 40, 41, ids=ids)
            q1, h1 = get(eng, 3, B, C.QD).clone(), get(eng, 0, B, C.H).clone()
            put(eng, 0, Rh)
            kv2 = kv0.clone()
            eng.decode_stage(0, 0, B, kv2, 40, 41)       # ids = None: h as written (B >= 3 unstaged: normed here)
            eng.decode_stage(1, 0, B, kv2, 40, 41)
            q2 = get(eng, 3, B, C.QD)
            assert torch.equal(bits(q1), bits(q2)) and torch.equal(bits(kv), bits(kv2))
            assert np.array_equal(f32(h1), Rh)
            live = np.abs(Rh).sum(-1) > 0               # (a pad row is zero, and so is its q)
            assert np.isfinite(f32(q1)).all() and bool(np.abs(f32(q1)[live]).sum(-1).all())
            assert not f32(q1)[~live].any()


# ---------------------------------------------------------------- stage 2
def _run_attn(eng, B, form, layer, rows, zero_h, ragged, mask=None, mask_dtype=None):
    """rows: (Lk, b) per batch row.  -> h, ao (B >= 3), ssq (unstaged), and the slab before / after."""
    kv = nan_slab(eng)
    q = np.zeros((B, C.QD), np.float32)
    h = np.zeros((B, C.H), np.float32)
    for i, (Lk, b) in enumerate(rows):
        qi, K, Vv, hi = C.attn_row(Lk, b)
        q[i] = qi
        h[i] = 0 if zero_h else hi
        kv[layer, 0, i, :Lk] = bf(K)
        kv[layer, 1, i, :Lk] = bf(Vv)
    kv0 = kv.clone()
    put(eng, 3, q)
    put(eng, 0, h)
    put(eng, 4, np.full((B, C.H), 7.0, np.float32))
    lens = [Lk - 1 for Lk, _ in rows]
    m = None
    if mask is not None:
        m = torch.from_numpy(C.mask_row(mask)).to(mask_dtype).to(DEV).contiguous()
    eng.decode_stage(2, layer, B, kv, lens, [n + 1 for n in lens], ragged=ragged, mask=m)
    out = dict(h=f32(get(eng, 0, B, C.H)), ao=f32(get(eng, 4, B, C.H)))
    if unstaged(B, form):
        out["ssq"] = f32(get(eng, 6, B, C.H // 16, torch.float32))
    assert torch.equal(bits(kv), bits(kv0)), "stage 2 wrote to the KV slab"
    return out


def _check_attn(name, eng, B, form, layer, rows, zero_h, got, mask=None, mask_round=True):
    refs = [C.attn_ref(Lk, b, layer, zero_h, mask, mask_round) for Lk, b in rows]
    Rh, Th = np.stack([r["Rh"] for r in refs]), np.stack([r["Th"] for r in refs])
    Ra, Ta = np.stack([r["Ra"] for r in refs]), np.stack([r["Ta"] for r in refs])
    C.check(name + " h", got["h"], Rh, Th, ulp=False)
    if B >= 3:
        C.check(name + " ao", got["ao"], Ra, Ta, ulp=False)
    else:
        assert (got["ao"] == 7.0).all()       # B <= 2: the combine stays in o_proj's registers
    if "ssq" in got:   # the partial sums of squares of the h the consuming norm reads: fp32 sums of 16 squares
        want = C.ssq_of(got["h"])
        assert np.allclose(got["ssq"], want, rtol=2e-6, atol=0), name + " ssq"


@pytest.mark.parametrize("zero_h", [False, True], ids=["res", "nores"])
@pytest.mark.parametrize("Lk", C.LKS)
def test_stage2_every_key_count_b1(eng, Lk, zero_h):
    for form in forms(1):
        set_form(eng, form)
        rows = [(Lk, 0)]
        _check_attn(f"stage2 Lk{Lk} B1 {form}", eng, 1, form, 0, rows, zero_h,
                    _run_attn(eng, 1, form, 0, rows, zero_h, False))


@pytest.mark.parametrize("zero_h", [False, True], ids=["res", "nores"])
@pytest.mark.parametrize("B", C.LOCK_BS[1:])
def test_stage2_lock_step(eng, B, zero_h):
    for Lk in C.LOCK_LKS:
        rows = [(Lk, b) for b in range(B)]
        for form in forms(B):
            set_form(eng, form)
            _check_attn(f"stage2 Lk{Lk} B{B} {form}", eng, B, form, 0, rows, zero_h,
                        _run_attn(eng, B, form, 0, rows, zero_h, False))


@pytest.mark.parametrize("zero_h", [False, True], ids=["res", "nores"])
@pytest.mark.parametrize("counts", [C.RAGGED16, C.RAGGED2], ids=["b16", "b2"])
def test_stage2_ragged(eng, counts, zero_h):
    B = len(counts)
    rows = [(Lk, b) for b, Lk in enumerate(counts)]
    for form in forms(B):
        set_form(eng, form)
        _check_attn(f"stage2 ragged B{B} {form}", eng, B, form, 1, rows, zero_h,
                    _run_attn(eng, B, form, 1, rows, zero_h, True))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", C.MASKS)
def test_stage2_mask_b1(eng, kind, dtype):
    rows = [(C.MASK_LK, 0)]
    for form in forms(1):
        set_form(eng, form)
        for zero_h in (False, True):
            got = _run_attn(eng, 1, form, 0, rows, zero_h, False, kind, dtype)
            _check_attn(f"stage2 mask {kind} {dtype} {form} zero_h {zero_h}", eng, 1, form, 0, rows, zero_h, got,
                        kind, dtype == torch.bfloat16)


# ---------------------------------------------------------------- stage 3, 4
@pytest.mark.parametrize("B", C.BATCHES)
def test_stage3_geglu(eng, B):
    R, T = C.geglu_ref(0)
    kv = nan_slab(eng)
    for form in forms(B):
        set_form(eng, form)
        put(eng, 0, C.h_rows()[:B])
        if unstaged(B, form):   # gate|up normalises on load from o_proj's partial sums of squares
            put(eng, 6, C.ssq_of(C.h_rows()[:B]).astype(np.float32), torch.float32)
        put(eng, 1, np.full((B, C.I), 7.0, np.float32))
        eng.decode_stage(3, 0, B, kv, 3, 4)
        C.check(f"stage3 B{B} {form}", f32(get(eng, 1, B, C.I)), R[:B], T[:B])


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("B", C.BATCHES)
def test_stage4_down(eng, B, layer):
    cfg, P = C.model()
    (Rh, Rn), (Th, Tn) = C.down_ref(layer)
    kv = nan_slab(eng)
    for form in forms(B):
        set_form(eng, form)
        put(eng, 1, C.act_rows()[:B])
        put(eng, 0, C.h_rows()[:B])
        put(eng, 5, np.full((B, C.H), 7.0, np.float32))
        eng.decode_stage(4, layer, B, kv, 3, 4)
        h, hn = f32(get(eng, 0, B, C.H)), f32(get(eng, 5, B, C.H))
        C.check(f"stage4 layer {layer} B{B} {form} h", h, Rh[:B], Th[:B])
        if unstaged(B, form) and layer == 0:   # + layer 1's input norm of the new h
            C.check(f"stage4 B{B} hn", hn, Rn[:B], Tn[:B])
            w = P["language_model.model.layers.1.input_layernorm.weight"]
            C.check_norm(f"stage4 B{B} hn", hn, O.rms_norm(h, w, D.dims(cfg)["eps"]))
        else:                                  # the last layer, the staged form, B <= 2: hn stays as it was
            assert (hn == 7.0).all()


# ---------------------------------------------------------------- stage 5
@pytest.mark.parametrize("B", C.BATCHES)
def test_stage5_logits_and_next_ids(eng, B):
    (Rl, _), (Tl, _) = C.logits_ref()
    kv = nan_slab(eng)
    for form in forms(B):
        set_form(eng, form)
        put(eng, 0, C.h_rows()[:B])
        put(eng, 7, np.full((B, 1), -1, np.int64), torch.int64)
        eng.decode_stage(5, 0, B, kv, 3, 4)
        lg = f32(get(eng, 2, B, C.V, torch.float32))
        nxt = get(eng, 7, B, 1, torch.int64).cpu().numpy()[:, 0]
        C.check(f"stage5 B{B} {form}", lg, Rl[:B], Tl[:B], ulp=False, bias=True)
        assert np.array_equal(nxt, np.argmax(lg, axis=-1))       # the first maximum of the logits it wrote


def test_stage5_exact_tie_takes_the_first_maximum(eng):
    """Embedding row 5 copied into row 997 (different lm_head workgroup partitions): bit-equal logits, next id 5."""
    E = eng.views["language_model.model.embed_tokens.weight"]
    keep = E[997].clone()
    kv = nan_slab(eng)
    try:
        E[997] = E[5]
        eng.prepare()
        for B in C.BATCHES:
            for form in forms(B):
                set_form(eng, form)
                put(eng, 0, C.tie_rows()[:B])
                eng.decode_stage(5, 0, B, kv, 3, 4)
                lg = get(eng, 2, B, C.V, torch.float32)
                nxt = get(eng, 7, B, 1, torch.int64).cpu()[:, 0]
                assert torch.equal(lg[:, 5].view(torch.int32), lg[:, 997].view(torch.int32)), (B, form)
                assert bool((lg.argmax(-1).cpu() == 5).all()) and bool((nxt == 5).all()), (B, form, nxt)
    finally:
        E[997] = keep
        eng.prepare()


# ---------------------------------------------------------------- the hook runs the production launch sequence
def _filled_slab(eng, lens):
    kv = nan_slab(eng)
    g = torch.Generator().manual_seed(3)
    for b, n in enumerate(lens):
        kv[:, :, b, :n] = torch.randn((2, 2, n, C.KD), generator=g).to(torch.bfloat16).to(DEV)
    return kv


@pytest.mark.parametrize("B,ragged", [(1, False), (2, False), (5, False), (16, False), (2, True), (16, True)])
def test_chained_stages_equal_the_eager_step(eng, B, ragged):
    eng.set_decode_staged_norm(-1)
    eng.set_decode_packed(-1)
    lens = [(53 * b + 70) % 300 + 1 for b in range(B)] if ragged else [100] * B
    pos = [n + 2 for n in lens] if ragged else [101] * B
    ids = torch.from_numpy(C.ids_rows()[:B]).to(DEV)
    kv0 = _filled_slab(eng, lens)
    kv_e = kv0.clone()
    nx_e = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    if ragged:
        lg_e = eng.decode_ragged(ids, kv_e, lens, pos, next_ids=nx_e)
    else:
        lg_e = eng.decode(ids, kv_e, lens[0], pos[0], next_ids=nx_e)
    torch.cuda.synchronize()
    kv_s = kv0.clone()
    eng.decode_stage(0, 0, B, kv_s, lens, pos, ids=ids, ragged=ragged)
    for layer in (0, 1):
        for stage in (1, 2, 3, 4):
            eng.decode_stage(stage, layer, B, kv_s, lens, pos, ids=ids, ragged=ragged)
    eng.decode_stage(5, 0, B, kv_s, lens, pos, ragged=ragged)
    lg_s = get(eng, 2, B, C.V, torch.float32)
    nx_s = get(eng, 7, B, 1, torch.int64)[:, 0]
    assert torch.equal(lg_s.view(torch.int32), lg_e.view(torch.int32))
    assert torch.equal(nx_s, nx_e) and bool((nx_e >= 0).all())
    assert torch.equal(bits(kv_s), bits(kv_e))
    assert bool(torch.isfinite(lg_e).all())


# ---------------------------------------------------------------- argument checks
def test_argument_checks(eng):
    kv = nan_slab(eng)
    ok = dict(kv=kv, kv_lens=3, positions=4)
    for stage, layer, B in ((6, 0, 1), (-1, 0, 1), (1, 2, 1), (3, -1, 1), (1, 0, 17), (1, 0, 0)):
        with pytest.raises(ValueError):
            eng.decode_stage(stage, layer, B, **ok)
    with pytest.raises(ValueError):   # a mask with B != 1
        eng.decode_stage(2, 0, 2, kv, 3, 4, mask=torch.zeros(4, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):   # kv_lens[b] + 1 > kv_max
        eng.decode_stage(1, 0, 1, kv, C.KV_MAX, 4)
    with pytest.raises(ValueError):   # a ragged row past the slab
        eng.decode_stage(1, 0, 2, kv, [3, C.KV_MAX], [4, 5], ragged=True)
    small = eng.new_kv(2, 64)
    with pytest.raises(ValueError):   # B over the slab's batch
        eng.decode_stage(1, 0, 3, small, 3, 4)
    caps = {3: C.MAX_BATCH * C.QD * 2, 4: C.MAX_BATCH * C.H * 2, 5: C.MAX_BATCH * C.H * 2,
            6: C.MAX_BATCH * (C.H // 16) * 4, 7: C.MAX_BATCH * 8}
    for which, cap in caps.items():
        eng.decode_buffer(which, torch.empty(cap, dtype=torch.uint8, device=DEV))            # the whole buffer
        with pytest.raises(ValueError):
            eng.decode_buffer(which, torch.empty(cap + 2, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        eng.decode_buffer(8, torch.empty(16, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
