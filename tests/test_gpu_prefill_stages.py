"""The language-model prefill, one stage of one row group at a time (pgmi_debug_prefill_stage: the prefill's own
launch code, stopped after each stage) against oracle/prefill_stage_ref.py: R = the reference's arithmetic (fp32
accumulation, bf16 where modeling_gemma.py rounds), T = float64 truth of the same bf16 inputs and weights.  Engine:
the 2-text-layer full-width config, vocabulary 1,000, max_batch 16, max_seq 320, max_kv 1024, synthetic weights,
prefill graphs off (the hook is eager; no test here captures or replays a graph).  The KV slab has 17 batch rows.

Cases (tests/prefill_stage_cases.py): A 1 x 288 (the M = 288 table plans), B 1 x 1, C 1 x 33 (fallback plans; then
the M = 288 table's four configurations forced for M = 33; then q|k|v forced to split, so the fused RoPE epilogue is
refused and rope_kv_append reduces slabs; then a tile without the RoPE epilogue), D 2 x 17 at kv_start 47 (row 1's
positions shifted; Dmax: positions up to 8191), E 3 x 40 ragged (1, 40, 23), F 9 x 8 lock-step and ragged (a second
row group of one row), G 1 x 17 at kv_start 500 (517 keys: the key-split attention; stages 1 and 2).  Stage 7 runs
on C, D, T3 (3 x 17 at 47), F, and past the config's max_kv on a 1040-token slab (X1, X3: the prefill attention
kernel + gemv_res branch).  A stage's inputs are seeded rows written through pgmi_debug_prefill_buffer.

Per compared tensor, row by row (decode_stage_cases.check, unchanged): rel_l2(G, T) <= 1.5 rel_l2(R, T); d(G) <= 3
d(R) with d(X) = max |X - T| / (|T| + rms T); q, K, V, hs, act, tn at least 99 % within 1 bf16 ulp of R, the GEMM
epilogues among them (q, K, V, hs, act) with a signed mean error within six standard errors of zero; norm outputs
(tn) also within 2 ulp of the norm of the kernel's own hs; logits the first two and the signed mean error.  Stage 0's hs equals R bit for bit.  Attention outputs (stage 2's
AO; stage 7's lastrows and the logits from them) are judged against T only: the prefill attention (k_attn_fs at
every Gemma size) and the tail's flash-decoding round the unnormalised e = exp(s - m) to bf16 where the reference
rounds the normalised p ("Deliberate deviations").  No threshold comes from the kernel's output.

Guards on every case: K/V slots a row must not read hold bf16 NaN and every output is finite; on a clone of a
seeded finite sentinel slab everything outside batch rows b < B (of the group), slots [kv_start, kv_start + L) of
the stage's layer is unchanged bit for bit; every workspace buffer (Hs, Tn, QKV, Qr, AO, ACT, lastrows, dAO) is
pre-filled with a sentinel past the stage's rows, and the rows a stage does not own -- past the group's B x L, and
the other group's rows of Hs, Tn, lastrows and the logits -- are unchanged after it.  A ragged row's pad slots
[lens[b], L) receive the K/V of their own (pad) rows like any other slot -- k_rope_kv and the fused epilogue
(kernels_gemm.hip rope_apply) write slot l < L of every row from that slot's normed row at that slot's position,
and nothing reads them: the row attends keys [0, kv_start + lens[b]) ("every row ... attends its own
keys") and the decode step overwrites them from lens[b] on -- so they are compared with R like every other slot.

The reference's own distances (tests/test_cpu_prefill_stage_refs.py measures them; worst row over the cases), i.e.
what the thresholds are 1.5 x and 3 x of, and the worst kernel / reference ratios measured on an MI355X:

    tensor                                  rel_l2(R, T)        d(R)                kernel / reference (rel_l2, d)
    stage 0 hs (G must equal R bit for bit) 1.6e-3 .. 2.0e-3    1.9e-3 .. 4.1e-3    equal
    stage 0 tn (layer 0's input norm)       2.2e-3 .. 2.6e-3    3.8e-3 .. 6.0e-3    1.00, 1.00
    stage 1 q / K / V                       1.6e-3 .. 3.4e-3    2.1e-3 .. 1.4e-2    1.00, 1.00
    stage 2 ao                              0 (one key) .. 5.5e-3   0 .. 2.8e-2     1.39 (A), 1.61 (G)
    stage 3 hs / tn                         2.4e-3 .. 3.1e-3    4.7e-3 .. 6.9e-3    1.00, 1.00
    stage 4 act                             3.5e-3 .. 3.7e-3    8.5e-3 .. 1.1e-2    1.00, 1.00
    stage 5 hs / tn, layer 0 and 1          2.3e-3 .. 3.0e-3    3.8e-3 .. 6.9e-3    1.00, 1.00
    stage 6 logits, every row / last rows   1.6e-3 .. 2.4e-3    2.4e-3 .. 5.4e-3    1.00, 1.00
    stage 7 ao / lastrows / logits          up to 4.7e-3 / 6.6e-3 / 7.4e-3   up to 2.0e-2 / 1.9e-2 / 2.3e-2
                                                                                    1.03, 1.08 / 1.02, 1.40 / 1.05, 1.20

(The ratios are those of the row each check prints, the one nearest its threshold; 1.00: the kernel's row equals the
reference's to three digits, its elements within 1 ulp of R at 100.00 %.)  Worst over the file: 1.39 x for rel-L2
and 1.61 x for d, both in stage 2, against the allowed 1.5 x and 3 x.  No test is skipped or marked xfail; case A
runs stage 5 on layer 0 only.  The file takes 12.0 s on an MI355X (99 tests, the CPU references included), beside
the decode file's 9.0 s (159 tests) in the same run; no sentinel row, KV slot or logits row outside a stage's own
was ever written."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import prefill_stage_cases as C
from oracle import paligemma_np as O
from oracle import prefill_stage_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BITS = 0x7FC1   # a bf16 NaN bit pattern
SENT = 7.0          # the workspace sentinel
GUARD = 8           # sentinel rows kept past a stage's rows
BF = torch.bfloat16
QKVN = C.QD + 2 * C.KD
HS, TN, QKV, QR, AO, ACT, LAST, DAO = range(8)


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    cfg, _ = C.model()
    e = Engine(cfg, max_batch=C.MAX_BATCH, max_seq=C.MAX_SEQ, max_kv=C.KV_MAX)
    e.fill_synthetic(C.SEED, W.init_policy)
    e.prepare()
    e.set_prefill_graph(False)
    yield e
    e.set_prefill_graph(True)


def bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(BF).to(DEV)


def f32(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def nan_slab(eng, kv_max=C.KV_MAX, fill=None):
    """A slab of bf16 NaNs; fill: a compact [2][2][B][tokens][KD] array copied to batch rows 0 .., tokens 0 .."""
    kv = eng.new_kv(C.KV_BATCH, kv_max)
    kv.view(torch.int16).fill_(NAN_BITS)
    if fill is not None:
        kv[:, :, :fill.shape[2], :fill.shape[3]] = bf(fill)
        nan = torch.from_numpy(np.isnan(fill)).to(DEV)
        kv[:, :, :fill.shape[2], :fill.shape[3]].view(torch.int16)[nan] = NAN_BITS
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


@contextlib.contextmanager
def forced(eng, plans):
    """GEMM plans forced per shape (process-wide overrides), removed on the way out."""
    try:
        for M, N, K, dual, cfg, split in plans:
            assert eng.lib.pgmi_tune_gemm_shape(M, N, K, dual, cfg, split) == 0
            got = [ctypes.c_int() for _ in range(4)]
            assert eng.lib.pgmi_debug_gemm_plan(M, N, K, dual, *[ctypes.byref(x) for x in got]) == 0
            assert (got[0].value, got[3].value) == (cfg, split)
        yield
    finally:
        for M, N, K, dual, _, _ in plans:
            eng.lib.pgmi_tune_gemm_shape(M, N, K, dual, -1, 0)


PLANS = {"": (), "table": C.C_TABLE_PLANS, "split": C.C_SPLIT_QKV, "plain": C.C_PLAIN_QKV}
RUNS = [(n, "") for n in C.STAGE_CASES] + [("C", "table")]
RUNS1 = RUNS + [("G", ""), ("Dmax", ""), ("C", "split"), ("C", "plain")]
run_ids = lambda runs: [n + ("-" + p if p else "") for n, p in runs]  # noqa: E731


class Work:
    """The prefill workspace as a test arms it: every buffer a sentinel over the stage's rows and GUARD rows past them,
    the stage's inputs on top.  read() returns what the engine holds afterwards; same() asserts that everything but
    the named row ranges is what was written."""

    def __init__(self, eng, c):
        self.eng = eng
        n_all, n_g = c.B * c.L + GUARD, min(C.GROUP, c.B) * c.L + GUARD
        shape = {HS: (n_all, C.H), TN: (n_all, C.H), QKV: (n_g, QKVN), QR: (n_g, C.QD), AO: (n_g, C.H),
                 ACT: (n_g, C.I), LAST: (C.MAX_BATCH, C.H), DAO: (C.MAX_BATCH, C.H)}
        self.t = {w: torch.full(s, SENT, dtype=BF, device=DEV) for w, s in shape.items()}

    def set(self, which, x, r0=0):
        x = C.rows2(x)
        self.t[which][r0:r0 + x.shape[0]] = bf(x)
        return self

    def flush(self):
        for w, t in self.t.items():
            self.eng.prefill_buffer(w, t, write=True)
        return self

    def read(self):
        got = {w: self.eng.prefill_buffer(w, torch.empty_like(t)) for w, t in self.t.items()}
        torch.cuda.synchronize()
        return got

    def same(self, got, name, changed):
        """changed: {which: (r0, r1)} -- the only rows a stage may have written."""
        for w, t in self.t.items():
            a, b = bits(got[w]).clone(), bits(t)
            if w in changed:
                r0, r1 = changed[w]
                a[r0:r1] = b[r0:r1]
            assert torch.equal(a, b), f"{name}: buffer {w} changed outside the stage's rows"


def logits_buf(c, logits_rows):
    """The call's logits and one sentinel row past them."""
    return torch.full((c.B * (c.L if logits_rows == 0 else 1) + 1, C.V), SENT, dtype=torch.float32, device=DEV)


def stage(eng, st, layer, g, name, kv, logits, logits_rows=0, ids=None, feats=None, embeds=None):
    c = C.CASES[name]
    if ids is None and embeds is None:   # the call's arguments are pgmi_lm_forward's, which refuses a call without either
        ids = torch.from_numpy(C.ids_feats(name)[0]).to(DEV)
    eng.prefill_stage(st, layer, g, kv, c.kv_start, c.pos, logits, ids=ids, image_feats=feats, embeds=embeds, B=c.B,
                      L=c.L, logits_rows=logits_rows, lens=c.lens)


def slab_same(kv, before, name, layer=None, rows=None, slots=None):
    """Everything outside [layer][K|V][rows][slots] is bit-unchanged."""
    back = kv.clone()
    if layer is not None:
        back[layer, :, rows, slots] = before[layer, :, rows, slots]
    assert torch.equal(bits(back), bits(before)), f"{name}: the KV slab changed outside the stage's rows"


# ---------------------------------------------------------------- stage 0
@pytest.mark.parametrize("name", C.STAGE_CASES)
def test_stage0_merge_and_input_norm(eng, sentinel, name):
    cfg, P = C.model()
    c = C.CASES[name]
    ids, feats = C.ids_feats(name)
    n = c.B * c.L
    forms = [("ids", C.stage0_ref(name), dict(ids=torch.from_numpy(ids).to(DEV), feats=bf(feats)))]
    if c.lens is None:   # given rows (the drop-in API's merge): scale_rows
        forms.append(("embeds", C.stage0_ref(name, embeds=True), dict(embeds=bf(C.rows(name, "emb")))))
    for form, ((Rh, Rn), (Th, Tn)), kw in forms:
        kv = sentinel.clone()
        w = Work(eng, c).flush()
        lg = logits_buf(c, 0)
        stage(eng, 0, 0, 0, name, kv, lg, **kw)
        got = w.read()
        hs, tn = f32(got[HS][:n]), f32(got[TN][:n])
        assert np.array_equal(hs, C.rows2(Rh)), f"stage0 {name} {form}: hs differs from the reference"
        live = np.abs(C.rows2(Rh)).sum(-1) > 0           # (pad ids and pad slots are zero rows, and so is their norm)
        C.check(f"stage0 {name} {form} tn", tn[live], C.rows2(Rn)[live], C.rows2(Tn)[live], bias=False)
        C.check_norm(f"stage0 {name} {form} tn", tn, C.rows2(Rn))
        assert not tn[~live].any()
        w.same(got, f"stage0 {name} {form}", {HS: (0, n), TN: (0, n)})
        slab_same(kv, sentinel, f"stage0 {name} {form}")
        assert bool((lg == SENT).all())


# ---------------------------------------------------------------- stage 1
@pytest.mark.parametrize("name,plan", RUNS1, ids=run_ids(RUNS1))
def test_stage1_qkv_rope_kv_append(eng, sentinel, name, plan):
    c = C.CASES[name]
    layer = C.LAYER[1]
    (Rq, Rk, Rv), (Tq, Tk, Tv) = C.stage1_ref(name)
    slots = slice(c.kv_start, c.kv_start + c.L)
    with forced(eng, PLANS[plan]):
        kv = sentinel.clone()
        for g, b0, Bg in C.groups(c):
            tag = f"stage1 {name} {plan} group {g}"
            before = kv.clone()
            w = Work(eng, c).set(TN, C.rows(name, "tn")).flush()
            lg = logits_buf(c, 0)
            stage(eng, 1, layer, g, name, kv, lg)
            got = w.read()
            sl = slice(b0, b0 + Bg)
            C.check(tag + " q", f32(got[QR][:Bg * c.L]), Rq[sl], Tq[sl])
            C.check(tag + " K", f32(kv[layer, 0, sl, slots]), Rk[sl], Tk[sl])     # (pad slots included: their own rows)
            C.check(tag + " V", f32(kv[layer, 1, sl, slots]), Rv[sl], Tv[sl])
            slab_same(kv, before, tag, layer, sl, slots)
            w.same(got, tag, {QR: (0, Bg * c.L), QKV: (0, Bg * c.L)})               # (QKV: scratch of the unfused path)
            assert bool((lg == SENT).all())


# ---------------------------------------------------------------- stage 2
@pytest.mark.parametrize("name", C.STAGE_CASES + ("G",))
def test_stage2_attention(eng, name):
    c = C.CASES[name]
    layer = C.LAYER[2]
    Ra, Ta = C.stage2_ref(name)
    q, fill = C.attn_inputs(name, layer)
    kv = nan_slab(eng, c.kv_max, fill)       # NaN: every slot at or past a row's kv_start + n_b, every other row
    before = kv.clone()
    for g, b0, Bg in C.groups(c):
        tag = f"stage2 {name} group {g}"
        sl = slice(b0, b0 + Bg)
        w = Work(eng, c).set(QR, q[sl]).flush()
        lg = logits_buf(c, 0)
        stage(eng, 2, layer, g, name, kv, lg)
        got = w.read()
        C.check(tag + " ao", f32(got[AO][:Bg * c.L]), Ra[sl], Ta[sl], ulp=False)
        w.same(got, tag, {AO: (0, Bg * c.L)})
        assert torch.equal(bits(kv), bits(before)), tag + ": the KV slab changed"


# ---------------------------------------------------------------- stage 3, 4, 5
def _res_norm(eng, name, plan, st, layer, src, what, ref, norm_w):
    cfg, P = C.model()
    c = C.CASES[name]
    (Rh, Rn), (Th, Tn) = ref
    kv = nan_slab(eng)
    before = kv.clone()
    with forced(eng, PLANS[plan]):
        for g, b0, Bg in C.groups(c):
            tag = f"stage{st} {name} {plan} layer {layer} group {g}"
            sl, own = slice(b0, b0 + Bg), (b0 * c.L, (b0 + Bg) * c.L)
            w = Work(eng, c).set(src, C.rows(name, what)[sl]).set(HS, C.rows(name, "hs")).flush()
            lg = logits_buf(c, 0)
            stage(eng, st, layer, g, name, kv, lg)
            got = w.read()
            hs, tn = f32(got[HS][own[0]:own[1]]), f32(got[TN][own[0]:own[1]])
            C.check(tag + " hs", hs, Rh[sl], Th[sl])
            C.check(tag + " tn", tn, Rn[sl], Tn[sl], bias=False)
            C.check_norm(tag + " tn", tn, O.rms_norm(hs, P[norm_w], R.dims(cfg)["eps"]))
            w.same(got, tag, {HS: own, TN: own})
            assert torch.equal(bits(kv), bits(before))


@pytest.mark.parametrize("name,plan", RUNS, ids=run_ids(RUNS))
def test_stage3_o_proj_residual_norm(eng, name, plan):
    layer = C.LAYER[3]
    _res_norm(eng, name, plan, 3, layer, AO, "ao", C.stage3_ref(name),
              f"language_model.model.layers.{layer}.post_attention_layernorm.weight")


@pytest.mark.parametrize("name,plan", RUNS, ids=run_ids(RUNS))
def test_stage4_gate_up_geglu(eng, name, plan):
    c = C.CASES[name]
    layer = C.LAYER[4]
    Ra, Ta = C.stage4_ref(name)
    kv = nan_slab(eng)
    with forced(eng, PLANS[plan]):
        for g, b0, Bg in C.groups(c):
            tag = f"stage4 {name} {plan} group {g}"
            w = Work(eng, c).set(TN, C.rows(name, "tn")).flush()
            lg = logits_buf(c, 0)
            stage(eng, 4, layer, g, name, kv, lg)
            got = w.read()
            C.check(tag + " act", f32(got[ACT][:Bg * c.L]), Ra[b0:b0 + Bg], Ta[b0:b0 + Bg])
            w.same(got, tag, {ACT: (0, Bg * c.L)})


# (case A, the only 288-row case, runs layer 0 alone: the final norm of layer 1 is the same kernel on every other case)
RUNS5 = [(n, p, layer) for n, p in RUNS for layer in (0, 1) if (n, layer) != ("A", 1)]


@pytest.mark.parametrize("name,plan,layer", RUNS5, ids=[f"{n}{'-' + p if p else ''}-layer{ly}" for n, p, ly in RUNS5])
def test_stage5_down_residual_norm(eng, name, plan, layer):
    nxt = "language_model.model.layers.1.input_layernorm.weight" if layer == 0 else "language_model.model.norm.weight"
    _res_norm(eng, name, plan, 5, layer, ACT, "act", C.stage5_ref(name, layer), nxt)


# ---------------------------------------------------------------- stage 6
@pytest.mark.parametrize("name", C.STAGE_CASES)
def test_stage6_logits_of_every_row(eng, name):
    c = C.CASES[name]
    (Rl, _), (Tl, _) = C.stage6_ref(name, 0)
    kv = nan_slab(eng)
    for g, b0, Bg in C.groups(c):
        tag = f"stage6 {name} logits_rows 0 group {g}"
        w = Work(eng, c).set(TN, C.rows(name, "tn")).flush()
        lg = logits_buf(c, 0)
        stage(eng, 6, 0, g, name, kv, lg, logits_rows=0)
        got = w.read()
        own = slice(b0 * c.L, (b0 + Bg) * c.L)
        C.check(tag, lg[own].cpu().numpy(), Rl[b0:b0 + Bg], Tl[b0:b0 + Bg], ulp=False, bias=True)
        lg[own] = SENT
        assert bool((lg == SENT).all()), tag + ": logits outside the group's rows changed"
        w.same(got, tag, {})


@pytest.mark.parametrize("name", C.STAGE_CASES)
def test_stage6_logits_of_the_last_rows(eng, name):
    c = C.CASES[name]
    (Rl, Rlast), (Tl, _) = C.stage6_ref(name, 1)
    kv = nan_slab(eng)
    for g, b0, Bg in C.groups(c):
        tag = f"stage6 {name} logits_rows 1 group {g}"
        w = Work(eng, c).set(HS, C.rows(name, "hs")).flush()
        lg = logits_buf(c, 1)
        stage(eng, 6, 0, g, name, kv, lg, logits_rows=1)
        got = w.read()
        own = slice(b0, b0 + Bg)
        # the copy (lock-step: slot L - 1) or the gather (ragged: slot lens[b] - 1), bit for bit
        assert np.array_equal(f32(got[LAST][own]), C.rows2(Rlast)[own]), tag + ": lastrows"
        C.check(tag, lg[own].cpu().numpy(), Rl[own], Tl[own], ulp=False, bias=True)
        lg[own] = SENT
        assert bool((lg == SENT).all()), tag + ": logits outside the group's rows changed"
        w.same(got, tag, {LAST: (b0, b0 + Bg)})


# ---------------------------------------------------------------- stage 7
@pytest.mark.parametrize("name", C.TAIL_CASES)
def test_stage7_last_row_tail(eng, name):
    """The last-row-only tail of logits_rows 2 and stage 6 on its rows; then, from the same inputs, the all-row
    stages 2 .. 5 and stage 6 of logits_rows 1: both logits meet the same conditions against the same R and T."""
    c = C.CASES[name]
    layer = C.LAYER[7]
    assert (c.kv_start + c.L <= C.KV_MAX) == (name[0] != "X")        # X: the branch past the config's max_kv
    (Rl, Ra, Rg), (Tl, Ta, Tg) = C.stage7_ref(name)
    q, fill = C.attn_inputs(name, layer)
    kv = nan_slab(eng, c.kv_max, fill)
    before = kv.clone()
    for g, b0, Bg in C.groups(c):
        tag = f"stage7 {name} group {g}"
        sl, own = slice(b0, b0 + Bg), (b0 * c.L, (b0 + Bg) * c.L)
        w = Work(eng, c).set(QR, q[sl]).set(HS, C.rows(name, "hs")).flush()
        lg = logits_buf(c, 2)
        stage(eng, 7, layer, g, name, kv, lg, logits_rows=2)
        got = w.read()
        C.check(tag + " lastrows", f32(got[LAST][sl]), Rl[sl], Tl[sl], ulp=False)
        w.same(got, tag, {LAST: (b0, b0 + Bg), DAO: (0, Bg)})
        if Bg >= 3 or name[0] == "X":        # the combined attention output is stored at B >= 3 and by the prefill kernel
            C.check(tag + " ao", f32(got[DAO][:Bg]), Ra[sl], Ta[sl], ulp=False)
        else:
            assert bool((got[DAO] == SENT).all())
        assert bool((lg == SENT).all())
        stage(eng, 6, 0, g, name, kv, lg, logits_rows=2)
        torch.cuda.synchronize()
        C.check(tag + " logits_rows 2", lg[sl].cpu().numpy(), Rg[sl], Tg[sl], ulp=False)
        lg[sl] = SENT
        assert bool((lg == SENT).all())
        # the all-row path on the same inputs
        w.flush()
        lg1 = logits_buf(c, 1)
        for st in (2, 3, 4, 5):
            stage(eng, st, layer, g, name, kv, lg1, logits_rows=1)
        stage(eng, 6, 0, g, name, kv, lg1, logits_rows=1)
        got = w.read()
        C.check(tag + " logits_rows 1", lg1[sl].cpu().numpy(), Rg[sl], Tg[sl], ulp=False)
        w.same(got, tag + " all rows", {HS: own, TN: own, AO: (0, Bg * c.L), ACT: (0, Bg * c.L), LAST: (b0, b0 + Bg)})
        assert torch.equal(bits(kv), bits(before)), tag + ": the KV slab changed"


# ---------------------------------------------------------------- the hook runs the production launch sequence
CHAIN = [(n, "", lr) for n in C.CHAIN_CASES for lr in (0, 1, 2)] + [("C", "table", 0), ("C", "split", 2)]


@pytest.mark.parametrize("name,plan,logits_rows", CHAIN, ids=[f"{n}{'-' + p if p else ''}-rows{lr}" for n, p, lr in CHAIN])
def test_chained_stages_equal_the_eager_prefill(eng, name, plan, logits_rows):
    c = C.CASES[name]
    ids_np, feats_np = C.ids_feats(name)
    ids, feats = torch.from_numpy(ids_np).to(DEV), bf(feats_np)
    kv0 = nan_slab(eng, c.kv_max, C.prior_kv(name)[:, :, :, :c.kv_start])
    with forced(eng, PLANS[plan]):
        kv_e = kv0.clone()
        lg_e = eng.lm_forward(kv_e, c.kv_start, c.pos, ids=ids, image_feats=feats, logits_rows=logits_rows, lens=c.lens)
        torch.cuda.synchronize()
        kv_s = kv0.clone()
        lg_s = torch.full_like(lg_e, SENT)
        # (a ragged call's logits_rows 2 is its logits_rows 1; L = 1 has no last-row-only form)
        tail = logits_rows == 2 and c.lens is None and c.L > 1
        kw = dict(logits_rows=logits_rows, ids=ids, feats=feats)
        stage(eng, 0, 0, 0, name, kv_s, lg_s, **kw)
        for g, _, _ in C.groups(c):
            for layer in (0, 1):
                stage(eng, 1, layer, g, name, kv_s, lg_s, **kw)
                for st in ((7,) if tail and layer == 1 else (2, 3, 4, 5)):
                    stage(eng, st, layer, g, name, kv_s, lg_s, **kw)
            stage(eng, 6, 0, g, name, kv_s, lg_s, **kw)
        torch.cuda.synchronize()
    assert torch.equal(bits(lg_s), bits(lg_e))
    assert torch.equal(bits(kv_s), bits(kv_e))
    assert bool(torch.isfinite(lg_e).all())
    # every slot of the call is written (finite), everything else is the slab as it was
    slots = slice(c.kv_start, c.kv_start + c.L)
    assert bool(torch.isfinite(kv_e[:, :, :c.B, slots].float()).all())
    back = kv_e.clone()
    back[:, :, :c.B, slots] = kv0[:, :, :c.B, slots]
    assert torch.equal(bits(back), bits(kv0))


# ---------------------------------------------------------------- argument checks
def test_argument_checks(eng):
    kv = nan_slab(eng)
    lg = torch.empty((9 * 8, C.V), dtype=torch.float32, device=DEV)
    ids = torch.full((9, 8), 5, dtype=torch.int64, device=DEV)
    ok = dict(kv=kv, kv_start=0, positions=np.arange(8)[None], logits=lg, ids=ids)
    eng.prefill_stage(1, 0, 1, **ok)      # (the arguments below are refused for the reason each names, not these)
    with pytest.raises(ValueError):       # neither ids nor embeds, as pgmi_lm_forward
        eng.prefill_stage(1, 0, 0, **dict(ok, ids=None, B=9, L=8))
    for st, layer, group in ((8, 0, 0), (-1, 0, 0), (1, 2, 0), (3, -1, 0), (1, 0, 2), (2, 0, -1), (7, 0, 0)):
        with pytest.raises(ValueError):
            eng.prefill_stage(st, layer, group, logits_rows=2, **ok)
    with pytest.raises(ValueError):       # stage 7 outside a logits_rows 2 call
        eng.prefill_stage(7, 1, 0, logits_rows=1, **ok)
    with pytest.raises(ValueError):       # what pgmi_lm_forward refuses: past the slab
        eng.prefill_stage(1, 0, 0, **dict(ok, kv_start=C.KV_MAX - 4))
    with pytest.raises(ValueError):       # a ragged length outside [1, L]
        eng.prefill_stage(1, 0, 0, lens=[8, 1, 5, 8, 3, 9, 2, 7, 4], **ok)
    with pytest.raises(ValueError):       # B over max_batch
        eng.prefill_stage(1, 0, 0, **dict(ok, ids=torch.full((17, 8), 5, dtype=torch.int64, device=DEV),
                                          logits=torch.empty((17 * 8, C.V), dtype=torch.float32, device=DEV)))
    n_all, n_g = C.MAX_BATCH * C.MAX_SEQ, C.GROUP * C.MAX_SEQ
    caps = {HS: n_all * C.H, TN: n_all * C.H, QKV: n_g * QKVN, QR: n_g * C.QD, AO: n_g * C.H, ACT: n_g * C.I,
            LAST: C.MAX_BATCH * C.H, DAO: C.MAX_BATCH * C.H}
    for which, cap in caps.items():
        eng.prefill_buffer(which, torch.empty(cap * 2, dtype=torch.uint8, device=DEV))           # the whole buffer
        with pytest.raises(ValueError):
            eng.prefill_buffer(which, torch.empty(cap * 2 + 2, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        eng.prefill_buffer(8, torch.empty(16, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
