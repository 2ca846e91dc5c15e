"""Decode at batch 1-2 on the lossless 13-bit weight images (pgmi_set_decode_packed): every output -- logits,
picked tokens, KV rows -- is bit for bit what the bf16 kernels give, on the 2-text-layer full-width config with a
vocabulary of 1,000 (lm_head's row groups are 16 rows at B = 1: the last one is partial)."""
import pytest
import torch

from oracle import weights as W
from pgmi import packed as P

pytestmark = pytest.mark.gpu
SEED, V, L0, KV, STEPS = 1234, 1000, 8, 32, 4
DOWN1 = "language_model.model.layers.1.mlp.down_proj.weight"
DOWN0 = "language_model.model.layers.0.mlp.down_proj.weight"


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.small_config(vision_layers=1, text_layers=2, vocab=V), max_batch=2, max_seq=64, max_kv=KV)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    return e


def _prompt(B):
    g = torch.Generator().manual_seed(7)
    return torch.randint(3, V - 64, (B, L0), generator=g).cuda()


def _run(eng, B, mode, on):
    """A short prefill, then 4 decode steps; everything the steps produce."""
    eng.set_decode_packed(on)
    kv = torch.zeros_like(eng.new_kv(B, KV))
    lg0 = eng.lm_forward(kv, 0, torch.arange(L0)[None], ids=_prompt(B), logits_rows=2)[:, 0]
    ids = lg0.argmax(-1).contiguous()
    out = [lg0.clone()]
    toks = torch.zeros((STEPS, B), dtype=torch.int64, device=ids.device)
    if mode in ("eager", "graph"):
        logits = torch.empty((B, V), dtype=torch.float32, device=ids.device)
        for t in range(STEPS):   # graph: step 1 eager, step 2 captured, steps 3-4 replayed (in-place feedback)
            eng.decode(ids, kv, L0 + t, L0 + 1 + t, logits=logits, next_ids=ids, graph=mode == "graph")
            out.append(logits.clone())
            toks[t] = ids
    else:
        for rep in range(2 if mode == "steps_graph" else 1):   # the second call replays the captured four steps
            kv[:, :, :, L0:] = 0
            ids.copy_(lg0.argmax(-1))
            out.append(eng.decode_steps(ids, kv, L0, L0 + 1, STEPS, tokens=toks, graph=mode == "steps_graph").clone())
    torch.cuda.synchronize()
    return out, toks.clone(), kv.clone()


def _same(a, b):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])
    assert bool(a[2][:, :, :, L0 + STEPS - 1].any())   # the last step's KV rows were written


def _all_equal(eng, cases=((1, "eager"), (2, "eager"), (1, "graph"), (2, "steps_graph"))):
    runs = {}
    for B, mode in cases:
        runs[B, mode] = _run(eng, B, mode, P.ALL_KINDS)
        _same(runs[B, mode], _run(eng, B, mode, 0))
    eng.set_decode_packed(P.ALL_KINDS)   # what the queries that follow describe
    return runs


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", ["eager", "graph", "steps", "steps_graph"])
def test_packed_equals_raw(eng, B, mode):
    on = _run(eng, B, mode, P.ALL_KINDS)
    assert eng.decode_packed_info()["packed"] == 5   # the packed kernels did run
    _same(on, _run(eng, B, mode, 0))


@pytest.mark.parametrize("B", [1, 2])
def test_default_setting_equals_raw(eng, B):
    """The default (-1): every kind at B = 1, lm_head alone at B = 2."""
    _same(_run(eng, B, "graph", -1), _run(eng, B, "graph", 0))
    eng.set_decode_packed(-1)
    info = eng.decode_packed_info()
    assert (info["mask"], info["mask_b2"]) == (P.ALL_KINDS, P.KINDS["lm_head"])


def test_synthetic_weights_pack_fully(eng):
    _run(eng, 1, "eager", P.ALL_KINDS)
    info = eng.decode_packed_info()
    H, I = 2048, 16384
    assert info["mask"] == P.ALL_KINDS and info["scanned"] == P.ALL_KINDS
    assert (info["packed"], info["raw"]) == (2 * 2 + 1, 0) and not info["alloc_failed"] and not info["mf_alloc_failed"]
    assert info["packed_bytes"] == (2 * 3 * I * H + V * H) * 13 // 8 and info["raw_bytes"] == 0
    assert all(eng.decode_packed_tensor(k, l) for k in (1, 2) for l in (0, 1)) and eng.decode_packed_tensor(4)
    eng.set_decode_packed(0)
    info = eng.decode_packed_info()
    assert (info["packed"], info["raw"], info["packed_bytes"]) == (0, 5, 0)
    assert info["raw_bytes"] == (2 * 3 * I * H + V * H) * 2
    eng.set_decode_packed(-1)
    assert eng.decode_packed_info()["mask"] == P.ALL_KINDS   # the default


def test_crafted_down_proj(eng):
    w = eng.views[DOWN1]
    keep = w.clone()
    bits = w.view(torch.int16)
    e_hi = int(((bits.int() >> 7) & 0xFF).max())
    try:
        # +0, -0, denormals, and elements at e_hi and e_hi - 30, spread over lanes, chunks, segments and rows
        for (r, k), b in {(0, 0): 0x0000, (0, 1): 0x8000, (0, 9): 0x0001, (1, 513): 0x807F,
                          (2, 2047): e_hi << 7 | 0x7F, (3, 2048): 0x8000 | e_hi << 7,
                          (2047, 16383): (e_hi - 30) << 7, (5, 4100): 0x8000 | (e_hi - 30) << 7 | 0x7F}.items():
            bits[r, k] = b - 0x10000 if b >= 0x8000 else b
        eng.prepare()
        _all_equal(eng)
        info = eng.decode_packed_info()
        assert (info["packed"], info["raw"]) == (5, 0) and eng.decode_packed_tensor(2, 1)
        # one element one binade too low: this tensor alone keeps the bf16 kernel
        bits[1000, 7777] = (e_hi - 31) << 7
        eng.prepare()
        _all_equal(eng)
        info = eng.decode_packed_info()
        assert (info["packed"], info["raw"]) == (4, 1) and info["raw_bytes"] == 2048 * 16384 * 2
        assert not eng.decode_packed_tensor(2, 1)
        assert eng.decode_packed_tensor(2, 0) and eng.decode_packed_tensor(4)
        assert all(eng.decode_packed_tensor(1, l) for l in (0, 1))
    finally:
        w.copy_(keep)
        eng.prepare()


def test_in_place_update(eng):
    before = _all_equal(eng, ((1, "eager"),))[1, "eager"]
    w = eng.views[DOWN0]
    try:
        w.mul_(2)          # exact in bf16: every exponent field, and e_hi, one higher
        eng.prepare()
        after = _all_equal(eng, ((1, "eager"), (1, "graph")))[1, "eager"]
        assert eng.decode_packed_info()["packed"] == 5
        assert not torch.equal(after[0][-1], before[0][-1])
    finally:
        w.mul_(0.5)
        eng.prepare()
    _same(_run(eng, 1, "eager", P.ALL_KINDS), before)


@pytest.mark.parametrize("B", [1, 2])
def test_single_kernels(eng, B):
    """pgmi_decode_kernel 2 (gate|up), 3 (down) and 4 (lm_head) write the same act / h / logits packed and raw."""
    g = torch.Generator().manual_seed(11)
    h = (torch.randn((B, 2048), generator=g) * 0.5).to(torch.bfloat16).cuda()
    act = (torch.randn((B, 16384), generator=g) * 0.25).to(torch.bfloat16).cuda()
    got = {}
    for on in (P.ALL_KINDS, 0):
        eng.set_decode_packed(on)
        res = []
        for layer in (0, 1):
            eng.decode_buffer(0, h, write=True)
            eng.decode_kernel(2, layer, B)
            res.append(eng.decode_buffer(1, torch.empty_like(act)))
            eng.decode_buffer(1, act, write=True)
            eng.decode_buffer(0, h, write=True)
            eng.decode_kernel(3, layer, B)
            res.append(eng.decode_buffer(0, torch.empty_like(h)))
        eng.decode_buffer(0, h, write=True)
        eng.decode_kernel(4, 0, B)
        res.append(eng.decode_buffer(2, torch.empty((B, V), dtype=torch.float32, device=h.device)))
        torch.cuda.synchronize()
        got[on] = res
    assert eng.decode_packed_info()["scanned"] == P.ALL_KINDS
    for a, b in zip(got[P.ALL_KINDS], got[0]):
        assert torch.equal(a, b) and bool(a.float().abs().sum() > 0)
    assert not torch.equal(got[0][1], h)   # down did add to h


@pytest.mark.parametrize("B", [1, 2])
def test_prefill_graphs_follow_the_packed_images(eng, B):
    """A last-row-only prefill runs the decode GEMVs, which read the 13-bit images once they exist: the step that
    builds the images drops the prefill graphs with the small decode graphs, so the prefill key seen before runs
    eagerly again (packed), is captured and replayed -- and gives the same logits bit for bit, the image being
    lossless."""
    from pgmi import _native as N
    eng.set_decode_packed(P.ALL_KINDS)   # every kind at B = 2 as well (its default reads lm_head alone)
    eng.prepare()                        # no images, empty caches
    assert eng.decode_packed_info()["packed"] == 0
    ids = _prompt(B)
    pos = torch.arange(L0)[None].expand(B, L0).contiguous()
    kv = torch.zeros_like(eng.new_kv(B, KV))
    logits = torch.empty((B, 1, V), dtype=torch.float32, device="cuda")

    def prefill():
        N.check(eng.lib.pgmi_lm_forward(eng.ctx, ids.data_ptr(), None, 0, None, B, L0, pos.data_ptr(), kv.data_ptr(),
                                        B, kv.shape[3], 0, logits.data_ptr(), 2, eng._s()))
        torch.cuda.synchronize()

    prefill()
    first = logits.clone()
    assert eng.lib.pgmi_graph_count(eng.ctx, 0) == 1
    step_logits = torch.empty((B, V), dtype=torch.float32, device="cuda")
    eng.decode(first[:, 0].argmax(-1).contiguous(), kv, L0, L0 + 1, logits=step_logits, graph=False)
    assert eng.decode_packed_info()["packed"] == 5
    assert eng.lib.pgmi_graph_count(eng.ctx, 0) == 0
    for _ in range(3):   # eager, capture, replay
        prefill()
        assert torch.equal(logits, first)
    assert eng.lib.pgmi_graph_count(eng.ctx, 0) == 1
