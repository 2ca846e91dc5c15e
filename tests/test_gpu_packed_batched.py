"""Batched decode (3..16 rows) on the fragment-major 13-bit weight images (pgmi_set_decode_packed_batched): every
output -- act, h, logits, picked tokens, KV rows -- is bit for bit what the bf16 launches give, on the 2-text-layer
full-width config with a vocabulary of 1,000 (lm_head's last 16-row group holds 8 rows).

No test here runs a prefill: KV rows [0, L0) come from a seeded generator, the rest is zero, the ids are random, and
the steps start at kv_len = L0 -- the decode path alone."""
import numpy as np
import pytest
import torch

from oracle import weights as W
from pgmi import packed as P

pytestmark = pytest.mark.gpu
SEED, V, L0, KV, STEPS, MAXB = 1234, 1000, 8, 32, 4, 16
H, I = 2048, 16384
DOWN1 = "language_model.model.layers.1.mlp.down_proj.weight"
DOWN0 = "language_model.model.layers.0.mlp.down_proj.weight"
GATE0 = "language_model.model.layers.0.mlp.gate_proj.weight"
MASKS = (7, 1, 2, 4, 0)
FULL_BYTES = (2 * 3 * I * H + ((V + 15) // 16 * 16) * H) * 13 // 8


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    e = Engine(W.small_config(vision_layers=1, text_layers=2, vocab=V), max_batch=MAXB, max_seq=64, max_kv=KV)
    e.fill_synthetic(SEED, W.init_policy)
    e.prepare()
    return e


_inputs = {}


def _start(eng, B):
    """(kv, ids) every run of B rows starts from: computed once, cloned by the runs."""
    if B not in _inputs:
        g = torch.Generator().manual_seed(100 + B)
        kv = torch.zeros(eng.new_kv(B, KV).shape, dtype=torch.bfloat16)
        kv[:, :, :, :L0] = (torch.randn(kv[:, :, :, :L0].shape, generator=g) * 0.5).to(torch.bfloat16)
        ids = torch.randint(3, V - 64, (B,), generator=g)
        _inputs[B] = (kv.cuda(), ids.cuda())
    kv, ids = _inputs[B]
    return kv.clone(), ids.clone()


RAGGED_LENS = [int(x) for x in np.random.default_rng(5).permutation(np.arange(1, 25))[:16]]


def _run(eng, B, mode, mask):
    """Decode steps from the seeded KV: (logits of every step, tokens, the whole KV slab, rows the last step wrote)."""
    eng.set_decode_packed_batched(mask)
    kv, ids = _start(eng, B)
    out = []
    toks = torch.zeros((STEPS, B), dtype=torch.int64, device=ids.device)
    logits = torch.empty((B, V), dtype=torch.float32, device=ids.device)
    last = [L0 + STEPS - 1] * B
    if mode in ("eager", "graph"):
        for t in range(STEPS):   # graph: step 1 eager, step 2 captured, steps 3-4 replayed (in-place feedback)
            eng.decode(ids, kv, L0 + t, L0 + t, logits=logits, next_ids=ids, graph=mode == "graph")
            out.append(logits.clone())
            toks[t] = ids
    elif mode in ("steps", "steps_graph"):
        kv0, ids0 = kv.clone(), ids.clone()
        for rep in range(3 if mode == "steps_graph" else 1):   # eager, captured, replayed
            kv.copy_(kv0)
            ids.copy_(ids0)
            out.append(eng.decode_steps(ids, kv, L0, L0, STEPS, logits=logits, tokens=toks,
                                        graph=mode == "steps_graph").clone())
    else:   # ragged: sixteen different lengths, two steps fed back in place
        assert B == 16 and len(set(RAGGED_LENS)) == 16 and min(RAGGED_LENS) >= 1 and max(RAGGED_LENS) <= 24
        out.append(eng.decode_ragged(ids, kv, RAGGED_LENS, RAGGED_LENS, n_steps=2, logits=logits, tokens=toks).clone())
        last = [n + 1 for n in RAGGED_LENS]
    torch.cuda.synchronize()
    wrote = all(bool(kv[:, :, b, last[b]].any()) for b in range(B))
    return out, toks.clone(), kv.clone(), wrote


def _same(a, b):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])
    assert a[3] and b[3]   # the last step's KV rows were written


def _fresh(*shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("B", [3, 8, 9, 16])
@pytest.mark.parametrize("staged", [0, 1])
def test_single_kernels(eng, B, staged):
    """pgmi_decode_kernel 2 (gate|up), 3 (down) and 4 (lm_head) write the same act / h / logits packed and raw: the
    smallest MFMA batch, the 8-row staging form's last row, the first batch on the 5-deep ring and 16-row staging,
    the full tile."""
    h = _fresh(B, H, seed=11, scale=0.5)
    act = _fresh(B, I, seed=12, scale=0.25)
    got = {}
    eng.set_decode_staged_norm(staged)
    try:
        for mask in (P.ALL_KINDS, 0):
            eng.set_decode_packed_batched(mask)
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
            got[mask] = res
            info = eng.decode_packed_batched_info()
            assert info["packed"] == (5 if mask else 0) and info["scanned"] == P.ALL_KINDS
    finally:
        eng.set_decode_staged_norm(-1)
    for a, b in zip(got[P.ALL_KINDS], got[0]):
        assert torch.equal(a, b) and bool(a.float().abs().sum() > 0)
    assert not torch.equal(got[0][1], h)   # down did add to h


@pytest.mark.parametrize("B,mode,staged", [
    (3, "eager", 0), (16, "eager", 0), (3, "graph", 0), (16, "graph", 0), (3, "steps", 0), (16, "steps", 0),
    (3, "steps_graph", 0), (16, "steps_graph", 0), (16, "ragged", 0),
    (3, "eager", 1), (16, "graph", 1)])   # and the step whose projections stage and normalise their rows themselves
def test_whole_step_equals_raw_under_every_mask(eng, B, mode, staged):
    eng.set_decode_staged_norm(staged)
    try:
        runs = [_run(eng, B, mode, m) for m in MASKS]
    finally:
        eng.set_decode_staged_norm(-1)
    for r in runs[:-1]:
        _same(r, runs[-1])
    assert bool(runs[-1][0][-1].abs().sum() > 0)


def test_the_packed_path_is_what_ran(eng):
    before = eng.decode_packed_info()
    _run(eng, 3, "eager", P.ALL_KINDS)
    info = eng.decode_packed_batched_info()
    assert info["mask"] == P.ALL_KINDS and info["scanned"] == P.ALL_KINDS
    assert (info["packed"], info["raw"]) == (2 * 2 + 1, 0) and not info["alloc_failed"]
    assert info["packed_bytes"] == FULL_BYTES == P.image_bytes_mf(2 * I, H) * 2 + P.image_bytes_mf(H, I) * 2 + \
        P.image_bytes_mf(V, H)
    assert all(eng.decode_packed_batched_tensor(k, l) for k in (1, 2) for l in (0, 1))
    assert eng.decode_packed_batched_tensor(4)
    eng.set_decode_packed_batched(2)
    info = eng.decode_packed_batched_info()
    assert (info["mask"], info["packed"], info["raw"]) == (2, 2, 3)
    assert not eng.decode_packed_batched_tensor(1, 0) and eng.decode_packed_batched_tensor(2, 1)
    eng.set_decode_packed_batched(0)
    info = eng.decode_packed_batched_info()
    assert (info["mask"], info["packed"], info["raw"], info["packed_bytes"]) == (0, 0, 5, 0)
    assert eng.decode_packed_info() == before   # the B <= 2 state is not touched by any of this


def test_a_tensor_that_does_not_fit(eng):
    w = eng.views[DOWN1]
    keep = w.clone()
    bits = w.view(torch.int16)
    e_hi = int(((bits.int() >> 7) & 0xFF).max())
    try:
        bits[1000, 7777] = (e_hi - 31) << 7   # one element one binade too low: this tensor alone stays bf16
        eng.prepare()
        assert eng.decode_packed_batched_info()["scanned"] == 0
        for B in (3, 16):
            _same(_run(eng, B, "eager", P.ALL_KINDS), _run(eng, B, "eager", 0))
        eng.set_decode_packed_batched(P.ALL_KINDS)
        info = eng.decode_packed_batched_info()
        assert (info["packed"], info["raw"]) == (4, 1) and not info["alloc_failed"]
        assert info["packed_bytes"] == FULL_BYTES - P.image_bytes_mf(H, I)
        assert not eng.decode_packed_batched_tensor(2, 1)
        assert eng.decode_packed_batched_tensor(2, 0) and eng.decode_packed_batched_tensor(4)
        assert all(eng.decode_packed_batched_tensor(1, l) for l in (0, 1))
    finally:
        w.copy_(keep)
        eng.prepare()


def test_weights_change_under_it(eng):
    before = _run(eng, 3, "eager", P.ALL_KINDS)
    _same(before, _run(eng, 3, "eager", 0))
    w = eng.views[DOWN0]
    try:
        w.mul_(2)          # exact in bf16: every exponent field, and e_hi, one higher
        eng.prepare()
        eng.set_decode_packed_batched(P.ALL_KINDS)
        assert eng.decode_packed_batched_info()["scanned"] == 0 and eng.decode_packed_batched_info()["packed"] == 0
        after = _run(eng, 3, "eager", P.ALL_KINDS)
        info = eng.decode_packed_batched_info()
        assert info["scanned"] == P.ALL_KINDS and info["packed"] == 5
        _same(after, _run(eng, 3, "eager", 0))
        _same(_run(eng, 3, "graph", P.ALL_KINDS), _run(eng, 3, "graph", 0))
        assert not torch.equal(after[0][-1], before[0][-1])
    finally:
        w.mul_(0.5)
        eng.prepare()
    _same(_run(eng, 3, "eager", P.ALL_KINDS), before)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("small", [-1, 0])
def test_batch_1_and_2_are_untouched(eng, B, small):
    eng.set_decode_packed(small)
    try:
        res = {}
        for mask in (P.ALL_KINDS, 0):
            eng.set_decode_packed_batched(mask)
            kv, ids = _start(eng, B)
            lg = eng.decode(ids, kv, L0, L0, graph=False).clone()
            torch.cuda.synchronize()
            res[mask] = (lg, kv)
            assert eng.decode_packed_info()["mask"] == (P.ALL_KINDS if small < 0 else 0)
        assert torch.equal(res[7][0], res[0][0]) and torch.equal(res[7][1], res[0][1])
        assert bool(res[0][0].abs().sum() > 0) and bool(res[0][1][:, :, :, L0].any())
    finally:
        eng.set_decode_packed(-1)
        eng.set_decode_packed_batched(0)


def test_a_switch_while_graphs_exist(eng):
    """A captured B = 3 step holds the bf16 launches: the setter drops it (and the other batched keys, nothing
    else), so the next call with the same buffers runs the packed launches eagerly -- the same bits."""
    count = lambda: eng.lib.pgmi_graph_count(eng.ctx, 1)
    eng.set_decode_packed_batched(0)
    eng.set_decode_staged_norm(-1)   # (drops every decode key: the counts below start from an empty cache)
    assert count() == 0
    kv3, ids3 = _start(eng, 3)
    want = eng.decode(ids3, kv3.clone(), L0, L0, graph=False).clone()   # the eager mask-0 result
    kv1, ids1 = _start(eng, 1)
    lg1 = torch.empty((1, V), dtype=torch.float32, device="cuda")
    n0 = count()
    for _ in range(2):   # a B = 1 key: seen, then captured
        eng.decode(ids1, kv1, L0, L0, logits=lg1, graph=True)
    n1 = count()
    assert n1 == n0 + 1
    logits = torch.empty((3, V), dtype=torch.float32, device="cuda")
    kv0 = kv3.clone()
    for _ in range(2):   # the B = 3 key: seen, then captured, with the mask at 0
        kv3.copy_(kv0)
        eng.decode(ids3, kv3, L0, L0, logits=logits, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(logits, want) and count() == n1 + 1
    eng.set_decode_packed_batched(P.ALL_KINDS)
    assert count() == n1    # the batched key is gone, the B = 1 key is still there
    kv3.copy_(kv0)
    eng.decode(ids3, kv3, L0, L0, logits=logits, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(logits, want)
    assert eng.decode_packed_batched_info()["packed"] == 5
    eng.set_decode_packed_batched(0)
    assert count() == n1


def test_lora_switch_on_gate_proj(eng):
    """An adapter on layer 0's gate_proj switched on and off at B = 3 with every kind packed: the image is rebuilt
    from the merged weights, then from the base again."""
    # delta = B . A doubles column 5 of the weight exactly (every row changes, every exponent there one higher)
    A = np.zeros((1, H), np.float32)
    A[0, 5] = 1
    Bf = eng.views[GATE0][:, 5:6].float().cpu().numpy()
    base = _run(eng, 3, "graph", P.ALL_KINDS)
    _same(base, _run(eng, 3, "graph", 0))
    eng.load_lora({GATE0: (A, Bf, 1.0)}, "gate")
    try:
        eng.set_lora("gate")
        eng.set_decode_packed_batched(P.ALL_KINDS)
        assert eng.decode_packed_batched_info()["scanned"] == P.ALL_KINDS & ~P.KINDS["gate_up"]
        on = _run(eng, 3, "graph", P.ALL_KINDS)
        assert eng.decode_packed_batched_info()["packed"] == 5
        _same(on, _run(eng, 3, "graph", 0))
        assert not torch.equal(on[0][-1], base[0][-1])
        eng.set_lora(None)
        off = _run(eng, 3, "graph", P.ALL_KINDS)
        _same(off, _run(eng, 3, "graph", 0))
        _same(off, base)
    finally:
        eng.set_lora(None)
        eng.unload_lora("gate")
        eng.set_decode_packed_batched(0)
