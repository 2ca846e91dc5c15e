"""The batch-1/2 o_proj combines the flash-decoding partial records of the attention in its prologue.  It loads
twelve records unconditionally, the chunk index clamped to the buffer's chunk count (a kernel argument) rather than
to the live count (which comes from the step record, a load the partials would otherwise wait for), and uses a
record only below the live count.  So whatever the records at or past the live count hold must not reach h: stage 2
(attention + o_proj) with the whole partial buffer pre-filled with NaN bit patterns must give, bit for bit, the h it
gives with the buffer zeroed.  max_kv 768: twelve chunks of 64 keys, the combine's register form."""
import numpy as np
import pytest
import torch

import decode_stage_cases as C
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
KV_MAX, CHUNKS, PART = 768, 12, 16 * 256 + 32
NAN_BITS_F32 = 0x7FC00123
KV_LENS = (0, 63, 64, 767)                      # live chunks 1, 1, 2 and 12 of 12


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    cfg, _ = C.model()
    e = Engine(cfg, max_batch=2, max_seq=64, max_kv=KV_MAX)
    e.fill_synthetic(C.SEED, W.init_policy)
    e.prepare()
    return e


@pytest.fixture(scope="module")
def inputs(eng):
    g = torch.Generator().manual_seed(11)
    kv = (torch.randn(tuple(eng.new_kv(2, KV_MAX).shape), generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    q = torch.randn((2, C.QD), generator=g).to(torch.bfloat16).to(DEV)
    h = torch.randn((2, C.H), generator=g).to(torch.bfloat16).to(DEV)
    return kv, q, h


def _stage2(eng, inputs, B, lens, ragged, fill_bits):
    kv, q, h = inputs
    part = torch.full((2, CHUNKS, PART), fill_bits, dtype=torch.int32, device=DEV)
    eng.decode_partials(part, write=True)
    eng.decode_buffer(3, q.clone(), write=True)
    eng.decode_buffer(0, h.clone(), write=True)
    eng.decode_stage(2, 0, B, kv, lens, [n + 1 for n in lens], ragged=ragged)
    out = eng.decode_buffer(0, torch.empty((2, C.H), dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()
    return out[:B].clone()


def _check(eng, inputs, B, lens, ragged):
    zero = _stage2(eng, inputs, B, lens, ragged, 0)
    nan = _stage2(eng, inputs, B, lens, ragged, NAN_BITS_F32)
    assert torch.isfinite(zero.float()).all() and torch.isfinite(nan.float()).all()
    assert torch.equal(zero.view(torch.int16), nan.view(torch.int16))
    assert not torch.equal(zero, inputs[2][:B])   # the stage ran: h moved


@pytest.mark.parametrize("kv_len", KV_LENS)
def test_oproj_ignores_stale_partials_b1(eng, inputs, kv_len):
    _check(eng, inputs, 1, [kv_len], False)


@pytest.mark.parametrize("lens", [(0, 767), (63, 64), (64, 0), (767, 63)])
def test_oproj_ignores_stale_partials_ragged_b2(eng, inputs, lens):
    _check(eng, inputs, 2, list(lens), True)


def test_partial_buffer_bounds(eng):
    """the records are [max_batch][chunks][16 * 256 + 32] fp32: the whole buffer copies, a longer copy is refused"""
    eng.decode_partials(torch.empty((2, CHUNKS, PART), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        eng.decode_partials(torch.empty(2 * CHUNKS * PART + 1, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
