"""The kernels' in-register cross-lane reductions (csrc/common.h: permlane swaps and DPP moves instead of LDS
permutes) against the numpy fp32 emulation of each site's xor butterfly (lane_reduce_cases.xor_tree), bit for bit
in every lane of every row.  pgmi_debug_lane_reduce runs one wave per row, four rows per workgroup: 1,024 random
rows make 256 workgroups, the 12 special rows (infinities, -0.0, denormals, equal maxima) three -- the smallest
grid in which a wave or row index mix-up shows -- and three rows one partly filled workgroup.
tests/test_cpu_lane_reduce.py shows that these rows tell the trees apart."""
import numpy as np
import pytest
import torch

import lane_reduce_cases as L
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from pgmi import Engine
    return Engine(W.small_config(vision_layers=1, text_layers=1, vocab=1024), max_batch=1, max_seq=64, max_kv=64)


@pytest.fixture(scope="module")
def rows():
    rnd, sp = L.random_rows(), L.special_rows()
    return {"grid256": rnd, "grid3": sp, "grid1": np.ascontiguousarray(np.concatenate([sp[9:11], rnd[:1]]))}


@pytest.fixture(scope="module")
def want(rows):
    return {(g, op): L.xor_tree(x, *L.OPS[op]) for g, x in rows.items() for op in L.OPS}


@pytest.mark.parametrize("grid", ["grid1", "grid3", "grid256"])
@pytest.mark.parametrize("op", sorted(L.OPS))
def test_lane_reduce_bits(eng, rows, want, grid, op):
    x = rows[grid]
    assert (x.shape[0] + 3) // 4 == int(grid[4:])
    got = eng.lane_reduce(op, torch.from_numpy(x).to(DEV))
    torch.cuda.synchronize()
    kind = L.OPS[op][0]
    if kind == "first_max":
        wv, wi = want[grid, op]
        gv, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
        bad = np.argwhere((L.bits(gv) != L.bits(wv)) | (gi != wi))
        assert bad.size == 0, f"op {op}: first (row, lane) {bad[0]}: got ({gv[tuple(bad[0])]}, {gi[tuple(bad[0])]}), " \
                              f"want ({wv[tuple(bad[0])]}, {wi[tuple(bad[0])]})"
        # the lowest index among the equal maxima of the lanes reduced over
        span = 64 if L.OPS[op][1] == L.DESC else 16
        seg = x.reshape(x.shape[0], 64 // span, span)
        first = (np.argmax(seg, axis=2) + np.arange(64 // span) * span).repeat(span, axis=1)
        assert np.array_equal(gi, first)
    else:
        g = got.cpu().numpy()
        bad = np.argwhere(L.bits(g) != L.bits(want[grid, op]))
        assert bad.size == 0, f"op {op}: {len(bad)} lanes differ, first (row, lane) {bad[0]}: got " \
                              f"{g[tuple(bad[0])]!r}, want {want[grid, op][tuple(bad[0])]!r}"


def test_lane_reduce_refuses_bad_arguments(eng):
    from pgmi import _native as N
    x = torch.zeros((4, 64), dtype=torch.float32, device=DEV)
    out = torch.empty_like(x)
    s = N.stream_handle(x.device)
    for op, n in ((-1, 4), (8, 4), (0, 0)):
        assert eng.lib.pgmi_debug_lane_reduce(eng.ctx, op, x.data_ptr(), n, out.data_ptr(), s) != 0
