"""The emulation tests/test_gpu_lane_reduce.py compares the GPU against (lane_reduce_cases.xor_tree), and the check
that its rows can tell one reduction tree from another: if every order of the adds gave the same bits on these rows,
a kernel with the wrong tree would pass."""
import numpy as np

import lane_reduce_cases as L


def test_rows_tell_the_trees_apart():
    """On the 1,024 random rows the ascending butterfly and a sequential sum each differ from the kernels'
    descending butterfly (o = 32 .. 1) in at least half the rows."""
    x = L.random_rows()
    ref = L.xor_tree(x, "sum", L.DESC)
    assert (L.bits(ref) == L.bits(ref)[:, :1]).all()          # a full butterfly: one value in every lane
    asc = L.xor_tree(x, "sum", L.ASC)
    seq = L.sequential_sum(x)
    d_asc = float((L.bits(asc)[:, 0] != L.bits(ref)[:, 0]).mean())
    d_seq = float((L.bits(seq) != L.bits(ref)[:, 0]).mean())
    print(f"rows differing from the descending tree: ascending {d_asc:.3f}, sequential {d_seq:.3f}")
    assert d_asc >= 0.5 and d_seq >= 0.5


def test_rotate_form_is_the_xor_butterfly():
    """The o = 4 step of the in-register form reads lane (l - 4) mod 16 of its row (descending trees, after o = 8)
    or lane l ^ 7 (ascending trees, after o = 1 and 2) instead of lane l ^ 4: the same bits in every lane."""
    x = np.concatenate([L.random_rows(), L.special_rows()])
    lanes = L.LANES

    def tree(offsets, src4):
        v = x.copy()
        for o in offsets:
            src = src4 if o == 4 else lanes ^ o
            v = (v + v[:, src]).astype(np.float32)
        return v

    ror4 = (lanes & ~15) | ((lanes - 4) & 15)
    assert np.array_equal(L.bits(tree(L.DESC, ror4)), L.bits(L.xor_tree(x, "sum", L.DESC)))
    assert np.array_equal(L.bits(tree(L.ASC, lanes ^ 7)), L.bits(L.xor_tree(x, "sum", L.ASC)))
    assert np.array_equal(L.bits(tree(L.ROW16_ASC, lanes ^ 7)), L.bits(L.xor_tree(x, "sum", L.ROW16_ASC)))
    # and the order matters: the half mirror is not lane ^ 4 in a descending tree
    assert not np.array_equal(L.bits(tree(L.DESC, lanes ^ 7)), L.bits(L.xor_tree(x, "sum", L.DESC)))


def test_first_max_picks_the_lowest_index():
    x = L.special_rows()
    v, ix = L.xor_tree(x, "first_max", L.DESC)
    assert (ix == np.argmax(x, axis=1)[:, None]).all()         # numpy's argmax: the first maximum
    assert np.array_equal(L.bits(v), L.bits(np.broadcast_to(x.max(axis=1, keepdims=True), x.shape).copy()))
    assert ix[9, 0] == 5 and ix[11, 0] == 48 and ix[10, 0] == 0
    v16, i16 = L.xor_tree(x, "first_max", L.ROW16_ASC)
    for r in range(4):                                         # each 16-lane row on its own
        seg = x[:, 16 * r:16 * r + 16]
        assert (i16[:, 16 * r:16 * r + 16] == (np.argmax(seg, axis=1) + 16 * r)[:, None]).all()
