"""pgmi/ragged.py: row lengths of a padded batch from its attention mask (pure torch, no GPU)."""
import pytest
import torch

from pgmi import ragged as R


def test_all_ones_selects_lock_step():
    assert R.lengths_from_mask(None) is None
    assert R.lengths_from_mask(torch.ones(3, 7, dtype=torch.int64)) is None
    assert R.lengths_from_mask(torch.ones(1, 1, dtype=torch.bool)) is None


def test_right_padded_lengths():
    m = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0]])
    lens = R.lengths_from_mask(m)
    assert isinstance(lens, torch.Tensor) and lens.dtype == torch.int32
    assert lens.tolist() == [5, 2, 1]
    assert R.lengths_from_mask(m.bool()).tolist() == [5, 2, 1]
    assert R.lengths_from_mask(m.float()).tolist() == [5, 2, 1]


def test_left_padded_lengths_and_shift():
    m = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 0, 1]])
    lens, shift = R.lengths_from_mask(m)
    assert lens.dtype == torch.int32 and lens.tolist() == [5, 2, 1]
    assert shift.tolist() == [0, 3, 4]


@pytest.mark.parametrize("rows", [
    [[1, 0, 1, 1], [1, 1, 1, 1]],   # a hole
    [[1, 1, 1, 1], [0, 0, 0, 0]],   # an empty row
    [[1, 2, 0, 0], [1, 1, 1, 1]],   # not 0 / 1
    [[0, 1, 1, 0], [1, 1, 1, 1]],   # padded on both sides
])
def test_bad_masks_raise(rows):
    with pytest.raises(ValueError):
        R.lengths_from_mask(torch.tensor(rows))
    with pytest.raises(ValueError):
        R.right_pad(torch.zeros(2, 4, dtype=torch.int64), torch.tensor(rows))


def test_mask_shape_checked():
    with pytest.raises(ValueError):
        R.lengths_from_mask(torch.ones(4))
    with pytest.raises(ValueError):
        R.right_pad(torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, 5))


def test_right_pad_moves_left_padding():
    pad = 0
    left = torch.tensor([[11, 12, 13, 14, 15], [7, 7, 7, 21, 22], [7, 7, 7, 7, 31]])
    lmask = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 0, 1]])
    want = torch.tensor([[11, 12, 13, 14, 15], [21, 22, pad, pad, pad], [31, pad, pad, pad, pad]])
    got, lens = R.right_pad(left, lmask, pad_id=pad)
    assert torch.equal(got, want) and got.dtype == left.dtype
    assert lens.tolist() == [5, 2, 1] and lens.dtype == torch.int32
    # a right-padded batch passes through, its pad slots rewritten to pad_id
    right = torch.tensor([[11, 12, 13, 14, 15], [21, 22, 9, 9, 9], [31, 9, 9, 9, 9]])
    rmask = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0]])
    got2, lens2 = R.right_pad(right, rmask, pad_id=pad)
    assert torch.equal(got2, want) and lens2.tolist() == [5, 2, 1]
