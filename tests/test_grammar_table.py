"""ops.grammar_table and ops._check_allow_table: the one conversion and the one shape check of a grammar's bit table, which the
sampler, the beam selection, the scorer and the three decode drivers share.  Host-side, so tested without a GPU."""
import numpy as np
import pytest
import torch

V = 337
W = (V + 31) // 32


def _table():
    return np.random.default_rng(3).integers(0, 2 ** 32, (V, W), dtype=np.uint64).astype(np.uint32)


def test_numpy_and_tensor_tables_give_the_same_int32_tensor():
    from musicgeneration_amd import ops
    t = _table()
    assert t.max() >= 2 ** 31                                                # bit 31 set somewhere: the view must not clip
    from_np = ops.grammar_table(t, "cpu")
    from_t = ops.grammar_table(torch.from_numpy(t.view(np.int32).copy()), "cpu")
    from_strided = ops.grammar_table(np.asfortranarray(t), "cpu")
    for got in (from_np, from_t, from_strided):
        assert got.dtype == torch.int32 and got.shape == (V, W) and got.is_contiguous()
        assert torch.equal(got, from_np)
        ops._check_allow_table(got, V)
    assert np.array_equal(from_np.numpy().view(np.uint32), t)                # bit for bit the table that went in
    assert ops.grammar_table(None, "cpu") is None
    ops._check_allow_table(None, V)


@pytest.mark.parametrize("shape", [(V - 1, W), (V, W + 1), (V, W - 1), (V * W,)])
def test_a_table_of_the_wrong_shape_is_refused(shape):
    from musicgeneration_amd import ops
    msg = r"allow_table must be a contiguous 32-bit integer tensor of shape \[V, ceil\(V/32\)\]"
    with pytest.raises(ValueError, match=msg):
        ops._check_allow_table(torch.zeros(shape, dtype=torch.int32), V)


def test_a_table_of_the_wrong_layout_is_refused():
    from musicgeneration_amd import ops
    msg = "allow_table must be a contiguous 32-bit integer tensor"
    with pytest.raises(ValueError, match=msg):
        ops._check_allow_table(torch.zeros(W, V, dtype=torch.int32).t(), V)  # the right shape, not contiguous
    with pytest.raises(ValueError, match=msg):
        ops._check_allow_table(torch.zeros(V, W, dtype=torch.int64), V)      # not 32-bit
