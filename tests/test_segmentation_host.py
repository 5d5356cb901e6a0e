"""CPU tests of the host rules of occlusionenv_amd/segmentation.py: the one function that turns (pred, target) into what
the native criterion and metrics calls read, and the names ``ops`` and ``encoder`` hand on.  No GPU call is made here: the
tensors only claim to be on a device, and every check under test runs before anything native."""
import pytest
import torch

from occlusionenv_amd import _native as nat
from occlusionenv_amd import encoder, ops, segmentation

N, S = 2, 32


class FakeCuda(torch.Tensor):
    is_cuda = True


def _fake(*shape):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.rand(*shape, generator=g).as_subclass(FakeCuda)


def test_contiguous_pair_is_passed_through():
    pred, target = _fake(N, 1, S, S), _fake(N, S, S)
    p, t, k = segmentation._map_pair(pred, target)
    assert tuple(p.shape) == (N, S, S) and p.is_contiguous() and p.dtype == torch.float32
    assert p.data_ptr() == pred.data_ptr()
    assert k == 1 and isinstance(k, int) and t.data_ptr() == target.data_ptr()


def test_pixel_strided_target_is_read_in_place():
    fs = _fake(N, S, S, 4)
    target = fs[..., 3]
    p, t, k = segmentation._map_pair(_fake(N, S, S), target)
    assert k == 4 and t.data_ptr() == target.data_ptr() and tuple(t.shape) == (N, S, S)
    assert (t.stride(0), t.stride(1), t.stride(2)) == (4 * S * S, 4 * S, 4)


@pytest.mark.parametrize("name", ["transposed", "batch_strided"])
def test_other_layouts_are_copied(name):
    target = _fake(N, S, S).transpose(1, 2) if name == "transposed" else _fake(2 * N, S, S)[::2]
    assert not target.is_contiguous()
    p, t, k = segmentation._map_pair(_fake(N, S, S), target)
    assert k == 1 and t.is_contiguous() and t.data_ptr() != target.data_ptr()
    assert torch.equal(torch.Tensor(t), torch.Tensor(target))


def test_rejections_come_before_any_native_call():
    with pytest.raises(ValueError, match="above 1024"):
        segmentation._map_pair(_fake(1, 1025, 1025), _fake(1, 1025, 1025))
    with pytest.raises(ValueError, match="differ"):
        segmentation._map_pair(_fake(N, S, S), _fake(3, S, S))
    with pytest.raises(ValueError, match=r"target must be \(N,S,S\)"):
        segmentation._map_pair(_fake(N, S, S), _fake(N, S, S + 1))
    for pred, target in ((torch.rand(N, S, S), _fake(N, S, S)), (_fake(N, S, S), torch.rand(N, S, S))):
        with pytest.raises(nat.NativeError, match="there is no CPU fallback"):
            segmentation._map_pair(pred, target)
    # the public entry points reach the same function
    for fn in (segmentation.seg_counts, segmentation.seg_criterion, segmentation.binary_dice_loss,
               segmentation.binary_cross_entropy, segmentation.occlusion_metrics):
        with pytest.raises(nat.NativeError, match="there is no CPU fallback"):
            fn(torch.rand(N, S, S), torch.rand(N, S, S))
        with pytest.raises(ValueError, match="above 1024"):
            fn(_fake(1, 1025, 1025), _fake(1, 1025, 1025))


def test_ops_and_encoder_hand_on_the_same_functions():
    for name in ("seg_criterion", "dice_from_sums", "binary_dice_loss", "binary_cross_entropy"):
        assert getattr(ops, name) is getattr(segmentation, name), name
    assert encoder.seg_counts is segmentation.seg_counts


def test_call_helpers():
    assert nat.ptr(None) is None and nat.ptr(None, 8) is None
    t = torch.zeros(4)
    assert nat.ptr(t).value == t.data_ptr() and nat.ptr(t, 8).value == t.data_ptr() + 8
    assert list(nat.row_chunks(0, 3)) == [] and list(nat.row_chunks(3, 3)) == [(0, 3)]
    assert list(nat.row_chunks(7, 3)) == [(0, 3), (3, 3), (6, 1)]
