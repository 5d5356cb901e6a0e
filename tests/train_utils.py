"""Helpers shared by the GPU tests of the native training paths: tests/test_gpu_decoder_train.py, tests/test_gpu_bn_train.py
and, through the shared bodies of tests/train_gpu_suite.py, the dense and separable pairs
tests/test_gpu_encoder_train.py / test_gpu_sep_encoder_train.py and tests/test_gpu_fullnet_train.py /
test_gpu_sep_fullnet_train.py."""
import torch

GUARD = 4096


def guarded(nbytes):
    """-> (whole, lo): a u8 allocation filled with 0xA5 whose window [lo, lo + nbytes) is 256-byte aligned and has at least
    GUARD bytes in front of it and behind it."""
    whole = torch.full((nbytes + 2 * GUARD + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, lo


def dice64(p, t):
    p, t = p.reshape(p.shape[0], -1), t.reshape(t.shape[0], -1).double()
    return (1.0 - ((p * t).sum(1) + 1.0) / ((p * p).sum(1) + (t * t).sum(1) + 1.0)).mean()


def bce64(p, t):
    t = t.reshape(p.shape).double()
    return (-(t * torch.log(p).clamp_min(-100.0) + (1.0 - t) * torch.log(1.0 - p).clamp_min(-100.0))).mean()


def grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
