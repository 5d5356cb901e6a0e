"""Helpers shared by the GPU tests of the native training paths, tests/test_gpu_bn_train.py and the shared bodies of
tests/train_gpu_suite.py: guarded device buffers and the check of their guards, the f64 Dice and BCE losses, and a
module's gradients by key."""
import torch

GUARD = 4096


def guarded(nbytes):
    """-> (whole, lo): a u8 allocation filled with 0xA5 whose window [lo, lo + nbytes) is 256-byte aligned and has at least
    GUARD bytes in front of it and behind it."""
    whole = torch.full((nbytes + 2 * GUARD + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, lo


def guards_intact(bufs, sizes):
    """``bufs`` = {name: guarded(sizes[name])} after the native calls: no byte in front of a window or behind it was written."""
    for k, (whole, lo) in bufs.items():
        assert lo >= GUARD and whole.numel() - (lo + sizes[k]) >= GUARD
        assert bool((whole[:lo] == 0xA5).all()), f"bytes in front of {k} were written"
        assert bool((whole[lo + sizes[k]:] == 0xA5).all()), f"bytes behind {k} were written"


def dice64(p, t):
    p, t = p.reshape(p.shape[0], -1), t.reshape(t.shape[0], -1).double()
    return (1.0 - ((p * t).sum(1) + 1.0) / ((p * p).sum(1) + (t * t).sum(1) + 1.0)).mean()


def bce64(p, t):
    t = t.reshape(p.shape).double()
    return (-(t * torch.log(p).clamp_min(-100.0) + (1.0 - t) * torch.log(1.0 - p).clamp_min(-100.0))).mean()


def grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
