"""Torch restatements of the serving kernels (csrc/iv2_serve.hip), any dtype, any device.  tests/test_iv2_serve_cpu.py proves the two
entry restatements against ``cat`` + add and an explicit loop over the clips in fp64; the GPU tests compare the kernels with them."""
import torch


def entry_fwd(patch, cls, pos):
    """out[b, 0] = cls + pos[0]; out[b, 1 + n] = patch[b, n] + pos[1 + n]"""
    B, N, D = patch.shape
    out = torch.empty((B, N + 1, D), dtype=patch.dtype, device=patch.device)
    out[:, 0] = (cls.reshape(D) + pos[0]).expand(B, -1)
    out[:, 1:] = patch + pos[1:]
    return out


def entry_bwd(g):
    """(dpatch, dpos, dcls): the patch rows of g, and the sum over the clips in the order b = 0, 1, ... starting from g[0]"""
    acc = g[0].clone()
    for b in range(1, g.shape[0]):
        acc += g[b]
    return g[:, 1:].clone(), acc, acc[0].clone()


def residual(x, y, gamma=None):
    """x + y * gamma, the product and the sum each rounded on their own (torch never contracts them)"""
    return x + (y if gamma is None else y * gamma)


def rms(x, g, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g
