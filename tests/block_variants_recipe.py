"""Restatements for the fused Block variants (layer-scale, proj / MLP dropout): the branch dropout mask in numpy, the fp64 block that
applies it, and the error bounds the kernel tests use.  Nothing here imports the package's kernels."""
import numpy as np
import torch

from oracle import vit_oracle as O

U24 = 2.0 ** -24  # unit roundoff of f32


def hash32_np(a, b, seed):
    """csrc/common.h hash32 on uint64 arrays (built like oracle.attention_dropout_keep): 32 well-mixed bits of (a, b, seed)"""
    m32 = np.uint64(0xFFFFFFFF)
    x = (np.asarray(a, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.asarray(b, dtype=np.uint64) * np.uint64(0x85EBCA77)
         + np.uint64(int(seed) & 0xFFFFFFFF)) & m32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m32
    x ^= x >> np.uint64(16)
    return x


def branch_keep(M: int, D: int, p: float, seed: int) -> torch.Tensor:
    """keep mask [M,D] (bool) of proj / MLP dropout: element (m, c) is kept iff hash32(m, c, seed) >= p * 2^32.  p is the f32 value the
    kernel receives."""
    thr = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    row = np.arange(M, dtype=np.uint64).reshape(M, 1)
    col = np.arange(D, dtype=np.uint64).reshape(1, D)
    return torch.from_numpy(hash32_np(row, col, seed) >= thr)


def inv_keep_f32(p: float) -> float:
    """fl32(1 / (1 - p)) as the library computes it (common.h make_drop: f32 arithmetic on the f32 p)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def gamma_n(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u) for f32: the relative bound on a sum of n rounded operations in any order"""
    return n * U24 / (1.0 - n * U24)


def block_fp64(x, P, prefix, num_heads, eps=1e-6, keep_masks=None, keep_prob=1.0, drop_p=0.0, drop_seeds=(0, 0)):
    """oracle.block in fp64 with proj_drop / Mlp.drop added (modeling_finetune.py:104-105, 52-53, 159-166): each branch is
    x + drop_path(gamma * dropout(branch)), the dropout mask injected from branch_keep over the [B*N, D] rows of the branch output."""
    B, N, D = x.shape

    def drop(t, seed):
        if drop_p <= 0.0:
            return t
        keep = branch_keep(B * N, D, drop_p, seed).reshape(B, N, D).to(t.dtype)
        return t * keep / (1.0 - float(np.float32(drop_p)))

    a = O.attention(O.layer_norm(x, P[prefix + "norm1.weight"], P[prefix + "norm1.bias"], eps), P, prefix + "attn.", num_heads)
    a = drop(a, drop_seeds[0])
    if prefix + "gamma_1" in P:
        a = P[prefix + "gamma_1"] * a
    x = x + O.drop_path(a, keep_masks[0] if keep_masks else None, keep_prob)
    m = O.mlp(O.layer_norm(x, P[prefix + "norm2.weight"], P[prefix + "norm2.bias"], eps), P, prefix + "mlp.")
    m = drop(m, drop_seeds[1])
    if prefix + "gamma_2" in P:
        m = P[prefix + "gamma_2"] * m
    return x + O.drop_path(m, keep_masks[1] if keep_masks else None, keep_prob)


def branch_grads_by_formula(g, a, W, bias, gamma, s_rows, keep, inv_keep):
    """The backward algebra of one branch y = res + s gamma keep inv_keep (a W^T + bias) from its inputs alone (all fp64):
    gb = s keep inv_keep g (no gamma);  d a = gb (diag(gamma) W);  T = gb^T a;  cs = colsum(gb);
    dW = gamma T;  dbias = gamma cs;  dgamma[n] = sum_k T[n,k] W[n,k] + bias[n] cs[n].  Returns (da, dW, dbias, dgamma)."""
    gb = g * s_rows[:, None] * keep * inv_keep
    da = gb @ (gamma[:, None] * W)
    T = gb.t() @ a
    cs = gb.sum(0)
    return da, gamma[:, None] * T, gamma * cs, (T * W).sum(1) + bias * cs
