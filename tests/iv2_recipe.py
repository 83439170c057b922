"""The InternVideo2 fixture (tests/golden/g26_internvideo2.npz, written by tools/make_goldens_internvideo2.py from the real reference) and
a torch restatement of the reference's forward (other_models/InternVideo2_single_modality/models/internvideo2.py, the unfused route:
use_flash_attn = use_fused_rmsnorm = use_fused_mlp = False).  No kernels, no GPU needed; any dtype, any device, autocast-capable.

The restatement follows the reference operator by operator, including the two places where the reference leaves the model's dtype: its
RMSNorm computes in float32 whatever comes in, and its LayerScale (force_fp32) multiplies in float32.  In a float64 run those two round
to 2^-24 relative, so "the fp64 golden" of this family carries that rounding; the restatement carries the same one, and
tests/test_iv2_cpu.py holds it to the recorded values within REPRO_TOL.

What the fixture holds.  The tiny model has 0.54 M parameters: its fp64 gradients alone are 4.3 MB, four times what a committed file may
weigh.  So the file records, per tensor, a DIGEST where the tensor is large (fp64: L2 norm, sum, 16 seeded Gaussian projections, the
first and last 32 elements -- ``digest``) and the whole fp64 tensor where it is small (<= WHOLE_MAX elements); parameters are recorded as
SHA-256 of their float32 bytes.  The CPU test proves that the restatement reproduces every digest and every whole tensor; the GPU tests
then take the full fp64 tensors from the restatement, which that proof makes the reference's own.
"""
import hashlib
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_internvideo2.npz")

# the tiny configuration of the issue: N = 2 frames x 2 x 2 patches + the class token = 9 tokens, head_dim 64
TINY = dict(embed_dim=128, num_heads=2, depth=2, mlp_ratio=4, attn_pool_num_heads=4, clip_embed_dim=64, patch_size=14, img_size=28,
            num_frames=2, tubelet_size=1, num_classes=2, init_values=0.1, drop_path_rate=0.0)
REF_ROUTE = dict(use_flash_attn=False, use_fused_rmsnorm=False, use_fused_mlp=False)  # arguments this package accepts and ignores
VARIANTS = OrderedDict([  # fixture (d): forward only
    ("plain_attn", dict(qkv_bias=True, qk_normalization=False, init_values=0)),
    ("sep_pos", dict(sep_pos_embed=True)),
])
BLOCK = dict(dim=128, num_heads=2, mlp_ratio=4, qkv_bias=False, init_values=0.1, qk_normalization=True)  # fixture (c), norm_layer = RMSNorm(eps 1e-6)
LABELS = (0, 1)
NOISE = 0.05
WHOLE_MAX = 2560
# fp64 rounding, except that one f32 rounding inside RMSNorm / LayerScale may fall the other way when its fp64 input differs in the last
# bit (2^-24 of one element): far below 1e-7 of a tensor's norm
REPRO_TOL = 1e-7


def clip(seed=2):
    return torch.randn(2, 3, 2, 28, 28, generator=torch.Generator().manual_seed(seed))


def block_input(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 9, 128, generator=g), torch.randn(2, 9, 128, generator=g)  # x, and the cotangent dy of loss = sum(y * dy)


def perturb_(named_params, seed=1):
    """seeded noise on every parameter, in iteration order: afterwards no gamma is 1 and no bias 0"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in named_params:
            p.add_(NOISE * torch.randn(p.shape, generator=g, dtype=torch.float32).to(p.dtype))


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().float().numpy()).tobytes()).hexdigest()


def digest(t, seed):
    """the record of a large tensor: fp64 [norm, sum, 16 projections on seeded Gaussian vectors, first 32, last 32]"""
    v = np.ascontiguousarray(t.detach().cpu().double().numpy()).reshape(-1)
    rng = np.random.default_rng(1000 + seed)
    proj = [float(v @ rng.standard_normal(v.size)) for _ in range(16)]
    return np.concatenate([[math.sqrt(float(v @ v)), float(v.sum())], proj, v[:32], v[-32:]])


def record(t, seed):
    t = t.detach().cpu().double()
    return t.numpy() if t.numel() <= WHOLE_MAX else digest(t, seed)


def matches(t, rec, seed):
    """deviation of tensor t from its record, relative to the record's norm (whole tensors: rel-L2; digests: the worst entry relative to
    the norm times the entry's natural scale -- a projection on a Gaussian vector has the scale of the norm itself)"""
    t = t.detach().cpu().double()
    if t.numel() <= WHOLE_MAX:
        ref = torch.as_tensor(rec).reshape(t.shape)
        return float((t - ref).norm() / ref.norm().clamp_min(1e-300))
    got = digest(t, seed)
    assert got.shape == rec.shape
    norm = max(float(rec[0]), 1e-300)
    scale = np.concatenate([[1.0, math.sqrt(t.numel())], np.ones(16 + 64)])
    return float(np.max(np.abs(got - rec) / (norm * scale)))


# ----------------------------------------------------------------------------- the restatement
def rmsnorm(x, w, eps=1e-6):
    dt = x.dtype
    h = x.to(torch.float32)
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return w * h.to(dt)


def layerscale(x, gamma):
    return (x.float() * gamma.float()).to(x.dtype)


def attention(P, pre, x, H, qk_norm):
    B, N, C = x.shape
    qkv = F.linear(x, P[pre + "qkv.weight"], P.get(pre + "qkv.bias")).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    if qk_norm:
        q = rmsnorm(q.transpose(1, 2).flatten(-2, -1), P[pre + "q_norm.weight"]).view(B, N, H, C // H).transpose(1, 2)
        k = rmsnorm(k.transpose(1, 2).flatten(-2, -1), P[pre + "k_norm.weight"]).view(B, N, H, C // H).transpose(1, 2)
    attn = ((q * (C // H) ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    x = (attn @ v).transpose(1, 2).reshape(B, N, C)
    return F.linear(x, P[pre + "proj.weight"], P[pre + "proj.bias"])


def mlp(P, pre, x):
    return F.linear(F.gelu(F.linear(x, P[pre + "fc1.weight"], P[pre + "fc1.bias"])), P[pre + "fc2.weight"], P[pre + "fc2.bias"])


def block(P, pre, x, H, qk_norm=True):
    a = attention(P, pre + "attn.", rmsnorm(x, P[pre + "norm1.weight"]), H, qk_norm)
    x = x + (layerscale(a, P[pre + "ls1.gamma"]) if pre + "ls1.gamma" in P else a)
    m = mlp(P, pre + "mlp.", rmsnorm(x, P[pre + "norm2.weight"]))
    return x + (layerscale(m, P[pre + "ls2.gamma"]) if pre + "ls2.gamma" in P else m)


def attention_pool(P, pre, x, H):
    B, N, C = x.shape
    ln = lambda t, n: F.layer_norm(t, (C,), P[pre + n + ".weight"], P[pre + n + ".bias"], 1e-5)
    x_q, x_k, x_v = ln(x.mean(1, keepdim=True) + 0, "norm1_q"), ln(x + 0, "norm1_k"), ln(x, "norm1_v")
    ca = pre + "cross_attn."
    heads = lambda t, n: F.linear(t, P[ca + n + ".weight"], P[ca + n + "_bias"]).reshape(B, t.shape[1], 1, H, -1).permute(2, 0, 3, 1, 4).squeeze(0)
    q, k, v = heads(x_q, "q"), heads(x_k, "k"), heads(x_v, "v")
    attn = ((q * (C // H) ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    x = (attn @ v).transpose(1, 2).reshape(B, 1, -1)
    return F.linear(x, P[ca + "proj.weight"], P[ca + "proj.bias"]).squeeze(1)


def model(P, x, cfg):
    """logits of the InternVideo2 configuration ``cfg`` (TINY plus a variant's overrides) with parameters P (state-dict keys)"""
    p, t = cfg["patch_size"], cfg["tubelet_size"]
    x = F.conv3d(x.to(P["patch_embed.proj.weight"].dtype), P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=(t, p, p))
    x = x.flatten(3).permute(0, 2, 3, 1)
    B, T, L, C = x.shape
    x = torch.cat((P["cls_token"].expand(B, -1, -1), x.reshape(B, T * L, C)), dim=1)
    if cfg.get("sep_pos_embed"):
        pos = P["pos_embed_spatial"].repeat(1, T, 1) + torch.repeat_interleave(P["pos_embed_temporal"], L, dim=1)
        pos = torch.cat([P["pos_embed_cls"].expand(pos.shape[0], -1, -1), pos], 1)
    else:
        pos = P["pos_embed"]
    x = x + pos
    for i in range(cfg["depth"]):
        x = block(P, f"blocks.{i}.", x, cfg["num_heads"], cfg.get("qk_normalization", True))
    x = attention_pool(P, "clip_projector.", x, cfg["attn_pool_num_heads"])
    x = F.layer_norm(x, (x.shape[-1],), P["fc_norm.weight"], P["fc_norm.bias"], 1e-5)
    return F.linear(x, P["head.weight"], P["head.bias"])


def leaves(named, dtype=None, device=None):
    """{key: detached leaf that requires grad} from (key, tensor) pairs"""
    return OrderedDict((k, v.detach().to(device=device, dtype=dtype).clone().requires_grad_()) for k, v in named)


def model_loss_and_grads(P, x, cfg, autocast=None):
    """logits, cross-entropy loss for LABELS, {key: gradient}; autocast = a 16-bit dtype runs the forward under torch.autocast"""
    labels = torch.tensor(LABELS, device=x.device)
    if autocast is None:
        logits = model(P, x, cfg)
    else:
        with torch.autocast(device_type=x.device.type, dtype=autocast):
            logits = model(P, x, cfg)
    loss = F.cross_entropy(logits.float() if autocast is not None else logits, labels)
    grads = torch.autograd.grad(loss, list(P.values()))
    return logits.detach(), loss.detach(), OrderedDict(zip(P, grads))


def block_loss_and_grads(P, x, dy, autocast=None):
    """y, {key: gradient} and dx for loss = sum(y * dy) of one Block with parameters P (keys without a prefix)"""
    x = x.detach().clone().requires_grad_()
    if autocast is None:
        y = block(P, "", x, BLOCK["num_heads"])
    else:
        with torch.autocast(device_type=x.device.type, dtype=autocast):
            y = block(P, "", x, BLOCK["num_heads"])
    grads = torch.autograd.grad((y.to(dy.dtype) * dy).sum(), [x, *P.values()])
    return y.detach(), grads[0], OrderedDict(zip(P, grads[1:]))


def load():
    return np.load(GOLDEN, allow_pickle=False)
