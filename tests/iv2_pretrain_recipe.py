"""The InternVideo2 MAE pre-training fixture (tests/golden/g27_iv2_pretrain.npz, written by tools/make_goldens_iv2_pretrain.py from the
real reference) and a torch restatement of the reference's forward
(other_models/InternVideo2_single_modality/models/internvideo2_pretrain_videomae.py: PretrainVideoMAEInternVideo2 with the unfused
encoder route and the decoder's plain attention).  No kernels, no GPU needed; any dtype, any device, autocast-capable.

The encoder blocks are those of tests/iv2_recipe.py (``block`` / ``rmsnorm``: the two places where the reference leaves the model's
dtype are restated there); the decoder block is VideoMAE's (modeling_finetune.py:137-166: LayerNorm, one qkv Linear, optional
gamma_1 / gamma_2).  Large tensors are recorded as digests, as tests/iv2_recipe.py describes; tests/test_iv2_pretrain_cpu.py holds
this restatement to every recorded value within ``iv2_recipe.REPRO_TOL``.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import iv2_recipe as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_iv2_pretrain.npz")

# the tiny configuration of the issue: N = 4 frames x 2 x 2 patches = 16 tokens, encoder and decoder head_dim 64.  ``norm_layer`` is
# partial(nn.LayerNorm, eps=1e-6), as the factory passes it: the builders add it (this table is data).
TINY = dict(img_size=28, patch_size=14, num_frames=4, tubelet_size=1, encoder_embed_dim=128, encoder_num_heads=2, encoder_depth=2,
            decoder_embed_dim=64, decoder_num_heads=1, decoder_depth=1, decoder_num_classes=588, mlp_ratio=4.0, drop_path_rate=0.0)
VARIANTS = OrderedDict([  # fixture (c): forward only
    ("sep_pos", dict(sep_pos_embed=True)),
    ("layerscale", dict(init_values=0.1)),
])
GRID = (4, 2, 2)  # (T, H, W) in tokens
N, NV = 16, 4
EPS = 1e-6
REPRO_TOL = R.REPRO_TOL


def clip(seed=2):
    return torch.randn(2, 3, 4, 28, 28, generator=torch.Generator().manual_seed(seed))


def mask():
    """tube masks [2, 16] (True = masked): clip b keeps spatial cell KEEP[b] of the four in every frame -- Nv = 4, Nm = 12, and the two
    clips see different tokens"""
    m = torch.ones(2, GRID[0], GRID[1] * GRID[2], dtype=torch.bool)
    for b, cell in enumerate((1, 2)):
        m[b, :, cell] = False
    return m.flatten(1)


def target(seed=4):
    return torch.randn(2, N - NV, 588, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- the restatement
def vit_block(P, pre, x, H):
    """modeling_finetune.py:137-166 with the naive attention (:86-106)"""
    B, n, C = x.shape
    h = F.layer_norm(x, (C,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], EPS)
    bias = None
    if pre + "attn.q_bias" in P:
        bias = torch.cat((P[pre + "attn.q_bias"], torch.zeros_like(P[pre + "attn.v_bias"]), P[pre + "attn.v_bias"]))
    qkv = F.linear(h, P[pre + "attn.qkv.weight"], bias).reshape(B, n, 3, H, -1).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = ((q * (C // H) ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    a = F.linear((attn @ v).transpose(1, 2).reshape(B, n, -1), P[pre + "attn.proj.weight"], P[pre + "attn.proj.bias"])
    x = x + (P[pre + "gamma_1"] * a if pre + "gamma_1" in P else a)
    h = F.layer_norm(x, (C,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], EPS)
    m = F.linear(F.gelu(F.linear(h, P[pre + "mlp.fc1.weight"], P[pre + "mlp.fc1.bias"])), P[pre + "mlp.fc2.weight"], P[pre + "mlp.fc2.bias"])
    return x + (P[pre + "gamma_2"] * m if pre + "gamma_2" in P else m)


def decoder_table(n, d, dtype, device):
    """modeling_finetune.py:195-205: fp64 angles, cast to fp32 (a constant of the model), then to the run's dtype (``type_as(x)``)"""
    j = np.arange(d)
    t = np.arange(n, dtype=np.float64)[:, None] / np.power(10000, 2 * (j // 2) / d)[None, :]
    t[:, 0::2], t[:, 1::2] = np.sin(t[:, 0::2]), np.cos(t[:, 1::2])
    return torch.tensor(t, dtype=torch.float32).unsqueeze(0).to(device=device, dtype=dtype)


def model(P, x, m, cfg):
    """the [B, Nm, 588] prediction of configuration ``cfg`` (TINY plus a variant's overrides) with parameters P (state-dict keys)"""
    p, t = cfg["patch_size"], cfg["tubelet_size"]
    w = P["encoder.patch_embed.proj.weight"]
    x = F.conv3d(x.to(w.dtype), w, P["encoder.patch_embed.proj.bias"], stride=(t, p, p)).flatten(2).transpose(1, 2)
    B, n, C = x.shape
    if cfg.get("sep_pos_embed"):
        T, L = GRID[0], GRID[1] * GRID[2]
        pos = P["encoder.pos_embed_spatial"].repeat(1, T, 1) + torch.repeat_interleave(P["encoder.pos_embed_temporal"], L, dim=1)
    else:
        pos = P["encoder.pos_embed"]
    x = x + pos
    m = m.to(x.device)
    xv = x[~m].reshape(B, -1, C)
    for i in range(cfg["encoder_depth"]):
        xv = R.block(P, f"encoder.blocks.{i}.", xv, cfg["encoder_num_heads"], True)
    xv = F.layer_norm(xv, (C,), P["encoder.norm.weight"], P["encoder.norm.bias"], EPS)
    xv = F.linear(xv, P["encoder_to_decoder.weight"])
    Cd = xv.shape[-1]
    table = decoder_table(n, Cd, x.dtype, x.device).expand(B, -1, -1)
    pv, pm = table[~m].reshape(B, -1, Cd), table[m].reshape(B, -1, Cd)
    full = torch.cat([xv + pv, P["mask_token"] + pm], dim=1)
    for i in range(cfg["decoder_depth"]):
        full = vit_block(P, f"decoder.blocks.{i}.", full, cfg["decoder_num_heads"])
    out = full[:, -pm.shape[1]:]
    out = F.layer_norm(out, (Cd,), P["decoder.norm.weight"], P["decoder.norm.bias"], EPS)
    return F.linear(out, P["decoder.head.weight"], P["decoder.head.bias"])


def model_loss_and_grads(P, x, m, y, cfg, autocast=None, scale=1.0):
    """prediction, MSE loss against y, {key: gradient of scale * loss}; autocast = a 16-bit dtype runs the forward under torch.autocast"""
    if autocast is None:
        out = model(P, x, m, cfg)
    else:
        with torch.autocast(device_type=x.device.type, dtype=autocast):
            out = model(P, x, m, cfg)
    loss = F.mse_loss(out.float() if autocast is not None else out, y)
    grads = torch.autograd.grad(loss * scale, list(P.values()))
    return out.detach(), loss.detach(), OrderedDict(zip(P, grads))


def load():
    return np.load(GOLDEN, allow_pickle=False)
