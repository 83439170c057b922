"""The InternVideo2 family (other_models/InternVideo2_single_modality/models/internvideo2.py; fine-tuned by jobs/finetune/IV2-S_DoTA.sh)
behind the reference's operator surface: class names, constructor arguments, attribute tree, state-dict keys and shapes, factory names
and the initialisation sequence (the same ``torch.manual_seed`` gives the same weights, pinned by tests/golden/g26_internvideo2.npz).

One route instead of the reference's two: ``use_flash_attn``, ``use_fused_rmsnorm``, ``use_fused_mlp``, ``fused_mlp_heuristic`` and
``layerscale_no_force_fp32`` are accepted and select nothing.  A block is ``x + drop_path(ls(branch(norm(x))))`` with

    norm    ops.RMSNormFn (csrc/rmsnorm.hip), emitting the 16-bit operand of the Linear behind it
    attn    ops.IV2AttentionFn: qkv Linear -> f32, q / k RMS normalisation over the full H*d width (one kernel pass that also casts v and
            applies the attention kernels' q contract), the head_dim-64 attention kernels, proj
    mlp     ops.MlpFn

and, with gradients enabled, layer scale, drop path and the residual as torch element-wise ops on the f32 stream.  Without gradients the
blocks run as one loop in which each half block's layer scale, residual and the norm behind it are ONE launch (``_blocks_eval``;
csrc/iv2_serve.hip, ops.set_iv2_serve_kernels).  The class token's concatenation and the ``+ pos_embed`` are one kernel pass in every mode
(ops.ClassTokenEntryFn): the table is trainable here and receives its gradient, summed over the clips in a fixed order.  The entry takes
what modeling_finetune.PatchEmbed takes: float clips, clips in the 16-bit operand format, uint8 frames [B,T,H,W,3] (with a ring offset)
and frame_store.FrameWindows -- so inference.score_video / SlidingWindow, FrameStore and the engines serve this family as they serve
the ViT.  ``clip_projector`` (attention pooling with one
query per clip, head_dim 24 at the shipped sizes) is composed of MeanPoolFn, LayerNormFn, LinearSplitFn (split-operand GEMMs) and a torch softmax over [B, heads, N].

There is no CPU path, and no "precise" mode for this family.
"""
from __future__ import annotations

import math
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.utils.checkpoint as checkpoint

from . import ops
from ._lib import TadError
from .frame_store import FrameWindows
from .modeling_finetune import DropPath, to_2tuple, trunc_normal_
from .registry import register_model


# ----------------------------------------------------------------------------- sin-cos position tables (models/pos_embed.py)
# The reference computes the angles in float32 (float32 positions and frequencies, einsum, sin / cos) and only the final table is float64
# (a float64 row of zeros for the class token is concatenated in front); the dtypes are kept so that the tables match bit for bit.
def _sincos_1d(dim, pos):
    """[len(pos), dim]: sin of pos x omega in the first half of the columns, cos in the second; omega_i = 10000^(-2 i / dim)"""
    assert dim % 2 == 0
    omega = np.arange(dim // 2, dtype=np.float32)
    omega /= dim / 2.0
    omega = 1.0 / 10000 ** omega
    ang = np.einsum("m,d->md", np.asarray(pos).reshape(-1), omega)
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=1)


def _sincos_2d_grid(dim, size):
    """[size*size, dim] over a square grid, row-major (h, w): the first half of the columns encodes w, the second h (``np.meshgrid(w, h)``
    puts w first)"""
    assert dim % 2 == 0
    ax = np.arange(size, dtype=np.float32)
    gw, gh = np.meshgrid(ax, ax)
    return np.concatenate([_sincos_1d(dim // 2, gw), _sincos_1d(dim // 2, gh)], axis=1)


def _with_cls(table, cls_token):
    return np.concatenate([np.zeros([1, table.shape[1]]), table], axis=0) if cls_token else table


def get_2d_sincos_pos_embed(embed_dim, grid_size, cls_token=False):
    return _with_cls(_sincos_2d_grid(embed_dim, grid_size), cls_token)


def get_1d_sincos_pos_embed(embed_dim, t_size, cls_token=False):
    return _with_cls(_sincos_1d(embed_dim, np.arange(t_size, dtype=np.float32)), cls_token)


def get_3d_sincos_pos_embed(embed_dim, grid_size, t_size, cls_token=False):
    """[t_size * grid_size^2 (+ 1), embed_dim], token order (t, h, w): a quarter of the columns encodes t, three quarters (h, w)"""
    assert embed_dim % 4 == 0
    d_s, d_t = embed_dim // 4 * 3, embed_dim // 4
    spatial = _sincos_2d_grid(d_s, grid_size)                                  # [HW, 3D/4]
    temporal = _sincos_1d(d_t, np.arange(t_size, dtype=np.float32))            # [T, D/4]
    hw = grid_size ** 2
    table = np.concatenate([np.repeat(temporal[:, None, :], hw, axis=1), np.repeat(spatial[None, :, :], t_size, axis=0)], axis=-1)
    return _with_cls(table.reshape(-1, embed_dim), cls_token)


# ----------------------------------------------------------------------------- modules
def _no_precise(what):
    if ops.get_precision() == "precise":
        raise TadError(f'{what}: precision "precise" has no route for the InternVideo2 family (use "fast" or "half")')


class RMSNorm(nn.Module):
    """internvideo2.py:119-130"""

    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states, out16=False):
        return ops.RMSNormFn.apply(hidden_states, self.weight, self.variance_epsilon, out16)


class LayerScale(nn.Module):
    """internvideo2.py:133-148: a per-channel factor on the f32 branch output (``force_fp32`` is what this path does anyway)"""

    def __init__(self, dim, init_values=1e-5, inplace=False, force_fp32=False):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))
        self.force_fp32 = force_fp32

    def forward(self, x):
        return x.float() * self.gamma.float()


class Attention(nn.Module):
    """internvideo2.py:151-219.  ``q_norm`` / ``k_norm`` are modules of ``norm_layer`` over the full ``dim`` (RMSNorm in this family);
    their weights go to the fused normalisation, the modules themselves are not called."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., use_flash_attn=False, causal=False,
                 norm_layer=nn.LayerNorm, qk_normalization=False, use_fused_rmsnorm=False):
        super().__init__()
        assert dim % num_heads == 0, 'dim should be divisible by num_heads'
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.use_flash_attn = use_flash_attn
        if causal:
            raise TadError("Attention: causal=True is never used by the reference (Block passes causal=False) and has no kernel")
        if attn_drop:
            raise TadError("Attention: the InternVideo2 family is built with attn_drop=0; attention dropout is not wired through IV2AttentionFn")
        self.qk_normalization = qk_normalization
        self.q_norm = norm_layer(dim) if qk_normalization else nn.Identity()
        self.k_norm = norm_layer(dim) if qk_normalization else nn.Identity()
        self.use_fused_rmsnorm = use_fused_rmsnorm
        if qk_normalization and not isinstance(self.q_norm, RMSNorm):
            raise TadError("Attention: qk_normalization has a kernel for RMSNorm only")

    def forward(self, x):
        gq, gk, eps = (self.q_norm.weight, self.k_norm.weight, self.q_norm.variance_epsilon) if self.qk_normalization else (None, None, 0.0)
        x = ops.IV2AttentionFn.apply(x, self.qkv.weight, self.qkv.bias, gq, gk, self.proj.weight, self.proj.bias, self.num_heads,
                                     self.scale, eps)
        return self.proj_drop(x)


class Mlp(nn.Module):
    """internvideo2.py:222-246"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, bias=True, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        bias = to_2tuple(bias)
        drop_probs = to_2tuple(drop)
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias[0])
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop_probs[0])
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias[1])
        self.drop2 = nn.Dropout(drop_probs[1])
        if not isinstance(self.act, nn.GELU) or getattr(self.act, "approximate", "none") != "none":
            raise TadError("Mlp: only the exact-erf nn.GELU activation has a fused kernel")
        if drop_probs[0]:
            raise TadError("Mlp: dropout between fc1 and fc2 is never used by this family and has no place in the fused MLP")

    def forward(self, x):
        _no_precise("Mlp")
        x = ops.MlpFn.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        return self.drop2(x)


class Block(nn.Module):
    """internvideo2.py:249-299"""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, use_flash_attn=False, use_fused_mlp=False, fused_mlp_heuristic=1,
                 with_cp=False, qk_normalization=False, layerscale_no_force_fp32=False, use_fused_rmsnorm=False):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, use_flash_attn=use_flash_attn,
                              causal=False, norm_layer=norm_layer, qk_normalization=qk_normalization, use_fused_rmsnorm=use_fused_rmsnorm)
        self.ls1 = LayerScale(dim, init_values=init_values, force_fp32=(not layerscale_no_force_fp32)) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.ls2 = LayerScale(dim, init_values=init_values, force_fp32=(not layerscale_no_force_fp32)) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.with_cp = with_cp
        self.use_fused_rmsnorm = use_fused_rmsnorm
        if not isinstance(self.norm1, RMSNorm):
            raise TadError("Block: the InternVideo2 block normalises with RMSNorm")

    def _inner_forward(self, x):
        x = x + self.drop_path1(self.ls1(self.attn(self.norm1(x, out16=True))))
        return x + self.drop_path2(self.ls2(self.mlp(self.norm2(x, out16=True))))

    def forward(self, x, residual=None):
        assert residual is None, "the unfused route carries no separate residual"
        # (first of all: the 1B and 6B models refuse with the attention route's own error, not with whatever their first norm says)
        ops.require_attn_head_dim(ops.head_dim_of(self.attn.qkv.weight, self.attn.num_heads))
        if self.with_cp and torch.is_grad_enabled():
            return checkpoint.checkpoint(self._inner_forward, x, use_reentrant=False)
        return self._inner_forward(x)


class CrossAttention(nn.Module):
    """internvideo2.py:18-80, as AttentionPoolingBlock calls it: ONE query row per clip, keys and values from all tokens.  The q / k / v /
    proj Linears run on the MFMA GEMMs with split operands (ops.LinearSplitFn: f32-level accuracy in every mode -- this head turns 2049
    tokens into the logits, and with 16-bit operands it alone cost more of the logits' accuracy than the encoder); the softmax over [B, heads, N] and its weighted sum are torch ops (2 N head_dim flops per head: no
    kernel is warranted, and head_dim 24 has none)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., attn_head_dim=None, out_dim=None):
        super().__init__()
        if out_dim is None:
            out_dim = dim
        self.num_heads = num_heads
        head_dim = dim // num_heads
        if attn_head_dim is not None:
            head_dim = attn_head_dim
        all_head_dim = head_dim * self.num_heads
        self.scale = qk_scale or head_dim ** -0.5
        assert all_head_dim == dim
        self.q = nn.Linear(dim, all_head_dim, bias=False)
        self.k = nn.Linear(dim, all_head_dim, bias=False)
        self.v = nn.Linear(dim, all_head_dim, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(all_head_dim))
            self.k_bias = nn.Parameter(torch.zeros(all_head_dim))
            self.v_bias = nn.Parameter(torch.zeros(all_head_dim))
        else:
            self.q_bias = None
            self.k_bias = None
            self.v_bias = None
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(all_head_dim, out_dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x, k=None, v=None):
        B, N, C = x.shape
        H = self.num_heads
        q = ops.LinearSplitFn.apply(x, self.q.weight, self.q_bias).reshape(B, N, H, -1).transpose(1, 2)              # [B,H,N_q,d]
        k = ops.LinearSplitFn.apply(k, self.k.weight, self.k_bias).reshape(B, k.shape[1], H, -1).transpose(1, 2)     # [B,H,N_k,d]
        v = ops.LinearSplitFn.apply(v, self.v.weight, self.v_bias).reshape(B, v.shape[1], H, -1).transpose(1, 2)
        attn = ((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
        attn = self.attn_drop(attn)
        x = (attn @ v).transpose(1, 2).reshape(B, N, -1)
        x = ops.LinearSplitFn.apply(x, self.proj.weight, self.proj.bias)
        return self.proj_drop(x)


class AttentiveBlock(nn.Module):
    """internvideo2.py:83-106"""

    def __init__(self, dim, num_heads, qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0., norm_layer=nn.LayerNorm,
                 attn_head_dim=None, out_dim=None):
        super().__init__()
        self.norm1_q = norm_layer(dim)
        self.norm1_k = norm_layer(dim)
        self.norm1_v = norm_layer(dim)
        self.cross_attn = CrossAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop,
                                         attn_head_dim=attn_head_dim, out_dim=out_dim)
        # (the reference builds this DropPath and never applies it: kept for the attribute tree)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    @staticmethod
    def _ln(norm, x):
        return ops.LayerNormFn.apply(x, norm.weight, norm.bias, norm.eps)

    def forward(self, x_q, x_kv, pos_q, pos_k, bool_masked_pos, rel_pos_bias=None):
        x_q = self._ln(self.norm1_q, x_q + pos_q)
        x_k = self._ln(self.norm1_k, x_kv + pos_k)
        x_v = self._ln(self.norm1_v, x_kv)
        return self.cross_attn(x_q, k=x_k, v=x_v)


class AttentionPoolingBlock(AttentiveBlock):
    """internvideo2.py:109-116: the query is the token mean"""

    def forward(self, x):
        x_q = ops.MeanPoolFn.apply(x).unsqueeze(1)
        return super().forward(x_q, x, 0, 0, bool_masked_pos=None, rel_pos_bias=None).squeeze(1)


class PatchEmbed(nn.Module):
    """internvideo2.py:302-334: Conv3d over tubelets, output [B, T, H*W, C].  ``proj`` stays an nn.Conv3d (names, shapes, default init);
    its arithmetic is the im2col + MFMA GEMM of ops.PatchEmbedFn, with no fused position table (the table is trainable and added in torch)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, num_frames=8, tubelet_size=1, norm_layer=None):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.tubelet_size = tubelet_size
        self.grid_size = (num_frames // tubelet_size, img_size[0] // patch_size[0], img_size[1] // patch_size[1])  # (T, H, W)
        self.num_patches = self.grid_size[0] * self.grid_size[1] * self.grid_size[2]
        self.proj = nn.Conv3d(in_channels=in_chans, out_channels=embed_dim, kernel_size=(tubelet_size, patch_size[0], patch_size[1]),
                              stride=(tubelet_size, patch_size[0], patch_size[1]))
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()
        if norm_layer:
            raise TadError("PatchEmbed: a norm behind the projection is never used by this family and has no route")

    # ---- input stage, as modeling_finetune.PatchEmbed has it: uint8 frames, frame-store windows and 16-bit clips straight into the
    # patch matrix.  inference.SlidingWindow / score_video, frame_store and the engines ask for exactly these attributes.
    input_mean = (0.485, 0.456, 0.406)
    input_std = (0.229, 0.224, 0.225)
    input_bgr = False
    t_offset = 0                        # ring-buffer start slot (inference.SlidingWindow)

    def set_input_normalization(self, mean, std, bgr=False):
        self.input_mean, self.input_std, self.input_bgr = tuple(float(v) for v in mean), tuple(float(v) for v in std), bool(bgr)

    def _check_u8(self, H, W, C):
        assert C == 3 and H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
        if ops.get_precision() == "precise":
            raise TadError('precision "precise" takes the normalised f32 clip (the uint8 input stage feeds the bf16 path)')
        _no_precise("PatchEmbed")
        if self.patch_size[0] != self.patch_size[1]:
            raise TadError("PatchEmbed: only square patches have a kernel")

    def forward(self, x):
        w, b, tub, p = self.proj.weight, self.proj.bias, self.tubelet_size, self.patch_size[0]
        if isinstance(x, FrameWindows):
            B, T, H, W, C = x.shape
            self._check_u8(H, W, C)
            y = ops.PatchEmbedWindowsFn.apply(x.store, x.idx, w, b, None, tub, p, self.input_mean, self.input_std, x.bgr)
        elif x.dtype == torch.uint8:
            if x.dim() != 5:
                raise TadError("PatchEmbed: uint8 frames come as [B,T,H,W,3]")
            B, T, H, W, C = x.shape
            self._check_u8(H, W, C)
            y = ops.PatchEmbedU8Fn.apply(x, w, b, None, tub, p, self.input_mean, self.input_std, self.input_bgr, int(self.t_offset))
        else:
            _no_precise("PatchEmbed")
            if x.dim() != 5 or not x.is_floating_point():
                raise TadError("PatchEmbed: this family takes clips [B,C,T,H,W] (float, or the 16-bit operand format), uint8 frames "
                               "[B,T,H,W,3] or frame-store windows")
            B, C, T, H, W = x.shape
            assert H == self.img_size[0] and W == self.img_size[1], \
                f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
            if self.patch_size[0] != self.patch_size[1]:
                raise TadError("PatchEmbed: only square patches have a kernel")
            if x.dtype == ops.K.operand_dtype():
                y = ops.PatchEmbed16Fn.apply(x, w, b, None, tub, p)
            else:
                y = ops.PatchEmbedFn.apply(x.float(), w, b, None, tub, p)
        return y.reshape(B, T // tub, -1, y.shape[-1])


class InternVideo2(nn.Module):
    """internvideo2.py:372-587"""

    def __init__(self, in_chans: int = 3, patch_size: int = 14, img_size: int = 224, qkv_bias: bool = False, drop_path_rate: float = 0.25,
                 embed_dim: int = 1408, head_drop_path_rate: float = 0., num_heads: int = 16, mlp_ratio: float = 4.3637,
                 init_values: float = 1e-5, qk_normalization: bool = True, depth: int = 40, use_flash_attn: bool = True,
                 use_fused_rmsnorm: bool = True, use_fused_mlp: bool = True, fused_mlp_heuristic: int = 1, attn_pool_num_heads: int = 16,
                 clip_embed_dim: int = 768, layerscale_no_force_fp32: bool = False, num_frames: int = 8, tubelet_size: int = 1,
                 sep_pos_embed: bool = False, use_checkpoint: bool = False, checkpoint_num: int = 0, fc_drop_rate: float = 0.,
                 num_classes: int = 1000, init_scale: float = 0.001):
        super().__init__()
        self.use_flash_attn = use_flash_attn
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        # (what inference.score_video / SlidingWindow, explain.token_grid and the engines ask a model: plain attributes, no state)
        self.num_frames = num_frames
        self.tubelet_size = tubelet_size
        self.num_classes = num_classes
        norm_layer_for_blocks = partial(RMSNorm, eps=1e-6)
        self.norm_layer_for_blocks = norm_layer_for_blocks
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim, num_frames=num_frames, tubelet_size=tubelet_size)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.sep_pos_embed = sep_pos_embed
        if sep_pos_embed:
            grid_size = self.patch_embed.grid_size
            self.grid_size = grid_size
            self.pos_embed_spatial = nn.Parameter(torch.zeros(1, grid_size[1] * grid_size[2], embed_dim))
            self.pos_embed_temporal = nn.Parameter(torch.zeros(1, grid_size[0], embed_dim))
            self.pos_embed_cls = nn.Parameter(torch.zeros(1, 1, embed_dim))
        else:
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, device="cpu")]  # (host values also under a meta-device construction)
        with_cp_list = [bool(use_checkpoint) and idx < checkpoint_num for idx in range(depth)]
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer_for_blocks, drop_path=dpr[i],
                  init_values=init_values, attn_drop=0., use_flash_attn=use_flash_attn, use_fused_mlp=use_fused_mlp,
                  fused_mlp_heuristic=fused_mlp_heuristic, with_cp=with_cp_list[i], qk_normalization=qk_normalization,
                  layerscale_no_force_fp32=layerscale_no_force_fp32, use_fused_rmsnorm=use_fused_rmsnorm)
            for i in range(depth)])
        self.clip_projector = AttentionPoolingBlock(dim=embed_dim, num_heads=attn_pool_num_heads, qkv_bias=True, qk_scale=None, drop=0.,
                                                    attn_drop=0., drop_path=head_drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=1e-5),
                                                    out_dim=clip_embed_dim)
        self.fc_norm = nn.LayerNorm(clip_embed_dim)
        self.fc_dropout = nn.Dropout(p=fc_drop_rate) if fc_drop_rate > 0 else nn.Identity()
        self.head = nn.Linear(clip_embed_dim, num_classes)

        self.init_pos_embed()
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)
        self.fix_init_weight()
        self.head.weight.data.mul_(init_scale)
        self.head.bias.data.mul_(init_scale)

    def init_pos_embed(self):
        D = self.embed_dim
        T, Hg, _ = self.patch_embed.grid_size
        if self.sep_pos_embed:
            self.pos_embed_spatial.data.copy_(torch.from_numpy(get_2d_sincos_pos_embed(D, Hg)).float().unsqueeze(0))
            self.pos_embed_temporal.data.copy_(torch.from_numpy(get_1d_sincos_pos_embed(D, T)).float().unsqueeze(0))
        else:
            self.pos_embed.data.copy_(torch.from_numpy(get_3d_sincos_pos_embed(D, Hg, T, cls_token=True)).float().unsqueeze(0))

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def fix_init_weight(self):
        for layer_id, layer in enumerate(self.blocks, start=1):
            for w in (layer.attn.proj.weight, layer.mlp.fc2.weight):
                w.data.div_(math.sqrt(2.0 * layer_id))

    @property
    def dtype(self):
        return self.patch_embed.proj.weight.dtype

    def get_num_layers(self):
        return len(self.blocks)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'pos_embed_spatial', 'pos_embed_temporal', 'pos_embed_cls', 'cls_token'}

    def _pos_table(self):
        if not self.sep_pos_embed:
            return self.pos_embed
        T, Hg, Wg = self.grid_size
        pos = self.pos_embed_spatial.repeat(1, T, 1) + torch.repeat_interleave(self.pos_embed_temporal, Hg * Wg, dim=1)
        return torch.cat([self.pos_embed_cls.expand(pos.shape[0], -1, -1), pos], 1)

    def _blocks_eval(self, x):
        """The blocks without autograd, as one loop that carries (x, xn): the residual stream and its RMSNorm as the next Linear's 16-bit
        operand.  Each half block ends in ONE launch (kernels.residual_rmsnorm: layer scale, residual, the next norm) where the module
        route runs a mul, an add and a norm; the arithmetic of x is the module route's (the product and the sum rounded on their own).
        DropPath is the identity here; a block without LayerScale (init_values=0) has a null gamma."""
        blocks = self.blocks
        for blk in blocks:  # (as Block.forward: the 1B and 6B models refuse with the attention route's own error before anything runs)
            ops.require_attn_head_dim(ops.head_dim_of(blk.attn.qkv.weight, blk.attn.num_heads))
        gamma = lambda ls: ops._f32c(ls.gamma) if isinstance(ls, LayerScale) else None
        x = ops._f32c(x)
        xn = blocks[0].norm1(x, out16=True)
        for i, blk in enumerate(blocks):
            nxt = blocks[i + 1].norm1 if i + 1 < len(blocks) else None
            y = ops._f32c(blk.attn(xn))
            x, xn = ops.K.residual_rmsnorm(x, y, gamma(blk.ls1), ops._f32c(blk.norm2.weight), blk.norm2.variance_epsilon, out=x if i else None)
            y = ops._f32c(blk.mlp(xn))
            x, xn = ops.K.residual_rmsnorm(x, y, gamma(blk.ls2), None if nxt is None else ops._f32c(nxt.weight),
                                           blk.norm2.variance_epsilon if nxt is None else nxt.variance_epsilon, out=x)
        return x

    def forward(self, x):
        _no_precise("InternVideo2")
        ops._need_gpu(x.store if isinstance(x, FrameWindows) else x, "InternVideo2")
        x = self.patch_embed(x)
        B, T, L, C = x.shape
        x = ops.ClassTokenEntryFn.apply(x.reshape(B, T * L, C), self.cls_token, self._pos_table())
        # (a model left in training mode under no_grad still drops paths: that is the module route's affair)
        drops = self.training and any(isinstance(m, DropPath) for blk in self.blocks for m in (blk.drop_path1, blk.drop_path2))
        if not torch.is_grad_enabled() and ops.get_iv2_serve_kernels() and len(self.blocks) and not drops:
            x = self._blocks_eval(x)
        else:
            for blk in self.blocks:
                x = blk(x)
        x = self.clip_projector(x)
        x = ops.LayerNormFn.apply(x, self.fc_norm.weight, self.fc_norm.bias, self.fc_norm.eps)
        return self.head(self.fc_dropout(x))


def _iv2(embed_dim, depth, num_heads, mlp_ratio=4, **kwargs):
    return InternVideo2(img_size=224, patch_size=14, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                        attn_pool_num_heads=16, clip_embed_dim=768, **kwargs)


@register_model
def internvideo2_small_patch14_224(pretrained=False, **kwargs):
    return _iv2(384, 12, 6, **kwargs)


@register_model
def internvideo2_base_patch14_224(pretrained=False, **kwargs):
    return _iv2(768, 12, 12, **kwargs)


@register_model
def internvideo2_large_patch14_224(pretrained=False, **kwargs):
    return _iv2(1024, 24, 16, **kwargs)


@register_model
def internvideo2_1B_patch14_224(pretrained=False, **kwargs):
    """head_dim 88: constructs; every block refuses to run with the attention route's error, "head_dim 88 has no kernel" """
    return _iv2(1408, 40, 16, mlp_ratio=48 / 11, **kwargs)


@register_model
def internvideo2_6B_patch14_224(pretrained=False, **kwargs):
    """head_dim 128 (and D = 3200, beyond the norm kernels' 2048): constructs; every block refuses to run with the attention route's
    "head_dim 128 has no kernel" before anything else is looked at"""
    return _iv2(3200, 48, 25, **kwargs)
