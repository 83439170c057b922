"""MAE pre-training of the InternVideo2 family (other_models/InternVideo2_single_modality/models/internvideo2_pretrain_videomae.py; driven
by iv2_run_mae_double_pretraining.py through engine_for_pretraining.train_one_epoch_double) behind the reference's operator surface:
class names, constructor arguments, attribute tree, state-dict keys and shapes, the factory name and the initialisation sequence (the
same ``torch.manual_seed`` gives the same weights, pinned by tests/golden/g27_iv2_pretrain.npz).

The encoder is InternVideo2's block stack (internvideo2.Block: RMSNorm, q / k normalisation, fused MLP) without class token and without
the pooling head; the decoder, the mask token and the constant sinusoid table of the decoder input are VideoMAE's (modeling_pretrain).
As in internvideo2.py there is one route: ``use_flash_attn``, ``use_fused_rmsnorm``, ``use_fused_mlp``, ``fused_mlp_heuristic`` and
``layerscale_no_force_fp32`` are accepted and select nothing.

What is new here is the encoder's entry.  Its position table is TRAINABLE (initialised from the 3-D sin-cos table) and is added before
the visible quarter of the tokens is kept: ``x = patch_embed(x) + pos_embed; x_vis = x[~mask].reshape(B, -1, C)``.  ops.VisibleTokensFn
(csrc/visible_tokens.hip) adds and selects in one pass over the visible rows and, on the way back, scatters the gradient and sums the
table's gradient over the clips in a fixed order, in one launch.  With ``sep_pos_embed`` the table is composed of its spatial and
temporal parts by torch ops and autograd carries the split.

Differences, by design (as in modeling_pretrain): ``forward(x, mask, num_masked=None)`` -- ``num_masked`` (identical for every clip, as
the reference's ``reshape(B, -1, C)`` requires) saves one device sync; there is no CPU path and no "precise" mode.
"""
from __future__ import annotations

import math
from functools import partial

import torch
import torch.nn as nn

from . import ops
from ._lib import TadError
from .internvideo2 import (Block, PatchEmbed, RMSNorm, _no_precise, get_1d_sincos_pos_embed, get_2d_sincos_pos_embed,
                           get_3d_sincos_pos_embed)
from .modeling_finetune import trunc_normal_
from .modeling_pretrain import PretrainVisionTransformerDecoder, _init_weights, get_sinusoid_encoding_table, token_indices
from .registry import register_model

__all__ = ['pretrain_videomae_internvideo2_patch14_224']


class iv2_PretrainVisionTransformerEncoder(nn.Module):
    """internvideo2_pretrain_videomae.py:22-231.  ``patch_embed`` is the reference's PatchEmbed_VideoMAE (the same parameters as
    internvideo2.PatchEmbed; its [B, T, H*W, C] output is flattened to [B, N, C] here); ``qk_scale``, ``drop_rate`` and
    ``attn_drop_rate`` are accepted and unused, as in the reference."""

    def __init__(self, num_classes=0, qk_scale=None, drop_rate=0., attn_drop_rate=0., norm_layer=nn.LayerNorm, in_chans: int = 3,
                 patch_size: int = 14, img_size: int = 224, qkv_bias: bool = False, drop_path_rate: float = 0.25, embed_dim: int = 1408,
                 num_heads: int = 16, mlp_ratio: float = 4.3637, init_values: float = 1e-5, qk_normalization: bool = True, depth: int = 40,
                 use_flash_attn: bool = True, use_fused_rmsnorm: bool = True, use_fused_mlp: bool = True, fused_mlp_heuristic: int = 1,
                 layerscale_no_force_fp32: bool = False, num_frames: int = 8, tubelet_size: int = 1, sep_pos_embed: bool = False,
                 use_checkpoint: bool = False, checkpoint_num: int = 0):
        super().__init__()
        self.use_flash_attn = use_flash_attn
        self.embed_dim = embed_dim
        norm_layer_for_blocks = partial(RMSNorm, eps=1e-6)
        self.norm_layer_for_blocks = norm_layer_for_blocks
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim, num_frames=num_frames, tubelet_size=tubelet_size)
        num_patches = self.patch_embed.num_patches
        self.sep_pos_embed = sep_pos_embed
        if sep_pos_embed:
            grid_size = self.patch_embed.grid_size
            self.grid_size = grid_size
            self.pos_embed_spatial = nn.Parameter(torch.zeros(1, grid_size[1] * grid_size[2], embed_dim))
            self.pos_embed_temporal = nn.Parameter(torch.zeros(1, grid_size[0], embed_dim))
            self.pos_embed_cls = nn.Parameter(torch.zeros(1, 1, embed_dim))  # (built and never used, as in the reference)
        else:
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, device="cpu")]
        with_cp_list = [bool(use_checkpoint) and idx < checkpoint_num for idx in range(depth)]
        self.num_classes = num_classes
        self.num_features = self.embed_dim
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer_for_blocks, drop_path=dpr[i],
                  init_values=init_values, attn_drop=0., use_flash_attn=use_flash_attn, use_fused_mlp=use_fused_mlp,
                  fused_mlp_heuristic=fused_mlp_heuristic, with_cp=with_cp_list[i], qk_normalization=qk_normalization,
                  layerscale_no_force_fp32=layerscale_no_force_fp32, use_fused_rmsnorm=use_fused_rmsnorm)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        if not isinstance(self.norm, nn.LayerNorm):
            raise TadError("iv2_PretrainVisionTransformerEncoder: the final norm has a kernel for nn.LayerNorm only")

        self.init_pos_embed()
        self.apply(self._init_weights)
        self.fix_init_weight()

    def init_pos_embed(self):
        D = self.embed_dim
        T, Hg, _ = self.patch_embed.grid_size
        if self.sep_pos_embed:
            self.pos_embed_spatial.data.copy_(torch.from_numpy(get_2d_sincos_pos_embed(D, Hg)).float().unsqueeze(0))
            self.pos_embed_temporal.data.copy_(torch.from_numpy(get_1d_sincos_pos_embed(D, T)).float().unsqueeze(0))
        else:
            self.pos_embed.data.copy_(torch.from_numpy(get_3d_sincos_pos_embed(D, Hg, T, cls_token=False)).float().unsqueeze(0))

    def _init_weights(self, m):
        _init_weights(m)  # xavier_uniform_ on every Linear: the same text as modeling_pretrain's

    def fix_init_weight(self):
        for layer_id, layer in enumerate(self.blocks, start=1):
            for w in (layer.attn.proj.weight, layer.mlp.fc2.weight):
                w.data.div_(math.sqrt(2.0 * layer_id))

    def get_num_layers(self):
        return len(self.blocks)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def _pos_table(self):
        if not self.sep_pos_embed:
            return self.pos_embed
        T, Hg, Wg = self.grid_size
        return self.pos_embed_spatial.repeat(1, T, 1) + torch.repeat_interleave(self.pos_embed_temporal, Hg * Wg, dim=1)

    def forward_features(self, x, mask, num_masked=None, vis_tok=None):
        if len(self.blocks):  # (first of all, as internvideo2.Block does: a width without an attention kernel refuses before any launch)
            ops.require_attn_head_dim(ops.head_dim_of(self.blocks[0].attn.qkv.weight, self.blocks[0].attn.num_heads))
        _no_precise("iv2_PretrainVisionTransformerEncoder")
        ops._need_gpu(x, "iv2_PretrainVisionTransformerEncoder")
        x = self.patch_embed(x)
        B, T, L, C = x.shape
        if vis_tok is None:
            vis_tok, _ = token_indices(mask.to(x.device).flatten(1), num_masked)
        x_vis = ops.VisibleTokensFn.apply(x.reshape(B, T * L, C), self._pos_table(), vis_tok)  # (x + pos_embed)[~mask].reshape(B, -1, C)
        for blk in self.blocks:
            x_vis = blk(x_vis)
        return ops.LayerNormFn.apply(x_vis, self.norm.weight, self.norm.bias, self.norm.eps)

    def forward(self, x, mask, num_masked=None, vis_tok=None):
        x = self.forward_features(x, mask, num_masked, vis_tok)
        if isinstance(self.head, nn.Identity):
            return x
        return ops.LinearFn.apply(x, self.head.weight, self.head.bias)


class PretrainVideoMAEInternVideo2(nn.Module):
    """internvideo2_pretrain_videomae.py:234-353.  ``encoder_to_decoder`` keeps nn.Linear's default initialisation (the reference
    defines ``_init_weights`` on this class and never applies it), and ``mask_token`` is drawn by timm's ``trunc_normal_`` with its
    absolute cut at +-2, not by modeling_pretrain's +-std variant."""

    def __init__(self, img_size=224, patch_size=14, encoder_in_chans=3, encoder_num_classes=0, encoder_embed_dim=768, encoder_depth=12,
                 encoder_num_heads=12, decoder_num_classes=588, decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=8, mlp_ratio=4.,
                 qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=0.,
                 use_learnable_pos_emb=False, use_checkpoint=False, layerscale_no_force_fp32: bool = False, num_frames: int = 8,
                 tubelet_size: int = 1, sep_pos_embed: bool = False, checkpoint_num: int = 0, num_classes=0, in_chans=0):
        super().__init__()
        self.encoder = iv2_PretrainVisionTransformerEncoder(
            img_size=img_size, patch_size=patch_size, in_chans=encoder_in_chans, num_classes=encoder_num_classes,
            embed_dim=encoder_embed_dim, depth=encoder_depth, num_heads=encoder_num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
            qk_scale=qk_scale, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer,
            init_values=init_values, tubelet_size=tubelet_size, use_checkpoint=use_checkpoint, use_flash_attn=True, use_fused_rmsnorm=True,
            use_fused_mlp=True, fused_mlp_heuristic=1, layerscale_no_force_fp32=layerscale_no_force_fp32, num_frames=num_frames,
            sep_pos_embed=sep_pos_embed, checkpoint_num=checkpoint_num)
        self.decoder = PretrainVisionTransformerDecoder(
            patch_size=patch_size, num_patches=self.encoder.patch_embed.num_patches, num_classes=decoder_num_classes,
            embed_dim=decoder_embed_dim, depth=decoder_depth, num_heads=decoder_num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
            qk_scale=qk_scale, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer,
            init_values=init_values, tubelet_size=tubelet_size, use_checkpoint=use_checkpoint)
        self.encoder_to_decoder = nn.Linear(encoder_embed_dim, decoder_embed_dim, bias=False)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.pos_embed = get_sinusoid_encoding_table(self.encoder.patch_embed.num_patches, decoder_embed_dim)
        trunc_normal_(self.mask_token, std=.02)
        self._pos_dev = None

    def _init_weights(self, m):
        _init_weights(m)  # (defined and never applied, as in the reference)

    def get_num_layers(self):
        return len(self.blocks)  # (raises AttributeError exactly as the reference's does, :333-334)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token', 'mask_token'}

    def _pos_on(self, device):
        if self._pos_dev is None or self._pos_dev.device != device:
            self._pos_dev = self.pos_embed[0].to(device=device, dtype=torch.float32).contiguous()
        return self._pos_dev

    def forward(self, x, mask, num_masked=None):
        if not x.is_cuda:
            raise TadError(f"PretrainVideoMAEInternVideo2: input is on {x.device}; the MI355X path runs HIP kernels only (no CPU fallback)")
        vis_tok, mask_tok = token_indices(mask.to(x.device).flatten(1), num_masked)
        x_vis = self.encoder(x, mask, vis_tok=vis_tok)                                          # [B, N_vis, C_e]
        x_vis = ops.LinearFn.apply(x_vis, self.encoder_to_decoder.weight, None)               # [B, N_vis, C_d]
        # the visible tokens keep their order; the constant sinusoid table is gathered accordingly (:347-350)
        x_full = ops.MaeAssembleFn.apply(x_vis, self.mask_token, self._pos_on(x.device), vis_tok.reshape(-1), mask_tok.reshape(-1))
        return self.decoder(x_full, mask_tok.shape[1])                                          # [B, N_mask, 3 * tubelet * patch^2]


@register_model
def pretrain_videomae_internvideo2_patch14_224(pretrained=False, **kwargs):
    """internvideo2_pretrain_videomae.py:356-365 (``pretrained`` is accepted and unused, as there)"""
    return PretrainVideoMAEInternVideo2(img_size=224, patch_size=14, encoder_embed_dim=384, encoder_depth=12, encoder_num_heads=6,
                                        encoder_num_classes=0, decoder_embed_dim=192, decoder_num_heads=3, decoder_num_classes=588,
                                        norm_layer=partial(nn.LayerNorm, eps=1e-6), mlp_ratio=4.0, **kwargs)
