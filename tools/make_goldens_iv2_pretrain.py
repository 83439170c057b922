#!/usr/bin/env python
"""Generate tests/golden/g27_iv2_pretrain.npz by running the REAL reference PretrainVideoMAEInternVideo2
(other_models/InternVideo2_single_modality/models/internvideo2_pretrain_videomae.py) on the CPU on the deterministic inputs of
tests/iv2_pretrain_recipe.py.  Only recorded inputs and outputs are stored (data, no program text); large tensors are stored as
digests, as tests/iv2_recipe.py describes.

    python tools/make_goldens_iv2_pretrain.py --reference <checkout of the reference>

The reference is imported the way tools/make_goldens_internvideo2.py imports it (stubs for timm and flash_attn, the models directory as
a synthetic package), with the repository root on ``sys.path`` for its ``modeling_pretrain``; ``einops`` must be installed.  The outer
class hard-wires the fused route for its encoder (use_flash_attn = use_fused_rmsnorm = use_fused_mlp = True) and lets the decoder
default to flash attention, neither of which exists on a CPU.  So two names are rebound IN THE LOADED MODULE'S NAMESPACE before the model
is built: ``iv2_PretrainVisionTransformerEncoder`` to a wrapper that forces the three switches to False, and
``PretrainVisionTransformerDecoder`` to one that forces ``use_flash_attn=False``.  The classes themselves, and with them every
parameter, every draw of the initialisation and every operator of the forward, are the reference's.
"""
import argparse
import importlib.util
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import iv2_pretrain_recipe as PR  # noqa: E402
import iv2_recipe as R  # noqa: E402
from make_goldens_internvideo2 import import_reference  # noqa: E402


def import_pretrain(ref):
    import_reference(ref)  # timm / flash_attn stubs, the synthetic package with pos_embed and internvideo2, the root on sys.path
    # what the root modeling_finetune / modeling_pretrain import beyond that (tools/make_goldens.py stubs the same two)
    def _no_drop_path(x, drop_prob=0.0, training=False):
        assert not (training and drop_prob), "fixtures use drop_path_rate=0"
        return x
    sys.modules["timm.models.layers"].drop_path = _no_drop_path
    fa = types.ModuleType("flash_attention_class")
    fa.FlashAttention = sys.modules["iv2_reference_models.flash_attention_class"].FlashAttention  # (raises when built)
    sys.modules["flash_attention_class"] = fa
    src = os.path.join(ref, "other_models", "InternVideo2_single_modality", "models", "internvideo2_pretrain_videomae.py")
    spec = importlib.util.spec_from_file_location("iv2_reference_models.internvideo2_pretrain_videomae", src)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)

    encoder, decoder = mod.iv2_PretrainVisionTransformerEncoder, mod.PretrainVisionTransformerDecoder

    def unfused_encoder(*a, **k):
        k.update(use_flash_attn=False, use_fused_rmsnorm=False, use_fused_mlp=False)
        return encoder(*a, **k)

    def plain_decoder(*a, **k):
        k.update(use_flash_attn=False)
        return decoder(*a, **k)
    mod.iv2_PretrainVisionTransformerEncoder, mod.PretrainVisionTransformerDecoder = unfused_encoder, plain_decoder
    return mod


def build(mod, **over):
    torch.manual_seed(0)
    return mod.PretrainVideoMAEInternVideo2(norm_layer=partial(nn.LayerNorm, eps=1e-6), **dict(PR.TINY, **over)), dict(PR.TINY, **over)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository")
    args = ap.parse_args()
    mod = import_pretrain(os.path.abspath(args.reference))
    out = {}

    # (a) the state dict right after construction
    model, cfg = build(mod)
    sd = model.state_dict()
    out["a/keys"] = np.array(list(sd))
    out["a/shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["a/sha256"] = np.array([R.sha(v) for v in sd.values()])
    out["a/no_weight_decay"] = np.array(sorted(model.no_weight_decay()))
    out["a/encoder_no_weight_decay"] = np.array(sorted(model.encoder.no_weight_decay()))
    out["a/decoder_no_weight_decay"] = np.array(sorted(model.decoder.no_weight_decay()))
    out["a/encoder_num_layers"] = np.array(model.encoder.get_num_layers())
    out["a/decoder_num_layers"] = np.array(model.decoder.get_num_layers())
    out["a/param_keys"] = np.array([k for k, _ in model.named_parameters()])
    out["a/num_parameters"] = np.array(sum(p.numel() for p in model.parameters()))

    # (b) perturbed parameters, fp64 forward / MSE loss against a seeded target / every gradient
    R.perturb_(model.named_parameters())
    out["b/sha256"] = np.array([R.sha(p) for _, p in model.named_parameters()])
    model.double()
    pred = model(PR.clip().double(), PR.mask())
    assert tuple(pred.shape) == (2, PR.N - PR.NV, 588)
    loss = nn.functional.mse_loss(pred, PR.target().double())
    loss.backward()
    out["b/output"], out["b/loss"] = R.record(pred, 1000), loss.detach().numpy()
    for i, (k, p) in enumerate(model.named_parameters()):
        assert p.grad is not None, k
        out["b/grad/" + k] = R.record(p.grad, i)

    # (c) forward-only variants
    for name, over in PR.VARIANTS.items():
        model, cfg = build(mod, **over)
        out[f"c/{name}/keys"] = np.array(list(model.state_dict()))
        R.perturb_(model.named_parameters())
        out[f"c/{name}/sha256"] = np.array([R.sha(p) for _, p in model.named_parameters()])
        with torch.no_grad():
            out[f"c/{name}/output"] = R.record(model.double()(PR.clip().double(), PR.mask()), 1000)

    path = PR.GOLDEN
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
