#!/usr/bin/env python
"""Generate tests/golden/g26_internvideo2.npz by running the REAL reference InternVideo2
(other_models/InternVideo2_single_modality/models/internvideo2.py) on the CPU, unfused route, on the deterministic inputs of
tests/iv2_recipe.py.  Only recorded inputs and outputs are stored (data, no program text); what is stored and why large tensors are
stored as digests is described in tests/iv2_recipe.py.

    python tools/make_goldens_internvideo2.py --reference <checkout of the reference>

Third-party modules the reference imports and this environment lacks: ``timm.models.layers`` / ``timm.models.registry`` are stubbed as
tools/make_goldens.py does (to_2tuple and trunc_normal_ from the reference's own in-repo copies, run_inference_simple.py; DropPath is
never built, every fixture has drop path 0); ``flash_attn.modules.mlp``, ``flash_attn.ops.rms_norm`` and the directory's
``flash_attention_class`` are stubbed with classes that raise.  internvideo2.py and pos_embed.py are loaded under a synthetic package, so
the directory's ``models/__init__.py`` and its other imports never run.
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

import iv2_recipe as R  # noqa: E402


def _raising(name):
    class _Absent(nn.Module):
        def __init__(self, *a, **k):
            raise RuntimeError(f"{name} is not available; the fixtures run the unfused route")
    _Absent.__name__ = name
    return _Absent


def import_reference(ref):
    sys.path.insert(0, ref)
    for name in ("cv2", "natsort"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["natsort"].natsorted = sorted
    import run_inference_simple as ris

    mods = {n: types.ModuleType(n) for n in ("timm", "timm.models", "timm.models.layers", "timm.models.registry", "flash_attn",
                                              "flash_attn.modules", "flash_attn.modules.mlp", "flash_attn.ops", "flash_attn.ops.rms_norm")}
    layers = mods["timm.models.layers"]
    layers.to_2tuple, layers.trunc_normal_, layers.DropPath = ris.to_2tuple, ris.trunc_normal_, _raising("DropPath")
    mods["timm.models.registry"].register_model = lambda f: f
    mods["flash_attn.modules.mlp"].FusedMLP = _raising("FusedMLP")
    mods["flash_attn.ops.rms_norm"].DropoutAddRMSNorm = _raising("DropoutAddRMSNorm")
    sys.modules.update(mods)

    src = os.path.join(ref, "other_models", "InternVideo2_single_modality", "models")
    pkg = types.ModuleType("iv2_reference_models")
    pkg.__path__ = []  # a package whose __init__ never runs
    sys.modules[pkg.__name__] = pkg
    fa = types.ModuleType(pkg.__name__ + ".flash_attention_class")
    fa.FlashAttention = _raising("FlashAttention")
    sys.modules[fa.__name__] = fa
    out = {}
    for name in ("pos_embed", "internvideo2"):
        spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.{name}", os.path.join(src, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        out[name] = mod
    return out["internvideo2"]


def build(iv2, **over):
    torch.manual_seed(0)
    cfg = dict(R.TINY, **R.REF_ROUTE, **over)
    return iv2.InternVideo2(**cfg), dict(R.TINY, **over)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository")
    args = ap.parse_args()
    iv2 = import_reference(os.path.abspath(args.reference))
    out = {}

    # (a) the state dict right after construction
    model, cfg = build(iv2)
    sd = model.state_dict()
    out["a/keys"] = np.array(list(sd))
    out["a/shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["a/sha256"] = np.array([R.sha(v) for v in sd.values()])
    out["a/no_weight_decay"] = np.array(sorted(model.no_weight_decay()))
    out["a/num_layers"] = np.array(model.get_num_layers())
    out["a/param_keys"] = np.array([k for k, _ in model.named_parameters()])

    # (b) perturbed parameters, fp64 forward / loss / gradients
    R.perturb_(model.named_parameters())
    out["b/sha256"] = np.array([R.sha(p) for _, p in model.named_parameters()])
    model.double()
    logits = model(R.clip().double())
    loss = nn.functional.cross_entropy(logits, torch.tensor(R.LABELS))
    loss.backward()
    out["b/logits"], out["b/loss"] = logits.detach().numpy(), loss.detach().numpy()
    for i, (k, p) in enumerate(model.named_parameters()):
        assert p.grad is not None, k
        out["b/grad/" + k] = R.record(p.grad, i)

    # (c) one Block
    torch.manual_seed(0)
    blk = iv2.Block(norm_layer=partial(iv2.RMSNorm, eps=1e-6), **R.BLOCK)
    R.perturb_(blk.named_parameters())
    out["c/keys"] = np.array([k for k, _ in blk.named_parameters()])
    out["c/sha256"] = np.array([R.sha(p) for _, p in blk.named_parameters()])
    blk.double()
    x, dy = (t.double() for t in R.block_input())
    x.requires_grad_()
    y = blk(x)
    (y * dy).sum().backward()
    out["c/y"], out["c/dx"] = y.detach().numpy(), x.grad.numpy()
    for i, (k, p) in enumerate(blk.named_parameters()):
        out["c/grad/" + k] = R.record(p.grad, i)

    # (d) forward-only variants
    for name, over in R.VARIANTS.items():
        model, cfg = build(iv2, **over)
        out[f"d/{name}/keys"] = np.array(list(model.state_dict()))
        R.perturb_(model.named_parameters())
        out[f"d/{name}/sha256"] = np.array([R.sha(p) for _, p in model.named_parameters()])
        with torch.no_grad():
            out[f"d/{name}/logits"] = model.double()(R.clip().double()).numpy()

    path = R.GOLDEN
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
