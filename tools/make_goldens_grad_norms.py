#!/usr/bin/env python3
"""Generate ``tests/golden/g21_grad_norms.npz`` by running the REAL reference (imported from its checkout; numpy and torch only, CPU) on
the seeded inputs of ``tests/grad_norms_recipe.py``:

* ``fixed.ft.<case>.<key>`` -- ``utils.collect_grad_norms`` on the reference's tiny fine-tuning model (``golden_recipe.TINY``) with the
  recipe's tensors installed as ``p.grad`` in float32, for the cases ``all`` / ``missing`` and the keys ``qkv`` [L,H,5], ``proj``
  [L,6], ``patch_embed`` [2]; ``fixed.ft.<case>.<key>.f64`` -- the same call with model and gradients in float64 (the float32 tensors
  widened, so the difference between the two is torch's own f32 error on these inputs);
* ``fixed.pt.<case>.<key>[.f64]`` -- ``utils.collect_grad_norms_pretrain`` on the tiny pre-training model (G8's) the same way (the
  function reads ``model.module.encoder``: the model sits in a one-attribute wrapper);
* ``traj.<case>.<key>`` -- the ``grad_norms`` dict ``engine_for_frame_finetuning.train_one_epoch(get_grad_norms=True)`` returns for
  the recipe of G19's ``exponential`` trajectory in float64, for ``update_freq`` 1 and 2 (cases ``uf1`` / ``uf2``), with G12's
  ``clip_grad``; ``traj.<case>.grad_norm`` -- the logged whole-model norms, to show that the coefficient is not 1.

The module stand-ins, ``build_tiny`` and ``import_frame_engine`` are those of make_goldens.py / make_goldens_frame_loss.py.  The
fixture holds arrays only.  Runs only where the reference is present; nothing of its source text is copied.

usage: python tools/make_goldens_grad_norms.py
"""
import argparse
import os
import sys
import types
import unittest.mock as mock
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_goldens as MG  # noqa: E402  (the timm / cv2 stand-ins, build_tiny, save; it puts tests/ on sys.path)
import make_goldens_frame_loss as MF  # noqa: E402
import golden_recipe as R  # noqa: E402
import frame_loss_recipe as FR  # noqa: E402
import grad_norms_recipe as GR  # noqa: E402


def fixed(collect, model, wrap, pre):
    """the three arrays of ``collect`` for both cases, in float32 and in float64"""
    arrs = {}
    for case in GR.FIXED_CASES:
        for dtype, suffix in ((torch.float32, ""), (torch.float64, ".f64")):
            m = model.to(dtype)
            GR.install_grads(m, case, dtype)
            out = collect(wrap(m))
            for key, a in zip(GR.KEYS, out):
                assert a.dtype == np.float64 and np.isfinite(a).all()
                arrs[f"{pre}.{case}.{key}{suffix}"] = a
        spread = np.concatenate([arrs[f"{pre}.{case}.{k}"].ravel() for k in GR.KEYS])
        spread = spread[spread > 0]
        print("G21", pre, case, "norms from %.3e to %.3e" % (spread.min(), spread.max()), "zeros:",
              sum(int((arrs[f"{pre}.{case}.{k}"] == 0).sum()) for k in GR.KEYS))
        assert spread.max() / spread.min() > 1e4, "the magnitudes must differ by several orders"
    return arrs


def trajectory(mf, ref_utils, eff, case):
    import optim_factory as of
    c, t, tc = R.G12, FR.TRAJECTORIES[GR.TRAJECTORY], GR.TRAJECTORY_CASES[case]
    model, _ = MG.build_tiny(mf, torch.float64)
    num_layers = model.get_num_layers()
    assigner = of.LayerDecayValueAssigner([c["layer_decay"] ** (num_layers + 1 - i) for i in range(num_layers + 2)])
    args = argparse.Namespace(opt="adamw", lr=c["base_lr"], weight_decay=c["weight_decay"], opt_eps=1e-8, opt_betas=(0.9, 0.999), momentum=0.9)
    opt = of.create_optimizer(args, model, skip_list=model.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                              get_layer_scale=assigner.get_scale)
    lr_sched = ref_utils.cosine_scheduler(c["base_lr"], c["min_lr"], 1, c["steps"], warmup_epochs=c["warmup_epochs"],
                                          start_warmup_value=c["start_warmup_value"], warmup_steps=c["warmup_steps"])
    wd_sched = ref_utils.cosine_scheduler(c["weight_decay"], c["weight_decay_end"], 1, c["steps"])

    class _Scaler(ref_utils.NativeScalerWithGradNormCount):
        def state_dict(self):
            d = super().state_dict()
            return d if "scale" in d else {"scale": 1.0}

    norms = []

    class _Logger(ref_utils.MetricLogger):
        def update(self, **kw):
            if "grad_norm" in kw:
                norms.append(np.nan if kw["grad_norm"] is None else float(kw["grad_norm"]))
            super().update(**kw)

    crit = MF.reference_criterion(ref_utils, t["loss"], 2)
    batches = MF._Loader((x.double(), y, a, dict(b, ttc=b["ttc"].float())) for x, y, a, b in GR.trajectory_batches(case))
    with mock.patch.object(ref_utils, "MetricLogger", _Logger), mock.patch("torch.cuda.synchronize"), mock.patch("torch.cuda.empty_cache"), \
            mock.patch.object(ref_utils, "print_memory_usage"), mock.patch.object(eff, "calculate_metrics", lambda *a, **k: (None,) * 10), \
            mock.patch.object(eff, "plot_figures", lambda *a, **k: None):
        out = eff.train_one_epoch(model, crit, batches, opt, torch.device("cpu"), 0, _Scaler(), max_norm=c["clip_grad"], start_steps=0,
                                  lr_schedule_values=lr_sched, wd_schedule_values=wd_sched, num_training_steps_per_epoch=c["steps"],
                                  update_freq=tc["update_freq"], with_ttc=t["with_ttc"], smoothed_labels_for_loss=t["smoothed_labels_for_loss"],
                                  get_grad_norms=True)
    gn = out[3]
    assert sorted(gn) == sorted(GR.KEYS) and len(norms) == tc["batches"]
    steps = [n for n in norms if not np.isnan(n)]
    print("G21 traj", case, "grad norms", norms, "qkv", gn["qkv"].ravel()[:5])
    assert len(steps) == c["steps"] and min(steps) > c["clip_grad"], "the coefficient must not be 1"
    arrs = {f"traj.{case}.{k}": np.asarray(gn[k], dtype=np.float64) for k in GR.KEYS}
    arrs[f"traj.{case}.grad_norm"] = np.array(norms)
    return arrs


def main():
    torch.set_num_threads(8)
    _, mf, _ = MG.import_reference()
    ref_utils, eff = MF.import_frame_engine()
    mp, _, _ = MG._pretrain_engine(mf)
    assert mp.__file__.startswith(MG.REF)
    arrs = {}
    ft, _ = MG.build_tiny(mf, torch.float32)
    arrs.update(fixed(ref_utils.collect_grad_norms, ft, lambda m: m, "fixed.ft"))
    cfg = GR.pretrain_config()
    pt = mp.PretrainVisionTransformer(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), use_flash_attn=False, **cfg)
    arrs.update(fixed(ref_utils.collect_grad_norms_pretrain, pt, lambda m: types.SimpleNamespace(module=m), "fixed.pt"))
    for case in GR.TRAJECTORY_CASES:
        arrs.update(trajectory(mf, ref_utils, eff, case))
    MG.save("g21_grad_norms", **arrs)
    size = os.path.getsize(os.path.join(MG.OUT, "g21_grad_norms.npz"))
    assert size <= 100_000, size


if __name__ == "__main__":
    main()
