#!/usr/bin/env python3
"""Generate ``tests/golden/g19_frame_losses.npz`` by running the REAL reference (imported from /root/reference; numpy and torch only,
CPU) on the seeded inputs of ``tests/frame_loss_recipe.py``:

* ``utils.FocalLoss`` / ``FocalLoss2`` / ``SmoothAPLoss`` / ``TemporalExponentialLoss`` / ``DoubleBCELoss`` in every ``--loss``
  configuration of run_frame_finetuning.py:571-586, on fp64 logits, with autograd for the gradient: per case and configuration the loss
  and the full ``dloss/dlogits`` (``loss.<case>.<configuration>`` / ``grad.…``);
* ``dataset/data_utils.compute_time_vector`` / ``smooth_labels`` on a handful of label vectors (``tv.<case>`` / ``sm.<case>.<k>``);
* three short fine-tune trajectories of the tiny model (``traj.<name>.*``: per-step loss, gradient norm, lr, class_acc, the epoch
  averages), driven through the reference's real ``engine_for_frame_finetuning.train_one_epoch`` with its ``with_ttc`` /
  ``smoothed_labels_for_loss`` switches, its scaler, schedules and optimizer factory, exactly as ``tools/make_goldens.py::g12`` drives
  ``engine_for_finetuning``.  That module imports plotting and metric packages at module level; the ones this image lacks are
  MagicMock stand-ins, and its end-of-epoch ``calculate_metrics`` / ``plot_figures`` (not part of the trajectory) are patched out.

``TemporalExponentialLoss`` is handed the time to the anomaly as float32: with the float64 vector of ``compute_time_vector`` its masked
assignment into a float32 weight is refused by the torch of this image (older ones cast silently), so float32 is the only form in which
the class runs; its weights are then exp() evaluated in f32, 1e-7 from the fp64 statement of the recipe.

The fixture holds arrays only.  Runs only where the reference is present; nothing of its source text is copied.

usage: python tools/make_goldens_frame_loss.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_goldens as MG  # noqa: E402  (the timm / cv2 stand-ins, build_tiny, save; it puts tests/ on sys.path)
import golden_recipe as R  # noqa: E402
import frame_loss_recipe as FR  # noqa: E402


def reference_criterion(ref_utils, name, classes):
    cfg = FR.CONFIGS[name]
    kind = cfg["kind"]
    if kind == "focal":
        return ref_utils.FocalLoss(alpha=cfg["alpha"], gamma=cfg["gamma"], multiplier=cfg["multiplier"])
    if kind == "focal2":
        return ref_utils.FocalLoss2(alpha=FR.class_alpha_for(cfg, classes), gamma=cfg["gamma"], multiplier=cfg["multiplier"])
    if kind == "2bce":
        return ref_utils.DoubleBCELoss()
    if kind == "smoothap":
        return ref_utils.SmoothAPLoss(delta=cfg["delta"])
    return ref_utils.TemporalExponentialLoss(alpha_pre=cfg["alpha_pre"], alpha_post=cfg["alpha_post"])


def losses(ref_utils):
    arrs = {}
    for case, (B, classes) in FR.CASES.items():
        logits, labels, ttc, soft = FR.inputs(case, B, classes)
        for name in FR.configs_for(classes):
            crit = reference_criterion(ref_utils, name, classes)
            z = logits.double().requires_grad_()
            kind = FR.CONFIGS[name]["kind"]
            loss = crit(z, soft.double()) if kind == "2bce" else crit(z, labels, ttc.float()) if kind == "exponential" else crit(z, labels)
            loss.backward()
            arrs[f"loss.{case}.{name}"] = FR.np64(loss)
            arrs[f"grad.{case}.{name}"] = FR.np64(z.grad)
    return arrs


def targets(du):
    arrs = {}
    for case, (labels, fps, TT, TA) in FR.TARGET_CASES.items():
        tv = du.compute_time_vector(labels, fps, TT, TA)
        assert tv.dtype == torch.float64
        arrs[f"tv.{case}"] = tv.numpy()
        for k, (before, after) in enumerate(FR.SMOOTH_LIMITS):
            sm = du.smooth_labels(torch.tensor(labels), tv, before, after)
            assert sm.dtype == torch.float32 and tuple(sm.shape) == (len(labels), 2)
            arrs[f"sm.{case}.{k}"] = sm.numpy()
    return arrs


def import_frame_engine():
    """engine_for_frame_finetuning with MagicMock stand-ins for the module-level imports this image lacks"""
    import unittest.mock as mock
    MG.g5_stubs()
    sys.modules["timm.utils"].accuracy = lambda *a, **k: None
    for name in ("pandas", "scipy", "scipy.special", "torchmetrics", "sklearn", "sklearn.metrics", "matplotlib", "matplotlib.pyplot", "seaborn",
                 "dataset.vis_tools", "anaysis.metrics"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = mock.MagicMock()
    import utils as ref_utils
    import engine_for_frame_finetuning as eff
    assert eff.__file__.startswith(MG.REF) and ref_utils.__file__.startswith(MG.REF)
    return ref_utils, eff


class _Loader(list):
    batch_size = 2       # (the engine asks its loader for one)


def trajectory(mf, ref_utils, eff, name):
    import argparse as _ap
    import unittest.mock as mock
    import optim_factory as of
    c, t = R.G12, FR.TRAJECTORIES[name]
    model, P = MG.build_tiny(mf, torch.float64)
    num_layers = model.get_num_layers()
    assigner = of.LayerDecayValueAssigner([c["layer_decay"] ** (num_layers + 1 - i) for i in range(num_layers + 2)])
    args = _ap.Namespace(opt="adamw", lr=c["base_lr"], weight_decay=c["weight_decay"], opt_eps=1e-8, opt_betas=(0.9, 0.999), momentum=0.9)
    opt = of.create_optimizer(args, model, skip_list=model.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                              get_layer_scale=assigner.get_scale)
    lr_sched = ref_utils.cosine_scheduler(c["base_lr"], c["min_lr"], 1, c["steps"], warmup_epochs=c["warmup_epochs"],
                                          start_warmup_value=c["start_warmup_value"], warmup_steps=c["warmup_steps"])
    wd_sched = ref_utils.cosine_scheduler(c["weight_decay"], c["weight_decay_end"], 1, c["steps"])

    class _Scaler(ref_utils.NativeScalerWithGradNormCount):
        def state_dict(self):
            d = super().state_dict()
            return d if "scale" in d else {"scale": 1.0}

    losses, norms, lrs, accs = [], [], [], []

    class _Logger(ref_utils.MetricLogger):
        def update(self, **kw):
            if "loss" in kw:
                losses.append(float(kw["loss"]))
            if "grad_norm" in kw:
                norms.append(None if kw["grad_norm"] is None else float(kw["grad_norm"]))
            if "lr" in kw:
                lrs.append(float(kw["lr"]))
            if "class_acc" in kw:
                accs.append(float(kw["class_acc"]))
            super().update(**kw)

    # the criterion of the --loss name (run_frame_finetuning.py:571-586); `exponential1` as the default instance, which is what the
    # name can only mean (the reference's own constructor call raises)
    crit = reference_criterion(ref_utils, t["loss"], 2)
    batches = _Loader((x.double(), y, a, dict(b, ttc=b["ttc"].float())) for x, y, a, b in FR.trajectory_batches())
    with mock.patch.object(ref_utils, "MetricLogger", _Logger), mock.patch("torch.cuda.synchronize"), mock.patch("torch.cuda.empty_cache"), \
            mock.patch.object(ref_utils, "print_memory_usage"), mock.patch.object(eff, "calculate_metrics", lambda *a, **k: (None,) * 10), \
            mock.patch.object(eff, "plot_figures", lambda *a, **k: None):
        avg = eff.train_one_epoch(model, crit, batches, opt, torch.device("cpu"), 0, _Scaler(), max_norm=c["clip_grad"], start_steps=0,
                                  lr_schedule_values=lr_sched, wd_schedule_values=wd_sched, num_training_steps_per_epoch=c["steps"],
                                  update_freq=c["update_freq"], with_ttc=t["with_ttc"], smoothed_labels_for_loss=t["smoothed_labels_for_loss"],
                                  get_grad_norms=False)[0]
    print("G19", name, "losses", losses, "grad norms", norms, "class_acc", accs)
    assert len(losses) == c["micro_batches"] and sum(n is not None for n in norms) == c["steps"] and len(accs) == c["micro_batches"]
    keys = sorted(k for k in avg if avg[k] is not None)
    pre = f"traj.{name}."
    arrs = {pre + "loss": np.array(losses), pre + "grad_norm": np.array([np.nan if n is None else n for n in norms]), pre + "lr": np.array(lrs),
            pre + "class_acc": np.array(accs), pre + "avg_keys": np.array(keys), pre + "avg_vals": np.array([float(avg[k]) for k in keys])}
    for k, p in model.named_parameters():
        for kk, v in R.summarize(p.detach().float()).items():
            arrs[f"{pre}after.{k}.{kk}"] = v
    return arrs


def main():
    torch.set_num_threads(8)
    _, mf, _ = MG.import_reference()
    ref_utils, eff = import_frame_engine()
    from dataset import data_utils as du
    assert du.__file__.startswith(MG.REF)
    arrs = losses(ref_utils)
    arrs.update(targets(du))
    for name in FR.TRAJECTORIES:
        arrs.update(trajectory(mf, ref_utils, eff, name))
    MG.save("g19_frame_losses", **arrs)
    size = os.path.getsize(os.path.join(MG.OUT, "g19_frame_losses.npz"))
    assert size <= 1_000_000, size


if __name__ == "__main__":
    main()
