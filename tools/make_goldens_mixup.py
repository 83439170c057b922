#!/usr/bin/env python3
"""Generate ``tests/golden/g14_mixup.npz`` by running the REAL reference's ``mixup.Mixup`` (imported from /root/reference; numpy and
torch only, CPU) on the seeded inputs of ``tests/mixup_recipe.py``, and its real ``engine_for_finetuning.train_one_epoch`` with that
Mixup as ``mixup_fn`` on the tiny model, exactly as ``tools/make_goldens.py::g12`` drives it without one.

The fixture holds arrays only.  Per case ``<mode>.<configuration>.<seed>``: the soft targets in full, the SHA-256 of the mixed clip's
bytes plus every 13th element of it, and one further ``np.random.rand()`` drawn after the call (pins the state of the stream).
Trajectory (``traj.*``): per-step loss, gradient norm, lr, the epoch averages and the parameter summaries after the last step.

Runs only where the reference is present; nothing of its source text is copied.

usage: python tools/make_goldens_mixup.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_goldens as MG  # noqa: E402  (the timm / cv2 stand-ins, build_tiny, save; it puts tests/ on sys.path)
import golden_recipe as R  # noqa: E402
import mixup_recipe as MR  # noqa: E402


def cases(ref_mixup):
    arrs = {}
    for key, mode, name, seed, shape in MR.cases():
        x = MR.clip(key, shape)
        y = MR.labels(key, shape[0])
        before = x.clone()
        fn = ref_mixup.Mixup(**MR.mixup_kwargs(mode, name))
        np.random.seed(seed)
        out, target = fn(x, y)
        arrs[f"{key}.next"] = np.array(np.random.rand())
        assert out is x and target.dtype == torch.float32 and tuple(target.shape) == (shape[0], MR.NUM_CLASSES)
        arrs[f"{key}.target"] = target.numpy()
        arrs[f"{key}.sha"] = MR.digest(x)
        arrs[f"{key}.sample"] = MR.sample(x)
        arrs[f"{key}.changed"] = np.array(int((x != before).sum()))
    return arrs


def trajectory(mf, ref_mixup):
    import argparse as _ap
    import unittest.mock as mock
    MG.g5_stubs()
    import utils as ref_utils
    import optim_factory as of
    import engine_for_finetuning as eff
    c = R.G12
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
                accs.append(kw["class_acc"])
            super().update(**kw)

    class _Criterion(nn.Module):
        def forward(self, x, target):
            return MR.soft_target_ce_fp64(x, target)

    fn = ref_mixup.Mixup(**MR.TRAJECTORY_MIXUP)
    batches = [(x.double(), y, a, b) for x, y, a, b in R.g12_batches()]
    np.random.seed(MR.TRAJECTORY_SEED)
    with mock.patch.object(ref_utils, "MetricLogger", _Logger), mock.patch("torch.cuda.synchronize"):
        avg = eff.train_one_epoch(model, _Criterion(), batches, opt, torch.device("cpu"), 0, _Scaler(), max_norm=c["clip_grad"],
                                  mixup_fn=fn, start_steps=0, lr_schedule_values=lr_sched, wd_schedule_values=wd_sched,
                                  num_training_steps_per_epoch=c["steps"], update_freq=c["update_freq"])
    print("G14 losses", losses, "grad norms", norms, "averaged", avg)
    assert len(losses) == c["micro_batches"] and all(a is None for a in accs) and "class_acc" not in avg
    arrs = {"traj.loss": np.array(losses), "traj.grad_norm": np.array([np.nan if n is None else n for n in norms]),
            "traj.lr": np.array(lrs), "traj.next": np.array(np.random.rand()),
            "traj.avg_keys": np.array(sorted(avg.keys())), "traj.avg_vals": np.array([float(avg[k]) for k in sorted(avg.keys())]),
            "traj.keys": np.array(list(P.keys()))}
    for k, p in model.named_parameters():
        for kk, v in R.summarize(p.detach().float()).items():
            arrs[f"traj.after.{k}.{kk}"] = v
    return arrs


def main():
    torch.set_num_threads(8)
    _, mf, _ = MG.import_reference()
    import mixup as ref_mixup
    assert ref_mixup.__file__.startswith(MG.REF)
    arrs = cases(ref_mixup)
    arrs.update(trajectory(mf, ref_mixup))
    MG.save("g14_mixup", **arrs)
    size = os.path.getsize(os.path.join(MG.OUT, "g14_mixup.npz"))
    assert size <= 1_000_000, size


if __name__ == "__main__":
    main()
