"""Seeded inputs and shared helpers of the gradient-norm fixture G21 (tests/golden/g21_grad_norms.npz, written by
tools/make_goldens_grad_norms.py from the reference's own ``utils.collect_grad_norms`` / ``collect_grad_norms_pretrain`` and
``engine_for_frame_finetuning.train_one_epoch(get_grad_norms=True)``).  The fixture holds results only; every input is regenerated
from here.

(a) / (b): fixed gradients.  Every parameter of the tiny fine-tuning model (``golden_recipe.TINY``) and of the tiny pre-training model
(G8's) gets a seeded tensor as its gradient.  Magnitudes differ per tensor by up to six orders (``scale_for``) and, inside a tensor,
per group of 64 rows (one head's slice of qkv.weight / q_bias / v_bias), so that neither a slot mix-up between tensors nor one between
heads or between Q, K and V can hide.  Two cases: ``all`` (every parameter holds a gradient) and ``missing`` (the gradients
``is_missing`` names are left None).

(c): the trajectory of G19's ``exponential`` case through the fine-tuning engine with the diagnostics on, once with ``update_freq``
1 (G12's first three micro-batches = three optimizer steps) and once with 2 (all six: three steps, each behind one raw micro-step);
G12's ``clip_grad`` 1.5 lies below every gradient norm of that trajectory (2 .. 5), so the coefficient is never 1."""
import torch

import frame_loss_recipe as FR
import golden_recipe as R

KEYS = ("qkv", "proj", "patch_embed")
FIXED_CASES = ("all", "missing")
HEAD_DIM = 64


def scale_for(name):
    """10^-4 .. 10^2, fixed by the parameter's name"""
    return 10.0 ** (R._seed_for("g21.scale." + name, 21) % 7 - 4)


def grad_for(name, shape):
    """the f32 gradient of parameter ``name``: N(0, 1) * scale_for(name) * (1 + index of the 64-row group along dim 0)"""
    g = R.tensor_for("g21.grad." + name, tuple(shape), seed=21)
    rows = (1 + torch.arange(shape[0]) // HEAD_DIM).to(torch.float32).view(-1, *([1] * (len(shape) - 1)))
    return g * rows * scale_for(name)


def is_missing(name):
    """the parameters whose gradient the ``missing`` case leaves None: every attn.proj.bias and the patch embedding's weight (names of
    the encoder; the pre-training wrapper prefixes ``encoder.``)"""
    n = name[len("encoder."):] if name.startswith("encoder.") else name
    return n.endswith("attn.proj.bias") or n == "patch_embed.proj.weight"


def install_grads(model, case, dtype=None):
    """``p.grad`` of every parameter of a plain torch model = its recipe tensor (None where the case leaves it out)"""
    assert case in FIXED_CASES
    for name, p in model.named_parameters():
        p.grad = None if (case == "missing" and is_missing(name)) else grad_for(name, p.shape).to(dtype or p.dtype)


def fill_flat_grads(model, case):
    """the same into gradients that are views of a flat buffer (optim.FusedAdamW): copied in place, zeros where the case leaves the
    gradient out -- a flat buffer has no None"""
    assert case in FIXED_CASES
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.grad is None:                                        # (not trainable: outside the flat buffer)
                continue
            if case == "missing" and is_missing(name):
                p.grad.zero_()
            else:
                p.grad.copy_(grad_for(name, p.shape))


def pretrain_config():
    """G8's tiny pre-training model"""
    return dict(img_size=32, patch_size=16, encoder_embed_dim=128, encoder_depth=2, encoder_num_heads=2, decoder_num_classes=1536,
                decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=1, mlp_ratio=4, qkv_bias=True, init_values=0., tubelet_size=2)


# ------------------------------------------------------------------ (c) the trajectory
TRAJECTORY = "exponential"                                    # the traj.* case of G19 whose recipe is driven
TRAJECTORY_CASES = {"uf1": dict(update_freq=1, batches=3), "uf2": dict(update_freq=2, batches=6)}


def trajectory_batches(case, dtype=torch.float32):
    return FR.trajectory_batches(dtype)[:TRAJECTORY_CASES[case]["batches"]]


def run_trajectory(E, model, device, dtype, criterion, case, grad_norms=None, scaler=None, optimizer=None):
    """G19's trajectory recipe (G12's schedules, layer decay and clipping) through ``E.train_one_epoch`` at the case's update_freq"""
    c, t = R.G12, FR.TRAJECTORIES[TRAJECTORY]
    opt = optimizer or E.create_optimizer(model, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"])
    lr_sched = E.cosine_scheduler(c["base_lr"], c["min_lr"], 1, c["steps"], warmup_epochs=c["warmup_epochs"],
                                  start_warmup_value=c["start_warmup_value"], warmup_steps=c["warmup_steps"])
    wd_sched = E.cosine_scheduler(c["weight_decay"], c["weight_decay_end"], 1, c["steps"])
    kw = {} if grad_norms is None else {"grad_norms": grad_norms}
    stats = E.train_one_epoch(model, criterion, trajectory_batches(case, dtype), opt, device, 0, scaler or E.NativeScalerWithGradNormCount(model),
                              max_norm=c["clip_grad"], start_steps=0, lr_schedule_values=lr_sched, wd_schedule_values=wd_sched,
                              num_training_steps_per_epoch=c["steps"], update_freq=TRAJECTORY_CASES[case]["update_freq"],
                              with_ttc=t["with_ttc"], smoothed_labels_for_loss=t["smoothed_labels_for_loss"], **kw)
    return opt, stats
