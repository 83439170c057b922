"""Mixup / CutMix and the soft-target losses without a GPU: this package's ``Mixup`` against the reference's own (golden G14,
tools/make_goldens_mixup.py) bit for bit on the torch path, the losses against an fp64 statement of their formulas, the fine-tune
trajectory with ``mixup_fn`` around the fp64 oracle, and the host-side validation of the new C entry points."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_recipe as R
import mixup_recipe as MR
import simple_tad_amd as T
from oracle import vit_oracle as O
from simple_tad_amd import engine as E
from simple_tad_amd.loss import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
from simple_tad_amd.mixup import Mixup, mixup_target

CASES = list(MR.cases())


@pytest.mark.parametrize("key,mode,name,seed,shape", CASES, ids=[c[0] for c in CASES])
def test_mixup_reproduces_the_reference_bit_for_bit(golden, key, mode, name, seed, shape):
    g = golden("g14_mixup")
    x, y = MR.clip(key, shape), MR.labels(key, shape[0])
    fn = Mixup(**MR.mixup_kwargs(mode, name))
    np.random.seed(seed)
    out, target = fn(x, y)
    after = np.random.rand()
    assert out is x
    assert np.array_equal(MR.digest(x), g[f"{key}.sha"]) and np.array_equal(MR.sample(x), g[f"{key}.sample"])
    assert target.dtype == torch.float32 and np.array_equal(target.numpy(), g[f"{key}.target"])
    assert after == float(g[f"{key}.next"])       # the numpy stream stands where the reference left it


def test_golden_cases_cover_the_ragged_shapes_and_every_kind(golden):
    g = golden("g14_mixup")
    shapes = set(MR.SHAPES.values())
    assert any(s[2] < s[3] for s in shapes) and any(s[3] != s[4] for s in shapes) and any(s[4] % 4 for s in shapes)
    assert len(CASES) >= 3 * 5 * 3
    changed = [int(g[f"{c[0]}.changed"]) for c in CASES]
    assert sum(n > 0 for n in changed) > len(CASES) // 2      # (prob 0.5 and lam == 1 leave some batches alone)


def test_constructor_keeps_the_reference_surface():
    fn = Mixup()
    assert (fn.mixup_alpha, fn.cutmix_alpha, fn.cutmix_minmax, fn.mix_prob, fn.switch_prob, fn.label_smoothing, fn.num_classes, fn.mode,
            fn.correct_lam, fn.mixup_enabled) == (1., 0., None, 1.0, 0.5, 0.1, 1000, 'batch', True, True)
    assert Mixup(cutmix_minmax=(0.2, 0.8)).cutmix_alpha == 1.0
    assert T.Mixup is Mixup and T.mixup.Mixup is Mixup and T.loss.SoftTargetCrossEntropy is SoftTargetCrossEntropy


@pytest.mark.parametrize("mode", MR.MODES)
def test_disabled_or_lam_one_leaves_the_bytes_alone_and_odd_batches_are_refused(mode):
    x = MR.clip("leave", (4, 3, 2, 6, 8))
    was = x.clone()
    y = torch.tensor([0, 1, 2, 3])
    fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=4, label_smoothing=0.0)
    fn.mixup_enabled = False
    np.random.seed(1)
    out, target = fn(x, y)
    assert out is x and torch.equal(x, was) and torch.equal(target, F.one_hot(y, 4).float())
    fn = Mixup(mixup_alpha=0.8, cutmix_alpha=0.0, prob=0.0, mode=mode, num_classes=4, label_smoothing=0.0)   # never mixed: lam == 1
    out, target = fn(x, y)
    assert torch.equal(x, was) and torch.equal(target, F.one_hot(y, 4).float())
    with pytest.raises(AssertionError, match="even"):
        fn(x[:3], y[:3])


def test_pair_mode_cuts_time_and_height_on_video():
    """mixup.py:187-188: the (H, W) box of pair mode lands on the T and H axes of a video sample, over the whole width"""
    x = MR.clip("pairquirk", (2, 3, 4, 12, 16))
    was = x.clone()
    fn = Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="pair", num_classes=2)
    np.random.seed(5)
    rows, lam = fn.plan(x.shape)
    kind, _, _, (t0, t1, y0, y1, x0, x1) = rows[0]
    assert kind == 2 and rows[1] == rows[0] and (x0, x1) == (0, 16) and t1 <= 4 and y1 <= 12
    np.random.seed(5)
    fn(x, torch.tensor([0, 1]))
    moved = (x[0] != was[0])
    assert bool(moved.any())
    inside = torch.zeros_like(moved)
    inside[:, t0:t1, y0:y1, :] = True
    assert not bool((moved & ~inside).any()) and torch.equal(x[0][:, t0:t1, y0:y1], was[1][:, t0:t1, y0:y1])


# ------------------------------------------------------------------ losses
def _soft_ce64(z, t):
    return torch.sum(-t.double() * torch.log_softmax(z.double(), -1), -1).mean()


@pytest.mark.parametrize("classes", [2, 174, 1000])
def test_soft_target_loss_matches_the_fp64_formula_on_cpu(classes):
    z = R.tensor_for(f"ce.z{classes}", (8, classes), seed=1, scale=3.0)
    z[0, 0], z[0, 1] = 60.0, -50.0      # a row with a large logit spread
    t = torch.softmax(R.tensor_for(f"ce.t{classes}", (8, classes), seed=2), -1)
    z32 = z.clone().requires_grad_()
    loss = SoftTargetCrossEntropy()(z32, t)
    loss.backward()
    z64 = z.double().requires_grad_()
    ref = _soft_ce64(z64, t)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 4e-6 * abs(ref.item())          # f32 evaluation of the same expression
    assert (z32.grad.double() - z64.grad).abs().max().item() <= 2e-7
    # fp64 inputs: the expression itself
    z64b = z.double().requires_grad_()
    again = SoftTargetCrossEntropy()(z64b, t.double())
    again.backward()
    assert abs(again.item() - ref.item()) <= 1e-14 * abs(ref.item()) and torch.allclose(z64b.grad, z64.grad, rtol=0, atol=1e-16)


@pytest.mark.parametrize("classes", [2, 174, 1000])
def test_label_smoothing_loss_is_the_soft_loss_of_the_smoothed_row(classes):
    s = 0.1
    z = R.tensor_for(f"ls.z{classes}", (6, classes), seed=3, scale=2.0).double()
    z[1, 0], z[1, 1] = 40.0, -40.0
    y = torch.arange(6) % classes
    t = torch.full((6, classes), s / classes, dtype=torch.float64)
    t[torch.arange(6), y] += 1 - s
    za, zb = z.clone().requires_grad_(), z.clone().requires_grad_()
    a = LabelSmoothingCrossEntropy(smoothing=s)(za, y)
    b = _soft_ce64(zb, t)
    a.backward()
    b.backward()
    assert abs(a.item() - b.item()) <= 1e-13 * abs(b.item()) and torch.allclose(za.grad, zb.grad, rtol=0, atol=1e-15)
    crit = LabelSmoothingCrossEntropy()
    assert crit.smoothing == 0.1 and crit.confidence == 0.9


def test_mixup_target_function_matches_its_formula():
    y = torch.tensor([2, 0, 1, 1])
    got = mixup_target(y, 3, lam=0.3, smoothing=0.1, device="cpu")
    off, on = 0.1 / 3, 1. - 0.1 + 0.1 / 3
    y1 = torch.full((4, 3), off).scatter_(1, y.view(-1, 1), on)
    y2 = torch.full((4, 3), off).scatter_(1, y.flip(0).view(-1, 1), on)
    assert torch.equal(got, y1 * 0.3 + y2 * (1. - 0.3))


# ------------------------------------------------------------------ the fine-tune loop with mixup_fn
def _build_tiny(device, dtype):
    c = R.TINY
    m = T.VisionTransformer(img_size=c["img_size"], patch_size=c["patch_size"], embed_dim=c["embed_dim"], depth=c["depth"],
                            num_heads=c["num_heads"], mlp_ratio=4, qkv_bias=True, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6),
                            all_frames=c["all_frames"], tubelet_size=c["tubelet_size"], num_classes=c["num_classes"], init_scale=1.0)
    shapes = R.vit_param_shapes(c["embed_dim"], c["depth"], c["num_classes"], tubelet=c["tubelet_size"], patch=c["patch_size"])
    m.load_state_dict(R.params_for(shapes, seed=3), strict=False)
    return m.to(device=device, dtype=dtype)


def run_g14_trajectory(model, device, dtype, criterion, fused_kernel=None, scaler=None):
    c = R.G12
    opt = E.create_optimizer(model, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"], fused_kernel=fused_kernel)
    lr_sched = E.cosine_scheduler(c["base_lr"], c["min_lr"], 1, c["steps"], warmup_epochs=c["warmup_epochs"],
                                  start_warmup_value=c["start_warmup_value"], warmup_steps=c["warmup_steps"])
    wd_sched = E.cosine_scheduler(c["weight_decay"], c["weight_decay_end"], 1, c["steps"])
    np.random.seed(MR.TRAJECTORY_SEED)
    stats = E.train_one_epoch(model, criterion, R.g12_batches(dtype), opt, device, 0, scaler or E.NativeScalerWithGradNormCount(model),
                              max_norm=c["clip_grad"], start_steps=0, lr_schedule_values=lr_sched, wd_schedule_values=wd_sched,
                              num_training_steps_per_epoch=c["steps"], update_freq=c["update_freq"], mixup_fn=Mixup(**MR.TRAJECTORY_MIXUP))
    return opt, stats


def check_g14_logged(stats, g, loss_tol, norm_rtol, loss_scaled=False):
    assert np.allclose(stats["loss"], g["traj.loss"], rtol=0, atol=loss_tol), (stats["loss"], g["traj.loss"])
    got = np.array([np.nan if n is None else n for n in stats["grad_norm"]])
    assert np.array_equal(np.isnan(got), np.isnan(g["traj.grad_norm"]))
    ok = ~np.isnan(got)
    assert np.allclose(got[ok], g["traj.grad_norm"][ok], rtol=norm_rtol), (got, g["traj.grad_norm"])
    assert np.allclose(stats["lr"], g["traj.lr"], rtol=1e-12)
    assert stats["class_acc"] == [None] * len(g["traj.loss"])                  # engine_for_finetuning.py:104-107
    avg = dict(zip([str(k) for k in g["traj.avg_keys"]], g["traj.avg_vals"]))
    assert "class_acc" not in avg and "class_acc" not in stats["averaged"]
    for k in ("loss", "lr", "min_lr", "grad_norm") + (() if loss_scaled else ("loss_scale",)):
        assert abs(stats["averaged"][k] - avg[k]) <= max(loss_tol, norm_rtol * abs(avg[k])), (k, stats["averaged"][k], avg[k])


def test_train_one_epoch_with_mixup_follows_the_reference_trajectory_around_the_oracle(golden):
    g = golden("g14_mixup")
    c = R.TINY
    m = _build_tiny("cpu", torch.float64)
    kw = dict(depth=c["depth"], num_heads=c["num_heads"], tubelet=c["tubelet_size"], patch=c["patch_size"])

    def oracle_forward(x):
        P = dict(m.named_parameters())
        return F.linear(O.forward_features(x, P, **kw), P["head.weight"], P["head.bias"])

    m.forward = oracle_forward
    opt, stats = run_g14_trajectory(m, torch.device("cpu"), torch.float64, SoftTargetCrossEntropy(), fused_kernel=False)
    assert np.random.rand() == float(g["traj.next"])
    check_g14_logged(stats, g, loss_tol=1e-12, norm_rtol=1e-10)
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g["traj.keys"]]
    for k, p in m.named_parameters():
        R.check_summary(p, g, "traj.after." + k, rtol=2e-6)


def test_default_loop_is_unchanged_without_mixup_fn():
    import inspect
    p = inspect.signature(E.train_one_epoch).parameters
    assert list(p)[-1] == "mixup_fn" and p["mixup_fn"].default is None


# ------------------------------------------------------------------ host validation of the C entry points
@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _plan(rows):
    tab = np.zeros((len(rows), 12), dtype=np.int32)
    for s, (kind, ws, wo, box, lam, oml) in enumerate(rows):
        tab[s, 0] = kind
        tab.view(np.float32)[s, 1:3] = (ws, wo)
        tab[s, 3:9] = box
        tab.view(np.float32)[s, 9:11] = (lam, oml)
    return tab


def test_host_validation_of_the_mixup_entry_points(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.tad_last_error_string
    assert lib.tad_mixup_clips(None, p, 2, 3, 4, 8, 8, None) == -1 and b"null" in err()
    assert lib.tad_mixup_clips(p, p, 3, 3, 4, 8, 8, None) == -1 and b"B=3" in err()
    assert lib.tad_mixup_clips(p, p, 2, 3, 0, 8, 8, None) == -1 and b"T=0" in err()
    assert lib.tad_mixup_clips(p, p, 2, 3, 16, 8192, 8192, None) == -1 and b"2^31" in err()
    assert lib.tad_mixup_clips(ctypes.c_void_p(p.value + 2), p, 2, 3, 4, 8, 8, None) == -1 and b"aligned" in err()
    good = (1, 0.25, 0.75, (0, 4, 0, 8, 0, 8), 0.25, 0.75)
    ok = _plan([good, good])
    assert lib.tad_mixup_plan_check(ok.ctypes.data, 2, 4, 8, 8) == 0
    assert lib.tad_mixup_plan_check(None, 2, 4, 8, 8) == -1 and b"null" in err()
    assert lib.tad_mixup_plan_check(_plan([good] * 3).ctypes.data, 3, 4, 8, 8) == -1 and b"B=3" in err()
    bad = _plan([good, (1, float("nan"), 0.75, (0, 4, 0, 8, 0, 8), 0.25, 0.75)])
    assert lib.tad_mixup_plan_check(bad.ctypes.data, 2, 4, 8, 8) == -1 and b"non-finite" in err() and b"sample 1" in err()
    bad = _plan([(2, 0., 1., (0, 4, 2, 9, 0, 8), 0.5, 0.5), good])
    assert lib.tad_mixup_plan_check(bad.ctypes.data, 2, 4, 8, 8) == -1 and b"outside the clip" in err()
    bad = _plan([(2, 0., 1., (0, 4, 5, 3, 0, 8), 0.5, 0.5), good])
    assert lib.tad_mixup_plan_check(bad.ctypes.data, 2, 4, 8, 8) == -1 and b"outside the clip" in err()
    bad = _plan([(7, 0., 1., (0, 4, 0, 8, 0, 8), 0.5, 0.5), good])
    assert lib.tad_mixup_plan_check(bad.ctypes.data, 2, 4, 8, 8) == -1 and b"kind=7" in err()
    assert lib.tad_mixup_target(p, None, p, 2, 5, 0.9, 0.02, None) == -1 and b"null" in err()
    assert lib.tad_mixup_target(p, p, p, 3, 5, 0.9, 0.02, None) == -1 and b"B=3" in err()
    assert lib.tad_mixup_target(p, p, p, 2, 0, 0.9, 0.02, None) == -1 and b"num_classes" in err()
    assert lib.tad_mixup_target(p, p, p, 2, 5, float("inf"), 0.02, None) == -1 and b"finite" in err()
    assert lib.tad_soft_target_ce(None, p, None, 0.0, p, p, 2, 5, None) == -1 and b"null" in err()
    assert lib.tad_soft_target_ce(p, p, p, 0.0, p, p, 2, 5, None) == -1 and b"exactly one" in err()
    assert lib.tad_soft_target_ce(p, None, None, 0.0, p, p, 2, 5, None) == -1 and b"exactly one" in err()
    assert lib.tad_soft_target_ce(p, p, None, 0.0, p, p, 2, 1, None) == -1 and b"num_classes=1" in err()
    assert lib.tad_soft_target_ce(p, None, p, 1.0, p, p, 2, 5, None) == -1 and b"smoothing" in err()


def test_plan_table_wrapper_checks_on_the_host(lib):
    from simple_tad_amd import kernels as K
    from simple_tad_amd._lib import TadError
    tab = K.mixup_plan_table([(1, 0.25, 0.75, (0, 4, 0, 8, 0, 8), 0.25, 0.75)] * 2, 4, 8, 8)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (2, 12) and tab[0, 0] == 1
    assert tab.view(torch.float32)[1, 2] == 0.75
    with pytest.raises(TadError, match="outside the clip"):
        K.mixup_plan_table([(2, 0., 1., (0, 5, 0, 8, 0, 8), 0.5, 0.5)] * 2, 4, 8, 8)
    with pytest.raises(TadError, match="GPU tensor"):
        K.mixup_clips(torch.zeros(2, 3, 4, 8, 8), tab)
