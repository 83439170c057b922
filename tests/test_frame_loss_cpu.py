"""The frame fine-tuning losses without a GPU: the fp64 statement of tests/frame_loss_recipe.py against the reference's own classes
(golden G19, tools/make_goldens_frame_loss.py), this package's modules on CPU tensors against both, ``frame_targets`` against the
reference's ``data_utils``, ``build_criterion``, the host-side validation of ``tad_frame_loss``, and the two new switches of the
engine -- including the three G19 trajectories of the reference's ``engine_for_frame_finetuning`` around the fp64 oracle."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_loss_recipe as FR
import golden_recipe as R
import simple_tad_amd as T
from oracle import vit_oracle as O
from simple_tad_amd import engine as E
from simple_tad_amd import frame_targets as FT
from simple_tad_amd import loss as L
from test_mixup_cpu import _build_tiny

CASE_CONFIGS = [(case, name) for case, (B, classes) in FR.CASES.items() for name in FR.configs_for(classes)]


def module_for(name, classes=2):
    """this package's criterion of a recipe configuration"""
    cfg = FR.CONFIGS[name]
    kind = cfg["kind"]
    if kind == "focal":
        return L.FocalLoss(alpha=cfg["alpha"], gamma=cfg["gamma"], multiplier=cfg["multiplier"])
    if kind == "focal2":
        return L.FocalLoss2(alpha=FR.class_alpha_for(cfg, classes), gamma=cfg["gamma"], multiplier=cfg["multiplier"])
    if kind == "2bce":
        return L.DoubleBCELoss()
    if kind == "smoothap":
        return L.SmoothAPLoss(delta=cfg["delta"])
    return L.TemporalExponentialLoss(alpha_pre=cfg["alpha_pre"], alpha_post=cfg["alpha_post"])


def call(crit, name, z, labels, ttc, soft):
    kind = FR.CONFIGS[name]["kind"]
    if kind == "2bce":
        return crit(z, soft.to(z.dtype) if z.dtype == torch.float64 else soft)
    return crit(z, labels, ttc) if kind == "exponential" else crit(z, labels)


@pytest.mark.parametrize("case,name", CASE_CONFIGS, ids=[f"{c}.{n}" for c, n in CASE_CONFIGS])
def test_fp64_recipe_reproduces_the_reference(golden, case, name):
    """1e-6 relative, loss and every gradient element (the reference's exponential weights are f32 values, 1e-7 from fp64's)"""
    g = golden("g19_frame_losses")
    B, classes = FR.CASES[case]
    logits, labels, ttc, soft = FR.inputs(case, B, classes)
    loss, grad = FR.loss_and_grad_fp64(name, logits, labels, ttc, soft)
    want_loss, want_grad = float(g[f"loss.{case}.{name}"]), g[f"grad.{case}.{name}"]
    assert want_loss > 0 and np.abs(want_grad).max() > 0
    assert abs(loss.item() - want_loss) <= 1e-6 * abs(want_loss), (loss.item(), want_loss)
    assert np.allclose(FR.np64(grad), want_grad, rtol=1e-6, atol=1e-12 * np.abs(want_grad).max())


@pytest.mark.parametrize("case,name", CASE_CONFIGS, ids=[f"{c}.{n}" for c, n in CASE_CONFIGS])
def test_modules_on_cpu_tensors_match_the_reference_and_the_recipe(golden, case, name):
    """f32 logits: the torch expression in f32 against G19.  A loss is a chain of about ten f32 operations whose errors (6e-8 each) the
    focal power magnifies by up to gamma + 1 = 7: 1e-5 relative on the loss, 1e-5 of the gradient's norm on the gradient.
    fp64 logits: the expression itself against the recipe's closed-form gradient, through autograd."""
    g = golden("g19_frame_losses")
    B, classes = FR.CASES[case]
    logits, labels, ttc, soft = FR.inputs(case, B, classes)
    crit = module_for(name, classes)
    z = logits.clone().requires_grad_()
    loss = call(crit, name, z, labels, ttc, soft)
    loss.backward()
    want_loss, want_grad = float(g[f"loss.{case}.{name}"]), g[f"grad.{case}.{name}"]
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss), (loss.item(), want_loss)
    assert np.linalg.norm(FR.np64(z.grad) - want_grad) <= 1e-5 * np.linalg.norm(want_grad)
    z64 = logits.double().requires_grad_()
    loss64 = call(crit, name, z64, labels, ttc, soft)
    loss64.backward()
    ref_loss, ref_grad = FR.loss_and_grad_fp64(name, logits, labels, ttc, soft)
    tol = 1e-6 if FR.CONFIGS[name]["kind"] == "exponential" else 1e-9      # (the f32 weight vector of the reference's expression)
    assert abs(loss64.item() - ref_loss.item()) <= tol * abs(ref_loss.item())
    assert np.allclose(FR.np64(z64.grad), FR.np64(ref_grad), rtol=tol, atol=1e-12 * float(ref_grad.abs().max()))


def test_reductions_and_small_gamma_take_the_torch_expression():
    logits, labels, _, _ = FR.inputs("b8", 8, 2)
    z = logits.double()
    ce = F.cross_entropy(z, labels, reduction="none")
    rows = 0.75 * (1 - torch.exp(-ce)) ** 2 * ce
    assert torch.allclose(L.FocalLoss(alpha=0.75, reduction="none")(z, labels), rows, rtol=1e-12)
    assert torch.allclose(L.FocalLoss(alpha=0.75, reduction="sum")(z, labels), rows.sum(), rtol=1e-12)
    at = torch.tensor([0.4, 0.6], dtype=torch.float64)[labels]
    assert torch.allclose(L.FocalLoss2(reduction="sum", gamma=0.5)(z, labels), ((1 - torch.exp(-ce)) ** 0.5 * at * ce).sum(), rtol=1e-12)
    assert torch.allclose(L.FocalLoss2(alpha=None)(z, labels), ((1 - torch.exp(-ce)) ** 2 * ce).mean(), rtol=1e-12)


def test_constructors_keep_the_reference_surface():
    f, f2, ap, ex, bce = L.FocalLoss(), L.FocalLoss2(), L.SmoothAPLoss(), L.TemporalExponentialLoss(), L.DoubleBCELoss(alpha=3, gamma=1, reduction="sum", multiplier=2.)
    assert (f.alpha, f.gamma, f.reduction, f.multiplier) == (1, 2, "mean", 1.)
    assert (f2.alpha, f2.gamma, f2.reduction, f2.multiplier) == ([0.40, 0.60], 2, "mean", 1.)
    assert ap.delta == 0.01 and (ex.alpha_pre, ex.alpha_post, ex.max_time_pre, ex.max_time_post) == (0.1, 0.5, 1.0, 0.5)
    assert T.FocalLoss is L.FocalLoss and T.build_criterion is L.build_criterion and T.frame_targets is FT
    z = torch.zeros(2, 2)
    assert bce(z, torch.full((2, 2), 0.5)).item() == pytest.approx(2 * np.log(2), rel=1e-6)     # the arguments are unused: a mean


def test_smoothap_without_a_positive_row_is_a_zero_that_can_be_differentiated():
    z = torch.randn(4, 2, requires_grad=True)
    loss = L.SmoothAPLoss()(z, torch.zeros(4, dtype=torch.int64))
    loss.backward()
    assert isinstance(loss, torch.Tensor) and loss.item() == 0.0 and bool((z.grad == 0).all())


def test_build_criterion_covers_the_eight_names():
    want = {"crossentropy": (torch.nn.CrossEntropyLoss, {}), "focal": (L.FocalLoss, dict(alpha=0.75, gamma=2, multiplier=1.)),
            "focal6x100": (L.FocalLoss, dict(alpha=0.75, gamma=6, multiplier=100)),
            "focal2_6": (L.FocalLoss2, dict(alpha=[0.40, 0.60], gamma=6, multiplier=50)),
            "focal2_2": (L.FocalLoss2, dict(alpha=[0.40, 0.60], gamma=2, multiplier=10)), "2bce": (L.DoubleBCELoss, {}),
            "smoothap": (L.SmoothAPLoss, dict(delta=0.01)), "exponential1": (L.TemporalExponentialLoss, dict(alpha_pre=0.1, alpha_post=0.5))}
    assert set(want) == set(L.LOSS_NAMES) and len(L.LOSS_NAMES) == 8
    for name, (cls, attrs) in want.items():
        crit = L.build_criterion(name)
        assert type(crit) is cls and all(getattr(crit, k) == v for k, v in attrs.items()), name
        if name not in ("crossentropy",):
            assert getattr(crit, "reduction", "mean") == "mean"
    with pytest.raises(NotImplementedError, match="focal3"):
        L.build_criterion("focal3")


# ------------------------------------------------------------------ targets
@pytest.mark.parametrize("case", list(FR.TARGET_CASES))
def test_frame_targets_match_the_reference(golden, case):
    g = golden("g19_frame_losses")
    labels, fps, TT, TA = FR.TARGET_CASES[case]
    tv = FT.compute_time_vector(labels, fps, TT, TA)
    assert tv.dtype == torch.float64 and np.array_equal(tv.numpy(), g[f"tv.{case}"])
    assert np.array_equal(FT.compute_time_vector(np.array(labels), fps, TT, TA).numpy(), g[f"tv.{case}"])
    for k, (before, after) in enumerate(FR.SMOOTH_LIMITS):
        sm = FT.smooth_labels(torch.tensor(labels), tv, before, after)
        assert sm.dtype == torch.float32 and np.allclose(sm.numpy(), g[f"sm.{case}.{k}"], rtol=0, atol=1e-7)
    if case == "none_10":
        assert not tv.any()
    else:
        assert (tv == 0).sum() == sum(labels) and (tv == FT.OUTSIDE).any() and ((tv > FT.OUTSIDE) & (tv < 0)).any() == (labels[0] == 0)


def test_target_cases_cover_what_they_should():
    c = FR.TARGET_CASES
    assert sum(c["none_10"][0]) == 0 and c["start_10"][0][0] == 1 and c["end_10"][0][-1] == 1
    assert {v[1] for v in c.values()} == {10, 30}
    assert np.count_nonzero(np.diff(c["two_10"][0]) == 1) == 2


# ------------------------------------------------------------------ host validation of the C entry point
@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_host_validation_of_tad_frame_loss(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = lambda n: ctypes.c_void_p(p.value + n)  # noqa: E731
    err = lib.tad_last_error_string
    FOCAL, FOCAL2, EXP, BCE, AP = 0, 1, 2, 3, 4

    def rc(kind, logits=p, labels=p, soft=None, ttc=None, ca=None, alpha=1., gamma=2., mult=1., pre=0.1, post=0.5, delta=0.01, loss=p, dz=p, B=4, C=2):
        return lib.tad_frame_loss(kind, logits, labels, soft, ttc, ca, alpha, gamma, mult, pre, post, delta, loss, dz, B, C, None)

    assert rc(9) == -1 and b"unknown kind=9" in err()
    assert rc(-1) == -1 and b"unknown kind=-1" in err()
    assert rc(FOCAL, logits=None) == -1 and b"null" in err()
    assert rc(FOCAL, dz=None) == -1 and b"null" in err()
    assert rc(FOCAL, loss=None) == -1 and b"null" in err()
    assert rc(FOCAL, labels=None) == -1 and b"exactly" in err() and b"labels=0" in err()
    assert rc(FOCAL, soft=p) == -1 and b"exactly" in err() and b"soft=1" in err()
    assert rc(FOCAL, ca=p) == -1 and b"exactly" in err() and b"class_alpha=1" in err()
    assert rc(FOCAL2, ttc=p) == -1 and b"exactly" in err() and b"ttc=1" in err()
    assert rc(EXP) == -1 and b"exactly" in err() and b"ttc=0" in err()
    assert rc(BCE, soft=p) == -1 and b"exactly" in err() and b"labels=1" in err()
    assert rc(BCE, labels=None) == -1 and b"exactly" in err() and b"soft=0" in err()
    assert rc(AP, ttc=p) == -1 and b"exactly" in err()
    assert rc(FOCAL, B=0) == -1 and b"B=0" in err()
    assert rc(FOCAL, C=1) == -1 and b"num_classes=1" in err()
    assert rc(BCE, labels=None, soft=p, C=3) == -1 and b"num_classes=3" in err()
    assert rc(AP, C=7) == -1 and b"num_classes=7" in err()
    assert rc(FOCAL, gamma=float("nan")) == -1 and b"gamma=nan" in err()
    assert rc(FOCAL, gamma=-1.) == -1 and b"gamma=-1" in err()
    assert rc(FOCAL2, gamma=0.5) == -1 and b"gamma=0.5 below 1" in err()
    assert rc(FOCAL, mult=float("inf")) == -1 and b"multiplier=inf" in err()
    assert rc(FOCAL, mult=-2.) == -1 and b"multiplier=-2" in err()
    assert rc(AP, delta=-0.5) == -1 and b"delta=-0.5" in err()
    assert rc(AP, delta=float("nan")) == -1 and b"delta=nan" in err()
    assert rc(EXP, ttc=p, pre=float("inf")) == -1 and b"alpha_pre=inf" in err()
    assert rc(FOCAL, logits=off(2)) == -1 and b"aligned" in err()
    assert rc(FOCAL, labels=off(4)) == -1 and b"aligned" in err()
    assert rc(EXP, ttc=off(1)) == -1 and b"aligned" in err()
    assert rc(BCE, labels=None, soft=off(2)) == -1 and b"aligned" in err()
    assert rc(FOCAL2, ca=off(3)) == -1 and b"aligned" in err()
    assert rc(FOCAL, loss=off(2)) == -1 and b"aligned" in err()
    assert rc(FOCAL, dz=off(1)) == -1 and b"aligned" in err()
    # Every refusal above is TAD_EINVAL (-1), returned in front of the launch.  Where there is no device, the launch itself is what
    # fails, with TAD_ELAUNCH (-2) and the runtime's message: so a call that passes every check does reach it, and none of the refused
    # ones did.  (With a device present these host pointers must not be launched on, and the check is left to the GPU tests.)
    if not torch.cuda.is_available():
        assert rc(FOCAL) == -2 and b"frame_loss:" in err() and b"aligned" not in err()
        assert rc(BCE, labels=None, soft=p) == -2


def test_scalars_the_entry_point_refuses_take_the_torch_expression(monkeypatch):
    """a negative or non-finite multiplier / alpha / delta / alpha_pre never reaches tad_frame_loss: the route test is host arithmetic"""
    from simple_tad_amd import kernels as K
    monkeypatch.setattr(L, "_on_hip", lambda x: True)                       # as if the logits were f32 on the GPU
    monkeypatch.setattr(K, "frame_loss", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the kernel")))
    logits, labels, ttc, soft = FR.inputs("b8", 8, 2)
    inf, nan = float("inf"), float("nan")
    for crit in (L.FocalLoss(multiplier=-1.), L.FocalLoss(multiplier=inf), L.FocalLoss(alpha=nan), L.FocalLoss(gamma=nan), L.FocalLoss(gamma=0.5),
                 L.FocalLoss2(multiplier=-2.), L.FocalLoss2(alpha=[0.4, inf]), L.FocalLoss2(gamma=inf), L.SmoothAPLoss(delta=-0.1),
                 L.SmoothAPLoss(delta=inf)):
        crit(logits, labels)
    for crit in (L.TemporalExponentialLoss(alpha_pre=inf), L.TemporalExponentialLoss(alpha_post=nan)):
        crit(logits, labels, ttc)
    with pytest.raises(AssertionError, match="reached the kernel"):         # (the probe is live: an ordinary instance does take the route)
        L.FocalLoss()(logits, labels)


def test_wrapper_checks_on_the_host(lib):
    from simple_tad_amd import kernels as K
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match="unknown kind"):
        K.frame_loss("hinge", torch.zeros(2, 2))
    with pytest.raises(TadError, match="GPU tensor"):
        K.frame_loss("focal", torch.zeros(2, 2), labels=torch.zeros(2, dtype=torch.int64))


# ------------------------------------------------------------------ the engine
def _oracle_model():
    c = R.TINY
    m = _build_tiny("cpu", torch.float64)
    kw = dict(depth=c["depth"], num_heads=c["num_heads"], tubelet=c["tubelet_size"], patch=c["patch_size"])

    def oracle_forward(x):
        P = dict(m.named_parameters())
        return F.linear(O.forward_features(x, P, **kw), P["head.weight"], P["head.bias"])

    m.forward = oracle_forward
    return m


def run_g19_trajectory(model, device, dtype, criterion, batches=None, fused_kernel=None, scaler=None, **switches):
    c = R.G12
    opt = E.create_optimizer(model, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"], fused_kernel=fused_kernel)
    lr_sched = E.cosine_scheduler(c["base_lr"], c["min_lr"], 1, c["steps"], warmup_epochs=c["warmup_epochs"],
                                  start_warmup_value=c["start_warmup_value"], warmup_steps=c["warmup_steps"])
    wd_sched = E.cosine_scheduler(c["weight_decay"], c["weight_decay_end"], 1, c["steps"])
    stats = E.train_one_epoch(model, criterion, FR.trajectory_batches(dtype) if batches is None else batches, opt, device, 0,
                              scaler or E.NativeScalerWithGradNormCount(model), max_norm=c["clip_grad"], start_steps=0,
                              lr_schedule_values=lr_sched, wd_schedule_values=wd_sched, num_training_steps_per_epoch=c["steps"],
                              update_freq=c["update_freq"], **switches)
    return opt, stats


def trajectory_switches(name):
    t = FR.TRAJECTORIES[name]
    return dict(with_ttc=t["with_ttc"], smoothed_labels_for_loss=t["smoothed_labels_for_loss"])


def check_g19_logged(stats, g, name, loss_tol, norm_rtol, loss_scaled=False):
    pre = f"traj.{name}."
    assert np.allclose(stats["loss"], g[pre + "loss"], rtol=0, atol=loss_tol), (stats["loss"], g[pre + "loss"])
    got = np.array([np.nan if n is None else n for n in stats["grad_norm"]])
    assert np.array_equal(np.isnan(got), np.isnan(g[pre + "grad_norm"]))
    ok = ~np.isnan(got)
    assert np.allclose(got[ok], g[pre + "grad_norm"][ok], rtol=norm_rtol), (got, g[pre + "grad_norm"])
    assert np.allclose(stats["lr"], g[pre + "lr"], rtol=1e-12)
    avg = dict(zip([str(k) for k in g[pre + "avg_keys"]], g[pre + "avg_vals"]))
    for k in ("loss", "lr", "min_lr", "grad_norm") + (() if loss_scaled else ("loss_scale",)):
        assert abs(stats["averaged"][k] - avg[k]) <= max(loss_tol, norm_rtol * abs(avg[k])), (k, stats["averaged"][k], avg[k])


@pytest.mark.parametrize("name", list(FR.TRAJECTORIES))
def test_train_one_epoch_follows_the_reference_frame_engine_around_the_oracle(golden, name):
    """the reference's engine_for_frame_finetuning.train_one_epoch in fp64 on the CPU against this package's loop, modules (their
    torch expressions) and switches.  1e-6 on the loss: the reference's BCE returns an f32 value for f32 smoothed labels, and its
    exponential weights are f32."""
    g = golden("g19_frame_losses")
    m = _oracle_model()
    crit = L.build_criterion(FR.TRAJECTORIES[name]["loss"])
    opt, stats = run_g19_trajectory(m, torch.device("cpu"), torch.float64, crit, fused_kernel=False, **trajectory_switches(name))
    check_g19_logged(stats, g, name, loss_tol=1e-6, norm_rtol=1e-5)
    assert np.array_equal(np.array(stats["class_acc"]), g[f"traj.{name}.class_acc"])          # always against the hard targets
    assert abs(stats["averaged"]["class_acc"] - g[f"traj.{name}.class_acc"].mean()) < 1e-12
    for k, p in m.named_parameters():
        R.check_summary(p, g, f"traj.{name}.after.{k}", rtol=1e-4)


class _Recording(torch.nn.Module):
    """cross entropy against the arg-max of whatever target arrives; keeps every call's arguments"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, outputs, target, *rest):
        self.calls.append((target.detach().clone(),) + tuple(r.detach().clone() for r in rest))
        return F.cross_entropy(outputs, target.argmax(-1) if target.dim() == 2 else target)


def test_with_ttc_passes_the_time_to_the_anomaly_as_third_argument():
    crit = _Recording()
    batches = FR.trajectory_batches(torch.float64)
    run_g19_trajectory(_oracle_model(), torch.device("cpu"), torch.float64, crit, batches=batches, fused_kernel=False, with_ttc=True)
    assert len(crit.calls) == len(batches)
    for (target, *rest), (_, y, _, extra) in zip(crit.calls, batches):
        assert len(rest) == 1 and torch.equal(rest[0], extra["ttc"]) and torch.equal(target, y)


def test_smoothed_labels_change_the_loss_target_but_not_class_acc():
    batches = FR.trajectory_batches(torch.float64)
    plain, smooth = _Recording(), _Recording()
    _, a = run_g19_trajectory(_oracle_model(), torch.device("cpu"), torch.float64, plain, batches=batches, fused_kernel=False)
    _, b = run_g19_trajectory(_oracle_model(), torch.device("cpu"), torch.float64, smooth, batches=batches, fused_kernel=False,
                              smoothed_labels_for_loss=True)
    for (target,), (_, y, _, extra) in zip(smooth.calls, batches):
        assert torch.equal(target, extra["smoothed_labels"])
    assert all(len(c) == 1 and c[0].dim() == 1 for c in plain.calls)
    # batch 2 holds a frame 0.6 s before its anomaly: hard label 0, smoothed label 0.92 -- the loss sees another class there
    assert smooth.calls[2][0][1].argmax() == 1 and batches[2][1][1] == 0
    assert a["loss"][:2] == b["loss"][:2] and a["loss"][2] != b["loss"][2]
    assert a["class_acc"][:4] == b["class_acc"][:4]        # same weights up to the second step, accuracy against the hard targets in both


def test_defaults_reproduce_an_unchanged_run_exactly():
    import inspect
    p = inspect.signature(E.train_one_epoch).parameters
    assert p["with_ttc"].default is False and p["smoothed_labels_for_loss"].default is False
    v = inspect.signature(E.validation_one_epoch).parameters
    assert list(v) == ["data_loader", "model", "device", "criterion", "with_ttc", "smoothed_labels_for_loss"] and v["criterion"].default is None
    crit = torch.nn.CrossEntropyLoss()
    _, a = run_g19_trajectory(_oracle_model(), torch.device("cpu"), torch.float64, crit, batches=R.g12_batches(torch.float64), fused_kernel=False)
    _, b = run_g19_trajectory(_oracle_model(), torch.device("cpu"), torch.float64, crit, fused_kernel=False)   # extra_info present, unused
    for k in E.METER_NAMES:
        assert a[k] == b[k], k
    assert a["averaged"] == b["averaged"]


def test_validation_takes_the_criterion_and_the_switches(monkeypatch):
    from simple_tad_amd import metrics as M
    monkeypatch.setattr(M, "calculate_metrics", lambda preds, labels: (None,) * 9 + ((None,) * 4,))     # (its counting is a HIP kernel)
    m = _oracle_model()
    batches = FR.trajectory_batches(torch.float64)
    base, _, _ = E.validation_one_epoch(batches, m, torch.device("cpu"))
    rec = _Recording()
    with_ce, _, _ = E.validation_one_epoch(batches, m, torch.device("cpu"), criterion=rec)
    assert with_ce == base and all(len(c) == 1 for c in rec.calls)
    rec = _Recording()
    both, my, _ = E.validation_one_epoch(batches, m, torch.device("cpu"), criterion=rec, with_ttc=True, smoothed_labels_for_loss=True)
    for (target, ttc), (_, _, _, extra) in zip(rec.calls, batches):
        assert torch.equal(target, extra["smoothed_labels"]) and torch.equal(ttc, extra["ttc"])
    assert both["acc"] == base["acc"] and both["loss"] != base["loss"]
    ex, _, _ = E.validation_one_epoch(batches, m, torch.device("cpu"), criterion=L.TemporalExponentialLoss(), with_ttc=True)
    assert 0 < ex["loss"] <= base["loss"]         # weights at most 1
