"""The frame fine-tuning losses on the MI355X: ``tad_frame_loss`` against the fp64 statement of tests/frame_loss_recipe.py under the
rule of ``test_soft_target_ce_is_as_close_to_fp64_as_torch_f32``, planted rows, guard bands, determinism, one C call and no host sync
per forward + backward, and the three G19 trajectories of the reference's frame engine through the HIP path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_loss_recipe as FR
import simple_tad_amd as T
from guarded import GuardedArena, same_bits
from simple_tad_amd import engine as E
from simple_tad_amd import kernels as K
from simple_tad_amd import loss as L
from test_frame_loss_cpu import call, check_g19_logged, module_for, run_g19_trajectory, trajectory_switches
from test_mixup_cpu import _build_tiny

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2), (2, 2), (7, 2), (64, 2), (65, 2), (257, 2), (5, 7)]
SHAPE_CONFIGS = [(B, C, n) for B, C in SHAPES for n in FR.configs_for(C)]
F32_TINY = 1.5e-45      # the smallest f32 subnormal: what an f32 result may differ by from ANY real number near zero


def kernel_operands(name, logits, labels, ttc, soft, device="cuda"):
    """(kind, operand tensors, scalars) of a recipe configuration (its name, or a dict like the recipe's) for K.frame_loss"""
    cfg = FR.CONFIGS[name] if isinstance(name, str) else name
    kind = cfg["kind"]
    ops = {}
    if kind != "2bce":
        ops["labels"] = labels.to(device)
    if kind == "2bce":
        ops["soft"] = soft.to(device)
    if kind == "exponential":
        ops["ttc"] = ttc.float().to(device)
    if kind == "focal2":
        ops["class_alpha"] = torch.tensor(FR.class_alpha_for(cfg, logits.shape[1]), dtype=torch.float32, device=device)
    return kind, ops, {k: v for k, v in cfg.items() if k not in ("kind", "class_alpha")}


def torch_f32(name, z, labels, ttc, soft):
    """the reference's expression, restated, evaluated by torch in f32 on the device of ``z``"""
    cfg = FR.CONFIGS[name]
    kind = cfg["kind"]
    if kind in ("focal", "focal2"):
        ce = F.cross_entropy(z, labels, reduction="none")
        pt = torch.exp(-ce)
        if kind == "focal":
            return torch.mean(cfg["multiplier"] * cfg["alpha"] * ((1 - pt) ** cfg["gamma"]) * ce)
        at = torch.tensor(FR.class_alpha_for(cfg, z.shape[1]), dtype=z.dtype, device=z.device)[labels]
        return torch.mean(((1 - pt) ** cfg["gamma"]) * (at * ce) * cfg["multiplier"])
    if kind == "exponential":
        ce = F.cross_entropy(z, labels, reduction="none")
        w = torch.ones_like(labels, dtype=torch.float)
        w[ttc < 0] = torch.exp(cfg["alpha_pre"] * ttc[ttc < 0])
        w[ttc > 0] = torch.exp(-cfg["alpha_post"] * ttc[ttc > 0])
        return (ce * torch.clamp(w, max=1.0)).mean()
    if kind == "2bce":
        bce = torch.nn.BCEWithLogitsLoss(reduction="none")
        return (bce(z[:, 0], soft[:, 0]) + bce(z[:, 1], soft[:, 1])).mean()
    p = F.softmax(z, dim=1)[:, 1]
    pos, neg = p[labels == 1], torch.sort(p[labels == 0])[0]
    loss = z.sum() * 0.0
    for pp in pos:
        loss = loss + torch.sum(torch.relu(neg - pp + cfg["delta"]))
    return loss / (pos.shape[0] if pos.shape[0] > 0 else 1.0)


def _rel(got, ref):
    return abs(got - ref) / abs(ref) if ref != 0 else abs(got)


def _errors(name, B, C):
    """relative errors against the fp64 statement, of the kernel (through the module) and of torch's own f32 evaluation of the
    reference's expression on the same inputs and device: RMS over the batches for the loss, relative L2 over all gradient elements
    of all batches.  At least 4 batches and at least 64 rows in all, so that the figure of a one-row batch is a statistic too."""
    err = {"kernel": [[], 0.0, 0.0], "torch": [[], 0.0, 0.0]}
    crit = module_for(name, C)
    for k in range(max(4, -(-64 // B))):
        logits, labels, ttc, soft = FR.inputs(f"gpu.{B}x{C}.{k}", B, C)
        ttc = ttc.float()                                             # the kernel's operand; all three evaluations take these values
        ref, ref_grad = FR.loss_and_grad_fp64(name, logits, labels, ttc, soft)
        dev = [t.cuda() for t in (labels, ttc, soft)]
        za = logits.cuda().requires_grad_()
        a = call(crit, name, za, *dev)
        assert a.grad_fn is not None and "FrameLoss" in type(a.grad_fn).__name__         # the HIP route, not the torch expression
        a.backward()
        zb = logits.cuda().requires_grad_()
        b = torch_f32(name, zb, *dev)
        b.backward()
        for who, loss, grad in (("kernel", a, za.grad), ("torch", b, zb.grad)):
            err[who][0].append(_rel(loss.item(), ref.item()))
            err[who][1] += (grad.double().cpu() - ref_grad).pow(2).sum().item()
            err[who][2] += ref_grad.pow(2).sum().item()
    return {n: (float(np.sqrt(np.mean(np.square(e[0])))), float(np.sqrt(e[1] / e[2])) if e[2] > 0 else float(np.sqrt(e[1]))) for n, e in err.items()}


@pytest.mark.parametrize("B,C,name", SHAPE_CONFIGS, ids=[f"{b}x{c}.{n}" for b, c, n in SHAPE_CONFIGS])
def test_frame_loss_is_as_close_to_fp64_as_torch_f32(B, C, name):
    """The kernel may lie twice as far from the fp64 value as torch's own f32 evaluation of the reference's expression does on the same
    inputs and device.  Measured on the MI355X (kernel / torch; loss: RMS relative error over the batches, gradient: relative L2):
      1x2 focal        loss 2.4e-08 / 4.8e-06   gradient 2.4e-08 / 6.3e-08
      1x2 focal6x100   loss 2.6e-08 / 1.2e-05   gradient 3.0e-08 / 1.5e-07
      1x2 focal_g1     loss 2.4e-08 / 3.0e-06   gradient 3.1e-08 / 5.6e-08
      1x2 focal2_6     loss 4.0e-08 / 1.2e-05   gradient 3.6e-08 / 1.6e-07
      1x2 focal2_2     loss 4.1e-08 / 4.8e-06   gradient 4.0e-08 / 7.0e-08
      1x2 2bce         loss 2.7e-08 / 7.3e-08   gradient 2.1e-08 / 3.8e-08
      1x2 smoothap     loss 0.0e+00 / 0.0e+00   gradient 0.0e+00 / 0.0e+00
      1x2 exponential1 loss 4.6e-08 / 1.3e-06   gradient 2.5e-08 / 3.9e-08
      2x2 focal        loss 2.5e-08 / 5.4e-07   gradient 2.4e-08 / 7.0e-08
      2x2 focal6x100   loss 2.6e-08 / 1.1e-06   gradient 2.8e-08 / 1.2e-07
      2x2 focal_g1     loss 2.1e-08 / 3.8e-07   gradient 2.9e-08 / 5.6e-08
      2x2 focal2_6     loss 4.0e-08 / 1.1e-06   gradient 3.0e-08 / 1.2e-07
      2x2 focal2_2     loss 3.7e-08 / 5.3e-07   gradient 4.2e-08 / 7.6e-08
      2x2 2bce         loss 2.6e-08 / 4.5e-08   gradient 2.2e-08 / 4.3e-08
      2x2 smoothap     loss 1.9e-08 / 1.1e-07   gradient 2.1e-08 / 1.1e-07
      2x2 exponential1 loss 2.3e-08 / 4.1e-07   gradient 2.4e-08 / 4.4e-08
      7x2 focal        loss 2.8e-08 / 7.4e-08   gradient 1.7e-08 / 9.1e-08
      7x2 focal6x100   loss 2.4e-08 / 1.1e-07   gradient 2.0e-08 / 1.1e-07
      7x2 focal_g1     loss 2.5e-08 / 5.6e-08   gradient 3.0e-08 / 7.7e-08
      7x2 focal2_6     loss 4.2e-08 / 9.8e-08   gradient 4.3e-08 / 1.2e-07
      7x2 focal2_2     loss 3.9e-08 / 1.2e-07   gradient 4.1e-08 / 9.8e-08
      7x2 2bce         loss 2.3e-08 / 7.0e-08   gradient 2.7e-08 / 6.3e-08
      7x2 smoothap     loss 3.0e-08 / 8.4e-08   gradient 2.5e-08 / 7.6e-08
      7x2 exponential1 loss 2.8e-08 / 5.4e-08   gradient 1.9e-08 / 7.3e-08
     64x2 focal        loss 1.4e-08 / 5.8e-08   gradient 2.2e-08 / 5.9e-08
     64x2 focal6x100   loss 1.8e-08 / 3.1e-08   gradient 2.4e-08 / 1.3e-07
     64x2 focal_g1     loss 2.3e-08 / 3.8e-08   gradient 2.9e-08 / 5.7e-08
     64x2 focal2_6     loss 3.0e-08 / 5.9e-08   gradient 4.6e-08 / 1.3e-07
     64x2 focal2_2     loss 3.6e-08 / 5.7e-08   gradient 4.6e-08 / 6.9e-08
     64x2 2bce         loss 3.8e-08 / 3.8e-08   gradient 2.3e-08 / 5.1e-08
     64x2 smoothap     loss 2.4e-08 / 5.9e-08   gradient 2.9e-08 / 2.0e-07
     64x2 exponential1 loss 2.7e-08 / 2.7e-08   gradient 2.0e-08 / 4.9e-08
     65x2 focal        loss 2.5e-08 / 3.7e-08   gradient 2.4e-08 / 6.6e-08
     65x2 focal6x100   loss 2.7e-08 / 8.4e-08   gradient 2.5e-08 / 1.3e-07
     65x2 focal_g1     loss 2.5e-08 / 5.6e-08   gradient 2.9e-08 / 5.5e-08
     65x2 focal2_6     loss 3.6e-08 / 6.5e-08   gradient 4.1e-08 / 1.3e-07
     65x2 focal2_2     loss 4.7e-08 / 4.7e-08   gradient 3.8e-08 / 9.6e-08
     65x2 2bce         loss 3.4e-08 / 4.4e-08   gradient 2.2e-08 / 5.4e-08
     65x2 smoothap     loss 2.0e-08 / 6.5e-08   gradient 2.3e-08 / 1.5e-07
     65x2 exponential1 loss 1.7e-08 / 2.2e-08   gradient 2.3e-08 / 5.3e-08
    257x2 focal        loss 1.2e-08 / 5.3e-08   gradient 2.2e-08 / 6.8e-08
    257x2 focal6x100   loss 2.6e-08 / 2.6e-08   gradient 2.4e-08 / 1.3e-07
    257x2 focal_g1     loss 3.7e-08 / 7.3e-08   gradient 2.8e-08 / 6.0e-08
    257x2 focal2_6     loss 5.5e-08 / 6.9e-08   gradient 4.3e-08 / 1.3e-07
    257x2 focal2_2     loss 2.6e-08 / 6.1e-08   gradient 4.2e-08 / 7.0e-08
    257x2 2bce         loss 3.7e-08 / 5.0e-08   gradient 2.3e-08 / 5.5e-08
    257x2 smoothap     loss 2.4e-08 / 1.5e-07   gradient 2.8e-08 / 4.1e-07
    257x2 exponential1 loss 2.1e-08 / 5.1e-08   gradient 2.3e-08 / 5.1e-08
      5x7 focal        loss 2.2e-08 / 6.4e-08   gradient 2.2e-08 / 7.4e-08
      5x7 focal6x100   loss 2.4e-08 / 5.8e-08   gradient 2.4e-08 / 1.2e-07
      5x7 focal_g1     loss 2.8e-08 / 5.9e-08   gradient 2.4e-08 / 5.5e-08
      5x7 focal2_6     loss 2.9e-08 / 9.7e-08   gradient 3.9e-08 / 1.2e-07
      5x7 focal2_2     loss 2.5e-08 / 5.3e-08   gradient 3.8e-08 / 7.5e-08
      5x7 exponential1 loss 2.2e-08 / 5.3e-08   gradient 2.7e-08 / 4.9e-08
    (one-row SmoothAP batches have no pair: loss and gradient are exactly zero on both sides.)"""
    e = _errors(name, B, C)
    print(f"frame_loss {name} {B}x{C}: loss rel err kernel {e['kernel'][0]:.3e} torch {e['torch'][0]:.3e}; "
          f"grad rel-L2 kernel {e['kernel'][1]:.3e} torch {e['torch'][1]:.3e}")
    assert e["kernel"][0] <= 2 * e["torch"][0] and e["kernel"][1] <= 2 * e["torch"][1], e


# ------------------------------------------------------------------ planted rows
def _kernel(name_or_cfg, logits, labels=None, ttc=None, soft=None):
    kind, ops, scalars = kernel_operands(name_or_cfg, logits, labels, ttc, soft)
    loss, dz = K.frame_loss(kind, logits.cuda(), **ops, **scalars)
    return loss.cpu().double()[0], dz.cpu().double()


def _close(got, ref, rtol):
    return bool(((got - ref).abs() <= rtol * ref.abs() + F32_TINY).all())


@pytest.mark.parametrize("gamma", [1, 2, 6])
def test_focal_keeps_its_relative_accuracy_on_a_confident_row_and_on_a_wrong_one(gamma):
    """ce ~ 1.1e-7 (logits 20 / 4, label 0) and ce ~ 30 (logits -15 / 15, label 0): within 1e-5 relative of fp64 -- or, where the
    fp64 value is below f32's range (gamma 6: 75 * (1.1e-7)^7), within one f32 subnormal of it.  The literal 1 - exp(-ce) of the same
    row is 6 % off in f32."""
    cfg = dict(kind="focal", alpha=0.75, gamma=gamma, multiplier=100 if gamma == 6 else 1.)
    sure, wrong = torch.tensor([[20., 4.]]), torch.tensor([[-15., 15.]])
    y = torch.tensor([0])
    ce64 = torch.log1p(torch.exp(torch.tensor(-16., dtype=torch.float64)))
    assert abs(ce64.item() - 1.125e-7) < 1e-9
    naive = (1 - torch.exp(-ce64.float().cuda())).double().cpu()
    exact = -torch.expm1(-ce64)
    assert abs(naive - exact) > 1e-5 * exact                                       # the naive difference is NOT within 1e-5
    for z in (sure, wrong, torch.cat([sure, wrong])):
        yy = y.repeat(z.shape[0])
        ref, ref_grad = FR.loss_and_grad_fp64(cfg, z, yy)
        loss, dz = _kernel(cfg, z, yy)
        print(f"gamma {gamma} rows {z.shape[0]}: loss {loss.item():.9e} fp64 {ref.item():.9e}")
        assert torch.isfinite(dz).all() and _close(loss, ref, 1e-5) and _close(dz, ref_grad, 1e-5), (loss, ref, dz, ref_grad)
    if gamma < 6:
        assert loss > 0 and bool((dz[0] != 0).all())                               # the confident row still has its gradient


def test_bce_takes_logits_of_ten_thousand():
    z = torch.tensor([[1e4, -1e4], [-1e4, 1e4], [1e4, 1e4], [0.5, -1e4]])
    soft = torch.tensor([[0.3, 0.7], [1.0, 0.0], [0.0, 1.0], [0.25, 0.75]])
    ref, ref_grad = FR.loss_and_grad_fp64("2bce", z, soft=soft)
    loss, dz = _kernel("2bce", z, soft=soft)
    assert torch.isfinite(loss) and torch.isfinite(dz).all() and _close(loss, ref, 1e-6) and _close(dz, ref_grad, 1e-6), (loss, ref, dz, ref_grad)


def test_exponential_weights_at_the_edges_of_time():
    ttc = torch.tensor([-3., -0.0, 0., 2., float("nan"), float("inf")], dtype=torch.float64)
    logits, labels, _, _ = FR.inputs("planted.exp", 6, 2)
    ref, ref_grad = FR.loss_and_grad_fp64("exponential1", logits, labels, ttc)
    assert torch.isfinite(ref) and bool((ref_grad[5] == 0).all()) and bool((ref_grad[4] != 0).all())      # weight 0 at +inf, 1 at NaN
    z = logits.cuda().requires_grad_()
    loss = L.TemporalExponentialLoss()(z, labels.cuda(), ttc.cuda())                                         # f64 in, cast on the device
    loss.backward()
    assert _close(loss.detach().cpu().double(), ref, 1e-5) and _close(z.grad.cpu().double(), ref_grad, 1e-5)
    assert bool((z.grad[5] == 0).all())


@pytest.mark.parametrize("case", ["all_positive", "all_negative", "one_positive", "tied"])
def test_smoothap_edge_batches(case):
    logits, labels, _, _ = FR.inputs("planted.ap." + case, 9, 2)
    if case == "all_positive":
        labels[:] = 1
    elif case == "all_negative":
        labels[:] = 0
    elif case == "one_positive":
        labels[:] = 0
        labels[4] = 1
    else:
        logits[1] = logits[0]                       # identical rows, one positive and one negative: the pair sits at delta, not at 0
        assert labels[0] == 1 and labels[1] == 0
    FR.assert_off_hinge(logits, labels)
    ref, ref_grad = FR.loss_and_grad_fp64("smoothap", logits, labels)
    z = logits.cuda().requires_grad_()
    loss = L.SmoothAPLoss()(z, labels.cuda())
    loss.backward()
    assert _close(loss.detach().cpu().double(), ref, 1e-5) and _close(z.grad.cpu().double(), ref_grad, 1e-5), (loss, ref)
    if case.startswith("all_"):
        assert loss.item() == 0.0 and bool((z.grad == 0).all())
    else:
        assert loss.item() > 0


# ------------------------------------------------------------------ guard bands, determinism
@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("rows_classes", [(2, 2), (65, 2), (5, 7)])
def test_frame_loss_stays_inside_its_operands(rows_classes, poison):
    B, C = rows_classes
    logits, labels, ttc, soft = FR.inputs(f"guard.{B}x{C}", B, C)
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    for name in FR.configs_for(C):
        arena.reset()
        kind, ops, scalars = kernel_operands(name, logits, labels, ttc, soft, device="cpu")
        z = arena.place(logits, role="input", name="logits")
        placed = {k: arena.place(v, role="input", name=k, index_range=C if k == "labels" else None) for k, v in ops.items()}
        with arena.route(K):
            loss, dz = K.frame_loss(kind, z, **placed, **scalars)
        arena.verify()
        assert arena.contains(loss) and arena.contains(dz)
        ref, ref_grad = FR.loss_and_grad_fp64(name, logits, labels, ttc.float(), soft)
        assert _close(loss.cpu().double()[0], ref, 1e-5), (name, loss, ref)
        assert float((dz.cpu().double() - ref_grad).abs().max()) <= 1e-5 * float(ref_grad.abs().max()), name


@pytest.mark.parametrize("rows_classes", [(257, 2), (5, 7)])
def test_two_calls_give_the_same_bits(rows_classes):
    B, C = rows_classes
    logits, labels, ttc, soft = FR.inputs(f"det.{B}x{C}", B, C)
    for name in FR.configs_for(C):
        kind, ops, scalars = kernel_operands(name, logits, labels, ttc, soft)
        z = logits.cuda()
        a, b = K.frame_loss(kind, z, **ops, **scalars), K.frame_loss(kind, z, **ops, **scalars)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), name


# ------------------------------------------------------------------ one launch, no host sync
def test_forward_and_backward_are_one_c_call_and_never_wait_for_the_device(monkeypatch):
    """every module's forward + backward calls ``tad_frame_loss`` once (the entry point launches one kernel) and reads nothing back:
    torch refuses a host synchronisation inside the block.  FocalLoss2 with a list ``alpha`` included, after its first call."""
    from simple_tad_amd import _lib
    lib = _lib.load()
    real, calls = lib.tad_frame_loss, []
    monkeypatch.setattr(lib, "tad_frame_loss", lambda *a: (calls.append(a[0]), real(*a))[1])
    logits, labels, ttc, soft = FR.inputs("nosync", 56, 2)
    dev = [t.cuda() for t in (labels, ttc, soft)]           # ttc float64, as the datasets deliver it
    assert dev[1].dtype == torch.float64
    z = logits.cuda().requires_grad_()
    crits = {n: L.build_criterion(n) for n in L.LOSS_NAMES if n != "crossentropy"}
    assert isinstance(crits["focal2_6"].alpha, list)
    for n, crit in crits.items():                           # (first call: library load, allocator warm-up, FocalLoss2's device copy)
        call(crit, n, z, *dev).backward()
    torch.cuda.synchronize()
    calls.clear()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                   # the mode is live in this build: a host read of device memory is refused
            dev[0].sum().item()
        for _ in range(3):
            for n, crit in crits.items():
                call(crit, n, z, *dev).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(calls) == 3 * len(crits) and bool(torch.isfinite(z.grad).all())


# ------------------------------------------------------------------ the fine-tune loop
# the half-mode loss scale: 2^20 is where a GradScaler settles for this model under cross entropy (test_engine_trajectory.py); the
# gradients of focal6x100 are 16-30 times larger (G19 norms 29 .. 72 against 2 .. 5), so its scale is 32 times smaller
HALF_SCALE = {"focal6x100": 2.0 ** 15, "exponential": 2.0 ** 20, "2bce": 2.0 ** 20}


@pytest.mark.parametrize("mode", ["precise", "fast", "half"])
@pytest.mark.parametrize("name", list(FR.TRAJECTORIES))
def test_hip_path_follows_the_g19_trajectory(golden, name, mode):
    """per-mode tolerances = those test_mixup_gpu.py takes for the same model.  The golden losses are of order 1 (0.4 .. 1.7, focal6x100's
    x100 included), so the absolute loss tolerance is a relative one as well and is applied as it stands.
    Measured on the MI355X (largest loss deviation / largest relative gradient-norm deviation; precise, fast, half):
    focal6x100   1.7e-06 / 4.0e-07,  1.1e-03 / 1.4e-03,  2.0e-04 / 3.0e-04
    exponential  2.9e-07 / 5.4e-07,  2.1e-04 / 9.1e-05,  2.3e-05 / 1.2e-05
    2bce         2.4e-07 / 2.8e-07,  6.0e-05 / 4.7e-05,  1.1e-05 / 1.5e-05"""
    from simple_tad_amd.optim import FusedAdamW
    g = golden("g19_frame_losses")
    assert 0.3 < g[f"traj.{name}.loss"].min() and g[f"traj.{name}.loss"].max() < 2.0
    m = _build_tiny("cuda", torch.float32)
    T.set_precision(mode)
    try:
        sc = E.NativeScalerWithGradNormCount(m, init_scale=HALF_SCALE[name]) if mode == "half" else None
        opt, stats = run_g19_trajectory(m, torch.device("cuda"), torch.float32, L.build_criterion(FR.TRAJECTORIES[name]["loss"]), scaler=sc,
                                        **trajectory_switches(name))
        assert sc is None or sc.skipped_steps == 0
    finally:
        T.set_precision("fast")
    assert isinstance(opt, FusedAdamW)
    loss_tol, norm_rtol = {"precise": (2e-5, 1e-3), "fast": (3e-3, 2e-2), "half": (4e-4, 3e-3)}[mode]
    got = np.array([np.nan if n is None else n for n in stats["grad_norm"]])
    ok = ~np.isnan(got)
    print(name, mode, "loss deviation", np.abs(np.array(stats["loss"]) - g[f"traj.{name}.loss"]).max(), "norm deviation (relative)",
          np.abs(got[ok] / g[f"traj.{name}.grad_norm"][ok] - 1).max())
    if mode == "half":
        assert stats["averaged"]["loss_scale"] == HALF_SCALE[name]
    check_g19_logged(stats, g, name, loss_tol=loss_tol, norm_rtol=norm_rtol, loss_scaled=mode == "half")
    if mode == "precise":
        assert np.array_equal(np.array(stats["class_acc"]), g[f"traj.{name}.class_acc"])
