"""Mixup / CutMix and the soft-target loss on the MI355X: ``tad_mixup_clips`` / ``tad_mixup_target`` against the reference's results
(golden G14) and against the reference's torch expression at the real clip shape, bit for bit; guard bands around every operand of the
three kernels; ``tad_soft_target_ce`` against the fp64 formula; the G14 fine-tune trajectory through the HIP path; no host sync."""
import numpy as np
import pytest
import torch

import golden_recipe as R
import mixup_recipe as MR
import simple_tad_amd as T
from guarded import GuardedArena, same_bits
from simple_tad_amd import engine as E
from simple_tad_amd import kernels as K
from simple_tad_amd.loss import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
from simple_tad_amd.mixup import Mixup, mixup_target
from test_mixup_cpu import _build_tiny, check_g14_logged, run_g14_trajectory

pytestmark = pytest.mark.gpu
CASES = list(MR.cases())
REAL = (32, 3, 16, 224, 224)


@pytest.mark.parametrize("key,mode,name,seed,shape", CASES, ids=[c[0] for c in CASES])
def test_hip_mixup_reproduces_the_reference_bit_for_bit(golden, key, mode, name, seed, shape):
    g = golden("g14_mixup")
    x, y = MR.clip(key, shape).cuda(), MR.labels(key, shape[0]).cuda()
    assert Mixup._fused(x, y)
    fn = Mixup(**MR.mixup_kwargs(mode, name))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    np.random.seed(seed)
    out, target = fn(x, y)
    after = np.random.rand()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert out is x and out.data_ptr() == x.data_ptr()
    assert extra < x.numel() * 4, (extra, x.numel() * 4)          # the plan table and the targets, no temporary of the clip's size
    assert np.array_equal(MR.digest(x), g[f"{key}.sha"]) and np.array_equal(MR.sample(x), g[f"{key}.sample"])
    assert target.dtype == torch.float32 and np.array_equal(target.cpu().numpy(), g[f"{key}.target"])
    assert after == float(g[f"{key}.next"])


@pytest.mark.parametrize("mode", MR.MODES)
@pytest.mark.parametrize("name", ["mixup", "cutmix", "switch"])
def test_real_shape_matches_the_torch_expression_on_the_device(mode, name):
    """32 x 3 x 16 x 224^2: the kernel against the reference's torch expressions evaluated on the device on a copy"""
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(REAL, device="cuda", generator=gen)
    y = torch.randint(0, 400, (REAL[0],), device="cuda", generator=gen)
    fn = Mixup(**dict(MR.CONFIGS[name], mode=mode, label_smoothing=0.1, num_classes=400))
    np.random.seed(11)
    rows, lam = fn.plan(x.shape)
    assert any(r[0] != 0 for r in rows)
    want = x.clone()
    if mode == "batch" and rows[0][0] == 1:       # mixup.py:205-206, literally
        flipped = want.flip(0).mul_(1. - lam)
        want.mul_(lam).add_(flipped)
        del flipped
    else:
        fn._mix_torch(want, rows)
    lam_t = lam if isinstance(lam, float) else torch.tensor(lam, device="cuda", dtype=torch.float32).unsqueeze(1)
    want_target = mixup_target(y, 400, lam_t, 0.1, "cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    np.random.seed(11)
    out, target = fn(x, y)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < (1 << 20)     # 308 MB clip: nothing but the table and the targets
    assert out.data_ptr() == x.data_ptr() and torch.equal(x, want) and torch.equal(target, want_target)


# ------------------------------------------------------------------ guard bands
def _rows_for(shape, kinds):
    """one plan row per sample; kinds = list of (kind, box or None)"""
    T_, H, W = shape[2:]
    return [(k, np.float32(0.3), np.float32(1) - np.float32(0.3), (0, T_, 0, H, 0, W) if box is None else box, np.float32(0.3),
             np.float32(0.7)) for k, box in kinds]


def _expected(x_host, rows):
    want = x_host.clone()
    B = len(rows)
    for i, (kind, ws, wo, (t0, t1, y0, y1, x0, x1), _, _) in enumerate(rows):
        if kind == 1:
            want[i] = x_host[i] * float(ws) + x_host[B - 1 - i] * float(wo)
        elif kind == 2:
            want[i][:, t0:t1, y0:y1, x0:x1] = x_host[B - 1 - i][:, t0:t1, y0:y1, x0:x1]
    return want


GUARD_CASES = {
    # name: (shape, per-sample (kind, box), elements the clip's base is offset by)
    "blend_vec": ((4, 3, 4, 12, 16), [(1, None)] * 4, 0),
    "blend_odd_w": ((4, 3, 2, 5, 7), [(1, None)] * 4, 0),
    "blend_offset_4_bytes": ((2, 3, 4, 8, 16), [(1, None)] * 2, 1),
    "blend_and_keep": ((4, 2, 3, 6, 8), [(1, None), (0, None), (1, None), (0, None)], 0),
    "paste_borders_low": ((4, 3, 4, 12, 16), [(2, (0, 4, 0, 5, 0, 7))] * 4, 0),
    "paste_borders_high": ((4, 3, 4, 12, 16), [(2, (1, 4, 6, 12, 9, 16))] * 4, 0),
    "paste_inside_vector": ((2, 3, 4, 12, 16), [(2, (1, 3, 2, 9, 5, 6)), (2, (0, 2, 1, 4, 2, 15))], 0),
    "paste_whole": ((2, 3, 2, 6, 8), [(2, None)] * 2, 0),
    "paste_empty": ((2, 3, 4, 12, 16), [(2, (2, 2, 3, 9, 4, 8)), (2, (0, 4, 5, 5, 0, 16))], 0),
    "paste_odd_w_offset": ((2, 3, 3, 5, 9), [(2, (0, 2, 1, 5, 3, 9)), (1, None)], 1),
    "paste_pair_style": ((4, 3, 4, 12, 16), [(2, (1, 4, 3, 10, 0, 16)), (0, None), (0, None), (2, (1, 4, 3, 10, 0, 16))], 0),
}


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("case", list(GUARD_CASES))
def test_mixup_kernels_stay_inside_their_operands(case, poison):
    shape, kinds, offset = GUARD_CASES[case]
    rows = _rows_for(shape, kinds)
    x_host = MR.clip("guard." + case, shape)
    n = x_host.numel()
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    flat = arena.place(torch.cat([torch.full((offset,), 123.0), x_host.flatten()]), role="inout", name="clips")
    x = flat[offset:].view(shape)
    assert x.data_ptr() % 16 == (4 * offset) % 16 and x.is_contiguous()
    table = K.mixup_plan_table(rows, *shape[2:])
    plan = arena.place(table, role="input", name="plan", index_range=3)
    labels_host = MR.labels("guard." + case, shape[0])
    labels = arena.place(labels_host, role="input", name="labels", index_range=MR.NUM_CLASSES)
    with arena.route(K):
        K.mixup_clips(x, plan)
        target = K.mixup_target(plan, labels, MR.NUM_CLASSES, 0.92, 0.02)
    arena.verify()
    assert same_bits(x.cpu(), _expected(x_host, rows))
    assert offset == 0 or bool((flat[:offset] == 123.0).all())
    assert arena.contains(target)
    on, off = torch.tensor(0.92), torch.tensor(0.02)
    y1 = torch.where(torch.nn.functional.one_hot(labels_host, MR.NUM_CLASSES).bool(), on, off)
    y2 = torch.where(torch.nn.functional.one_hot(labels_host.flip(0), MR.NUM_CLASSES).bool(), on, off)
    assert same_bits(target.cpu(), y1 * float(np.float32(0.3)) + y2 * float(np.float32(0.7)))


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("rows_classes", [(2, 2), (5, 174), (33, 1000), (3, 67)])
def test_soft_target_ce_stays_inside_its_operands(rows_classes, poison):
    B, classes = rows_classes
    z_host = R.tensor_for(f"guard.ce.z{B}x{classes}", (B, classes), seed=4, scale=3.0)
    t_host = torch.softmax(R.tensor_for(f"guard.ce.t{B}x{classes}", (B, classes), seed=5), -1)
    y_host = torch.arange(B) % classes
    arena = GuardedArena(48 << 20, "cuda", poison=poison)
    z = arena.place(z_host, role="input", name="logits")
    t = arena.place(t_host, role="input", name="target")
    y = arena.place(y_host, role="input", name="labels", index_range=classes)
    with arena.route(K):
        loss, dz = K.soft_target_ce(z, target=t)
        loss_h, dz_h = K.soft_target_ce(z, labels=y, smoothing=0.1)
    arena.verify()
    z64 = z_host.double().requires_grad_()
    ref = torch.sum(-t_host.double() * torch.log_softmax(z64, -1), -1).mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item()) and (dz.cpu().double() - z64.grad).abs().max().item() < 1e-6
    z64 = z_host.double().requires_grad_()
    ref = LabelSmoothingCrossEntropy(0.1)(z64, y_host)
    ref.backward()
    assert abs(loss_h.item() - ref.item()) < 1e-5 * abs(ref.item()) and (dz_h.cpu().double() - z64.grad).abs().max().item() < 1e-6


# ------------------------------------------------------------------ the loss kernel against the fp64 statement
def _ce_errors(classes, batches=16, rows=32):
    """relative errors against the fp64 formula, of the kernel and of torch's own f32 evaluation of the same expression on the
    device: RMS over the batches for the loss, relative L2 over all gradient elements of all batches"""
    err = {"kernel": [[], 0.0, 0.0], "torch": [[], 0.0, 0.0]}
    for k in range(batches):
        z = R.tensor_for(f"ce.gpu.z{classes}", (rows, classes), seed=k, scale=3.0)
        z[0, 0], z[0, 1] = 60.0, -50.0      # a row with a large logit spread
        t = torch.softmax(R.tensor_for(f"ce.gpu.t{classes}", (rows, classes), seed=100 + k, scale=2.0), -1)
        z, t = z.cuda(), t.cuda()
        z64 = z.double().requires_grad_()
        ref = torch.sum(-t.double() * torch.log_softmax(z64, -1), -1).mean()
        ref.backward()
        za = z.clone().requires_grad_()
        a = SoftTargetCrossEntropy()(za, t)
        a.backward()
        zb = z.clone().requires_grad_()
        b = torch.sum(-t * torch.log_softmax(zb, -1), -1).mean()
        b.backward()
        for name, loss, grad in (("kernel", a, za.grad), ("torch", b, zb.grad)):
            err[name][0].append(((loss.double() - ref) / ref).item())
            err[name][1] += (grad.double() - z64.grad).pow(2).sum().item()
            err[name][2] += z64.grad.pow(2).sum().item()
    return {n: (float(np.sqrt(np.mean(np.square(e[0])))), float(np.sqrt(e[1] / e[2]))) for n, e in err.items()}


@pytest.mark.parametrize("classes", [2, 174, 400, 1000])
def test_soft_target_ce_is_as_close_to_fp64_as_torch_f32(classes):
    """The kernel may lie twice as far from the fp64 value as torch's own f32 evaluation of the same expression does on the same
    inputs and device (another summation order, nothing more).  Measured on the MI355X (loss RMS relative error over 16 batches of
    32 rows / gradient relative L2):
    classes    2: loss kernel 3.2e-08, torch 4.1e-08; gradient kernel 6.2e-08, torch 6.2e-08
    classes  174: loss kernel 3.1e-08, torch 4.1e-08; gradient kernel 7.4e-08, torch 8.5e-08
    classes  400: loss kernel 2.6e-08, torch 4.8e-08; gradient kernel 7.3e-08, torch 8.9e-08
    classes 1000: loss kernel 2.5e-08, torch 3.9e-08; gradient kernel 8.4e-08, torch 9.5e-08
    (with the row losses added in f32 instead of double the loss figures were 7.7e-08 / 6.3e-08 / 4.8e-08 / 7.8e-08.)"""
    e = _ce_errors(classes)
    print(f"soft_target_ce classes={classes}: loss rel err kernel {e['kernel'][0]:.3e} torch {e['torch'][0]:.3e}; "
          f"grad rel-L2 kernel {e['kernel'][1]:.3e} torch {e['torch'][1]:.3e}")
    assert e["kernel"][0] <= 2 * e["torch"][0] and e["kernel"][1] <= 2 * e["torch"][1], e


def test_label_smoothing_on_the_device_is_the_soft_loss_of_the_smoothed_row():
    z = R.tensor_for("ls.gpu.z", (32, 174), seed=1, scale=3.0).cuda()
    y = (torch.arange(32) * 7 % 174).cuda()
    t = torch.full((32, 174), 0.1 / 174, device="cuda")
    t[torch.arange(32), y] += 0.9
    za, zb = z.clone().requires_grad_(), z.clone().requires_grad_()
    a = LabelSmoothingCrossEntropy(0.1)(za, y)
    b = SoftTargetCrossEntropy()(zb, t)
    (a * 3).backward()
    (b * 3).backward()
    assert a.dim() == 0 and abs(a.item() - b.item()) <= 2e-7 * abs(b.item()) and torch.allclose(za.grad, zb.grad, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------ the fine-tune loop
@pytest.mark.parametrize("mode", ["precise", "fast", "half"])
def test_hip_path_follows_the_g14_trajectory(golden, mode):
    """per-mode tolerances = those of test_engine_trajectory.py for the same model without mixup"""
    from test_engine_trajectory import HALF_SCALE_G12
    from simple_tad_amd.optim import FusedAdamW
    g = golden("g14_mixup")
    m = _build_tiny("cuda", torch.float32)
    init = {k: p.detach().clone() for k, p in m.named_parameters()}
    T.set_precision(mode)
    try:
        sc = E.NativeScalerWithGradNormCount(m, init_scale=HALF_SCALE_G12) if mode == "half" else None
        opt, stats = run_g14_trajectory(m, torch.device("cuda"), torch.float32, SoftTargetCrossEntropy(), scaler=sc)
        assert sc is None or sc.skipped_steps == 0
    finally:
        T.set_precision("fast")
    assert isinstance(opt, FusedAdamW) and np.random.rand() == float(g["traj.next"])
    loss_tol, norm_rtol, step_tol = {"precise": (2e-5, 1e-3, 1e-3), "fast": (3e-3, 2e-2, 8.4e-2), "half": (4e-4, 3e-3, 4.5e-2)}[mode]
    print(mode, "loss deviation", np.abs(np.array(stats["loss"]) - g["traj.loss"]).max())
    check_g14_logged(stats, g, loss_tol=loss_tol, norm_rtol=norm_rtol, loss_scaled=mode == "half")
    worst = 0.0
    for k, p in m.named_parameters():
        head = torch.from_numpy(g[f"traj.after.{k}.head"]).double()
        n = head.numel()
        got, was = p.detach().double().cpu().flatten()[:n], init[k].double().cpu().flatten()[:n]
        e = ((got - head).norm() / (head - was).norm().clamp_min(1e-12)).item()
        worst = max(worst, e)
        assert e < step_tol, (k, e)
    print(mode, "worst parameter-update deviation (relative to the update)", worst)


@pytest.mark.parametrize("mode", MR.MODES)
def test_mixup_call_does_not_synchronise_with_the_host(mode):
    x = MR.clip("nosync", (8, 3, 4, 16, 16)).cuda()
    y = MR.labels("nosync", 8).cuda()
    fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=MR.NUM_CLASSES)
    np.random.seed(3)
    fn(x, y)            # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):     # the mode is live in this build: a host read of device memory is refused
            y.sum().item()
        for _ in range(4):
            fn(x, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
