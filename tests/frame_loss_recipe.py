"""Seeded inputs of the frame fine-tuning loss fixture G19 (tests/golden/g19_frame_losses.npz, written by
tools/make_goldens_frame_loss.py from the reference's own ``utils.FocalLoss`` / ``FocalLoss2`` / ``SmoothAPLoss`` /
``TemporalExponentialLoss`` / ``DoubleBCELoss`` and ``dataset/data_utils.py``), and an fp64 statement of the five formulas and of their
gradients with respect to the logits.  The fixture holds results only; every input is regenerated from here.

The fp64 statement is closed-form (no autograd), and it is written the way the kernel has to be written: ``1 - pt`` as ``-expm1(-ce)``,
``logsumexp`` through ``log1p`` of everything but one maximal element, so that it keeps its relative accuracy on a row with
``ce ~ 1e-7`` where the literal expression has lost half of fp64's digits."""
import numpy as np
import torch

import golden_recipe as R

# every --loss configuration of run_frame_finetuning.py:571-586 but plain cross entropy; `exponential1` = the default
# TemporalExponentialLoss (the reference's own call raises a TypeError); `focal_g1` adds the gamma == 1 edge of the kernel
CONFIGS = {
    "focal": dict(kind="focal", alpha=0.75, gamma=2, multiplier=1.),
    "focal6x100": dict(kind="focal", alpha=0.75, gamma=6, multiplier=100),
    "focal_g1": dict(kind="focal", alpha=1, gamma=1, multiplier=1.),
    "focal2_6": dict(kind="focal2", class_alpha=[0.40, 0.60], gamma=6, multiplier=50),
    "focal2_2": dict(kind="focal2", class_alpha=[0.40, 0.60], gamma=2, multiplier=10),
    "2bce": dict(kind="2bce"),
    "smoothap": dict(kind="smoothap", delta=0.01),
    "exponential1": dict(kind="exponential", alpha_pre=0.1, alpha_post=0.5),
}
TWO_CLASS_ONLY = ("2bce", "smoothap")
CASES = {"b8": (8, 2), "b33": (33, 2), "c7": (5, 7)}   # [B, classes]
TTC_VALUES = (-100., -1.8, -0.9, -0.2, 0., 0., 0.1, 0.45, 1.0, 3.0)
HINGE_MARGIN = 1e-5


def configs_for(classes):
    return [n for n, c in CONFIGS.items() if classes == 2 or c["kind"] not in TWO_CLASS_ONLY]


def class_alpha_for(cfg, classes):
    """the per-class weights of a focal2 configuration at ``classes`` classes (the reference's two, continued for the 7-class case)"""
    a = cfg.get("class_alpha")
    return None if a is None else [a[c] if c < len(a) else 0.25 + 0.1 * c for c in range(classes)]


def smoothap_margin(logits, labels, delta):
    """the smallest |p_j - p_i + delta| over (positive i, negative j) pairs, in fp64 (inf without a pair)"""
    z = logits.double()
    p = torch.sigmoid(z[:, 1] - z[:, 0])
    h = p[labels == 0].unsqueeze(0) - p[labels == 1].unsqueeze(1) + delta
    return float(h.abs().min()) if h.numel() else float("inf")


def assert_off_hinge(logits, labels, delta=0.01):
    """A CONDITION ON THE INPUTS of a SmoothAP comparison, not a tolerance: no pair may sit within 1e-5 of the hinge in fp64, or one f32
    ulp of a probability decides whether the pair is active and two correct evaluations differ by a whole 1/P in a gradient."""
    m = smoothap_margin(logits, labels, delta)
    assert m >= HINGE_MARGIN, f"a SmoothAP pair lies {m:.3e} from the hinge: choose other inputs"


def inputs(tag, B, classes, scale=2.0, delta=0.01):
    """(logits f32 [B,classes], labels int64 [B], ttc f64 [B], soft f32 [B,2]) of a seeded case.  Both classes 0 and 1 occur when
    B >= 2; the logits are the first seeded draw that keeps every SmoothAP pair off the hinge (two-class cases)."""
    g = torch.Generator().manual_seed(R._seed_for("g19.aux." + tag, 19))
    labels = torch.randint(0, classes, (B,), generator=g)
    if B >= 2:
        labels[0], labels[1] = 1, 0
    ttc = torch.tensor(TTC_VALUES, dtype=torch.float64)[torch.randint(0, len(TTC_VALUES), (B,), generator=g)]
    a = torch.sigmoid(2.0 * torch.randn(B, generator=g))
    a[::3] = (labels[::3] == 1).float()        # a third of the rows keep a hard 0 / 1 target
    soft = torch.stack((1 - a, a), dim=-1).float()
    for seed in range(64):
        logits = R.tensor_for("g19.z." + tag, (B, classes), seed=seed, scale=scale)
        if classes != 2 or smoothap_margin(logits, labels, delta) >= HINGE_MARGIN:
            break
    if classes == 2:
        assert_off_hinge(logits, labels, delta)
    return logits, labels, ttc, soft


# ------------------------------------------------------------------ the formulas in fp64, with their gradients
def _ce_terms(z, y):
    """(ce [B], d ce / d z [B,C]) with the relative accuracy of fp64 also where ce is tiny"""
    rows = torch.arange(z.shape[0])
    m, top = z.max(dim=1)
    e = torch.exp(z - m.unsqueeze(1))
    e[rows, top] = 0.0
    lse = torch.log1p(e.sum(dim=1))                      # logsumexp(z) - m
    ce = lse + (m - z[rows, y])
    d = torch.exp(z - m.unsqueeze(1) - lse.unsqueeze(1))
    d[rows, y] = torch.expm1(-ce)                        # softmax[y] - 1
    return ce, d


def loss_and_grad_fp64(name_or_cfg, logits, labels=None, ttc=None, soft=None):
    """(loss 0-dim, d loss / d logits [B,C]) of a configuration, fp64 tensors"""
    cfg = CONFIGS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg
    z = logits.double()
    B, C = z.shape
    kind = cfg["kind"]
    if kind in ("focal", "focal2"):
        ce, d = _ce_terms(z, labels)
        gamma = float(cfg["gamma"])
        if kind == "focal":
            k = torch.full((B,), float(cfg["multiplier"]) * float(cfg["alpha"]), dtype=torch.float64)
        else:
            ca = class_alpha_for(cfg, C)
            k = float(cfg["multiplier"]) * (torch.ones(B, dtype=torch.float64) if ca is None else torch.tensor(ca, dtype=torch.float64)[labels])
        u, pt = -torch.expm1(-ce), torch.exp(-ce)
        ug1 = torch.ones_like(u) if gamma == 1.0 else u ** (gamma - 1.0)
        row = k * ug1 * u * ce
        coef = k * (ug1 * u + gamma * ug1 * pt * ce)
        return row.mean(), coef.unsqueeze(1) * d / B
    if kind == "exponential":
        ce, d = _ce_terms(z, labels)
        t = ttc.double()
        w = torch.ones_like(t)
        w = torch.where(t < 0, torch.exp(cfg["alpha_pre"] * t), w)
        w = torch.where(t > 0, torch.exp(-cfg["alpha_post"] * t), w)
        w = torch.clamp(w, max=1.0)
        return (w * ce).mean(), w.unsqueeze(1) * d / B
    if kind == "2bce":
        assert C == 2
        t = soft.double()
        row = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
        return row.sum(dim=1).mean(), (torch.sigmoid(z) - t) / B
    if kind == "smoothap":
        assert C == 2
        dlt = float(cfg["delta"])
        diff = z[:, 1] - z[:, 0]
        p, q = torch.sigmoid(diff), torch.sigmoid(-diff)
        pos, neg = labels == 1, labels == 0
        P = max(int(pos.sum()), 1)
        h = p[neg].unsqueeze(0) - p[pos].unsqueeze(1) + dlt          # [positives, negatives]
        active = (h > 0).double()
        dp = torch.zeros(B, dtype=torch.float64)
        dp[pos] = -active.sum(dim=1) / P
        dp[neg] = active.sum(dim=0) / P
        g1 = dp * p * q
        return torch.relu(h).sum() / P, torch.stack((-g1, g1), dim=1)
    raise KeyError(kind)


# ------------------------------------------------------------------ the targets (frame_targets.py against dataset/data_utils.py)
def _ranges(n, *spans):
    v = [0] * n
    for a, b in spans:
        v[a:b] = [1] * (b - a)
    return v


TARGET_CASES = {   # name: (per-frame labels, fps, TT, TA)
    "none_10": (_ranges(40), 10, 2, 1),
    "start_10": (_ranges(60, (0, 7)), 10, 2, 1),
    "end_10": (_ranges(60, (52, 60)), 10, 2, 1),
    "middle_30": (_ranges(200, (90, 110)), 30, 2, 1),
    "two_10": (_ranges(90, (25, 31), (40, 44)), 10, 2, 1),
    "two_30": (_ranges(240, (70, 95), (180, 181)), 30, 2, 1),
    "wide_10": (_ranges(80, (30, 40)), 10, 1.5, 2.5),
}
SMOOTH_LIMITS = ((2, 1), (1.5, 2.5))     # (before_limit, after_limit) each time vector is smoothed with


# ------------------------------------------------------------------ the fine-tune trajectories of G19
# golden_recipe.G12's six micro-batches and schedules; the loader's fourth item carries the time to the anomaly and the smoothed labels
TRAJECTORIES = {
    "focal6x100": dict(loss="focal6x100", with_ttc=False, smoothed_labels_for_loss=False),
    "exponential": dict(loss="exponential1", with_ttc=True, smoothed_labels_for_loss=False),
    "2bce": dict(loss="2bce", with_ttc=False, smoothed_labels_for_loss=True),
}
TRAJECTORY_TTC = [[-1.5, 0.0], [0.0, 0.0], [-100., -0.6], [0.0, 0.4], [-0.2, 0.0], [0.0, 0.0]]    # 0 where G12's label is 1


def _smoothed(labels, t):
    a = (labels == 1).double()
    before, after = (t >= -2) & (t < 0), (t > 0) & (t <= 1)
    a = torch.where(before, 1 / (1 + torch.exp(-6 * (t + 1))), a)
    a = torch.where(after, 1 / (1 + torch.exp(-12 * (0.5 - t))), a)
    return torch.stack((1 - a, a), dim=-1).float()


def trajectory_batches(dtype=torch.float32):
    """G12's micro-batches as (samples, targets, None, {"ttc": f64 [2], "smoothed_labels": f32 [2,2]}), the tuple
    engine_for_frame_finetuning iterates over"""
    out = []
    for i, (x, y, _, _) in enumerate(R.g12_batches(dtype)):
        t = torch.tensor(TRAJECTORY_TTC[i], dtype=torch.float64)
        assert bool(((y == 1) == (t == 0)).all())
        out.append((x, y, None, {"ttc": t, "smoothed_labels": _smoothed(y, t)}))
    return out


def np64(t):
    return t.detach().double().cpu().numpy()
