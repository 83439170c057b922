"""Whole-tensor gradient parity and stochastic depth against an fp64 oracle.

The real-size pins of tests/test_real_size.py compare each gradient with the G11 fixture through its first 256 flattened elements and
its sum of squares only.  Here the oracle (oracle/vit_oracle.py) runs the same ViT-B/16 16x224x224 step in float64 on the device, on the
GPU model's own fp32 weights, and is first checked against that fixture; every one of the 162 gradient tensors of each precision mode
is then compared with it WHOLE.  The same oracle, fed the drop-path masks that are injected into the production consumption path
(VisionTransformer._presample_drop_path -> DropPath.presampled -> the rowscale epilogues, the LayerNorm backward and the block-chain
hand-off), checks the benchmarked training configuration.  The small-shape tests at the end cover the DropPath sampler itself,
activation checkpointing with drop path, and layer-scale training, against the CPU fp64 oracle."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_recipe as R
import simple_tad_amd as T
from oracle import vit_oracle as O
from simple_tad_amd import ops
from simple_tad_amd.modeling_finetune import DropPath
from test_real_size import build_vitb, check_weights, head_err, sq_err

pytestmark = pytest.mark.gpu

HALF_SCALE = 4096.0   # the loss scale of test_real_size's half-mode test
# whole-tensor rel-L2 bounds per mode.  precise: the documented parity gate; half: README's "every gradient tensor within 1e-3";
# fast: 1.5x the worst tensor measured on MI355X (6.72e-3, see test_whole_gradient_tensors_at_real_shape)
BOUND = {"precise": 1e-3, "half": 1e-3, "fast": 1.0e-2}


def rell2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def whole_err(got, ref):
    """(rel-L2, max|err| / RMS) of a whole tensor against its fp64 reference, on the reference's device"""
    ref = ref.detach()
    d = got.detach().to(device=ref.device, dtype=torch.float64) - ref
    n = ref.norm()
    if float(n) == 0.0:   # a branch that every sample dropped: the kernel path must give exact zeros as well
        e = float(d.abs().max())
        return e, e
    rms = n / ref.numel() ** 0.5
    return (d.norm() / n).item(), (d.abs().max() / rms).item()


def table(title, errs):
    """one line per parameter kind (the 12 blocks' tensors of one name together): worst rel-L2 and where, worst max|err|/RMS"""
    kinds = {}
    for k, (rel, mx) in errs.items():
        kind = ".".join(k.split(".")[2:]) if k.startswith("blocks.") else k
        kinds.setdefault(kind, []).append((rel, mx, k))
    rels = [v[0] for v in errs.values()]
    worst = max(errs, key=lambda k: errs[k][0])
    lines = [f"{title}: {len(errs)} tensors, rel-L2 median {np.median(rels):.2e} worst {errs[worst][0]:.2e} ({worst}); "
             f"max|err|/RMS worst {max(v[1] for v in errs.values()):.2e}"]
    for kind, v in kinds.items():
        w = max(v)
        lines.append(f"  {kind:<24} rel-L2 worst {w[0]:.2e} ({w[2]})  median {np.median([e[0] for e in v]):.2e}  "
                     f"max|err|/RMS worst {max(e[1] for e in v):.2e}")
    print("\n" + "\n".join(lines))


def fp64_step(m, x, y, keep_masks=None, keep_prob=1.0):
    """the oracle's forward + CE loss + backward in float64 on the device of `x`, on the fp32 weights of `m` cast to fp64"""
    P = {k: v.detach().double().requires_grad_() for k, v in m.state_dict().items()}
    feats = O.forward_features(x.double(), P, depth=len(m.blocks), num_heads=m.num_heads, tubelet=2, patch=16,
                               keep_masks=keep_masks, keep_prob=keep_prob)
    logits = F.linear(feats, P["head.weight"], P["head.bias"])
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return SimpleNamespace(feats=feats.detach(), logits=logits.detach(), loss=loss.item(),
                           grads={k: P[k].grad for k, _ in m.named_parameters()})


def run_mode(m, x, y, mode):
    """one forward + CE loss + backward of the HIP path; returns (features, logits, loss, unscaled gradients by name)"""
    m.zero_grad(set_to_none=True)
    T.set_precision(mode)
    try:
        feats = m.forward_features(x)
        logits = m.head(feats)
        loss = F.cross_entropy(logits, y)
        (loss * HALF_SCALE if mode == "half" else loss).backward()
    finally:
        T.set_precision("fast")
    s = HALF_SCALE if mode == "half" else 1.0
    grads = {k: p.grad / s for k, p in m.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()), mode
    return feats.detach(), logits.detach(), loss.item(), grads


# ------------------------------------------------------------------------------------------------- A: the fp64 reference on the device
@pytest.fixture(scope="module")
def vitb(golden):
    g = golden("g11_vitb_grads")
    m, x, y = build_vitb()
    check_weights(m, g)
    m = m.cuda().train()
    x, y = x.cuda(), y.cuda()
    return SimpleNamespace(g=g, m=m, x=x, y=y, ref=fp64_step(m, x, y))


def test_fp64_device_reference_matches_reference_golden(vitb):
    """the fp64 oracle on the device reproduces the reference's own fp64 run (G11) before it serves as the truth: the only expected
    difference is the ~2e-7 last-bit noise of the regenerated weights that check_weights documents"""
    g, ref = vitb.g, vitb.ref
    e_f, e_l = rell2(ref.feats, g["features"]), rell2(ref.logits, g["logits"])
    e_loss = abs(ref.loss - float(g["loss"]))
    assert list(ref.grads) == [str(k) for k in g["grad_keys"]]
    e_g = {k: max(head_err(v, g, "grad." + k), sq_err(v, g, "grad." + k)) for k, v in ref.grads.items()}
    worst = max(e_g, key=e_g.get)
    print(f"\nfp64 oracle on the device vs G11: features {e_f:.2e} logits {e_l:.2e} loss {e_loss:.2e} "
          f"gradient slice / sum of squares worst {e_g[worst]:.2e} ({worst})")
    assert e_f <= 1e-6 and e_l <= 1e-6 and e_loss <= 1e-7, (e_f, e_l, e_loss)
    assert e_g[worst] <= 1e-5, (worst, e_g[worst])


# ------------------------------------------------------------------------------------------------- B: whole tensors, three modes
@pytest.mark.parametrize("mode", ["precise", "half", "fast"])
def test_whole_gradient_tensors_at_real_shape(vitb, mode):
    """every one of the 162 gradient tensors of ViT-B/16 16x224x224 (B = 2) against the fp64 oracle, whole: rel-L2 within the mode's
    bound.  Measured on MI355X, worst tensor (median): precise 1.04e-5 (6.2e-6) against the 1e-3 parity gate; half (loss scale
    4096) 8.11e-4 (5.0e-4) against README's 1e-3; fast (bf16 operands) 6.72e-3 (4.3e-3) -> bound 1.0e-2.  In all three the worst
    is blocks.10.attn.q_bias, a sum over 3136 tokens of the q gradient, which at seeded init is ~100x below the v gradient.
    The largest single element error is 1.9e-4 / 1.6e-2 / 1.2e-1 of the tensor's RMS (printed, not bounded)."""
    feats, logits, loss, grads = run_mode(vitb.m, vitb.x, vitb.y, mode)
    ref = vitb.ref
    errs = {k: whole_err(v, ref.grads[k]) for k, v in grads.items()}
    table(f"{mode} ViT-B real shape, whole gradient tensors vs fp64 (features {rell2(feats, ref.feats):.2e}, logits "
          f"{rell2(logits, ref.logits):.2e}, loss {abs(loss - ref.loss):.2e})", errs)
    assert len(errs) == 162
    over = {k: v[0] for k, v in errs.items() if not v[0] <= BOUND[mode]}
    assert not over, (mode, BOUND[mode], over)


# ------------------------------------------------------------------------------------------------- C: stochastic depth at the real shape
# (attention-branch mask, MLP-branch mask) per block, B = 2; block 0 has drop-path rate 0 (no DropPath module).  Every branch keeps
# at least one sample, so no gradient tensor is identically zero.
DP_MASKS = {
    1: ([1, 1], [1, 1]),
    2: ([0, 1], [1, 0]),   # dp1 != dp2 for both samples
    3: ([1, 0], [1, 0]),   # sample 1 dropped in both branches
    4: ([1, 1], [0, 1]),   # blocks 3 and 4 both drop in dp2: the chain hand-off carries a rowscale with zeros
    5: ([0, 1], [1, 1]),
    6: ([1, 1], [1, 1]),
    7: ([1, 0], [0, 1]),
    8: ([1, 1], [1, 0]),
    9: ([0, 1], [1, 1]),
    10: ([1, 1], [1, 1]),
    11: ([1, 1], [1, 0]),  # the last block's dp2 (no successor: scale_cast at the start of its backward)
}


def inject_drop_path(m, masks):
    """replace the instance's one-launch sampler by one that presamples these masks as the per-sample scales mask / keep (float32, as
    the sampler computes them); returns the oracle's per-block keep_masks / keep_prob"""
    dev = m.head.weight.device
    scales, keep_masks, keep_prob = {}, [], []
    for i, blk in enumerate(m.blocks):
        d = blk.drop_path
        if not isinstance(d, DropPath):
            assert i not in masks
            keep_masks.append(None)
            keep_prob.append(1.0)
            continue
        keep = 1.0 - d.drop_prob
        mk = [torch.tensor(v, dtype=torch.float32) for v in masks[i]]
        scales[i] = [(v / torch.tensor(keep, dtype=torch.float32)).to(dev) for v in mk]
        keep_masks.append([v.double().to(dev) for v in mk])
        keep_prob.append(keep)

    def presample(batch, device):
        for i, s in scales.items():
            m.blocks[i].drop_path.presampled = [s[0].clone(), s[1].clone()]
    m._presample_drop_path = presample
    return keep_masks, keep_prob


@pytest.fixture(scope="module")
def vitb_dp(vitb):
    m = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=16, tubelet_size=2, final_reduction="fc_norm",
                       use_flash_attn=False, init_scale=1.0, drop_path_rate=0.2)
    m.load_state_dict(vitb.m.state_dict())
    m = m.cuda().train()
    keeps = sorted({round(1.0 - b.drop_path.drop_prob, 6) for b in m.blocks if isinstance(b.drop_path, DropPath)})
    assert len(keeps) == 11   # a different keep probability in every block with stochastic depth
    keep_masks, keep_prob = inject_drop_path(m, DP_MASKS)
    return SimpleNamespace(m=m, ref=fp64_step(m, vitb.x, vitb.y, keep_masks=keep_masks, keep_prob=keep_prob))


@pytest.mark.parametrize("mode", ["fast", "half"])
def test_stochastic_depth_at_real_shape(vitb, vitb_dp, mode):
    """the benchmarked training configuration (fused blocks, block-chain hand-off, drop path) with drop_path_rate 0.2 and the fixed
    mask pattern DP_MASKS, every gradient tensor whole against the fp64 oracle under the same masks; same bounds as without drop path.
    Measured on MI355X, worst tensor (median): fast 7.75e-3 (3.8e-3), half 9.71e-4 (4.7e-4), both blocks.11.norm1.bias.  The two
    differ by 2^-3, the ratio of the bf16 and half unit roundoffs: operand rounding in an ill-conditioned sum (the two clips' CE
    gradients have opposite signs), not a mis-applied scale, which would not shrink with the operand format."""
    m = vitb_dp.m
    ops._chain.hits = 0
    feats, logits, loss, grads = run_mode(m, vitb.x, vitb.y, mode)
    assert all(not b.drop_path.presampled for b in m.blocks if isinstance(b.drop_path, DropPath))   # every injected scale consumed
    assert ops._chain.hits == 11 and ops._chain.pending == 0   # blocks 0..10 took the rowscaled copy made by blocks 1..11
    ref = vitb_dp.ref
    errs = {k: whole_err(v, ref.grads[k]) for k, v in grads.items()}
    table(f"{mode} ViT-B real shape, drop path 0.2 with injected masks, whole gradient tensors vs fp64 (features "
          f"{rell2(feats, ref.feats):.2e}, logits {rell2(logits, ref.logits):.2e}, loss {abs(loss - ref.loss):.2e})", errs)
    assert rell2(logits, ref.logits) < (1e-3 if mode == "half" else 4.4e-3)
    over = {k: v[0] for k, v in errs.items() if not v[0] <= BOUND[mode]}
    assert not over, (mode, BOUND[mode], over)


# ------------------------------------------------------------------------------------------------- D: small shapes, CPU fp64 oracle
# one label for every clip: the clips' CE gradients then add up in the bias gradients (sums over the batch).  With mixed labels at
# random init they nearly cancel, and a bias gradient of a block where drop path kept one clip of each label becomes a small
# difference of bf16-rounded terms (measured 6.7e-2 rel-L2 for an fc2 bias; every other tensor below 1.5e-2).
SAME_LABEL = torch.tensor([1, 1, 1, 1])


def _small(depth=4, **kw):
    torch.manual_seed(0)
    m = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=depth, num_heads=2, mlp_ratio=4, qkv_bias=True,
                            all_frames=4, tubelet_size=2, num_classes=2, init_scale=1.0, **kw)
    R.rerandomize_1d(m)
    return m.cuda().train()


def record_samples(m):
    """wrap every DropPath's sample() so that each scale vector it hands out is recorded, per block"""
    rec = {}
    for i, blk in enumerate(m.blocks):
        d = blk.drop_path
        if isinstance(d, DropPath):
            rec[i] = []

            def wrapped(batch, device, _orig=d.sample, _r=rec[i]):
                s = _orig(batch, device)
                _r.append(None if s is None else s.detach().clone())
                return s
            d.sample = wrapped
    return rec


def small_oracle_check(m, x, y, logits, masks):
    """the model's gradients against the CPU fp64 oracle under the given per-block (dp1, dp2) scale vectors"""
    keep_masks, keep_prob = [], []
    for i, blk in enumerate(m.blocks):
        if i in masks:
            keep = 1.0 - blk.drop_path.drop_prob
            inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(keep, dtype=torch.float32)
            for s in masks[i]:
                assert bool(((s == 0) | (s == inv.to(s.device))).all()), (i, s)   # every scale is 0 or 1/keep
            keep_masks.append([(s != 0).double().cpu() for s in masks[i]])
            keep_prob.append(keep)
        else:
            keep_masks.append(None)
            keep_prob.append(1.0)
    P = {k: v.detach().double().cpu().requires_grad_() for k, v in m.state_dict().items()}
    ref = O.forward(x.double(), P, depth=len(m.blocks), num_heads=2, tubelet=2, patch=16, keep_masks=keep_masks, keep_prob=keep_prob)
    F.cross_entropy(ref, y).backward()
    e_l = rell2(logits, ref)
    assert all(p.grad is not None for p in m.parameters())
    errs = {k: rell2(p.grad, P[k].grad) for k, p in m.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"\nlogits {e_l:.2e}, gradients rel-L2 median {np.median(list(errs.values())):.2e} worst {errs[worst]:.2e} ({worst})")
    # 1.5x the worst measured on MI355X over the two tests below: logits 1.77e-3, a gradient 6.04e-3 (a q_bias; median 2.1e-3)
    assert e_l < 2.7e-3, e_l
    for k, e in errs.items():
        assert e < 9e-3, (k, e)


def test_drop_path_sampler_vs_oracle():
    """the one-launch sampler of the training forward (VisionTransformer._presample_drop_path): every scale it hands the fused
    blocks is 0 or 1/keep with each block's own keep probability, both occur, and the gradients match the oracle fed those masks"""
    m = _small(depth=4, drop_path_rate=0.5)
    rec = record_samples(m)
    torch.manual_seed(11)
    x = torch.randn(4, 3, 4, 32, 32)
    y = SAME_LABEL
    logits = m(x.cuda())
    F.cross_entropy(logits, y.cuda()).backward()
    assert sorted(rec) == [1, 2, 3] and all(len(v) == 2 for v in rec.values()), {k: len(v) for k, v in rec.items()}
    allv = torch.cat([s.cpu() for v in rec.values() for s in v])
    assert bool((allv == 0).any()) and bool((allv > 1).any()), allv
    small_oracle_check(m, x, y, logits, {i: v for i, v in rec.items()})


def test_checkpointing_with_drop_path_recomputes_the_same_masks():
    """use_checkpoint=True: each block samples its scales in the forward and again in the recompute of the backward; the recompute
    must draw bit-identical scales (the checkpoint restores the device RNG state), and the gradients match the oracle"""
    m = _small(depth=4, drop_path_rate=0.5, use_checkpoint=True)
    rec = record_samples(m)
    torch.manual_seed(11)
    x = torch.randn(4, 3, 4, 32, 32)
    y = SAME_LABEL
    logits = m(x.cuda())
    assert all(len(v) == 2 for v in rec.values())
    F.cross_entropy(logits, y.cuda()).backward()
    assert sorted(rec) == [1, 2, 3] and all(len(v) == 4 for v in rec.values()), {k: len(v) for k, v in rec.items()}
    for i, v in rec.items():
        assert torch.equal(v[0], v[2]) and torch.equal(v[1], v[3]), i
    allv = torch.cat([s.cpu() for v in rec.values() for s in v])
    assert bool((allv == 0).any()) and bool((allv > 1).any()), allv
    small_oracle_check(m, x, y, logits, {i: v[:2] for i, v in rec.items()})
    # the plain (presampling) path fed the same scales gives the same gradients bit for bit
    m2 = _small(depth=4, drop_path_rate=0.5)
    m2.load_state_dict(m.state_dict())
    inject_drop_path(m2, {i: [(s != 0).float().tolist() for s in v[:2]] for i, v in rec.items()})
    l2 = m2(x.cuda())
    F.cross_entropy(l2, y.cuda()).backward()
    assert torch.equal(l2, logits)
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p.grad, p2.grad), k


def test_layer_scale_training_with_drop_path_vs_oracle():
    """init_values > 0 (the composed Block path) in training: per-channel gammas, injected drop-path masks that differ between the
    two branches and between consecutive blocks, every gradient -- gamma_1 and gamma_2 included -- against the fp64 oracle, with the
    tolerances of test_model_gpu's one-block drop-path test (measured on MI355X: output 4.2e-5, input gradient 4.5e-5, weight
    gradients 7.2e-3 worst, a q_bias; gammas 3.3e-3)"""
    c = R.TINY
    depth, D = 3, c["embed_dim"]
    m = T.VisionTransformer(img_size=c["img_size"], patch_size=c["patch_size"], embed_dim=D, depth=depth, num_heads=c["num_heads"],
                            mlp_ratio=4, qkv_bias=True, norm_layer=__import__("functools").partial(torch.nn.LayerNorm, eps=1e-6),
                            all_frames=c["all_frames"], tubelet_size=c["tubelet_size"], num_classes=c["num_classes"], init_scale=1.0,
                            init_values=0.1, drop_path_rate=0.5)
    P = R.params_for(R.vit_param_shapes(D, depth, c["num_classes"], tubelet=c["tubelet_size"], patch=c["patch_size"]), seed=5)
    for i in range(depth):
        for gname in ("gamma_1", "gamma_2"):
            P[f"blocks.{i}.{gname}"] = R.tensor_for(f"ls.{i}.{gname}", (D,), scale=0.05, shift=0.1)
    m.load_state_dict(P, strict=True)
    m = m.cuda().train()
    assert all(not b._fusable() for b in m.blocks)
    masks = {1: ([0.0, 1.0], [1.0, 0.0]), 2: ([1.0, 0.0], [0.0, 1.0])}
    for i, (m1, m2) in masks.items():
        keep = 1.0 - m.blocks[i].drop_path.drop_prob
        m.blocks[i].drop_path.presampled = [torch.tensor(m1, device="cuda") / keep, torch.tensor(m2, device="cuda") / keep]
    xin = R.tensor_for("ls.x", (2, 8, D))
    dy = R.tensor_for("ls.dy", (2, 8, D))
    xg = xin.cuda().requires_grad_()
    t = xg
    for blk in m.blocks:
        t = blk(t)
    t.backward(dy.cuda())
    assert all(not b.drop_path.presampled for b in m.blocks if isinstance(b.drop_path, DropPath))
    Pd = {k: v.double().requires_grad_() for k, v in P.items() if k.startswith("blocks.")}
    xd = xin.double().requires_grad_()
    r = xd
    for i in range(depth):
        km = [torch.tensor(v, dtype=torch.float64) for v in masks[i]] if i in masks else None
        r = O.block(r, Pd, f"blocks.{i}.", c["num_heads"], keep_masks=km, keep_prob=1.0 - m.blocks[i].drop_path.drop_prob if km else 1.0)
    r.backward(dy.double())
    e_y, e_x = rell2(t, r), rell2(xg.grad, xd.grad)
    assert all(p.grad is not None for p in m.blocks.parameters())
    errs = {k: rell2(p.grad, Pd["blocks." + k].grad) for k, p in m.blocks.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"\nlayer scale + drop path, {depth} composed blocks: output {e_y:.2e} input gradient {e_x:.2e} weight gradients worst "
          f"{errs[worst]:.2e} ({worst}); gammas {max(v for k, v in errs.items() if 'gamma' in k):.2e}")
    assert e_y < 5e-3 and e_x < 1e-2, (e_y, e_x)
    assert len(errs) == depth * 15 and sum("gamma" in k for k in errs) == 2 * depth
    for k, e in errs.items():
        assert e < 2e-2, (k, e)
