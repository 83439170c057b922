"""What does a saliency map cost?  ViT-B/16, 16 x 224^2, --windows clips resident on the device, in the "fast" (bfloat16) and "half" (IEEE
half) modes; four things interleaved in one process, per mode:

  forward          the plain evaluation forward (model(x) under no_grad)
  rollout          explain.attention_rollout: the same forward under ops.capture_attention (the forward kernel also writes lse, the qkv of
                   every layer stays alive) + one kernels.attn_colsum launch per layer + the blend in torch
  attn_colsum      one launch at the model's shape, beside
  attn_fwd         one launch of the forward's attention kernel on the same qkv
  torch_rollout    the "without this kernel" leg: the same vector recurrence from the same captured records composed in torch, which
                   MATERIALISES the softmax of one layer at a time ([B,H,N,N] f32: 0.94 GB at 8 windows; f32 matmul + softmax + einsum)

Every leg is warmed up once, then --rounds (>= 3) rounds run every leg once for --iters timed iterations (device events around the whole
loop).  Medians and spread over the rounds.  The figure to judge by: rollout_ms / forward_ms.  Nothing is asserted.

Writes ONE JSON object to --out (default profiles/explain.json) and prints it on one line.

usage: python tools/bench_explain.py [--windows 8] [--iters 5] [--rounds 3] [--out profiles/explain.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import simple_tad_amd as T  # noqa: E402
from simple_tad_amd import explain, kernels as K, ops  # noqa: E402

FRAMES, SIZE = 16, 224
LOG2E = 1.4426950408889634


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_rollout(records, start, residual):
    """token_rollout's recurrence with the softmax of each layer materialised by torch"""
    v = start
    for qkv, lse, B, N, H, d, scale, qs in reversed(records):
        x5 = qkv.reshape(B, N, 3, H, d)
        q, k = x5[:, :, 0].permute(0, 2, 1, 3).float(), x5[:, :, 1].permute(0, 2, 1, 3).float()
        s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / LOG2E if qs else scale)  # (a pre-scaled q carries scale * log2e)
        p = torch.softmax(s, dim=-1)
        c = torch.einsum("bi,bhij->bhj", v, p)
        v = residual * v + (1 - residual) * c.mean(1)
    return v / v.sum(-1, keepdim=True)


def one_mode(mode, args, dev):
    T.set_precision(mode)
    torch.manual_seed(0)
    model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=FRAMES, tubelet_size=2,
                           final_reduction="fc_norm", init_scale=0.001, use_flash_attn=True).to(dev).eval()
    B = args.windows
    x = torch.randn(B, 3, FRAMES, SIZE, SIZE, device=dev)
    with torch.no_grad():
        with ops.capture_attention(model) as records:
            plain = model(x)
    qkv, lse, _, N, H, d, scale, qs = records[-1]
    start = torch.full((B, N), 1.0 / N, device=dev)
    sal = explain.token_rollout(records, start)
    ref = torch_rollout(records, start, 0.5)
    agree = float(((sal - ref).abs() / ref).max())

    @torch.no_grad()
    def forward():
        model(x)

    legs = {"forward": forward, "rollout": lambda: explain.attention_rollout(model, x),
            "attn_colsum": lambda: K.attn_colsum(qkv, lse, start, B, N, H, scale, q_prescaled=qs, d=d),
            "attn_fwd": lambda: K.attn_fwd(qkv, B, N, H, scale, want_lse=False, q_prescaled=qs, d=d),
            "torch_rollout": lambda: torch_rollout(records, start, 0.5)}
    assert torch.equal(explain.attention_rollout(model, x)[0], plain), "logits under capture differ from the plain forward"
    for fn in legs.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn, args.iters * (10 if k.startswith("attn_") else 1)))
    out = {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    flops = 2.0 * B * H * N * N * d
    out["attn_colsum"]["tflops"] = round(flops / med["attn_colsum"] / 1e9, 1)
    out["attn_fwd"]["tflops"] = round(2 * flops / med["attn_fwd"] / 1e9, 1)
    out["ratios"] = {"rollout_over_forward": round(med["rollout"] / med["forward"], 4),
                     "attn_colsum_over_attn_fwd": round(med["attn_colsum"] / med["attn_fwd"], 4),
                     "torch_rollout_over_kernel_rollout_extra": round(med["torch_rollout"] / max(med["rollout"] - med["forward"], 1e-9), 2)}
    out["kernel_vs_torch_rollout_max_rel_diff"] = agree
    out["layers"], out["tokens"], out["heads"], out["head_dim"] = len(records), N, H, d
    out["torch_softmax_bytes_per_layer"] = 4 * B * H * N * N
    del records, model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_explain needs a GPU"
    assert args.rounds >= 3, "at least three rounds"
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        modes = {mode: one_mode(mode, args, dev) for mode in ("fast", "half")}
    finally:
        T.set_precision("fast")
    out = {"bench": "explain", "device": torch.cuda.get_device_name(dev), "model": "vit_base_patch16_224", "windows": args.windows,
           "frames": FRAMES, "iters": args.iters, "rounds": args.rounds, "modes": modes,
           "judge_by": "ratios.rollout_over_forward (the plain forward runs the unchanged kernels); no threshold asserted"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
