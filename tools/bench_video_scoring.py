#!/usr/bin/env python3
"""Windows per second of scoring one whole video, three routes interleaved in one process (needs a GPU; bench.py is another tool
and is not touched by this one):

  (a) store        inference.score_video: the frames uploaded once, the patch matrix of every batch built straight from the store
  (b) materialise  the same forwards on ``store[idx]`` copied out per batch -- what the package could do before the store route; the
                   host steps are score_video's own (sequencer, one upload, validated table per batch, softmax, read-backs), so the two
                   routes differ in the input stage only
  (c) sliding      one SlidingWindow.push + predict per frame (one window per forward), eager and with use_graph
and the input stage of one batch alone: tad_im2col_frame_windows against copy-out + tad_im2col_tubelets_u8 of the copy.

Workload: ViT-B/16 at 16 x 224^2, a synthetic video of 116 frames = 101 windows at view_step 1 (three batches of 32 and a ragged one
of 5).  Every route is warmed up on every batch shape it uses (the sliding window with a graph: on every ring offset); a leg repeats
whole-video passes between two device synchronisations until at least ``--seconds`` have passed; the legs alternate over ``--rounds``
rounds and the table gives the median and the spread (min .. max) per route.  Host-to-device frame bytes per video are COUNTED, not
timed: F * H * W * 3 for (a) / (b) / (c) against S * T * H * W * 3 for a loader that uploads every window as a clip.
Outputs are compared before anything is timed: (a) and (b) must agree bit for bit; (c) runs at batch size 1, so its logits may differ
from the batched ones in the last bits -- the largest difference is printed.

usage: python tools/bench_video_scoring.py [--seconds 1.0] [--rounds 3] [--precision fast|half] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="least duration of one timed leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=116)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--precision", default="fast", choices=["fast", "half"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_video_scoring needs a GPU: there is no CPU path and a CPU time says nothing")
    import simple_tad_amd as T
    from simple_tad_amd import FrameStore
    from simple_tad_amd import kernels as K
    from simple_tad_amd.inference import IMAGENET_MEAN, IMAGENET_STD, SlidingWindow, score_video
    from simple_tad_amd.sequencing import RegularSequencer

    dev = torch.device("cuda", 0)
    T.set_precision(args.precision)
    torch.manual_seed(0)
    model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=16, tubelet_size=2, final_reduction="fc_norm",
                           drop_path_rate=0.0, init_scale=1.0, use_flash_attn=True).to(dev).eval()
    H = W = 224
    Tn, bs = 16, args.batch_size
    frames = torch.randint(0, 256, (args.frames, H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).numpy()
    table = np.asarray(RegularSequencer(10, Tn, 1).get_sequences(args.frames, 10), dtype=np.int64)
    S = len(table)
    frame_bytes = H * W * 3

    def route_store():
        return score_video(model, frames, orig_fps=10, target_fps=10, batch_size=bs)["logits"]

    def route_materialise():
        """score_video's own steps (sequencer, one upload, validated index table per batch, eval-mode switch, softmax, two read-backs) with
        ONE difference: every batch is copied out of the store as uint8 clips [B,T,H,W,3] and takes the model's uint8 clip route"""
        windows = np.asarray(RegularSequencer(10, Tn, 1).get_sequences(len(frames), 10), dtype=np.int64)
        store = FrameStore(args.frames, H, W, dev)
        store.append(frames)
        model.patch_embed.set_input_normalization(IMAGENET_MEAN, IMAGENET_STD, bgr=False)
        was = model.training
        model.eval()
        with torch.no_grad():
            outs = [model(store.windows(windows[lo:lo + bs]).materialize()) for lo in range(0, len(windows), bs)]
        model.train(was)
        logits = torch.cat(outs).float()
        prob = torch.softmax(logits, dim=1)[:, 1]
        prob.cpu()
        return logits.cpu()

    def make_sliding(use_graph):
        sw = SlidingWindow(model, bgr=False, use_graph=use_graph)

        def run():
            sw.count, sw.start = 0, 0
            outs = []
            for f in frames:
                sw.push(f)
                if sw.full:
                    outs.append(sw.predict())
            return torch.cat(outs).float().cpu()
        return run

    routes = {"store": route_store, "materialise": route_materialise, "sliding_eager": make_sliding(False), "sliding_graph": make_sliding(True)}
    # ---- warm-up (every batch shape incl. the ragged last batch; every ring offset of the graph route) and the output comparison
    ref = {k: fn() for k, fn in routes.items()}
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    assert all(v.shape == (S, 2) for v in ref.values()), {k: tuple(v.shape) for k, v in ref.items()}
    assert torch.equal(ref["store"], ref["materialise"]), "the store route and the materialised clips disagree"
    diffs = {k: float((ref[k] - ref["store"]).abs().max()) for k in ("sliding_eager", "sliding_graph")}

    def leg(fn, units=S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while True:
            fn()
            n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= args.seconds:
                return n * units / dt

    # ---- the input stage alone, on one batch of `bs` windows: the patch matrix straight from the store against the copy-out of the clips
    # followed by the im2col of the copy (200 launches between two synchronisations per call)
    st = FrameStore(args.frames, H, W, dev)
    st.append(frames)
    fw = st.windows(table[:bs])
    REP = 200

    def stage_store():
        for _ in range(REP):
            K.im2col_frame_windows(fw.store, fw.idx, 2, 16, IMAGENET_MEAN, IMAGENET_STD)

    def stage_copy():
        for _ in range(REP):
            K.im2col_tubelets_u8(fw.materialize(), 2, 16, IMAGENET_MEAN, IMAGENET_STD)

    stages = {"patch_matrix_from_store": stage_store, "copy_out_then_im2col": stage_copy}
    for fn in stages.values():
        fn()
    rates = {k: [] for k in routes}
    stage_rates = {k: [] for k in stages}
    for _ in range(max(3, args.rounds)):
        for k, fn in routes.items():  # alternate the legs inside every round
            rates[k].append(leg(fn))
        for k, fn in stages.items():
            stage_rates[k].append(leg(fn, REP))
    out = {"workload": f"ViT-B/16 16x224^2, {args.frames} frames, {S} windows, batch {bs}, precision {args.precision}",
           "device": torch.cuda.get_device_name(0),
           "windows_per_s": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for k, v in rates.items()},
           "h2d_frame_bytes_per_video": {"store": args.frames * frame_bytes, "materialise": args.frames * frame_bytes,
                                         "sliding": args.frames * frame_bytes, "clip_per_window_loader": S * Tn * frame_bytes},
           "input_stage_us_per_batch": {k: {"median": 1e6 / statistics.median(v), "min": 1e6 / max(v), "max": 1e6 / min(v)} for k, v in stage_rates.items()},
           "max_abs_logit_diff_vs_store": diffs, "store_equals_materialise_bitwise": True}
    print(f"{'route':<16}{'windows/s median':>18}{'min':>10}{'max':>10}")
    for k, v in out["windows_per_s"].items():
        print(f"{k:<16}{v['median']:>18.1f}{v['min']:>10.1f}{v['max']:>10.1f}")
    for k, v in out["input_stage_us_per_batch"].items():
        print(f"{k:<28}{v['median']:>8.1f} us per batch of {bs} (host clock over {REP} launches; {v['min']:.1f} .. {v['max']:.1f})")
    print("H2D frame bytes per video:", out["h2d_frame_bytes_per_video"])
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
