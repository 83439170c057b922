#!/usr/bin/env python3
"""Many cameras at once: ``StreamBank`` (one ragged ingest launch and one batched forward per tick) against the way the package served
them before it, one ``SlidingWindow`` per camera (one upload, one resize launch and one batch-1 forward per camera and tick).

  models    internvideo2_small_patch14_224 at 8 x 224 x 224 and vit_base_patch16_224 at 16 x 224 x 224, fast mode
  cameras   S = 32, raw frames of three sizes in turn (1280 x 720, 1920 x 1080, 640 x 480), host numpy arrays as a decoder leaves them
  tick      a frame for every camera (push_raw), then a score for every camera (predict), the scores read back: what a serving loop does

Legs, interleaved round by round in one process after every leg has been warmed up past one lap of its rings (so every captured graph
exists): ``bank_eager``, ``bank_graph``, ``windows_eager``, ``windows_graph``.  A leg's time is a host clock around ``--ticks`` ticks ending
in a device synchronise, per tick; reported are the median over ``--rounds`` and the spread (max - min).  Before anything is timed the
bank's logits are compared with the windows' (the batch size differs, so the bits may: the largest difference is reported, not asserted).

On its own, with device events around ``--calls`` back-to-back calls: the ingest launch for the 32 frames (already packed on the device)
against 32 calls of ``resize_frames`` on the same frames, into the same store slots -- and the launch's bytes per second over its
algorithmic bytes: the distinct source pixels under a tap (a shrink by more than 4 skips rows and columns) plus the bytes written.

usage: python tools/bench_stream_bank.py [--streams 32] [--rounds 5] [--ticks 6] [--calls 200] [--out profiles/stream_bank.json]
Prints one JSON line and writes it to ``--out``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = ((720, 1280), (1080, 1920), (480, 640))
MODELS = (("internvideo2_small_patch14_224", dict(num_classes=2)),
          ("vit_base_patch16_224", dict(pretrained=False, num_classes=2, all_frames=16, tubelet_size=2, final_reduction="fc_norm", init_scale=0.001)))


def stats(v):
    return {"ms": round(float(np.median(v)), 4), "spread_ms": round(max(v) - min(v), 4), "rounds_ms": [round(t, 4) for t in v]}


def tapped_pixels(n_src, n_dst):
    from simple_tad_amd.frame_resize import cubic_coeffs
    first, _ = cubic_coeffs(n_src, n_dst)
    return len(np.unique(np.clip(first[:, None] + np.arange(4)[None, :], 0, n_src - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=6, help="ticks per round and leg")
    ap.add_argument("--calls", type=int, default=200, help="device calls per round of the ingest measurement")
    ap.add_argument("--models", default=",".join(m for m, _ in MODELS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bank.json"))
    a = ap.parse_args()
    S = a.streams

    import torch
    import simple_tad_amd as T
    from simple_tad_amd import kernels as K, stream_bank as SB
    from simple_tad_amd.frame_resize import resize_frames
    from simple_tad_amd.inference import SlidingWindow
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_bank: no GPU (a measurement does not fall back)")
    T.set_precision("fast")
    rng = np.random.RandomState(0)
    # four frames per camera, used in turn: enough that no tick repeats the one before it
    pool = [[rng.randint(0, 256, (*SIZES[s % 3], 3), dtype=np.uint8) for _ in range(4)] for s in range(S)]
    ids = list(range(S))
    res = {"bench": "stream_bank", "device": torch.cuda.get_device_name(0), "streams": S, "sizes": [list(s) for s in SIZES], "rounds": a.rounds,
           "ticks": a.ticks, "raw_mb_per_tick": round(sum(p[0].nbytes for p in pool) / 1e6, 1), "models": {}}

    # ---------------------------------------------------------------- the ingest launch on its own
    H = W = 224
    store = torch.zeros((S, H, W, 3), dtype=torch.uint8, device="cuda")
    frames = [p[0] for p in pool]
    table, offsets, nbytes, nh, nv = SB.plan_ingest([f.shape[:2] for f in frames], ids, [False] * S, H, W, S)
    host = np.zeros(nbytes + 64, dtype=np.uint8)
    for f, at in zip(frames, offsets):
        host[at:at + f.size] = f.reshape(-1)
    src, tab = torch.from_numpy(host).cuda(), table.cuda()
    dev_frames = [torch.from_numpy(f[None]).cuda() for f in frames]

    def one_launch():
        K.ingest_frames(src, nbytes, store, tab, S, nh, nv)

    def per_frame():
        for s in range(S):
            resize_frames(dev_frames[s], (H, W), out=store[s:s + 1])

    per_frame()
    want = store.clone()
    store.zero_()
    one_launch()
    assert torch.equal(store, want), "the ragged launch and the per-frame calls must give the same bytes"

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    routes = {"ingest_frames": (one_launch, a.calls), "resize_frames_x%d" % S: (per_frame, max(1, a.calls // 8))}
    for fn, _ in routes.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, (fn, calls) in routes.items():
            ms[k].append(timed(fn, calls))
    tapped = sum(tapped_pixels(f.shape[0], H) * tapped_pixels(f.shape[1], W) * 3 for f in frames)
    written = S * H * W * 3
    med = float(np.median(ms["ingest_frames"]))
    res["ingest"] = {**{k: stats(v) for k, v in ms.items()}, "source_mb": round(sum(f.nbytes for f in frames) / 1e6, 2),
                     "algorithmic_mb": round((tapped + written) / 1e6, 2), "ingest_gb_per_s": round((tapped + written) / (med * 1e-3) / 1e9, 1),
                     "per_frame_over_ingest": round(float(np.median(ms["resize_frames_x%d" % S])) / med, 2)}
    del store, src, tab, dev_frames, want

    # ---------------------------------------------------------------- whole ticks
    for name, kw in MODELS:
        if name not in a.models.split(","):
            continue
        model = T.create_model(name, **kw).cuda().eval()
        Tn = int(model.num_frames)
        tick_no = {}

        def bank_leg(use_graph):
            bank = T.StreamBank(model, streams=S, mean=MEAN, std=STD, bgr=True, use_graph=use_graph)

            def tick(i):
                bank.push_raw(ids, [pool[s][i % 4] for s in ids])
                return bank.predict()["logits"].cpu() if bank.ready else None
            return tick

        def windows_leg(use_graph):
            wins = [SlidingWindow(model, MEAN, STD, bgr=True, use_graph=use_graph) for _ in ids]

            def tick(i):
                outs = []
                for s in ids:
                    wins[s].push_raw(pool[s][i % 4])
                    if wins[s].full:
                        outs.append(wins[s].predict())
                return torch.cat(outs).float().cpu() if outs else None
            return tick

        legs = {"bank_eager": bank_leg(False), "bank_graph": bank_leg(True), "windows_eager": windows_leg(False), "windows_graph": windows_leg(True)}
        last = {}
        for k, tick in legs.items():  # fill the rings, then one whole lap: every ring offset's graph is captured before anything is timed
            for i in range(2 * Tn + 1):
                last[k] = tick(i)
            tick_no[k] = 2 * Tn + 1
        diff = {k: float((last[k] - last["windows_eager"]).abs().max()) for k in legs}
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, tick in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    tick(tick_no[k])
                    tick_no[k] += 1
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.ticks)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res["models"][name] = {"clip": [Tn, 224, 224], **{k: stats(v) for k, v in ms.items()},
                               "max_abs_logit_diff_vs_windows_eager": diff,
                               "windows_eager_over_bank_eager": round(med["windows_eager"] / med["bank_eager"], 2),
                               "windows_graph_over_bank_graph": round(med["windows_graph"] / med["bank_graph"], 2)}
        del legs, model
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
