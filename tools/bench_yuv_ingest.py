#!/usr/bin/env python3
"""Cameras that deliver 4:2:0 YUV: ``StreamBank.push_yuv`` (the planes packed as they come, converted inside the resize launch) against
the route the package offered before it for the same pictures, ``push_raw`` with RGB frames.

  models    internvideo2_small_patch14_224 at 8 x 224 x 224 and vit_base_patch16_224 at 16 x 224 x 224, fast mode
  cameras   S = 32, NV12 surfaces of three sizes in turn (1280 x 720, 1920 x 1080, 640 x 480), contiguous, BT.601, host numpy arrays
  tick      a frame for every camera (push_yuv / push_raw), then a score for every camera (predict), the scores read back

(a) Whole tick.  Legs ``yuv`` and ``rgb``, interleaved round by round in one process after each has been warmed up past one lap of its
rings.  A leg's time is a host clock around ``--ticks`` ticks ending in a device synchronise, per tick; reported are the median over
``--rounds`` and the spread (max - min), and the bytes each leg packs and uploads per tick.  The ``rgb`` leg is handed RGB frames that
were converted BEFORE anything is timed: it leaves out the host conversion a deployment with YUV cameras would have to add in front
of ``push_raw``, so it understates what ``push_yuv`` saves.  Both legs must hold the same store bytes and give the same logits bits
before anything is timed (asserted).

(b) Launch alone.  With device events around ``--calls`` back-to-back calls on device-resident buffers: one ``ingest_yuv`` launch for
the 32 surfaces against one ``ingest_frames`` launch on the 32 converted frames, into the same store slots.

A pair is called "apart" only when its medians differ by more than both spreads.

usage: python tools/bench_yuv_ingest.py [--streams 32] [--rounds 5] [--ticks 6] [--calls 200] [--out profiles/yuv_ingest.json]
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


def apart(a, b):
    """do the medians differ by more than both spreads?"""
    return bool(abs(a["ms"] - b["ms"]) > max(a["spread_ms"], b["spread_ms"]))


def nv12_to_rgb(buf, h, w, cset):
    """the header's formula on a contiguous NV12 surface (even h, w), in int32 numpy: what the rgb leg's frames are made with, untimed"""
    y_off, cy, cvr, cug, cvg, cub = cset
    Y = buf[:h * w].reshape(h, w).astype(np.int32)
    uv = buf[h * w:].reshape(h // 2, w // 2, 2).astype(np.int32) - 128
    U = np.repeat(np.repeat(uv[..., 0], 2, 0), 2, 1)
    V = np.repeat(np.repeat(uv[..., 1], 2, 0), 2, 1)
    yy = np.maximum(Y - y_off, 0) * cy + (1 << 19)
    out = np.stack([(yy + cvr * V) >> 20, (yy + cvg * V + cug * U) >> 20, (yy + cub * U) >> 20], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=6, help="ticks per round and leg")
    ap.add_argument("--calls", type=int, default=200, help="device calls per round of the launch measurement")
    ap.add_argument("--models", default=",".join(m for m, _ in MODELS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_ingest.json"))
    a = ap.parse_args()
    S = a.streams

    import torch
    import simple_tad_amd as T
    from simple_tad_amd import kernels as K, stream_bank as SB
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv_ingest: no GPU (a measurement does not fall back)")
    T.set_precision("fast")
    rng = np.random.RandomState(0)
    cset = SB.COLOUR_SETS["bt601"]
    # two pictures per camera, used in turn: no tick repeats the one before it
    yuv_pool = [[rng.randint(0, 256, (SIZES[s % 3][0] * 3 // 2, SIZES[s % 3][1]), dtype=np.uint8) for _ in range(2)] for s in range(S)]
    rgb_pool = [[nv12_to_rgb(f.reshape(-1), *SIZES[s % 3], cset) for f in yuv_pool[s]] for s in range(S)]
    ids = list(range(S))
    res = {"bench": "yuv_ingest", "device": torch.cuda.get_device_name(0), "streams": S, "sizes": [list(s) for s in SIZES], "format": "nv12",
           "matrix": "bt601", "rounds": a.rounds, "ticks": a.ticks,
           "yuv_mb_per_tick": round(sum(p[0].nbytes for p in yuv_pool) / 1e6, 1), "rgb_mb_per_tick": round(sum(p[0].nbytes for p in rgb_pool) / 1e6, 1),
           "rgb_leg_excludes_host_conversion": True, "models": {}}

    # ---------------------------------------------------------------- (b) the launch on its own
    H = W = 224
    store = torch.zeros((S, H, W, 3), dtype=torch.uint8, device="cuda")
    frames = [SB.YuvFrame.of(p[0]) for p in yuv_pool]
    ytab, yoff, ybytes, ynh, ynv, ync = SB.plan_ingest_yuv([f.layout for f in frames], ids, [False] * S, H, W, S)
    host = np.zeros(ybytes + 64, dtype=np.uint8)
    for f, at in zip(frames, yoff):
        host[at:at + f.nbytes] = f.data.numpy()[:f.nbytes]
    ysrc, ytab = torch.from_numpy(host).cuda(), ytab.cuda()
    rgbs = [p[0] for p in rgb_pool]
    rtab, roff, rbytes, rnh, rnv = SB.plan_ingest([f.shape[:2] for f in rgbs], ids, [False] * S, H, W, S)
    host = np.zeros(rbytes + 64, dtype=np.uint8)
    for f, at in zip(rgbs, roff):
        host[at:at + f.size] = f.reshape(-1)
    rsrc, rtab = torch.from_numpy(host).cuda(), rtab.cuda()

    def yuv_launch():
        K.ingest_yuv(ysrc, ybytes, store, ytab, S, ynh, ynv, ync)

    def rgb_launch():
        K.ingest_frames(rsrc, rbytes, store, rtab, S, rnh, rnv)

    rgb_launch()
    want = store.clone()
    store.zero_()
    yuv_launch()
    assert torch.equal(store, want), "ingest_yuv and ingest_frames on the converted frames must give the same bytes"

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    routes = {"ingest_yuv": yuv_launch, "ingest_frames": rgb_launch}
    for fn in routes.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, fn in routes.items():
            ms[k].append(timed(fn, a.calls))
    st = {k: stats(v) for k, v in ms.items()}
    res["launch"] = {**st, "yuv_source_mb": round(ybytes / 1e6, 2), "rgb_source_mb": round(rbytes / 1e6, 2),
                     "yuv_over_rgb": round(st["ingest_yuv"]["ms"] / st["ingest_frames"]["ms"], 3), "apart": apart(st["ingest_yuv"], st["ingest_frames"])}
    del store, ysrc, rsrc, want

    # ---------------------------------------------------------------- (a) whole ticks
    for name, kw in MODELS:
        if name not in a.models.split(","):
            continue
        model = T.create_model(name, **kw).cuda().eval()
        Tn = int(model.num_frames)
        banks = {"yuv": T.StreamBank(model, streams=S, mean=MEAN, std=STD, bgr=False), "rgb": T.StreamBank(model, streams=S, mean=MEAN, std=STD, bgr=False)}

        def tick(k, i):
            if k == "yuv":
                banks[k].push_yuv(ids, [yuv_pool[s][i % 2] for s in ids])
            else:
                banks[k].push_raw(ids, [rgb_pool[s][i % 2] for s in ids])
            return banks[k].predict()["logits"].cpu() if banks[k].ready else None

        last, tick_no = {}, {}
        for k in banks:  # fill the rings, then one whole lap
            for i in range(2 * Tn + 1):
                last[k] = tick(k, i)
            tick_no[k] = 2 * Tn + 1
        assert torch.equal(banks["yuv"].store, banks["rgb"].store) and torch.equal(last["yuv"], last["rgb"]), "both legs hold the same pictures"
        ms = {k: [] for k in banks}
        for _ in range(a.rounds):
            for k in banks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    tick(k, tick_no[k])
                    tick_no[k] += 1
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.ticks)
        st = {k: stats(v) for k, v in ms.items()}
        res["models"][name] = {"clip": [Tn, 224, 224], **st, "rgb_over_yuv": round(st["rgb"]["ms"] / st["yuv"]["ms"], 3), "apart": apart(st["yuv"], st["rgb"])}
        del banks, model
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
