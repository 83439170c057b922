#!/usr/bin/env python3
"""Generate ``tests/golden/g23_frame_ingest.npz`` by running the REAL reference's ``video_transforms.pad_wide_clips`` (imported from a
checkout of the reference; CPU torch) under ``torch.manual_seed``.

``cv2`` is replaced by a recording stand-in: ``copyMakeBorder``, ``addWeighted`` and ``resize`` note their arguments and hand their
first argument on, so what a call of the reference's ``do_pad`` asks of OpenCV is seen from outside.  Per case ``(seed, h, w)``:
``torch.manual_seed(seed)``, then ``CLIPS`` calls of ``pad_wide_clips(h, w, crop_size)`` in a row, each followed by one ``do_pad`` on a
token frame.  Stored per case:

* ``pads`` float64 [CLIPS, 8] = (mode, pad_top, pad_bottom, alpha, colour[0..2], crop_size asked of resize); mode 0 none, 1 black,
  2 color, 3 reflect, 4 replicate.  alpha is what ``addWeighted`` was given, so it is known for ``reflect`` alone (NaN elsewhere: the
  reference draws it and drops it);
* ``state`` uint8: ``torch.get_rng_state()`` after the last clip.

Nothing of the reference's text is copied; the file holds data only.  The archive is written with fixed timestamps, so it regenerates
byte for byte.

usage: python tools/make_goldens_frame_ingest.py [--reference DIR]      (default: $TAD_REFERENCE)
"""
import argparse
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
CLIPS = 24
CROP = 224
# (seed, h, w): camera frames, a small wide frame, a barely wide one (pads of 0 or 1), a square and a tall one (w <= h: never padded)
CASES = [(0, 720, 1280), (1, 45, 80), (2, 63, 64), (3, 64, 64), (4, 80, 45)]
NONE, BLACK, COLOR, REFLECT, REPLICATE = range(5)


class _StandIn(types.ModuleType):
    """an empty module: any name asked of it is an empty class (enough for ``from x import y`` and for a base class)"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = sys.modules.get(f"{self.__name__}.{name}")
        return sub if sub is not None else type(name, (), {})


class RecordingCv2(types.ModuleType):
    """stands in for cv2: the three calls pad_wide_clips makes are recorded, each hands its first argument on"""
    BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT = "constant", "replicate", "reflect"
    INTER_CUBIC = "cubic"

    def __init__(self):
        super().__init__("cv2")
        self.calls = []

    def copyMakeBorder(self, src, top, bottom, left, right, borderType, value=None):
        self.calls.append(("border", top, bottom, left, right, borderType, value))
        return src

    def addWeighted(self, src1, alpha, src2, beta, gamma):
        self.calls.append(("weighted", alpha, beta, gamma))
        return src1

    def resize(self, src, dsize=None, interpolation=None):
        self.calls.append(("resize", dsize, interpolation))
        return src


def import_reference(ref_dir):
    cv2 = RecordingCv2()
    sys.modules["cv2"] = cv2
    for name in ("decord", "torchvision", "pandas", "tqdm", "PIL"):
        try:
            importlib.import_module(name)
        except ImportError:
            subs = ("", ".transforms", ".transforms.functional") if name == "torchvision" else ("",)
            for sub in subs:
                sys.modules[name + sub] = _StandIn(name + sub)
    sys.path.insert(0, ref_dir)
    vt = importlib.import_module("video_transforms")
    assert os.path.abspath(vt.__file__).startswith(os.path.abspath(ref_dir)), vt.__file__
    vt.cv2 = cv2
    return vt, cv2


def observe(calls):
    """(mode, pad_top, pad_bottom, alpha, c0, c1, c2, size) of one do_pad, from the calls it made"""
    borders = [c for c in calls if c[0] == "border"]
    weighted = [c for c in calls if c[0] == "weighted"]
    resizes = [c for c in calls if c[0] == "resize"]
    assert len(resizes) == 1 and resizes[0][2] == "cubic" and resizes[0][1][0] == resizes[0][1][1], calls
    size = resizes[0][1][0]
    if not borders:
        assert not weighted
        return (NONE, 0, 0, float("nan"), 0, 0, 0, size)
    assert all(b[3] == 0 and b[4] == 0 and b[1:3] == borders[0][1:3] for b in borders)
    top, bottom = borders[0][1:3]
    kinds = [b[5] for b in borders]
    if kinds == ["reflect", "constant"]:
        (_, alpha, beta, gamma), = weighted
        assert list(borders[1][6]) == [0, 0, 0] and beta == 1 - alpha and gamma == 0
        return (REFLECT, top, bottom, alpha, 0, 0, 0, size)
    assert not weighted and len(borders) == 1
    if kinds == ["replicate"]:
        return (REPLICATE, top, bottom, float("nan"), 0, 0, 0, size)
    assert kinds == ["constant"]
    colour = list(borders[0][6])
    return (COLOR if any(colour) else BLACK, top, bottom, float("nan"), *colour, size)


def build(vt, cv2):
    arrs = {"cases": np.array(CASES, dtype=np.int64), "crop_size": np.array(CROP)}
    for seed, h, w in CASES:
        torch.manual_seed(seed)
        rows = []
        for _ in range(CLIPS):
            do_pad = vt.pad_wide_clips(h, w, CROP)
            del cv2.calls[:]
            do_pad(object())
            rows.append(observe(cv2.calls))
        key = f"s{seed}.{h}x{w}"
        arrs[f"{key}.pads"] = np.array(rows, dtype=np.float64)
        arrs[f"{key}.state"] = torch.get_rng_state().numpy()
        print(f"{key}: modes {[int(r[0]) for r in rows]}")
    return arrs


def check_coverage(arrs):
    """the cases cover what they are there for"""
    wide = np.concatenate([arrs[f"s{s}.{h}x{w}.pads"] for s, h, w in CASES if w > h])
    assert set(wide[:, 0].astype(int)) == {NONE, BLACK, COLOR, REFLECT, REPLICATE}
    for s, h, w in CASES:
        p = arrs[f"s{s}.{h}x{w}.pads"]
        assert (p[:, 7] == CROP).all() and (p[:, 1:3] <= 0.5 * max(w - h, 0) + 0.5).all()
        if w <= h:
            assert (p[:, 0] == NONE).all()
    refl = wide[wide[:, 0] == REFLECT]
    assert ((refl[:, 3] >= 0) & (refl[:, 3] <= 0.7)).all() and np.isnan(wide[wide[:, 0] != REFLECT][:, 3]).all()


def write_npz(path, arrs):
    """an .npz (deflated) whose bytes depend on the arrays alone: fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TAD_REFERENCE"))
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "video_transforms.py")):
        sys.exit("give the reference's checkout: --reference DIR or TAD_REFERENCE")
    arrs = build(*import_reference(args.reference))
    check_coverage(arrs)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g23_frame_ingest.npz")
    write_npz(path, arrs)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB, {len(arrs)} arrays)")
    assert size <= 1 << 20, size


if __name__ == "__main__":
    main()
