#!/usr/bin/env python3
"""Generate ``tests/golden/g20_spatial_sampling.npz`` by running the REAL reference's ``spatial_sampling`` (``kinetics.py``, imported
from a checkout of the reference; CPU torch) on the seeded clips of ``tests/spatial_sampling_recipe.py``.

Per case: ``random.seed(seed)`` and ``np.random.seed(seed)``, then ``spatial_sampling`` on clip 0, 1, 2 in one process.  Stored:

* ``windows`` int32 [B * T, 11] = (clip, frame, i, j, h, w, rh, rw, oy, ox, flip): the source window every frame was resized from, the
  grid it was resized to, the offset of the crop in that grid and the flip.  All observed from outside: ``interpolate`` is watched for
  the view it is given and the size it is asked for, ``random_crop`` / ``uniform_crop`` for the view they return, ``horizontal_flip``
  for whether it returns another tensor;
* ``next_py`` / ``next_np``: the next ``random.random()`` and ``np.random.uniform()`` after the last clip (the positions of the streams);
* ``out`` f32 [B, 3, T, S, S];
* ``gap`` = max |out - out64|, where out64 is the same call under the same draws on the ``.double()`` clip: how far the reference's own
  f32 arithmetic is from the exact resample.  (With ``motion_shift`` the reference collects the frames in an f32 tensor, so out64 is
  the double resample rounded to f32 once.)

Nothing of the reference's text is copied.  The inputs are not stored: only their SHA-256.  The archive is written with fixed
timestamps, so the file regenerates byte for byte.

``kinetics.py`` and ``video_transforms.py`` import ``cv2``, ``decord``, ``torchvision``, ``pandas`` and ``tqdm`` at module level; for
each of those that is not installed an empty stand-in module is registered before the import (``spatial_sampling`` touches none).

usage: python tools/make_goldens_spatial_sampling.py [--reference DIR]      (default: $TAD_REFERENCE)
"""
import argparse
import importlib
import io
import os
import random
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spatial_sampling_recipe as SR  # noqa: E402


class _StandIn(types.ModuleType):
    """an empty module: any name asked of it is an empty class (enough for ``from x import y`` and for a base class)"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = sys.modules.get(f"{self.__name__}.{name}")
        return sub if sub is not None else type(name, (), {})


def import_reference(ref_dir):
    for name in ("cv2", "decord", "torchvision", "pandas", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            subs = ("", ".transforms", ".transforms.functional") if name == "torchvision" else ("",)
            for sub in subs:
                sys.modules[name + sub] = _StandIn(name + sub)
    sys.path.insert(0, ref_dir)
    ref = importlib.import_module("kinetics")
    vt = importlib.import_module("video_transforms")
    for m in (ref, vt):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_dir)), m.__file__
    return ref, vt


class Watch:
    """what one call of spatial_sampling did to its clip, seen from outside"""

    def __init__(self, vt):
        self.vt = vt
        self.saved = {}

    def __enter__(self):
        vt, F = self.vt, torch.nn.functional
        self.resizes, self.crop, self.flip = [], None, 0
        self.saved = {"interpolate": F.interpolate, "random_crop": vt.random_crop, "uniform_crop": vt.uniform_crop,
                      "horizontal_flip": vt.horizontal_flip}

        def interpolate(input, size=None, **kw):
            self.resizes.append((input.storage_offset(), tuple(input.shape), tuple(int(v) for v in size)))
            return self.saved["interpolate"](input, size=size, **kw)

        def cropper(name):
            def crop(images, *a, **kw):
                r = self.saved[name](images, *a, **kw)
                view = r[0] if isinstance(r, tuple) else r
                assert images.is_contiguous()
                self.crop = divmod(view.storage_offset() - images.storage_offset(), images.shape[3])
                return r
            return crop

        def horizontal_flip(prob, images, *a, **kw):
            r = self.saved["horizontal_flip"](prob, images, *a, **kw)
            self.flip = int(r[0] is not images)
            return r

        F.interpolate = interpolate
        vt.random_crop, vt.uniform_crop, vt.horizontal_flip = cropper("random_crop"), cropper("uniform_crop"), horizontal_flip
        return self

    def __exit__(self, *exc):
        torch.nn.functional.interpolate = self.saved["interpolate"]
        for name in ("random_crop", "uniform_crop", "horizontal_flip"):
            setattr(self.vt, name, self.saved[name])

    def windows(self, clip, T, H, W, S):
        """the rows (clip, frame, i, j, h, w, rh, rw, oy, ox, flip) of the call"""
        oy, ox = self.crop if self.crop is not None else (0, 0)
        if not self.resizes:                                  # the jitter left the clip as it was
            per_frame = [(0, 0, H, W, H, W)] * T
        elif len(self.resizes) == 1:                          # one resize of all frames
            off, shape, size = self.resizes[0]
            assert shape[1] == T
            i, j = divmod(off, W)
            per_frame = [(i, j, shape[2], shape[3], *size)] * T
        else:                                                 # one resize per frame (motion_shift)
            assert len(self.resizes) == T
            per_frame = []
            for t, (off, shape, size) in enumerate(self.resizes):
                assert shape[1] == 1
                i, j = divmod(off - t * H * W, W)
                per_frame.append((i, j, shape[2], shape[3], *size))
        for win in per_frame:
            assert 0 <= win[0] and win[0] + win[2] <= H and 0 <= win[1] and win[1] + win[3] <= W, win
        return [(clip, t, *win, oy, ox, self.flip) for t, win in enumerate(per_frame)]


def build(ref, vt):
    arrs = {"input.sha": SR.inputs_digest()}
    for key, seed, (H, W), kw in SR.CASES:
        x = torch.from_numpy(SR.clips(H, W))
        S = kw["crop_size"]
        random.seed(seed)
        np.random.seed(seed)
        out = np.zeros((SR.B, 3, SR.T, S, S), dtype=np.float32)
        rows, gap = [], 0.0
        for b in range(SR.B):
            state = random.getstate(), np.random.get_state()
            clip = x[b].clone()                                           # (its own storage: the watched offsets count from frame 0)
            with Watch(vt) as watch:
                got = ref.spatial_sampling(clip, **kw)
            rows += watch.windows(b, SR.T, H, W, S)
            after = random.getstate(), np.random.get_state()
            random.setstate(state[0])
            np.random.set_state(state[1])
            got64 = ref.spatial_sampling(clip.double(), **kw)           # the same draws, in doubles
            assert random.getstate() == after[0] and all(np.array_equal(p, q) for p, q in zip(np.random.get_state(), after[1]))
            # (motion_shift collects its frames in an f32 tensor whatever the clip's type: there out64 is the double resample rounded once)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, SR.T, S, S)
            assert got64.dtype == (torch.float32 if kw.get("motion_shift") else torch.float64)
            out[b] = got.numpy()
            gap = max(gap, float((got.double() - got64).abs().max()))
        arrs[f"{key}.next_py"] = np.array(random.random())
        arrs[f"{key}.next_np"] = np.array(np.random.uniform())
        arrs[f"{key}.windows"] = np.array(rows, dtype=np.int32)
        arrs[f"{key}.out"] = out
        arrs[f"{key}.gap"] = np.array(gap)
        print(f"{key}: gap {gap:.3g}; windows of frame 0 (i, j, h, w, rh, rw, oy, ox, flip) {[r[2:] for r in rows if r[1] == 0]}")
    return arrs


def check_coverage(arrs):
    """the cases cover what they are there for"""
    win = {c[0]: arrs[f"{c[0]}.windows"] for c in SR.CASES}
    assert (win["wide1.37x53"][:, 5] == 1).all() and (win["wide1.37x53"][:, 4] > 1).all()
    assert (win["high1.37x53"][:, 4] == 1).all() and (win["high1.37x53"][:, 5] > 1).all()
    assert (win["fallback.6x120"][:, 2:6] == (0, 56, 6, 8)).all()
    assert (win["noflip.37x53"][:, 10] == 0).all()
    flips = np.concatenate([win[k][:, 10] for k in win if not k.startswith(("noflip", "idx"))])
    assert (flips == 0).any() and (flips == 1).any()
    assert (win["up.17x19"][:, 4:6] < 32).all() and (win["down.37x53"][:, 4:6] > 16).any()
    shift = win["shift.37x53"].reshape(SR.B, SR.T, 11)
    assert any(len({tuple(r[2:6]) for r in clip}) > 1 for clip in shift)                 # frames of a clip have boxes of their own
    assert (win["scale1.20x27"][:, 4:8] == (20, 27, 20, 27)).all() and (win["scale1.20x27"][:, 8:10] > 0).any()
    assert float(arrs["scale1.20x27.gap"]) == 0.0
    for k in ("jitter.20x27", "inverse.20x27"):
        assert (win[k][:, 2:6] == (0, 0, 20, 27)).all() and len({tuple(r[6:8]) for r in win[k]}) > 1
    assert [tuple(win[f"idx{i}.10x14"][0, 6:10]) for i in range(3)] == [(8, 11, 0, 0), (8, 11, 0, 2), (8, 11, 0, 3)]
    assert [tuple(win[f"idx{i}.15x10"][0, 6:10]) for i in range(3)] == [(12, 8, 0, 0), (12, 8, 2, 0), (12, 8, 4, 0)]


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
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "kinetics.py")):
        sys.exit("give the reference's checkout: --reference DIR or TAD_REFERENCE")
    arrs = build(*import_reference(args.reference))
    check_coverage(arrs)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g20_spatial_sampling.npz")
    write_npz(path, arrs)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB, {len(arrs)} arrays)")
    assert size <= 1 << 20, size


if __name__ == "__main__":
    main()
