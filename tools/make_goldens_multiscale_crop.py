#!/usr/bin/env python3
"""Generate ``tests/golden/g18_multiscale_crop.npz`` by running the REAL reference's ``transforms.GroupMultiScaleCrop`` (imported
from a checkout of the reference; numpy and PIL only) on the seeded frames of ``tests/multiscale_crop_recipe.py``.

Per case: ``random.seed(seed)``, then the transform on the PIL frames of clip 0, 1, 2 in one process.  Stored: the crop
``(w, h, x0, y0)`` of every clip (observed from outside: ``_sample_crop_size`` is wrapped), the next ``random.random()`` after the
last clip (the position of the stream) and the output frames.  Nothing of the reference's text is copied.  The inputs are not
stored: only their SHA-256.

The reference's ``transforms.py`` imports ``torchvision`` at module level; where torchvision is not installed, empty stand-in
modules are registered for ``torchvision``, ``torchvision.transforms`` and ``torchvision.transforms.functional`` before the import
(``GroupMultiScaleCrop`` touches none of them).

usage: python tools/make_goldens_multiscale_crop.py [--reference DIR]      (default: $TAD_REFERENCE)
"""
import argparse
import importlib
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiscale_crop_recipe as MR  # noqa: E402


def import_reference(ref_dir):
    try:
        importlib.import_module("torchvision")
    except ImportError:
        for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
        sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    sys.path.insert(0, ref_dir)
    ref = importlib.import_module("transforms")
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(ref_dir)), ref.__file__
    return ref


def build(ref, Image):
    arrs = {"input.sha": MR.inputs_digest()}
    for key, seed, (Hs, Ws), S, kw, kind in MR.CASES:
        x = MR.frames(Hs, Ws, kind)
        tf = ref.GroupMultiScaleCrop(S, **{k: list(v) if k == "scales" else v for k, v in kw.items()})
        crops = []
        orig = tf._sample_crop_size

        def watch(im_size, orig=orig, crops=crops):
            r = orig(im_size)
            crops.append([int(v) for v in r])
            return r

        tf._sample_crop_size = watch
        random.seed(seed)
        out = np.zeros((MR.B, MR.T, S, S, 3), dtype=np.uint8)
        for b in range(MR.B):
            imgs, _ = tf(([Image.fromarray(x[b, t]) for t in range(MR.T)], None))
            for t, img in enumerate(imgs):
                out[b, t] = np.asarray(img)
        arrs[f"{key}.next_py"] = np.array(random.random())
        arrs[f"{key}.crops"] = np.array(crops, dtype=np.int32)
        arrs[f"{key}.out"] = out
        print(f"{key}: crops (w, h, x0, y0) {crops}")
    return arrs


def check_coverage(arrs):
    """the cases cover what they are there for"""
    crops = {c[0]: arrs[f"{c[0]}.crops"] for c in MR.CASES}
    assert (crops["snap.34x60"][:, :2] == 32).any() and (crops["snap.34x60"][:, :2] != 32).any()
    assert (crops["k17.120x200"][:, :2] > 16 * 7).any()
    four = np.concatenate([crops[k] for k in crops if k.startswith("down.")])
    assert len({tuple(r[:2]) for r in four}) >= 4 and len({tuple(r[2:]) for r in four}) >= 6
    assert (crops["up.20x23"][:, :2] < 32).all()
    for r in crops["nodistort.45x80"]:
        assert r[0] == r[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TAD_REFERENCE"))
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "transforms.py")):
        sys.exit("give the reference's checkout: --reference DIR or TAD_REFERENCE")
    from PIL import Image
    arrs = build(import_reference(args.reference), Image)
    check_coverage(arrs)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g18_multiscale_crop.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB, {len(arrs)} arrays)")
    assert size <= 1 << 20, size


if __name__ == "__main__":
    main()
