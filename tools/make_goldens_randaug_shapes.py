#!/usr/bin/env python3
"""Generate ``tests/golden/g25_rand_augment_shapes.npz``: the per-op cases of fixture G16 (tools/make_goldens_randaug.py) at the other
shapes of ``tests/randaug_recipe.py`` (``RR.SHAPES``: frames of one pixel, one row, one column, below 3 pixels in a direction, a real
224 x 224 frame, non-square mid sizes), by running the REAL reference's ``rand_augment.AugmentOp`` (the same checkout as the G16 tool
reads; numpy and PIL only) on the seeded frames of ``RR.frames_at``.

Per shape ``<B>x<T>x<H>x<W>`` and per case of ``RR.op_cases()``: ``AugmentOp(name, prob=1.0, magnitude=m, hparams)`` on the PIL frames
of each clip, ``random.seed(seed)`` before each clip so that all clips share the sign.  Stored per shape, in the order of
``RR.op_cases()`` (whose keys are stored as ``cases``): the argument the level function returned (``<shape>.args``, NaN for the ops
without one) and the SHA-256 of every output frame (``<shape>.sha``, uint8 [case, B, T, 32]), not the frames; and the SHA-256 of the
inputs (``<shape>.input.sha``).  The reference is observed from outside; nothing of its text is copied.  A second run gives the same
arrays, and says so.

usage: python tools/make_goldens_randaug_shapes.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import randaug_recipe as RR  # noqa: E402
from make_goldens_randaug import REF, pil_clip  # noqa: E402


def shape_cases(ref, Image, shape):
    B, T, H, W = shape
    sk = RR.shape_key(shape)
    x = RR.frames_at(B, T, H, W, RR.SHAPES_SEED)
    arrs = {f"{sk}.input.sha": RR.digest(x)}
    cases = RR.op_cases()
    args = np.zeros(len(cases), dtype=np.float64)
    shas = np.zeros((len(cases), B, T, 32), dtype=np.uint8)
    changed = 0
    for k, (key, name, m, seed, rs) in enumerate(cases):
        op = ref.AugmentOp(name, prob=1.0, magnitude=m, hparams={"translate_const": int(H * 0.45), "interpolation": rs})
        random.seed(seed)
        arg = op.level_fn(m, op.hparams)[0] if op.level_fn is not None else float("nan")
        for b in range(B):
            random.seed(seed)
            for t, img in enumerate(op(pil_clip(Image, x, b))):
                out = np.asarray(img)
                assert out.shape == (H, W, 3) and out.dtype == np.uint8, (sk, key, out.shape)
                shas[k, b, t] = RR.digest(out)
                changed += int((out != x[b, t]).any())
        args[k] = arg
    arrs[f"{sk}.args"], arrs[f"{sk}.sha"] = args, shas
    print(f"{sk}: {len(cases)} cases, {changed} of {len(cases) * B * T} output frames differ from their input")
    return arrs


def main():
    sys.path.insert(0, REF)
    import rand_augment as ref
    from PIL import Image
    assert ref.__file__.startswith(REF)
    for seed, negated in zip(RR.SIGN_SEEDS, (True, False)):
        random.seed(seed)
        assert (random.random() > 0.5) == negated
    arrs = {"shapes": np.array(RR.SHAPES, dtype=np.int32), "seed": np.array(RR.SHAPES_SEED, dtype=np.int32),
            "cases": np.array([c[0] for c in RR.op_cases()])}
    for shape in RR.SHAPES:
        arrs.update(shape_cases(ref, Image, shape))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g25_rand_augment_shapes.npz")
    if os.path.exists(path):
        with np.load(path, allow_pickle=False) as old:
            same = set(old.files) == set(arrs) and all(old[k].dtype == arrs[k].dtype and old[k].tobytes() == arrs[k].tobytes() for k in arrs)
        print("the arrays equal those of the existing file" if same else "the arrays DIFFER from those of the existing file")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB, {len(arrs)} arrays)")
    assert size <= 1 << 20, size


if __name__ == "__main__":
    main()
