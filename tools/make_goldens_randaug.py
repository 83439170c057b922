#!/usr/bin/env python3
"""Generate ``tests/golden/g16_rand_augment.npz`` by running the REAL reference's ``rand_augment.py`` (imported from /root/reference;
numpy and PIL only) on the seeded frames of ``tests/randaug_recipe.py``.

Per-op cases ``op.<name>...``: ``AugmentOp(name, prob=1.0, magnitude=m, hparams)`` on the two PIL frames of each of the three clips,
``random.seed(seed)`` before each clip so that all clips share the sign.  Stored: the argument the level function returned and the
output frames.  Policy cases ``policy...``: the whole ``rand_augment_transform`` under ``random.seed(s); np.random.seed(s)``, clip
after clip in one process.  Stored per (clip, layer): the chosen op's name, whether it was applied, its argument, the resample mode of
every frame; then the next ``random.random()`` and ``np.random.random()`` (the positions of both streams) and the output frames.
What the reference chose is observed from outside (its ops' functions are wrapped); nothing of its text is copied.  The inputs are
not stored: only their SHA-256.

usage: python tools/make_goldens_randaug.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import randaug_recipe as RR  # noqa: E402


def pil_clip(Image, x, b):
    return [Image.fromarray(x[b, t]) for t in range(x.shape[1])]


def op_cases(ref, Image, x):
    arrs = {}
    for seed, negated in zip(RR.SIGN_SEEDS, (True, False)):
        random.seed(seed)
        assert (random.random() > 0.5) == negated
    for key, name, m, seed, rs in RR.op_cases():
        op = ref.AugmentOp(name, prob=1.0, magnitude=m, hparams={"translate_const": int(RR.H * 0.45), "interpolation": rs})
        random.seed(seed)
        arg = op.level_fn(m, op.hparams)[0] if op.level_fn is not None else float("nan")
        out = np.zeros_like(x)
        for b in range(x.shape[0]):
            random.seed(seed)
            for t, img in enumerate(op(pil_clip(Image, x, b))):
                out[b, t] = np.asarray(img)
        assert (out != x).any(), key
        arrs[f"{key}.arg"] = np.array(arg, dtype=np.float64)
        arrs[f"{key}.out"] = out
        print(f"{key}: arg {arg}, {int((out != x).sum())} of {x.size} bytes changed")
    return arrs


def policy_cases(ref, Image, x, drive):
    arrs = {}
    Bn, Tn = x.shape[:2]
    for key, seed, oplist, interp in RR.POLICIES:
        hp = {"translate_const": int(RR.H * 0.45)}
        if interp is not None:
            hp["interpolation"] = interp
        names = list(drive) if oplist == "drive" else None
        ra = ref.rand_augment_transform(RR.POLICY, hp, names)
        names = names or list(ref._RAND_INCREASING_TRANSFORMS)
        name_of = {id(op): n for op, n in zip(ra.ops, names)}
        log = []                              # one entry per op call: [name, applied, arg, [resample per frame]]

        def watch_call(orig):
            def call(self, img_list):
                log.append([name_of[id(self)], False, float("nan"), []])
                return orig(self, img_list)
            return call

        def watch_fn(fn):
            def run(img, *args, **kw):
                log[-1][1] = True
                if args:
                    log[-1][2] = float(args[0])
                return fn(img, *args, **kw)
            return run

        def watch_interp(orig):
            def pick(kwargs):
                r = orig(kwargs)
                log[-1][3].append(int(r))
                return r
            return pick

        saved = ref.AugmentOp.__call__, ref._interpolation
        ref.AugmentOp.__call__ = watch_call(saved[0])
        ref._interpolation = watch_interp(saved[1])
        for op in ra.ops:
            op.aug_fn = watch_fn(op.aug_fn)
        try:
            random.seed(seed)
            np.random.seed(seed)
            out = np.zeros_like(x)
            for b in range(Bn):
                for t, img in enumerate(ra(pil_clip(Image, x, b))):
                    out[b, t] = np.asarray(img)
            arrs[f"{key}.next_py"] = np.array(random.random())
            arrs[f"{key}.next_np"] = np.array(np.random.random())
        finally:
            ref.AugmentOp.__call__, ref._interpolation = saved
        assert len(log) == Bn * ra.num_layers == Bn * 3
        arrs[f"{key}.ops"] = np.array([e[0] for e in log])
        arrs[f"{key}.applied"] = np.array([e[1] for e in log])
        arrs[f"{key}.args"] = np.array([e[2] for e in log], dtype=np.float64)
        arrs[f"{key}.resample"] = np.array([(e[3] + [0] * Tn)[:Tn] for e in log], dtype=np.int8)
        arrs[f"{key}.out"] = out
        print(f"{key}: " + "  ".join(f"{e[0]}{'' if e[1] else '(skipped)'}" for e in log))
    return arrs


def drive_transforms():
    """the list of names video_transforms.DRIVE_TRANSFORMS, read as data (the module itself needs cv2)"""
    import ast
    with open(os.path.join(REF, "video_transforms.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "DRIVE_TRANSFORMS":
            return ast.literal_eval(node.value)
    raise KeyError("DRIVE_TRANSFORMS")


def main():
    sys.path.insert(0, REF)
    import rand_augment as ref
    from PIL import Image
    assert ref.__file__.startswith(REF)
    x = RR.frames()
    arrs = {"input.sha": RR.digest(x)}
    arrs.update(op_cases(ref, Image, x))
    arrs.update(policy_cases(ref, Image, x, drive_transforms()))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g16_rand_augment.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB, {len(arrs)} arrays)")
    assert size <= 1 << 20, size


if __name__ == "__main__":
    main()
