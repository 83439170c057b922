#!/usr/bin/env python3
"""Generate ``tests/golden/g15_random_erasing.npz`` by running the REAL reference's ``random_erasing.RandomErasing`` (imported from
/root/reference; ``random`` and torch only, CPU) on the seeded inputs of ``tests/erasing_recipe.py``.

Per case ``<mode>.<configuration>.<seed>`` the reference is called on each [T,C,H,W] clip of a batch [B,C,T,H,W] in turn, as its
datasets call it, with one continuing ``random`` stream (``random.seed(seed)`` and ``torch.manual_seed(seed)`` before the first clip).
Stored: the packed boolean mask of the changed elements, the SHA-256 of the erased batch's bytes plus every 13th element of it, and one
further ``random.random()`` drawn after the last clip (pins the position of the stream).

The fixture holds arrays only.  Runs only where the reference is present; nothing of its source text is copied.

usage: python tools/make_goldens_erasing.py
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import erasing_recipe as ER  # noqa: E402


def cases(ref):
    arrs = {}
    for key, mode, name, seed, shape in ER.cases():
        x = ER.clip(key, shape)
        before = x.clone()
        fn = ref.RandomErasing(**ER.erasing_kwargs(mode, name))
        random.seed(seed)
        torch.manual_seed(seed)
        for b in range(shape[0]):
            view = x[b].permute(1, 0, 2, 3)          # [T,C,H,W], as dota.py:327-329 hands it over
            assert fn(view) is view
        arrs[f"{key}.next"] = np.array(random.random())
        changed = (x != before).numpy()
        per_clip = changed.reshape(shape[0], -1).any(1)
        p = ER.CONFIGS[name]["probability"]
        assert per_clip.any() and (p >= 1.0 or not per_clip.all()), (key, per_clip)   # no case is a no-op, none with p < 1 erases all
        arrs[f"{key}.mask"] = ER.pack_mask(changed)
        arrs[f"{key}.sha"] = ER.digest(x)
        arrs[f"{key}.sample"] = ER.sample(x)
        print(f"{key}: {int(changed.sum())} of {changed.size} elements changed, clips {per_clip.astype(int).tolist()}")
    return arrs


def main():
    torch.set_num_threads(1)
    sys.path.insert(0, REF)
    import random_erasing as ref
    assert ref.__file__.startswith(REF)
    arrs = cases(ref)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g15_random_erasing.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB)")
    assert size <= 100_000, size


if __name__ == "__main__":
    main()
