#!/usr/bin/env python3
"""Generate ``tests/golden/g22_sequencing.npz`` by running the REAL reference (``dataset.sequencing`` imported from its checkout; numpy
and torch only) on the cases of ``tests/sequencing_recipe.py``:

* ``<case>.count`` -- the number of windows ``get_sequences`` returns, -1 where it returns ``None``;
* ``<case>.idx``   -- all window indices flattened (count * seq_length int64 values; empty for ``None``);
* ``<case>.seq_length`` / ``<case>.seq_step`` -- the attributes the reference's object carries.

The fixture holds arrays only.  Runs only where the reference is present; nothing of its source text is copied.

usage: python tools/make_goldens_sequencing.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_goldens as MG  # noqa: E402  (REF, save; it puts tests/ on sys.path)
import sequencing_recipe as SR  # noqa: E402


def main():
    sys.path.insert(0, MG.REF)
    from dataset import sequencing as ref
    assert ref.__file__.startswith(MG.REF)
    arrs = {}
    for case in SR.CASES:
        seq, windows = SR.run_case(ref, case)
        count, flat = SR.pack(windows)
        name = case["name"]
        arrs[f"{name}.count"], arrs[f"{name}.idx"] = count, flat
        arrs[f"{name}.seq_length"], arrs[f"{name}.seq_step"] = np.array(seq.seq_length, dtype=np.int64), np.array(seq.seq_step, dtype=np.int64)
        print("G22", name, "windows:", int(count), "first:", None if windows is None else windows[0], "last:", None if windows is None else windows[-1])
        if name in SR.EXPECTED_COUNTS:
            assert int(count) == SR.EXPECTED_COUNTS[name], (name, int(count))
    MG.save("g22_sequencing", **arrs)
    assert os.path.getsize(os.path.join(MG.OUT, "g22_sequencing.npz")) <= 100_000


if __name__ == "__main__":
    main()
