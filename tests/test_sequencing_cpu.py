"""simple_tad_amd.sequencing against the reference's dataset/sequencing.py, index for index (fixture G22: tests/golden/g22_sequencing.npz,
cases in tests/sequencing_recipe.py), plus the reference's assertion errors."""
import os

import numpy as np
import pytest

import sequencing_recipe as SR
from simple_tad_amd import sequencing as S

G22 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_sequencing.npz"))
BY_NAME = {c["name"]: c for c in SR.CASES}


def windows_of(name):
    return SR.run_case(S, BY_NAME[name])[1]


@pytest.mark.parametrize("name", [c["name"] for c in SR.CASES])
def test_windows_equal_the_reference(name):
    seq, windows = SR.run_case(S, BY_NAME[name])
    count, flat = SR.pack(windows)
    assert int(count) == int(G22[f"{name}.count"])
    assert (windows is None) == (int(G22[f"{name}.count"]) == -1)
    assert flat.dtype == G22[f"{name}.idx"].dtype and np.array_equal(flat, G22[f"{name}.idx"])
    assert seq.seq_length == int(G22[f"{name}.seq_length"]) and seq.seq_step == int(G22[f"{name}.seq_step"])
    if windows is not None:
        assert all(isinstance(i, int) for w in windows for i in w) and all(len(w) == seq.seq_length for w in windows)


def test_fixture_holds_what_was_measured_on_the_reference():
    """the window counts and landmarks stated with the cases (measured on the reference on the CPU), read from the FIXTURE"""
    for name, n in SR.EXPECTED_COUNTS.items():
        assert int(G22[f"{name}.count"]) == n, name

    def fx(name, length):
        return G22[f"{name}.idx"].reshape(-1, length)
    assert fx("reg_step2", 16)[0, 0] == 1
    w = fx("reg_fps3", 16)
    assert w[-1, -1] == 60 and (np.diff(w, axis=1) == 3).all()
    assert fx("start_added", 4)[-1].tolist() == [0, 1, 2, 3] and np.array_equal(fx("start_added", 4)[:4], fx("reg_len4", 4))
    assert fx("unsafe_none", 4)[:, -1].tolist() == [4, 9, 12, 13, 14, 19]
    assert fx("unsafe_fps3", 4)[0].tolist() == [2, 5, 8, 11]
    assert int(G22["reg_view1.count"]) == 101


def test_return_types_and_inputs():
    assert windows_of("reg_short") is None and windows_of("start_short") is None and windows_of("reg_fps3_short") is None
    r = S.RegularSequencer(10, 4, 5)
    by_count = r.get_sequences(23, 10)
    assert r.get_sequences(list(range(23)), 10) == by_count and r.get_sequences(np.zeros(23), 10) == by_count
    import torch
    assert r.get_sequences(torch.zeros(23), 10) == by_count
    assert isinstance(r, S.BasicSequencer_Abs) and isinstance(S.UnsafeOverlapSequencer(10, 4), S.BasicLabeledSequencer_Abs)
    assert S.UnsafeOverlapSequencer(10, 4, 5, 2).surrounding_timesteps == (2, 2)
    assert S.UnsafeOverlapSequencer(10, 4, 5).surrounding_timesteps == (0, 0)
    with pytest.warns(UserWarning):
        assert S.RegularSequencer(10, 1.6).seq_length == 16


def test_assertions_of_the_reference():
    for cls in (S.RegularSequencer, S.RegularSequencerWithStart, S.UnsafeOverlapSequencer):
        with pytest.raises(AssertionError, match="Step must be at least 1"):
            cls(10, 16, 0)
        with pytest.raises(AssertionError, match="non-zero and positive"):
            cls(0, 16)
        with pytest.raises(ValueError):
            cls(10, "16")
        arg = [False] * 40 if cls is S.UnsafeOverlapSequencer else 40
        with pytest.raises(AssertionError, match="divisible"):
            cls(10, 16).get_sequences(arg, 25)
        with pytest.raises(AssertionError, match="must be positive"):
            cls(10, 16).get_sequences(arg, 0)
    with pytest.raises(AssertionError):
        S.UnsafeOverlapSequencer(10, 4, 1, (1, -1))
