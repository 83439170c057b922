"""Cases of the sequencing fixture G22 (tests/golden/g22_sequencing.npz, written by tools/make_goldens_sequencing.py from the
reference's own ``dataset.sequencing``).  The fixture holds results only: per case the number of windows (-1 where the reference
returns ``None``) and all window indices flattened; every input is restated here.

A case: (name, class name, constructor kwargs, frames, input fps, labels).  ``labels`` is None for the two regular sequencers (they
are called with the frame COUNT) and a list of bools for UnsafeOverlapSequencer (then ``frames == len(labels)``)."""

_L20 = [False] * 12 + [True] * 3 + [False] * 5
_L30 = [False] * 20 + [True] * 4 + [False] * 6


def _c(name, cls, kw, frames, fps, labels=None):
    assert labels is None or len(labels) == frames
    return dict(name=name, cls=cls, kw=kw, frames=frames, fps=fps, labels=labels)


def _r(freq, length, step):
    return dict(seq_frequency=freq, seq_length=length, step=step)


CASES = [
    _c("reg_exact", "RegularSequencer", _r(10, 16, 1), 16, 10),
    _c("reg_short", "RegularSequencer", _r(10, 16, 1), 15, 10),
    _c("reg_step2", "RegularSequencer", _r(10, 16, 2), 41, 10),
    _c("reg_fps3", "RegularSequencer", _r(10, 16, 3), 61, 30),
    _c("reg_len4", "RegularSequencer", _r(10, 4, 5), 23, 10),
    _c("reg_view1", "RegularSequencer", _r(10, 16, 1), 116, 10),        # the scoring benchmark's video: 101 windows
    _c("reg_fps3_short", "RegularSequencer", _r(10, 16, 1), 45, 30),    # span 46 > 45 frames
    _c("start_added", "RegularSequencerWithStart", _r(10, 4, 5), 23, 10),
    _c("start_plain", "RegularSequencerWithStart", _r(10, 16, 10), 70, 10),
    _c("start_short", "RegularSequencerWithStart", _r(10, 16, 1), 15, 10),
    _c("start_fps3", "RegularSequencerWithStart", _r(10, 4, 7), 40, 30),
    _c("unsafe_none", "UnsafeOverlapSequencer", dict(_r(10, 4, 5), surrounding_timesteps=None), 20, 10, _L20),
    _c("unsafe_2", "UnsafeOverlapSequencer", dict(_r(10, 4, 5), surrounding_timesteps=2), 20, 10, _L20),
    _c("unsafe_1_3", "UnsafeOverlapSequencer", dict(_r(10, 4, 5), surrounding_timesteps=(1, 3)), 20, 10, _L20),
    _c("unsafe_fps3", "UnsafeOverlapSequencer", dict(_r(10, 4, 2), surrounding_timesteps=1), 30, 30, _L30),
    _c("unsafe_last", "UnsafeOverlapSequencer", dict(_r(10, 4, 3), surrounding_timesteps=1), 12, 10, [False] * 11 + [True]),
]

# what the issue's author measured on the reference (window counts; -1 = None), restated so that the fixture itself is checked too
EXPECTED_COUNTS = {"reg_exact": 1, "reg_short": -1, "reg_step2": 13, "reg_fps3": 6, "reg_len4": 4, "start_added": 5, "start_plain": 7,
                   "unsafe_none": 6, "unsafe_2": 10, "unsafe_1_3": 10, "unsafe_fps3": 9}


def run_case(module, case):
    """``get_sequences`` of the case on ``module`` (the reference's dataset.sequencing or simple_tad_amd.sequencing)"""
    seq = getattr(module, case["cls"])(**case["kw"])
    return seq, seq.get_sequences(case["frames"] if case["labels"] is None else list(case["labels"]), case["fps"])


def pack(windows):
    """(count, flat int64 indices): what the fixture stores per case"""
    import numpy as np
    if windows is None:
        return np.array(-1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.array(len(windows), dtype=np.int64), np.asarray(windows, dtype=np.int64).reshape(-1)
