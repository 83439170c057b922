"""Which frames form window i of a video (reference: dataset/sequencing.py; used by every dataset, e.g. dota.py:209, 555).

A sequencer turns a video of F frames recorded at ``input_frequency`` into windows of ``seq_length`` frame indices spaced
``input_frequency // seq_frequency`` apart.  All three anchor their windows at the END of the video: the last window always ends on
frame F - 1, and the first regular window starts at whatever remainder the step leaves.  Constructor arguments, attribute names,
``get_sequences`` signatures, return values (lists of lists of ints, ``None`` for a video shorter than one window) and the
assertions are the reference's; tests/golden/g22_sequencing.npz pins them index for index.

The span of one window in input frames is ``span = (seq_length - 1) * fps_step + 1`` (the reference's ``actual_seq_length``).
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

__all__ = ["BasicSequencer_Abs", "BasicLabeledSequencer_Abs", "RegularSequencer", "RegularSequencerWithStart", "UnsafeOverlapSequencer"]


def _check_step(step):
    assert step > 0, f"Step must be at least 1. Given: {step}"


def _fps_step(input_frequency, seq_frequency):
    assert input_frequency > 0, f"Input frequency must be positive. Given: {input_frequency}"
    assert input_frequency % seq_frequency == 0, \
        ("Cannot convert input frequency to target frequency! Input frequency must be divisible by target "
         f"frequency. Input frequency: {input_frequency}, target frequency: {seq_frequency}")
    return input_frequency // seq_frequency


def _count(timesteps_nb):
    return len(timesteps_nb) if isinstance(timesteps_nb, (Sequence, np.ndarray, torch.Tensor)) else timesteps_nb


class BasicSequencer_Abs:
    def __init__(self, seq_frequency: int, seq_length: Union[int, float]):
        assert seq_frequency > 0, "Sequence frequency must be non-zero and positive!"
        self.seq_frequency = seq_frequency
        if isinstance(seq_length, float) and seq_length > 0:  # a float is a duration in seconds
            self.seq_length = round(seq_length * seq_frequency)
            warnings.warn(f"Sequence length {seq_length} is a float: taken as seconds, i.e. {self.seq_length} timesteps.")
        elif isinstance(seq_length, int):
            self.seq_length = seq_length
        else:
            raise ValueError(f"seq_length must be a positive float (seconds) or an int (timesteps), but given: {seq_length}.")

    def get_sequences(self, timesteps_nb, input_frequency: int):
        raise NotImplementedError


class BasicLabeledSequencer_Abs(BasicSequencer_Abs):
    def get_sequences(self, labels: Sequence, input_frequency: int):
        raise NotImplementedError


def _regular(seq_length, seq_step, timesteps_nb, fps_step):
    """windows every ``seq_step`` INPUT frames, the last one ending on the last frame -> (windows, first start) or (None, None)"""
    stretch = fps_step * seq_length
    span = stretch - (fps_step - 1)
    if span > timesteps_nb:
        return None, None
    slack = timesteps_nb - span
    first = slack % seq_step
    windows = [list(range(s, s + stretch, fps_step)) for s in range(first, slack + 1, seq_step)]
    assert all(len(w) == seq_length for w in windows), "Sequences are not of the desired length!"
    assert len(windows) == int(slack // seq_step) + 1, "Number of sequences is incorrect!"
    assert windows[-1][-1] == timesteps_nb - 1, "The last sequence does not end on the last frame!"
    return windows, first


class RegularSequencer(BasicSequencer_Abs):
    def __init__(self, seq_frequency: int, seq_length: Union[int, float], step: int = 1):
        super().__init__(seq_frequency=seq_frequency, seq_length=seq_length)
        _check_step(step)
        self.seq_step = step  # counted in input frames

    def get_sequences(self, timesteps_nb: Union[int, Sequence, np.ndarray, torch.Tensor], input_frequency: int):
        fps_step = _fps_step(input_frequency, self.seq_frequency)
        return _regular(self.seq_length, self.seq_step, _count(timesteps_nb), fps_step)[0]


class RegularSequencerWithStart(BasicSequencer_Abs):
    """RegularSequencer plus one window at frame 0 (appended LAST) when the first regular window starts too far into the video"""

    def __init__(self, seq_frequency: int, seq_length: Union[int, float], step: int = 1):
        super().__init__(seq_frequency=seq_frequency, seq_length=seq_length)
        _check_step(step)
        self.seq_step = step  # counted in input frames

    def get_sequences(self, timesteps_nb: Union[int, Sequence, np.ndarray, torch.Tensor], input_frequency: int):
        fps_step = _fps_step(input_frequency, self.seq_frequency)
        windows, first = _regular(self.seq_length, self.seq_step, _count(timesteps_nb), fps_step)
        if windows is None:
            return None
        if first > min(0.3 * input_frequency, 5):
            extra = list(range(0, fps_step * self.seq_length, fps_step))
            assert len(extra) == self.seq_length
            windows.append(extra)
        return windows


class UnsafeOverlapSequencer(BasicLabeledSequencer_Abs):
    """Binary frame labels in, windows out: the regular windows (here ``step`` counts TARGET-frequency frames: it is multiplied by
    fps_step) plus every window that ends on an unsafe frame, plus ``surrounding_timesteps`` windows before / after each of those
    (None or 0: none; n: n on both sides; (a, b): a before, b after -- in input frames)."""

    def __init__(self, seq_frequency: int, seq_length: Union[int, float], step: int = 1,
                 surrounding_timesteps: Optional[Union[int, Tuple[int, int]]] = None):
        super().__init__(seq_frequency=seq_frequency, seq_length=seq_length)
        _check_step(step)
        self.seq_step = step  # counted in target-frequency frames
        if not surrounding_timesteps:
            self.surrounding_timesteps = (0, 0)
        elif isinstance(surrounding_timesteps, int) and surrounding_timesteps >= 0:
            self.surrounding_timesteps = (surrounding_timesteps, surrounding_timesteps)
        elif isinstance(surrounding_timesteps, Sequence) and len(surrounding_timesteps) == 2:
            assert all((isinstance(st, int) and st >= 0) for st in surrounding_timesteps), \
                f"surrounding_timesteps must be a Sequence of two non-negative ints! Given: {surrounding_timesteps}"
            self.surrounding_timesteps = surrounding_timesteps

    def get_sequences(self, is_unsafe: Sequence[bool], input_frequency: int):
        fps_step = _fps_step(input_frequency, self.seq_frequency)
        n = len(is_unsafe)
        stride = fps_step * self.seq_step
        span = fps_step * self.seq_length - (fps_step - 1)
        slack = n - span
        first_end = slack % stride + span - 1  # last frame of the first regular window: no window can end earlier
        ends = list(range(first_end, n, stride))
        assert len(ends) == int(slack // stride) + 1, "Number of sequences is incorrect!"
        before, after = self.surrounding_timesteps
        for i in range(first_end, n):
            if is_unsafe[i]:
                ends.extend(range(max(first_end, i - before), min(n - 1, i + after + 1)))
        windows = [list(range(e - span + 1, e + 1, fps_step)) for e in sorted(set(ends))]
        assert all(len(w) == self.seq_length for w in windows), "Sequences are not of the desired length!"
        assert windows[-1][-1] == n - 1, "The last sequence does not end on the last frame!"
        return windows
