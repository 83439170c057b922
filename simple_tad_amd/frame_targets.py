"""Host-side targets of the frame fine-tuning losses: the counterparts of ``dataset/data_utils.py:6-75`` of the reference.

``compute_time_vector`` turns a video's per-frame labels into the time to (negative) or since (positive) the nearest anomalous range,
in seconds -- the ``ttc`` that ``loss.TemporalExponentialLoss`` weighs its rows with -- and ``smooth_labels`` turns labels plus that
vector into the temporally smoothed [N, 2] targets of ``loss.DoubleBCELoss``.  Both run once per video when a dataset is built: plain
numpy / torch on the host, no kernel."""
from __future__ import annotations

import numpy as np
import torch

OUTSIDE = -100.   # the value of a frame outside both windows (data_utils.py:54)


def compute_time_vector(labels, fps, TT=2, TA=1):
    """data_utils.compute_time_vector (:6-56): float64 tensor [len(labels)].
    0 for an anomalous frame (label == 1) and for a video without any; ``-d / fps`` when the next anomalous frame is ``d <= int(TT *
    fps)`` frames ahead (this window has priority); else ``+d / fps`` when the last anomalous frame is ``d <= int(TA * fps)`` frames
    behind; else -100."""
    labels = np.array(labels)
    n = len(labels)
    time_vector = torch.zeros(n, dtype=torch.float64)
    anomalous = np.where(labels == 1)[0]
    if len(anomalous) == 0:
        return time_vector
    tt_frames, ta_frames = int(TT * fps), int(TA * fps)
    frames = np.arange(n)
    nxt = np.searchsorted(anomalous, frames, side="right")             # index of the first anomalous frame after each frame
    ahead = np.where(nxt < len(anomalous), anomalous[np.minimum(nxt, len(anomalous) - 1)] - frames, np.iinfo(np.int64).max)
    prv = np.searchsorted(anomalous, frames, side="left") - 1           # index of the last anomalous frame before each frame
    behind = np.where(prv >= 0, frames - anomalous[np.maximum(prv, 0)], np.iinfo(np.int64).max)
    out = np.full(n, OUTSIDE, dtype=np.float64)
    after = behind <= ta_frames
    out[after] = behind[after] / fps
    before = ahead <= tt_frames
    out[before] = -ahead[before] / fps
    out[labels == 1] = 0.0
    return torch.from_numpy(out)


def smooth_labels(labels, time_vector, before_limit=2, after_limit=1):
    """data_utils.smooth_labels (:59-75): f32 [N, 2] = (1 - a, a) with the anomaly target ``a`` = the hard label, except
    ``sigmoid(kb * (t + before_limit / 2))`` for ``-before_limit <= t < 0`` and ``sigmoid(ka * (after_limit / 2 - t))`` for
    ``0 < t <= after_limit``, ``kb = 12 / before_limit``, ``ka = 12 / after_limit``.  ``labels`` and ``time_vector`` are tensors [N]."""
    xb, xa = before_limit / 2, after_limit / 2
    kb, ka = 12 / before_limit, 12 / after_limit
    before_mask = (time_vector >= -before_limit) & (time_vector < 0)
    after_mask = (time_vector > 0) & (time_vector <= after_limit)
    target_anomaly = (labels == 1).float()
    target_anomaly[before_mask] = (1 / (1 + torch.exp(-kb * (time_vector[before_mask] + xb)))).float()
    target_anomaly[after_mask] = (1 / (1 + torch.exp(-ka * (-time_vector[after_mask] + xa)))).float()
    return torch.stack((1 - target_anomaly, target_anomaly), dim=-1)
