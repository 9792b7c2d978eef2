"""Restatement of the reference's --image-weights arithmetic for the tests and tools/mb_sampling.py: `labels_to_class_weights`
and `labels_to_image_weights` (basics/utils/general.py:220-244, with `int` where the reference writes `np.int`), the stdlib's
`random.choices` (accumulate, total, bisect) and the epoch block of Train.py:339-341 - numpy and the standard library only.
`device_cum` recomputes the cumulative weights in the association order include/sodt_hip.h documents for
sodt_weighted_choices, with element-wise float64 additions on the host."""
from __future__ import annotations

import random
from bisect import bisect
from itertools import accumulate
from math import isfinite

import numpy as np
import torch

U = 2.0 ** -53                                          # unit roundoff of float64


def labels_to_class_weights(labels, nc=80):
    """general.py:220-236 -> float64 numpy (nc,), or None when no labels are loaded."""
    if labels[0] is None:
        return None
    labels = np.concatenate(labels, 0)
    classes = labels[:, 0].astype(np.int32)
    weights = np.bincount(classes, minlength=nc)
    weights[weights == 0] = 1
    weights = 1 / weights
    weights /= weights.sum()
    return weights


def class_counts(labels, nc):
    """general.py:241: one np.bincount per image -> (n_img, nc) int64."""
    return np.array([np.bincount(x[:, 0].astype(int), minlength=nc) for x in labels])


def labels_to_image_weights(labels, nc=80, class_weights=np.ones(80)):
    """general.py:239-244."""
    return (class_weights.reshape(1, nc) * class_counts(labels, nc)).sum(1)


def choices(weights, k, rand=random.random):
    """random.choices(range(n), weights=weights, k=k) of CPython's Lib/random.py -> (indices, cum_weights)."""
    cum = list(accumulate(weights))
    n = len(cum)
    total = cum[-1] + 0.0
    if total <= 0.0:
        raise ValueError("Total of weights must be greater than zero")
    if not isfinite(total):
        raise ValueError("Total of weights must be finite")
    hi = n - 1
    return [bisect(cum, rand() * total, 0, hi) for _ in range(k)], cum


def epoch(labels, nc, model_class_weights, maps, k=None):
    """Train.py:339-341 -> (cw, iw, indices); model_class_weights is what Train.py:275 attached (class weights * nc)."""
    cw = np.asarray(model_class_weights) * (1 - maps) ** 2 / nc
    iw = labels_to_image_weights(labels, nc=nc, class_weights=cw)
    idx, _ = choices(iw, len(labels) if k is None else k)
    return cw, iw, idx


def _block_scan(x):
    """x (..., 256, per) float64 -> inclusive prefixes in the order of the header's `block scan`, and the block sums."""
    s = x.clone()
    for j in range(1, x.shape[-1]):                      # serial inside a thread
        s[..., j] = s[..., j - 1] + x[..., j]
    v = s[..., -1].reshape(*x.shape[:-2], 4, 64).clone()  # thread sums by wave and lane
    for o in (1, 2, 4, 8, 16, 32):                       # Hillis-Steele inside a wave
        nxt = v.clone()
        nxt[..., o:] = v[..., o:] + v[..., :-o]
        v = nxt
    wsum = v[..., 63]
    zero = torch.zeros_like(wsum[..., 0])
    p1 = wsum[..., 0]
    p2 = p1 + wsum[..., 1]
    p3 = p2 + wsum[..., 2]
    wave_prefix = torch.stack((zero, p1, p2, p3), -1)
    lane_prefix = torch.cat((torch.zeros_like(v[..., :1]), v[..., :-1]), -1)
    prefix = (wave_prefix.unsqueeze(-1) + lane_prefix).reshape(*x.shape[:-1])
    return prefix.unsqueeze(-1) + s, p3 + wsum[..., 3]


def device_cum(iw, W):
    """The inclusive prefix sums of iw (n) float64 in sodt_weighted_choices' documented order; W = SODT_CHOICES_BLOCK."""
    iw = torch.as_tensor(iw, dtype=torch.float64).cpu()
    n = iw.numel()
    nb = (n + W - 1) // W
    a = torch.zeros(nb * W, dtype=torch.float64)
    a[:n] = iw
    local, totals = _block_scan(a.reshape(nb, 256, W // 256))                           # phase 1
    per = (nb + 255) // 256
    t = torch.zeros(256 * per, dtype=torch.float64)
    t[:nb] = totals
    inclusive, _ = _block_scan(t.reshape(256, per))                                      # phase 2
    offset = torch.cat((torch.zeros(1, dtype=torch.float64), inclusive.reshape(-1)[:nb - 1]))
    return (offset.reshape(nb, 1) + local.reshape(nb, W)).reshape(-1)[:n]               # phase 3
