"""Time --image-weights (csrc/sampling.hip, sampling.py) on synthetic labels at two sizes - VEDAI-like (1,246 images, about 3
labels each, 8 classes) and COCO-like (118,287 images, 866,643 labels, 80 classes) - against the reference's host path as
restated in tests/sampling_ref.py (one np.bincount per image, the product, random.choices) on the same machine's host.
Prints one JSON line per size.  There is no pass/fail threshold on a time.

Per size:
  counts_us, image_weights_us, choices_us
                 device events around `--reps` back-to-back calls of one entry, divided by the calls; the median of 5 such
                 windows.  The caches are WARM: every call reads what the call before it read (all of it fits the L2 / the
                 Infinity Cache), as the epoch loop finds the count matrix after a validation pass only by luck.
                 choices_us covers the four launches of sodt_weighted_choices with k = n_img draws;
  *_bytes        bytes each entry moves by its access pattern (the binary search of the draws is counted as
                 ceil(log2 n) reads of 8 bytes per draw);
  construct_ms   ImageWeights(labels, nc): concatenation on the host, upload, counts, class weights and the one read, by the
                 wall clock, median of 5;
  epoch_ms       ImageWeights.choices(...) by the wall clock, from the k draws of `random` to the list of ints, median of 5;
  host_epoch_ms  the restated reference for the same epoch (labels_to_image_weights + random.choices), median of 5.

usage: python tools/mb_sampling.py [--reps 20]
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG = "small-object-detection-transformers_amd"
SIZES = (("vedai", 1246, 3738, 8), ("coco", 118287, 866643, 80))      # tag, images, labels, classes


def dataset(n_img, n_labels, nc, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.multinomial(n_labels, np.full(n_img, 1.0 / n_img))
    allc = np.zeros((n_labels, 5), dtype=np.float32)
    allc[:, 0] = rng.integers(0, nc, n_labels)
    allc[:, 1:] = rng.uniform(0.05, 0.95, (n_labels, 4))
    return np.split(allc, np.cumsum(lens)[:-1])


def device_us(fn, reps):
    """Median over 5 windows of (device time of `reps` calls) / reps, in microseconds."""
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / reps)
    return round(statistics.median(out), 2)


def wall_ms(fn):
    out = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3)


def one(tag, n_img, n_labels, nc, reps):
    import sampling_ref as SR
    S = importlib.import_module(PKG + ".sampling")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    labels = dataset(n_img, n_labels, nc)
    maps = np.random.default_rng(1).uniform(0.0, 1.0, nc)
    obj = S.ImageWeights(labels, nc, dev)                                               # (also loads the library, warms the allocator)
    mcw = obj.class_weights_host * nc
    res = dict(size=tag, n_img=n_img, labels=n_labels, nc=nc, reps=reps)
    # the three entries on their own
    lens = np.array([len(l) for l in labels])
    cls = torch.from_numpy(np.concatenate(labels)[:, 0].astype(np.int32)).to(dev)
    img = torch.from_numpy(np.repeat(np.arange(n_img, dtype=np.int32), lens)).to(dev)
    counts = torch.zeros(n_img, nc, dtype=torch.int32, device=dev)
    total = torch.zeros(nc, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    res["counts_us"] = device_us(lambda: ops.class_counts(cls, img, n_img, nc, counts, total, status), reps)
    res["counts_bytes"] = 8 * n_labels + 12 * n_labels                                  # two int32 reads, an int32 and an int64 atomic
    cw = torch.from_numpy(mcw * (1 - maps) ** 2 / nc).to(dev)
    iw = torch.empty(n_img, dtype=torch.float64, device=dev)
    res["image_weights_us"] = device_us(lambda: ops.image_weights(obj.class_counts, cw, iw), reps)
    res["image_weights_bytes"] = 4 * n_img * nc + 8 * nc * ((n_img + 255) // 256) + 8 * n_img
    k = n_img
    u = torch.rand(k, dtype=torch.float64, device=dev)
    wsb = ops.weighted_choices_workspace_bytes(n_img, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    cum = torch.empty(n_img, dtype=torch.float64, device=dev)
    out = torch.zeros(k + 1, dtype=torch.int32, device=dev)
    res["choices_us"] = device_us(lambda: ops.weighted_choices(iw, u, out[:k], cum, out[k:], ws), reps)
    res["choices_bytes"] = 8 * n_img * 4 + 2 * wsb + k * (8 + 4 + 8 * math.ceil(math.log2(max(n_img, 2))))
    # the Python layer and the host path, by the wall clock
    res["construct_ms"] = wall_ms(lambda: S.ImageWeights(labels, nc, dev))
    res["epoch_ms"] = wall_ms(lambda: obj.choices(mcw, maps))
    res["host_epoch_ms"] = wall_ms(lambda: SR.epoch(labels, nc, mcw, maps))
    random.seed(0)
    got = obj.choices(mcw, maps)
    random.seed(0)
    res["indices_equal_host"] = got == SR.epoch(labels, nc, mcw, maps)[2]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    for tag, n_img, n_labels, nc in SIZES:
        one(tag, n_img, n_labels, nc, args.reps)


if __name__ == "__main__":
    main()
