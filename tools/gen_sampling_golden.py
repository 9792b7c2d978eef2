"""Write tests/golden/sampling.pt: the reference's own `labels_to_class_weights` and `labels_to_image_weights`
(basics/utils/general.py:220-244) and the expressions of Train.py:275 and :339-341 with the stdlib's `random.choices`, run on
small synthetic label sets.  Runs only where the reference source tree is importable (the build machine); it reads
oracle.gen_golden.import_reference() for the module stubs, as tools/gen_autoanchor_golden.py does, and changes nothing
under oracle/.

`labels_to_image_weights` of the reference uses `np.int`, which this numpy no longer has, so the flag raises before it draws
anything.  The generator sets `np.int = int` around the reference call - the alias numpy itself removed - and takes it away
again; nothing else of the reference is touched.

The fixture holds data only.  Per case: `tag`, `seed` (given to random.seed before Train.py:341), `nc`, `k`, `labels` (all
labels (M, 5) float32 [class, x, y, w, h] in image order) with `lens` (n_img) labels per image, `maps` (nc) float64,
`class_weights` (what labels_to_class_weights returned), `model_class_weights` (Train.py:275: the former * nc), `cw`
(Train.py:339), `image_weights` (:340), `indices` (:341, int32) and `state`, random.getstate() after the call.

Cases: nc 1, 8, 80; n_img 1, 2, 65, 1025, 3077; images without labels (first and last among them); a class without labels;
maps that contain 0 and 1; k below and above n_img.

A seed is taken only if every x = u * total of the case lies at least 1e-9 * total away from every entry of the reference's
cumulative weights: two float64 summation orders of n non-negative terms differ by at most 2 (n - 1) 2^-53 relative, 7e-13
at n = 3077, so another order cannot move a draw across a boundary.  The smallest margin found is printed.

usage: python tools/gen_sampling_golden.py
"""
from __future__ import annotations

import importlib
import os
import random
import sys
from itertools import accumulate

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import sampling_ref as SR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampling.pt")
MARGIN = 1e-9
# tag, nc, n_img, k (None: n_img), most labels per image
CASES = (("nc1_n1", 1, 1, None, 3), ("nc8_n2_k5", 8, 2, 5, 4), ("nc8_n65", 8, 65, None, 5), ("nc80_n1025_k300", 80, 1025, 300, 6),
         ("nc8_n1025_k2000", 8, 1025, 2000, 4), ("nc80_n3077", 80, 3077, None, 4))


def dataset(rng, nc, n_img, most):
    """Labels with empty images (the first and the last among them where n_img > 2), one class never used (nc > 1)."""
    used = np.arange(nc) if nc == 1 else np.delete(np.arange(nc), nc // 2)
    if n_img <= 2 and nc > 2:
        used = used[:-1]                                # (the perfect class weighs nothing: keep the total positive)
    labels = []
    for i in range(n_img):
        m = int(rng.integers(0, most + 1))
        if n_img > 2 and i in (0, n_img - 1) or n_img == 2 and i == 1:
            m = 0
        elif n_img <= 2:
            m = max(m, 1)
        l = np.zeros((m, 5), dtype=np.float32)
        l[:, 0] = rng.choice(used, m)
        l[:, 1:] = rng.uniform(0.05, 0.95, (m, 4))
        labels.append(l)
    maps = rng.uniform(0.0, 1.0, nc)
    if nc > 2:
        maps[0], maps[nc - 1] = 0.0, 1.0                # an unlearnt and a perfect class
    return labels, maps


def run_reference(G, seed, labels, nc, maps, k):
    """Train.py:275 and :339-341, the reference's functions and the stdlib's random.choices."""
    class_weights = G.labels_to_class_weights(labels, nc)
    model_class_weights = class_weights * nc                                            # Train.py:275 (without .to(device))
    n = len(labels)
    random.seed(seed)
    cw = model_class_weights.cpu().numpy() * (1 - maps) ** 2 / nc
    np.int = int                                        # the alias general.py:241 needs; numpy removed it in 1.24
    try:
        iw = G.labels_to_image_weights(labels, nc=nc, class_weights=cw)
    finally:
        del np.int
    indices = random.choices(range(n), weights=iw, k=n if k is None else k)
    return class_weights, model_class_weights, cw, iw, indices, random.getstate()


def margin(seed, iw, k):
    """The smallest distance of a draw u * total from a cumulative weight, relative to the total."""
    cum = np.array(list(accumulate(iw)))
    random.seed(seed)
    x = np.array([random.random() for _ in range(k)]) * cum[-1]
    j = np.searchsorted(cum, x)
    near = np.minimum(np.abs(x - cum[np.clip(j, 0, len(cum) - 1)]), np.abs(x - cum[np.clip(j - 1, 0, len(cum) - 1)]))
    return float(near.min() / cum[-1])


def main():
    import_reference()
    G = importlib.import_module("reference.basics.utils.general")
    cases, smallest = [], float("inf")
    for ci, (tag, nc, n_img, k, most) in enumerate(CASES):
        labels, maps = dataset(np.random.default_rng(100 + ci), nc, n_img, most)
        seed = 1000 * (ci + 1)
        while True:
            cwt, mcw, cw, iw, indices, state = run_reference(G, seed, labels, nc, maps, k)
            mg = margin(seed, iw, len(indices))
            if mg >= MARGIN:
                break
            seed += 1
        # the restatement must be the reference, bit for bit, before anything is stored
        random.seed(seed)
        r_cw, r_iw, r_idx = SR.epoch(labels, nc, SR.labels_to_class_weights(labels, nc) * nc, maps, k)
        assert np.array_equal(r_cw, cw) and np.array_equal(r_iw, iw) and r_idx == indices and random.getstate() == state, tag
        smallest = min(smallest, mg)
        empty = sum(len(l) == 0 for l in labels)
        print(f"[sampling golden] {tag}: seed {seed}, {sum(len(l) for l in labels)} labels, {empty} empty images, "
              f"{len(indices)} draws, margin {mg:.2e} of the total")
        cases.append(dict(tag=tag, seed=seed, nc=nc, k=len(indices), labels=torch.from_numpy(np.concatenate(labels, 0)),
                          lens=torch.tensor([len(l) for l in labels]), maps=torch.from_numpy(maps), class_weights=cwt.clone(),
                          model_class_weights=mcw.clone(), cw=torch.from_numpy(cw), image_weights=torch.from_numpy(iw),
                          indices=torch.tensor(indices, dtype=torch.int32), state=state))
    torch.save(dict(cases=cases), OUT)
    print(f"[sampling golden] smallest margin {smallest:.2e} of the total (required {MARGIN:.0e}); "
          f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
