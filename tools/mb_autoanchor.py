"""Time autoanchor (csrc/autoanchor.hip, autoanchor.py): `kmean_anchors(gen=1000, n=9)` end to end on synthetic labels at
two sizes, about 3.7k labels (VEDAI-sized) and about 860k (COCO-sized), against the numpy restatement of
tests/autoanchor_ref.py on the same machine's host.  Prints one JSON line per size.

Per size, in a fresh process under its own time limit (`--all` starts them; `--labels N` is one of them):
  end_to_end_s   wall clock of the second kmean_anchors call (the first pays for the library load and the allocator),
                 host draws, uploads and reads included;
  stats_ms, evolve_ms, kmeans_ms
                 device events around each of the three entries: one sodt_anchor_stats over all labels, the `gen`
                 generations of sodt_anchor_evolve in one call, and the restarts of sodt_kmeans_lloyd up to the last done
                 flag (that one includes the host reads between chunks);
  launches       kernels per call: 1 for the stats, `gen` for the evolution, chunks x 8 for k-means;
  host_*         the restatement by the wall clock.  At the large size it runs `--host-gen` generations and
                 `--host-restarts` restarts, and host_s_scaled extends that linearly to `gen` and 30.

usage: python tools/mb_autoanchor.py --all
       python tools/mb_autoanchor.py --labels 3700 [--gen 1000] [--host-gen 1000] [--host-restarts 30]
"""
from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG = "small-object-detection-transformers_amd"
SIZES = ((3700, 1000, 30, 300), (860000, 20, 2, 900))          # labels, host generations, host restarts, time limit (s)


def dataset(n_labels, seed=0):
    rng = np.random.default_rng(seed)
    n_img = max(1, n_labels // 8)
    shapes = np.stack([rng.choice([480, 512, 640], n_img), rng.choice([480, 512, 640], n_img)], 1).astype(np.float64)
    per = np.full(n_img, n_labels // n_img)
    per[:n_labels - per.sum()] += 1
    labels = []
    for m in per:
        size = np.exp(rng.uniform(np.log(0.006), np.log(0.6), m))
        asp = np.exp(rng.uniform(-np.log(4.0), np.log(4.0), m))
        l = np.zeros((m, 5))
        l[:, 3], l[:, 4] = np.minimum(size * np.sqrt(asp), 0.95), np.minimum(size / np.sqrt(asp), 0.95)
        labels.append(l)
    return types.SimpleNamespace(shapes=shapes, labels=labels)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def one(args):
    import autoanchor_ref as AR
    AA = importlib.import_module(PKG + ".autoanchor")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    ds = dataset(args.labels)
    n, gen, thr = 9, args.gen, 4.0
    res = dict(labels=args.labels, n=n, gen=gen)
    for rep in range(2):
        np.random.seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            k = AA.kmean_anchors(ds, n=n, img_size=640, thr=thr, gen=gen, verbose=False)
        torch.cuda.synchronize()
        res["end_to_end_s"] = round(time.perf_counter() - t0, 4)
    # the three entries on their own
    wh0 = AR.label_wh(ds.shapes, ds.labels, 640)
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    np.random.seed(1)
    idx = AR.initial_rows(len(wh), n)
    v = AR.draw_mutations(gen, (n, 2))
    wh_d = torch.from_numpy(wh).to(dev).float()
    obs = torch.from_numpy(wh / s).to(dev)
    k_d = torch.from_numpy(k).to(dev)
    res["stats_ms"] = round(events(lambda: AA._stats(wh_d, k_d.float().view(1, n, 2), thr))[0], 4)
    res["stats_ms"] = round(events(lambda: AA._stats(wh_d, k_d.float().view(1, n, 2), thr))[0], 4)
    iters = [0]
    real = ops.kmeans_lloyd

    def counted(*a):
        iters[0] += a[6]
        return real(*a)
    ops.kmeans_lloyd = counted
    try:
        ms, (_, _, curs, _) = events(lambda: AA._kmeans_device(obs, torch.from_numpy(idx).to(dev)))
    finally:
        ops.kmeans_lloyd = real
    res.update(kmeans_ms=round(ms, 3), kmeans_launches=iters[0], kmeans_winner=int(np.argmin(curs)))
    f = AA._stats(wh_d, k_d.float().view(1, n, 2), thr)[0, 1:2] / AA._count(len(wh), dev)
    ws = torch.empty(ops.anchor_evolve_workspace_bytes(len(wh)), dtype=torch.uint8, device=dev)
    acc = torch.zeros(gen, dtype=torch.int32, device=dev)
    v_d = torch.from_numpy(v).to(dev)
    ms, _ = events(lambda: ops.anchor_evolve(wh_d, 1.0 / thr, k_d.clone(), f.clone(), v_d, acc, ws))
    res.update(evolve_ms=round(ms, 3), evolve_launches=gen, evolve_us_per_generation=round(1e3 * ms / max(gen, 1), 2))
    # the restatement on the host
    hg, hr = min(args.host_gen, gen), args.host_restarts
    np.random.seed(1)
    t0 = time.perf_counter()
    book, _, info = AR.kmeans(wh / s, n, restarts=hr)
    t1 = time.perf_counter()
    if len(book) == n:
        AR.evolve(wh, (book * s)[np.argsort((book * s).prod(1))], 1.0 / thr, v[:hg])
    t2 = time.perf_counter()
    res.update(host_kmeans_s=round(t1 - t0, 3), host_restarts=hr, host_evolve_s=round(t2 - t1, 3), host_gen=hg,
               host_s_scaled=round((t1 - t0) * 30 / hr + (t2 - t1) * gen / max(hg, 1), 2))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--labels", type=int, default=3700)
    ap.add_argument("--gen", type=int, default=1000)
    ap.add_argument("--host-gen", type=int, default=1000)
    ap.add_argument("--host-restarts", type=int, default=30)
    args = ap.parse_args()
    if not args.all:
        return one(args)
    for labels, hg, hr, limit in SIZES:                       # a fresh process each, under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--labels", str(labels), "--gen", str(args.gen), "--host-gen", str(hg),
               "--host-restarts", str(hr)]
        r = subprocess.run(cmd, timeout=limit)
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
