"""Time weighted boxes fusion (csrc/wbf.hip) on synthetic predictions: B = 8 images of N = 49,152 rows (the stride-4
grid of a 512 x 512 input, 3 anchors), nc = 3, with about `--candidates` rows per image above conf_thres.  Prints one
JSON line.

Device times are medians of three windows of events on the current stream.  Phases:
  candidates  sodt_wbf_candidates alone;
  sort        sodt_wbf_fuse with skip_box_thr = +inf: every row is dropped, so the five radix sorts, the key kernels and
              the output kernels run over all B * N slots and the clustering kernel finds no segment;
  fuse        sodt_wbf_fuse as it is, minus `sort`: the clustering kernel.  Its time per candidate step divides by the
              longest (image, label) segment, the sequential chain that bounds it.
Both scan shapes (64 and 256 lanes per segment) are timed.

--reference (build machine only: needs the reference source tree) times the reference's own `weighted_boxes` on image 0
of the same inputs on the CPU by the wall clock; --host times tests/wbf_ref.py's numpy restatement the same way.

usage: python tools/mb_wbf.py [--candidates 2000] [--batch 8] [--reps 3]
       python tools/mb_wbf.py --candidates 2000 --reference
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG = "small-object-detection-transformers_amd"
N, NC, S = 49152, 3, 512


def synthetic(B, n_cand, seed=0, objects=300):
    """(B, N, 5+nc) f32 on the CPU: `objects` objects per image, each row a jittered copy of one of them; the first
    n_cand rows of a random order carry an objectness above the threshold, the others far below."""
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand(B, objects, 2, generator=g) * (S - 40) + 20
    wh = torch.rand(B, objects, 2, generator=g) * 24 + 8
    lab = torch.randint(0, NC, (B, objects), generator=g)
    own = torch.randint(0, objects, (B, N), generator=g)
    z = torch.zeros(B, N, 5 + NC)
    z[..., 0:2] = torch.gather(ctr, 1, own[..., None].expand(-1, -1, 2)) + torch.randn(B, N, 2, generator=g) * 1.5
    z[..., 2:4] = torch.gather(wh, 1, own[..., None].expand(-1, -1, 2)) * (1 + torch.randn(B, N, 2, generator=g) * 0.08)
    z[..., 5:] = torch.rand(B, N, NC, generator=g) * 0.3
    z[..., 5:].scatter_(2, torch.gather(lab, 1, own)[..., None], torch.rand(B, N, 1, generator=g) * 0.6 + 0.4)
    rank = torch.rand(B, N, generator=g).argsort(1).argsort(1)
    z[..., 4] = torch.where(rank < n_cand, torch.rand(B, N, generator=g) * 0.2 + 0.8, torch.full((B, N), 0.01))
    return z


def event_ms(fn, reps, inner):
    fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        for _ in range(inner):
            fn()
        e.record()
    torch.cuda.synchronize()
    t = [s.elapsed_time(e) / inner for s, e in ev]
    return float(np.median(t)), [round(v, 4) for v in t]


def host(a):
    z = synthetic(a.batch, a.candidates)[:1]
    if a.reference:
        from oracle.gen_golden import import_reference
        import_reference()
        G = importlib.import_module("reference.basics.utils.general")
        fn, name = (lambda: G.weighted_boxes(z.clone(), S, conf_thres=0.25, iou_thres=0.45)), "reference"
    else:
        import wbf_ref as WR
        fn, name = (lambda: WR.weighted_boxes(z.numpy(), S, 0.25, 0.45)), "restatement"
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    rows = int(((z[0, :, 4] > 0.25) & ((z[0, :, 5:] * z[0, :, 4:5]).max(-1).values > 0.25)).sum())
    print(json.dumps({"mode": name, "images": 1, "candidates": rows, "clusters": int(len(out[0][0]) if a.host else len(out[0])),
                      "cpu_s_per_image": round(float(np.median(t)), 3), "cpu_s_all": [round(v, 3) for v in t]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", action="store_true", help="time the reference on the CPU (build machine only)")
    ap.add_argument("--host", action="store_true", help="time tests/wbf_ref.py on the CPU")
    a = ap.parse_args()
    if a.reference or a.host:
        return host(a)
    ops = importlib.import_module(PKG + ".ops")
    wbf = importlib.import_module(PKG + ".wbf")
    dev = torch.device("cuda:0")
    B = a.batch
    z = synthetic(B, a.candidates).to(dev)
    boxes = torch.empty(B, N, 4, device=dev)
    scores = torch.empty(B, N, device=dev)
    labels = torch.empty(B, N, dtype=torch.int32, device=dev)
    src = torch.empty(B, N, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.wbf_fuse_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
    ob, os_, ol = torch.empty(B, N, 4, device=dev), torch.empty(B, N, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev)
    oc = torch.empty(B, dtype=torch.int32, device=dev)

    def cand():
        ops.wbf_candidates(z, 0.25, S, boxes, scores, labels, src, counts)

    def fuse(lanes, skip=0.0):
        ops.wbf_fuse(boxes, scores, labels, None, src, counts, [1.0], 0.45, skip, 0, False, ws, ob, os_, ol, oc, None, lanes)

    cand()
    n = counts.tolist()
    seg = max(int((labels[b, :n[b]] == c).sum()) for b in range(B) for c in range(NC))
    res = {"mode": "device", "batch": B, "rows": N, "nc": NC, "candidates_per_image": n, "longest_segment": seg,
           "workspace_mib": round(ws.numel() / 2**20, 1)}
    res["candidates_ms"], res["candidates_ms_all"] = event_ms(cand, a.reps, 10)
    res["sort_ms"], res["sort_ms_all"] = event_ms(lambda: fuse(64, float("inf")), a.reps, 5)
    for lanes in (64, 256):
        t, al = event_ms(lambda: fuse(lanes), a.reps, 2)
        res[f"fuse_total_ms_{lanes}"], res[f"fuse_total_ms_{lanes}_all"] = round(t, 4), al
        res[f"cluster_ms_{lanes}"] = round(t - res["sort_ms"], 4)
        res[f"us_per_step_{lanes}"] = round(1e3 * (t - res["sort_ms"]) / seg, 3)
        res[f"clusters_{lanes}"] = oc.tolist()
    t0 = time.perf_counter()
    out = wbf.weighted_boxes(z, S, 0.25, 0.45)
    torch.cuda.synchronize()
    res["weighted_boxes_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    res["candidates_ms"], res["sort_ms"] = round(res["candidates_ms"], 4), round(res["sort_ms"], 4)
    assert [len(o) for o in out] == res["clusters_64"] == res["clusters_256"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
