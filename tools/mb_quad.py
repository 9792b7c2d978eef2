"""sodt_preprocess_u8_quad (csrc/quad.hip), the one launch of `--quad` + pre-processing (datasets.py:637-664 + Train.py:364-374),
against two other ways to the same f32 inputs from the loader's plain 4n-sample uint8 batch on the device:

  (a) one launch:     preprocess_batch(imgs, irs, f, quad=modes)                       sodt_preprocess_u8_quad
  (b) two launches:   preprocess_batch(*quad_batch(imgs, irs, modes), f)               sodt_quad_u8 + sodt_preprocess_u8
  (c) ATen + launch:  collate_fn4's own torch calls on the device tensors (tests/quad_ref.py: float / interpolate / cast per
                      zoom group, cat per tile group, stack), then preprocess_batch     ATen kernels + sodt_preprocess_u8

B = 16 source samples, 3 + 3 channels of 1024^2 uint8, down_factor 2, under an all-tile, an all-zoom and a mixed mask.  Every
path is warmed first; then the three alternate in one process, three windows of --iters calls each under device events.
Printed per mask: the median and the three windows of each path, the bytes (a) needs from shapes (uint8 read + f32 written; a
zoom group reads one of its four images) and its bytes per second, and the spread of the windows.  The results of the three
paths are compared once per mask: (a) and (b) must agree bit for bit, the distance to (c) is printed.

usage: python tools/mb_quad.py [--iters 50] [--batch 16] [--load 1024] [--down-factor 2]
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "small-object-detection-transformers_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16, help="source samples (4 per quad image)")
    ap.add_argument("--load", type=int, default=1024, help="side of the uint8 images the loader delivers")
    ap.add_argument("--down-factor", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_quad.py measures on the GPU; there is nothing to time without one")
    from quad_ref import quad_ref_device
    P = importlib.import_module(PKG + ".preprocess")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, L, f = a.batch, a.load, a.down_factor
    n = B // 4
    rgb = torch.randint(0, 256, (B, 3, L, L), generator=g, dtype=torch.uint8).to(dev)
    ir = torch.randint(0, 256, (B, 3, L, L), generator=g, dtype=torch.uint8).to(dev)
    masks = [("all tile", (False,) * n), ("all zoom", (True,) * n), ("mixed", tuple(i % 2 == 0 for i in range(n)))]

    def one(modes):
        return P.preprocess_batch(rgb, ir, f, quad=modes)

    def two(modes):
        return P.preprocess_batch(*P.quad_batch(rgb, ir, modes), f)

    def aten(modes):
        return P.preprocess_batch(*quad_ref_device(rgb, ir, modes), f)

    def window(fn, modes):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn(modes)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    for name, modes in masks:                           # warm every path, pin the launches, compare the results
        with ops.Recorder() as rec:
            o = one(modes)
        assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8_quad"], [c[2] for c in rec.calls]
        with ops.Recorder() as rec:
            t = two(modes)
        assert [c[2] for c in rec.calls] == ["sodt_quad_u8", "sodt_preprocess_u8"], [c[2] for c in rec.calls]
        r = aten(modes)
        same = torch.equal(o[0], t[0]) and torch.equal(o[1], t[1])
        d = max(float((o[0] - r[0]).abs().max()), float((o[1] - r[1]).abs().max()))
        print(f"{name}: one launch == two launches bit for bit: {same}; max |one launch - ATen path| = {d:.2e}", flush=True)
        assert same
        del o, t, r
        for _ in range(5):
            one(modes)
            two(modes)
            aten(modes)
    torch.cuda.synchronize()
    So = 2 * L // f
    print(f"B={B} source samples -> {n} quad images, 3+3 channels of {L}^2 uint8, down_factor {f} -> {So}^2 f32: "
          f"us per call, median of three windows of {a.iters} (the windows)")
    for name, modes in masks:
        ta, tb, tc = [], [], []
        for _ in range(3):                              # alternate the paths: drift of the machine hits all of them
            ta.append(window(one, modes))
            tb.append(window(two, modes))
            tc.append(window(aten, modes))
        read = sum(6 * L * L * (1 if m else 4) for m in modes)
        wrote = n * 6 * So * So * 4
        ma, mb, mc = sorted(ta)[1], sorted(tb)[1], sorted(tc)[1]
        w = lambda ts: ", ".join(f"{v * 1e3:.1f}" for v in ts)
        sp = lambda ts: (max(ts) - min(ts)) * 1e3
        print(f"{name}: (a) one launch {ma * 1e3:.1f} ({w(ta)}) reads {read / 1e6:.0f} MB writes {wrote / 1e6:.0f} MB -> "
              f"{(read + wrote) / ma / 1e9:.2f} TB/s | (b) two launches {mb * 1e3:.1f} ({w(tb)}) | (c) ATen + launch {mc * 1e3:.1f} ({w(tc)}) | "
              f"(b)/(a) {mb / ma:.2f}x, (c)/(a) {mc / ma:.2f}x, spread (a) {sp(ta):.1f} (b) {sp(tb):.1f} (c) {sp(tc):.1f} us", flush=True)


if __name__ == "__main__":
    main()
