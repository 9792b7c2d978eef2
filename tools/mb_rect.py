"""The bf16 training step (bench.py's model and step: forward, ComputeLoss, hand-written backward, fused SGD + EMA) on a
rectangular batch against the square one, on ONE model built at 1024.  Default sizes: 8 x 1024 x 1024 (the bench shape), 8 x 768 x
1280 (0.94 of its pixels; stage 3 is 48 x 80 tokens and pads to 64 x 96 for its 32-token window, as 8 x 768 x 768 does) and 8 x 512 x
2048 (the same pixels as the square; stage 3 is 32 x 128 tokens, one window high: nothing pads).  Every size is warmed (the first
step records its plan), then the sizes alternate, three windows of --iters steps each under device events.  Printed per size: ms
per step (median and the three windows), ns per pixel, the run-to-run spread, and the ratio of its per-pixel rate to the square's.

--names SIZE prints the launch names of that size's recorded lists with their counts, for reading beside a kernel trace of
`python tools/mb_rect.py --sizes SIZE --iters N`.

usage: python tools/mb_rect.py [--iters 10] [--batch 8] [--sizes 1024x1024 768x1280 512x2048] [--names 768x1280]
"""
import argparse
import collections
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "small-object-detection-transformers_amd"


def _hw(s):
    h, _, w = s.partition("x")
    return int(h), int(w or h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--built", type=int, default=1024, help="img_size the model is built with")
    ap.add_argument("--sizes", type=_hw, nargs="+", default=[(1024, 1024), (768, 1280), (512, 2048)], help="HxW; the first is the yardstick")
    ap.add_argument("--names", type=_hw, default=None, help="print the recorded launch names of this size")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_rect.py measures on the GPU; there is nothing to time without one")
    import bench
    O = importlib.import_module(PKG + ".optim")
    LS = importlib.import_module(PKG + ".loss")
    dev = torch.device("cuda:0")
    B = a.batch
    model = bench.build_model(a.built, dev, torch.bfloat16)
    for hw in a.sizes:
        if not model.runs_at(hw):
            raise SystemExit(f"the model built at {a.built} does not run {hw[0]} x {hw[1]} (Model.runs_at)")
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    ema = O.ModelEMA(model)
    opt = O.FusedSGD(O.set_weight_decay(model), model=model, lr=0.01, momentum=0.937, nesterov=True, ema=ema)
    compute_loss = LS.ComputeLoss(model)
    targets = LS.synthetic_targets(B, 32, 8, seed=0).to(dev)
    g = torch.Generator().manual_seed(2)
    data = {hw: (torch.rand(B, 3, *hw, generator=g).to(dev), torch.rand(B, 3, *hw, generator=g).to(dev)) for hw in a.sizes}

    def step(hw):
        x, xi = data[hw]
        pred, _ = model(x, xi, "RGB+IR")
        loss = compute_loss(pred, targets)[0]
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        ema.update(model)

    def window(hw):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            step(hw)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    for hw in a.sizes:
        for _ in range(3):
            step(hw)
    torch.cuda.synchronize()
    eng = model._get_engine()
    if a.names is not None:
        key = next(k for k in eng.plans if k[1] == (a.names[0] if a.names[0] == a.names[1] else a.names) and k[3])
        plan = eng.plans[key]
        for part in ("fwd_main", "bwd_main"):
            cnt = collections.Counter(c[2] for c in getattr(plan, part))
            print(f"{a.names[0]}x{a.names[1]} {part}: " + ", ".join(f"{n} x{k}" for n, k in sorted(cnt.items())), flush=True)
    times = {hw: [] for hw in a.sizes}
    for _ in range(3):                                  # alternate the sizes: drift of the machine hits all of them
        for hw in a.sizes:
            times[hw].append(window(hw))
    print(f"B={B}, bf16 training step, model built at {a.built}: ms per step, median of three windows of {a.iters} (the windows)")
    base = None
    for hw in a.sizes:
        t = times[hw]
        med = sorted(t)[1]
        px = B * hw[0] * hw[1]
        rate = med * 1e6 / px
        base = rate if base is None else base
        print(f"{hw[0]}x{hw[1]}: {med:.2f} ms ({', '.join(f'{v:.2f}' for v in t)}), {rate:.3f} ns/pixel, spread {max(t) - min(t):.2f} ms "
              f"({(max(t) - min(t)) / med * 100:.1f} %), {B * 1e3 / med:.1f} img/s, per-pixel rate {rate / base:.3f}x the first size's", flush=True)


if __name__ == "__main__":
    main()
