"""sodt_sgd_ema_step and sodt_adam_ema_step over the real model's flat buffers (22,007,851 parameters, bf16 mirror and EMA
attached): device-event time per launch and the algorithmic bytes per second (30 B / element for SGD, 38 B for Adam).  The
buffers of one launch (0.66 / 0.84 GB) do not fit the 256 MB Infinity Cache, so back-to-back launches stream from HBM.

usage: python tools/mb_optim.py [--size 512] [--iters 50]
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "small-object-detection-transformers_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_optim.py measures on the GPU; there is nothing to time without one")
    import bench
    O = importlib.import_module(PKG + ".optim")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    model = bench.build_model(a.size, dev, torch.bfloat16)
    ema = O.ModelEMA(model)
    g = torch.Generator().manual_seed(0)
    x, ir = (torch.rand(1, 3, a.size, a.size, generator=g).to(dev) for _ in range(2))
    model(x, ir, "RGB+IR")[0][0].float().square().mean().backward()      # real gradients, and the bf16 mirror exists
    eng = model._get_engine()
    n = eng.flat_param.numel()
    print(f"{sum(p.numel() for p in model.parameters())} parameters, flat buffer of {n} elements, mirror {list(eng.flat_cast)}", flush=True)
    opts = {"sodt_sgd_ema_step": (O.FusedSGD(O.set_weight_decay(model), model=model, lr=1e-4, ema=ema), 30),
            "sodt_adam_ema_step": (O.FusedAdam(O.set_weight_decay(model), model=model, lr=1e-5, betas=(0.937, 0.999), ema=ema), 38)}
    for name, (opt, nbytes) in opts.items():
        best = []
        for _ in range(3):                                # three windows: their spread is printed
            with ops.Recorder() as rec:
                opt.step()                                # (warm-up; the gradients stay: no zero_grad)
            assert [c[2] for c in rec.calls] == [name]
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                opt._launch_step(eng, ema.flat, eng.flat_cast[torch.bfloat16], 1.0, 0.9999)
            e.record()
            torch.cuda.synchronize()
            best.append(s.elapsed_time(e) / a.iters)
        t = sorted(best)[1]
        print(f"{name}: {t * 1e3:.1f} us per launch (three windows of {a.iters}: {', '.join(f'{b * 1e3:.1f}' for b in best)} us), "
              f"{nbytes} B x {n} = {nbytes * n / 1e6:.0f} MB -> {nbytes * n / t / 1e9:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
