"""sodt_sgd_ema_step and sodt_adam_ema_step over the real model's flat buffers (22,007,851 parameters, bf16 mirror and EMA
attached): device-event time per launch and the algorithmic bytes per second (30 B / element for SGD, 38 B for Adam).  The
buffers of one launch (0.66 / 0.84 GB) do not fit the 256 MB Infinity Cache, so back-to-back launches stream from HBM.

Where the library has the control path, the same for sodt_grad_stats (4 B / element read, plus the group map) and the two
_ctl steps (reading a record sodt_grad_stats filled from the same finite gradients), and with --scaler the host wall time of
`scaler.step(opt); scaler.update()` on pre-filled gradients: the time the host needs to ISSUE an iteration (what limits a
host that replays ahead of the GPU) and the time per iteration once the device has finished.  --scaler also runs on a tree
without the control path, where GradScaler.step unscales the gradient views itself and reads found_inf on the host.

usage: python tools/mb_optim.py [--size 512] [--iters 50] [--scaler [--scaler-iters 100]]
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
    ap.add_argument("--scaler", action="store_true", help="also time scaler.step(opt); scaler.update() on the host")
    ap.add_argument("--scaler-iters", type=int, default=100)
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
    cast = eng.flat_cast[torch.bfloat16]

    def timed(name, nbytes, launch, warm):
        best = []
        for _ in range(3):                                # three windows: their spread is printed
            warm()                                        # (warm-up; the gradients stay: no zero_grad)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                launch()
            e.record()
            torch.cuda.synchronize()
            best.append(s.elapsed_time(e) / a.iters)
        t = sorted(best)[1]
        print(f"{name}: {t * 1e3:.1f} us per launch (three windows of {a.iters}: {', '.join(f'{b * 1e3:.1f}' for b in best)} us), "
              f"{nbytes} B x {n} = {nbytes * n / 1e6:.0f} MB -> {nbytes * n / t / 1e9:.2f} TB/s", flush=True)

    def recorded_step(opt, names):
        def warm():
            with ops.Recorder() as rec:
                opt.step()
            assert [c[2] for c in rec.calls] == names
        return warm
    for name, (opt, nbytes) in opts.items():
        timed(name, nbytes, lambda: opt._launch_step(eng, ema.flat, cast, 1.0, 0.9999), recorded_step(opt, [name]))
    if hasattr(ops, "grad_stats"):                        # the control path: stats, then the step that reads its record
        for name, (opt, nbytes) in opts.items():
            opt.skip_nonfinite = True
            warm = recorded_step(opt, ["sodt_grad_stats", name + "_ctl"])
            warm()
            ctl = opt._ctl
            if name.startswith("sodt_sgd"):
                timed("sodt_grad_stats", 4, lambda: ops.grad_stats(eng.flat_grad, opt._groups, ctl, None, None, 1.0, 10.0, True), warm)
            timed(name + "_ctl", nbytes, lambda: opt._launch_step_ctl(eng, ema.flat, cast, ctl, 0.9999), warm)
            timed("sodt_grad_stats + " + name + "_ctl", nbytes + 4, opt.step, warm)
            opt.skip_nonfinite = False
    if a.scaler:
        import time
        for name, (opt, _) in opts.items():
            scaler = torch.amp.GradScaler("cuda", init_scale=1.0)      # scale 1: unscaling in place leaves the gradients as they are
            scaler.scale(torch.zeros((), device=dev))
            fused = bool(getattr(opt, "_step_supports_amp_scaling", False))
            for _ in range(5):
                scaler.step(opt)
                scaler.update()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.scaler_iters):
                scaler.step(opt)
                scaler.update()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print(f"scaler.step + scaler.update with {type(opt).__name__} ({'device-side control path' if fused else 'GradScaler unscales and reads found_inf on the host'}): "
                  f"host issues an iteration in {(t1 - t0) / a.scaler_iters * 1e6:.0f} us, {(t2 - t0) / a.scaler_iters * 1e6:.0f} us per iteration "
                  f"with the device drained ({a.scaler_iters} iterations)", flush=True)


if __name__ == "__main__":
    main()
