"""sodt_sgd_ema_step and sodt_adam_ema_step over the real model's flat buffers (22,007,851 parameters, bf16 mirror and EMA
attached): device-event time per launch and the algorithmic bytes per second (30 B / element for SGD, 38 B for Adam).  The
buffers of one launch (0.66 / 0.84 GB) do not fit the 256 MB Infinity Cache, so back-to-back launches stream from HBM.

Where the library has the control path, the same for sodt_grad_stats (4 B / element read, plus the group map) and the two
_ctl steps (reading a record sodt_grad_stats filled from the same finite gradients), and with --scaler the host wall time of
`scaler.step(opt); scaler.update()` on pre-filled gradients: the time the host needs to ISSUE an iteration (what limits a
host that replays ahead of the GPU) and the time per iteration once the device has finished.  --scaler also runs on a tree
without the control path, where GradScaler.step unscales the gradient views itself and reads found_inf on the host.

--sam: the three kernels of csrc/sam.hip on the same buffers, non-adaptive and adaptive (bytes per element: norm 4 / 8 read,
perturb 8 read + 8 + 2 written, restore 4 + 4; the group map is on top), and first_step + second_step as optim.FusedSAM issues
them against the reference's per-tensor loop (tests/sam_ref.PerTensorSAM: a norm, a clone and an add_ per tensor, a copy back
per tensor) around the same FusedSGD: device time per pair and the time the host needs to issue one.

usage: python tools/mb_optim.py [--size 512] [--iters 50] [--scaler [--scaler-iters 100]] [--sam]
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
    ap.add_argument("--sam", action="store_true", help="also time the SAM kernels and FusedSAM's step pair against the per-tensor form")
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
    if a.sam:
        sam_section(a, O, ops, model, eng, ema, cast, n, timed)
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


def sam_section(a, O, ops, model, eng, ema, cast, n, timed):
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sam_ref as SR
    nothing = lambda: None
    for adaptive in (False, True):
        sam = O.FusedSAM(O.set_weight_decay(model), O.FusedSGD, model, rho=0.05, adaptive=adaptive, lr=1e-4, ema=ema)
        base = sam.base_optimizer
        sam.first_step()                                  # binds the engine, makes the record and old_p
        sam.second_step()
        groups, rec, old = base._groups, sam._rec, sam._old
        rho, flags = [0.05] * len(sam.param_groups), [adaptive] * len(sam.param_groups)
        tag = "adaptive" if adaptive else "non-adaptive"
        timed(f"sodt_sam_norm ({tag})", 8 if adaptive else 4,
              lambda: ops.sam_norm(eng.flat_param if adaptive else None, eng.flat_grad, groups, flags, rec), nothing)
        keep = eng.flat_param.clone()                     # (back-to-back perturbations walk p away; it is put back afterwards)
        timed(f"sodt_sam_perturb ({tag})", 18,
              lambda: ops.sam_perturb(eng.flat_param, eng.flat_grad, old, cast, groups, rho, flags, rec), nothing)
        eng.flat_param.copy_(keep)
        if not adaptive:
            timed("sodt_sam_restore", 8, lambda: ops.sam_restore(eng.flat_param, old, groups), nothing)

    def pair(name, first, second):
        for _ in range(3):
            first(), second()
        dev_t, host_t = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s.record()
            for _ in range(a.iters):
                first(), second()
            e.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev_t.append(s.elapsed_time(e) / a.iters * 1e3)
            host_t.append((t1 - t0) / a.iters * 1e6)
        print(f"{name}: device {sorted(dev_t)[1]:.0f} us per first_step + second_step (three windows of {a.iters}: "
              f"{', '.join(f'{t:.0f}' for t in dev_t)}), host issues one in {sorted(host_t)[1]:.0f} us", flush=True)
        return sorted(dev_t)[1]
    sam = O.FusedSAM(O.set_weight_decay(model), O.FusedSGD, model, rho=0.05, lr=1e-4, ema=ema)
    fused = pair("FusedSAM (norm + perturb, restore + sodt_sgd_ema_step)", sam.first_step, sam.second_step)
    per = SR.PerTensorSAM(O.FusedSGD([dict(g, rho=0.05, adaptive=False) for g in O.set_weight_decay(model)], model=model, lr=1e-4, ema=ema))
    loop = pair("per-tensor torch form around the same FusedSGD", per.first_step, per.second_step)
    print(f"fused pair / per-tensor form: {fused / loop:.3f} of the device time", flush=True)


if __name__ == "__main__":
    main()
