"""sodt_preprocess_u8_ms (csrc/multiscale.hip), the one launch of `--multi-scale` (Train.py:364-374 + 396-402), against what ran
before it for the same result: preprocess_batch (sodt_preprocess_u8) followed by the two ATen interpolations of the loop.  B = 8,
3 + 3 channels of 1024^2 uint8, down_factor 2, drawn sizes S = 576, 768, 1024, 1536.  Every shape is warmed first; then the two
paths alternate in one process, three windows of --iters launches each under device events.  Printed per size: the median and
the three windows of both, the bytes each needs from shapes (uint8 in + f32 out; the three launches also write and read the f32
intermediate at the shrunk size) and the achieved bytes per second.  Both outputs are compared once per size.

--loop N then runs N training steps (bench.py's model and step, bf16) whose size is drawn per step by multi_scale_size with
runs_at, and prints per step the size, whether the engine had a plan for it, the step time and torch.cuda.memory_reserved():
the cost of the engine's four-plan LRU under changing sizes.

usage: python tools/mb_multiscale.py [--iters 50] [--sizes 576 768 1024 1536] [--loop 32 [--loop-batch 8] [--loop-seed 0]]
"""
import argparse
import importlib
import os
import random
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "small-object-detection-transformers_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--load", type=int, default=1024, help="side of the uint8 batch the loader delivers")
    ap.add_argument("--down-factor", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[576, 768, 1024, 1536])
    ap.add_argument("--loop", type=int, default=0, help="also run this many training steps over drawn sizes")
    ap.add_argument("--loop-batch", type=int, default=8)
    ap.add_argument("--loop-seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_multiscale.py measures on the GPU; there is nothing to time without one")
    P = importlib.import_module(PKG + ".preprocess")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, L, f = a.batch, a.load, a.down_factor
    rgb = torch.randint(0, 256, (B, 3, L, L), generator=g, dtype=torch.uint8).to(dev)
    ir = torch.randint(0, 256, (B, 3, L, L), generator=g, dtype=torch.uint8).to(dev)
    mid = L // f

    def fused(S):
        return P.preprocess_batch(rgb, ir, f, size=S)

    def three(S):
        x, xi = P.preprocess_batch(rgb, ir, f)
        return (F.interpolate(x, size=[S, S], mode="bilinear", align_corners=False),
                F.interpolate(xi, size=[S, S], mode="bilinear", align_corners=False))

    def window(fn, S):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn(S)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    sizes = [S for S in a.sizes if S != mid]            # S == mid is the plain sodt_preprocess_u8 launch on both sides
    for S in sizes:                                     # warm every shape of both paths, pin the launches, compare the results
        with ops.Recorder() as rec:
            o = fused(S)
        assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8_ms"], [c[2] for c in rec.calls]
        r = three(S)
        d = max(float((o[0] - r[0]).abs().max()), float((o[1] - r[1]).abs().max()))
        print(f"S={S}: max |one launch - three launches| = {d:.2e}", flush=True)
        for _ in range(5):
            fused(S)
            three(S)
    torch.cuda.synchronize()
    u8_in = B * 6 * L * L
    inter = B * 6 * mid * mid * 4
    print(f"B={B}, 3+3 channels of {L}^2 uint8, down_factor {f}: us per call, median of three windows of {a.iters} (the windows)")
    for S in sizes:
        tf, tt = [], []
        for _ in range(3):                              # alternate the two paths: drift of the machine hits both
            tf.append(window(fused, S))
            tt.append(window(three, S))
        out = B * 6 * S * S * 4
        bf, bt = u8_in + out, u8_in + out + 2 * inter
        mf, mt = sorted(tf)[1], sorted(tt)[1]
        print(f"S={S}: one launch {mf * 1e3:.1f} ({', '.join(f'{v * 1e3:.1f}' for v in tf)}) {bf / 1e6:.0f} MB -> {bf / mf / 1e9:.2f} TB/s | "
              f"three launches {mt * 1e3:.1f} ({', '.join(f'{v * 1e3:.1f}' for v in tt)}) {bt / 1e6:.0f} MB -> {bt / mt / 1e9:.2f} TB/s | "
              f"ratio {mt / mf:.2f}x, spread one {(max(tf) - min(tf)) * 1e3:.1f} us, three {(max(tt) - min(tt)) * 1e3:.1f} us", flush=True)
    if a.loop:
        loop(a, dev, P)


def loop(a, dev, P):
    import bench
    O = importlib.import_module(PKG + ".optim")
    LS = importlib.import_module(PKG + ".loss")
    B, L, f = a.loop_batch, a.load, a.down_factor
    mid = L // f
    model = bench.build_model(mid, dev, torch.bfloat16)
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    ema = O.ModelEMA(model)
    opt = O.FusedSGD(O.set_weight_decay(model), model=model, lr=0.01, momentum=0.937, nesterov=True, ema=ema)
    compute_loss = LS.ComputeLoss(model)
    g = torch.Generator().manual_seed(1)
    rgb = torch.randint(0, 256, (B, 3, L, L), generator=g, dtype=torch.uint8).to(dev)
    ir = torch.randint(0, 256, (B, 3, L, L), generator=g, dtype=torch.uint8).to(dev)
    targets = LS.synthetic_targets(B, 32, 8, seed=1).to(dev)
    rng = random.Random(a.loop_seed)
    eng = model._get_engine()
    print(f"loop: model built at {mid}, B={B}, bf16, sizes from multi_scale_size({L}, ({mid}, {mid}), gs=64, runs_at), "
          f"{eng.MAX_PLANS} plans kept", flush=True)
    for step in range(a.loop):
        ns = P.multi_scale_size(L, (mid, mid), gs=64, rng=rng, runs_at=model.runs_at)
        had = any(k[1] == ns[0] for k in eng.plans)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, xi = P.preprocess_batch(rgb, ir, f, size=ns)
        pred, _ = model(x, xi, "RGB+IR")
        loss = compute_loss(pred, targets)[0]
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"step {step:2d}: S={ns[0]:4d} {'plan kept' if had else 'new plan '} {dt * 1e3:8.1f} ms, loss/B {float(loss.detach()) / B:.4f}, "
              f"reserved {torch.cuda.memory_reserved() / 2 ** 30:.1f} GiB, allocated {torch.cuda.memory_allocated() / 2 ** 30:.1f} GiB", flush=True)


if __name__ == "__main__":
    main()
