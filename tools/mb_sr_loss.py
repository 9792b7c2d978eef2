"""sodt_sr_l1_fwd / sodt_sr_l1_bwd (csrc/srloss.hip) at the shape of output_sr in BASELINE config 5 (B = 4 @ 2048^2: (4, 4, 4096,
4096) f32, 1 GiB; uint8 targets, 0.25 GiB): device-event time per launch and the algorithmic bytes per second - 5 B / element
forward, 9 B backward.  1.25 / 2.25 GiB per launch do not fit the 256 MB Infinity Cache, so back-to-back launches stream from
HBM.  Beside them the torch spelling of Train.py:420-427 on f32 targets, value and gradient through autograd.

usage: python tools/mb_sr_loss.py [--batch 4] [--size 4096] [--iters 20]
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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_sr_loss.py measures on the GPU; there is nothing to time without one")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    o = torch.rand(B, 4, S, S, generator=g, device=dev)
    rgb = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8, device=dev)
    ir = torch.randint(0, 256, (B, 1, S, S), generator=g, dtype=torch.uint8, device=dev)
    n = o.numel()
    ws = torch.empty(ops.sr_l1_workspace_bytes(B, 4, S, S), dtype=torch.uint8, device=dev)
    loss, up, dsr = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(o)

    def timed(name, nbytes, launch):
        best = []
        for _ in range(3):                                # three windows: their spread is printed
            launch()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                launch()
            e.record()
            torch.cuda.synchronize()
            best.append(s.elapsed_time(e) / a.iters * 1e3)
        us = min(best)
        rate = f", {nbytes / us / 1e6:.2f} TB/s over {nbytes / 2**30:.2f} GiB" if nbytes else ""
        print(f"{name}: {us:.1f} us ({', '.join(f'{b:.1f}' for b in best)}){rate}", flush=True)
        return us

    f = timed("sodt_sr_l1_fwd (uint8 targets)", 5 * n, lambda: ops.sr_l1_fwd(o, rgb, ir, "RGB+IR", ws, loss))
    b = timed("sodt_sr_l1_bwd (uint8 targets)", 9 * n, lambda: ops.sr_l1_bwd(o, rgb, ir, "RGB+IR", up, dsr))
    print(f"both: {f + b:.1f} us, {14 * n / (f + b) / 1e6:.2f} TB/s over {14 * n / 2**30:.2f} GiB; loss {float(loss):.7f}", flush=True)
    del dsr
    leaf = o.requires_grad_(True)
    L1 = torch.nn.L1Loss()

    def torch_term(make_targets):
        leaf.grad = None
        image, ir_image = (rgb.float() / 255.0, ir.float() / 255.0) if make_targets else (image_f, ir_f)
        (0.1 * (L1(leaf[:, 0:3], image) + L1(leaf[:, 3:], ir_image[:, 0:1]))).backward()
    image_f, ir_f = rgb.float() / 255.0, ir.float() / 255.0
    t = timed("torch expression, value + gradient, f32 targets given", 0, lambda: torch_term(False))
    t2 = timed("torch expression, value + gradient, f32 targets made from uint8", 0, lambda: torch_term(True))
    print(f"fused / torch: {t / (f + b):.1f}x (targets given), {t2 / (f + b):.1f}x (targets made per call)", flush=True)


if __name__ == "__main__":
    main()
