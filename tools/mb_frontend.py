"""Micro-benchmark of the front-end kernels (sodt_frontend_fwd / _bwd) at the bench shape (B=8 @ 1024^2)."""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("small-object-detection-transformers_amd.ops")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = "cuda:0"
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand(a.B, 3, a.S, a.S, generator=g).to(dev)
    ir = torch.rand(a.B, 1, a.S, a.S, generator=g).to(dev)
    w = (torch.randn(4, 48, 16, generator=g) * 0.2).to(dev)
    b = (torch.randn(4, 48, generator=g) * 0.1).to(dev)
    gam = (1 + 0.1 * torch.randn(4, 48, generator=g)).to(dev)
    bet = (0.1 * torch.randn(4, 48, generator=g)).to(dev)
    t = a.S // 4
    irp = ir[:, 0]
    y = torch.zeros(a.B * t * t, 192, device=dev, dtype=dt)
    ops.frontend_fwd(rgb, irp, a.S * a.S, w, b, gam, bet, y, a.B, a.S, a.S)
    dy = torch.randn_like(y)
    wsb = torch.empty(ops.frontend_bwd_workspace_bytes(a.B, a.S, a.S) // 4, device=dev)
    dw, db, dg, dbe = torch.zeros_like(w), torch.zeros_like(b), torch.zeros_like(gam), torch.zeros_like(bet)
    for name, fn in (("fwd", lambda: ops.frontend_fwd(rgb, irp, a.S * a.S, w, b, gam, bet, y, a.B, a.S, a.S)),
                     ("bwd", lambda: ops.frontend_bwd(rgb, irp, a.S * a.S, w, b, gam, bet, dy, dw, db, dg, dbe, a.B, a.S, a.S)),
                     ("bwd+ws", lambda: ops.frontend_bwd(rgb, irp, a.S * a.S, w, b, gam, bet, dy, dw, db, dg, dbe, a.B, a.S, a.S, ws=wsb))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"frontend_{name} {a.dtype} B={a.B} S={a.S}: {e0.elapsed_time(e1) / a.iters:.4f} ms")


if __name__ == "__main__":
    main()

