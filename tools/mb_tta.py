"""Test-time augmentation (basics/models/model.py:155-184): ``Model.forward(augment=True)`` against the same result composed
from ATen ``flip`` / ``interpolate`` / ``pad`` / ``cat`` and three plain forwards, and the two kernels of csrc/tta.hip alone against
their ATen equivalents.  B = 8 at 1024 x 1024, bf16, on a model built at 1024 (bench.py's model): passes at 1024 / 896 / 704.

Every shape is warmed first; then the two sides of a comparison alternate in one process, three windows of --iters calls each
(--kernel-iters for the kernels alone) under device events.  Printed: the median and the three windows of both sides; for the
kernels alone also the bytes they need from shapes (``sodt_tta_scale``: per pass the source planes read once and the padded planes written; ``sodt_detect_decode_tta``:
the raw head output read and z written) and the achieved bytes per second.  The results of both sides are compared once.

usage: python tools/mb_tta.py [--iters 20] [--kernel-iters 200] [--batch 8] [--size 1024]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=200, help="calls per window of the kernels-alone comparisons")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_tta.py measures on the GPU; there is nothing to time without one")
    import bench
    import tta_ref
    T = importlib.import_module(PKG + ".tta")
    ops = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    model = bench.build_model(S, dev, torch.bfloat16).eval()
    eng = model._get_engine()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    ir = torch.rand(B, 3, S, S, generator=g).to(dev)
    scales, flips = T.check_passes(model.tta_scales, model.tta_flips)
    sizes = T.tta_sizes((S, S), scales, 32, model.runs_at)
    made = [k for k in range(len(scales)) if scales[k] != 1 or flips[k]]
    passes = [(*sizes[k], flips[k]) for k in made]
    print(f"B={B}, 3+3 channels of {S}^2 f32, bf16 engine; passes (scale, flip, content, padded): "
          f"{[(s, f, *z) for s, f, z in zip(scales, flips, sizes)]}", flush=True)

    def aten_inputs():
        out = []
        for si, fi, (_, pad) in zip(scales, flips, sizes):
            out.append(tuple(tta_ref.scale_img(t.flip(fi) if fi else t, si, padded=pad) for t in (x, ir)))
        return out

    def aten_tail(zs):
        y = []
        for yi, si, fi in zip(zs, scales, flips):
            yi[..., :4] /= si
            if fi == 2:
                yi[..., 1] = S - yi[..., 1]
            elif fi == 3:
                yi[..., 0] = S - yi[..., 0]
            y.append(yi)
        return torch.cat(y, 1)

    def fused():
        with torch.no_grad():
            return model(x, ir, augment=True)[0]

    def composed():
        with torch.no_grad():
            return aten_tail([model(xi, iri)[0] for xi, iri in aten_inputs()])

    def scale_kernel():
        return T.scale_pair(x, ir, passes)

    def scale_aten():
        return [p for k, p in enumerate(aten_inputs()) if k in made]

    # the raw head outputs of the three passes, kept for the decode comparison (copies: the engine may reuse its own)
    with torch.no_grad():
        preds = [eng.run(xi, iri, torch.bfloat16, False)[0].clone() for xi, iri in aten_inputs()]
    rows = sum(p.shape[1] * p.shape[2] * p.shape[3] for p in preds)
    zbuf = torch.empty(B, rows, preds[0].shape[-1], device=dev)

    def decode_kernel():
        off = 0
        for p, si, fi in zip(preds, scales, flips):
            off = eng.decode_tta(p, zbuf, off, si, fi, S, S)
        return zbuf

    def decode_aten():
        return aten_tail([eng.decode(p) for p in preds])

    def window(fn, iters):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters

    def compare(name, one, other, iters, bytes_one=None):
        for _ in range(3):                                  # warm every shape of both sides
            one()
            other()
        t1, t2 = [], []
        for _ in range(3):                                  # alternate: drift of the machine hits both
            t1.append(window(one, iters))
            t2.append(window(other, iters))
        m1, m2 = sorted(t1)[1], sorted(t2)[1]
        rate = f" {bytes_one / 1e6:.0f} MB -> {bytes_one / m1 / 1e9:.2f} TB/s |" if bytes_one else " |"
        print(f"{name}: engine {m1 * 1e3:.1f} us ({', '.join(f'{v * 1e3:.1f}' for v in t1)}){rate} "
              f"ATen {m2 * 1e3:.1f} us ({', '.join(f'{v * 1e3:.1f}' for v in t2)}) | difference {(m2 - m1) * 1e3:.1f} us, "
              f"ratio {m2 / m1:.3f}x, spread engine {(max(t1) - min(t1)) * 1e3:.1f} us, ATen {(max(t2) - min(t2)) * 1e3:.1f} us", flush=True)

    # launches of the engine's side, and the results of both sides once
    names, real = [], ops._launch

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    fused()
    ops._launch = spy
    try:
        zf = fused()
    finally:
        ops._launch = real
    print(f"augmented forward, live launches beside the three replayed plans: {names}", flush=True)
    zc = composed()
    d_box = float((zf[..., :4] - zc[..., :4]).abs().max())
    d_cls = float((zf[..., 4:] - zc[..., 4:]).abs().max())
    print(f"z {tuple(zf.shape)}: max |engine - composed| boxes {d_box:.3e} (pixels), scores {d_cls:.3e} "
          "(bf16 forwards on inputs that differ by the resize's rounding)", flush=True)
    for (o1, o2), (r1, r2) in zip(scale_kernel(), scale_aten()):
        print(f"scaled inputs {tuple(o1.shape)}: max |kernel - ATen| = {max(float((o1 - r1).abs().max()), float((o2 - r2).abs().max())):.2e}")
    print(f"decoded rows: max |kernel - ATen| = {float((decode_kernel() - decode_aten()).abs().max()):.2e}", flush=True)

    planes = B * 6
    scale_bytes = sum(planes * 4 * (S * S + hp * wp) for _, (hp, wp), _ in passes)
    decode_bytes = 2 * zbuf.numel() * 4
    compare("augmented forward", fused, composed, a.iters)
    compare("sodt_tta_scale (one launch) vs flip + interpolate + pad", scale_kernel, scale_aten, a.kernel_iters, scale_bytes)
    compare("3 x sodt_detect_decode_tta vs 3 x decode + div + rsub + cat", decode_kernel, decode_aten, a.kernel_iters, decode_bytes)


if __name__ == "__main__":
    main()
