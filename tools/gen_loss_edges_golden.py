"""Write tests/golden/loss_edges.pt: the reference's own ComputeLoss (basics/utils/loss.py:90-224) on the small edge cases of
tests/loss_cases.py - rectangular grids, gr < 1, anchor_t of 2 / 4 / 8, nc of 1 / 2 / 32 with 1 / 3 / 8 anchors, pos-weights
without focal loss, thresholds hit exactly, a crowded 4 x 4 grid, tiny and ragged launch shapes.  Runs only where the
reference source tree is importable (the build machine); it reads oracle.gen_golden.import_reference() for the module stubs
and changes nothing under oracle/.

Layout: {"inputs": {key: {pred, targets, anchors}}, "cases": [{name, input, hyp, gr, nc, out, dpred, out64, out_ref_err,
dpred_ref_err}]}; cases that share a head output and targets share one `inputs` entry.  Per case the four returned losses
and d(loss * batch) / d(pred) in float32 as in training, and the same class run once more in float64 (default dtype
switched): `out64`, and `out_ref_err` / `dpred_ref_err` = max |float32 reference - float64 reference|, the reference's own
rounding error.

Left to the float64 restatement of tests/loss_ref.py alone (loss_cases' `golden` flag):
  * oor_mixed, oor_valid, oor_all: the reference's class indexes tobj with the image column and raises on a row whose image
    index is B or larger (and wraps -1 round to the last image), where the kernel skips such rows;
  * large_rand_plain, large_rand_focal2: the float32 reference's error on them is what their test measures.

usage: python tools/gen_loss_edges_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loss_cases as LC  # noqa: E402
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loss_edges.pt")


class _Det:
    pass


class _M(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def reference_loss(LM, c, dtype):
    """The reference class built and called under `dtype` as the default dtype; returns (four losses, dpred, matches)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        m, det = _M(), _Det()
        det.nl, det.na, det.nc, det.stride = 1, c["anchors"].shape[0], c["nc"], torch.tensor([4.])
        det.anchors = c["anchors"][None].to(dtype)
        m.detect, m.hyp, m.gr = [det], dict(c["hyp"]), c["gr"]
        cl = LM.ComputeLoss(m)
        assert (type(cl.BCEcls).__name__ == "FocalLoss") == (c["hyp"]["fl_gamma"] > 0)
        p = c["pred"].detach().to(dtype).clone().requires_grad_(True)
        tg = c["targets"].to(dtype)
        out = cl([p], tg)
        out[0].backward()
        n = cl.build_targets([p], tg)[2][0][0].shape[0]
        return [x.detach().reshape(-1) for x in out], p.grad, n
    finally:
        torch.set_default_dtype(old)


def main():
    import_reference()
    LM = importlib.import_module("reference.basics.utils.loss")
    inputs, cases = {}, []
    for name in LC.GOLDEN_NAMES:
        c = LC.case(name)
        assert c["golden"]
        key = next((k for k, v in inputs.items() if all(v[f].shape == c[f].shape and torch.equal(v[f], c[f])
                                                        for f in ("pred", "targets", "anchors"))), None)
        if key is None:
            key = name
            inputs[key] = dict(pred=c["pred"].clone(), targets=c["targets"].clone(), anchors=c["anchors"].clone())
        out, dpred, n = reference_loss(LM, c, torch.float32)
        out64, dpred64, n64 = reference_loss(LM, c, torch.float64)
        assert dpred.dtype == torch.float32 and dpred64.dtype == torch.float64 and n == n64 and n > 0
        assert bool(torch.isfinite(dpred).all()) and bool(torch.isfinite(dpred64).all())
        out_err = max(float((a.double() - b).abs().max()) for a, b in zip(out, out64))
        d_err = float((dpred.double() - dpred64).abs().max())
        print(f"[edges golden] {name}: input {key}, {c['targets'].shape[0]} targets, {n} matches, loss {float(out[0]):.6f} (lbox "
              f"{float(out[1]):.5f} lobj {float(out[2]):.5f} lcls {float(out[3]):.5f}); f32 vs f64: losses {out_err:.2e}, dpred "
              f"{d_err:.2e} (max|dpred| {float(dpred.abs().max()):.3e})")
        cases.append(dict(name=name, input=key, hyp=dict(c["hyp"]), gr=c["gr"], nc=c["nc"], out=[x.clone() for x in out],
                          dpred=dpred, out64=torch.cat(out64), out_ref_err=out_err, dpred_ref_err=d_err))
    torch.save(dict(inputs=inputs, cases=cases), OUT)
    print(f"[edges golden] wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
