"""Write tests/golden/loss_focal.pt: the reference's own ComputeLoss (basics/utils/loss.py:90-163) with hyp['fl_gamma'] > 0,
i.e. with FocalLoss(BCEWithLogitsLoss(pos_weight), gamma, alpha=0.25) around the class and the objectness term
(loss.py:36-62, :103-108), on small fixed head outputs and targets.  Runs only where the reference source tree is
importable (the build machine); it reads oracle.gen_golden.import_reference() for the module stubs and changes nothing
under oracle/.

Per case: inputs, the four returned losses and d(loss * batch) / d(pred) in float32 as in training, and the same class
run once more in float64 (default dtype switched, so every constant the class creates is a double): `out64`, and
`out_ref_err` / `dpred_ref_err` = max |float32 reference - float64 reference|, the reference's own rounding error, which
is what a float32 implementation can be held to.  Logits are uniform in [-8, 8], where the reference's autograd is
finite for every gamma (1 - p_t stays above 3e-4).

usage: python tools/gen_loss_focal_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_torch as R  # noqa: E402
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loss_focal.pt")
ANCHORS = torch.tensor([[10., 13.], [16., 30.], [33., 23.]]) / 4          # models/model.yaml:8 on the stride-4 grid

# (fl_gamma, cls_pw, obj_pw, batch, grid, targets per image)
CASES = [(0.5, 1.0, 1.0, 2, 16, 10),
         (1.5, 1.0, 1.0, 1, 32, 20),
         (2.0, 1.0, 1.0, 1, 16, 0),
         (1.5, 1.0, 1.0, 1, 16, 1),
         (2.0, 1.5, 0.7, 2, 16, 10)]


class _Det:
    pass


class _M(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def reference_loss(LM, hyp, pred, tg, dtype):
    """The reference class built and called under `dtype` as the default dtype; returns (four losses, dpred)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        m, det = _M(), _Det()
        det.nl, det.na, det.nc, det.stride = 1, 3, 8, torch.tensor([4.])
        det.anchors = ANCHORS[None].to(dtype)
        m.detect, m.hyp, m.gr = [det], dict(hyp), 1.0
        cl = LM.ComputeLoss(m)
        assert type(cl.BCEcls).__name__ == "FocalLoss" and type(cl.BCEobj).__name__ == "FocalLoss"
        p = pred.detach().to(dtype).clone().requires_grad_(True)
        out = cl([p], tg.to(dtype))
        out[0].backward()
        return [x.detach().reshape(-1) for x in out], p.grad
    finally:
        torch.set_default_dtype(old)


def main():
    import_reference()
    LM = importlib.import_module("reference.basics.utils.loss")
    cases = []
    for seed, (gamma, cls_pw, obj_pw, B, t, per) in enumerate(CASES):
        g = torch.Generator().manual_seed(300 + seed)
        pred = torch.rand(B, 3, t, t, 13, generator=g) * 16.0 - 8.0
        tg = R.synthetic_targets(B, per, 8, seed=300 + seed) if per else torch.zeros(0, 6)
        tg[:, 4:6] *= 256.0 / t                                           # box sizes in the anchors' range on this grid
        hyp = dict(R.LOSS_HYP, fl_gamma=gamma, cls_pw=cls_pw, obj_pw=obj_pw)
        out, dpred = reference_loss(LM, hyp, pred, tg, torch.float32)
        out64, dpred64 = reference_loss(LM, hyp, pred, tg, torch.float64)
        assert dpred.dtype == torch.float32 and dpred64.dtype == torch.float64
        assert bool(torch.isfinite(dpred).all()) and bool(torch.isfinite(dpred64).all())
        n = R.build_targets(pred, tg, ANCHORS)[2][0].shape[0]
        assert (n > 0) == (per > 0), "a case with targets must match some"
        out_err = max(float((a.double() - b).abs().max()) for a, b in zip(out, out64))
        d_err = float((dpred.double() - dpred64).abs().max())
        print(f"[focal golden] gamma {gamma} pw ({cls_pw}, {obj_pw}) B={B} grid {t}: {tg.shape[0]} targets, {n} matches, "
              f"loss {float(out[0]):.6f} (lbox {float(out[1]):.5f} lobj {float(out[2]):.5f} lcls {float(out[3]):.5f}); "
              f"f32 vs f64: losses {out_err:.2e}, dpred {d_err:.2e} (max|dpred| {float(dpred.abs().max()):.3e})")
        cases.append(dict(pred=pred, targets=tg, anchors=ANCHORS.clone(), hyp=hyp, gr=1.0, out=[x.clone() for x in out],
                          dpred=dpred, out64=torch.cat(out64), out_ref_err=out_err, dpred_ref_err=d_err))
    torch.save(cases, OUT)
    print(f"[focal golden] wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
