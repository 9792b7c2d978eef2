"""Host restatement of the reference's ComputeLoss for one detection layer (basics/utils/loss.py:116-224, FocalLoss :36-62,
CIoU general.py:347-389) with autograd, the yardstick of test_loss_ref_host.py, test_loss_edges_gpu.py and
test_loss_focal_gpu.py.  Built on oracle.ref_torch.build_targets and bbox_ciou; fl_gamma == 0 and > 0, any na, nc >= 1,
ny != nx.

* `compute_loss_f64`: the discrete decisions (anchor-ratio test, the four neighbour tests, .long(), the clamp) are taken
  the way the reference takes them, in float32, by build_targets on the float32 tensors; the continuous arithmetic (tbox,
  CIoU, BCE / focal, the means) is redone in float64 from the float32 inputs.
* `compute_loss_f32`: the same statement with everything in float32, i.e. the reference's own arithmetic; its distance to
  `compute_loss_f64` is the rounding error a float32 implementation can be held to.
* `candidates`: the (b, a, gj, gi, tcls) rows of build_targets in the reference's order, in either precision.

Rows whose image index is outside [0, B) are removed before build_targets.  The kernel skips such rows where the
reference would raise.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import ref_torch as R


def focal(x, t, pw, gamma):
    """FocalLoss.forward (loss.py:45-59) with reduction='mean', alpha = 0.25."""
    bce = F.binary_cross_entropy_with_logits(x, t, pos_weight=x.new_tensor([pw]), reduction="none")
    p = x.sigmoid()
    p_t = t * p + (1 - t) * (1 - p)
    a_t = t * 0.25 + (1 - t) * 0.75
    return (bce * a_t * (1.0 - p_t) ** gamma).mean()


def _bce(x, t, pw, gamma):
    if gamma > 0:
        return focal(x, t, pw, gamma)
    return F.binary_cross_entropy_with_logits(x, t, pos_weight=x.new_tensor([pw]))


def in_range_rows(targets, B):
    """The rows whose image index (truncated like .long()) lies in [0, B)."""
    b = targets[:, 0].long()
    return targets[(b >= 0) & (b < B)]


def candidates(shape, targets, anchors, anchor_t, dtype=torch.float32):
    """build_targets' candidates for a head output of `shape` = (B, na, ny, nx, no), decided in `dtype`, in the reference's
    order: list of (b, a, gj, gi, tcls)."""
    tg = in_range_rows(targets.float(), shape[0]).to(dtype)
    tcls, _, (b, a, gj, gi), _ = R.build_targets(torch.empty(shape, dtype=dtype), tg, anchors.float().to(dtype), anchor_t)
    return list(zip(b.tolist(), a.tolist(), gj.tolist(), gi.tolist(), tcls.tolist()))


def _compute(pred, targets, anchors, hyp, gr, nc, dtype):
    p32 = pred.detach().float()
    B, na, ny, nx, no = p32.shape
    assert no == nc + 5 and anchors.shape == (na, 2)
    tg32 = in_range_rows(targets.detach().float(), B)
    a32 = anchors.detach().float()
    gamma = float(hyp.get("fl_gamma", 0.0))
    # float32 decisions; a second call with the row number in the class column (which no decision reads) tells which
    # target each candidate came from
    tcls, tbox32, (b, a, gj, gi), _ = R.build_targets(p32, tg32, a32, hyp["anchor_t"])
    rows = tg32.clone()
    rows[:, 1] = torch.arange(tg32.shape[0], dtype=torch.float32)
    src = R.build_targets(p32, rows, a32, hyp["anchor_t"])[0]
    p = p32.to(dtype).requires_grad_(True)
    tg, anc = tg32.to(dtype), a32.to(dtype)
    lcls, lbox = p.new_zeros(1), p.new_zeros(1)
    tobj = torch.zeros_like(p[..., 0])
    n = int(b.shape[0])
    if n:
        gain = torch.tensor([nx, ny, nx, ny], dtype=dtype)
        g = tg[src, 2:6] * gain                                     # loss.py:184
        tbox = torch.cat((g[:, :2] - torch.stack((gi, gj), 1).to(dtype), g[:, 2:]), 1)      # :220, after the in-place clamp
        ps = p[b, a, gj, gi]
        pxy = ps[:, :2].sigmoid() * 2. - 0.5
        pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * anc[a]
        iou = R.bbox_ciou(torch.cat((pxy, pwh), 1).T, tbox)
        lbox = lbox + (1.0 - iou).mean()
        tobj[b, a, gj, gi] = (1.0 - gr) + gr * iou.detach().clamp(0)               # duplicates: the last entry wins (CPU)
        if nc > 1:
            tc = torch.zeros_like(ps[:, 5:])
            tc[range(n), tcls] = 1.0
            lcls = lcls + _bce(ps[:, 5:], tc, hyp["cls_pw"], gamma)
    lobj = _bce(p[..., 4], tobj, hyp["obj_pw"], gamma).reshape(1) * 4.0
    lbox, lobj, lcls = lbox * hyp["box"], lobj * hyp["obj"], lcls * hyp["cls"]
    loss = (lbox + lobj + lcls) * B
    loss.backward()
    return loss.detach(), lbox.detach(), lobj.detach(), lcls.detach(), n, p.grad


def compute_loss_f64(pred, targets, anchors, hyp, gr=1.0, nc=8):
    """-> (loss * B, lbox, lobj, lcls, n, dpred): the four float64 values ComputeLoss.__call__ returns (loss.py:163), the
    number of candidates and d(loss * B) / d(pred) in float64, on the float32 values of `pred`, `targets`, `anchors`.
    Rows whose image index is outside [0, B) are removed before build_targets.  The kernel skips such rows where the
    reference would raise."""
    return _compute(pred, targets, anchors, hyp, gr, nc, torch.float64)


def compute_loss_f32(pred, targets, anchors, hyp, gr=1.0, nc=8):
    """The same statement in float32 throughout: the reference's arithmetic."""
    return _compute(pred, targets, anchors, hyp, gr, nc, torch.float32)


def gates(ref_out, ref_dpred):
    """The project's gates for the loss kernel: 2e-5 * max(1, |ref|) on each of the four losses, 2e-6 + 2e-5 * max|dpred|
    on the gradient."""
    return [2e-5 * max(1.0, float(r.abs().max())) for r in ref_out], 2e-6 + 2e-5 * float(ref_dpred.abs().max())
