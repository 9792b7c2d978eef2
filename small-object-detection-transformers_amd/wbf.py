"""Weighted boxes fusion on the GPU - the drop-in for `weighted_boxes` (`utils/general.py:515`, the alternative to
non_max_suppression at test.py:152-153) and for the `weighted_boxes_fusion` it calls
(`utils/ensemble_boxes/ensemble_boxes_wbf.py:150`).

Candidate selection, the sort, the sequential clustering and the confidence rescaling run in HIP kernels (csrc/wbf.hip)
behind the C ABI (`sodt_wbf_candidates`, `sodt_wbf_fuse`) for the whole batch at once; the host reads the per-image
counts once, at the very end, to slice the result.  The clustering reproduces the reference's arithmetic (float32
coordinate sums updated through float64, float64 score sums, float64 IoU), so its match decisions are the reference's.

Differences from the reference, all documented in DESIGN.md:
  * candidates are walked by label, then descending weighted score, then ascending source row, and clusters come out
    by descending score, then label, then creation order; the reference's argsort()[::-1] leaves equal scores unordered.
  * `weighted_boxes` takes `xyxy=True` to return corner boxes; the default is the reference's actual return value,
    [cx, cy, w, h] in pixels (general.py:552-554 converts back with xyxy2xywh although the docstring says xyxy).
  * the 10 s time limit (general.py:559-561) does not exist.
  * where the reference prints and calls exit() (unknown conf_type, length mismatches) a ValueError is raised.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import ops

CONF_TYPES = {"avg": 0, "max": 1, "box_and_model_avg": 2, "absent_model_aware_avg": 3}
MAX_MODELS = 32


def _fuse(boxes, scores, labels, model, src, counts, weights, iou_thr, skip_box_thr, conf_type, allows_overflow,
          member=False, scan_lanes=0):
    """(B, cap) candidates -> (out_boxes (B, cap, 4), out_scores, out_labels, out_counts (B), member or None); no host read."""
    B, cap = scores.shape
    dev = scores.device
    ws = torch.empty(ops.wbf_fuse_workspace_bytes(B, cap), dtype=torch.uint8, device=dev)
    out_boxes = torch.empty(B, cap, 4, dtype=torch.float32, device=dev)
    out_scores = torch.empty(B, cap, dtype=torch.float32, device=dev)
    out_labels = torch.empty(B, cap, dtype=torch.int32, device=dev)
    out_counts = torch.empty(B, dtype=torch.int32, device=dev)
    mem = torch.empty(B, cap, dtype=torch.int32, device=dev) if member else None
    ops.wbf_fuse(boxes, scores, labels, model, src, counts, weights, iou_thr, skip_box_thr, conf_type, allows_overflow, ws,
                 out_boxes, out_scores, out_labels, out_counts, mem, scan_lanes)
    return out_boxes, out_scores, out_labels, out_counts, mem


def _weighted_boxes_device(prediction: torch.Tensor, image_size, conf_thres: float = 0.25, iou_thres: float = 0.45,
                          xyxy: bool = False, return_member: bool = False):
    """(Internal; the tests use it.)  `weighted_boxes` without its final host read: returns rows (B, N, 6) f32, of which the first counts[b] of image b
    are valid, and counts (B) int32 on the device (and, with return_member, (B, N) int32: the output row each
    prediction row was fused into, -1 for a row that was no candidate)."""
    if not prediction.is_cuda:
        raise RuntimeError("weighted_boxes: the prediction must live on the GPU (there is no CPU fallback)")
    if prediction.dim() != 3 or prediction.shape[2] < 6:
        raise ValueError(f"prediction must be (B, N, 5 + nc), got {tuple(prediction.shape)}")
    pred = prediction.detach()
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        pred = pred.float().contiguous()
    B, N, _ = pred.shape
    dev = pred.device
    with torch.cuda.device(dev):
        if B == 0 or N == 0:
            rows = torch.zeros(B, N, 6, dtype=torch.float32, device=dev)
            member = torch.full((B, N), -1, dtype=torch.int32, device=dev)
            counts = torch.zeros(B, dtype=torch.int32, device=dev)
            return (rows, counts, member) if return_member else (rows, counts)
        boxes = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
        scores = torch.empty(B, N, dtype=torch.float32, device=dev)
        labels = torch.empty(B, N, dtype=torch.int32, device=dev)
        src = torch.empty(B, N, dtype=torch.int32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        ops.wbf_candidates(pred, conf_thres, image_size, boxes, scores, labels, src, counts)
        ob, os_, ol, oc, mem = _fuse(boxes, scores, labels, None, src, counts, [1.0], iou_thres, 0.0, 0, False,
                                     member=return_member)
        b = ob.double()                                   # general.py:552-554 run in numpy float64
        if not xyxy:
            b = torch.stack(((b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0],
                             b[..., 3] - b[..., 1]), -1)
        b = b * image_size
        rows = torch.cat((b.float(), os_.unsqueeze(-1), ol.float().unsqueeze(-1)), -1)
        if not return_member:
            return rows, oc
        # member is indexed by candidate slot: carry it back to the prediction row the candidate came from
        slot = torch.arange(N, device=dev).unsqueeze(0) < counts.unsqueeze(1)
        member = torch.full((B, N + 1), -1, dtype=torch.int32, device=dev)
        member.scatter_(1, torch.where(slot, src.long(), torch.full_like(src, N, dtype=torch.long)), mem)
        return rows, oc, member[:, :N].contiguous()


def weighted_boxes(prediction: torch.Tensor, image_size, conf_thres: float = 0.25, iou_thres: float = 0.45,
                   classes: Optional[Sequence[int]] = None, agnostic: bool = False, multi_label: bool = False,
                   labels=(), xyxy: bool = False) -> List[torch.Tensor]:
    """Weighted boxes fusion of the eval output (B, N, 5 + nc) of `Model.forward`; one (n, 6) f32 tensor per image on
    the prediction's device.  Columns 0:4 are what the reference returns, [cx, cy, w, h] in pixels (general.py:552-554);
    `xyxy=True` - the only extension - gives [x1, y1, x2, y2], which is what test.py:155-264, scale_coords and
    DetectionMetrics take.  Columns 4, 5: confidence and class.

    `classes`, `agnostic`, `multi_label` and `labels` are accepted and ignored, as in the reference: general.py:515-516
    declares them, and the body (general.py:522-563) never reads one of them (its multi_label branch, :539-541, is
    commented out)."""
    rows, counts = _weighted_boxes_device(prediction, image_size, conf_thres, iou_thres, xyxy)
    n = counts.tolist()                                   # the one host read
    return [rows[b, :n[b]] for b in range(rows.shape[0])]


def weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights=None, iou_thr: float = 0.55,
                          skip_box_thr: float = 0.0, conf_type: str = "avg", allows_overflow: bool = False):
    """ensemble_boxes_wbf.py:150-225 for one image: one entry per model of boxes (n, 4) corners in [0, 1], scores (n) and
    labels (n), all device tensors.  Returns (boxes (m, 4) f32, scores (m) f32, labels (m) f32) on the device, by
    descending score.  A weights list of the wrong length is replaced by ones, as in the reference (:169-171)."""
    return _weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights, iou_thr, skip_box_thr, conf_type,
                                  allows_overflow)


def _weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights=None, iou_thr=0.55, skip_box_thr=0.0,
                           conf_type="avg", allows_overflow=False, return_member=False) -> Tuple[torch.Tensor, ...]:
    """(Internal; the tests use return_member.)  weighted_boxes_fusion; with return_member also (sum n) int32: the output
    row of each input box, -1 if skipped."""
    if conf_type not in CONF_TYPES:
        raise ValueError(f"unknown conf_type {conf_type!r}: must be one of {', '.join(CONF_TYPES)}")
    M = len(boxes_list)
    if M < 1 or M > MAX_MODELS:
        raise ValueError(f"weighted_boxes_fusion takes 1 to {MAX_MODELS} models, got {M}")
    if len(scores_list) != M or len(labels_list) != M:
        raise ValueError("boxes_list, scores_list and labels_list must have one entry per model")
    for t in range(M):
        if len(boxes_list[t]) != len(scores_list[t]):
            raise ValueError(f"model {t}: {len(boxes_list[t])} boxes and {len(scores_list[t])} scores")
        if len(boxes_list[t]) != len(labels_list[t]):
            raise ValueError(f"model {t}: {len(boxes_list[t])} boxes and {len(labels_list[t])} labels")
    if weights is None or len(weights) != M:
        weights = [1.0] * M
    weights = [float(w) for w in weights]
    if not all(torch.is_tensor(t) and t.is_cuda for t in list(boxes_list) + list(scores_list) + list(labels_list)):
        raise RuntimeError("weighted_boxes_fusion: the boxes, scores and labels must live on the GPU (there is no CPU fallback)")
    dev = boxes_list[0].device
    with torch.cuda.device(dev):
        boxes = torch.cat([b.detach().reshape(-1, 4).float() for b in boxes_list], 0).contiguous()
        n = boxes.shape[0]
        if n == 0:
            empty = (torch.zeros(0, 4, device=dev), torch.zeros(0, device=dev), torch.zeros(0, device=dev))
            return empty + (torch.zeros(0, dtype=torch.int32, device=dev),) if return_member else empty
        scores = torch.cat([s.detach().reshape(-1).float() for s in scores_list], 0).contiguous()
        labels = torch.cat([l.detach().reshape(-1).to(torch.int32) for l in labels_list], 0).contiguous()
        model = torch.cat([torch.full((len(s),), t, dtype=torch.int32, device=dev) for t, s in enumerate(scores_list)], 0)
        counts = torch.full((1,), n, dtype=torch.int32, device=dev)
        ob, os_, ol, oc, mem = _fuse(boxes.view(1, n, 4), scores.view(1, n), labels.view(1, n), model.view(1, n), None,
                                     counts, weights, iou_thr, skip_box_thr, CONF_TYPES[conf_type], allows_overflow,
                                     member=return_member)
        m = int(oc.item())                                # the one host read
        out = (ob[0, :m], os_[0, :m], ol[0, :m].float())
        return out + (mem[0],) if return_member else out
