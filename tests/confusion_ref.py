"""Host restatements for the confusion-matrix tests and tools/mb_metrics.py --confusion.

* `process_batch_np`: ConfusionMatrix.process_batch (metrics.py:117-155) in numpy f32 on top of metrics_ref's box_iou,
  with the package's tie rule (equal IoU: the lower label index, then the lower detection index).  Where no two
  competing pairs have equal IoU - `tie_free` - the reference's result does not depend on how its argsort orders
  ties, and this restatement equals it; test_confusion_host.py pins that on tests/golden/confusion.pt.
* `update_np`: the batch form on letterboxed inputs (scale_coords / xywh2xyxy as test.py:170 and :213-214).
* `host_path`: the reference's own path on torch tensors wherever they live - box_iou on their device, then the
  `.cpu().numpy()` read and the numpy / Python matching of metrics.py:132-155, once per image.
* `output_to_target_np`: plots.py:105-112.
"""
from __future__ import annotations

import numpy as np
import torch

import metrics_ref as MR


def _pairs(det, labels, conf, iou_thres):
    """Kept detections, and the candidate pairs (label, detection, iou) with iou > iou_thres (metrics.py:127-132)."""
    det = np.asarray(det, np.float32).reshape(-1, 6)
    labels = np.asarray(labels, np.float32).reshape(-1, 5)
    det = det[det[:, 4] > np.float32(conf)]
    iou = MR._iou_np(labels[:, 1:], det[:, :4])
    li, di = np.nonzero(iou > np.float32(iou_thres))
    return det, labels, li, di, iou[li, di]


def tie_free(det, labels, conf=0.25, iou_thres=0.45) -> bool:
    """No two candidate pairs that share a detection, or share a label, have the same IoU."""
    _, _, li, di, v = _pairs(det, labels, conf, iou_thres)
    for key in (di, li):
        o = np.lexsort((v, key))
        k, s = key[o], v[o]
        if np.any((k[1:] == k[:-1]) & (s[1:] == s[:-1])):
            return False
    return True


def process_batch_np(matrix, det, labels, nc, conf=0.25, iou_thres=0.45) -> None:
    """Adds one image into matrix ((nc+1, nc+1) int64)."""
    det, labels, li, di, v = _pairs(det, labels, conf, iou_thres)
    gc, dc = labels[:, 0].astype(np.int64), det[:, 5].astype(np.int64)
    for per_detection in (True, False):        # metrics.py:136-139: per detection, then per label among the survivors
        o = np.lexsort((di, li, -v))           # descending IoU, then label, then detection
        li, di, v = li[o], di[o], v[o]
        first = np.unique(di if per_detection else li, return_index=True)[1]
        li, di, v = li[first], di[first], v[first]
    hit = np.zeros(len(gc), bool)
    hit[li] = True
    np.add.at(matrix, (gc[li], dc[di]), 1)                     # metrics.py:148
    np.add.at(matrix, (np.full((~hit).sum(), nc), gc[~hit]), 1)   # metrics.py:150
    if len(li):                                                # metrics.py:152
        lost = np.ones(len(dc), bool)
        lost[di] = False
        np.add.at(matrix, (dc[lost], np.full(lost.sum(), nc)), 1)


def native_boxes(det_b, labels_b, geom_b):
    """One image of a letterboxed batch in native pixels: predn (n, 6) and [cls x1 y1 x2 y2] (test.py:170, :213-216)."""
    det_b = np.asarray(det_b, np.float32).reshape(-1, 6)
    lab = np.asarray(labels_b, np.float32).reshape(-1, 5)     # [cls x y w h]
    predn = det_b.copy()
    predn[:, :4] = MR._scale_np(det_b[:, :4], geom_b)
    hw, hh = lab[:, 3] / np.float32(2), lab[:, 4] / np.float32(2)
    tbox = MR._scale_np(np.stack([lab[:, 1] - hw, lab[:, 2] - hh, lab[:, 1] + hw, lab[:, 2] + hh], 1), geom_b)
    return predn, np.concatenate([lab[:, :1], tbox], 1)


def update_np(matrix, dets, targets, geom, nc, conf=0.25, iou_thres=0.45, check_ties=False) -> bool:
    """dets: list of (n_i, 6); targets (nt, 6) [img cls x y w h]; geom (B, 5).  Returns tie_free over all images."""
    targets = np.asarray(targets, np.float32).reshape(-1, 6)
    ok = True
    for b, d in enumerate(dets):
        predn, lab = native_boxes(d, targets[targets[:, 0] == b, 1:], geom[b])
        if check_ties:
            ok = ok and tie_free(predn, lab, conf, iou_thres)
        process_batch_np(matrix, predn, lab, nc, conf, iou_thres)
    return ok


def host_path(matrix, detections, labels, nc, conf=0.25, iou_thres=0.45) -> None:
    """process_batch as the reference runs it: box_iou and torch.where on the tensors' device, one .cpu().numpy() per
    image, the reduction in numpy and the counting in Python loops (metrics.py:127-155).  matrix: numpy (nc+1, nc+1)."""
    detections = detections[detections[:, 4] > conf]
    gt_classes = labels[:, 0].int()
    detection_classes = detections[:, 5].int()
    a, b = labels[:, 1:], detections[:, :4]
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(0).prod(2)
    iou = inter / (a1[:, None] + a2 - inter)
    x = torch.where(iou > iou_thres)
    if x[0].shape[0]:
        m = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
        if x[0].shape[0] > 1:
            m = m[np.lexsort((m[:, 1], m[:, 0], -m[:, 2]))]
            m = m[np.unique(m[:, 1], return_index=True)[1]]
            m = m[np.lexsort((m[:, 1], m[:, 0], -m[:, 2]))]
            m = m[np.unique(m[:, 0], return_index=True)[1]]
    else:
        m = np.zeros((0, 3))
    n = m.shape[0] > 0
    m0, m1, _ = m.transpose().astype(np.int32)
    for i, gc in enumerate(gt_classes):
        j = m0 == i
        if n and sum(j) == 1:
            matrix[gc, detection_classes[m1[j]]] += 1
        else:
            matrix[nc, gc] += 1
    if n:
        for i, dc in enumerate(detection_classes):
            if not any(m1 == i):
                matrix[dc, nc] += 1


def output_to_target_np(output):
    """plots.py:105-112 with xyxy2xywh (general.py:259-266) in f32; an empty list of boxes gives shape (0, 7)."""
    rows = []
    for i, o in enumerate(output):
        for *box, conf, cls in np.asarray(o, np.float32).reshape(-1, 6):
            x1, y1, x2, y2 = box
            rows.append([np.float32(i), cls, (x1 + x2) / np.float32(2), (y1 + y2) / np.float32(2), x2 - x1, y2 - y1, conf])
    return np.asarray(rows, np.float32).reshape(-1, 7)
