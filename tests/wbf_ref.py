"""numpy restatement of the reference's weighted boxes fusion, shared by tests/test_wbf_host.py (which pins it to
tests/golden/wbf.pt, the reference's own results), tests/test_wbf_gpu.py and tools/mb_wbf.py.

What it restates: `weighted_boxes` (basics/utils/general.py:515-563) and `weighted_boxes_fusion`
(basics/utils/ensemble_boxes/ensemble_boxes_wbf.py:150-225) with the number formats the reference actually uses:
  * the weighted score is the float64 product of the float32 score and the float64 model weight;
  * a cluster of one member is the candidate's float64 row; a fused cluster is get_weighted_box's float32 row: float32
    coordinate sums updated through float64 (`f32 += f64` rounds each add), the score sum in float64, the fused
    coordinate float32(float64(acc) / sum);
  * in the confidence rescaling a float32 score times a Python int stays float32, anything touching a float64 is float64.
The IoU of two boxes is evaluated in float64 from their float32 coordinates.

Two orders the reference leaves to an unstable argsort are fixed here as the device code fixes them: candidates are
walked by label, then descending weighted score, then ascending source index; clusters come out by descending score,
then label, then creation order.  The fixtures hold no such ties, so on them both rules agree with the reference.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
CONF_TYPES = ("avg", "max", "box_and_model_avg", "absent_model_aware_avg")


def iou_many(A, b):
    """bb_intersection_over_union (:11-28) of every row of A (k, 4) with b (4,), float64; zero intersection -> 0.0."""
    A = A.astype(F64)
    b = b.astype(F64)
    inter = np.maximum(0.0, np.minimum(A[:, 2], b[2]) - np.maximum(A[:, 0], b[0])) * \
        np.maximum(0.0, np.minimum(A[:, 3], b[3]) - np.maximum(A[:, 1], b[1]))
    aa = (A[:, 2] - A[:, 0]) * (A[:, 3] - A[:, 1])
    ab = (b[2] - b[0]) * (b[3] - b[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        v = inter / (aa + ab - inter)
    return np.where(inter == 0.0, 0.0, v)


def _confidence(conf_type, allows_overflow, weights, n, ssum, smax, wsum, models):
    """:196-218 for one cluster; returns a float64 (a fused cluster's value has been rounded to float32)."""
    W = weights.sum()
    present = np.unique(np.asarray(models))
    mask = np.ones(len(weights), dtype=bool)
    mask[present] = False
    if n == 1:
        s, w = F64(ssum), F64(wsum)
        if conf_type == "box_and_model_avg":
            return F64(s * n / w * weights[present].sum() / W)
        if conf_type == "absent_model_aware_avg":
            return F64(s * n / (w + weights[mask].sum()))
        if not allows_overflow:
            return F64(s * n / W) if n < W else F64(s * W / W)
        return F64(s * n / W)
    s = F32(smax) if conf_type == "max" else F32(F64(ssum) / n)
    w = F32(wsum)
    sn = F32(s * F32(n))
    if conf_type == "box_and_model_avg":
        t = F32(sn / w)
        return F64(F32(F64(t) * weights[present].sum() / W))
    if conf_type == "absent_model_aware_avg":
        return F64(F32(F64(sn) / (F64(w) + weights[mask].sum())))
    if not allows_overflow and not n < W:
        return F64(F32(F64(s) * W / W))
    return F64(F32(F64(sn) / W))


def fuse(boxes, scores, labels, models=None, weights=None, iou_thr=0.55, skip_box_thr=0.0, conf_type="avg",
         allows_overflow=False, src=None, trace=None):
    """One image.  boxes (n, 4) f32 corners, scores (n) f32, labels (n) int, models (n) int (None: model 0), weights: one
    float per model (None: 1.0), src: tie-break index (None: position).
    Returns boxes (m, 4) f32, scores (m) f64, labels (m) int64, member (n) int64 = output row of each input's cluster
    (-1: dropped).  trace (a list) receives (label, matched cluster index within the label or -1) per walked candidate."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    scores = np.asarray(scores, F32).reshape(-1)
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    n = len(scores)
    models = np.zeros(n, np.int64) if models is None else np.asarray(models).astype(np.int64).reshape(-1)
    weights = np.ones(int(models.max()) + 1 if n else 1) if weights is None else np.asarray(weights, F64)
    src = np.arange(n) if src is None else np.asarray(src).astype(np.int64)
    assert conf_type in CONF_TYPES
    ws = scores.astype(F64) * weights[models]
    keep = np.nonzero(~(scores < F32(skip_box_thr)))[0]
    order = keep[np.lexsort((src[keep], -ws[keep], labels[keep]))]
    cl = []                                              # [label, creation, score, box]
    slot_of = np.full(n, -1, np.int64)
    p = 0
    while p < len(order):
        lab = labels[order[p]]
        e = p
        while e < len(order) and labels[order[e]] == lab:
            e += 1
        seg = order[p:e]
        k = 0
        cbox = np.zeros((len(seg), 4), F32)
        acc = np.zeros((len(seg), 4), F32)
        ssum = np.zeros(len(seg), F64)
        wsum = np.zeros(len(seg), F64)
        smax = np.zeros(len(seg), F64)
        members = [[] for _ in seg]
        for j in seg:
            c, s = boxes[j], ws[j]
            bi = -1
            if k:
                v = iou_many(cbox[:k], c)
                m = int(np.argmax(v))                    # the first maximum: the lowest cluster index
                if v[m] > iou_thr:
                    bi = m
            if trace is not None:
                trace.append((int(lab), bi))
            if bi < 0:
                bi = k
                k += 1
                cbox[bi] = c
            acc[bi] = (acc[bi].astype(F64) + s * c.astype(F64)).astype(F32)
            ssum[bi] += s
            wsum[bi] += weights[models[j]]
            smax[bi] = s if not members[bi] else max(smax[bi], s)
            members[bi].append(j)
            if len(members[bi]) > 1:
                cbox[bi] = (acc[bi].astype(F64) / ssum[bi]).astype(F32)
        for q in range(k):
            conf = _confidence(conf_type, allows_overflow, weights, len(members[q]), ssum[q], smax[q], wsum[q],
                               models[members[q]])
            slot_of[members[q]] = len(cl)
            cl.append((lab, q, conf, cbox[q].copy()))
        p = e
    if not cl:
        return np.zeros((0, 4), F32), np.zeros(0, F64), np.zeros(0, np.int64), slot_of
    sc = np.array([c[2] for c in cl], F64)
    out = np.lexsort((np.array([c[1] for c in cl]), np.array([c[0] for c in cl]), -sc))
    rank = np.empty(len(cl), np.int64)
    rank[out] = np.arange(len(cl))
    member = np.where(slot_of >= 0, rank[np.maximum(slot_of, 0)], -1)
    return (np.stack([cl[i][3] for i in out]), sc[out], np.array([cl[i][0] for i in out], np.int64), member)


def candidates(z, conf_thres, image_size):
    """general.py:523-544 for one image z (N, 5+nc) f32: boxes (n, 4) f32 normalised corners, scores, labels, rows."""
    z = np.asarray(z, F32)
    conf, S = F32(conf_thres), F32(image_size)
    rows = np.nonzero(z[:, 4] > conf)[0]
    x = z[rows]
    cls = x[:, 5:] * x[:, 4:5]
    lab = np.argmax(cls, 1) if len(x) else np.zeros(0, np.int64)
    sc = cls[np.arange(len(x)), lab] if len(x) else np.zeros(0, F32)
    cx, cy, w, h = (x[:, i] / S for i in range(4))
    box = np.stack([cx - w / F32(2), cy - h / F32(2), cx + w / F32(2), cy + h / F32(2)], 1).astype(F32)
    k = sc > conf
    return box[k], sc[k], lab[k], rows[k]


def weighted_boxes(prediction, image_size, conf_thres=0.25, iou_thres=0.45, xyxy=False, trace=None):
    """general.py:515-563.  Returns per image ((n, 6) f32 [cx cy w h conf cls] in pixels - corners with xyxy=True -,
    member (N) int64: the output row each prediction row went into, -1 for none)."""
    out = []
    for z in np.asarray(prediction, F32):
        box, sc, lab, rows = candidates(z, conf_thres, image_size)
        b, s, l, m = fuse(box, sc, lab, iou_thr=iou_thres, skip_box_thr=0, src=rows, trace=trace)
        b = b.astype(F64)
        if not xyxy:                                     # general.py:552-554, numpy float64
            b = np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
        b = b * image_size
        member = np.full(len(z), -1, np.int64)
        member[rows] = m
        out.append((np.concatenate([b, s[:, None], l[:, None].astype(F64)], 1).astype(F32).reshape(-1, 6), member))
    return out


def by_label(trace):
    """{label: [decision, ...]} of a trace in walk order (the reference walks labels in first-seen order, this file in
    ascending order; within a label the order is the same)."""
    out = {}
    for lab, bi in trace:
        out.setdefault(int(lab), []).append(int(bi))
    return out
