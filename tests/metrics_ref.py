"""Host restatements of the reference's validation statistics, used as yardsticks by test_metrics_host.py,
test_metrics_gpu.py and tools/mb_metrics.py.

* `match_np`: test.py:155-240 (scale_coords, xywh2xyxy, box_iou, the greedy per-class walk) in numpy f32.
* `ap_per_class_np`: metrics.py:18-106 in numpy; `stable=True` breaks confidence ties by row order.
* `host_loop` / `host_results`: the reference's loop as test.py writes it - per image, per class, per candidate,
  with the .tolist() / .item() / .cpu() reads - on torch tensors wherever they live, then the reference's means.
"""
from __future__ import annotations

import numpy as np
import torch

NIOU = 10
_trapz = getattr(np, "trapezoid", None) or np.trapz


def iouv_np() -> np.ndarray:
    return torch.linspace(0.5, 0.95, NIOU).numpy()


def geometry(img_hw, shape):
    """scale_coords' (h0, w0, gain, padw, padh) for one image (general.py:323-330), f64."""
    h1, w1 = img_hw
    (h0, w0), rp = shape
    if rp is None:
        gain = min(h1 / h0, w1 / w0)
        return h0, w0, gain, (w1 - w0 * gain) / 2, (h1 - h0 * gain) / 2
    return h0, w0, rp[0][0], rp[1][0], rp[1][1]


def _scale_np(b, g):
    h0, w0, gain, pw, ph = (np.float32(v) for v in g)
    b = b.astype(np.float32).copy()
    b[:, [0, 2]] -= pw
    b[:, [1, 3]] -= ph
    b[:, :4] /= gain
    b[:, [0, 2]] = np.minimum(np.maximum(b[:, [0, 2]], np.float32(0)), w0)
    b[:, [1, 3]] = np.minimum(np.maximum(b[:, [1, 3]], np.float32(0)), h0)
    return b


def _iou_np(a, b):
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), np.float32(0))
    h = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), np.float32(0))
    inter = w * h
    return inter / ((a1[:, None] + a2[None, :]) - inter)


def match_np(det, det_off, targets, geom, iouv):
    """Returns (correct uint8 (n_det, 10), tcls f64 in image order) for one batch; geom rows in f64 or f32."""
    det, targets = np.asarray(det, np.float32), np.asarray(targets, np.float32)
    correct = np.zeros((det.shape[0], NIOU), np.uint8)
    tcls = []
    for b in range(len(det_off) - 1):
        pred = det[det_off[b]:det_off[b + 1]]
        labels = targets[targets[:, 0] == b, 1:]
        nl = len(labels)
        tcls.extend(labels[:, 0].tolist())
        if len(pred) == 0 or nl == 0:
            continue
        predn = _scale_np(pred[:, :4], geom[b])
        half_w, half_h = labels[:, 3] / np.float32(2), labels[:, 4] / np.float32(2)
        tbox = np.stack([labels[:, 1] - half_w, labels[:, 2] - half_h, labels[:, 1] + half_w, labels[:, 2] + half_h], 1)
        tbox = _scale_np(tbox, geom[b])
        cor = correct[det_off[b]:det_off[b + 1]]
        for cls in np.unique(labels[:, 0]):
            ti = np.nonzero(labels[:, 0] == cls)[0]
            pi = np.nonzero(pred[:, 5] == cls)[0]
            if not len(pi):
                continue
            iou = _iou_np(predn[pi], tbox[ti])
            best, arg = iou.max(1), iou.argmax(1)        # argmax: the first maximum
            taken = set()
            for j in np.nonzero(best > iouv[0])[0]:
                d = ti[arg[j]]
                if d not in taken:
                    taken.add(d)
                    cor[pi[j]] = best[j] > iouv
    return correct, np.asarray(tcls, np.float64)


def _compute_ap(recall, precision):
    mrec = np.concatenate(([0.], recall, [recall[-1] + 0.01]))
    mpre = np.concatenate(([1.], precision, [0.]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    return _trapz(np.interp(x, mrec, mpre), x)


def ap_per_class_np(tp, conf, pred_cls, target_cls, stable=True):
    """metrics.py:18-78 restated; returns (p, r, ap, f1, classes int32)."""
    tp = np.asarray(tp).astype(np.int64)
    conf, pred_cls, target_cls = np.asarray(conf), np.asarray(pred_cls), np.asarray(target_cls)
    i = np.argsort(-conf, kind="stable" if stable else "quicksort")
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nc = unique_classes.shape[0]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = (target_cls == c).sum()
        n_p = i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + 1e-16)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j] = _compute_ap(recall[:, j], precision[:, j])
    f1 = 2 * p * r / (p + r + 1e-16)
    i = f1.mean(0).argmax()
    return p[:, i], r[:, i], ap, f1[:, i], unique_classes.astype("int32")


def host_loop(out, targets, img_hw, shapes, stats, iouv):
    """test.py:155-240 for one batch, written the way the reference writes it (torch on the tensors' device, one
    Python iteration per image / class / candidate).  Appends (correct, conf, pcls, tcls) per image to `stats`."""
    dev = targets.device
    h1, w1 = img_hw
    for si, pred in enumerate(out):
        labels = targets[targets[:, 0] == si, 1:]
        nl = len(labels)
        tcls = labels[:, 0].tolist() if nl else []
        if len(pred) == 0:
            if nl:
                stats.append((torch.zeros(0, NIOU, dtype=torch.bool), torch.Tensor(), torch.Tensor(), tcls))
            continue
        h0, w0, gain, pw, ph = geometry((h1, w1), shapes[si])

        def scale(c):
            c[:, [0, 2]] -= pw
            c[:, [1, 3]] -= ph
            c[:, :4] /= gain
            c[:, 0].clamp_(0, w0)
            c[:, 1].clamp_(0, h0)
            c[:, 2].clamp_(0, w0)
            c[:, 3].clamp_(0, h0)
            return c
        predn = scale(pred.clone())
        correct = torch.zeros(pred.shape[0], NIOU, dtype=torch.bool, device=dev)
        if nl:
            detected = []
            tcls_tensor = labels[:, 0]
            xy, wh = labels[:, 1:3], labels[:, 3:5]
            tbox = scale(torch.cat((xy - wh / 2, xy + wh / 2), 1))
            for cls in torch.unique(tcls_tensor):
                ti = (cls == tcls_tensor).nonzero(as_tuple=False).view(-1)
                pi = (cls == pred[:, 5]).nonzero(as_tuple=False).view(-1)
                if pi.shape[0]:
                    a, b = predn[pi, :4], tbox[ti]
                    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
                    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
                    inter = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(0).prod(2)
                    ious, i = (inter / (a1[:, None] + a2 - inter)).max(1)
                    detected_set = set()
                    for j in (ious > iouv[0]).nonzero(as_tuple=False):
                        d = ti[i[j]]
                        if d.item() not in detected_set:
                            detected_set.add(d.item())
                            detected.append(d)
                            correct[pi[j]] = ious[j] > iouv
                            if len(detected) == nl:
                                break
        stats.append((correct.cpu(), pred[:, 4].cpu(), pred[:, 5].cpu(), tcls))


def host_results(stats, nc, stable=True):
    """test.py:255-262 and :343-346 on the collected stats: (mp, mr, map50, map, maps)."""
    stats = [np.concatenate(x, 0) for x in zip(*stats)]
    mp = mr = map50 = map_ = 0.0
    ap_class = []
    if len(stats) and stats[0].any():
        p, r, ap, f1, ap_class = ap_per_class_np(*stats, stable=stable)
        ap50, ap = ap[:, 0], ap.mean(1)
        mp, mr, map50, map_ = p.mean(), r.mean(), ap50.mean(), ap.mean()
    maps = np.zeros(nc) + map_
    for i, c in enumerate(ap_class):
        maps[c] = ap[i]
    return mp, mr, map50, map_, maps
