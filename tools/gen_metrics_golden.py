"""Write tests/golden/metrics.pt: the validation statistics of test.py:155-264 computed by the reference's own
helpers on hand-built batches.  Runs only where the reference source tree is importable (the build machine); it
reads oracle.gen_golden.import_reference() for the module stubs and changes nothing under oracle/.

The reference's `ap_per_class`, `box_iou`, `scale_coords` and `xywh2xyxy` are called as they are.  The matching
loop sits inline in `test()` (test.py:155-240), which cannot be called without a model and a data loader, so its
control flow is restated below on top of those helpers, line for line.

Every case uses distinct confidences: the reference sorts with np.argsort(-conf), which is not stable, so tied
confidences have no defined order there.

usage: python tools/gen_metrics_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics.pt")
IMG = (640, 640)


def letterbox_shape(h0, w0, img_hw=IMG):
    """The loader's shapes[si] for a rect letterbox into img_hw: ((h0, w0), ((h / h0, w / w0), (padw, padh)))."""
    r = min(img_hw[0] / h0, img_hw[1] / w0)
    h, w = int(round(h0 * r)), int(round(w0 * r))
    return (h0, w0), ((h / h0, w / w0), ((img_hw[1] - w) / 2, (img_hw[0] - h) / 2))


def shifted(box, iou):
    """box moved right so that its IoU with box is `iou` (same size)."""
    x1, y1, x2, y2 = box
    dx = (x2 - x1) * (1 - iou) / (1 + iou)
    return [x1 + dx, y1, x2 + dx, y2]


def xyxy_to_label(cls, b):
    return [cls, (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, b[2] - b[0], b[3] - b[1]]


class Case:
    def __init__(self, tag, nc, seed):
        self.tag, self.nc, self.rng = tag, nc, np.random.default_rng(seed)
        self.shapes, self.preds, self.labels = [], [], []

    def image(self, shape, labels=(), preds=()):
        """labels: [cls, x1, y1, x2, y2]; preds: [x1, y1, x2, y2, cls] (confidence assigned later), input pixels."""
        self.shapes.append(shape)
        b = len(self.shapes) - 1
        self.labels += [[b] + xyxy_to_label(l[0], l[1:5]) for l in labels]
        self.preds.append([list(p) for p in preds])
        return b

    def finish(self, sort_rows=True, extra_targets=()):
        n = sum(len(p) for p in self.preds)
        conf = (0.02 + 0.96 * self.rng.permutation(n) / max(n, 1)).astype(np.float32)   # distinct
        det, k = [], 0
        for p in self.preds:
            rows = [[*q[:4], conf[k + j], q[4]] for j, q in enumerate(p)]
            k += len(p)
            if sort_rows:
                rows.sort(key=lambda r: -r[4])                 # NMS output order
            det.append(torch.tensor(rows, dtype=torch.float32).view(-1, 6))
        tg = torch.tensor(self.labels + [list(t) for t in extra_targets], dtype=torch.float32).view(-1, 6)
        tg = tg[torch.from_numpy(self.rng.permutation(len(tg)))]   # targets in no particular image order
        return det, tg


def reference_stats(G, det, targets, img_hw, shapes, iouv):
    """test.py:155-240 restated on the reference's helpers (CPU tensors)."""
    stats = []
    niou = iouv.numel()
    for si, pred in enumerate(det):
        labels = targets[targets[:, 0] == si, 1:]
        nl = len(labels)
        tcls = labels[:, 0].tolist() if nl else []
        if len(pred) == 0:
            if nl:
                stats.append((torch.zeros(0, niou, dtype=torch.bool), torch.Tensor(), torch.Tensor(), tcls))
            continue
        predn = pred.clone()
        G.scale_coords(img_hw, predn[:, :4], shapes[si][0], shapes[si][1])
        correct = torch.zeros(pred.shape[0], niou, dtype=torch.bool)
        if nl:
            detected = []
            tcls_tensor = labels[:, 0]
            tbox = G.xywh2xyxy(labels[:, 1:5])
            G.scale_coords(img_hw, tbox, shapes[si][0], shapes[si][1])
            for cls in torch.unique(tcls_tensor):
                ti = (cls == tcls_tensor).nonzero(as_tuple=False).view(-1)
                pi = (cls == pred[:, 5]).nonzero(as_tuple=False).view(-1)
                if pi.shape[0]:
                    ious, i = G.box_iou(predn[pi, :4], tbox[ti]).max(1)
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
    return stats


def geometry(img_hw, shape):
    (h0, w0), rp = shape
    if rp is None:
        gain = min(img_hw[0] / h0, img_hw[1] / w0)
        return [h0, w0, gain, (img_hw[1] - w0 * gain) / 2, (img_hw[0] - h0 * gain) / 2]
    return [h0, w0, rp[0][0], rp[1][0], rp[1][1]]


def random_boxes(rng, n, lo, hi, smin=8, smax=80):
    xy = rng.uniform(lo, hi, (n, 2))
    wh = rng.uniform(smin, smax, (n, 2))
    return np.concatenate([xy, xy + wh], 1)


def jitter(rng, b, s):
    return [v + rng.normal(0, s) for v in b]


def build_cases():
    cases = []
    # 1. letterbox ratio_pad geometry, labels and predictions running into the padding (clipped at the image border)
    c = Case("letterbox_clip", 3, 1)
    for h0, w0 in ((375, 500), (500, 333), (480, 640)):
        sh = letterbox_shape(h0, w0)
        (_, _), (_, (pw, ph)) = sh
        x_hi, y_hi = IMG[1] - pw, IMG[0] - ph
        labs = [[0, pw - 6, ph + 20, pw + 40, ph + 70], [1, x_hi - 50, y_hi - 30, x_hi + 9, y_hi + 4],
                [2, 200, 200, 260, 250], [1, pw + 100, ph - 3, pw + 160, ph + 40]]
        preds = []
        for l in labs:
            preds.append(jitter(c.rng, l[1:5], 2.0) + [l[0]])
            preds.append(jitter(c.rng, l[1:5], 9.0) + [l[0]])
        preds.append([x_hi - 20, y_hi - 20, x_hi + 15, y_hi + 12, 2])
        c.image(sh, labs, preds)
    cases.append((c, c.finish()))

    # 2. IoUs straddling each of the 10 thresholds (one target per prediction, two classes)
    c = Case("iou_straddle", 2, 2)
    labs, preds = [], []
    for k, t in enumerate(np.linspace(0.5, 0.95, 10)):
        for s, d in enumerate((-0.004, 0.004)):
            x0, y0 = 20 + 60 * k, 40 + 200 * s
            box = [x0, y0, x0 + 48, y0 + 64]
            cls = (k + s) % 2
            labs.append([cls] + box)
            preds.append(shifted(box, t + d) + [cls])
    c.image(letterbox_shape(427, 640), labs, preds)
    cases.append((c, c.finish()))

    # 3. duplicates of an already matched target (false positives), also with rows NOT in confidence order
    for sort_rows in (True, False):
        c = Case("duplicate" + ("" if sort_rows else "_row_order"), 2, 3 + sort_rows)
        box = [100, 100, 180, 160]
        box2 = [300, 300, 340, 380]
        c.image(((640, 640), ((1.0, 1.0), (0.0, 0.0))), [[0] + box, [1] + box2],
                [shifted(box, 0.9) + [0], shifted(box, 0.75) + [0], shifted(box, 0.6) + [0], shifted(box, 0.3) + [0],
                 shifted(box2, 0.8) + [1], shifted(box2, 0.97) + [1]])
        cases.append((c, c.finish(sort_rows=sort_rows)))

    # 4. a prediction exactly as close to two targets (gain 0.5, no pad: exact arithmetic) -> the lower target index
    c = Case("equidistant", 1, 5)
    c.image(((1280, 1280), ((0.5, 0.5), (0.0, 0.0))), [[0, 100, 100, 124, 120], [0, 116, 100, 140, 120]],
            [[100, 100, 140, 120, 0], [100, 100, 140, 120, 0], [400, 400, 420, 420, 0]])
    cases.append((c, c.finish()))

    # 5. a class only in predictions (3) and a class only in labels (2)
    c = Case("class_only_pred_or_label", 4, 6)
    for _ in range(2):
        boxes = random_boxes(c.rng, 6, 50, 500)
        labs = [[int(k % 3)] + list(b) for k, b in enumerate(boxes)]
        preds = [jitter(c.rng, l[1:5], 3.0) + [l[0]] for l in labs if l[0] != 2]
        preds += [list(b) + [3] for b in random_boxes(c.rng, 3, 50, 500)]
        c.image(letterbox_shape(512, 640), labs, preds)
    cases.append((c, c.finish()))

    # 6. images with labels and no predictions, predictions and no labels, neither; a target row of no image
    c = Case("empty_images", 3, 7)
    boxes = random_boxes(c.rng, 8, 60, 400)
    c.image(letterbox_shape(600, 640), [[k % 3] + list(b) for k, b in enumerate(boxes[:3])], [])
    c.image(letterbox_shape(640, 480), [], [list(b) + [1] for b in boxes[3:6]])
    c.image(letterbox_shape(640, 640), [], [])
    labs = [[k % 3] + list(b) for k, b in enumerate(boxes[5:])]
    c.image(((320, 320), None), labs, [jitter(c.rng, l[1:5], 2.0) + [l[0]] for l in labs])
    cases.append((c, c.finish(extra_targets=[[4, 1, 200, 200, 30, 30]])))   # image 4 is not in the batch

    # 7. nc == 1
    c = Case("nc1", 1, 8)
    for h0, w0 in ((360, 640), (640, 640)):
        boxes = random_boxes(c.rng, 12, 40, 500)
        labs = [[0] + list(b) for b in boxes]
        preds = [jitter(c.rng, l[1:5], 4.0) + [0] for l in labs[:10]] + [list(b) + [0] for b in random_boxes(c.rng, 4, 40, 500)]
        c.image(letterbox_shape(h0, w0), labs, preds)
    cases.append((c, c.finish()))

    # 8. a larger random batch: 8 classes, some images without ratio_pad
    c = Case("random", 8, 9)
    for b in range(6):
        h0, w0 = int(c.rng.integers(300, 900)), int(c.rng.integers(300, 900))
        sh = letterbox_shape(h0, w0) if b % 3 else ((h0, w0), None)
        boxes = random_boxes(c.rng, int(c.rng.integers(5, 25)), 0, 600)
        labs = [[int(c.rng.integers(0, 8))] + list(bb) for bb in boxes]
        preds = []
        for l in labs:
            for _ in range(int(c.rng.integers(0, 4))):
                preds.append(jitter(c.rng, l[1:5], float(c.rng.uniform(1, 12))) +
                             [l[0] if c.rng.random() < 0.8 else int(c.rng.integers(0, 8))])
        preds += [list(bb) + [int(c.rng.integers(0, 8))] for bb in random_boxes(c.rng, 15, 0, 600)]
        c.image(sh, labs, preds)
    cases.append((c, c.finish()))
    return cases


def main():
    import_reference()
    G = importlib.import_module("reference.basics.utils.general")
    M = importlib.import_module("reference.basics.utils.metrics")
    iouv = torch.linspace(0.5, 0.95, 10)
    out = []
    for c, (det, tg) in build_cases():
        stats = reference_stats(G, det, tg.clone(), IMG, c.shapes, iouv)
        st = [np.concatenate(x, 0) for x in zip(*stats)]
        assert st[0].any() and len(np.unique(st[1])) == len(st[1]), c.tag
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)          # np.trapz
            p, r, ap, f1, ap_class = M.ap_per_class(*st, plot=False)
        correct = torch.from_numpy(st[0]).to(torch.uint8)     # images without predictions add no rows
        off = np.zeros(len(det) + 1, dtype=np.int32)
        np.cumsum([len(d) for d in det], out=off[1:])
        rp = torch.tensor([[*s[1][0], *s[1][1]] if s[1] is not None else [0.0] * 4 for s in c.shapes], dtype=torch.float64)
        out.append(dict(
            tag=c.tag, nc=c.nc, img_hw=torch.tensor(IMG),
            det=torch.cat(det), det_off=torch.from_numpy(off), targets=tg,
            h0w0=torch.tensor([s[0] for s in c.shapes], dtype=torch.int64), ratio_pad=rp,
            rp_none=torch.tensor([s[1] is None for s in c.shapes]),
            geom=torch.tensor([geometry(IMG, s) for s in c.shapes], dtype=torch.float64),
            correct=correct, tcls=torch.from_numpy(st[3]),
            p=torch.from_numpy(p.copy()), r=torch.from_numpy(r.copy()), f1=torch.from_numpy(f1.copy()), ap=torch.from_numpy(ap.copy()),
            ap_class=torch.from_numpy(ap_class), nt=torch.from_numpy(np.bincount(st[3].astype(np.int64), minlength=c.nc))))
        print(f"[metrics golden] {c.tag}: {len(det)} images, {int(off[-1])} detections, {len(tg)} targets, "
              f"{int(correct.sum())} true entries, ap_class {ap_class.tolist()}")
    assert len(correct) == int(off[-1])
    torch.save(out, OUT)
    print(f"[metrics golden] wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
