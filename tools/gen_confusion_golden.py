"""Write tests/golden/confusion.pt: the reference's own ConfusionMatrix (basics/utils/metrics.py:109-158) run on
hand-built and random images.  Runs only where the reference source tree is importable (the build machine); it reads
oracle.gen_golden.import_reference() for the module stubs, as tools/gen_metrics_golden.py does, and changes nothing
under oracle/.

The fixture holds inputs and results only: per case nc, conf, iou_thres, the images as (detections (N, 6)
[x1 y1 x2 y2 conf cls], labels (M, 5) [cls x1 y1 x2 y2]) in native pixels - process_batch's arguments - and the
matrix the reference holds after all of them.

Condition on every image: no two candidate pairs that share a detection or a label have the same IoU.  The reference
orders pairs with a plain argsort, which is not stable, so among equal IoUs its winner is unspecified.  The random cases
are redrawn with the next seed until the condition holds; the hand-built ones assert it.

usage: python tools/gen_confusion_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import confusion_ref as CR  # noqa: E402
from gen_metrics_golden import jitter, random_boxes, shifted  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "confusion.pt")
F = np.float32


def up(v, k=1):
    """The float32 k steps above (below for k < 0) v."""
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf if k > 0 else -np.inf))
    return float(v)


def random_image(rng, nc, n_lab, miss=0.2, wrong=0.2, extra=6):
    """Labels with up to 3 jittered detections each (some of another class), plus stray detections."""
    boxes = random_boxes(rng, n_lab, 0, 900)
    labels = [[int(rng.integers(0, nc))] + list(b) for b in boxes]
    dets = []
    for l in labels:
        if rng.random() < miss:
            continue
        for _ in range(int(rng.integers(1, 4))):
            cls = l[0] if rng.random() > wrong else int(rng.integers(0, nc))
            dets.append(jitter(rng, l[1:5], float(rng.uniform(0.5, 10))) + [float(rng.uniform(0.05, 0.99)), cls])
    dets += [list(b) + [float(rng.uniform(0.05, 0.99)), int(rng.integers(0, nc))] for b in random_boxes(rng, extra, 0, 900)]
    rng.shuffle(dets)
    return dets, labels


def iou_at(G, value, rng):
    """A (label, detection) pair of boxes whose float32 box_iou is exactly `value`: a detection (0, 0, w, h) inside a
    label (0, 0, W, H) with w h / (W H) near value, drawn until the reference's box_iou hits it."""
    for _ in range(200):
        W, H, h = (rng.uniform(40, 200, 20000).astype(F) for _ in range(3))
        h = np.minimum(h, H)
        w = (F(value) * W * H / h * rng.uniform(1 - 2e-6, 1 + 2e-6, W.size)).astype(F)
        inter = w * h
        hit = np.nonzero((w < W) & (inter / ((W * H + inter) - inter) == F(value)))[0]
        for i in hit:
            lab, det = [0.0, 0.0, float(W[i]), float(H[i])], [0.0, 0.0, float(w[i]), float(h[i])]
            if G.box_iou(torch.tensor([lab]), torch.tensor([det]))[0, 0].numpy() == F(value):
                return lab, det
    raise AssertionError(f"no box pair with IoU {value!r}")


def moved(box, dx, dy):
    return [box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy]


def build_cases(G):
    cases = []

    def case(tag, nc, images, conf=0.25, iou_thres=0.45):
        cases.append(dict(tag=tag, nc=nc, conf=conf, iou_thres=iou_thres, images=images))

    # 1. VEDAI-like: 8 classes, six images into one matrix (matches, wrong classes, misses, strays); redrawn on a tie
    for tag, nc, n_img, n_lab in (("vedai_mix", 8, 6, (10, 40)), ("nc1", 1, 3, (5, 30))):
        seed = 100
        while True:
            rng = np.random.default_rng(seed)
            images = [random_image(rng, nc, int(rng.integers(*n_lab))) for _ in range(n_img)]
            if all(CR.tie_free(np.array(d, F).reshape(-1, 6), np.array(l, F).reshape(-1, 5)) for d, l in images):
                break
            seed += 1
        print(f"[confusion golden] {tag}: seed {seed}")
        case(tag, nc, images)

    box, box2, box3 = [100, 100, 180, 160], [300, 300, 340, 380], [500, 120, 560, 200]
    # 2. labels and no detection above conf (one far below, one exactly at conf); then an image that does match
    case("labels_no_detection_above_conf", 8,
         [([shifted(box, 0.9) + [0.10, 2], shifted(box2, 0.9) + [0.25, 3]], [[2] + box, [3] + box2]),
          ([shifted(box, 0.8) + [0.60, 2]], [[2] + box])])
    # 3. detections and no labels: nothing is counted
    case("detections_no_labels", 8, [([box + [0.9, 1], box2 + [0.8, 5]], []), ([shifted(box, 0.7) + [0.9, 4]], [[4] + box])])
    # 4. every detection misses: the labels count as missed, the detections are NOT counted (metrics.py:152)
    case("all_miss", 8, [([moved(box, 300, 0) + [0.9, 1], moved(box2, -250, 40) + [0.8, 5], shifted(box3, 0.3) + [0.7, 6]],
                          [[1] + box, [5] + box2, [6] + box3])])
    # 5. one detection over two labels: it keeps the closer label, the other label is missed
    two = [100, 100, 200, 160]
    case("detection_over_two_labels", 8,
         [([two + [0.9, 3]], [[3] + shifted(two, 0.62), [4] + moved(two, -(two[2] - two[0]) * (1 - 0.55) / (1 + 0.55), 0)])])
    # 6. two detections on one label: the closer one is the match, the other a background count
    case("two_detections_one_label", 8,
         [([shifted(box, 0.7) + [0.9, 2], shifted(box, 0.85) + [0.5, 2], shifted(box, 0.5) + [0.95, 7]], [[2] + box])])
    # 7. the order of the two reductions: A overlaps L1 (0.8) and L2 (0.6), B overlaps L1 (0.9).  A keeps L1 in the first
    #    pass and loses it to B in the second, so L2 is missed although A overlaps it above the threshold.
    L1 = [200.0, 200.0, 300.0, 260.0]
    A = shifted(L1, 0.8)
    L2 = shifted(A, 0.6)
    B = moved(L1, -100 * (1 - 0.9) / (1 + 0.9), 0)
    case("reduction_order", 8, [([A + [0.9, 1], B + [0.8, 5]], [[1] + L1, [6] + L2])])
    # 8. wrong-class matches land off the diagonal
    case("wrong_class", 8, [([shifted(box, 0.9) + [0.9, 0], shifted(box2, 0.8) + [0.7, 7], shifted(box3, 0.75) + [0.6, 6]],
                             [[1] + box, [2] + box2, [6] + box3])])
    # 9. confidences at conf and one float32 step either side (strict >)
    case("at_conf", 8, [([shifted(box, 0.9) + [0.25, 1], shifted(box2, 0.9) + [up(0.25), 2], shifted(box3, 0.9) + [up(0.25, -1), 3]],
                         [[1] + box, [2] + box2, [3] + box3])])
    # 10. IoUs at float32(iou_thres) and one step either side (strict >), for the default threshold and for 0.6, whose
    #     float32 value lies above the double 0.6
    rng = np.random.default_rng(7)
    for tag, thr in (("iou_ulp", 0.45), ("iou_ulp_06", 0.6)):
        images = []
        for k, step in enumerate((0, 1, -1)):       # one pair per image, at the origin
            lab, det = iou_at(G, up(thr, step) if step else F(thr), rng)
            images.append(([det + [0.9, k]], [[k] + lab]))
        case(tag, 8, images, iou_thres=thr)
    return cases


def main():
    import_reference()
    G = importlib.import_module("reference.basics.utils.general")
    M = importlib.import_module("reference.basics.utils.metrics")
    out = []
    for c in build_cases(G):
        ref = M.ConfusionMatrix(c["nc"], conf=c["conf"], iou_thres=c["iou_thres"])
        images = []
        for dets, labels in c["images"]:
            d = torch.tensor(dets, dtype=torch.float32).view(-1, 6)
            l = torch.tensor(labels, dtype=torch.float32).view(-1, 5)
            assert CR.tie_free(d.numpy(), l.numpy(), c["conf"], c["iou_thres"]), c["tag"]
            ref.process_batch(d.clone(), l.clone())
            images.append((d, l))
        m = torch.from_numpy(ref.matrix.copy())
        assert m.dtype == torch.float64 and torch.equal(m, m.round())
        out.append(dict(tag=c["tag"], nc=c["nc"], conf=c["conf"], iou_thres=c["iou_thres"], images=images,
                        matrix=m.to(torch.int64)))
        print(f"[confusion golden] {c['tag']}: {len(images)} images, {sum(len(d) for d, _ in images)} detections, "
              f"{sum(len(l) for _, l in images)} labels, diagonal {int(m.diagonal()[:-1].sum())}, "
              f"off-diagonal {int(m[:-1, :-1].sum() - m.diagonal()[:-1].sum())}, "
              f"missed {int(m[-1].sum())}, background {int(m[:, -1].sum())}")
    torch.save(out, OUT)
    print(f"[confusion golden] wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
