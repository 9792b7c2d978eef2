"""Write tests/golden/wbf.pt: the reference's own `weighted_boxes` (basics/utils/general.py:515-563) and
`weighted_boxes_fusion` (basics/utils/ensemble_boxes/ensemble_boxes_wbf.py:150-225) run on hand-built and random
inputs.  Runs only where the reference source tree is importable (the build machine); it reads
oracle.gen_golden.import_reference() for the module stubs (numba.jit becomes the identity, which leaves the arithmetic
as it is), as tools/gen_confusion_golden.py does, and changes nothing under oracle/.

The fixture holds inputs and results only:
  weighted_boxes: per case image_size, conf_thres, iou_thres, prediction (B, N, 5+nc) f32 and the reference's list of
      (n, 6) f32 rows - [cx cy w h conf cls] in pixels, whatever its docstring says (general.py:552-554);
  fusion: per group the per-model boxes / scores / labels, weights, iou_thr, skip_box_thr, and per run of the group
      conf_type, allows_overflow and the reference's float64 boxes, scores, labels;
  both: `trace`, the value find_matching_box returned for every candidate, per label in walk order (-1: new cluster).

Conditions on every random case, redrawn with the next seed until they hold (the reference's argsort()[::-1] is not
stable, and its match is a strict comparison):
  * no two candidates of an image have the same weighted score;
  * no two output clusters of an image have the same score (compared after rounding to float32);
  * every nonzero IoU the reference evaluates differs from iou_thr by more than 1e-5.
The hand-built cases sit outside that margin on purpose and use exactly representable numbers:
  exact threshold   A = (0, 0, .5, .25), B = (0, 0, .25, .25): IoU exactly 0.5; no match at iou_thr 0.5, a match one
                    float32 step below it;
  equal IoU         two clusters placed symmetrically around a third candidate: the earlier cluster takes it;
  drift             the sequential dependence.  Chain 1 (fused only): a tall box and a wide box fuse into a squarer one,
                    and a larger square matches that fused box (IoU 0.4443 at iou_thr 0.42) although it matches
                    neither member alone (0.4167 each); all three margins are 4e-3 or more.  Chain 2 (fused, not
                    first): translated boxes, the third matches the fused box and not the box the cluster held
                    before the fusion.  Chain 3 (member only): the third matches that first box, not the fused one,
                    and starts a cluster.
  zero intersection touching boxes: IoU 0.0, no match even at iou_thr 0;
  empty             an image with no candidate gives (0, 6).

usage: python tools/gen_wbf_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "wbf.pt")
F = np.float32
CONF_TYPES = ("avg", "max", "box_and_model_avg", "absent_model_aware_avg")
S = 512


class Recorder:
    """Wraps the reference's bb_intersection_over_union and find_matching_box to see what it evaluates and decides."""

    def __init__(self, E):
        self.E = E
        self.iou0, self.find0 = E.bb_intersection_over_union, E.find_matching_box
        E.bb_intersection_over_union = self.iou
        E.find_matching_box = self.find
        self.reset()

    def reset(self):
        self.ious, self.trace = [], []

    def iou(self, A, B):
        v = self.iou0(A, B)
        if v != 0:
            self.ious.append(float(v))
        return v

    def find(self, boxes_list, new_box, match_iou):
        index, best = self.find0(boxes_list, new_box, match_iou)
        self.trace.append((int(new_box[0]), int(index)))
        return index, best

    def margin(self, thr):
        return min((abs(v - thr) for v in self.ious), default=1.0)

    def take_trace(self):
        t = torch.tensor(self.trace, dtype=torch.int64).view(-1, 2)
        self.reset()
        return t


def objects(rng, n_obj, n_det, nc, spread=0.02):
    """n_obj objects in the unit square, each with 1..n_det jittered detections: boxes (n, 4) f32, labels (n)."""
    boxes, labels = [], []
    for _ in range(n_obj):
        w, h = rng.uniform(0.03, 0.15, 2)
        x, y = rng.uniform(0.0, 1.0 - w), rng.uniform(0.0, 1.0 - h)
        lab = int(rng.integers(0, nc))
        for _ in range(int(rng.integers(1, n_det + 1))):
            j = rng.normal(0, spread, 4) * np.array([w, h, w, h]) * 5
            boxes.append([x + j[0], y + j[1], x + w + j[2], y + h + j[3]])
            labels.append(lab if rng.random() > 0.1 else int(rng.integers(0, nc)))
    return np.array(boxes, F).reshape(-1, 4), np.array(labels, np.int64)


def prediction_from(boxes, scores, labels, nc, extra=None):
    """Decoded rows (N, 5+nc) whose candidate boxes, scores and labels are the given ones: obj = 1, the label's class
    score = the score, every other class lower; `extra` rows are appended as they are."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    z = np.zeros((len(boxes), 5 + nc), F)
    z[:, 0] = (boxes[:, 0] + boxes[:, 2]) / 2 * S
    z[:, 1] = (boxes[:, 1] + boxes[:, 3]) / 2 * S
    z[:, 2] = (boxes[:, 2] - boxes[:, 0]) * S
    z[:, 3] = (boxes[:, 3] - boxes[:, 1]) * S
    z[:, 4] = 1.0
    for i, (s, l) in enumerate(zip(scores, labels)):
        z[i, 5:] = F(s) * F(0.25)
        z[i, 5 + int(l)] = s
    if extra is not None:
        z = np.concatenate([z, extra.astype(F)], 0)
    return z


def shift(b, dx, dy=0.0):
    return [b[0] + dx, b[1] + dy, b[2] + dx, b[3] + dy]


def hand_images():
    """(tag, nc, iou_thres, boxes, scores, labels) of one image each."""
    below = float(np.nextafter(F(0.5), F(0)))
    A, B = [0, 0, .5, .25], [0, 0, .25, .25]
    C = [.25, .25, .5, .5]
    b1 = [.25, .25, .75, .75]
    far = [.875, .875, 1.0, 1.0]
    return [
        ("exact_thr_no_match", 1, 0.5, [A, B], [.9, .8], [0, 0]),
        ("exact_thr_step_below", 1, below, [A, B], [.9, .8], [0, 0]),
        ("equal_iou_left_first", 1, 0.5, [shift(C, -.0625), shift(C, .0625), C], [.9, .8, .7], [0, 0, 0]),
        ("equal_iou_right_first", 1, 0.5, [shift(C, -.0625), shift(C, .0625), C], [.8, .9, .7], [0, 0, 0]),
        ("drift_matches_fused_only", 3, 0.42, [[0, 0, .1875, .3125], [0, 0, .3125, .1875], [0, 0, .375, .375], far],
         [.9, .8, .7, .6], [1, 1, 1, 1]),
        ("drift_matches_fused_not_first", 3, 0.5, [b1, shift(b1, .125), shift(b1, .2), far], [.9, .8, .7, .6], [1, 1, 1, 1]),
        ("drift_matches_member_only", 3, 0.5, [b1, shift(b1, .125), shift(b1, -.125), far], [.9, .8, .7, .6], [1, 1, 1, 2]),
        ("zero_intersection", 1, 0.0, [[0, 0, .25, .25], [.25, 0, .5, .25], [0, .25, .25, .5]], [.9, .8, .7], [0, 0, 0]),
    ]


def random_prediction(rng, B, nc, n_obj, empty=()):
    """(B, N, 5+nc): jittered objects, rows below the objectness and the confidence threshold among them."""
    imgs = []
    for b in range(B):
        boxes, labels = objects(rng, int(rng.integers(n_obj[0], n_obj[1])), 4, nc)
        scores = rng.uniform(0.26, 0.99, len(boxes)).astype(F)
        z = prediction_from(boxes, scores, labels, nc)
        z[:, 4] = rng.uniform(0.8, 1.0, len(z)).astype(F)           # conf = obj * cls, a real product
        z[:, 5:] = (z[:, 5:] / z[:, 4:5]).astype(F)
        low = rng.random(len(z))
        z[low < 0.1, 4] = rng.uniform(0.0, 0.25, int((low < 0.1).sum())).astype(F)      # obj below conf_thres
        z[(low > 0.9), 5:] *= F(0.2)                                                      # obj * cls below conf_thres
        if b in empty:
            z[:, 4] = F(0.1)
        imgs.append(z)
    N = max(len(z) for z in imgs)
    out = np.zeros((B, N, 5 + nc), F)
    for b, z in enumerate(imgs):
        out[b, :len(z)] = z
        perm = rng.permutation(N)
        out[b] = out[b][perm]
    return out


def distinct(v):
    v = np.asarray(v)
    return len(np.unique(v)) == len(v)


def main():
    import_reference()
    G = importlib.import_module("reference.basics.utils.general")
    E = importlib.import_module("reference.basics.utils.ensemble_boxes.ensemble_boxes_wbf")
    assert G.weighted_boxes_fusion is E.weighted_boxes_fusion
    rec = Recorder(E)
    wb_cases, fu_cases = [], []

    def run_wb(tag, pred, conf_thres, iou_thres, check):
        """The reference on one batch; returns the case, or None when `check` and a condition fails."""
        rec.reset()
        p = torch.from_numpy(pred)
        out = G.weighted_boxes(p.clone(), S, conf_thres=conf_thres, iou_thres=iou_thres)
        assert torch.equal(p, torch.from_numpy(pred)) and all(o.dtype == torch.float32 and o.shape[1] == 6 for o in out)
        if check:
            conf = (p[..., 5:] * p[..., 4:5]).max(-1).values
            ok = rec.margin(iou_thres) > 1e-5
            for b in range(len(p)):
                c = conf[b][(p[b, :, 4] > conf_thres) & (conf[b] > conf_thres)]
                ok = ok and distinct(c.numpy()) and distinct(out[b][:, 4].numpy())
            if not ok:
                return None
        print(f"[wbf golden] weighted_boxes {tag}: B {pred.shape[0]} N {pred.shape[1]} nc {pred.shape[2] - 5} -> "
              f"{[len(o) for o in out]} rows, {len(rec.ious)} nonzero IoUs, margin {rec.margin(iou_thres):.2e}")
        return dict(tag=tag, image_size=S, conf_thres=conf_thres, iou_thres=iou_thres, prediction=p, out=out,
                    trace=rec.take_trace())

    hand = hand_images()
    for tag, nc, thr, boxes, scores, labels in hand:
        wb_cases.append(run_wb(tag, prediction_from(boxes, scores, labels, nc)[None], 0.25, thr, False))
    # the empty image alone, and between two unequal ones
    low = np.zeros((1, 4, 6), F)
    low[..., :4] = 100.0
    low[..., 4] = 0.2
    low[..., 5] = 1.0
    wb_cases.append(run_wb("empty", low, 0.25, 0.45, False))
    for tag, B, nc, n_obj, empty in (("rand_nc1_b1", 1, 1, (30, 40), ()), ("rand_nc3_b3", 3, 3, (10, 40), (1,))):
        seed = 100
        while True:
            c = run_wb(tag, random_prediction(np.random.default_rng(seed), B, nc, n_obj, empty), 0.25, 0.45, True)
            if c is not None:
                break
            seed += 1
        print(f"[wbf golden] {tag}: seed {seed}")
        wb_cases.append(c)

    def run_fu(tag, bl, sl, ll, weights, iou_thr, skip, conf_type, overflow, check):
        rec.reset()
        boxes, scores, labels = E.weighted_boxes_fusion([b.copy() for b in bl], [s.copy() for s in sl], [l.copy() for l in ll],
                                                        weights=weights, iou_thr=iou_thr, skip_box_thr=skip,
                                                        conf_type=conf_type, allows_overflow=overflow)
        if check:
            w = np.ones(len(bl)) if weights is None else np.array(weights)
            ws = np.concatenate([s.astype(np.float64) * w[t] for t, s in enumerate(sl)])
            keep = np.concatenate(sl) >= skip
            if not (distinct(ws[keep]) and distinct(scores.astype(F)) and rec.margin(iou_thr) > 1e-5):
                return None
        return dict(conf_type=conf_type, allows_overflow=overflow, boxes=torch.from_numpy(np.asarray(boxes, np.float64)),
                    scores=torch.from_numpy(np.asarray(scores, np.float64)),
                    labels=torch.from_numpy(np.asarray(labels, np.float64)), trace=rec.take_trace())

    def group(tag, bl, sl, ll, weights, iou_thr, skip, runs):
        return dict(tag=tag, boxes_list=[torch.from_numpy(b) for b in bl], scores_list=[torch.from_numpy(s) for s in sl],
                    labels_list=[torch.from_numpy(l) for l in ll], weights=weights, iou_thr=iou_thr, skip_box_thr=skip, runs=runs)

    for tag, nc, thr, boxes, scores, labels in hand:
        bl, sl, ll = [np.array(boxes, F)], [np.array(scores, F)], [np.array(labels, np.int64)]
        fu_cases.append(group("hand_" + tag, bl, sl, ll, None, thr, 0.0,
                              [run_fu(tag, bl, sl, ll, None, thr, 0.0, "avg", False, False)]))
    for n_models, weights in ((1, None), (2, [2.0, 1.0]), (3, [1.5, 0.7, 1.0])):
        seed = 200
        while True:
            rng = np.random.default_rng(seed)
            base, lab = objects(rng, 25, 1, 3)
            bl, sl, ll = [], [], []
            for t in range(n_models):                  # every model sees most objects, each a little differently
                k = rng.random(len(base)) < 0.8
                jit = rng.normal(0, 0.004, (int(k.sum()), 4))
                bl.append((base[k] + jit).astype(F))
                sl.append(rng.uniform(0.05, 0.99, int(k.sum())).astype(F))
                ll.append(lab[k].copy())
            sl[0][0] = F(0.3)                          # a score exactly at skip_box_thr stays in
            cs = [run_fu(f"m{n_models}", bl, sl, ll, weights, 0.55, float(F(0.3)), ct, ov, True)
                  for ct in CONF_TYPES for ov in (False, True)]
            if all(c is not None for c in cs):
                break
            seed += 1
        print(f"[wbf golden] fusion, {n_models} model(s): seed {seed}, {sum(len(s) for s in sl)} boxes -> "
              f"{len(cs[0]['scores'])} clusters")
        fu_cases.append(group(f"models_{n_models}", bl, sl, ll, weights, 0.55, float(F(0.3)), cs))
    torch.save(dict(weighted_boxes=wb_cases, fusion=fu_cases), OUT)
    print(f"[wbf golden] wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
