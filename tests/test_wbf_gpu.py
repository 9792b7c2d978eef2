"""Weighted boxes fusion on the GPU (csrc/wbf.hip through wbf.weighted_boxes / wbf.weighted_boxes_fusion) against the
reference's own results (tests/golden/wbf.pt, written by tools/gen_wbf_golden.py) and against the host restatement of
tests/wbf_ref.py, which test_wbf_host.py pins to the same fixture.

Pass criteria: the number of clusters, their labels, their order and the cluster every candidate went into are
identical; float32 values agree to rtol = 2.4e-7, atol = 0 (two float32 steps).  The kernel follows the reference's
float64 and float32 operations one by one, so nothing but a differently contracted float64 multiply-add ahead of a
final float32 rounding could move a value.  Every comparison prints the worst difference it saw (pytest -s)."""
import importlib
import os

import numpy as np
import pytest
import torch

import wbf_ref as WR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "wbf.pt")
pytestmark = pytest.mark.gpu
RTOL = 2.4e-7
WORST = {"rel": 0.0}


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


@pytest.fixture(scope="module")
def wbf(pkg):
    return importlib.import_module(pkg.__name__ + ".wbf")


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size == 0:
        return
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(ref == got, 0.0, np.abs(got - ref) / np.abs(ref))
    WORST["rel"] = max(WORST["rel"], float(rel.max()))
    print(f"[wbf] {what}: worst relative difference {rel.max():.3e} (worst so far {WORST['rel']:.3e})")
    assert (np.abs(got - ref) <= RTOL * np.abs(ref)).all(), (what, float(rel.max()))


@pytest.mark.parametrize("xyxy", [False, True])
def test_weighted_boxes_every_golden_case(gold, wbf, dev, xyxy):
    for c in gold["weighted_boxes"]:
        pred = c["prediction"].to(dev)
        rows, counts, member = wbf._weighted_boxes_device(pred, c["image_size"], c["conf_thres"], c["iou_thres"], xyxy=xyxy,
                                                         return_member=True)
        out = wbf.weighted_boxes(pred, c["image_size"], c["conf_thres"], c["iou_thres"], xyxy=xyxy)
        ref = WR.weighted_boxes(c["prediction"].numpy(), c["image_size"], c["conf_thres"], c["iou_thres"], xyxy=xyxy)
        assert len(out) == len(ref) == pred.shape[0] and counts.tolist() == [len(r) for r, _ in ref], c["tag"]
        for b, (o, (r, m)) in enumerate(zip(out, ref)):
            assert o.dtype == torch.float32 and o.device == pred.device and tuple(o.shape) == r.shape, c["tag"]
            assert torch.equal(o, rows[b, :len(r)])
            want = r if xyxy else c["out"][b].numpy()          # the default return value against the reference itself
            assert np.array_equal(o[:, 5].cpu().numpy(), want[:, 5]), c["tag"]
            close(o[:, :5].cpu().numpy(), want[:, :5], f"{c['tag']}[{b}] xyxy={xyxy}")
            assert np.array_equal(member[b].cpu().numpy(), m), c["tag"]


def test_fusion_every_golden_run(gold, wbf, dev):
    for g in gold["fusion"]:
        bl = [b.to(dev) for b in g["boxes_list"]]
        sl = [s.to(dev) for s in g["scores_list"]]
        ll = [l.to(dev) for l in g["labels_list"]]
        cat = [np.concatenate([t.numpy() for t in g[k]]) for k in ("boxes_list", "scores_list", "labels_list")]
        models = np.concatenate([np.full(len(s), t) for t, s in enumerate(g["scores_list"])])
        for r in g["runs"]:
            tag = f"{g['tag']} {r['conf_type']} overflow={r['allows_overflow']}"
            b, s, l, member = wbf._weighted_boxes_fusion(bl, sl, ll, g["weights"], g["iou_thr"], g["skip_box_thr"], r["conf_type"],
                                                        r["allows_overflow"], return_member=True)
            assert b.dtype == s.dtype == torch.float32 and b.is_cuda
            assert np.array_equal(l.cpu().numpy().astype(np.float64), r["labels"].numpy()), tag
            close(b.cpu().numpy(), r["boxes"].numpy().astype(np.float32), tag + " boxes")
            close(s.cpu().numpy(), r["scores"].numpy().astype(np.float32), tag + " scores")
            ref_member = WR.fuse(*cat, models, g["weights"], g["iou_thr"], g["skip_box_thr"], r["conf_type"], r["allows_overflow"])[3]
            assert np.array_equal(member.cpu().numpy(), ref_member), tag


def _grid_case(rng, n_clusters, extra_label=True):
    """n_clusters disjoint boxes of label 0 on a 20 x 20 grid, each its own cluster, and a second, lower-scored box on
    the first, the middle and the last of them (so the match is found in every pass of the scan); label 1 holds a
    handful more."""
    cells = rng.permutation(400)[:n_clusters]
    x, y = (cells % 20) * 0.05, (cells // 20) * 0.05
    boxes = np.stack([x + 0.005, y + 0.005, x + 0.045, y + 0.045], 1)
    dup = sorted({0, n_clusters // 2, n_clusters - 1})
    boxes = np.concatenate([boxes, boxes[dup] + rng.normal(0, 0.001, (len(dup), 4))])
    labels = np.zeros(len(boxes), np.int64)
    if extra_label:
        more = np.stack([[0.1, 0.1, 0.3, 0.3], [0.11, 0.1, 0.31, 0.3], [0.6, 0.6, 0.8, 0.9]])
        boxes, labels = np.concatenate([boxes, more]), np.concatenate([labels, np.ones(3, np.int64)])
    n = len(boxes)
    scores = np.linspace(0.95, 0.30, n)                          # distinct; the grid boxes first, so they all lead
    perm = rng.permutation(n)
    return boxes[perm].astype(np.float32), scores[perm].astype(np.float32), labels[perm]


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("n_clusters", [1, 2, 63, 64, 65, 257])
def test_scan_seams(wbf, dev, n_clusters, lanes):
    boxes, scores, labels = _grid_case(np.random.default_rng(n_clusters), n_clusters)
    rb, rs, rl, rm = WR.fuse(boxes, scores, labels, iou_thr=0.55)
    assert (rl == 0).sum() == n_clusters and len(rs) == n_clusters + 2
    n = len(scores)
    tb = torch.from_numpy(boxes).to(dev).view(1, n, 4)
    ts = torch.from_numpy(scores).to(dev).view(1, n)
    tl = torch.from_numpy(labels).to(dev).to(torch.int32).view(1, n)
    counts = torch.full((1,), n, dtype=torch.int32, device=dev)
    ob, os_, ol, oc, mem = wbf._fuse(tb, ts, tl, None, None, counts,
                                     [1.0], 0.55, 0.0, 0, False, member=True, scan_lanes=lanes)
    m = int(oc.item())
    assert m == len(rs)
    assert np.array_equal(ol[0, :m].cpu().numpy(), rl) and np.array_equal(mem[0].cpu().numpy(), rm)
    close(ob[0, :m].cpu().numpy(), rb, f"seam {n_clusters} lanes {lanes} boxes")
    close(os_[0, :m].cpu().numpy(), rs.astype(np.float32), f"seam {n_clusters} lanes {lanes} scores")


@pytest.mark.parametrize("conf_type", ["box_and_model_avg", "absent_model_aware_avg"])
def test_twelve_models_sum_like_numpy(wbf, dev, conf_type):
    """More than seven weights: numpy sums them pairwise, and the confidence depends on the order of that sum."""
    rng = np.random.default_rng(12)
    M = 12
    weights = [float(w) for w in rng.uniform(0.3, 2.0, M)]
    base = np.array([[0.1, 0.1, 0.3, 0.3], [0.5, 0.5, 0.8, 0.7], [0.2, 0.6, 0.4, 0.9]])
    bl, sl, ll = [], [], []
    sc = rng.permutation(np.linspace(0.2, 0.9, 3 * M)).astype(np.float32).reshape(M, 3)
    for t in range(M):
        k = np.array([True, t % 3 != 0, t == 5])                 # object 0: all models, object 2: one model
        bl.append((base[k] + rng.normal(0, 0.002, (int(k.sum()), 4))).astype(np.float32))
        sl.append(sc[t][k])
        ll.append(np.zeros(int(k.sum()), np.int64))
    models = np.concatenate([np.full(len(s), t) for t, s in enumerate(sl)])
    rb, rs, rl, rm = WR.fuse(np.concatenate(bl), np.concatenate(sl), np.concatenate(ll), models, weights, 0.55, 0.0, conf_type)
    assert len(rs) == 3
    b, s, l, member = wbf._weighted_boxes_fusion([torch.from_numpy(a).to(dev) for a in bl], [torch.from_numpy(a).to(dev) for a in sl],
                                                [torch.from_numpy(a).to(dev) for a in ll], weights, 0.55, 0.0, conf_type,
                                                return_member=True)
    assert np.array_equal(member.cpu().numpy(), rm) and np.array_equal(l.cpu().numpy(), rl)
    close(b.cpu().numpy(), rb, f"12 models {conf_type} boxes")
    close(s.cpu().numpy(), rs.astype(np.float32), f"12 models {conf_type} scores")


def test_shuffled_rows_and_repeated_calls_are_bit_identical(gold, wbf, dev):
    c = next(c for c in gold["weighted_boxes"] if c["tag"] == "rand_nc3_b3")
    pred = c["prediction"].to(dev)
    first = wbf.weighted_boxes(pred, c["image_size"], c["conf_thres"], c["iou_thres"])
    again = wbf.weighted_boxes(pred, c["image_size"], c["conf_thres"], c["iou_thres"])
    perm = torch.randperm(pred.shape[1], generator=torch.Generator().manual_seed(3)).to(dev)
    shuffled = wbf.weighted_boxes(pred[:, perm].contiguous(), c["image_size"], c["conf_thres"], c["iou_thres"])
    assert sum(len(o) for o in first) > 0
    for a, b, s in zip(first, again, shuffled):
        assert torch.equal(a, b) and torch.equal(a, s)


def test_no_host_read_before_the_counts(gold, wbf, dev):
    c = next(c for c in gold["weighted_boxes"] if c["tag"] == "rand_nc3_b3")
    pred = c["prediction"].to(dev)
    wbf.weighted_boxes(pred, c["image_size"])                    # allocator and library warm
    torch.cuda.synchronize()
    probe = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            rows, counts = wbf._weighted_boxes_device(pred, c["image_size"], c["conf_thres"], c["iou_thres"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert detects, "torch.cuda.set_sync_debug_mode('error') does not flag .item(): the check above proves nothing"
    assert counts.tolist() == [len(o) for o in c["out"]]
