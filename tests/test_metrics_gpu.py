"""Validation statistics on the GPU (csrc/metrics.hip through sodt_amd.metrics) against the reference's own results
(tests/golden/metrics.pt, written by tools/gen_metrics_golden.py) and against the host restatements of
tests/metrics_ref.py: `correct` must be identical, p / r / f1 / ap within 1e-9, classes and counts equal."""
import importlib
import os

import numpy as np
import pytest
import torch

import metrics_ref as MR
from oracle import ref_torch as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "metrics.pt")
pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module(pkg.__name__ + ".metrics")


def _shapes(c):
    out = []
    for (h0, w0), rp, none in zip(c["h0w0"].tolist(), c["ratio_pad"].tolist(), c["rp_none"].tolist()):
        out.append(((h0, w0), None if none else ((rp[0], rp[1]), (rp[2], rp[3]))))
    return out


def _split(det, off):
    return [det[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and (a.size == 0 or float(np.abs(a - b).max()) <= TOL)


def _check_ap(got, want):
    p, r, ap, f1, cls = got
    wp, wr, wap, wf1, wcls = want
    assert np.array_equal(cls, wcls), (cls, wcls)
    assert _close(p, wp) and _close(r, wr) and _close(ap, wap) and _close(f1, wf1)


def test_golden_correct(ops, dev):
    for c in torch.load(GOLD):
        det, tg = c["det"].to(dev), c["targets"].to(dev)
        off = c["det_off"].to(dev)
        correct = torch.empty(det.shape[0], 10, dtype=torch.uint8, device=dev)
        tcls = torch.empty(tg.shape[0], device=dev)
        ws = torch.empty(ops.eval_match_workspace_bytes(len(off) - 1, det.shape[0], tg.shape[0]), dtype=torch.uint8,
                         device=dev)
        ops.eval_match(det, off, tg, c["geom"].float().to(dev), torch.linspace(0.5, 0.95, 10).tolist(), ws, correct, tcls)
        assert torch.equal(correct.cpu(), c["correct"]), c["tag"]
        t = tcls.cpu().double()
        assert torch.equal(t[t >= 0], c["tcls"]), c["tag"]


def test_golden_detection_metrics(metrics, dev):
    for c in torch.load(GOLD):
        m = metrics.DetectionMetrics(c["nc"], dev)
        det = c["det"].to(dev)
        m.update(_split(det, c["det_off"].tolist()), c["targets"].to(dev), tuple(c["img_hw"].tolist()), _shapes(c))
        correct, conf, pcls, tcls = m.stats()
        assert np.array_equal(correct, c["correct"].numpy().astype(bool)), c["tag"]
        assert np.array_equal(tcls, c["tcls"].numpy()), c["tag"]
        _check_ap(metrics.ap_per_class(correct, conf, pcls, tcls),
                  (c["p"].numpy(), c["r"].numpy(), c["ap"].numpy(), c["f1"].numpy(), c["ap_class"].numpy()))
        res = m.compute()
        assert np.array_equal(res.ap_class, c["ap_class"].numpy()) and np.array_equal(res.nt, c["nt"].numpy()), c["tag"]
        assert _close(res.p, c["p"].numpy()) and _close(res.r, c["r"].numpy())
        assert _close(res.ap50, c["ap"].numpy()[:, 0]) and _close(res.ap, c["ap"].numpy().mean(1))
        assert abs(res.map50 - c["ap"].numpy()[:, 0].mean()) <= TOL


def _procedural(rng, B, ndet, nc, img=640.0, labels=(5, 40)):
    """Random NMS-like rows (descending confidence per image) and pixel-space targets near some of them."""
    dets, tgs = [], []
    for b in range(B):
        nl = int(rng.integers(*labels))
        xy = rng.uniform(0, img - 60, (nl, 2))
        wh = rng.uniform(6, 60, (nl, 2))
        tcls = rng.integers(0, nc, nl)
        tgs.append(np.concatenate([np.full((nl, 1), b), tcls[:, None], xy + wh / 2, wh], 1))
        n = int(rng.integers(0, ndet + 1))
        src = rng.integers(0, nl, n)
        jit = rng.normal(0, rng.uniform(0.5, 8, (n, 1)), (n, 4))
        boxes = np.concatenate([xy[src], xy[src] + wh[src]], 1) + jit
        fake = rng.random(n) < 0.3
        boxes[fake] = np.concatenate([u := rng.uniform(0, img - 60, (int(fake.sum()), 2)), u + 30], 1)
        pc = np.where(rng.random(n) < 0.85, tcls[src], rng.integers(0, nc, n))
        conf = np.sort(rng.random(n).astype(np.float32))[::-1]
        dets.append(np.concatenate([boxes, conf[:, None], pc[:, None]], 1).astype(np.float32))
    tg = np.concatenate(tgs).astype(np.float32)
    return dets, tg[rng.permutation(len(tg))]


def _shapes_for(rng, B, img_hw=(640, 640)):
    out = []
    for b in range(B):
        h0, w0 = int(rng.integers(200, 1200)), int(rng.integers(200, 1200))
        if b % 4 == 0:
            out.append(((h0, w0), None))
        else:
            r = min(img_hw[0] / h0, img_hw[1] / w0)
            h, w = round(h0 * r), round(w0 * r)
            out.append(((h0, w0), ((h / h0, w / w0), ((img_hw[1] - w) / 2, (img_hw[0] - h) / 2))))
    return out


def _restate(dets, tg, shapes, img_hw):
    off = np.zeros(len(dets) + 1, np.int64)
    np.cumsum([len(d) for d in dets], out=off[1:])
    geom = [MR.geometry(img_hw, s) for s in shapes]
    return MR.match_np(np.concatenate(dets), off, tg, geom, MR.iouv_np())


def test_procedural_2000_images(metrics, dev):
    rng = np.random.default_rng(0)
    B, nc, img_hw = 2000, 8, (640, 640)
    dets, tg = _procedural(rng, B, 300, nc)
    shapes = _shapes_for(rng, B)
    m = metrics.DetectionMetrics(nc, dev)
    for b0 in range(0, B, 250):                      # targets of each batch, re-indexed per batch as the loader does
        sel = (tg[:, 0] >= b0) & (tg[:, 0] < b0 + 250)
        t = tg[sel].copy()
        t[:, 0] -= b0
        m.update([torch.from_numpy(d).to(dev) for d in dets[b0:b0 + 250]], torch.from_numpy(t).to(dev), img_hw,
                 shapes[b0:b0 + 250])
    correct, conf, pcls, tcls = m.stats()
    assert correct.shape[0] > 250000
    want_c, _ = _restate(dets, tg, shapes, img_hw)
    assert np.array_equal(correct, want_c.astype(bool))
    assert np.array_equal(np.sort(tcls), np.sort(tg[:, 1].astype(np.float64)))
    want = MR.ap_per_class_np(want_c, np.concatenate(dets)[:, 4], np.concatenate(dets)[:, 5], tcls)
    _check_ap(metrics.ap_per_class(correct, conf, pcls, tcls), want)
    res = m.compute()
    assert np.array_equal(res.ap_class, want[4]) and _close(res.p, want[0]) and _close(res.ap, want[2].mean(1))


def test_tied_confidences_are_stable(metrics, dev):
    rng = np.random.default_rng(1)
    n = 50000
    tp = rng.random((n, 10)) < np.linspace(0.7, 0.1, 10)
    conf = (rng.integers(0, 20, n) / 20).astype(np.float32)             # 20 distinct values: long tied runs
    pcls = rng.integers(0, 5, n).astype(np.float32)
    tcls = rng.integers(0, 6, 3000).astype(np.float64)
    got = metrics.ap_per_class(torch.from_numpy(tp).to(dev), torch.from_numpy(conf).to(dev),
                               torch.from_numpy(pcls).to(dev), torch.from_numpy(tcls).to(dev))
    _check_ap(got, MR.ap_per_class_np(tp, conf, pcls, tcls, stable=True))


def test_repeated_recall_runs(metrics, dev):
    # long runs of equal recall (false positives after each true positive) and confidences placed exactly on and
    # between the points of np.linspace(0, 1, 1000): every bracket rule of np.interp is exercised
    px = np.linspace(0, 1, 1000)
    conf = np.concatenate([px[::-7][:120], (px[1:121] + px[:120]) / 2]).astype(np.float32)
    n = len(conf)
    tp = np.zeros((n, 10), bool)
    tp[::17, :4] = True
    tp[::40, 4:] = True
    tp[n - 1, :] = True
    pcls = np.zeros(n, np.float32)
    tcls = np.zeros(30)
    _check_ap(metrics.ap_per_class(tp, conf, pcls, tcls), MR.ap_per_class_np(tp, conf, pcls, tcls))


def test_empty_cases(metrics, dev):
    m = metrics.DetectionMetrics(8, dev)
    m.update([], torch.zeros((0, 6), device=dev), (640, 640), [])                      # an empty batch
    res = m.compute()
    assert (res.mp, res.mr, res.map50, res.map) == (0.0, 0.0, 0.0, 0.0) and not res.maps.any() and res.nt.shape == (1,)
    shapes = [((640, 640), None)] * 4
    m.update([torch.zeros((0, 6), device=dev)] * 4, torch.zeros((0, 6), device=dev), (640, 640), shapes)   # all empty
    assert m.compute().map == 0.0 and m.stats()[0].shape == (0, 10)
    tg = torch.tensor([[3, 0, 50, 60, 10, 10], [1, 2, 100, 100, 20, 20]], dtype=torch.float32, device=dev)
    m.update([torch.zeros((0, 6), device=dev)] * 4, tg, (640, 640), shapes)                # labels, no predictions
    res = m.compute()
    assert res.map == 0.0 and res.nt.shape == (1,)
    assert m.stats()[3].tolist() == [2.0, 0.0]                                             # image order


def test_many_labels_in_one_image(metrics, dev):
    rng = np.random.default_rng(2)
    dets, tg = _procedural(rng, 2, 300, 3, labels=(5000, 5001))
    shapes = _shapes_for(rng, 2)
    m = metrics.DetectionMetrics(3, dev)
    m.update([torch.from_numpy(d).to(dev) for d in dets], torch.from_numpy(tg).to(dev), (640, 640), shapes)
    correct = m.stats()[0]
    want, _ = _restate(dets, tg, shapes, (640, 640))
    assert np.array_equal(correct, want.astype(bool)) and correct.any()


def test_workspace_sizes(ops):
    assert ops.eval_match_workspace_bytes(4, 1200, 5000) > 0
    assert ops.ap_per_class_workspace_bytes(10 ** 6, 5000, 80) > 10 ** 6 * 120     # tpc + envelope per row
    assert ops.ap_per_class_workspace_bytes(0, 0, 1) > 0


def test_end_to_end_after_nms(metrics, pkg, dev):
    nms = importlib.import_module(pkg.__name__ + ".nms")
    rng = np.random.default_rng(3)
    nc, img_hw = 8, (1024, 1024)
    m = metrics.DetectionMetrics(nc, dev)
    stats = []
    iouv = torch.linspace(0.5, 0.95, 10)
    for batch in range(3):
        z = R.synthetic_predictions(4, 6000, nc, seed=10 + batch).to(dev)
        out = nms.non_max_suppression(z, 0.05, 0.5, multi_label=True)
        tg = []
        for b, o in enumerate(out):                  # labels: jittered copies of some detections, plus misses
            o = o.cpu().numpy()
            k = o[rng.random(len(o)) < 0.4]
            xy, wh = (k[:, :2] + k[:, 2:4]) / 2, k[:, 2:4] - k[:, :2]
            xy += rng.normal(0, 2, xy.shape)
            miss = rng.uniform(0, 1000, (3, 2))
            tg.append(np.concatenate([np.full((len(k) + 3, 1), b),
                                      np.concatenate([k[:, 5], rng.integers(0, nc, 3)])[:, None],
                                      np.concatenate([xy, miss]), np.concatenate([wh, np.full((3, 2), 20.0)])], 1))
        tg = torch.from_numpy(np.concatenate(tg).astype(np.float32))
        shapes = _shapes_for(rng, 4, img_hw)
        m.update(out, tg.to(dev), img_hw, shapes)
        MR.host_loop([o.cpu() for o in out], tg, img_hw, shapes, stats, iouv)     # the same tensors, on the host
    res = m.compute()
    mp, mr, map50, map_, maps = MR.host_results(stats, nc)
    assert map50 > 0.05
    for a, b in ((res.mp, mp), (res.mr, mr), (res.map50, map50), (res.map, map_)):
        assert abs(a - b) <= TOL, (a, b)
    assert _close(res.maps, maps)


def test_golden_ap_bit_exact(metrics, dev):
    # stricter than the 1e-9 above: metrics.hip is built without FMA contraction, so the f64 path reproduces numpy's
    # rounding exactly (a contracted build differs in the last bit of about half the AP entries)
    for c in torch.load(GOLD):
        det = c["det"].numpy()
        p, r, ap, f1, cls = metrics.ap_per_class(c["correct"].numpy().astype(bool), det[:, 4], det[:, 5], c["tcls"].numpy())
        for name, v in (("p", p), ("r", r), ("ap", ap), ("f1", f1)):
            assert np.array_equal(v, c[name].numpy()), (c["tag"], name)
