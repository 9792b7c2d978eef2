"""The confusion matrix on the GPU (csrc/metrics.hip: sodt_confusion_update through metrics.ConfusionMatrix) against
the reference's own matrices (tests/golden/confusion.pt, written by tools/gen_confusion_golden.py) and against the host
restatement of tests/confusion_ref.py, which test_confusion_host.py pins to the same fixture.

Every comparison is exact: the counts are integers, and the IoUs are the f32 box_iou that sodt_eval_match already
reproduces bit for bit.  Generated inputs must be free of IoU ties between competing pairs (the reference leaves those
unordered); a draw with a tie is discarded and counted, and more than 5 % discarded draws fail the sweep."""
import importlib
import os

import numpy as np
import pytest
import torch

import confusion_ref as CR
import metrics_ref as MR
from oracle import ref_torch as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "confusion.pt")
pytestmark = pytest.mark.gpu
IMG = (640, 640)


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module(pkg.__name__ + ".metrics")


def _letterbox(h0, w0, img_hw=IMG):
    r = min(img_hw[0] / h0, img_hw[1] / w0)
    h, w = round(h0 * r), round(w0 * r)
    return (h0, w0), ((h / h0, w / w0), ((img_hw[1] - w) / 2, (img_hw[0] - h) / 2))


def _draw(rng, B, nc, n_det=(0, 301), n_lab=(0, 2001), img=640.0):
    """A letterboxed batch: NMS-like rows per image (confidences on both sides of 0.25, most near a label, some of
    another class, some stray), pixel-space xywh targets in shuffled order, and the loader's shapes."""
    dets, tgs, shapes = [], [], []
    for b in range(B):
        nl, n = int(rng.integers(*n_lab)), int(rng.integers(*n_det))
        xy = rng.uniform(0, img - 60, (nl, 2))
        wh = rng.uniform(6, 60, (nl, 2))
        tcls = rng.integers(0, nc, nl)
        tgs.append(np.concatenate([np.full((nl, 1), b), tcls[:, None], xy + wh / 2, wh], 1))
        boxes = np.concatenate([u := rng.uniform(0, img - 60, (n, 2)), u + rng.uniform(6, 60, (n, 2))], 1)
        pc = rng.integers(0, nc, n)
        if nl:
            src = rng.integers(0, nl, n)
            near = rng.random(n) < 0.8
            jit = rng.normal(0, rng.uniform(0.3, 6, (n, 1)), (n, 4))
            boxes[near] = (np.concatenate([xy[src], xy[src] + wh[src]], 1) + jit)[near]
            same = near & (rng.random(n) < 0.8)
            pc[same] = tcls[src][same]
        conf = np.sort(rng.random(n).astype(np.float32))[::-1]
        dets.append(np.concatenate([boxes, conf[:, None], pc[:, None]], 1).astype(np.float32))
        shapes.append(((int(rng.integers(200, 1200)), int(rng.integers(200, 1200))), None) if b % 4 == 0 else
                      _letterbox(int(rng.integers(200, 1200)), int(rng.integers(200, 1200))))
    tg = np.concatenate(tgs).astype(np.float32).reshape(-1, 6)
    return dets, tg[rng.permutation(len(tg))], shapes


def _geom(shapes, img_hw=IMG):
    return [MR.geometry(img_hw, s) for s in shapes]


def _gpu_update(cm, dets, tg, shapes, dev, img_hw=IMG):
    cm.update([torch.from_numpy(d).to(dev) for d in dets], torch.from_numpy(tg).to(dev), img_hw, shapes)


def test_golden_process_batch(metrics, dev):
    for c in torch.load(GOLD):
        cm = metrics.ConfusionMatrix(c["nc"], conf=c["conf"], iou_thres=c["iou_thres"])
        for det, lab in c["images"]:
            cm.process_batch(det.to(dev), lab.to(dev))
        got = cm.matrix
        assert got.dtype == np.float64 and got.shape == (c["nc"] + 1, c["nc"] + 1)
        assert np.array_equal(got, c["matrix"].numpy().astype(np.float64)), c["tag"]


def test_batch_form_equals_per_image_process_batch(metrics, dev):
    rng = np.random.default_rng(11)
    nc, B = 8, 5
    dets, tg, _ = _draw(rng, B, nc, n_det=(40, 301), n_lab=(10, 60))
    dets[3] = dets[3][:0]                                                   # an image without detections
    shapes = [_letterbox(375, 500), _letterbox(500, 333), _letterbox(480, 600), ((720, 1280), None), _letterbox(1000, 700)]
    geom = _geom(shapes)
    assert all(g[2] != 1.0 and (g[3] != 0.0 or g[4] != 0.0) for g in geom)   # non-unit gain, non-zero pad
    tg = np.concatenate([tg, np.array([[B, 1, 300, 300, 40, 40]], np.float32)])[rng.permutation(len(tg) + 1)]   # image B: not in the batch
    assert not np.all(np.diff(tg[:, 0]) >= 0)                               # targets in shuffled order
    batch = metrics.ConfusionMatrix(nc)
    _gpu_update(batch, dets, tg, shapes, dev)
    single = metrics.ConfusionMatrix(nc)
    want = np.zeros((nc + 1, nc + 1), np.int64)
    for b in range(B):
        predn, lab = CR.native_boxes(dets[b], tg[tg[:, 0] == b, 1:], geom[b])    # host-scaled boxes of image b
        assert CR.tie_free(predn, lab)
        single.process_batch(torch.from_numpy(predn).to(dev), torch.from_numpy(lab).to(dev))
        CR.process_batch_np(want, predn, lab, nc)
    got = batch.matrix
    assert np.array_equal(got, single.matrix)
    assert np.array_equal(got, want.astype(np.float64))
    assert got[:nc, :nc].sum() > 20 and got[nc].sum() > 0 and got[:, nc].sum() > 0


SWEEP = [  # (B, nc, detections per image, labels per image)
    (16, 80, (0, 301), (0, 2001)), (16, 8, (0, 301), (0, 2001)), (16, 1, (0, 301), (0, 2001)),
    (8, 8, (250, 301), (20, 60)), (8, 80, (250, 301), (20, 60)), (3, 1, (0, 40), (0, 10)),
    (1, 8, (300, 301), (2000, 2001)), (5, 8, (0, 1), (0, 300)), (5, 8, (0, 301), (0, 1)),
    (7, 80, (0, 301), (0, 200)), (2, 1, (300, 301), (1500, 2001)), (12, 8, (0, 120), (0, 500)),
]


def test_random_sweep_against_restatement(metrics, dev):
    rng = np.random.default_rng(21)
    draws = discarded = 0
    for rep in range(4):
        for B, nc, n_det, n_lab in SWEEP:
            draws += 1
            dets, tg, shapes = _draw(rng, B, nc, n_det, n_lab)
            want = np.zeros((nc + 1, nc + 1), np.int64)
            if not CR.update_np(want, dets, tg, _geom(shapes), nc, check_ties=True):
                discarded += 1
                continue
            cm = metrics.ConfusionMatrix(nc)
            _gpu_update(cm, dets, tg, shapes, dev)
            got = cm.matrix
            assert np.array_equal(got, want.astype(np.float64)), (B, nc, n_det, n_lab)
            # the same images in another order: same matrix
            perm = rng.permutation(B)
            inv = np.empty(B, np.int64)
            inv[perm] = np.arange(B)
            tg2 = tg.copy()
            tg2[:, 0] = inv[tg[:, 0].astype(np.int64)]
            cm2 = metrics.ConfusionMatrix(nc)
            _gpu_update(cm2, [dets[i] for i in perm], tg2, [shapes[i] for i in perm], dev)
            assert np.array_equal(cm2.matrix, got), (B, nc, n_det, n_lab)
    print(f"random sweep: {draws} draws, {discarded} discarded for IoU ties")
    assert discarded <= 0.05 * draws, f"{discarded} of {draws} draws discarded for IoU ties"


def test_accumulation_reset_and_attributes(metrics, dev):
    rng = np.random.default_rng(31)
    nc = 8
    dets, tg, shapes = _draw(rng, 6, nc, n_det=(50, 301), n_lab=(5, 80))
    want = np.zeros((nc + 1, nc + 1), np.int64)
    assert CR.update_np(want, dets, tg, _geom(shapes), nc, check_ties=True)
    whole = metrics.ConfusionMatrix(nc)
    _gpu_update(whole, dets, tg, shapes, dev)
    parts = metrics.ConfusionMatrix(nc)
    for b0 in (0, 2, 4):                              # three calls of two images, re-indexed per call as the loader does
        t = tg[(tg[:, 0] >= b0) & (tg[:, 0] < b0 + 2)].copy()
        t[:, 0] -= b0
        _gpu_update(parts, dets[b0:b0 + 2], t, shapes[b0:b0 + 2], dev)
    m = parts.matrix
    assert np.array_equal(m, whole.matrix) and np.array_equal(m, want.astype(np.float64))
    assert m.dtype == np.float64 and m.shape == (nc + 1, nc + 1) and m.sum() > 0
    assert (parts.nc, parts.conf, parts.iou_thres) == (nc, 0.25, 0.45)
    assert np.array_equal(parts.normalized(), m / (m.sum(0).reshape(1, nc + 1) + 1E-6))
    with pytest.raises(NotImplementedError):
        parts.plot(save_dir=".", names=["a"] * nc)
    parts.reset()
    assert not parts.matrix.any() and parts.bad_classes() == (0, 0)
    parts.update([], torch.zeros((0, 6), device=dev), IMG, [])              # an empty batch
    parts.process_batch(torch.zeros((0, 6), device=dev), torch.zeros((0, 5), device=dev))
    assert not parts.matrix.any()


def test_bad_classes_are_reported_not_written(metrics, dev):
    nc = 8
    b0, b1, b2, b3 = [100, 100, 180, 160], [300, 300, 340, 380], [500, 120, 560, 200], [50, 400, 90, 460]
    lab = torch.tensor([[1] + b0, [8] + b1, [2] + b2, [2.5] + b3, [-1] + [600, 600, 620, 620]], dtype=torch.float32)
    det = torch.tensor([b0 + [0.9, 9], b2 + [0.8, 2], [10, 10, 30, 30, 0.7, 3], [10, 500, 30, 530, 0.1, 77]], dtype=torch.float32)
    cm = metrics.ConfusionMatrix(nc)
    cm.process_batch(det.to(dev), lab.to(dev))
    assert cm.bad_classes() == (3, 1)                 # labels 8, 2.5, -1; the kept detection of class 9 (77 is below conf)
    with pytest.raises(ValueError):
        cm.matrix
    raw = cm._matrix.cpu().numpy().reshape(nc + 1, nc + 1)
    assert raw[2, 2] == 1 and raw[3, nc] == 1 and raw.sum() == 2    # [1, 9], [nc, 8], [nc, 2.5], [nc, -1], [9, nc]: not written


def test_tie_rule(metrics, dev):
    # equal IoUs (exact arithmetic): a detection as close to two labels takes the lower label, and of two identical
    # detections the lower one keeps the label - the documented rule where the reference leaves the order open
    lab = np.array([[1, 100, 100, 124, 120], [2, 116, 100, 140, 120]], np.float32)
    det = np.array([[100, 100, 140, 120, 0.9, 3], [100, 100, 140, 120, 0.8, 4]], np.float32)
    assert not CR.tie_free(det, lab)
    cm = metrics.ConfusionMatrix(8)
    cm.process_batch(torch.from_numpy(det).to(dev), torch.from_numpy(lab).to(dev))
    want = np.zeros((9, 9), np.int64)
    CR.process_batch_np(want, det, lab, 8)
    got = cm.matrix
    assert np.array_equal(got, want.astype(np.float64))
    assert got[1, 3] == 1 and got[8, 2] == 1 and got[4, 8] == 1 and got.sum() == 3


def test_no_synchronisation(metrics, dev):
    rng = np.random.default_rng(41)
    nc = 8
    dets, tg, shapes = _draw(rng, 4, nc, n_det=(50, 301), n_lab=(5, 80))
    out = [torch.from_numpy(d).to(dev) for d in dets]
    tg_d = torch.from_numpy(tg).to(dev)
    predn, lab = CR.native_boxes(dets[1], tg[tg[:, 0] == 1, 1:], _geom(shapes)[1])
    predn_d, lab_d = torch.from_numpy(predn).to(dev), torch.from_numpy(lab).to(dev)
    cm = metrics.ConfusionMatrix(nc)
    cm.update(out, tg_d, IMG, shapes)
    cm.process_batch(predn_d, lab_d)
    before = cm.matrix
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                # the mode does flag a device read
        cm.update(out, tg_d, IMG, shapes)               # raises if anything on the way reads the device
        cm.process_batch(predn_d, lab_d)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(cm.matrix, 2 * before) and before.sum() > 0


def test_output_to_target(metrics, pkg, dev):
    nms = importlib.import_module(pkg.__name__ + ".nms")
    z = R.synthetic_predictions(4, 6000, 8, seed=5).to(dev)
    out = nms.non_max_suppression(z, 0.05, 0.5, multi_label=True)
    out = [out[0], out[1][:0], out[2], out[3][:0]]                          # empty images among them
    got = metrics.output_to_target(out)
    want = CR.output_to_target_np([o.cpu().numpy() for o in out])
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape and want.shape[0] > 10
    assert np.array_equal(got.cpu().numpy(), want)
    assert set(np.unique(want[:, 0]).tolist()) == {0.0, 2.0}
    empty = metrics.output_to_target([o[:0] for o in out])
    assert tuple(empty.shape) == (0, 7)
