"""non_max_suppression_batch (sodt_nms_batch, csrc/nms_batch.hip): the whole batch in one launch sequence without a host
read, against the golden outputs of the reference's own function (tests/golden/nms.pt), the oracle restatement of
general.py:425-512 and the per-image path of this package.  The gates are those of tests/test_nms_gpu.py: kept candidate
ids IDENTICAL, conf / cls equal, box coordinates (an f32 matmul in the reference's merge) within 1e-3 px."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "nms.pt")
pytestmark = pytest.mark.gpu
MAX_DET = 300


@pytest.fixture(scope="module")
def nms(pkg):
    return importlib.import_module(pkg.__name__ + ".nms")


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module(pkg.__name__ + ".metrics")


def _check_image(o, i, ro, ri):
    assert o.shape == ro.shape, (o.shape, ro.shape)
    assert torch.equal(i.cpu(), ri.cpu().long()), "kept candidate ids differ"
    if o.numel():
        assert torch.equal(o[:, 4:].cpu(), ro[:, 4:].cpu()), "conf / cls differ"
        assert float((o[:, :4].cpu() - ro[:, :4].cpu()).abs().max()) < 1e-3


def _check(out, idx, ref_out, ref_idx):
    assert len(out) == len(ref_out)
    for o, i, ro, ri in zip(out, idx, ref_out, ref_idx):
        _check_image(o, i, ro, ri)


def _check_packed(dets):
    """The packed form itself: offsets start at 0, grow by at most 300 per image, and everything past offsets[B] is zero."""
    off = dets.offsets.cpu()
    assert dets.rows.shape == (dets.B * MAX_DET, 6) and dets.index.shape == (dets.B * MAX_DET,)
    assert off.dtype == torch.int32 and off.shape == (dets.B + 1,) and int(off[0]) == 0
    d = off[1:] - off[:-1]
    assert bool((d >= 0).all()) and bool((d <= MAX_DET).all())
    assert torch.equal(dets.counts().cpu(), d)
    end = int(off[-1])
    assert not dets.rows[end:].any() and not dets.index[end:].any()


# ---- 1. the goldens -------------------------------------------------------------------------------------------------

def test_golden_cases(nms, dev):
    cases = torch.load(GOLD)
    assert len(cases) == 8
    for c in cases:
        z = R.synthetic_predictions(c["B"], c["N"], c["nc"], seed=c["seed"])
        dets = nms.non_max_suppression_batch(z.to(dev), c["conf"], c["iou"], classes=c["classes"], agnostic=c["agnostic"],
                                             multi_label=c["multi_label"], labels=c.get("labels", ()))
        _check_packed(dets)
        out, idx = dets.to_list(return_index=True)
        _check(out, idx, c["out"], c["index"])
    assert sum("labels" in c for c in cases) >= 2


def test_labels_on_the_device_and_refusals(nms, dev):
    c = next(c for c in torch.load(GOLD) if "labels" in c)
    z = R.synthetic_predictions(c["B"], c["N"], c["nc"], seed=c["seed"])
    dets = nms.non_max_suppression_batch(z.to(dev), c["conf"], c["iou"], multi_label=c["multi_label"],
                                         labels=[l.to(dev) for l in c["labels"]])
    _check(*dets.to_list(return_index=True), c["out"], c["index"])
    with pytest.raises(RuntimeError):
        nms.non_max_suppression_batch(z, 0.25, 0.45)                                     # CPU tensor: no fallback
    with pytest.raises(ValueError):
        nms.non_max_suppression_batch(z.to(dev)[0], 0.25, 0.45)                          # (N, 5 + nc): wrong rank
    with pytest.raises(ValueError):
        nms.non_max_suppression_batch(z.to(dev), 0.25, 0.45, labels=[torch.zeros(1, 5)])   # one label tensor per image


# ---- 2. one mixed batch ---------------------------------------------------------------------------------------------
# N = 4096 rows of synthetic_predictions(1, 4096, 8, seed=6, clusters=200), objectness floored at 0.2 and class scores at
# 0.05 so that a live row passes conf 0.001 with every class (0.2 * 0.05 = 0.01); objectness 0 past the first k rows
# leaves exactly k live rows.  `single`: all but the best class score of a row are zeroed, one candidate per row.
# The oracle keeps 0, 1, 1, 1, 2, 183, 300 and 300 rows of these eight images.
MIX = [(0, True), (1, True), (63, True), (64, True), (65, True), (2999, True), (3000, True), (4096, False)]
MIX_CONF, MIX_IOU = 0.001, 0.6


def _mixed_batch():
    base = R.synthetic_predictions(1, 4096, 8, seed=6, clusters=200)[0]
    imgs = []
    for k, single in MIX:
        z = base.clone()
        z[:, 4] = z[:, 4].clamp(min=0.2)
        z[k:, 4] = 0.0
        z[:, 5:] = z[:, 5:].clamp(min=0.05)
        if single:
            keep = torch.zeros_like(z[:, 5:])
            keep[torch.arange(z.shape[0]), z[:, 5:].argmax(1)] = 1.0
            z[:, 5:] *= keep
        imgs.append(z)
    return torch.stack(imgs)


@pytest.fixture(scope="module")
def mixed():
    """The batch and the oracle's result for every image alone, multi_label on (the validation setting)."""
    z = _mixed_batch()
    ref = [R.non_max_suppression(z[b:b + 1].clone(), MIX_CONF, MIX_IOU, multi_label=True, return_index=True)
           for b in range(z.shape[0])]
    return z, [r[0][0] for r in ref], [r[1][0] for r in ref]


def test_mixed_batch_against_the_oracle(nms, dev, mixed):
    z, ro, ri = mixed
    n_cand = [int((z[b, :, 5:] * z[b, :, 4:5] > MIX_CONF).sum()) for b in range(len(MIX))]
    assert n_cand == [0, 1, 63, 64, 65, 2999, 3000, 32768]
    kept = [len(i) for i in ri]
    assert kept[0] == 0 and kept[1] == 1                       # nothing; one candidate is not merged (n > 1 fails)
    assert 0 < kept[5] < MAX_DET and kept[6] == MAX_DET        # 2999 merges and filters, 3000 does not (general.py:499)
    assert kept[7] == MAX_DET                                  # 32768 candidates: the 30000 cut, then the 300 cut
    dets = nms.non_max_suppression_batch(z.to(dev), MIX_CONF, MIX_IOU, multi_label=True)
    _check_packed(dets)
    out, idx = dets.to_list(return_index=True)
    _check(out, idx, ro, ri)
    perm = [7, 2, 5, 0, 6, 3, 1, 4]
    pout, pidx = nms.non_max_suppression_batch(z[perm].to(dev), MIX_CONF, MIX_IOU, multi_label=True).to_list(True)
    for q, b in enumerate(perm):
        assert torch.equal(pidx[q], idx[b]) and torch.equal(pout[q], out[b]), f"image {b} changed at position {q}"


def test_mixed_batch_single_label(nms, dev):
    z = _mixed_batch()[[1, 4, 5, 6, 7]]
    ro, ri = R.non_max_suppression(z.clone(), MIX_CONF, MIX_IOU, multi_label=False, return_index=True)
    assert [len(i) for i in ri][3:] == [MAX_DET, MAX_DET]
    _check(*nms.non_max_suppression_batch(z.to(dev), MIX_CONF, MIX_IOU).to_list(True), ro, ri)


# ---- 3. the 300 cut and the redundancy filter -----------------------------------------------------------------------

def _grid_boxes(copies):
    """301 disjoint 16 px boxes on a 40 px grid, each present `copies` times: copy c of box k is row c * 301 + k with the
    class-2 score 0.9 - 0.3 c - 0.0005 k (all distinct, copy 0 in front, all above conf 0.25 after the objectness 0.9)."""
    k = torch.arange(301)
    z = torch.zeros(301 * copies, 13)
    for c in range(copies):
        r = slice(c * 301, (c + 1) * 301)
        z[r, 0] = 20.0 + 40.0 * (k % 18)
        z[r, 1] = 20.0 + 40.0 * (k // 18)
        z[r, 2:4] = 16.0
        z[r, 4] = 0.9
        z[r, 5 + 2] = 0.9 - 0.3 * c - 0.0005 * k
    return z


def test_max_det_cut_and_redundancy_filter(nms, dev):
    twice, once = _grid_boxes(2), _grid_boxes(1)
    pad = torch.zeros(301, 13)                                  # dead rows: every image of a batch has N = 602
    z = torch.stack([twice, torch.cat([once, pad]), R.synthetic_predictions(1, 602, 8, seed=12)[0]])
    ro, ri = R.non_max_suppression(z.clone(), 0.25, 0.45, return_index=True)
    assert len(ri[0]) == MAX_DET and ri[0][:3].tolist() == [2, 10, 18]      # 301 survive NMS, 300 the cut, all are pairs
    assert len(ri[1]) == 0 and len(ri[2]) > 0                               # no box has a second member: all redundant
    dets = nms.non_max_suppression_batch(z.to(dev), 0.25, 0.45)
    _check_packed(dets)
    out, idx = dets.to_list(return_index=True)
    _check(out, idx, ro, ri)
    assert idx[0][:3].tolist() == [2, 10, 18] and dets.counts().tolist()[:2] == [MAX_DET, 0]


# ---- 4. ties and isolation ------------------------------------------------------------------------------------------

def test_ties_and_isolation(nms, dev):
    """Identical boxes with identical scores in image 1: the first in candidate order survives, and the images next to
    it give what they give alone."""
    tie = torch.zeros(200, 13)
    tie[:, :4] = torch.tensor([100.0, 100.0, 20.0, 30.0])
    tie[:, 4] = 0.9
    tie[:, 5 + 3] = 0.8
    tie[100:, :2] += 500.0
    side = R.synthetic_predictions(2, 200, 8, seed=21)
    z = torch.stack([side[0], tie, side[1]])
    ro, ri = R.non_max_suppression(z.clone(), 0.25, 0.45, multi_label=True, return_index=True)
    out, idx = nms.non_max_suppression_batch(z.to(dev), 0.25, 0.45, multi_label=True).to_list(True)
    _check(out, idx, ro, ri)
    assert idx[1].tolist() == [0 * 8 + 3, 100 * 8 + 3]
    for b in (0, 2):
        o1, i1 = nms.non_max_suppression_batch(z[b:b + 1].to(dev), 0.25, 0.45, multi_label=True).to_list(True)
        assert torch.equal(i1[0], idx[b]) and torch.equal(o1[0], out[b])


# ---- 5. agreement with the list path --------------------------------------------------------------------------------

def test_agrees_with_the_list_path(nms, dev, mixed):
    zd = mixed[0].to(dev)
    lo, li = nms.non_max_suppression(zd, MIX_CONF, MIX_IOU, multi_label=True, return_index=True)
    out, idx = nms.non_max_suppression_batch(zd, MIX_CONF, MIX_IOU, multi_label=True).to_list(return_index=True)
    _check(out, idx, lo, li)
    assert all(o.device == zd.device and o.dtype == torch.float32 and i.dtype == torch.long for o, i in zip(out, idx))


# ---- 6. the workspace -----------------------------------------------------------------------------------------------

def test_workspace_bounds_and_refusals(pkg, ops, nms, dev):
    B, N, nc, conf, iou = 3, 700, 8, 0.25, 0.45
    z = R.synthetic_predictions(B, N, nc, seed=31).to(dev)
    need = ops.nms_batch_workspace_bytes(B, N, nc, True)
    assert need == ops.nms_batch_workspace_bytes(B, N, nc, True) and need < ops.nms_batch_workspace_bytes(B + 1, N, nc, True)
    assert ops.nms_batch_workspace_bytes(B, N, nc, False) < need
    pad = 4096
    buf = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device=dev)
    rows = torch.full((B * MAX_DET, 6), 7.0, device=dev)
    index = torch.full((B * MAX_DET,), 7, dtype=torch.int32, device=dev)
    off = torch.full((B + 1,), 7, dtype=torch.int32, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((rows == 7.0).all()) and bool((index == 7).all()) and bool((off == 7).all())

    with pytest.raises(RuntimeError, match="status 1"):        # SODT_EINVAL: one byte short
        ops.nms_batch(z, None, None, conf, iou, True, None, False, buf[pad:pad + need - 1], rows, index, off)
    assert untouched()
    fn = pkg._lib.load().sodt_nms_batch                         # a null z cannot be said through the tensor wrapper
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = fn(None, B, N, nc, None, None, 0, ctypes.c_float(conf), ctypes.c_float(iou), 1, None, 0,
            buf[pad:].data_ptr(), need, rows.data_ptr(), index.data_ptr(), off.data_ptr(), st)
    assert rc == pkg._lib.EINVAL and untouched()
    assert bool((buf == 0xA5).all())

    ops.nms_batch(z, None, None, conf, iou, True, None, False, buf[pad:pad + need], rows, index, off)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + need:] == 0xA5).all()), "wrote outside the workspace"
    got = nms.BatchDetections(rows, index, off, B)
    _check_packed(got)
    want = nms.non_max_suppression_batch(z, conf, iou, multi_label=True)
    assert torch.equal(got.offsets, want.offsets) and torch.equal(got.rows, want.rows) and torch.equal(got.index, want.index)
    assert int(off[-1]) > 0


# ---- 7. no host read ------------------------------------------------------------------------------------------------

def _validation_batch(dev, B=4, N=3000, nc=8):
    """Predictions, pixel-space targets cut from their own rows (so true positives exist) and the loader's shapes."""
    z = R.synthetic_predictions(B, N, nc, seed=5)
    g = torch.Generator().manual_seed(7)
    tg = []
    for b in range(B):
        r = torch.randperm(N, generator=g)[:40]
        tg.append(torch.cat([torch.full((40, 1), float(b)), z[b, r, 5:].argmax(1, keepdim=True).float(), z[b, r, :4]], 1))
    shapes = [((1024, 1024), None), ((960, 1024), None), ((1024, 768), None), ((512, 512), None)][:B]
    return z.to(dev), torch.cat(tg).to(dev), shapes


def test_no_host_read_through_the_statistics(nms, metrics, dev):
    z, tg, shapes = _validation_batch(dev)
    nc, hw = z.shape[2] - 5, (1024, 1024)

    def run(batched):
        dets = nms.non_max_suppression_batch(z, 0.05, 0.6, multi_label=True)
        dm, cm = metrics.DetectionMetrics(nc, dev), metrics.ConfusionMatrix(nc, conf=0.25, iou_thres=0.45, device=dev)
        dm.update(dets if batched else batched_list, tg, hw, shapes)
        cm.update(dets if batched else batched_list, tg, hw, shapes)
        return dm, cm

    batched_list = nms.non_max_suppression_batch(z, 0.05, 0.6, multi_label=True).to_list()    # allocator and library warm
    assert sum(len(o) for o in batched_list) > 0
    run(True)
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
            dm, cm = run(True)                                  # raises if anything on the way reads the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert detects, "torch.cuda.set_sync_debug_mode('error') does not flag .item(): the check above proves nothing"
    dm_l, cm_l = run(False)
    res, want = dm.compute(), dm_l.compute()
    assert float(want.map50) > 0                                # there are true positives to get wrong
    for a, b in zip(res, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(dm.stats(), dm_l.stats()):
        assert np.array_equal(a, b)
    assert np.array_equal(cm.matrix, cm_l.matrix) and cm.matrix.sum() > 0


# ---- 8. launches ----------------------------------------------------------------------------------------------------

def test_launch_list_does_not_depend_on_the_batch(nms, ops, dev):
    z = R.synthetic_predictions(4, 900, 8, seed=41).to(dev)
    names = {}
    for B in (1, 4):
        with ops.Recorder() as rec:
            nms.non_max_suppression_batch(z[:B], 0.25, 0.45, multi_label=True)
        names[B] = [c[2] for c in rec.calls]
    assert names[1] == names[4] == ["sodt_nms_batch"]
