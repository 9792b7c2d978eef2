"""Validation statistics on the GPU - the drop-ins for the per-image true-positive matching and the mAP of
`basics/test.py:155-264`, for `ap_per_class` (`basics/utils/metrics.py:18-78`) and for `ConfusionMatrix`
(`basics/utils/metrics.py:109-158`).

Everything after NMS runs in HIP kernels (csrc/metrics.hip) behind the C ABI (`sodt_eval_match`,
`sodt_ap_per_class`, `sodt_confusion_update`): `DetectionMetrics.update` launches one matching pass per batch and
appends to device buffers without synchronising (non_max_suppression has already read the per-image counts, so
packing the batch needs no device read); `compute()` runs ap_per_class on the device and synchronises once.
`ConfusionMatrix.update` / `.process_batch` add into a device matrix the same way; `.matrix` synchronises once.
torch only allocates and packs here.  Both `update`s also take the `BatchDetections` of `non_max_suppression_batch` in
place of the list: its packed rows and device offsets go to the same entries as they are, with no host read at all.

Differences from the reference, documented in DESIGN.md:
  * predictions with equal confidence keep their row order (a stable sort); the reference's np.argsort(-conf) is
    not stable, so its order of tied predictions - and with it p / r / ap - is unspecified.
  * `plot=True` raises NotImplementedError: the PR / F1 curves are not drawn.
  * classes are integral values below 4096; a target row whose image index is not in the batch takes part in no
    statistic, as in the reference.
  * ConfusionMatrix: candidate pairs with equal IoU go to the lower label index, then the lower detection index; the
    reference's `matches[:, 2].argsort()[::-1]` is not stable, so its winner among equal IoUs is unspecified.
  * ConfusionMatrix: pair indices are int32.  The reference casts them to int16 (metrics.py:144), which wraps above
    32,767 labels or detections per image; below that the two agree (NMS keeps at most 300 detections).
  * ConfusionMatrix.plot raises NotImplementedError; `normalized()` returns the array it would draw.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Sequence

import numpy as np
import torch

from . import ops
from .nms import BatchDetections

NIOU = 10
MAX_CLASSES = 4096

DetectionResult = namedtuple("DetectionResult", "mp mr map50 map maps nt p r ap50 ap ap_class")


def iou_vector() -> torch.Tensor:
    """test.py:100: torch.linspace(0.5, 0.95, 10), f32, computed on the host as the reference does."""
    return torch.linspace(0.5, 0.95, NIOU)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the validation statistics run on the GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _as_dev(x, dtype, dev) -> torch.Tensor:
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(device=dev, dtype=dtype).contiguous()


def _ap_device(tp: torch.Tensor, conf: torch.Tensor, pcls: torch.Tensor, tcls: torch.Tensor, nc: int):
    """Launch sodt_ap_per_class and read its results back after one synchronisation.
    Returns (p, r, f1, ap, classes, nt_count, info) as numpy arrays cut to the unique classes (info: see the header)."""
    dev = tp.device
    n, nt = tp.shape[0], tcls.numel()
    ws = torch.empty(max(1, ops.ap_per_class_workspace_bytes(n, nt, nc)), dtype=torch.uint8, device=dev)
    fo = torch.empty(nc * (3 + NIOU), dtype=torch.float64, device=dev)     # p | r | f1 | ap
    io = torch.empty(2 * nc + 4, dtype=torch.int32, device=dev)             # classes | nt_count | info
    ops.ap_per_class(tp, conf, pcls, tcls, nc, ws, fo[:nc], fo[nc:2 * nc], fo[2 * nc:3 * nc], fo[3 * nc:],
                     io[:nc], io[nc:2 * nc], io[2 * nc:])
    fh = torch.empty(fo.shape, dtype=fo.dtype, pin_memory=True)
    ih = torch.empty(io.shape, dtype=io.dtype, pin_memory=True)
    fh.copy_(fo, non_blocking=True)
    ih.copy_(io, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    f, i = fh.numpy(), ih.numpy()
    info = i[2 * nc:].copy()
    nu = int(info[0])
    if info[1]:
        raise ValueError(f"{int(info[1])} target classes are not integral values in [0, {nc})")
    p, r, f1 = f[:nu].copy(), f[nc:nc + nu].copy(), f[2 * nc:2 * nc + nu].copy()
    ap = f[3 * nc:].reshape(nc, NIOU)[:nu].copy()
    return p, r, f1, ap, i[:nu].copy(), i[nc:2 * nc].astype(np.int64), info


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir=".", names=()):
    """metrics.py:18-78 on the GPU.  tp (n, 10) bool / uint8, conf (n), pred_cls (n), target_cls (nt): numpy arrays
    or GPU tensors.  Returns numpy (p, r, ap, f1, unique_classes.astype('int32')) like the reference."""
    if plot:
        raise NotImplementedError("ap_per_class(plot=True): the PR / F1 curves are not drawn")
    dev = tp.device if isinstance(tp, torch.Tensor) and tp.is_cuda else _device()
    tp_d = _as_dev(tp, torch.uint8, dev)
    if tp_d.dim() != 2 or tp_d.shape[1] != NIOU:
        raise ValueError(f"tp must be (n, {NIOU}), got {tuple(tp_d.shape)}")
    conf_d = _as_dev(conf, torch.float32, dev).view(-1)
    pcls_d = _as_dev(pred_cls, torch.float32, dev).view(-1)
    tcls_d = _as_dev(target_cls, torch.float32, dev).view(-1)
    if conf_d.numel() != tp_d.shape[0] or pcls_d.numel() != tp_d.shape[0]:
        raise ValueError("tp, conf and pred_cls must have one row per prediction")
    if tcls_d.numel():
        lo, hi = (float(v) for v in torch.aminmax(tcls_d))
        if lo < 0:
            raise ValueError("target classes must be non-negative")
        nc = int(hi) + 1
    else:
        nc = 1
    p, r, f1, ap, classes, _, _ = _ap_device(tp_d, conf_d, pcls_d, tcls_d, nc)
    return p, r, ap, f1, classes.astype(np.int32)


def _geometry(img_hw, shape) -> list:
    """[h0, w0, gain, padw, padh] of scale_coords (general.py:323-330), in double, for one image."""
    h1, w1 = float(img_hw[0]), float(img_hw[1])
    (h0, w0), ratio_pad = shape[0], (shape[1] if len(shape) > 1 else None)
    if ratio_pad is None:
        gain = min(h1 / h0, w1 / w0)
        padw, padh = (w1 - w0 * gain) / 2, (h1 - h0 * gain) / 2
    else:
        gain, (padw, padh) = ratio_pad[0][0], ratio_pad[1]
    return [float(h0), float(w0), float(gain), float(padw), float(padh)]


class DetectionMetrics:
    """test.py:155-264 on the GPU: per-image true-positive matching as batches arrive, ap_per_class at the end.

        metrics = DetectionMetrics(nc, device)
        for img, ir, targets, paths, shapes in loader:
            ...                                            # targets[:, 2:] in input pixels (test.py:149)
            out = non_max_suppression(...)
            metrics.update(out, targets, img.shape[2:], shapes)
        res = metrics.compute()                            # mp, mr, map50, map, maps, nt, p, r, ap50, ap, ap_class
    """

    def __init__(self, nc: int, device):
        if not 1 <= int(nc) <= MAX_CLASSES:
            raise ValueError(f"nc must be in [1, {MAX_CLASSES}], got {nc}")
        self.nc = int(nc)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DetectionMetrics runs on the GPU (there is no CPU fallback)")
        self.iouv = iou_vector()
        self.reset()

    def reset(self) -> None:
        self.seen = 0
        self._correct, self._det, self._tcls = [], [], []
        self._used = []         # per batch: None (list input, every row used) or the device int32[1] count of used rows

    def update(self, out, targets: torch.Tensor, img_hw, shapes) -> None:
        """out: non_max_suppression's list ((n_i, 6) per image) or non_max_suppression_batch's BatchDetections; targets
        (nt, 6) [img cls x y w h] in input pixels; img_hw = img.shape[2:]; shapes: the loader's per-image
        ((h0, w0), ((gain_h, gain_w), (padw, padh)) or None)."""
        B = len(out)
        if len(shapes) != B:
            raise ValueError(f"{len(shapes)} shapes for {B} images")
        self.seen += B
        if B == 0:
            return
        dev = self.device
        if isinstance(out, BatchDetections):     # packed on the device already: B * 300 rows, of which offsets[B] are used
            self._match(out.rows, out.offsets, targets, img_hw, shapes, out.offsets[B:B + 1])
            return
        counts = [int(o.shape[0]) for o in out]
        off = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(counts, out=off[1:])
        n_det = int(off[-1])
        det = (torch.cat([o.detach().to(dev, torch.float32).view(-1, 6) for o in out]) if n_det
               else torch.zeros((0, 6), dtype=torch.float32, device=dev)).contiguous()
        off_d = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
        self._match(det, off_d, targets, img_hw, shapes, None)

    def _match(self, det, off_d, targets, img_hw, shapes, used) -> None:
        """One sodt_eval_match over det (n_det, 6) / off_d (B+1); `used`: see reset().  With a BatchDetections n_det is
        the upper bound B * 300 and the entry clamps to the offsets; the rows of `correct` it never writes are cut off in
        _packed(), where the host reads the device anyway."""
        dev = self.device
        B, n_det = off_d.numel() - 1, det.shape[0]
        tg = targets.detach().to(dev, torch.float32).reshape(-1, 6).contiguous()
        geom_h = torch.tensor([_geometry(img_hw, s) for s in shapes], dtype=torch.float32).pin_memory()
        geom_d = geom_h.to(dev, non_blocking=True)
        correct = torch.empty((n_det, NIOU), dtype=torch.uint8, device=dev)
        tcls = torch.empty(tg.shape[0], dtype=torch.float32, device=dev)
        ws = torch.empty(ops.eval_match_workspace_bytes(B, n_det, tg.shape[0]), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            ops.eval_match(det, off_d, tg, geom_d, self.iouv.tolist(), ws, correct, tcls)
        self._correct.append(correct)
        self._det.append(det)
        self._tcls.append(tcls)
        self._used.append(used)

    def _packed(self):
        dev = self.device
        if not self._det:
            return (torch.zeros((0, NIOU), dtype=torch.uint8, device=dev), torch.zeros(0, device=dev),
                    torch.zeros(0, device=dev), torch.zeros(0, device=dev))
        dets, corrects = self._det, self._correct
        batched = [i for i, u in enumerate(self._used) if u is not None]
        if batched:             # drop the unused (zero / never written) rows of the batched updates: one host read for all
            used = torch.cat([self._used[i] for i in batched]).tolist()
            dets, corrects = list(dets), list(corrects)
            for i, n in zip(batched, used):
                dets[i], corrects[i] = dets[i][:n], corrects[i][:n]
        det = torch.cat(dets)
        return torch.cat(corrects), det[:, 4].contiguous(), det[:, 5].contiguous(), torch.cat(self._tcls)

    def stats(self):
        """The reference's `stats` after test.py:255: numpy (correct bool (n, 10), conf f32, pcls f32, tcls f64)."""
        correct, conf, pcls, tcls = (t.cpu().numpy() for t in self._packed())
        return correct.astype(bool), conf, pcls, tcls[tcls >= 0].astype(np.float64)

    def compute(self) -> DetectionResult:
        """test.py:256-262 and :343-346.  With no true positive at all the reference's zeros come back (nt is then
        zeros(1), as test.py:263 sets it, and the per-class arrays are empty)."""
        correct, conf, pcls, tcls = self._packed()
        with torch.cuda.device(self.device):
            p, r, _, ap, ap_class, nt, info = _ap_device(correct, conf, pcls, tcls, self.nc)
        if int(info[2]) == 0:       # test.py:256: stats[0].any() is false
            e = np.zeros(0)
            return DetectionResult(0.0, 0.0, 0.0, 0.0, np.zeros(self.nc) + 0.0, np.zeros(1), e, e, e, e,
                                   np.zeros(0, dtype=np.int32))
        ap50, apm = ap[:, 0], ap.mean(1)
        mp, mr, map50, map_ = p.mean(), r.mean(), ap50.mean(), apm.mean()
        maps = np.zeros(self.nc) + map_
        for i, c in enumerate(ap_class):
            maps[c] = apm[i]
        return DetectionResult(mp, mr, map50, map_, maps, nt, p, r, ap50, apm, ap_class.astype(np.int32))


def _pack(out: Sequence[torch.Tensor], dev):
    """The NMS list as packed (n_det, 6) f32 rows and (B+1) int32 device offsets; the counts are host shapes."""
    off = np.zeros(len(out) + 1, dtype=np.int32)
    np.cumsum([int(o.shape[0]) for o in out], out=off[1:])
    det = (torch.cat([o.detach().to(dev, torch.float32).view(-1, 6) for o in out]) if int(off[-1])
           else torch.zeros((0, 6), dtype=torch.float32, device=dev)).contiguous()
    return det, torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)


class ConfusionMatrix:
    """metrics.py:109-158 on the GPU, with the reference's constructor.  Rows are predicted classes, columns true
    classes, index nc is the background, exactly as the reference fills them.

        confusion_matrix = ConfusionMatrix(nc)
        for ...:
            out = non_max_suppression(...)
            confusion_matrix.update(out, targets, img.shape[2:], shapes)   # DetectionMetrics.update's arguments
        confusion_matrix.matrix                                            # numpy (nc+1, nc+1) f64, one synchronisation
    """

    def __init__(self, nc: int, conf: float = 0.25, iou_thres: float = 0.45, device=None):
        if not 1 <= int(nc) <= MAX_CLASSES:
            raise ValueError(f"nc must be in [1, {MAX_CLASSES}], got {nc}")
        self.nc, self.conf, self.iou_thres = int(nc), conf, iou_thres
        self.device = _device() if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ConfusionMatrix runs on the GPU (there is no CPU fallback)")
        self._matrix = torch.zeros((self.nc + 1) ** 2, dtype=torch.int64, device=self.device)
        self._info = torch.zeros(2, dtype=torch.int32, device=self.device)

    def reset(self) -> None:
        self._matrix.zero_()
        self._info.zero_()

    def _launch(self, det, off, tg, geom) -> None:
        ws = torch.empty(max(1, ops.confusion_workspace_bytes(off.numel() - 1, det.shape[0], tg.shape[0])),
                         dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            ops.confusion_update(det, off, tg, geom, self.nc, self.conf, self.iou_thres, ws, self._matrix, self._info)

    def process_batch(self, detections: torch.Tensor, labels: torch.Tensor) -> None:
        """The reference's per-image call (test.py:216): detections (N, 6) [x1 y1 x2 y2 conf cls] and labels (M, 5)
        [cls x1 y1 x2 y2], both already in native pixels.  The boxes are used as they are."""
        dev = self.device
        det, off = _pack([detections.reshape(-1, 6)], dev)
        lab = labels.detach().to(dev, torch.float32).reshape(-1, 5)
        tg = torch.cat([torch.zeros((lab.shape[0], 1), dtype=torch.float32, device=dev), lab], 1).contiguous()
        self._launch(det, off, tg, None)

    def update(self, out, targets: torch.Tensor, img_hw, shapes) -> None:
        """process_batch for every image of a batch in one launch sequence; the arguments of DetectionMetrics.update
        (the NMS list or a BatchDetections, whose rows and device offsets are used as they are).
        Images without detections count their labels as missed (what process_batch does when it is given none)."""
        B = len(out)
        if len(shapes) != B:
            raise ValueError(f"{len(shapes)} shapes for {B} images")
        if B == 0:
            return
        dev = self.device
        det, off = (out.rows, out.offsets) if isinstance(out, BatchDetections) else _pack(out, dev)
        tg = targets.detach().to(dev, torch.float32).reshape(-1, 6).contiguous()
        geom = torch.tensor([_geometry(img_hw, s) for s in shapes], dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        self._launch(det, off, tg, geom)

    def _read(self):
        host = torch.empty(self._matrix.numel() + 2, dtype=torch.int64, pin_memory=True)
        host.copy_(torch.cat([self._matrix, self._info.to(torch.int64)]), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        a = host.numpy()
        return a[:-2].reshape(self.nc + 1, self.nc + 1), int(a[-2]), int(a[-1])

    def bad_classes(self):
        """(labels, kept detections) seen so far whose class is not an integral value in [0, nc); none of them counted."""
        return self._read()[1:]

    @property
    def matrix(self) -> np.ndarray:
        """The reference's attribute: numpy float64 (nc+1, nc+1).  Reads the device once."""
        m, bad_l, bad_d = self._read()
        if bad_l or bad_d:
            raise ValueError(f"{bad_l} label and {bad_d} detection classes are not integral values in [0, {self.nc})")
        return m.astype(np.float64)

    def normalized(self) -> np.ndarray:
        """The array plot() draws (metrics.py:164), before it blanks the cells below 0.005."""
        m = self.matrix
        return m / (m.sum(0).reshape(1, self.nc + 1) + 1E-6)

    def plot(self, save_dir="", names=()):
        raise NotImplementedError("ConfusionMatrix.plot: the heat map is not drawn; normalized() returns its array")

    def print(self):
        m = self.matrix
        for i in range(self.nc + 1):
            print(" ".join(map(str, m[i])))


def output_to_target(output: Sequence[torch.Tensor]) -> torch.Tensor:
    """plots.py:105-112 on the device: the NMS list as one (n, 7) f32 tensor [batch_id, class, x, y, w, h, conf]
    (xyxy2xywh of general.py:259-266), without the reference's .cpu() and Python loop per box."""
    dev = output[0].device if len(output) else _device()
    det, _ = _pack(output, dev)
    ids = np.repeat(np.arange(len(output), dtype=np.float32), [int(o.shape[0]) for o in output])
    bid = torch.from_numpy(ids).pin_memory().to(dev, non_blocking=True)
    x1, y1, x2, y2, conf, cls = det.unbind(1)
    return torch.stack([bid, cls, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, conf], 1)
