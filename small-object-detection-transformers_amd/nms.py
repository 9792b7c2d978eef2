"""non_max_suppression on the GPU - the drop-in for `utils/general.py:425` (called from
test.py:145 on the eval output of `Model.forward`).

Same signature and return value as the reference: a list with one (n, 6) f32 tensor
[x1, y1, x2, y2, conf, cls] per image, on the prediction's device.  Everything after the
Detect decode - candidate selection, class-offset NMS, the 300-detection cut, merge-NMS and
the redundancy filter - runs in HIP kernels (csrc/nms.hip) behind the C ABI
(`sodt_nms_candidates`, `sodt_nms_select`); the host only reads two counters per image.

Differences from the reference, all documented in DESIGN.md:
  * `labels` (autolabelling rows, general.py:451-458): each image's (nl, 5) [cls, x, y, w, h] rows are appended to its
    prediction rows with obj = 1 and a one-hot class before the device kernels run (candidate row index N + k).
  * ties between equal scores are broken by candidate order (a stable sort), where
    torchvision.ops.nms / argsort leave the order unspecified.
  * the 10 s time limit (general.py:509-511) does not exist.

`non_max_suppression_batch` is the same function for the whole batch at once (csrc/nms_batch.hip, `sodt_nms_batch`): one
launch sequence whatever B is, no host read, the result packed on the device as a `BatchDetections` that the validation
statistics (metrics.py) take directly.  `non_max_suppression` itself is unchanged.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import ops

MAX_DET = 300


def non_max_suppression(prediction: torch.Tensor, conf_thres: float = 0.25, iou_thres: float = 0.45,
                        classes: Optional[Sequence[int]] = None, agnostic: bool = False, multi_label: bool = False,
                        labels=(), return_index: bool = False) -> List[torch.Tensor]:
    if not prediction.is_cuda:
        raise RuntimeError("non_max_suppression: the prediction must live on the GPU (there is no CPU fallback)")
    if prediction.dim() != 3 or prediction.shape[2] < 6:
        raise ValueError(f"prediction must be (B, N, 5 + nc), got {tuple(prediction.shape)}")
    pred = prediction.detach()
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        pred = pred.float().contiguous()
    B, N, no = pred.shape
    nc = no - 5
    dev = pred.device
    ml = bool(multi_label) and nc > 1
    allow = None
    if classes is not None:
        allow = torch.zeros(nc, dtype=torch.uint8, device=dev)
        idx = torch.as_tensor([int(c) for c in classes if 0 <= int(c) < nc], dtype=torch.long, device=dev)
        allow[idx] = 1
    nlab = [len(l) for l in labels] if labels else []
    if nlab and len(nlab) != B:
        raise ValueError("labels: one (nl, 5) tensor per image")
    Nx = N + (max(nlab) if nlab else 0)
    cap = Nx * nc if ml else Nx
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    out_rows = torch.empty(MAX_DET, 6, dtype=torch.float32, device=dev)
    out_idx = torch.empty(MAX_DET, dtype=torch.int32, device=dev)
    output = [torch.zeros((0, 6), device=dev)] * B
    index = [torch.zeros((0,), dtype=torch.long, device=dev)] * B
    with torch.cuda.device(dev):
        for b in range(B):
            pb = pred[b]
            if nlab and nlab[b]:                          # general.py:451-458
                l = labels[b].to(device=dev, dtype=torch.float32)
                v = torch.zeros((nlab[b], no), device=dev)
                v[:, :4] = l[:, 1:5]
                v[:, 4] = 1.0
                v[torch.arange(nlab[b], device=dev), l[:, 0].long() + 5] = 1.0
                pb = torch.cat((pb, v), 0).contiguous()
            ops.nms_candidates(pb, conf_thres, ml, allow, keys, counters[0:1])
            n = int(counters[0].item())
            if n == 0:
                continue
            ws = torch.empty(ops.nms_workspace_bytes(n), dtype=torch.uint8, device=dev)
            ops.nms_select(pb, keys, n, iou_thres, agnostic, ws, out_rows, out_idx, counters[1:2])
            m = int(counters[1].item())
            output[b] = out_rows[:m].clone()
            index[b] = out_idx[:m].long()
    return (output, index) if return_index else output


class BatchDetections:
    """What non_max_suppression_batch returns: the detections of B images packed image after image, on the device.

    rows (B*300, 6) f32 [x1 y1 x2 y2 conf cls], index (B*300,) int32 candidate ids row * nc + class, offsets (B+1,) int32:
    image b owns [offsets[b], offsets[b+1]); everything from offsets[B] on is zero.  Nothing here has been read by the
    host: `DetectionMetrics.update` / `ConfusionMatrix.update` take the object as it is, `to_list()` synchronises once."""
    __slots__ = ("rows", "index", "offsets", "B")

    def __init__(self, rows: torch.Tensor, index: torch.Tensor, offsets: torch.Tensor, B: int):
        self.rows, self.index, self.offsets, self.B = rows, index, offsets, int(B)

    def __len__(self) -> int:
        return self.B

    def counts(self) -> torch.Tensor:
        """Detections per image, (B,) int32 on the device."""
        return self.offsets[1:] - self.offsets[:-1]

    def to_list(self, return_index: bool = False):
        """The list non_max_suppression returns (and its index list with return_index); one synchronisation."""
        off = self.offsets.tolist()
        output = [self.rows[off[b]:off[b + 1]] for b in range(self.B)]
        if not return_index:
            return output
        return output, [self.index[off[b]:off[b + 1]].long() for b in range(self.B)]


def _upload(host: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device without waiting for the device (pinned staging, asynchronous copy)."""
    return host.pin_memory().to(dev, non_blocking=True)


def non_max_suppression_batch(prediction: torch.Tensor, conf_thres: float = 0.25, iou_thres: float = 0.45,
                              classes: Optional[Sequence[int]] = None, agnostic: bool = False, multi_label: bool = False,
                              labels=()) -> BatchDetections:
    """general.py:425-512 for the whole batch in one launch sequence (csrc/nms_batch.hip, `sodt_nms_batch`): the same
    detections per image as `non_max_suppression`, but no host read, no per-image launch and no per-image allocation - the
    host runs ahead of the device into `DetectionMetrics.update` / `ConfusionMatrix.update`, which take the result as it is.
    `labels`: the reference's list of one (nl, 5) [cls, x, y, w, h] tensor per image (general.py:451-458); the lengths
    come from the host shapes."""
    if not prediction.is_cuda:
        raise RuntimeError("non_max_suppression_batch: the prediction must live on the GPU (there is no CPU fallback)")
    if prediction.dim() != 3 or prediction.shape[2] < 6:
        raise ValueError(f"prediction must be (B, N, 5 + nc), got {tuple(prediction.shape)}")
    pred = prediction.detach()
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        pred = pred.float().contiguous()
    B, N, no = pred.shape
    nc = no - 5
    dev = pred.device
    ml = bool(multi_label) and nc > 1
    nlab = [len(l) for l in labels] if labels else []
    if nlab and len(nlab) != B:
        raise ValueError("labels: one (nl, 5) tensor per image")
    rows = torch.empty((B * MAX_DET, 6), dtype=torch.float32, device=dev)
    index = torch.empty(B * MAX_DET, dtype=torch.int32, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    if B == 0:
        return BatchDetections(rows, index, offsets.zero_(), 0)
    allow = None
    if classes is not None:
        allow_h = torch.zeros(nc, dtype=torch.uint8)
        allow_h[[int(c) for c in classes if 0 <= int(c) < nc]] = 1
        allow = _upload(allow_h, dev)
    lab_d = nlab_d = None
    lab_cap = max(nlab) if nlab else 0
    if lab_cap:
        host = torch.zeros((B, lab_cap, 5), dtype=torch.float32)
        for b, l in enumerate(labels):
            if nlab[b] and not l.is_cuda:
                host[b, :nlab[b]] = l.detach().float().reshape(-1, 5)
        lab_d = _upload(host, dev)
        for b, l in enumerate(labels):
            if nlab[b] and l.is_cuda:
                lab_d[b, :nlab[b]] = l.detach().to(dev, torch.float32).reshape(-1, 5)
        nlab_d = _upload(torch.tensor(nlab, dtype=torch.int32), dev)
    with torch.cuda.device(dev):
        ws = torch.empty(ops.nms_batch_workspace_bytes(B, N + lab_cap, nc, ml), dtype=torch.uint8, device=dev)
        ops.nms_batch(pred, lab_d, nlab_d, conf_thres, iou_thres, ml, allow, agnostic, ws, rows, index, offsets)
    return BatchDetections(rows, index, offsets, B)
