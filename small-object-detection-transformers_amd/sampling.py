"""Train.py's --image-weights on the GPU: the class weights Train.py:275 attaches to the model, and the epoch-boundary block
of Train.py:335-347 - class weights scaled by (1 - maps) ** 2, image weights, `random.choices`, the broadcast to the ranks.

The reference rebuilds the (n_img, nc) class-count matrix with one np.bincount per image at every epoch (general.py:241,
and `np.int` there no longer exists in numpy).  `ImageWeights` counts once, at construction, in one launch over all labels
(`sodt_class_counts`); an epoch is then `sodt_image_weights` (one f64 accumulator per image, classes ascending) and
`sodt_weighted_choices` (a three-phase f64 scan in a fixed order, then Python's `bisect` per draw) - csrc/sampling.hip
behind the C ABI.  The only host read of an epoch is the copy that brings the indices back; the status word rides in it.

The random stream: `choices` draws exactly `k` values with `random.random()` from Python's global generator, in draw order,
before it touches the device - `random.choices` draws the same values in the same order.  So `random.getstate()` after a
call that returns equals the reference's, and the indices equal the reference's whenever no `u * total` falls within
rounding of a cumulative weight (DESIGN.md section 4.18 has the bound).

Differences from the reference, all documented in DESIGN.md:
  * a label class outside [0, nc) raises ValueError at construction; the reference's bincount would grow that image's row
    and fail (or not) in the product that follows.
  * `random.choices` tests the total before it draws, so when it raises it has consumed nothing; here the total is known
    only on the device, after the draws went up, so the `k` values are consumed when `choices` raises.
  * the device parts have no CPU fallback.
"""
from __future__ import annotations

import contextlib
import random

import numpy as np
import torch

from . import _lib as L
from . import ops

MAX_IMAGES = 1 << 24                                  # sodt_weighted_choices: n and k
_BAD_LABEL = L.SAMPLING_BAD_CLASS | L.SAMPLING_BAD_IMAGE


def _device_of(dev=None) -> torch.device:
    if dev is not None and torch.device(dev).type == "cuda":
        return torch.device(dev)
    if not torch.cuda.is_available():
        raise RuntimeError("sampling: the class counts, the image weights and the draw run on the GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _on(dev: torch.device):
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def _host_f64(a, n: int, what: str) -> np.ndarray:
    """`a` (a numpy array or a tensor, a device tensor is read) as a float64 numpy vector of n values."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.shape != (n,):
        raise ValueError(f"{what} has shape {tuple(a.shape)}, expected ({n},)")
    return a.astype(np.float64, copy=False)


def _upload(host: np.ndarray, dev: torch.device) -> torch.Tensor:
    """One asynchronous copy of a host vector through pinned memory (a pageable copy would wait for the device)."""
    return torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)


def tree_sum(w: torch.Tensor) -> torch.Tensor:
    """The sum of a vector in the order `ImageWeights.class_weights` is normalised with: padded with +0.0 to the next power
    of two, then the upper half is added onto the lower half until one value is left.  Element-wise IEEE additions only,
    so the device and the host form the same bits."""
    p = 1 << max(w.numel() - 1, 0).bit_length()
    v = torch.zeros(p, dtype=w.dtype, device=w.device)
    v[:w.numel()] = w
    while v.numel() > 1:
        h = v.numel() // 2
        v = v[:h] + v[h:]
    return v[0]


class ImageWeights:
    """The epoch-loop object of --image-weights.

        iw = ImageWeights(dataset.labels, nc, device)              # the labels go up once, the counts are built once
        model.class_weights = iw.class_weights * nc                # Train.py:275
        ...
        dataset.indices = iw.choices(model.class_weights, maps)    # Train.py:339-341, at every epoch boundary

    labels: a list of (m_i, 5) arrays [class, x, y, w, h], one per image (m_i may be 0).
    .class_counts (n_img, nc) int32 and .class_weights (nc) float64 are device tensors; .class_weights_host is the numpy copy
    that came back with the construction's one read (pass `iw.class_weights_host * nc` to `choices` to keep an epoch at one
    synchronisation: a device tensor of class weights has to be read first)."""

    def __init__(self, labels, nc: int, device=None):
        if len(labels) == 0 or labels[0] is None:
            raise ValueError("ImageWeights needs the loaded labels, one (m, 5) array per image")
        if not 1 <= len(labels) <= MAX_IMAGES:
            raise ValueError(f"ImageWeights handles 1 to {MAX_IMAGES} images, got {len(labels)}")
        if not 1 <= int(nc) <= 65536:
            raise ValueError(f"nc must be in 1..65536, got {nc}")
        self.n, self.nc = len(labels), int(nc)
        self.device = dev = _device_of(device)
        lens = np.fromiter((len(x) for x in labels), dtype=np.int64, count=self.n)
        m = int(lens.sum())
        both = np.empty(2 * m, dtype=np.int32)                                          # classes, then image ids: one upload
        if m:
            both[:m] = np.concatenate([np.asarray(x)[:, 0] for x in labels if len(x)]).astype(np.int32)   # general.py:226
            both[m:] = np.repeat(np.arange(self.n, dtype=np.int32), lens)
        with _on(dev):
            up = _upload(both, dev)
            self.class_counts = torch.zeros(self.n, self.nc, dtype=torch.int32, device=dev)
            self.class_total = torch.zeros(self.nc, dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            ops.class_counts(up[:m], up[m:], self.n, self.nc, self.class_counts, self.class_total, status)
            # general.py:233-235 on the device: empty bins count 1, reciprocals, normalised by their tree_sum (tensor / tensor
            # is an IEEE division)
            w = torch.ones(self.nc, dtype=torch.float64, device=dev) / self.class_total.clamp(min=1).double()
            self.class_weights = w / tree_sum(w)
            host = torch.cat((status.double(), self.class_weights)).cpu().numpy()      # the one read of the construction
        if int(host[0]) & _BAD_LABEL:
            raise ValueError(f"a label class lies outside [0, {self.nc})")
        self.class_weights_host = host[1:].copy()

    def image_weights(self, cw) -> torch.Tensor:
        """general.py:242 for the counts kept on the device: cw, `nc` class weights (numpy or tensor), -> (n_img) float64 on
        the device.  No host read unless cw is a device tensor of another device."""
        with _on(self.device):
            if torch.is_tensor(cw) and cw.device == self.device:
                if cw.shape != (self.nc,):
                    raise ValueError(f"class_weights has shape {tuple(cw.shape)}, expected ({self.nc},)")
                cw_d = cw.detach().double().contiguous()
            else:
                cw_d = _upload(_host_f64(cw, self.nc, "class_weights"), self.device)
            iw = torch.empty(self.n, dtype=torch.float64, device=self.device)
            ops.image_weights(self.class_counts, cw_d, iw)
        return iw

    def choices_device(self, class_weights, maps, k=None) -> torch.Tensor:
        """`choices` up to, and without, the copy back: (k + 1) int32 on the device, the k indices and the status word.
        Nothing here waits for the device when class_weights and maps are host values."""
        k = self.n if k is None else int(k)
        if not 0 <= k <= MAX_IMAGES:
            raise ValueError(f"k must be in 0..{MAX_IMAGES}, got {k}")
        cw0, maps = _host_f64(class_weights, self.nc, "class_weights"), _host_f64(maps, self.nc, "maps")
        u = [random.random() for _ in range(k)]                                         # random.choices' draws, in its order
        cw = cw0 * (1 - maps) ** 2 / self.nc                                            # Train.py:339, float64 on the host
        host = np.empty(self.nc + k, dtype=np.float64)
        host[:self.nc], host[self.nc:] = cw, u
        dev = self.device
        with _on(dev):
            up = _upload(host, dev)                                                     # class weights and draws: one upload
            iw = torch.empty(self.n, dtype=torch.float64, device=dev)
            ops.image_weights(self.class_counts, up[:self.nc], iw)
            wsb = ops.weighted_choices_workspace_bytes(self.n, k)
            buf = torch.empty(wsb + 8 * self.n, dtype=torch.uint8, device=dev)          # the workspace, then cum
            out = torch.zeros(k + 1, dtype=torch.int32, device=dev)
            ops.weighted_choices(iw, up[self.nc:], out[:k], buf[wsb:].view(torch.float64), out[k:], buf[:wsb])
        return out

    def choices(self, class_weights, maps, k=None, return_device: bool = False):
        """Train.py:339-341 in one call: `random.choices(range(n_img), weights=iw, k=k)` for the image weights of
        cw = class_weights * (1 - maps) ** 2 / nc, as a list of ints (what `dataset.indices` holds).  k defaults to n_img.
        class_weights: the `nc` weights Train.py:275 attached (numpy or tensor); maps: the per-class AP of the epoch.
        Raises random.choices' ValueError when the total weight is not positive or not finite.  return_device=True returns
        (list, int32 device tensor)."""
        out = self.choices_device(class_weights, maps, k)
        host = out.cpu()                                                                # the one synchronisation of an epoch
        status = int(host[-1])
        if status & L.SAMPLING_ZERO_TOTAL:
            raise ValueError("Total of weights must be greater than zero")
        if status & L.SAMPLING_NONFINITE_TOTAL:
            raise ValueError("Total of weights must be finite")
        idx = host[:-1].tolist()
        return (idx, out[:-1]) if return_device else idx


def labels_to_class_weights(labels, nc: int = 80):
    """general.py:220-236: class weights (inverse frequency) from the training labels, a float64 CPU tensor of nc values."""
    if labels[0] is None:                                                               # no labels loaded
        return torch.Tensor()
    return torch.from_numpy(ImageWeights(labels, nc).class_weights_host)


def labels_to_image_weights(labels, nc: int = 80, class_weights=np.ones(80)):
    """general.py:239-244: image weights from class_weights and the image contents, a float64 numpy (n_img,) array."""
    return ImageWeights(labels, nc).image_weights(class_weights).cpu().numpy()


def broadcast_indices(indices, n: int, src: int = 0):
    """Train.py:343-347: rank `src` passes the list `choices` returned, the others None; one int32 broadcast on the backend's
    device (the GPU for nccl, the CPU otherwise), and every rank gets the list of n indices back."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("broadcast_indices needs an initialised process group")
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    if dist.get_rank() == src:
        if indices is None or len(indices) != n:
            raise ValueError(f"rank {src} passes the {n} indices, got {'None' if indices is None else len(indices)}")
        t = torch.tensor(indices, dtype=torch.int32).to(dev)
    else:
        t = torch.zeros(n, dtype=torch.int32, device=dev)
    dist.broadcast(t, src)
    return t.tolist()
