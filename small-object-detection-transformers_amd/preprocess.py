"""Input pre-processing of the reference's training / evaluation loop on the device.

Train.py:364-374 moves the uint8 batch to the GPU, converts it with ``.float() / 255.0`` and, when the images were loaded at
``train_img_size = down_factor x test_img_size`` (defaults 1024 / 512, Train.py:94,612-613), shrinks RGB and IR with
``F.interpolate(..., mode='bilinear', align_corners=True)``: four full-tensor ATen kernels and two f32 intermediates at the
loaded resolution.  ``preprocess_batch`` is that in ONE launch (csrc/preprocess.hip, ``sodt_preprocess_u8``): uint8 planes
in, f32 planes out, the layout ``Model.forward`` / the front-end kernel read.  test.py:124-129 is the ``down_factor=1`` case.

``--multi-scale`` (Train.py:396-402) then draws a size per step and resizes both batches once more with
``F.interpolate(..., size=ns, mode='bilinear', align_corners=False)``.  ``multi_scale_size`` is the draw, ``preprocess_batch(...,
size=ns)`` the resize, still in ONE launch from the uint8 batch (csrc/multiscale.hip, ``sodt_preprocess_u8_ms``).
"""
from __future__ import annotations

import math
import random
from typing import Callable, Optional, Sequence, Tuple, Union

import torch

from . import ops


def _size_hw(size) -> Tuple[int, int]:
    """size of preprocess_batch: an int (square) or (h, w), positive ints"""
    hw = (size, size) if isinstance(size, int) else tuple(size) if isinstance(size, (tuple, list, torch.Size)) else None
    if hw is None or len(hw) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in hw):
        raise ValueError(f"size must be a positive int or (h, w) of positive ints (Train.py:400: ns), got {size!r}")
    return hw


def preprocess_batch(imgs: torch.Tensor, irs: torch.Tensor, down_factor: int = 1,
                     size: Union[None, int, Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """imgs, irs: uint8 (B, C, H, W) on the GPU -> f32 (B, C, H // down_factor, W // down_factor) in [0, 1].

    size (an int or (h, w)): the ``ns`` of ``--multi-scale`` (Train.py:400-402) - the result is resized once more, half-pixel
    bilinear, to (B, C, h, w), in the same single launch.  None, or the shrunk size itself, is the call without it (the
    reference skips the interpolation when ``sf == 1``)."""
    if imgs.dtype != torch.uint8 or irs.dtype != torch.uint8:
        raise TypeError("preprocess_batch takes the uint8 batch of the data loader (Train.py:362)")
    if not imgs.is_cuda or not irs.is_cuda:
        raise RuntimeError("preprocess_batch needs the batch on the GPU (Train.py:364: imgs.to(device)); there is no CPU fallback")
    if imgs.dim() != 4 or irs.dim() != 4 or imgs.shape[0] != irs.shape[0] or imgs.shape[2:] != irs.shape[2:]:
        raise ValueError("imgs and irs must be (B, C, H, W) with the same batch and size")
    if down_factor < 1:
        raise ValueError("down_factor >= 1 (Train.py:94: int(train_img_size / test_img_size))")
    hw = None if size is None else _size_hw(size)
    imgs, irs = imgs.contiguous(), irs.contiguous()
    B, c1, H, W = imgs.shape
    c2 = irs.shape[1]
    Ho, Wo = H // down_factor, W // down_factor
    if hw is None or hw == (Ho, Wo):
        out1 = torch.empty(B, c1, Ho, Wo, device=imgs.device, dtype=torch.float32)
        out2 = torch.empty(B, c2, Ho, Wo, device=imgs.device, dtype=torch.float32)
        ops._launch("sodt_preprocess_u8", imgs.data_ptr(), irs.data_ptr(), out1.data_ptr(), out2.data_ptr(), B, c1, c2, H, W, Ho, Wo)
        return out1, out2
    out1 = torch.empty(B, c1, *hw, device=imgs.device, dtype=torch.float32)
    out2 = torch.empty(B, c2, *hw, device=imgs.device, dtype=torch.float32)
    ops._launch("sodt_preprocess_u8_ms", imgs.data_ptr(), irs.data_ptr(), out1.data_ptr(), out2.data_ptr(), B, c1, c2, H, W, Ho, Wo,
                hw[0], hw[1])
    return out1, out2


def multi_scale_size(imgsz: int, shape: Sequence[int], gs: int = 32, rng=random,
                     runs_at: Optional[Callable[[int], bool]] = None) -> Tuple[int, int]:
    """The size ``--multi-scale`` resizes this step's batch to (Train.py:397-400), with integer arguments to ``randrange``
    (the reference passes ``imgsz * 0.5`` and ``imgsz * 1.5 + gs``, floats that Python >= 3.12 refuses):

        sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5) + gs) // gs * gs
        sf = sz / max(shape)
        ns = [math.ceil(x * sf / gs) * gs for x in shape]          # shape itself when sf == 1

    shape is ``imgs.shape[2:]`` of the pre-processed batch; the result goes to ``preprocess_batch(..., size=ns)``.  Exactly ONE
    draw is taken from rng per call, so the rest of the loop's ``random`` stream (the augmentation) stays where the reference's is.

    runs_at (``Model.runs_at``): where it refuses the drawn sz, sz moves to the nearest accepted size among those the draw
    can give (the gs grid from ``int(imgsz * 0.5) // gs * gs`` to ``(int(imgsz * 1.5) + gs - 1) // gs * gs``), the larger one on a
    tie; ValueError if it accepts none of them.  This CHANGES the distribution: the reference draws the grid sizes uniformly
    (an end size less often where the range does not start or end on the grid), here every refused size adds its probability to its nearest accepted neighbour - for a model
    built at 512 with imgsz 512 and gs 64, the draws of 256 .. 448 all land on 512, which then takes 5/9 of the steps instead
    of 1/9, and 576 .. 768 keep theirs.  Without runs_at the distribution is the reference's."""
    lo, hi = int(imgsz * 0.5), int(imgsz * 1.5) + gs
    sz = rng.randrange(lo, hi) // gs * gs
    if runs_at is not None and not runs_at(sz):
        ok = [s for s in range(lo // gs * gs, (hi - 1) // gs * gs + 1, gs) if runs_at(s)]
        if not ok:
            raise ValueError(f"no size of the gs = {gs} grid between {lo // gs * gs} and {(hi - 1) // gs * gs} is accepted by runs_at")
        sz = min(ok, key=lambda s: (abs(s - sz), -s))
    sf = sz / max(shape)
    if sf == 1:
        return tuple(int(x) for x in shape)
    return tuple(math.ceil(x * sf / gs) * gs for x in shape)
