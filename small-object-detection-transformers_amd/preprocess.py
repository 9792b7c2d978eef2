"""Input pre-processing of the reference's training / evaluation loop on the device.

Train.py:364-374 moves the uint8 batch to the GPU, converts it with ``.float() / 255.0`` and, when the images were loaded at
``train_img_size = down_factor x test_img_size`` (defaults 1024 / 512, Train.py:94,612-613), shrinks RGB and IR with
``F.interpolate(..., mode='bilinear', align_corners=True)``: four full-tensor ATen kernels and two f32 intermediates at the
loaded resolution.  ``preprocess_batch`` is that in ONE launch (csrc/preprocess.hip, ``sodt_preprocess_u8``): uint8 planes
in, f32 planes out, the layout ``Model.forward`` / the front-end kernel read.  test.py:124-129 is the ``down_factor=1`` case.

``--multi-scale`` (Train.py:396-402) then draws a size per step and resizes both batches once more with
``F.interpolate(..., size=ns, mode='bilinear', align_corners=False)``.  ``multi_scale_size`` is the draw, ``preprocess_batch(...,
size=ns)`` the resize, still in ONE launch from the uint8 batch (csrc/multiscale.hip, ``sodt_preprocess_u8_ms``).

``--quad`` (Train.py:223, ``LoadImagesAndLabels.collate_fn4``, basics/utils/datasets.py:637-664) turns a batch of 4n images into n
images of twice the side on the host, per group of four either the first one zoomed 2x or the four tiled 2 x 2.  Here the loader
keeps its plain ``collate_fn``: ``quad_modes`` is the draw, ``quad_targets`` the labels, ``preprocess_batch(..., quad=modes)`` the
f32 inputs in ONE launch from the 4n uint8 images (csrc/quad.hip, ``sodt_preprocess_u8_quad``), and ``quad_batch`` the uint8 quad
batch itself (``sodt_quad_u8``) for ``SRLoss`` under ``--super``.
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


QUAD_MAX_GROUPS = 64      # the modes travel to the kernels as the bits of one 64-bit argument


def _check_u8_pair(imgs: torch.Tensor, irs: torch.Tensor, who: str) -> None:
    if imgs.dtype != torch.uint8 or irs.dtype != torch.uint8:
        raise TypeError(f"{who} takes the uint8 batch of the data loader (Train.py:362)")
    if not imgs.is_cuda or not irs.is_cuda:
        raise RuntimeError(f"{who} needs the batch on the GPU (Train.py:364: imgs.to(device)); there is no CPU fallback")
    if imgs.dim() != 4 or irs.dim() != 4 or imgs.shape[0] != irs.shape[0] or imgs.shape[2:] != irs.shape[2:]:
        raise ValueError("imgs and irs must be (B, C, H, W) with the same batch and size")


def _quad_mask(modes, B: int) -> int:
    """modes of quad_modes for a batch of B -> the zoom_mask of the C entries (bit g: group g zooms)"""
    if B < 4 or B // 4 > QUAD_MAX_GROUPS:
        raise ValueError(f"--quad needs 4 .. {4 * QUAD_MAX_GROUPS + 3} samples (1 .. {QUAD_MAX_GROUPS} groups of four), got {B}")
    if not isinstance(modes, (tuple, list)) or len(modes) != B // 4 or any(not isinstance(m, bool) for m in modes):
        raise ValueError(f"modes must be {B // 4} bools, one per group of four (quad_modes({B})), got {modes!r}")
    return sum(1 << g for g, m in enumerate(modes) if m)


def quad_modes(B: int, rng=random) -> Tuple[bool, ...]:
    """The draws of collate_fn4 for a batch of B samples (datasets.py:645-647): one ``rng.random() < 0.5`` per group of four, in
    group order, True = zoom the group's first sample, False = tile the four.  Exactly B // 4 draws and nothing else are taken
    from rng, so a loop whose loader runs with ``num_workers=0`` keeps the reference's ``random`` stream (with worker processes
    the reference draws from the workers' own generators and there is nothing to align)."""
    if isinstance(B, bool) or not isinstance(B, int) or B < 4 or B // 4 > QUAD_MAX_GROUPS:
        raise ValueError(f"--quad needs 4 .. {4 * QUAD_MAX_GROUPS + 3} samples (1 .. {QUAD_MAX_GROUPS} groups of four), got {B!r}")
    return tuple(rng.random() < 0.5 for _ in range(B // 4))


def quad_targets(targets: torch.Tensor, modes: Sequence[bool]) -> torch.Tensor:
    """The labels of collate_fn4 (datasets.py:642-662) from those of the plain ``collate_fn``: targets f32 (nt, 6) =
    (image, cls, x, y, w, h) with rows in image order, on any device.  A zoom group keeps the rows of its first sample
    unchanged; a tile group keeps all four, ``(label + ho + wo) * s`` in f32 in the reference's order (sample 4g+1 lies below:
    y + 1, 4g+2 to the right: x + 1, 4g+3 both; then x, y, w, h halve).  Column 0 becomes the group.  Rows of samples 1 .. 3 of a
    zoom group and of the remainder past 4 * len(modes) disappear.  Row order: group, source sample, source order."""
    n = len(modes)
    if n < 1 or n > QUAD_MAX_GROUPS or any(not isinstance(m, bool) for m in modes):
        raise ValueError(f"modes must be 1 .. {QUAD_MAX_GROUPS} bools (quad_modes), got {modes!r}")
    if targets.dim() != 2 or targets.shape[1] != 6 or targets.dtype != torch.float32:
        raise ValueError("targets must be f32 (nt, 6) = (image, cls, x, y, w, h) (datasets.py:630-634)")
    dev = targets.device
    idx = targets[:, 0].long()
    zoom = torch.tensor(list(modes), dtype=torch.bool, device=dev)
    g, k = idx.div(4, rounding_mode="floor"), idx % 4
    keep = (idx >= 0) & (idx < 4 * n)
    keep &= ~zoom[g.clamp(0, n - 1)] | (k == 0)
    t, g, k = targets[keep], g[keep], k[keep]
    ho = torch.zeros_like(t)
    wo = torch.zeros_like(t)
    ho[:, 3] = ((k == 1) | (k == 3)).float()
    wo[:, 2] = (k >= 2).float()
    s = torch.tensor([1, 1, .5, .5, .5, .5], dtype=torch.float32, device=dev)
    out = torch.where(zoom[g][:, None], t, (t + ho + wo) * s)
    out[:, 0] = g.float()
    return out


def quad_batch(imgs: torch.Tensor, irs: torch.Tensor, modes: Sequence[bool]) -> Tuple[torch.Tensor, torch.Tensor]:
    """imgs, irs: uint8 (B, C, H, W) on the GPU -> the uint8 (B // 4, C, 2H, 2W) batches collate_fn4 returns under modes, in ONE
    launch (``sodt_quad_u8``): what ``SRLoss`` takes under ``--super``, and what ``--multi-scale`` resizes."""
    _check_u8_pair(imgs, irs, "quad_batch")
    mask = _quad_mask(modes, imgs.shape[0])
    imgs, irs = imgs.contiguous(), irs.contiguous()
    B, c1, H, W = imgs.shape
    c2 = irs.shape[1]
    out1 = torch.empty(B // 4, c1, 2 * H, 2 * W, device=imgs.device, dtype=torch.uint8)
    out2 = torch.empty(B // 4, c2, 2 * H, 2 * W, device=imgs.device, dtype=torch.uint8)
    ops._launch("sodt_quad_u8", imgs.data_ptr(), irs.data_ptr(), out1.data_ptr(), out2.data_ptr(), B, c1, c2, H, W, mask)
    return out1, out2


def preprocess_batch(imgs: torch.Tensor, irs: torch.Tensor, down_factor: int = 1,
                     size: Union[None, int, Sequence[int]] = None,
                     quad: Optional[Sequence[bool]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """imgs, irs: uint8 (B, C, H, W) on the GPU -> f32 (B, C, H // down_factor, W // down_factor) in [0, 1].

    size (an int or (h, w)): the ``ns`` of ``--multi-scale`` (Train.py:400-402) - the result is resized once more, half-pixel
    bilinear, to (B, C, h, w), in the same single launch.  None, or the shrunk size itself, is the call without it (the
    reference skips the interpolation when ``sf == 1``).

    quad (the modes of ``quad_modes``): the batch is the loader's plain 4n-sample batch and the result is that of the call on
    ``quad_batch(imgs, irs, quad)``, bit for bit: f32 (B // 4, C, 2H // down_factor, 2W // down_factor), in ONE launch from the
    4n images with no uint8 intermediate (``sodt_preprocess_u8_quad``).  With a size other than that shape it is two
    launches, ``sodt_quad_u8`` and ``sodt_preprocess_u8_ms``."""
    _check_u8_pair(imgs, irs, "preprocess_batch")
    if down_factor < 1:
        raise ValueError("down_factor >= 1 (Train.py:94: int(train_img_size / test_img_size))")
    hw = None if size is None else _size_hw(size)
    if quad is not None:
        mask = _quad_mask(quad, imgs.shape[0])
        B, c1, H, W = imgs.shape
        Ho, Wo = 2 * H // down_factor, 2 * W // down_factor
        if hw is not None and hw != (Ho, Wo):
            return preprocess_batch(*quad_batch(imgs, irs, quad), down_factor, size=hw)
        imgs, irs = imgs.contiguous(), irs.contiguous()
        out1 = torch.empty(B // 4, c1, Ho, Wo, device=imgs.device, dtype=torch.float32)
        out2 = torch.empty(B // 4, irs.shape[1], Ho, Wo, device=imgs.device, dtype=torch.float32)
        ops._launch("sodt_preprocess_u8_quad", imgs.data_ptr(), irs.data_ptr(), out1.data_ptr(), out2.data_ptr(), B, c1,
                    irs.shape[1], H, W, Ho, Wo, mask)
        return out1, out2
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
