"""Test-time augmentation (basics/models/model.py:155-184, the ``--augment`` of basics/test.py): the host side.

The augmented forward is three pieces of the reference - ``scale_img`` (basics/utils/torch_utils.py:249-259) on the flipped
input, a plain eval forward, the de-scale / de-flip of model.py:178-182 - and the engine runs the first and the last as one
launch each (csrc/tta.hip): ``sodt_tta_scale`` makes every scaled input of a call, RGB and IR, at once, and
``sodt_detect_decode_tta`` decodes each pass straight into its rows of the concatenated output.

One deviation from the reference: the padded size of a scaled copy.  The reference pads to ``ceil(side * si / gs) * gs`` with
``gs = int(model.stride.max())`` = 4, sizes its own window blocks assert on (428 and 344 pixels at 512).  ``tta_sizes`` starts
from the same formula with ``gs = max(stride, 32)`` and moves the result to the smallest size ``Model.runs_at`` accepts - more
pad pixels (0.447) to the right and below, the content itself unchanged."""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _lib as L

MAX_PASSES = L.TTA_MAX_PASSES
SCALES = (1, 0.83, 0.67)         # model.py:157
FLIPS = (None, 3, None)          # model.py:158 (2 = up-down, 3 = left-right)

Size = Tuple[int, int]


def check_passes(scales, flips) -> Tuple[Tuple[float, ...], Tuple[int, ...]]:
    """Validate ``Model.tta_scales`` / ``Model.tta_flips``: sequences of equal length, 1 .. 4 entries, every scale a number in
    (0, 1], every flip None, 2 or 3.  Returns (scales, flips) as tuples with None -> 0.  ValueError otherwise."""
    if not isinstance(scales, (tuple, list)) or not isinstance(flips, (tuple, list)):
        raise ValueError(f"tta_scales and tta_flips must be tuples or lists, got {scales!r} and {flips!r}")
    if len(scales) != len(flips):
        raise ValueError(f"tta_scales and tta_flips must have the same length, got {len(scales)} and {len(flips)}")
    if not 1 <= len(scales) <= MAX_PASSES:
        raise ValueError(f"test-time augmentation runs 1 .. {MAX_PASSES} passes, got {len(scales)}")
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not 0 < s <= 1:
            raise ValueError(f"every entry of tta_scales must be a number in (0, 1], got {s!r}")
    for f in flips:
        if f is not None and (isinstance(f, bool) or f not in (2, 3)):
            raise ValueError(f"every entry of tta_flips must be None, 2 (up-down) or 3 (left-right), got {f!r}")
    return tuple(scales), tuple(0 if f is None else int(f) for f in flips)


def tta_sizes(hw: Size, scales: Sequence[float], gs: int = 32,
              runs_at: Optional[Callable[[Size], bool]] = None) -> List[Tuple[Size, Size]]:
    """Content and padded size of every pass of an (H, W) input: one ``((h, w), (Hp, Wp))`` per scale, in order; a scale of 1
    gives ``((H, W), (H, W))``.  Pure host code.

    (h, w) = (int(H * si), int(W * si)) is the reference's (torch_utils.py:255).  (Hp, Wp) starts at the reference's
    ``ceil(side * si / gs) * gs`` (torch_utils.py:258).  Where ``runs_at`` (``Model.runs_at``) refuses that pair, the padded
    size becomes the accepted pair of smallest area among (Hp + 32 i, Wp + 32 j) up to (H, W), the smaller height on a tie;
    (H, W) itself is always a candidate, so the search ends wherever the plain forward runs.  ValueError if nothing is accepted."""
    H, W = hw
    out = []
    for si in scales:
        if si == 1:
            out.append(((H, W), (H, W)))
            continue
        h, w = int(H * si), int(W * si)
        if h < 1 or w < 1:
            raise ValueError(f"scale {si} leaves no pixel of a {H} x {W} input")
        H0, W0 = (math.ceil(x * si / gs) * gs for x in (H, W))
        pad = (H0, W0)
        if runs_at is not None and not runs_at(pad):
            cand = {(a, b) for a in range(H0, H + 1, 32) for b in range(W0, W + 1, 32)} | {(H, W)}
            pad = next((c for c in sorted(cand, key=lambda c: (c[0] * c[1], c[0])) if runs_at(c)), None)
            if pad is None:
                raise ValueError(f"no padded size between {H0} x {W0} and {H} x {W} is accepted by runs_at (scale {si})")
        out.append(((h, w), pad))
    return out


def _check_img(img: torch.Tensor, who: str) -> None:
    if not img.is_cuda:
        raise RuntimeError(f"{who} needs its input on the GPU: there is no CPU fallback")
    if img.dim() != 4 or img.dtype != torch.float32:
        raise ValueError(f"{who} takes f32 (B, C, H, W) tensors, got {tuple(img.shape)} {img.dtype}")


def scale_pair(x: torch.Tensor, ir: Optional[torch.Tensor],
               passes: Sequence[Tuple[Size, Size, Optional[int]]]) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """The inputs of the augmented passes, both modalities and all passes in ONE launch (``sodt_tta_scale``).  x, ir: f32
    (B, C, H, W) on the GPU (ir may be None); passes: up to four ``((h, w), (Hp, Wp), flip)`` - the input is flipped along
    dimension ``flip`` (None / 0, 2 or 3), resized to (h, w) half-pixel bilinear and padded with 0.447 to (Hp, Wp).  Returns one
    ``(xi, iri)`` per pass, f32 (B, C, Hp, Wp)."""
    from . import ops
    _check_img(x, "scale_pair")
    if ir is not None:
        _check_img(ir, "scale_pair")
        if ir.shape[0] != x.shape[0] or ir.shape[2:] != x.shape[2:]:
            raise ValueError("x and ir must have the same batch and size")
        ir = ir.contiguous()
    x = x.contiguous()
    if not 1 <= len(passes) <= MAX_PASSES:
        raise ValueError(f"1 .. {MAX_PASSES} passes per launch, got {len(passes)}")
    B = x.shape[0]
    outs, table = [], []
    for (h, w), (Hp, Wp), flip in passes:
        flip = 0 if flip is None else flip
        if flip not in (0, 2, 3) or not (0 < h <= Hp and 0 < w <= Wp):
            raise ValueError(f"bad pass: content {h} x {w}, padded {Hp} x {Wp}, flip {flip}")
        o1 = torch.empty(B, x.shape[1], Hp, Wp, device=x.device, dtype=torch.float32)
        o2 = None if ir is None else torch.empty(B, ir.shape[1], Hp, Wp, device=x.device, dtype=torch.float32)
        outs.append((o1, o2))
        table.append((o1, o2, (h, w), flip))
    ops.tta_scale(x, ir, table)
    return outs


def scale_img(img: torch.Tensor, ratio: float = 1.0, same_shape: bool = False, gs: int = 32) -> torch.Tensor:
    """``scale_img`` of basics/utils/torch_utils.py:249-259 on a device tensor, one launch: img f32 (B, C, H, W) resized to
    (int(H * ratio), int(W * ratio)) and padded with 0.447 to the ``gs`` multiple above ``side * ratio`` (to (H, W) itself
    with ``same_shape``).  ``ratio == 1.0`` returns img itself, as there.  A ``same_shape`` call that would have to crop
    (ratio > 1) is refused."""
    if ratio == 1.0:
        return img
    _check_img(img, "scale_img")
    H, W = img.shape[2:]
    s = (int(H * ratio), int(W * ratio))
    pad = (H, W) if same_shape else tuple(math.ceil(x * ratio / gs) * gs for x in (H, W))
    if s[0] > pad[0] or s[1] > pad[1]:
        raise ValueError(f"scale_img(ratio={ratio}, same_shape=True) crops {s} to {pad}: not built")
    return scale_pair(img, None, [(s, pad, None)])[0][0]
