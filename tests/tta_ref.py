"""CPU torch restatement of the reference's test-time augmentation (basics/models/model.py:155-184): ``scale_img``
(basics/utils/torch_utils.py:249-259) with the padded size as an explicit argument, the de-scale / de-flip of model.py:178-182,
and the whole composition around any plain forward.  tools/gen_tta_golden.py asserts that the first two reproduce the
reference's own code exactly on the cases of tests/golden/tta.pt; the tests and tools/mb_tta.py use them on further shapes."""
import math

import torch
import torch.nn.functional as F


def padded_size(hw, ratio, gs):
    """torch_utils.py:258"""
    return tuple(math.ceil(x * ratio / gs) * gs for x in hw)


def scale_img(img, ratio=1.0, same_shape=False, gs=32, padded=None):
    """torch_utils.py:249-259; ``padded`` (Hp, Wp) replaces the gs multiple (and same_shape) where given."""
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode="bilinear", align_corners=False)
    if padded is not None:
        h, w = padded
    elif not same_shape:
        h, w = padded_size((h, w), ratio, gs)
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=0.447)


def flip_scale(img, fi, ratio, padded):
    """model.py:161-162 for one modality: the flip comes before the resize"""
    return scale_img(img.flip(fi) if fi else img, ratio, padded=padded)


def descale_deflip(yi, si, fi, img_size):
    """model.py:178-182 on a copy of yi (..., no): img_size = (height, width) of the ORIGINAL input"""
    yi = yi.clone()
    yi[..., :4] /= si
    if fi == 2:
        yi[..., 1] = img_size[0] - yi[..., 1]
    elif fi == 3:
        yi[..., 0] = img_size[1] - yi[..., 0]
    return yi


def augmented_forward(forward, x, ir, scales, flips, padded, make_inputs=None):
    """model.py:155-184: ``forward(xi, iri)`` is the plain eval forward returning z (B, rows, no) on any device; padded[k] is
    the padded size of pass k (ignored where the scale is 1); ``make_inputs(k) -> (xi, iri)`` replaces the torch calls that make
    the pass's inputs.  The de-scale / de-flip runs on the CPU; returns the concatenated z there."""
    img_size = x.shape[-2:]
    y = []
    for k, (si, fi) in enumerate(zip(scales, flips)):
        if make_inputs is not None:
            xi, iri = make_inputs(k)
        else:
            xi, iri = flip_scale(x, fi, si, padded[k]), flip_scale(ir, fi, si, padded[k])
        y.append(descale_deflip(forward(xi, iri).cpu(), si, fi, img_size))
    return torch.cat(y, 1)
