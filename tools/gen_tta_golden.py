"""Write tests/golden/tta.pt: the reference's own pieces of test-time augmentation (basics/models/model.py:155-184) on small
tensors.  Runs only where the reference source tree is importable (the build machine); it reads
oracle.gen_golden.import_reference() for the module stubs and changes nothing under oracle/.

Two lists are recorded.  ``scale``: ``scale_img`` of basics/utils/torch_utils.py:249-259 called on f32 tensors - scales 0.83
and 0.67, odd sizes, a rectangle, ``gs`` 32 and 64, ``same_shape`` and the ratio-1 return.  ``deflip``: lines 178-182 of
basics/models/model.py - the de-scale and de-flip, which exist only inside ``Model.forward`` - executed from the reference's
source file on small ``yi`` tensors for every scale and flip.  tests/tta_ref.py must reproduce every result exactly, or
nothing is written.

usage: python tools/gen_tta_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys
import textwrap

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import tta_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tta.pt")

# (name, shape, ratio, same_shape, gs)
SCALE_CASES = [("sq36_083_gs32", (1, 1, 36, 36), 0.83, False, 32),
               ("odd37x29_067_gs32", (1, 1, 37, 29), 0.67, False, 32),
               ("rect48x72_083_gs64", (1, 1, 48, 72), 0.83, False, 64),
               ("rect24x72_067_gs32", (1, 1, 24, 72), 0.67, False, 32),
               ("b2_33x35_067_same_shape", (2, 1, 33, 35), 0.67, True, 32),
               ("c3_16x16_ratio1", (1, 3, 16, 16), 1.0, False, 32)]
DEFLIP_LINES = (178, 182)        # basics/models/model.py, 1-based, inclusive
IMG_SIZE = (96, 128)


def main():
    model_mod = import_reference()[0]
    TU = importlib.import_module("reference.basics.utils.torch_utils")
    lines = open(model_mod.__file__).read().splitlines()[DEFLIP_LINES[0] - 1: DEFLIP_LINES[1]]
    assert lines[0].strip().startswith("yi[..., :4] /= si") and "img_size[1] - yi[..., 0]" in lines[-1], lines
    deflip_code = compile(textwrap.dedent("\n".join(lines)), model_mod.__file__, "exec")
    g = torch.Generator().manual_seed(15)
    scale = []
    for name, shape, ratio, same, gs in SCALE_CASES:
        img = torch.rand(*shape, generator=g)
        out = TU.scale_img(img.clone(), ratio, same, gs)
        mine = tta_ref.scale_img(img.clone(), ratio, same, gs)
        assert out.shape == mine.shape and torch.equal(out, mine), name
        if ratio != 1.0 and not same:       # the explicit padded size is the same call
            assert torch.equal(tta_ref.scale_img(img.clone(), ratio, padded=tuple(out.shape[2:])), out), name
        print(f"[tta golden] {name}: {tuple(shape)} -> {tuple(out.shape)}")
        scale.append(dict(name=name, img=img, ratio=ratio, same_shape=same, gs=gs, out=out))
    deflip = []
    for si in (1, 0.83, 0.67):
        for fi in (None, 2, 3):
            yi = torch.rand(2, 6, 13, generator=g) * 120.0
            ns = dict(yi=yi.clone(), si=si, fi=fi, img_size=IMG_SIZE)
            exec(deflip_code, ns)
            mine = tta_ref.descale_deflip(yi, si, fi, IMG_SIZE)
            assert torch.equal(mine, ns["yi"]), (si, fi)
            deflip.append(dict(yi=yi, si=si, fi=fi, img_size=IMG_SIZE, out=ns["yi"]))
    torch.save(dict(scale=scale, deflip=deflip), OUT)
    size = os.path.getsize(OUT)
    print(f"[tta golden] wrote {OUT} ({size} bytes)")
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
