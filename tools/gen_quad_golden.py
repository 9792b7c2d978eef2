"""Write tests/golden/quad.pt: the reference's own ``LoadImagesAndLabels.collate_fn4`` (basics/utils/datasets.py:637-664, the
loader of ``--quad``) on small sample lists.  Runs only where the reference source tree is importable (the build machine);
it reads oracle.gen_golden.import_reference() for the module stubs and changes nothing under oracle/.

Per case: the sample list is built (uint8 images with some 0 and some 255 pixels, 0 .. 5 labels per sample, one sample with
none), ``random`` is seeded, the reference function is called, and the inputs, the seed, the modes that seed gives (the
``random.random() < 0.5`` of each group, drawn again from the same seed) and the three outputs are recorded.  tests/quad_ref.py
must reproduce the three outputs exactly from the inputs and the modes, or nothing is written.

The reference function is called once per GROUP, on the group's four samples (the last group's call also gets the remainder
past 4n, which the function drops itself), after one seeding per case: as written it rebinds its tuple ``ir`` to the first
group's IR image (datasets.py:650 / :655), so from the second group on ``ir[i]`` indexes that image's channels and the call
raises IndexError for any batch of eight or more.  One call per group is the function's own arithmetic and its own draw, one
per call and in group order, for every group; column 0 of each call's labels (0, the call's only group) is then set to the
group's index as datasets.py:661-662 would.

usage: python tools/gen_quad_golden.py
"""
from __future__ import annotations

import importlib
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
from quad_ref import quad_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "quad.pt")

# (name, B, H, W, IR channels, modes): the case's seed is the first of 0, 1, ... whose draws are these modes
CASES = [("b4_8x8", 4, 8, 8, 3, (True,)),
         ("b8_5x7_ir1", 8, 5, 7, 1, (True, False)),
         ("b9_16x12_one_dropped", 9, 16, 12, 3, (False, True)),
         ("b4_1x9", 4, 1, 9, 3, (True,)),
         ("b12_24x40_mixed", 12, 24, 40, 1, (True, False, True)),
         ("b8_6x10_all_zoom", 8, 6, 10, 3, (True, True)),
         ("b8_6x10_all_tile", 8, 6, 10, 3, (False, False))]


def modes_of(seed, n):
    rng = random.Random(seed)
    return tuple(rng.random() < 0.5 for _ in range(n))


def samples(case, B, H, W, c_ir):
    g = torch.Generator().manual_seed(1000 + case)
    imgs = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    irs = torch.randint(0, 256, (B, c_ir, H, W), generator=g, dtype=torch.uint8)
    for x in (imgs, irs):                                     # both ends of the range in every image
        flat = x.view(B, -1)
        flat[:, 0] = 0
        flat[:, -1] = 255
        if flat.shape[1] > 4:
            flat[:, 1], flat[:, -2] = 255, 0
    labels = []
    for i in range(B):
        nl = 0 if i == 1 else int(torch.randint(0, 6, (1,), generator=g))
        l = torch.zeros(nl, 6)
        l[:, 1] = torch.randint(0, 8, (nl,), generator=g).float()
        l[:, 2:4] = torch.rand(nl, 2, generator=g)
        l[:, 4:6] = torch.rand(nl, 2, generator=g) * 0.3 + 0.01
        labels.append(l)
    return imgs, irs, labels


def main():
    import_reference()
    D = importlib.import_module("reference.basics.utils.datasets")
    cases = []
    for ci, (name, B, H, W, c_ir, want) in enumerate(CASES):
        n = B // 4
        seed = next(s for s in range(10000) if modes_of(s, n) == want)
        modes = modes_of(seed, n)
        imgs, irs, labels = samples(ci, B, H, W, c_ir)
        batch = [(imgs[i].clone(), irs[i].clone(), labels[i].clone(), f"{name}/{i}", None) for i in range(B)]
        random.seed(seed)
        outs = []
        for g in range(n):
            o = D.LoadImagesAndLabels.collate_fn4(batch[4 * g: 4 * g + 4] if g < n - 1 else batch[4 * g:])
            assert o[0].shape[0] == o[1].shape[0] == 1 and bool((o[2][:, 0] == 0).all())
            o[2][:, 0] = g
            outs.append(o)
        img4, ir4, label4 = (torch.cat([o[k] for o in outs], 0) for k in range(3))
        assert img4.dtype == ir4.dtype == torch.uint8 and img4.shape == (n, 3, 2 * H, 2 * W) and ir4.shape == (n, c_ir, 2 * H, 2 * W)
        r = quad_ref(imgs, irs, labels, modes)
        assert torch.equal(r[0], img4) and torch.equal(r[1], ir4) and torch.equal(r[2], label4), name
        assert all(int(x.min()) == 0 and int(x.max()) == 255 for x in imgs) and any(l.shape[0] == 0 for l in labels)
        print(f"[quad golden] {name}: seed {seed}, modes {modes}, {sum(l.shape[0] for l in labels)} labels in, {label4.shape[0]} out")
        cases.append(dict(name=name, imgs=imgs, irs=irs, labels=labels, seed=seed, modes=modes, img4=img4, ir4=ir4, label4=label4))
    torch.save(cases, OUT)
    size = os.path.getsize(OUT)
    print(f"[quad golden] wrote {OUT} ({size} bytes)")
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
