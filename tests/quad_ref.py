"""CPU torch restatement of ``LoadImagesAndLabels.collate_fn4`` (basics/utils/datasets.py:637-664, the loader of ``--quad``) with
the per-group draws as an argument instead of ``random.random() < 0.5``.  The zoom is spelled as the reference spells it,
``F.interpolate(x.float(), scale_factor=2., mode='bilinear', align_corners=False).type(uint8)``, so this file - not an integer
formula - is what the device kernels are held to.  tools/gen_quad_golden.py asserts that it reproduces the reference's own
function exactly on the cases of tests/golden/quad.pt; the tests and tools/mb_quad.py use it on further shapes."""
import torch
import torch.nn.functional as F


def _zoom(x):
    return F.interpolate(x.unsqueeze(0).float(), scale_factor=2., mode="bilinear", align_corners=False)[0].type(x.type())


def _tile(x, i):
    return torch.cat((torch.cat((x[i], x[i + 1]), 1), torch.cat((x[i + 2], x[i + 3]), 1)), 2)


def quad_ref(imgs, irs, labels, modes):
    """imgs, irs: uint8 (B, C, H, W) (or sequences of B (C, H, W) tensors); labels: B tensors f32 (nl_i, 6); modes: B // 4 bools,
    True = zoom.  Returns (uint8 (n, C, 2H, 2W), uint8 (n, C_ir, 2H, 2W), f32 (sum nl, 6)); no input is modified."""
    n = len(imgs) // 4
    assert len(modes) == n and len(irs) == len(imgs) == len(labels)
    ho = torch.tensor([[0., 0, 0, 1, 0, 0]])
    wo = torch.tensor([[0., 0, 1, 0, 0, 0]])
    s = torch.tensor([[1, 1, .5, .5, .5, .5]])
    img4, ir4, label4 = [], [], []
    for g in range(n):
        i = 4 * g
        if modes[g]:
            im, ir, l = _zoom(imgs[i]), _zoom(irs[i]), labels[i].clone()
        else:
            im, ir = _tile(imgs, i), _tile(irs, i)
            l = torch.cat((labels[i], labels[i + 1] + ho, labels[i + 2] + wo, labels[i + 3] + ho + wo), 0) * s
        l[:, 0] = g
        img4.append(im)
        ir4.append(ir)
        label4.append(l)
    return torch.stack(img4, 0), torch.stack(ir4, 0), torch.cat(label4, 0)


def plain_targets(labels):
    """The label tensor of the plain ``collate_fn`` (datasets.py:630-634): column 0 is the sample index."""
    out = []
    for i, l in enumerate(labels):
        l = l.clone()
        l[:, 0] = i
        out.append(l)
    return torch.cat(out, 0) if out else torch.zeros(0, 6)


def quad_ref_device(imgs, irs, modes):
    """The image side of quad_ref as ATen calls on whatever device the (B, C, H, W) uint8 batches live on (tools/mb_quad.py)."""
    n = imgs.shape[0] // 4
    return (torch.stack([_zoom(imgs[4 * g]) if modes[g] else _tile(imgs, 4 * g) for g in range(n)], 0),
            torch.stack([_zoom(irs[4 * g]) if modes[g] else _tile(irs, 4 * g) for g in range(n)], 0))
