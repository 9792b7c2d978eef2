"""Write tests/golden/sam.pt: the reference's own `SAM` (basics/utils/sam.py) around torch.optim.SGD(nesterov, momentum 0.937)
and torch.optim.Adam, run on CPU on six small tensors with prescribed gradients.  Runs only where the reference source tree
is importable (the build machine); it reads oracle.gen_golden.import_reference() for the module stubs, as
tools/gen_sampling_golden.py does, and changes nothing under oracle/.

The fixture holds data only.  Shared by all cases: `sizes`, `group_of` (the group of each tensor), `p0` (six float32 tensors
whose sizes are no multiples of 4, except the 64, stored end to end as one; tests/sam_ref.split takes them apart), `g1` / `g2`
(STEPS rows of the same layout: the gradient at w and the one at w + e(w) of every step).  Three groups: decayed matrices and
undecayed 1-D parameters, as set_weight_decay splits them (basics/optimizer.py:35-49), and the biases as a group of their own
with another learning rate (Train.py:129-136), so that a wrong chunk -> group map shows.

Per case (`kind` sgd / adam x `adaptive` False / True x `rho` 0.05 / 2.0; the large rho makes e(w) comparable with w, so
that a wrong factor cannot hide under the rounding of w): `groups` (the hyper-parameters of each group), and for float32
(`f32`) and for the same class run on float64 tensors (`f64`) the per-step `norm`, `first` (parameters after first_step) and
`second` (parameters after second_step), each STEPS rows of the six tensors end to end; `dist`: per step, the distance of the
float32 run from the float64 one - `norm` relative to the float64 norm, `first` / `second` per tensor relative to
max|float64| + 1e-5.

tests/sam_ref.Sam64 must reproduce the float64 records within 1e-12 (same relative measure) before anything is stored.

usage: python tools/gen_sam_golden.py
"""
from __future__ import annotations

import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import sam_ref as SR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sam.pt")
SIZES = (1, 3, 13, 35, 64, 101)
GROUP_OF = (2, 1, 0, 0, 1, 0)             # 0: decayed, 1: 1-D / not decayed, 2: biases
STEPS = 3


def groups_of(kind, rho, adaptive):
    base = [dict(lr=0.01, weight_decay=0.00048), dict(lr=0.02, weight_decay=0.0), dict(lr=0.05, weight_decay=0.0)]
    for g in base:
        g.update(rho=rho, adaptive=adaptive)
        if kind == "sgd":
            g.update(momentum=0.937, nesterov=True)
        else:
            g.update(lr=g["lr"] * 0.1, betas=(0.937, 0.999), eps=1e-8)
    return base


def run_reference(SAM, kind, groups, p0, g1, g2, dtype):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]
    pg = [dict(params=[p for p, k in zip(ps, GROUP_OF) if k == gi], **{k: v for k, v in g.items() if k not in ("rho", "adaptive")})
          for gi, g in enumerate(groups)]
    kw = dict(momentum=0.937, nesterov=True, lr=0.01) if kind == "sgd" else dict(lr=1e-3)
    opt = SAM(pg, torch.optim.SGD if kind == "sgd" else torch.optim.Adam, rho=groups[0]["rho"], adaptive=groups[0]["adaptive"], **kw)
    out = dict(norm=[], first=[], second=[])
    for s in range(STEPS):
        for p, g in zip(ps, g1[s]):
            p.grad = g.to(dtype).clone()
        out["norm"].append(opt._grad_norm().detach().clone())
        opt.first_step(zero_grad=True)
        out["first"].append([p.detach().clone() for p in ps])
        for p, g in zip(ps, g2[s]):
            p.grad = g.to(dtype).clone()
        opt.second_step(zero_grad=True)
        out["second"].append([p.detach().clone() for p in ps])
    return out


def packed(r):
    """one tensor per record: norm (STEPS), first / second (STEPS, sum of SIZES) - sam_ref.split takes them apart again"""
    return dict(norm=torch.stack(r["norm"]), first=torch.stack([torch.cat(x) for x in r["first"]]),
                second=torch.stack([torch.cat(x) for x in r["second"]]))


def rel(a, b):
    """|a - b| relative to max|b| + 1e-5, b the float64 side"""
    return float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-5)


def main():
    import_reference()
    SAM = importlib.import_module("reference.basics.utils.sam").SAM
    gen = torch.Generator().manual_seed(17)
    p0 = [torch.randn(n, generator=gen) * 0.5 for n in SIZES]
    g1 = [[torch.randn(n, generator=gen) * 0.1 for n in SIZES] for _ in range(STEPS)]
    g2 = [[torch.randn(n, generator=gen) * 0.1 for n in SIZES] for _ in range(STEPS)]
    cases, worst64 = [], 0.0
    for kind in ("sgd", "adam"):
        for adaptive in (False, True):
            for rho in (0.05, 2.0):
                groups = groups_of(kind, rho, adaptive)
                r32 = run_reference(SAM, kind, groups, p0, g1, g2, torch.float32)
                r64 = run_reference(SAM, kind, groups, p0, g1, g2, torch.float64)
                # the restatement must be the reference's float64 run before anything is stored
                ref = SR.Sam64(kind, p0, GROUP_OF, groups)
                for s in range(STEPS):
                    n = ref.first_step(g1[s])
                    e = [abs(float(n) - float(r64["norm"][s])) / float(r64["norm"][s])]
                    e += [rel(a, b) for a, b in zip(ref.p, r64["first"][s])]
                    ref.second_step(g2[s])
                    e += [rel(a, b) for a, b in zip(ref.p, r64["second"][s])]
                    worst64 = max(worst64, max(e))
                    assert max(e) <= 1e-12, (kind, adaptive, rho, s, e)
                dist = dict(norm=[abs(float(a) - float(b)) / float(b) for a, b in zip(r32["norm"], r64["norm"])],
                            first=[[rel(a, b) for a, b in zip(x, y)] for x, y in zip(r32["first"], r64["first"])],
                            second=[[rel(a, b) for a, b in zip(x, y)] for x, y in zip(r32["second"], r64["second"])])
                tag = f"{kind}_{'adaptive' if adaptive else 'plain'}_rho{rho}"
                ratio = max(float((f - o.double()).abs().max()) / float(o.abs().max())
                            for f, o in zip(r64["first"][0], p0))
                print(f"[sam golden] {tag}: norms {[round(float(n), 6) for n in r64['norm']]}; max|e_w| / max|w| at step 0 up to "
                      f"{ratio:.3f}; f32 vs f64: norm {max(dist['norm']):.2e}, first {max(map(max, dist['first'])):.2e}, "
                      f"second {max(map(max, dist['second'])):.2e}")
                cases.append(dict(tag=tag, kind=kind, adaptive=adaptive, rho=rho, groups=groups, f32=packed(r32), f64=packed(r64),
                                  dist=dist))
    torch.save(dict(sizes=SIZES, group_of=GROUP_OF, steps=STEPS, p0=torch.cat(p0), g1=torch.stack([torch.cat(g) for g in g1]),
                    g2=torch.stack([torch.cat(g) for g in g2]), cases=cases), OUT)
    print(f"[sam golden] restatement vs the reference's float64 run: worst {worst64:.2e} (required 1e-12); "
          f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
