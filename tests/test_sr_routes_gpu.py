"""The super-resolution branch's units against float64, the way SRBranch runs them: the per-unit methods that decoder_forward /
decoder_backward / edsr_forward / edsr_backward call in sequence (sr.py: _dec_entry_* / _dec_tail_* / _head_* / _resblock_* /
_body_close_* / _up_* / _close_*), each on a branch of its own, and the EDSR(depth 2) walk through edsr_forward / edsr_backward;
then the engine's taps into and out of the branch, exactly.  The counterpart of tests/test_head_routes_gpu.py.

Gate.  bf16 routes: |T_gpu - T_A| / |T_A| <= 3 e_emul(T) + 1e-5, where A is the exact unit in float64 on the operands the route
reads and e_emul(T) = |T_B - T_A| / |T_A| with B the same float64 graph with a straight-through bf16 rounding wherever the bf16
route stores a value (tests/sr_cases.py; the list is in the docstrings of oracle.ref_torch.sr_decoder / edsr).  f32 routes: 2e-3.
The constants are block_cases'; nothing in a gate comes from a kernel.  Gated: the unit output, every input gradient, every
parameter gradient; the two slices of the concatenation and g.cu / g.a separately; out and din again on the first / last grid
row and column of every unit with a 3x3; the Upsampler stage's output by (y & 1, x & 1) parity, its weight / bias gradient rows
by plane and the input gradient of a gradient confined to one parity.  Where no store point reaches a tensor (sr_cases.untouched)
e_emul is 0 and the gate is the floor.

Per case the test also pins the launches by family (sr_cases.EXPECTED: a family that is not listed must not launch), that a
second forward reproduces the output bit for bit (the buffers are reused), and that a second backward without clearing the
gradients doubles every parameter gradient and reproduces the input gradients.

test_engine_taps: on Model(sr=True) the segments Engine._sr_segs builds give bit for bit the Decoder output of the same features
materialised with torch, and Engine._add_extra returns g.low / g.x to the tapped features' gradients exactly (small integers).

Measured on an MI355X, worst tensor of each group as err / gate (3 e_emul + 1e-5, or 2e-3 on f32; the floor where e_emul is 0),
with e_emul in DESIGN.md section 2, "SR units against float64":

    case                          out (+subsets)     din (+subsets)     weight gradients   bias gradients     second backward
    dec_entry-B2-8x12-bf16        1.7e-03 / 5.0e-03  2.4e-03 / 7.1e-03  1.7e-03 / 5.0e-03                     2.4e-03 / 7.1e-03
    dec_entry-B1-6x10-bf16        2.2e-03 / 6.5e-03  2.4e-03 / 7.1e-03  1.7e-03 / 5.1e-03                     2.4e-03 / 7.1e-03
    dec_entry_engine-B2-8x12-bf16 2.1e-03 / 6.4e-03  2.4e-03 / 7.1e-03  1.6e-03 / 4.7e-03                     2.4e-03 / 7.1e-03
    dec_tail-B2-8x12-bf16         2.9e-03 / 8.8e-03  4.9e-02 / 1.5e-01  4.7e-02 / 1.4e-01  8.2e-09 / 1.0e-05  4.7e-02 / 1.4e-01
    dec_tail-B1-6x10-bf16         2.9e-03 / 8.7e-03  3.9e-02 / 1.2e-01  2.9e-02 / 8.8e-02  0.0e+00 / 1.0e-05  3.9e-02 / 1.2e-01
    head-B2-7x6-bf16              1.7e-03 / 5.0e-03  2.5e-03 / 7.6e-03  1.8e-03 / 5.4e-03  1.5e-03 / 4.5e-03  2.5e-03 / 7.6e-03
    head-B1-10x36-bf16            1.7e-03 / 5.0e-03  2.5e-03 / 7.4e-03  1.8e-03 / 5.4e-03  1.8e-03 / 5.3e-03  2.5e-03 / 7.4e-03
    head-B1-18x34-bf16            1.6e-03 / 5.0e-03  2.5e-03 / 7.4e-03  1.8e-03 / 5.4e-03  1.7e-03 / 5.2e-03  2.5e-03 / 7.4e-03
    resblock-B2-7x6-bf16          1.8e-03 / 5.5e-03  1.8e-03 / 5.5e-03  1.7e-03 / 5.1e-03  1.7e-03 / 5.2e-03  1.8e-03 / 5.5e-03
    resblock-B1-10x36-bf16        1.8e-03 / 5.4e-03  1.9e-03 / 5.6e-03  1.7e-03 / 5.1e-03  2.1e-03 / 6.2e-03  1.9e-03 / 5.6e-03
    resblock-B1-18x34-bf16        1.8e-03 / 5.3e-03  1.8e-03 / 5.3e-03  1.7e-03 / 5.0e-03  2.0e-03 / 5.9e-03  2.0e-03 / 5.9e-03
    body_close-B2-7x6-bf16        1.7e-03 / 5.1e-03  1.6e-03 / 4.9e-03  4.3e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.6e-03 / 4.9e-03
    body_close-B1-10x36-bf16      1.6e-03 / 4.9e-03  1.6e-03 / 5.0e-03  8.1e-08 / 1.0e-05  7.7e-09 / 1.0e-05  1.6e-03 / 5.0e-03
    body_close-B1-18x34-bf16      1.7e-03 / 5.2e-03  1.6e-03 / 4.8e-03  9.0e-08 / 1.0e-05  1.3e-08 / 1.0e-05  1.6e-03 / 4.8e-03
    up-B2-7x6-bf16                1.7e-03 / 5.0e-03  2.6e-03 / 7.9e-03  4.4e-08 / 1.0e-05  6.7e-09 / 1.0e-05  2.6e-03 / 7.9e-03
    up-B1-10x36-bf16              1.7e-03 / 5.0e-03  2.7e-03 / 8.2e-03  8.2e-08 / 1.0e-05  2.1e-08 / 1.0e-05  2.7e-03 / 8.2e-03
    close-ch3-B2-7x6-bf16         1.1e-07 / 1.0e-05  1.7e-03 / 5.1e-03  4.0e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.7e-03 / 5.1e-03
    close-ch3-B1-18x34-bf16       1.2e-07 / 1.0e-05  1.7e-03 / 5.2e-03  7.4e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.7e-03 / 5.2e-03
    close-ch4-B2-7x6-bf16         1.1e-07 / 1.0e-05  1.8e-03 / 5.3e-03  4.1e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.8e-03 / 5.3e-03
    close-ch4-B1-18x34-bf16       1.2e-07 / 1.0e-05  1.7e-03 / 5.0e-03  7.4e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.7e-03 / 5.0e-03
    dec_entry-B2-8x12-f32         3.7e-07 / 2.0e-03  2.4e-07 / 2.0e-03  1.5e-07 / 2.0e-03                     2.4e-07 / 2.0e-03
    dec_entry-B1-6x10-f32         3.7e-07 / 2.0e-03  2.3e-07 / 2.0e-03  1.2e-07 / 2.0e-03                     2.3e-07 / 2.0e-03
    dec_entry_engine-B2-8x12-f32  3.6e-07 / 2.0e-03  2.4e-07 / 2.0e-03  1.4e-07 / 2.0e-03                     2.4e-07 / 2.0e-03
    dec_tail-B2-8x12-f32          9.2e-07 / 2.0e-03  7.4e-07 / 2.0e-03  9.2e-07 / 2.0e-03  8.2e-09 / 2.0e-03  9.2e-07 / 2.0e-03
    dec_tail-B1-6x10-f32          9.0e-07 / 2.0e-03  7.2e-07 / 2.0e-03  8.7e-07 / 2.0e-03  0.0e+00 / 2.0e-03  8.7e-07 / 2.0e-03
    head-B2-7x6-f32               4.0e-07 / 2.0e-03  4.0e-07 / 2.0e-03  6.9e-08 / 2.0e-03  1.0e-08 / 2.0e-03  4.0e-07 / 2.0e-03
    head-B1-10x36-f32             4.2e-07 / 2.0e-03  4.2e-07 / 2.0e-03  1.6e-07 / 2.0e-03  1.5e-08 / 2.0e-03  4.2e-07 / 2.0e-03
    head-B1-18x34-f32             4.2e-07 / 2.0e-03  4.2e-07 / 2.0e-03  1.6e-07 / 2.0e-03  2.9e-08 / 2.0e-03  4.2e-07 / 2.0e-03
    resblock-B2-7x6-f32           2.5e-07 / 2.0e-03  2.4e-07 / 2.0e-03  4.3e-07 / 2.0e-03  4.5e-07 / 2.0e-03  4.5e-07 / 2.0e-03
    resblock-B1-10x36-f32         2.8e-07 / 2.0e-03  2.8e-07 / 2.0e-03  5.1e-07 / 2.0e-03  4.9e-07 / 2.0e-03  5.1e-07 / 2.0e-03
    resblock-B1-18x34-f32         2.9e-07 / 2.0e-03  2.8e-07 / 2.0e-03  4.9e-07 / 2.0e-03  5.5e-07 / 2.0e-03  5.6e-07 / 2.0e-03
    body_close-B2-7x6-f32         2.6e-07 / 2.0e-03  4.0e-07 / 2.0e-03  5.3e-08 / 2.0e-03  0.0e+00 / 2.0e-03  4.0e-07 / 2.0e-03
    body_close-B1-10x36-f32       2.8e-07 / 2.0e-03  4.1e-07 / 2.0e-03  1.2e-07 / 2.0e-03  1.3e-08 / 2.0e-03  4.1e-07 / 2.0e-03
    body_close-B1-18x34-f32       2.9e-07 / 2.0e-03  4.2e-07 / 2.0e-03  1.2e-07 / 2.0e-03  1.3e-08 / 2.0e-03  4.2e-07 / 2.0e-03
    up-B2-7x6-f32                 4.1e-07 / 2.0e-03  7.8e-07 / 2.0e-03  5.4e-08 / 2.0e-03  6.7e-09 / 2.0e-03  7.8e-07 / 2.0e-03
    up-B1-10x36-f32               4.2e-07 / 2.0e-03  8.3e-07 / 2.0e-03  1.2e-07 / 2.0e-03  2.1e-08 / 2.0e-03  8.3e-07 / 2.0e-03
    close-ch3-B2-7x6-f32          4.6e-07 / 2.0e-03  8.7e-08 / 2.0e-03  4.9e-08 / 2.0e-03  0.0e+00 / 2.0e-03  8.7e-08 / 2.0e-03
    close-ch3-B1-18x34-f32        4.1e-07 / 2.0e-03  9.1e-08 / 2.0e-03  1.2e-07 / 2.0e-03  0.0e+00 / 2.0e-03  1.2e-07 / 2.0e-03
    close-ch4-B2-7x6-f32          4.3e-07 / 2.0e-03  1.0e-07 / 2.0e-03  5.1e-08 / 2.0e-03  0.0e+00 / 2.0e-03  1.0e-07 / 2.0e-03
    close-ch4-B1-18x34-f32        4.1e-07 / 2.0e-03  1.1e-07 / 2.0e-03  1.2e-07 / 2.0e-03  0.0e+00 / 2.0e-03  1.2e-07 / 2.0e-03
    close-ch8-B1-10x36-bf16       1.7e-03 / 5.2e-03  1.7e-03 / 5.0e-03  6.7e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.7e-03 / 5.0e-03
    close-ch12-B1-10x36-bf16      1.5e-03 / 4.5e-03  1.7e-03 / 5.0e-03  9.6e-08 / 1.0e-05  0.0e+00 / 1.0e-05  1.7e-03 / 5.0e-03
    walk-B1-7x6-bf16              4.2e-03 / 1.2e-02  5.3e-03 / 1.6e-02  4.3e-03 / 1.3e-02  4.2e-03 / 1.2e-02  4.2e-03 / 1.2e-02
    walk-B2-10x12-bf16            4.3e-03 / 1.3e-02  1.3e-02 / 4.0e-02  6.3e-03 / 1.8e-02  6.2e-03 / 1.8e-02  6.2e-03 / 1.8e-02
    walk-B1-7x6-f32               1.0e-06 / 2.0e-03  1.6e-06 / 2.0e-03  1.6e-06 / 2.0e-03  1.4e-06 / 2.0e-03  1.6e-06 / 2.0e-03
    walk-B2-10x12-f32             1.1e-06 / 2.0e-03  1.6e-06 / 2.0e-03  1.8e-06 / 2.0e-03  1.9e-06 / 2.0e-03  1.9e-06 / 2.0e-03
"""
import importlib
from collections import Counter

import pytest
import torch

import gemm_cases as G
import sr_cases as SC

pytestmark = pytest.mark.gpu
BF, F32 = SC.BF, SC.F32
PKG = SC.PKG

_gpu_error = []      # a HIP error in one case: the cases after it launch nothing more


def families(names):
    return dict(Counter(f for f in map(SC.family, names) if f is not None))


def branch_for(dev, case):
    """a fresh SRBranch over the Decoder's or EDSR's parameters (f32 masters on the device, zeroed gradient accumulators)"""
    S = importlib.import_module(PKG + ".sr")
    pre = SC.DEC if case.kind.startswith("dec_") else SC.ED
    sd = {k: v.float().contiguous().to(dev) for k, v in SC.params(case.ch).items() if k.startswith(pre)}
    return S.SRBranch(sd, case.dtype)


class Unit:
    """one case on the device: fwd() / bwd() run the unit through the branch's own methods and return clones of what they wrote"""

    def __init__(self, dev, ops, case):
        self.ops, self.case, self.br = ops, case, branch_for(dev, case)
        self.t = {k: (v.to(dev).contiguous() if k == "dy_nchw" else v.to(case.dtype).to(dev)) for k, v in SC.inputs(case).items()}

    def fwd(self):
        c, br, t, Seg = self.case, self.br, self.t, self.ops.SegSpec
        B, H, W = c.B, c.H, c.W
        k = c.kind
        if k in ("dec_entry", "dec_entry_engine"):
            h, w = H // 2, W // 2
            if k == "dec_entry":
                low, x = [Seg(t["low"])], [Seg(t["x"])]
            else:                # Engine._sr_segs for the default head: an up-sampled view; an up-sampled view and a dense part
                low = [Seg(t["low_half"], SC.C1, 0, 0, 0, 1, 1, h, w)]
                x = [Seg(t["xa_half"], SC.C2 // 2, 0, 0, 0, 1, 1, h // 2, w // 2), Seg(t["xb"], SC.C2 // 2, 0, 0, 0, 1, 0, h, w)]
            cat = br._dec_entry_fwd(low, x, B, H, W)
            return {"cat.x": cat[:, :SC.CX].clone(), "cat.a": cat[:, SC.CX:].clone()}
        if k == "dec_tail":
            cat = br._buf("cat", (B * H * W, SC.CX + SC.CA))
            cat.copy_(torch.cat((t["cat_x"], t["a_pre"].relu()), 1))
            return {"out": br._dec_tail_fwd(cat, B, H, W).clone()}
        if k == "head":
            y = br._head_fwd(t["x"], B, H, W)
        elif k == "resblock":
            y = br._resblock_fwd(0, t["x"], B, H, W)
        elif k == "body_close":
            y = br._body_close_fwd(t["x"], t["h"], B, H, W)
        elif k == "up":
            y = br._up_fwd(0, t["x"], B, H, W)
        elif k == "close":
            y = SC.tok(br._close_fwd(t["x"], B, H, W))
        else:
            y = SC.tok(br.edsr_forward(t["x"], B, H, W))
        return {"out": y.clone()}

    def bwd(self, parity=None):
        c, br, t = self.case, self.br, self.t
        B, H, W = c.B, c.H, c.W
        k = c.kind
        if k in ("dec_entry", "dec_entry_engine"):
            d_low, d_x = br._dec_entry_bwd(t["dcu"], t["da"])
            return {"d_low": d_low.clone(), "d_x": d_x.clone()}
        if k == "dec_tail":
            dcu, da = br._dec_tail_bwd(t["dy"])
            return {"g.cu": dcu.clone(), "g.a": da.clone()}
        if k == "head":
            d = br._head_bwd(t["dr"].clone(), t["d_rb"], B, H, W)        # (dr is summed into in place)
        elif k == "resblock":
            d = br._resblock_bwd(0, t["dy"], B, H, W)
        elif k == "body_close":
            d = br._body_close_bwd(t["dy"], B, H, W)
        elif k == "up":
            dy = t["dy"] if parity is None else t["dy"] * SC.parity_masks(B, 2 * H, 2 * W)[parity].to(t["dy"].device).view(-1, 1)
            d = br._up_bwd(0, dy.contiguous(), B)
        elif k == "close":
            d = br._close_bwd(t["dy_nchw"], B, H, W, 0)
        else:
            d = br.edsr_backward(t["dy_nchw"])
        return {"din": d.clone()}

    def grads(self):
        pre, names = SC.param_names(self.case)
        return {n: self.br.g[pre + n].clone() for n in names}


class Measure:
    """prints every figure, collects what is out of its gate"""

    def __init__(self, case, ref):
        self.case, self.ref, self.bad = case, ref, []

    def __call__(self, what, got, name, scale=1.0):
        base = name.split("[")[0]
        v = got[name] if name in got else SC.subset(self.case, base, name[name.index("[") + 1:-1], got[base])
        a = self.ref.A[name] * scale
        err, lim = SC.rel_l2(v.reshape(a.shape), a), SC.gate(self.case, self.ref, name)
        print(f"SRROUTE {self.case.id} {what} {name} err {err:.3e} gate {lim:.3e} e_emul {self.ref.e_emul.get(name, float('nan')):.3e}")
        if not err <= lim:
            self.bad.append(f"{what} {name}: {err:.3e} > {lim:.3e}")


@pytest.mark.parametrize("case", SC.CASES, ids=[c.id for c in SC.CASES])
def test_sr_route(dev, case):
    if _gpu_error:
        pytest.fail(f"not run: an earlier case ended in a GPU error ({_gpu_error[0]})")
    ops = importlib.import_module(PKG + ".ops")
    ref = SC.reference(case)
    SC.check_reference(case, ref)
    got, again, twice, res = {}, {}, {}, {}
    try:
        u = Unit(dev, ops, case)
        fwd_names = G.launched_kernels(lambda: res.__setitem__("f", u.fwd()))
        got.update(res["f"])
        bwd_names = G.launched_kernels(lambda: res.__setitem__("b", u.bwd()))
        got.update(res["b"])
        got.update(u.grads())
        again = u.fwd()                                           # the buffers are reused: the same bits
        twice.update(u.bwd())                                     # gradients NOT cleared: every parameter gradient doubles
        twice.update(u.grads())
        if case.kind == "up":                                     # what each plane launch reads back, alone
            for p in SC.parity_masks(case.B, 2 * case.H, 2 * case.W):
                got[f"din[{p}]"] = u.bwd(parity=p)["din"]
        torch.cuda.synchronize()
    except RuntimeError as e:
        _gpu_error.append(f"{case.id}: {e}")
        raise

    m = Measure(case, ref)
    want_f, want_b = SC.expected(case)
    for what, names, want in (("forward", fwd_names, want_f), ("backward", bwd_names, want_b)):
        if families(names) != want:
            m.bad.append(f"{what} launched {families(names)}, the unit is {want} (all kernels: {names})")
    for k, v in again.items():
        if not torch.equal(v, got[k]):
            m.bad.append(f"second forward: {k} differs")
    for name in ref.A:
        m("once", got, name)
    pnames = SC.param_names(case)[1]
    for name in ref.A:
        base = name.split("[")[0]
        if base in twice and not name.startswith("din[p"):        # (the one-parity runs came after)
            m("twice", twice, name, 2.0 if base in pnames else 1.0)
    assert not m.bad, f"{case.id}: " + "; ".join(m.bad)


# ------------------------------------------------------------------ the engine's taps
def _dense(seg, B):
    """the feature a K-segment of Engine._sr_segs stands for, materialised with torch: [B * H * W][klen] on the segment's target grid"""
    v = seg.t[:, seg.coff: seg.coff + seg.klen].reshape(B, seg.Hi, seg.Wi, seg.klen)
    for _ in range(seg.shr):
        v = v.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return v.reshape(-1, seg.klen)


def _small_ints(shape, seed, dev, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-8, 9, tuple(shape), generator=g).to(dtype).to(dev)      # sums of five stay exact in bf16


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_engine_taps(dev, dtype):
    """Engine._sr_segs / _sr_extra / _add_extra on Model(sr=True) at S = 128, B = 2, after one training forward."""
    from oracle import ref_torch as R
    from test_model_sr_gpu import build
    ops = importlib.import_module(PKG + ".ops")
    S, B = 128, 2
    t = S // 4
    model, _ = build(dev, S)
    model.compute_dtype = dtype
    model.train()
    x_rgb, x_ir = R.synthetic_inputs(B, S, seed=1)
    model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
    eng = model._get_engine()
    plan = next(p for p in eng.plans.values() if p.dt == dtype and p.training and p.B == B and p.sr is not None)
    br = plan.sr

    # ---- forward: the views against the same features materialised
    low, deep = eng._sr_segs(plan)
    assert [(s.klen, s.shr) for s in low] == [(128, 1)] and [(s.klen, s.shr) for s in deep] == [(256, 1), (256, 0)]
    d3_views = br.decoder_forward(low, deep, B, t, t).clone()
    low_d = torch.cat([_dense(s, B) for s in low], 1).contiguous()
    deep_d = torch.cat([_dense(s, B) for s in deep], 1).contiguous()
    assert tuple(low_d.shape) == (B * t * t, 128) and tuple(deep_d.shape) == (B * (t // 2) ** 2, 512)
    d3_dense = br.decoder_forward([ops.SegSpec(low_d)], [ops.SegSpec(deep_d)], B, t, t).clone()
    torch.cuda.synchronize()
    assert float(d3_dense.float().abs().max()) > 0 and torch.equal(d3_views, d3_dense)

    # ---- return: g.low / g.x into the tapped features' gradients
    extra = eng._sr_extra(plan)
    assert len(extra) == 3 and sum(len(v) for v in extra.values()) == 3
    for j, k in enumerate(("g.low", "g.x")):
        br.bufs[k].copy_(_small_ints(br.bufs[k].shape, 11 + j, dev, dtype))
    seen = set()
    for n, (ref, entries) in enumerate(extra.items()):
        (buf, lds, coff, c, shr, H), = entries
        seen.add((lds, coff, c, shr))
        Hs = H >> shr
        ld, off = c + 24, 16
        target = _small_ints((B * Hs * Hs, ld), 21 + n, dev, dtype)
        want = target.clone()
        part = buf[:, coff: coff + c].float().view(B, H, H, c)
        if shr:
            part = part.view(B, Hs, 2, Hs, 2, c).sum((2, 4))
        want[:, off: off + c] = (want[:, off: off + c].float() + part.reshape(-1, c)).to(dtype)
        eng._add_extra(plan, extra, ref, (target, ld, off))
        torch.cuda.synchronize()
        assert torch.equal(target[:, :off], want[:, :off]) and torch.equal(target[:, off + c:], want[:, off + c:]), (ref, "margins")
        assert torch.equal(target, want), (ref, float((target.float() - want.float()).abs().max()))
    assert seen == {(128, 0, 128, 1), (512, 0, 256, 1), (512, 256, 256, 0)}
