"""``--quad`` on the device (LoadImagesAndLabels.collate_fn4, basics/utils/datasets.py:637-664): sodt_quad_u8 and
sodt_preprocess_u8_quad (csrc/quad.hip) against the reference's own outputs (tests/golden/quad.pt) and against tests/quad_ref.py,
the CPU torch restatement that spells the zoom as ``F.interpolate(...).type(uint8)``, on further shapes and every mask.

Gates: the uint8 quad batch is exact (``torch.equal``); the fused f32 inputs are (1) bit-identical to ``preprocess_batch`` on the
materialised quad batch and (2) within 1e-6 of the float64 evaluation of ``quad_ref(...) / 255`` followed by
``F.interpolate(align_corners=True)``, the gate tests/test_preprocess_gpu.py holds that arithmetic to.  Then the routing, the
bounds of both C entries, their refusals, ``quad_targets`` on the device, and two training steps on quad inputs."""
import ctypes
import importlib
import os

import pytest
import torch
import torch.nn.functional as F

from quad_ref import plain_targets, quad_ref

pytestmark = pytest.mark.gpu
PKG = "small-object-detection-transformers_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W): widths on and off the 16-byte grid of the uint8 rows and the 4-pixel grid of the f32 rows, an odd height, two
# groups, one-pixel images, and rows long enough for more than one 16-byte unit per half
SHAPES = [(4, 16, 16), (4, 33, 18), (8, 7, 50), (4, 1, 1), (4, 64, 48)]


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(PKG + ".preprocess")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "quad.pt"))


def _modes(mask, n):
    return tuple(bool(mask >> g & 1) for g in range(n))


def _pair(B, H, W, c_ir=3):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    rgb = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    ir = torch.randint(0, 256, (B, c_ir, H, W), generator=g, dtype=torch.uint8)
    for x in (rgb, ir):                                    # both ends of the range, next to each other
        x.view(B, -1)[:, 0] = 255
        x.view(B, -1)[:, -1] = 0
    return rgb, ir


_REF = {}


def _ref(B, H, W, mask):
    """quad_ref of _pair(B, H, W) under mask, computed once per module"""
    key = (B, H, W, mask)
    if key not in _REF:
        rgb, ir = _pair(B, H, W)
        _REF[key] = quad_ref(rgb, ir, [torch.zeros(0, 6)] * B, _modes(mask, B // 4))[:2]
    return _REF[key]


def test_quad_batch_is_the_reference(dev, P, golden):
    for c in golden:
        rgb, ir = c["imgs"].to(dev), c["irs"].to(dev)
        o1, o2 = P.quad_batch(rgb, ir, tuple(c["modes"]))
        assert o1.dtype == o2.dtype == torch.uint8
        assert torch.equal(o1.cpu(), c["img4"]) and torch.equal(o2.cpu(), c["ir4"]), c["name"]
        assert torch.equal(rgb.cpu(), c["imgs"]) and torch.equal(ir.cpu(), c["irs"])


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_quad_batch_every_mask(dev, P, B, H, W):
    rgb, ir = _pair(B, H, W)
    d1, d2 = rgb.to(dev), ir.to(dev)
    n = B // 4
    for mask in range(1 << n):
        o1, o2 = P.quad_batch(d1, d2, _modes(mask, n))
        r1, r2 = _ref(B, H, W, mask)
        assert o1.shape == (n, 3, 2 * H, 2 * W) and torch.equal(o1.cpu(), r1) and torch.equal(o2.cpu(), r2), mask
    assert torch.equal(d1.cpu(), rgb) and torch.equal(d2.cpu(), ir)


def test_quad_batch_64_groups(dev, P):
    """n = 64, alternating modes from group 0 = tile: bit 63 of the mask is set and has to arrive"""
    B, H, W = 256, 4, 4
    rgb, ir = _pair(B, H, W, 1)
    modes = tuple(g % 2 == 1 for g in range(64))
    assert modes[63]
    o1, o2 = P.quad_batch(rgb.to(dev), ir.to(dev), modes)
    r1, r2, _ = quad_ref(rgb, ir, [torch.zeros(0, 6)] * B, modes)
    assert torch.equal(o1.cpu(), r1) and torch.equal(o2.cpu(), r2)
    f1, f2 = P.preprocess_batch(rgb.to(dev), ir.to(dev), 1, quad=modes)
    assert torch.equal(f1.cpu(), r1.float() / 255.0) and torch.equal(f2.cpu(), r2.float() / 255.0)


@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_preprocess(dev, P, B, H, W, f):
    if 2 * H // f < 1 or 2 * W // f < 1:
        with pytest.raises(RuntimeError):                  # no output pixel: the entry refuses, as sodt_preprocess_u8 does
            P.preprocess_batch(*[x.to(dev) for x in _pair(B, H, W)], f, quad=_modes(0, B // 4))
        return
    rgb, ir = _pair(B, H, W)
    d1, d2 = rgb.to(dev), ir.to(dev)
    n = B // 4
    Ho, Wo = 2 * H // f, 2 * W // f
    for mask in range(1 << n):
        modes = _modes(mask, n)
        o = P.preprocess_batch(d1, d2, f, quad=modes)
        two = P.preprocess_batch(*P.quad_batch(d1, d2, modes), f)
        worst = 0.0
        for got, want, q in zip(o, two, _ref(B, H, W, mask)):
            assert got.dtype == torch.float32 and got.shape == (n, 3, Ho, Wo)
            assert torch.equal(got, want), (mask, float((got - want).abs().max()))
            x = q.double() / 255.0
            if f > 1:
                x = F.interpolate(x, size=[Ho, Wo], mode="bilinear", align_corners=True)
            worst = max(worst, float((got.cpu().double() - x).abs().max()))
        print(f"B={B} {H}x{W} /{f} mask {mask:b}: vs f64 {worst:.2e} (gate 1e-6)")
        assert worst <= 1e-6


def test_fused_preprocess_on_the_golden_cases(dev, P, golden):
    for c in golden:
        o = P.preprocess_batch(c["imgs"].to(dev), c["irs"].to(dev), 1, quad=tuple(c["modes"]))
        assert torch.equal(o[0].cpu(), c["img4"].float() / 255.0) and torch.equal(o[1].cpu(), c["ir4"].float() / 255.0), c["name"]


def test_routing(dev, P, ops):
    B, H, W, f = 8, 32, 32, 2
    rgb, ir = [x.to(dev) for x in _pair(B, H, W)]
    modes = (True, False)
    with ops.Recorder() as rec:
        plain = P.preprocess_batch(rgb, ir, f)
    assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8"] and plain[0].shape == (B, 3, 16, 16)
    with ops.Recorder() as rec:
        P.preprocess_batch(rgb, ir, f, size=24, quad=None)
    assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8_ms"]
    with ops.Recorder() as rec:
        qb = P.quad_batch(rgb, ir, modes)
    assert [c[2] for c in rec.calls] == ["sodt_quad_u8"]
    want = P.preprocess_batch(*qb, f)
    for size in (None, 32, (32, 32), [32, 32]):
        with ops.Recorder() as rec:
            got = P.preprocess_batch(rgb, ir, f, size=size, quad=modes)
        assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8_quad"], size
        assert got[0].shape == (2, 3, 32, 32) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for size in (48, (24, 40), 64, 1):
        with ops.Recorder() as rec:
            got = P.preprocess_batch(rgb, ir, f, size=size, quad=modes)
        assert [c[2] for c in rec.calls] == ["sodt_quad_u8", "sodt_preprocess_u8_ms"], size
        two = P.preprocess_batch(*qb, f, size=size)
        assert got[0].shape == two[0].shape and torch.equal(got[0], two[0]) and torch.equal(got[1], two[1]), size


@pytest.mark.parametrize("modes", [(), (True,), (True, False, True), (1, 0), (True, None), [True, 0.0], "ab", 3, tuple([False] * 65)])
def test_bad_modes_raise_before_any_launch(dev, P, ops, modes):
    B = 260 if isinstance(modes, tuple) and len(modes) == 65 else 8
    rgb = torch.zeros(B, 3, 4, 4, dtype=torch.uint8, device=dev)
    with ops.Recorder() as rec:
        with pytest.raises(ValueError):
            P.preprocess_batch(rgb, rgb, 1, quad=modes)
        with pytest.raises(ValueError):
            P.preprocess_batch(rgb, rgb, 1, size=6, quad=modes)
        with pytest.raises(ValueError):
            P.quad_batch(rgb, rgb, modes)
    assert rec.calls == []


def test_fewer_than_four_samples_raise(dev, P, ops):
    rgb = torch.zeros(3, 3, 4, 4, dtype=torch.uint8, device=dev)
    with ops.Recorder() as rec:
        with pytest.raises(ValueError):
            P.preprocess_batch(rgb, rgb, 1, quad=())
        with pytest.raises(ValueError):
            P.quad_batch(rgb, rgb, ())
    assert rec.calls == []


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("lead", [1024, 1021])          # the 16-byte stores of an aligned row, the scalar stores of a misaligned one
def test_writes_stay_inside_the_outputs(dev, pkg, P, lead):
    B, H, W, c_ir, f, modes, mask = 8, 33, 18, 1, 2, (True, False), 0b01
    rgb, ir = _pair(B, H, W, c_ir)
    rgb, ir = rgb.to(dev), ir.to(dev)
    lib = pkg._lib.load()
    n, Ho, Wo = B // 4, 2 * H // f, 2 * W // f
    # sodt_quad_u8: uint8 outputs inside buffers of 0xA5
    want = P.quad_batch(rgb, ir, modes)
    bufs = [(torch.full((lead + n * c * 4 * H * W + 1024,), 0xA5, dtype=torch.uint8, device=dev), n * c * 4 * H * W) for c in (3, c_ir)]
    outs = [b[lead: lead + k] for b, k in bufs]
    rc = lib.sodt_quad_u8(rgb.data_ptr(), ir.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), B, 3, c_ir, H, W, mask, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for (b, k), w in zip(bufs, want):
        assert bool((b[:lead] == 0xA5).all()) and bool((b[lead + k:] == 0xA5).all())
        assert torch.equal(b[lead: lead + k], w.reshape(-1))
    # sodt_preprocess_u8_quad: f32 outputs inside buffers of a sentinel
    want = P.preprocess_batch(rgb, ir, f, quad=modes)
    sentinel = -12345.0
    bufs = [(torch.full((lead + n * c * Ho * Wo + 1024,), sentinel, device=dev), n * c * Ho * Wo) for c in (3, c_ir)]
    outs = [b[lead: lead + k] for b, k in bufs]
    rc = lib.sodt_preprocess_u8_quad(rgb.data_ptr(), ir.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), B, 3, c_ir, H, W, Ho, Wo,
                                     mask, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    s = torch.tensor(sentinel).view(torch.int32).item()
    for (b, k), w in zip(bufs, want):
        raw = b.view(torch.int32)
        assert bool((raw[:lead] == s).all()) and bool((raw[lead + k:] == s).all())
        assert torch.equal(b[lead: lead + k], w.reshape(-1))


def test_einval_leaves_outputs_untouched(dev, pkg):
    B, H, W, Ho, Wo = 8, 8, 8, 12, 12
    rgb = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev)
    ir = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev)
    lib = pkg._lib.load()
    two31 = 1 << 31
    # sodt_preprocess_u8_quad(rgb, ir, out_rgb, out_ir, B, c_rgb, c_ir, H, W, Hout, Wout, mask)
    o1 = torch.full((2, 3, Ho, Wo), float("nan"), device=dev)
    o2 = torch.full((2, 3, Ho, Wo), float("nan"), device=dev)
    good = [rgb.data_ptr(), ir.data_ptr(), o1.data_ptr(), o2.data_ptr(), B, 3, 3, H, W, Ho, Wo, 0b10]
    bad = [{i: None} for i in range(4)]                    # a null pointer
    bad += [{4: 3}, {4: 0}, {4: -8}, {4: 260}]             # B < 4; B / 4 > 64
    bad += [{5: 0}, {5: -1}, {6: -1}]                      # a non-positive channel count (c_ir = 0 is allowed)
    for i in range(7, 11):                                 # a non-positive size
        bad += [{i: 0}, {i: -1}]
    bad += [{9: 2 * H + 1}, {10: 2 * W + 1}]               # Hout > 2H, Wout > 2W
    bad += [{7: 32768, 9: 32768}, {8: 32768, 10: 32768},   # 2H * Hout, 2W * Wout reach 2^31
            {7: 23171, 8: 23171, 9: 1, 10: 1}]             # 4 * H * W reaches 2^31 (23171^2 * 4 > 2^31)
    assert 2 * 32768 * 32768 >= two31 and 4 * 23171 * 23171 >= two31 and 2 * 23171 < two31
    for patch in bad:
        args = list(good)
        for i, v in patch.items():
            args[i] = v
        rc = lib.sodt_preprocess_u8_quad(*args, _stream())
        assert rc == pkg._lib.EINVAL, (patch, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    assert lib.sodt_preprocess_u8_quad(*good, _stream()) == 0          # and the unpatched call is accepted
    torch.cuda.synchronize()
    assert bool((o1 == 0).all()) and bool((o2 == 0).all())
    # sodt_quad_u8(rgb, ir, out_rgb, out_ir, B, c_rgb, c_ir, H, W, mask)
    u1 = torch.full((2, 3, 2 * H, 2 * W), 0xA5, dtype=torch.uint8, device=dev)
    u2 = torch.full((2, 3, 2 * H, 2 * W), 0xA5, dtype=torch.uint8, device=dev)
    good = [rgb.data_ptr(), ir.data_ptr(), u1.data_ptr(), u2.data_ptr(), B, 3, 3, H, W, 0b10]
    bad = [{i: None} for i in range(4)]
    bad += [{4: 3}, {4: 0}, {4: -8}, {4: 260}, {5: 0}, {5: -1}, {6: -1}, {7: 0}, {7: -1}, {8: 0}, {8: -1}, {7: 23171, 8: 23171}]
    for patch in bad:
        args = list(good)
        for i, v in patch.items():
            args[i] = v
        rc = lib.sodt_quad_u8(*args, _stream())
        assert rc == pkg._lib.EINVAL, (patch, rc)
    torch.cuda.synchronize()
    assert bool((u1 == 0xA5).all()) and bool((u2 == 0xA5).all())
    assert lib.sodt_quad_u8(*good, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((u1 == 0).all()) and bool((u2 == 0).all())


def test_no_ir_channels(dev, pkg):
    """c_ir = 0 with null IR pointers, as sodt_preprocess_u8 allows"""
    B, H, W = 4, 5, 7
    rgb, _ = _pair(B, H, W)
    lib = pkg._lib.load()
    r1 = quad_ref(rgb, rgb, [torch.zeros(0, 6)] * B, (True,))[0]
    u = torch.empty(1, 3, 2 * H, 2 * W, dtype=torch.uint8, device=dev)
    o = torch.empty(1, 3, 2 * H, 2 * W, device=dev)
    d = rgb.to(dev)
    assert lib.sodt_quad_u8(d.data_ptr(), None, u.data_ptr(), None, B, 3, 0, H, W, 1, _stream()) == 0
    assert lib.sodt_preprocess_u8_quad(d.data_ptr(), None, o.data_ptr(), None, B, 3, 0, H, W, 2 * H, 2 * W, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(u.cpu(), r1) and torch.equal(o.cpu(), r1.float() / 255.0)


def test_quad_targets_on_the_device(dev, P, golden):
    for c in golden:
        got = P.quad_targets(plain_targets(c["labels"]).to(dev), tuple(c["modes"]))
        assert got.device.type == "cuda" and torch.equal(got.cpu(), c["label4"]), c["name"]
    assert P.quad_targets(torch.zeros(0, 6, device=dev), (False,)).shape == (0, 6)


def test_training_steps_on_quad_inputs(dev, P):
    """Train.py:364-453 in miniature under --quad: the loader's plain batch of 8 -> quad_modes' draws (here fixed: group 0 zooms,
    group 1 tiles) -> quad_targets, preprocess_batch(quad=) -> forward -> ComputeLoss -> loss * 4 (Train.py:441-442) -> backward
    -> FusedSGD.  The logits of the first forward are held to those of the same model fed inputs made from quad_ref on the CPU."""
    from test_model_gpu import build
    O = importlib.import_module(PKG + ".optim")
    LS = importlib.import_module(PKG + ".loss")
    model = build(dev, 256)[0]
    model.compute_dtype = torch.float32
    model.train()
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    opt = O.FusedSGD(O.set_weight_decay(model), model=model, lr=0.01, momentum=0.937, nesterov=True)
    compute_loss = LS.ComputeLoss(model)
    B, S, modes = 8, 128, (True, False)
    rgb, ir = _pair(B, S, S)
    g = torch.Generator().manual_seed(5)
    labels = []
    for i in range(B):
        nl = 1 + i % 3
        l = torch.zeros(nl, 6)
        l[:, 1] = torch.randint(0, 8, (nl,), generator=g).float()
        l[:, 2:4] = torch.rand(nl, 2, generator=g) * 0.8 + 0.1
        l[:, 4:6] = torch.rand(nl, 2, generator=g) * 0.2 + 0.05
        labels.append(l)
    r1, r2, rl = quad_ref(rgb, ir, labels, modes)
    targets = P.quad_targets(plain_targets(labels).to(dev), modes)
    assert torch.equal(targets.cpu(), rl)
    d1, d2 = rgb.to(dev), ir.to(dev)
    ref_pred, _ = model((r1.float() / 255.0).to(dev), (r2.float() / 255.0).to(dev), "RGB+IR")
    want = ref_pred[0].detach().clone()
    losses = []
    for step in range(2):
        x, xi = P.preprocess_batch(d1, d2, 1, quad=modes)
        assert x.shape == xi.shape == (2, 3, 256, 256)
        pred, _ = model(x, xi, "RGB+IR")
        if step == 0:
            err = float((pred[0].detach() - want).abs().max())
            print(f"logits, fused quad inputs vs quad_ref inputs: {err:.3e} (|logit| max {float(want.abs().max()):.2f})")
            assert pred[0].shape == want.shape == (2, 3, 64, 64, 13) and err <= 1e-3
        loss = compute_loss(pred, targets)[0] * 4.
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        assert loss.detach().isfinite().all()
        for name, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (step, name)
        if step == 0:
            opt.zero_grad(set_to_none=True)
    print(f"losses (x 4) of the two steps: {[round(v, 4) for v in losses]}")
    assert all(v == v and abs(v) != float("inf") for v in losses), losses
