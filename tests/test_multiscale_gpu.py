"""``--multi-scale`` on the device (Train.py:396-402): sodt_preprocess_u8_ms (csrc/multiscale.hip) against the calls the reference's
loop makes - ``x.float() / 255.0``, ``F.interpolate(size=[i // down_factor ...], align_corners=True)``, then
``F.interpolate(size=ns, align_corners=False)`` - computed with the same torch functions on the CPU; the routing of
``preprocess_batch(..., size=)``; the bounds of the C entry; the whole model and a training loop over drawn sizes; and
``Model.runs_at`` against what the engine itself runs or refuses.

Parity gates (those of tests/test_preprocess_gpu.py): (1) <= 1e-6 against the float64 evaluation of the three calls - both
stages take the source index and the blend weight from an exact integer quotient / remainder and the stage-1 values are rounded
to f32 as the reference's intermediate is, so the result is the formula's value up to a handful of f32 roundings of numbers
<= 1; (2) against the float32 calls within their own coordinate noise, two ulps of the largest f32 source coordinate, once per
stage: 1e-6 + 2 eps (max(H, W) + max(Hmid, Wmid))."""
import ctypes
import importlib
import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
PKG = "small-object-detection-transformers_amd"
EPS = float(torch.finfo(torch.float32).eps)

# (B, H, W, down_factor, ns, IR channels).  Stage 2 shrinks and grows, one side only, odd sizes and widths that are no multiple
# of four, one output pixel, 8x growth, more than one tile (768 > 256 columns, 32 rows), a patch that only a narrower and
# one-row tile fits (1200 -> 256 columns: 64 x 1), a shrink by more than four in area ((1, 1), (4, 8): stage 1 per output pixel
# instead of the LDS patch) and one whose patch fits no LDS (16384 -> 2 columns).
CASES = [(2, 64, 64, 2, (48, 48), 3), (2, 64, 64, 2, (96, 96), 3), (1, 64, 64, 1, (32, 32), 3), (1, 64, 64, 1, (96, 64), 1),
         (2, 100, 74, 2, (64, 32), 3), (1, 37, 29, 3, (32, 32), 3), (1, 96, 120, 4, (64, 96), 3), (1, 66, 62, 2, (31, 33), 1),
         (1, 64, 64, 2, (1, 1), 3), (1, 8, 8, 2, (64, 64), 3), (1, 1024, 1024, 2, (768, 768), 3),
         (1, 8, 1200, 1, (64, 256), 3), (1, 50, 70, 1, (4, 8), 3), (1, 1, 16384, 1, (4096, 2), 1)]


def _ref(x_u8, f, ns, dt):
    x = x_u8.to(dt) / 255.0
    x = F.interpolate(x, size=[i // f for i in x.shape[2:]], mode="bilinear", align_corners=True)
    return F.interpolate(x, size=list(ns), mode="bilinear", align_corners=False)


def _pair(B, H, W, f, c_ir=3):
    g = torch.Generator().manual_seed(B * 1000 + H + f)
    rgb = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    ir = torch.randint(0, 256, (B, c_ir, H, W), generator=g, dtype=torch.uint8)
    return rgb, ir


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(PKG + ".preprocess")


@pytest.mark.parametrize("B,H,W,f,ns,c_ir", CASES)
def test_multiscale_matches_torch(dev, P, B, H, W, f, ns, c_ir):
    rgb, ir = _pair(B, H, W, f, c_ir)
    o1, o2 = P.preprocess_batch(rgb.to(dev), ir.to(dev), f, size=ns)
    torch.cuda.synchronize()
    assert o1.shape == (B, 3, *ns) and o2.shape == (B, c_ir, *ns) and o1.dtype == o2.dtype == torch.float32
    noise = 1e-6 + 2.0 * EPS * (max(H, W) + max(H // f, W // f))
    for o, x in ((o1, rgb), (o2, ir)):
        e64 = float((o.cpu().double() - _ref(x, f, ns, torch.float64)).abs().max())
        e32 = float((o.cpu() - _ref(x, f, ns, torch.float32)).abs().max())
        print(f"B={B} {H}x{W} /{f} -> {ns}: vs f64 {e64:.2e} (gate 1e-6), vs f32 {e32:.2e} (gate {noise:.2e})")
        assert e64 <= 1e-6
        assert e32 <= noise


def test_int_size_is_square(dev, P):
    rgb, ir = _pair(1, 64, 64, 2)
    a = P.preprocess_batch(rgb.to(dev), ir.to(dev), 2, size=48)
    b = P.preprocess_batch(rgb.to(dev), ir.to(dev), 2, size=(48, 48))
    assert a[0].shape == (1, 3, 48, 48) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_routing(dev, P, ops):
    rgb, ir = _pair(2, 64, 64, 2)
    rgb, ir = rgb.to(dev), ir.to(dev)
    plain = P.preprocess_batch(rgb, ir, 2)
    for size in (None, 32, (32, 32), [32, 32]):
        with ops.Recorder() as rec:
            got = P.preprocess_batch(rgb, ir, 2, size=size)
        assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8"], size
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    for size in (48, (32, 48), (96, 96), (31, 33), (64, 64), 1):
        with ops.Recorder() as rec:
            got = P.preprocess_batch(rgb, ir, 2, size=size)
        assert [c[2] for c in rec.calls] == ["sodt_preprocess_u8_ms"], size
        assert got[0].shape[2:] == got[1].shape[2:] == ((size, size) if isinstance(size, int) else tuple(size))


@pytest.mark.parametrize("size", [0, -32, (32, 0), (32,), (32, 32, 32), 32.0, (32.0, 32), "32", True, (None, 32)])
def test_bad_size_raises_before_any_launch(dev, P, ops, size):
    rgb, ir = _pair(1, 64, 64, 2)
    with ops.Recorder() as rec:
        with pytest.raises(ValueError):
            P.preprocess_batch(rgb.to(dev), ir.to(dev), 2, size=size)
    assert rec.calls == []


def _entry(pkg):
    return pkg._lib.load().sodt_preprocess_u8_ms


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("lead", [1024, 1021])          # the 16-byte stores of an aligned row, the scalar stores of a misaligned one
def test_writes_stay_inside_the_outputs(dev, pkg, P, lead):
    B, H, W, f, ns, c_ir = 1, 66, 62, 2, (31, 33), 1
    rgb, ir = _pair(B, H, W, f, c_ir)
    rgb, ir = rgb.to(dev), ir.to(dev)
    want = P.preprocess_batch(rgb, ir, f, size=ns)
    sentinel = -12345.0
    bufs = []
    for c in (3, c_ir):
        n = B * c * ns[0] * ns[1]
        bufs.append((torch.full((lead + n + 1024,), sentinel, device=dev), n))
    outs = [b[lead: lead + n] for b, n in bufs]
    rc = _entry(pkg)(rgb.data_ptr(), ir.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), B, 3, c_ir, H, W, H // f, W // f,
                     ns[0], ns[1], _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for (b, n), w in zip(bufs, want):
        raw = b.view(torch.int32)
        s = torch.tensor(sentinel).view(torch.int32).item()
        assert bool((raw[:lead] == s).all()) and bool((raw[lead + n:] == s).all())
        assert torch.equal(b[lead: lead + n], w.reshape(-1))


def test_einval_leaves_outputs_untouched(dev, pkg):
    B, H, W, Hm, Wm, Ho, Wo = 1, 16, 16, 8, 8, 12, 12
    rgb = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev)
    ir = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev)
    o1 = torch.full((B, 3, Ho, Wo), float("nan"), device=dev)
    o2 = torch.full((B, 3, Ho, Wo), float("nan"), device=dev)
    good = [rgb.data_ptr(), ir.data_ptr(), o1.data_ptr(), o2.data_ptr(), B, 3, 3, H, W, Hm, Wm, Ho, Wo]
    bad = []
    for i in range(4):                                    # a null pointer
        bad.append({i: None})
    for i in range(4, 13):                                # a non-positive batch, channel count or size
        bad += [{i: 0}, {i: -1}]
    bad += [{9: H + 1}, {10: W + 1}]                      # a "shrink" that grows
    two31 = 1 << 31
    bad += [{7: 65536, 9: 32768}, {8: 65536, 10: 32768},  # o * (in - 1) of stage 1 reaches 2^31
            {11: two31 // (2 * Hm)}, {12: two31 // (2 * Wm)},      # (2 o + 1) * mid of stage 2
            {7: 46341, 8: 46341, 9: 1, 10: 1}]            # the pixel offset inside one source plane
    fn = _entry(pkg)
    for patch in bad:
        args = list(good)
        for i, v in patch.items():
            args[i] = v
        rc = fn(*args, _stream())
        assert rc == pkg._lib.EINVAL, (patch, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    assert fn(*good, _stream()) == 0                      # and the unpatched call is accepted
    torch.cuda.synchronize()
    assert bool((o1 == 0).all()) and bool((o2 == 0).all())


@pytest.fixture(scope="module")
def model512(dev):
    from test_model_gpu import build
    return build(dev, 512)[0]


def _u8_pair_1024(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (1, 3, 1024, 1024), generator=g, dtype=torch.uint8).to(dev),
            torch.randint(0, 256, (1, 3, 1024, 1024), generator=g, dtype=torch.uint8).to(dev))


def test_whole_model_on_fused_inputs(dev, P, model512):
    """Built at 512, run at S = 576 (stage 3 padded, pos_embed dropped): the logits from the one-launch inputs against the logits from
    the inputs torch resizes, within the project's logit gate."""
    model = model512
    model.compute_dtype = torch.float32
    model.eval()
    rgb, ir = _u8_pair_1024(dev, 5)
    a = P.preprocess_batch(rgb, ir, 2, size=576)
    b = [_ref(x, 2, (576, 576), torch.float32) for x in (rgb, ir)]
    assert a[0].shape == b[0].shape == (1, 3, 576, 576)
    with torch.no_grad():
        pa = model(a[0], a[1], "RGB+IR")[1][0].clone()
        pb = model(b[0], b[1], "RGB+IR")[1][0].clone()
    assert pa.shape == (1, 3, 144, 144, 13)
    err = float((pa - pb).abs().max())
    print(f"logits at S=576, fused inputs vs torch-resized inputs: {err:.3e} (|logit| max {float(pb.abs().max()):.2f})")
    assert err <= 1e-3


@pytest.mark.parametrize("S", [96, 320, 512, 544, 576])
def test_runs_at_is_what_the_engine_runs(dev, model512, S):
    model = model512
    model.compute_dtype = torch.float32
    model.eval()
    x = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(S)).to(dev)
    if model.runs_at(S):
        with torch.no_grad():
            z = model(x, x, "RGB+IR")[0]
        assert z.shape == (1, 3 * (S // 4) ** 2, 13) and bool(torch.isfinite(z).all())
    else:
        with pytest.raises((NotImplementedError, ValueError)):
            with torch.no_grad():
                model(x, x, "RGB+IR")
    assert model.runs_at(S) == (S in (512, 576))


LOOP_SEED = 80959       # chosen on the CPU: its 8 draws are 768, 576, 576, 512, 576, 768, 640, 704


def test_training_loop_over_drawn_sizes(dev, P):
    """Train.py:364-453 in miniature under --multi-scale: uint8 batch -> preprocess_batch(size=multi_scale_size(...)) -> forward ->
    ComputeLoss -> backward -> FusedSGD, bf16, the size drawn per step.  Five distinct sizes pass through the engine's four-plan LRU."""
    from test_model_gpu import build
    O = importlib.import_module(PKG + ".optim")
    LS = importlib.import_module(PKG + ".loss")
    E = importlib.import_module(PKG + ".engine")
    model = build(dev, 512)[0]
    model.compute_dtype = torch.bfloat16
    model.train()
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    opt = O.FusedSGD(O.set_weight_decay(model), model=model, lr=0.01, momentum=0.937, nesterov=True)
    compute_loss = LS.ComputeLoss(model)
    rgb, ir = _u8_pair_1024(dev, 7)
    targets = LS.synthetic_targets(1, 16, 8, seed=1).to(dev)
    rng = random.Random(LOOP_SEED)
    sizes, losses = [], []
    for step in range(8):
        ns = P.multi_scale_size(1024, (512, 512), gs=64, rng=rng, runs_at=model.runs_at)
        x, xi = P.preprocess_batch(rgb, ir, 2, size=ns)
        assert x.shape == (1, 3, *ns)
        pred, _ = model(x, xi, "RGB+IR")
        S = ns[0]
        assert pred[0].shape == (1, 3, S // 4, S // 4, 13), (step, ns, pred[0].shape)
        loss = compute_loss(pred, targets)[0]
        loss.backward()
        opt.step()
        if step < 7:
            opt.zero_grad(set_to_none=True)
        sizes.append(ns)
        losses.append(float(loss.detach()))
    print(f"sizes {[s[0] for s in sizes]}, losses {[round(v, 4) for v in losses]}")
    assert all(h == w for h, w in sizes) and len(set(sizes)) >= 3 and max(h for h, _ in sizes) <= 768, sizes
    assert all(v == v and abs(v) != float("inf") for v in losses), losses
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    eng = model._get_engine()
    assert len(eng.plans) <= E.Engine.MAX_PLANS
