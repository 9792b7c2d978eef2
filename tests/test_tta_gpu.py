"""Test-time augmentation on the device (basics/models/model.py:155-184): ``sodt_tta_scale`` against torch's flip + interpolate +
pad on the CPU, the bounds of both C entries, ``sodt_detect_decode_tta`` against the plain decode followed by the reference's
CPU arithmetic, and ``Model.forward(augment=True)`` against the same composition made of its parts (tests/tta_ref.py).

Parity gates of the scale kernel (those of tests/test_multiscale_gpu.py for its one ``align_corners=False`` stage): (1) <= 1e-6
against the float64 evaluation - the source index and the weight come from an exact integer quotient / remainder, so the result is
the formula's value up to a handful of f32 roundings of numbers <= 1; (2) against the float32 calls within their own coordinate
noise, two ulps of the largest f32 source coordinate: 1e-6 + 2 eps max(H, W).  Everything else is compared bit for bit."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

import tta_ref

pytestmark = pytest.mark.gpu
PKG = "small-object-detection-transformers_amd"
EPS = float(torch.finfo(torch.float32).eps)
PAD = torch.tensor(0.447, dtype=torch.float32)


@pytest.fixture(scope="module")
def T(pkg):
    return importlib.import_module(PKG + ".tta")


def _pair(B, H, W, c_ir=3, seed=0):
    g = torch.Generator().manual_seed(1000 * B + 7 * H + W + seed)
    return torch.rand(B, 3, H, W, generator=g), torch.rand(B, c_ir, H, W, generator=g)


def _ref(x, content, padded, flip, dt):
    x = x.to(dt)
    x = x.flip(flip) if flip else x
    x = F.interpolate(x, size=list(content), mode="bilinear", align_corners=False)
    return F.pad(x, [0, padded[1] - content[1], 0, padded[0] - content[0]], value=0.447)


def _content(H, W, r):
    return (int(H * r), int(W * r))


# (B, H, W, IR channels, passes = [(content, padded, flip)]).  0.83 with a left-right flip (content 53 in 64), a rectangle at 0.67,
# odd sizes with a width that is no multiple of four and an up-down flip, more than one tile (832 > 256 columns), a content of
# one pixel, a content that fills the padded size, one-channel IR, two and three passes in one launch.
CASES = [(2, 64, 64, 3, [(_content(64, 64, 0.83), (64, 64), 3)]),
         (1, 64, 96, 3, [(_content(64, 96, 0.67), (64, 64), None)]),
         (1, 37, 29, 1, [(_content(37, 29, 0.83), (32, 32), 2)]),
         (1, 8, 1200, 3, [(_content(8, 1200, 0.67), (32, 832), None)]),
         (1, 8, 8, 3, [((1, 1), (32, 32), 3)]),
         (1, 64, 64, 1, [((32, 32), (32, 32), 2)]),
         (1, 64, 96, 3, [(_content(64, 96, 0.83), (64, 96), 3), (_content(64, 96, 0.67), (64, 64), None)]),
         (1, 45, 51, 1, [((45, 51), (45, 51), 3), ((37, 42), (64, 64), 2), ((30, 34), (33, 35), None)])]


@pytest.mark.parametrize("B,H,W,c_ir,passes", CASES)
def test_scale_matches_torch(dev, T, ops, B, H, W, c_ir, passes):
    assert _content(64, 64, 0.83) == (53, 53) and _content(64, 96, 0.67) == (42, 64) and _content(8, 1200, 0.67) == (5, 804)
    x, ir = _pair(B, H, W, c_ir)
    with ops.Recorder() as rec:
        outs = T.scale_pair(x.to(dev), ir.to(dev), passes)
    torch.cuda.synchronize()
    assert [c[2] for c in rec.calls] == ["sodt_tta_scale"]
    assert len(outs) == len(passes)
    noise = 1e-6 + 2.0 * EPS * max(H, W)
    for (o1, o2), (content, padded, flip) in zip(outs, passes):
        assert o1.shape == (B, 3, *padded) and o2.shape == (B, c_ir, *padded) and o1.dtype == o2.dtype == torch.float32
        for o, src in ((o1, x), (o2, ir)):
            o = o.cpu()
            e64 = float((o.double() - _ref(src, content, padded, flip, torch.float64)).abs().max())
            e32 = float((o - _ref(src, content, padded, flip, torch.float32)).abs().max())
            print(f"B={B} {H}x{W} -> {content} in {padded} flip {flip}: vs f64 {e64:.2e} (gate 1e-6), vs f32 {e32:.2e} (gate {noise:.2e})")
            assert e64 <= 1e-6
            assert e32 <= noise
            assert bool((o[:, :, content[0]:, :] == PAD).all()) and bool((o[:, :, :, content[1]:] == PAD).all())
            if content == (H, W):                                  # weights exactly 0: the flipped copy itself
                assert torch.equal(o[:, :, :H, :W], src.flip(flip) if flip else src)


@pytest.mark.parametrize("flip", [3, 2])
def test_ratio_one_is_the_flipped_copy(dev, T, flip):
    x, ir = _pair(2, 40, 72, 1)
    (o1, o2), = T.scale_pair(x.to(dev), ir.to(dev), [((40, 72), (40, 72), flip)])
    assert torch.equal(o1.cpu(), x.flip(flip)) and torch.equal(o2.cpu(), ir.flip(flip))


def test_scale_img_is_the_references_call(dev, T, ops):
    x, _ = _pair(1, 48, 72)
    xd = x.to(dev)
    assert T.scale_img(xd, 1.0) is xd
    for ratio, same, gs in ((0.83, False, 64), (0.67, False, 32), (0.67, True, 32)):
        with ops.Recorder() as rec:
            got = T.scale_img(xd, ratio, same, gs)
        want = tta_ref.scale_img(x, ratio, same, gs)
        assert [c[2] for c in rec.calls] == ["sodt_tta_scale"]
        assert got.shape == want.shape and float((got.cpu() - want).abs().max()) <= 1e-6 + 2.0 * EPS * 72
    with pytest.raises(ValueError):
        T.scale_img(xd, 1.5, same_shape=True)


# ------------------------------------------------------------------ entry bounds
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_scale_einval_leaves_outputs_untouched(dev, pkg):
    L = pkg._lib
    fn = L.load().sodt_tta_scale
    B, H, W = 1, 16, 16
    rgb = torch.zeros(B, 3, H, W, device=dev)
    ir = torch.zeros(B, 1, H, W, device=dev)
    o1 = torch.full((B, 3, 32, 32), float("nan"), device=dev)
    o2 = torch.full((B, 1, 32, 32), float("nan"), device=dev)
    good_pass = dict(out_rgb=o1.data_ptr(), out_ir=o2.data_ptr(), h=13, w=13, Hp=32, Wp=32, flip=3)

    def call(args, entries, npass=None):
        tab = (L.TtaPass * max(len(entries), 1))(*[L.TtaPass(**e) for e in entries])
        return fn(*args, tab, len(entries) if npass is None else npass, _stream())
    good = [rgb.data_ptr(), ir.data_ptr(), B, 3, 1, H, W]
    bad_args = [{0: None}, {1: None}, {2: 0}, {2: -1}, {3: 0}, {4: -1}, {5: 0}, {5: -1}, {6: 0}, {6: -1},
                {5: 65536, 6: 32768}]                                      # H * W reaches 2^31
    for patch in bad_args:
        args = list(good)
        for i, v in patch.items():
            args[i] = v
        assert call(args, [good_pass]) == L.EINVAL, patch
    bad_pass = [dict(out_rgb=None), dict(out_ir=None), dict(h=0), dict(w=0), dict(h=-1), dict(Hp=0), dict(Wp=-1), dict(h=33), dict(w=33),
                dict(flip=1), dict(flip=4), dict(flip=-1), dict(h=1 << 27, Hp=1 << 27)]      # 2 * h * H reaches 2^31
    for patch in bad_pass:
        assert call(good, [dict(good_pass, **patch)]) == L.EINVAL, patch
        assert call(good, [good_pass, dict(good_pass, **patch)]) == L.EINVAL, patch      # a bad second pass stops the first too
    assert call(good, [good_pass] * 5) == L.EINVAL                        # more than four passes
    assert call(good, [good_pass], npass=0) == L.EINVAL
    assert fn(*good, None, 1, _stream()) == L.EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    assert call(good, [good_pass]) == 0                                   # and the unpatched call is accepted
    torch.cuda.synchronize()
    for o in (o1, o2):
        assert bool((o[:, :, :13, :13] == 0).all()) and bool((o[:, :, 13:, :] == PAD.item()).all()) and bool((o[:, :, :, 13:] == PAD.item()).all())


@pytest.mark.parametrize("lead", [1024, 1021])          # the 16-byte stores of an aligned row, the scalar stores of a misaligned one
def test_scale_writes_stay_inside_the_outputs(dev, pkg, T, lead):
    L = pkg._lib
    B, H, W, c_ir, content, padded = 1, 37, 29, 1, (30, 24), (33, 35)
    x, ir = _pair(B, H, W, c_ir)
    x, ir = x.to(dev), ir.to(dev)
    want = T.scale_pair(x, ir, [(content, padded, 3)])[0]
    sentinel = -12345.0
    bufs = []
    for c in (3, c_ir):
        n = B * c * padded[0] * padded[1]
        bufs.append((torch.full((lead + n + 1024,), sentinel, device=dev), n))
    outs = [b[lead: lead + n] for b, n in bufs]
    tab = (L.TtaPass * 1)(L.TtaPass(out_rgb=outs[0].data_ptr(), out_ir=outs[1].data_ptr(), h=content[0], w=content[1],
                                    Hp=padded[0], Wp=padded[1], flip=3))
    rc = L.load().sodt_tta_scale(x.data_ptr(), ir.data_ptr(), B, 3, c_ir, H, W, tab, 1, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for (b, n), w in zip(bufs, want):
        assert bool((b[:lead] == sentinel).all()) and bool((b[lead + n:] == sentinel).all())
        assert torch.equal(b[lead: lead + n], w.reshape(-1))


# ------------------------------------------------------------------ the decode of one pass
B_D, NA, NY, NX, NO = 2, 3, 5, 7, 13
IMG_H, IMG_W = 40, 56
ROWS = NA * NY * NX
SENT = -54321.0


@pytest.fixture(scope="module")
def decode_case(dev, ops):
    g = torch.Generator().manual_seed(11)
    raw = (torch.randn(B_D, NA, NY, NX, NO, generator=g) * 2).to(dev)
    ag = torch.tensor([10., 13, 16, 30, 33, 23]).to(dev)
    z = torch.empty(B_D, ROWS, NO, device=dev)
    ops.detect_decode(raw, ag, z, B_D, NA, NY, NX, NO, 4.0)
    return raw, ag, z.cpu()


@pytest.mark.parametrize("flip", [0, 2, 3])
@pytest.mark.parametrize("si", [1, 0.83, 0.67])
def test_decode_tta_is_plain_decode_then_the_references_arithmetic(dev, ops, decode_case, si, flip):
    raw, ag, plain = decode_case
    off, total = 17, ROWS + 40
    z = torch.full((B_D, total, NO), SENT, device=dev)
    with ops.Recorder() as rec:
        ops.detect_decode_tta(raw, ag, z, B_D, NA, NY, NX, NO, 4.0, off, si, flip, IMG_H, IMG_W)
    torch.cuda.synchronize()
    assert [c[2] for c in rec.calls] == ["sodt_detect_decode_tta"]
    z = z.cpu()
    want = tta_ref.descale_deflip(plain, si, flip if flip else None, (IMG_H, IMG_W))
    assert torch.equal(z[:, off: off + ROWS], want)
    assert bool((z[:, :off] == SENT).all()) and bool((z[:, off + ROWS:] == SENT).all())
    if si == 1 and flip == 0:
        assert torch.equal(z[:, off: off + ROWS], plain)


def test_decode_tta_einval_leaves_output_untouched(dev, pkg, decode_case):
    L = pkg._lib
    fn = L.load().sodt_detect_decode_tta
    raw, ag, _ = decode_case
    total = ROWS + 8
    z = torch.full((B_D, total, NO), SENT, device=dev)
    F32 = ctypes.c_float
    good = [raw.data_ptr(), ag.data_ptr(), z.data_ptr(), B_D, NA, NY, NX, NO, F32(4.0), 8, total, F32(0.83), 3, IMG_H, IMG_W]
    bad = [{0: None}, {1: None}, {2: None}, {3: 0}, {4: 0}, {5: -1}, {6: 0}, {7: 4}, {9: -1}, {9: 9}, {10: ROWS - 1},
           {11: F32(0.0)}, {11: F32(-0.5)}, {11: F32(float("nan"))}, {11: F32(float("inf"))}, {12: 1}, {12: 4}, {13: 0}, {14: -3}]
    for patch in bad:
        args = list(good)
        for i, v in patch.items():
            args[i] = v
        assert fn(*args, _stream()) == L.EINVAL, patch
    torch.cuda.synchronize()
    assert bool((z == SENT).all())
    assert fn(*good, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((z[:, :8] == SENT).all()) and not bool((z[:, 8:] == SENT).any())


# ------------------------------------------------------------------ the whole path
@pytest.fixture(scope="module")
def model512(dev):
    from test_model_gpu import build
    model = build(dev, 512)[0]
    model.compute_dtype = torch.float32
    model.eval()
    return model


def _spy(ops, fn):
    names, real = [], ops._launch

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    ops._launch = spy
    try:
        out = fn()
    finally:
        ops._launch = real
    return out, names


def _composition(model, T, x, ir):
    """The augmented forward made of its parts: tta.scale_pair, the plain forward per pass, the reference's CPU arithmetic, cat."""
    scales, flips = T.check_passes(model.tta_scales, model.tta_flips)
    H, W = x.shape[2:]
    sizes = T.tta_sizes((H, W), scales, 32, model.runs_at)

    def make_inputs(k):
        if scales[k] == 1 and not flips[k]:
            return x, ir
        return T.scale_pair(x, ir, [(*sizes[k], flips[k])])[0]

    def forward(xi, iri):
        return model(xi, iri, "RGB+IR")[0]
    with torch.no_grad():
        want = tta_ref.augmented_forward(forward, x, ir, scales, [f if f else None for f in flips], None, make_inputs)
    return want, sizes


@pytest.fixture(scope="module")
def run768(dev, ops, T, model512):
    model = model512
    x, ir = _pair(1, 768, 768, 3, seed=5)
    x, ir = x.to(dev), ir.to(dev)
    with torch.no_grad():
        a = model(x, ir, "RGB+IR")[0].clone()
        (b, plain_names) = _spy(ops, lambda: model(x, ir, "RGB+IR")[0].clone())
        out, names = _spy(ops, lambda: model(x, ir, augment=True))
        _, plain_after = _spy(ops, lambda: model(x, ir, "RGB+IR")[0])
    want, sizes = _composition(model, T, x, ir)
    return dict(a=a, b=b, out=out, names=names, plain_names=plain_names, plain_after=plain_after, want=want, sizes=sizes)


def test_augmented_forward_768(run768):
    r = run768
    assert torch.equal(r["a"], r["b"]), "the plain eval forward is not bit-reproducible at 768 x 768"
    assert [p for _, p in r["sizes"]] == [(768, 768), (640, 640), (576, 576)]
    assert isinstance(r["out"], tuple) and len(r["out"]) == 2 and r["out"][1] is None
    z = r["out"][0]
    assert z.shape == (1, 3 * (192 * 192 + 160 * 160 + 144 * 144), 13) and z.dtype == torch.float32
    assert torch.equal(z.cpu(), r["want"])
    names = r["names"]
    assert names.count("sodt_tta_scale") == 1 and names.count("sodt_detect_decode_tta") == 3 and "sodt_detect_decode" not in names
    assert names[0] == "sodt_tta_scale" and names[-1] == "sodt_detect_decode_tta"
    assert r["plain_names"] == r["plain_after"] and r["plain_names"][-1] == "sodt_detect_decode"
    assert "sodt_tta_scale" not in r["plain_after"] and "sodt_detect_decode_tta" not in r["plain_after"]
    # the first pass is the plain forward itself: scale 1, no flip, rows 0 .. 3 * 192 * 192
    assert torch.equal(z[:, :3 * 192 * 192], r["a"])


def test_augmented_forward_rectangle(dev, ops, T, model512):
    model = model512
    x, ir = _pair(1, 768, 640, 1, seed=6)
    x, ir = x.to(dev), ir.to(dev)
    with torch.no_grad():
        a = model(x, ir, "RGB+IR")[0].clone()
        b = model(x, ir, "RGB+IR")[0].clone()
        (z, second), names = _spy(ops, lambda: model(x, ir, "RGB+IR", augment=True))
    assert torch.equal(a, b), "the plain eval forward is not bit-reproducible at 768 x 640"
    want, sizes = _composition(model, T, x, ir)
    assert second is None and [c for c, _ in sizes] == [(768, 640), (637, 531), (514, 428)]
    assert z.shape == (1, 3 * sum((hp // 4) * (wp // 4) for _, (hp, wp) in sizes), 13)
    assert torch.equal(z.cpu(), want)
    assert names.count("sodt_tta_scale") == 1 and names.count("sodt_detect_decode_tta") == 3


def test_augmented_forward_bf16(dev, model512):
    model = model512
    x, ir = _pair(2, 768, 768, 3, seed=8)
    model.compute_dtype = torch.bfloat16
    try:
        with torch.no_grad():
            z, second = model(x.to(dev), ir.to(dev), augment=True)
    finally:
        model.compute_dtype = torch.float32
    assert second is None and z.shape == (2, 3 * (192 * 192 + 160 * 160 + 144 * 144), 13) and z.dtype == torch.float32
    assert bool(torch.isfinite(z).all())


def test_nms_takes_the_concatenated_rows(pkg, run768):
    """Downstream: the row count is not 3 * ny * nx of any single grid, and both NMS entries take it."""
    nms = importlib.import_module(PKG + ".nms")
    z = run768["out"][0]
    conf = float((z[..., 4:5] * z[..., 5:]).max(-1).values.median())      # random-init scores are tiny: keep about half the rows
    dets, idx = nms.non_max_suppression(z, conf, 0.45, multi_label=False, return_index=True)
    bdets, bidx = nms.non_max_suppression_batch(z, conf, 0.45, multi_label=False).to_list(return_index=True)
    assert len(dets) == len(bdets) == 1 and int(dets[0].shape[0]) > 0
    assert all(torch.equal(a, b) for a, b in zip(idx, bidx))
    assert all(torch.equal(a[:, 4:], b[:, 4:]) for a, b in zip(dets, bdets))


def test_training_mode_is_refused_and_custom_passes_run(dev, ops, T, model512):
    model = model512
    x, ir = _pair(1, 576, 576, 3, seed=9)
    x, ir = x.to(dev), ir.to(dev)
    model.train()
    try:
        with ops.Recorder() as rec:
            with pytest.raises(ValueError, match="eval"):
                model(x, ir, "RGB+IR", augment=True)
        assert rec.calls == []
    finally:
        model.eval()
    model.tta_scales, model.tta_flips = (1, 0.67), (2, None)
    try:
        with torch.no_grad():
            (z, second), names = _spy(ops, lambda: model(x, ir, augment=True))
        want, sizes = _composition(model, T, x, ir)
        model.tta_flips = (2,)
        with pytest.raises(ValueError, match="same length"):
            model(x, ir, augment=True)
    finally:
        model.tta_scales, model.tta_flips = (1, 0.83, 0.67), (None, 3, None)
    assert second is None and [p for _, p in sizes] == [(576, 576), (512, 512)]
    assert z.shape == (1, 3 * (144 * 144 + 128 * 128), 13)
    assert torch.equal(z.cpu(), want)
    assert names.count("sodt_tta_scale") == 1 and names.count("sodt_detect_decode_tta") == 2      # the flipped full-size copy is a pass of the one launch
