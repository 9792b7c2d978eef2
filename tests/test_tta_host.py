"""Test-time augmentation, host side (no GPU): tests/tta_ref.py against the reference's own results in tests/golden/tta.pt
(tools/gen_tta_golden.py), ``tta.tta_sizes`` with stub and real ``runs_at``, the validation of ``tta_scales`` / ``tta_flips``,
and the order of the refusals of ``Model.forward(augment=True)``."""
import importlib
import os

import pytest
import torch

import tta_ref

PKG = "small-object-detection-transformers_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "tta.pt")


@pytest.fixture(scope="module")
def T(pkg):
    return importlib.import_module(PKG + ".tta")


@pytest.fixture(scope="module")
def M(pkg):
    return importlib.import_module(PKG + ".model")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


# ------------------------------------------------------------------ the restatement against the reference's results
def test_ref_scale_img_matches_reference(gold):
    seen = set()
    for c in gold["scale"]:
        out = tta_ref.scale_img(c["img"].clone(), c["ratio"], c["same_shape"], c["gs"])
        assert out.shape == c["out"].shape and torch.equal(out, c["out"]), c["name"]
        if c["ratio"] == 1.0:
            assert tta_ref.scale_img(c["img"], 1.0) is c["img"]
        elif not c["same_shape"]:
            h, w = c["img"].shape[2:]
            s = (int(h * c["ratio"]), int(w * c["ratio"]))
            pad = tuple(c["out"].shape[2:])
            assert pad == tta_ref.padded_size((h, w), c["ratio"], c["gs"])
            assert torch.equal(tta_ref.scale_img(c["img"].clone(), c["ratio"], padded=pad), c["out"])
            assert bool((c["out"][:, :, s[0]:, :] == 0.447).all()) and bool((c["out"][:, :, :, s[1]:] == 0.447).all())
        seen.add((c["ratio"], c["gs"]))
    assert {(0.83, 32), (0.67, 32), (0.83, 64)} <= seen
    assert any(c["img"].shape[2] != c["img"].shape[3] for c in gold["scale"])
    assert any(c["img"].shape[2] % 2 and c["img"].shape[3] % 2 for c in gold["scale"])


def test_ref_descale_deflip_matches_reference(gold):
    assert {(c["si"], c["fi"]) for c in gold["deflip"]} == {(s, f) for s in (1, 0.83, 0.67) for f in (None, 2, 3)}
    for c in gold["deflip"]:
        yi = c["yi"].clone()
        out = tta_ref.descale_deflip(yi, c["si"], c["fi"], c["img_size"])
        assert torch.equal(out, c["out"]), (c["si"], c["fi"])
        assert torch.equal(yi, c["yi"])                                        # the argument is not modified
        assert torch.equal(out[..., 4:], c["yi"][..., 4:])


def test_descale_is_the_f32_division(gold):
    """What the device kernel restates: ATen's CPU ``yi[..., :4] /= si`` is the IEEE f32 quotient by float32(si), and the
    de-flip subtracts from float32(size)."""
    for c in gold["deflip"]:
        want = c["yi"].clone()
        q = (want[..., :4].double() / float(torch.tensor(c["si"], dtype=torch.float32))).float()      # exact quotient, rounded once
        want[..., :4] = q
        if c["fi"] == 2:
            want[..., 1] = (float(c["img_size"][0]) - want[..., 1].double()).float()
        elif c["fi"] == 3:
            want[..., 0] = (float(c["img_size"][1]) - want[..., 0].double()).float()
        assert torch.equal(want, c["out"]), (c["si"], c["fi"])


def test_ref_composition_concatenates_the_passes():
    x = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(3))
    ir = torch.rand(1, 1, 64, 96, generator=torch.Generator().manual_seed(4))
    seen = []

    def forward(xi, iri):                       # a stand-in decode: one row per 4 x 4 cell, columns 0 / 1 hold the cell's centre
        seen.append((xi, iri))
        ny, nx = xi.shape[2] // 4, xi.shape[3] // 4
        z = torch.zeros(1, ny * nx, 6)
        z[0, :, 0] = (torch.arange(nx).float() * 4 + 2).repeat(ny)
        z[0, :, 1] = (torch.arange(ny).float() * 4 + 2).repeat_interleave(nx)
        z[0, :, 4] = xi.mean()
        return z
    padded = [(64, 96), (64, 96), (64, 64)]
    z = tta_ref.augmented_forward(forward, x, ir, (1, 0.83, 0.67), (None, 3, None), padded)
    assert z.shape == (1, 16 * 24 + 16 * 24 + 16 * 16, 6)
    assert seen[0][0] is x and seen[0][1] is ir
    assert seen[1][0].shape == (1, 3, 64, 96) and seen[2][0].shape == (1, 3, 64, 64) and seen[2][1].shape == (1, 1, 64, 64)
    assert torch.equal(seen[1][0], tta_ref.scale_img(x.flip(3), 0.83, padded=(64, 96)))
    assert torch.equal(z[0, :384, 0], (torch.arange(24).float() * 4 + 2).repeat(16))
    assert torch.equal(z[0, 384, :2], torch.stack([96 - torch.tensor(2.0) / 0.83, torch.tensor(2.0) / 0.83]))
    assert torch.equal(z[0, 768, :2], torch.tensor(2.0).repeat(2) / 0.67)


# ------------------------------------------------------------------ tta_sizes
def test_sizes_accepted_at_once(T):
    calls = []

    def runs_at(s):
        calls.append(s)
        return True
    got = T.tta_sizes((768, 768), (1, 0.83, 0.67), 32, runs_at)
    assert got == [((768, 768), (768, 768)), ((637, 637), (640, 640)), ((514, 514), (544, 544))]
    assert calls == [(640, 640), (544, 544)]                     # one question per scaled pass, none for the scale of 1
    assert T.tta_sizes((768, 640), (0.83,), 64, None) == [((637, 531), (640, 576))]          # no runs_at: the reference's formula
    assert T.tta_sizes((100, 60), (0.67,), 32) == [((67, 40), (96, 64))]


def test_sizes_bumped_on_one_side(T):
    got = T.tta_sizes((768, 640), (0.83,), 32, lambda s: s[1] >= 576)
    assert got == [((637, 531), (640, 576))]                      # from (640, 544): the width alone moves
    got = T.tta_sizes((640, 768), (0.83,), 32, lambda s: s[0] >= 576)
    assert got == [((531, 637), (576, 640))]


def test_sizes_fall_back_to_the_input_size(T):
    assert T.tta_sizes((768, 768), (0.83, 0.67), 32, lambda s: s == (768, 768)) == [((637, 637), (768, 768)), ((514, 514), (768, 768))]
    # (H, W) is a candidate even where the 32-pixel grid from the start does not reach it
    assert T.tta_sizes((100, 100), (0.67,), 32, lambda s: s == (100, 100)) == [((67, 67), (100, 100))]
    with pytest.raises(ValueError, match="accepted by runs_at"):
        T.tta_sizes((768, 768), (0.83,), 32, lambda s: False)


def test_sizes_tie_goes_to_the_smaller_height(T):
    ok = {(576, 640), (640, 576), (768, 768)}
    assert T.tta_sizes((768, 768), (0.67,), 32, lambda s: s in ok) == [((514, 514), (576, 640))]
    ok = {(640, 576), (608, 608)}                                 # the smaller area wins before the tie rule
    assert T.tta_sizes((768, 768), (0.67,), 32, lambda s: s in ok) == [((514, 514), (640, 576))]


@pytest.fixture(scope="module")
def model512(M):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "configs", "SRyolo_MF.yaml")))
    cfg["backbone"][0][3][0] = 512
    return M.Model(cfg, input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)


def test_sizes_with_the_real_runs_at(T, model512):
    m = model512
    assert not m.pad_shifted_blocks
    # 512 on a model built at 512: 448 and 352 are refused, and so is 480: both scaled copies pad to 512 itself
    assert T.tta_sizes((512, 512), (1, 0.83, 0.67), 32, m.runs_at) == [((512, 512), (512, 512)), ((424, 424), (512, 512)),
                                                                       ((343, 343), (512, 512))]
    # 768: 640 runs as it is, 544 moves to 576
    got = T.tta_sizes((768, 768), (1, 0.83, 0.67), 32, m.runs_at)
    assert got == [((768, 768), (768, 768)), ((637, 637), (640, 640)), ((514, 514), (576, 576))]
    # a rectangle: every padded pair is one runs_at accepts, holds the content, and no accepted pair of the grid is smaller
    got = T.tta_sizes((768, 640), (1, 0.83, 0.67), 32, m.runs_at)
    assert [c for c, _ in got] == [(768, 640), (637, 531), (514, 428)]
    for si, ((h, w), (hp, wp)) in zip((1, 0.83, 0.67), got):
        assert m.runs_at((hp, wp)) and h <= hp <= 768 and w <= wp <= 640
        if si != 1:
            h0, w0 = tta_ref.padded_size((768, 640), si, 32)
            smaller = [(a, b) for a in range(h0, 769, 32) for b in range(w0, 641, 32)
                       if m.runs_at((a, b)) and (a * b, a) < (hp * wp, hp)]
            assert not smaller, smaller
    assert got[1][1] == (640, 576) and got[2][1] == (576, 512)
    m.pad_shifted_blocks = True                                   # with the switch every multiple of 32 from 576 runs, and 544
    try:
        assert T.tta_sizes((768, 768), (0.67,), 32, m.runs_at) == [((514, 514), (544, 544))]
    finally:
        m.pad_shifted_blocks = False


# ------------------------------------------------------------------ validation
def test_check_passes(T):
    assert T.check_passes((1, 0.83, 0.67), (None, 3, None)) == ((1, 0.83, 0.67), (0, 3, 0))
    assert T.check_passes([1, 0.67], [2, None]) == ((1, 0.67), (2, 0))
    assert T.check_passes((1.0,) * 4, (None, 2, 3, None))[1] == (0, 2, 3, 0)
    assert (T.SCALES, T.FLIPS, T.MAX_PASSES) == ((1, 0.83, 0.67), (None, 3, None), 4)
    for scales, flips in [((1, 0.83), (None,)), ((), ()), ((1,) * 5, (None,) * 5), ((1, 0.83), (None, 1)), ((1, 0.83), (None, 4)),
                          ((1, 0.83), (None, True)), ((1, 0.0), (None, None)), ((1, -0.5), (None, None)), ((1, 1.5), (None, None)),
                          ((1, "0.83"), (None, None)), ((1, float("nan")), (None, None)), (0.83, None), ((1, True), (None, None))]:
        with pytest.raises(ValueError):
            T.check_passes(scales, flips)


def test_model_defaults_are_the_references(M, T):
    m = M.Model("model.yaml", input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)
    assert m.tta_scales == (1, 0.83, 0.67) and m.tta_flips == (None, 3, None)          # model.py:157-158
    assert max(int(m.stride.max()), 32) == 32


# ------------------------------------------------------------------ the refusals of forward(augment=True), in order
def test_augment_refusals(M):
    m = M.Model("model.yaml", input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)
    x = torch.zeros(1, 3, 64, 64)
    m.eval()
    with pytest.raises(NotImplementedError):                      # the input_mode check stays first
        m(x, x, "RGB", augment=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x, "RGB+IR", augment=True)
    m.train()
    with pytest.raises(ValueError, match="eval"):                 # training mode: before the device check
        m(x, x, "RGB+IR", augment=True)
    with pytest.raises(NotImplementedError):
        m(x, x, "RGB", augment=True)
    m.eval()
    m.export = True
    with pytest.raises(ValueError, match="eval"):
        m(x, x, "RGB+IR", augment=True)
    m.export = False
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # and the plain forward refuses as it did
        m(x, x, "RGB+IR")


def test_scale_helpers_refuse_cpu_tensors(T):
    x = torch.zeros(1, 3, 64, 64)
    assert T.scale_img(x, 1.0) is x                               # torch_utils.py:251-252
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.scale_img(x, 0.83)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.scale_pair(x, x, [((53, 53), (64, 64), 3)])
