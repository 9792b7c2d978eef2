"""Host side of ``--quad`` (LoadImagesAndLabels.collate_fn4, basics/utils/datasets.py:637-664), no GPU: tests/quad_ref.py against
the outputs the reference's own function gave (tests/golden/quad.pt, written by tools/gen_quad_golden.py), ``preprocess.quad_modes``
against the recorded draws, ``preprocess.quad_targets`` on CPU tensors against the recorded labels bit for bit, and the two new
entries in the header and the binding."""
import importlib
import os
import random

import pytest
import torch

from quad_ref import plain_targets, quad_ref

PKG = "small-object-detection-transformers_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(PKG + ".preprocess")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "quad.pt"))


def test_golden_covers_the_cases(golden):
    shapes = {(tuple(c["imgs"].shape), c["irs"].shape[1]) for c in golden}
    for want in (((4, 3, 8, 8), 3), ((8, 3, 5, 7), 1), ((9, 3, 16, 12), 3), ((4, 3, 1, 9), 3)):
        assert want in shapes, want
    mixed = [c for c in golden if c["imgs"].shape == (12, 3, 24, 40)]
    assert mixed and all(len(set(c["modes"])) == 2 for c in mixed)
    assert any(all(c["modes"]) and len(c["modes"]) > 1 for c in golden) and any(not any(c["modes"]) and len(c["modes"]) > 1 for c in golden)
    for c in golden:
        assert all(int(x.min()) == 0 and int(x.max()) == 255 for x in c["imgs"])
        assert all(0 <= l.shape[0] <= 5 for l in c["labels"]) and any(l.shape[0] == 0 for l in c["labels"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "quad.pt")) < 200 * 1024


def test_quad_ref_is_the_reference(golden):
    for c in golden:
        ins = [c["imgs"].clone(), c["irs"].clone(), [l.clone() for l in c["labels"]]]
        img4, ir4, label4 = quad_ref(*ins, c["modes"])
        assert img4.dtype == ir4.dtype == torch.uint8 and label4.dtype == torch.float32
        assert torch.equal(img4, c["img4"]) and torch.equal(ir4, c["ir4"]) and torch.equal(label4, c["label4"]), c["name"]
        assert torch.equal(ins[0], c["imgs"]) and torch.equal(ins[1], c["irs"])          # and the inputs come back unchanged
        assert all(torch.equal(a, b) for a, b in zip(ins[2], c["labels"]))


def test_quad_modes_are_the_recorded_draws(P, golden):
    for c in golden:
        B = c["imgs"].shape[0]
        got = P.quad_modes(B, rng=random.Random(c["seed"]))
        assert got == tuple(c["modes"]) and isinstance(got, tuple) and all(isinstance(m, bool) for m in got), c["name"]
        random.seed(c["seed"])                                   # the default source is the random module, as in the reference
        assert P.quad_modes(B) == tuple(c["modes"])


@pytest.mark.parametrize("B", [4, 7, 9, 64, 259])
def test_quad_modes_take_one_draw_per_group(P, B):
    for seed in range(5):
        rng, twin = random.Random(seed), random.Random(seed)
        modes = P.quad_modes(B, rng=rng)
        plain = [twin.random() for _ in range(B // 4)]
        assert rng.getstate() == twin.getstate()
        assert modes == tuple(v < 0.5 for v in plain)


@pytest.mark.parametrize("B", [3, 260, 0, -4])
def test_quad_modes_refuse_the_batch(P, B):
    rng = random.Random(0)
    state = rng.getstate()
    with pytest.raises(ValueError):
        P.quad_modes(B, rng=rng)
    assert rng.getstate() == state


def test_quad_targets_are_the_reference_labels(P, golden):
    for c in golden:
        targets = plain_targets(c["labels"])
        before = targets.clone()
        got = P.quad_targets(targets, tuple(c["modes"]))
        assert got.dtype == torch.float32 and got.shape == c["label4"].shape, c["name"]
        assert torch.equal(got, c["label4"]), c["name"]
        assert bool((got.view(torch.int32) == c["label4"].view(torch.int32)).all()), c["name"]      # bit for bit
        assert got.shape[0] == 0 or int(got[:, 0].max()) < len(c["modes"])
        assert torch.equal(targets, before)


def test_quad_targets_edges(P):
    out = P.quad_targets(torch.zeros(0, 6), (True, False))
    assert out.shape == (0, 6) and out.dtype == torch.float32
    # sample 9 of a batch of 10 lies past 4n = 8; samples 1 .. 3 of the zoom group 0 disappear
    t = torch.tensor([[i, 1., .25, .5, .1, .2] for i in range(10)])
    out = P.quad_targets(t, (True, False))
    assert out[:, 0].tolist() == [0., 1., 1., 1., 1.]
    assert out[0].tolist() == t[0].tolist()
    assert torch.equal(out[1:, 2], torch.tensor([.125, .125, .625, .625])) and torch.equal(out[1:, 3], torch.tensor([.25, .75, .25, .75]))
    assert bool((out[:, 0] < 2).all())
    for bad in ((), (1, 0), tuple([True] * 65), ("a",)):
        with pytest.raises(ValueError):
            P.quad_targets(t, bad)


def test_header_declares_and_lib_binds_the_entries(pkg):
    # declared, exported and bound type for type: tests/test_abi_and_host.py, for every entry; the arities stay pinned here
    assert len(pkg._lib.SIGNATURES["sodt_quad_u8"]) == 11 and len(pkg._lib.SIGNATURES["sodt_preprocess_u8_quad"]) == 13
