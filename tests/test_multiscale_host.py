"""Host side of ``--multi-scale`` (Train.py:396-402), no GPU: ``preprocess.multi_scale_size`` against the integer restatement of
lines 397-400 written out here, its one draw per call, the snap to the sizes ``runs_at`` accepts, and ``Model.runs_at`` on a model
built at 512 (S = 512 and every multiple of 64 from 576: what Engine._block_geo / _block_route run; tests/test_multiscale_gpu.py
holds the predicate against the engine itself)."""
import importlib
import math
import random

import pytest

PKG = "small-object-detection-transformers_amd"


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(PKG + ".preprocess")


def _reference(imgsz, shape, gs, rng):
    """Train.py:397-400 with int() around the two float arguments of randrange"""
    sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5) + gs) // gs * gs
    sf = sz / max(shape)
    if sf != 1:
        return tuple(math.ceil(x * sf / gs) * gs for x in shape)
    return tuple(shape)


@pytest.mark.parametrize("imgsz,shape,gs", [(1024, (512, 512), 32), (640, (480, 640), 32)])
def test_multi_scale_size_is_the_reference_lines(P, imgsz, shape, gs):
    seen = set()
    for seed in range(50):
        got = P.multi_scale_size(imgsz, shape, gs, rng=random.Random(seed))
        assert got == _reference(imgsz, shape, gs, random.Random(seed)), seed
        assert isinstance(got, tuple) and all(isinstance(v, int) and v % gs == 0 for v in got)
        seen.add(got)
    assert len(seen) > 10                                       # the seeds do cover the range
    if shape[0] != shape[1]:
        assert any(h * shape[1] != w * shape[0] for h, w in seen)      # the per-side ceil moves the aspect ratio somewhere


@pytest.mark.parametrize("runs_at", [None, lambda s: s % 64 == 0 and (s == 512 or s >= 576)])
def test_one_draw_per_call(P, runs_at):
    for seed in range(20):
        rng, twin = random.Random(seed), random.Random(seed)
        P.multi_scale_size(512, (512, 512), 64, rng=rng, runs_at=runs_at)
        twin.randrange(256, 768 + 64)
        assert rng.getstate() == twin.getstate(), seed


def test_default_rng_is_the_random_module(P):
    random.seed(11)
    a = P.multi_scale_size(1024, (512, 512))
    assert a == _reference(1024, (512, 512), 32, random.Random(11))


class _Fixed:
    """a random source whose one draw is known"""

    def __init__(self, value):
        self.value, self.calls = value, 0

    def randrange(self, lo, hi):
        assert lo <= self.value < hi
        self.calls += 1
        return self.value


def test_snap_to_the_sizes_the_model_runs(P):
    runs_at = lambda s: s % 64 == 0 and (s == 512 or s >= 576)
    seen = set()
    for seed in range(50):
        h, w = P.multi_scale_size(512, (512, 512), 64, rng=random.Random(seed), runs_at=runs_at)
        assert h == w and h in (512, 576, 640, 704, 768), (seed, h)
        seen.add(h)
    assert len(seen) == 5
    for draw in (256, 300, 448, 511):                           # sz = 256 .. 448: all nearest to 512
        rng = _Fixed(draw)
        assert P.multi_scale_size(512, (512, 512), 64, rng=rng, runs_at=runs_at) == (512, 512) and rng.calls == 1
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(831), runs_at=runs_at) == (768, 768)
    # an accepted draw is left alone, and without a predicate so is a refused one
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(640), runs_at=runs_at) == (640, 640)
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(256)) == (256, 256)


def test_snap_ties_go_to_the_larger_size(P):
    only = lambda *ok: (lambda s: s in ok)
    # 448 lies 64 from 384 and from 512; 512 lies 128 from 384 and from 640
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(448), runs_at=only(384, 512)) == (512, 512)
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(512), runs_at=only(384, 640)) == (640, 640)
    # no tie: the nearer one, smaller or larger
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(448), runs_at=only(384, 576)) == (384, 384)
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(320), runs_at=only(256, 448)) == (256, 256)
    # only sizes the draw itself can give are candidates: 832 and 192 lie outside the reference's range
    assert P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(768), runs_at=only(256, 832)) == (256, 256)
    with pytest.raises(ValueError):
        P.multi_scale_size(512, (512, 512), 64, rng=_Fixed(768), runs_at=only(192, 832))


def test_snap_refuses_when_nothing_runs(P):
    rng = _Fixed(400)
    with pytest.raises(ValueError):
        P.multi_scale_size(512, (512, 512), 64, rng=rng, runs_at=lambda s: False)
    assert rng.calls == 1


def test_snapped_size_keeps_the_per_side_ceil(P):
    # 480 x 640 at a snapped sz = 576: sf = 0.9, ns = (ceil(432 / 64), ceil(576 / 64)) * 64
    got = P.multi_scale_size(512, (480, 640), 64, rng=_Fixed(530), runs_at=lambda s: s >= 576)
    assert got == (448, 576)


def test_model_runs_at(pkg):
    M = importlib.import_module(PKG + ".model")
    m = M.Model("model.yaml", input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)
    assert m.image_encoder.img_size == 512
    assert m._engine is None
    for S in range(32, 1601, 32):
        assert m.runs_at(S) == (S == 512 or (S >= 576 and S % 64 == 0)), S
    for S in (0, -64, 500, 577, 512.0, True):
        assert m.runs_at(S) is False, S
    assert m._engine is None                                   # answered from the module tree: no engine, no library call
