"""The three BatchNorm+SiLU row-streaming kernels of csrc/head.hip on their own, through the C ABI: sodt_bn_silu_fwd,
sodt_bn_silu_bwd_reduce and sodt_bn_silu_bwd_apply.  A thread of these kernels keeps one 16-byte channel group for the whole launch
and walks several rows per trip, so the cases are chosen around that walk:

* M = 1 and 3: fewer rows than one pass of a workgroup (256 / (C / KPL) rows: 32, 16, 8 in bf16 and 16, 8, 4 in f32 at C = 64, 128,
  256), most threads of the workgroup have no row at all;
* M = 257: a ragged last trip (a trip is several passes; rows past M are zero-filled on the way in and must not be stored);
* M = 4099: more than one workgroup, a prime number of rows, the grid stride in use;
* dy as the right half of a buffer twice as wide (lddy = 2 C, dy_off = C), the way the C3 backward hands it over; the left half
  is NaN.

Every operand lies between two rows of NaN (tests/test_sr_movement_gpu.py::_guarded), so a read outside a view poisons the result,
and every output lies inside a buffer of sentinels that are compared afterwards, so a write outside it shows.

References: the kernels' sigmoid is the hardware exp and reciprocal approximation (csrc/common.h: sigmoid_f), which torch cannot
reproduce bit for bit, so the reference is the kernel's expression evaluated in float64 from the very inputs the kernel gets (mean and
rstd as the f32 values handed over), at the tolerances of tests/test_kernels_gpu.py::test_bn_silu (its `close`).  That dz is bit
for bit what the previous kernel gave is checked where both exist, by `tools/ab_norm.py --check --parent-lib`.  What IS exact here:
dgamma / dbeta are their old value plus (float)red, added once.
"""
import functools

import pytest
import torch

from test_kernels_gpu import close, rnd
from test_sr_movement_gpu import _guarded

pytestmark = pytest.mark.gpu

DTS = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")]
SHAPES = [(M, Cc) for M in (1, 3, 257, 4099) for Cc in (64, 128, 256)]
SENT = 7.0


def _cpu(shape, dt, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


@functools.lru_cache(maxsize=None)
def _case(dt, M, Cc, dev):
    """inputs (guarded, on the device) and the float64 reference of everything the three kernels compute; never modified"""
    z = _guarded(_cpu((M, Cc), dt, 1, 1.5) + 0.3, dev)
    dy = _guarded(_cpu((M, Cc), dt, 4), dev)
    g = rnd((Cc,), dev, torch.float32, 2) * 0.2 + 1
    b = rnd((Cc,), dev, torch.float32, 3) * 0.2
    zd = z.double()
    mr = torch.stack([zd.mean(0), 1 / torch.sqrt(zd.var(0, unbiased=False) + 1e-3)]).float().contiguous()
    mu, rs, ga, be = mr[0].double(), mr[1].double(), g.double(), b.double()
    xh = (zd - mu) * rs
    a = xh * ga + be
    sg = torch.sigmoid(a)
    gg = dy.double() * sg * (1 + a * (1 - sg))
    red = torch.stack([gg.sum(0), (gg * xh).sum(0)])
    dz = ga * rs * (gg - red[0] / M - xh * (red[1] / M))
    return dict(z=z, dy=dy, g=g, b=b, mr=mr, y=a * sg, red=red, dz=dz, sumabs=float(gg.abs().sum(0).max()),
                terms=float((ga * rs * gg).abs().max()))


def _in_sentinels(M, Cc, ld, dt, dev, rows=2):
    """a [M][ld] view whose first Cc columns the kernel may write, inside a buffer of SENT"""
    buf = torch.full((M + 2 * rows, ld), SENT, device=dev, dtype=dt)
    return buf, buf[rows: rows + M]


def _sentinels_kept(buf, M, Cc, rows=2):
    return bool((buf[:rows] == SENT).all()) and bool((buf[rows + M:] == SENT).all()) and bool((buf[rows: rows + M, Cc:] == SENT).all())


def _dy_slice(c, M, Cc, dev):
    """dy as the right half of a [M][2 C] buffer between NaN rows, the left half NaN"""
    wide = torch.full((M + 4, 2 * Cc), float("nan"), dtype=c["dy"].dtype)
    wide[2: 2 + M, Cc:] = c["dy"].cpu()
    return wide.to(dev)[2: 2 + M]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,Cc", SHAPES)
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "slice"])
def test_bn_silu_fwd(ops, dev, dt, M, Cc, wide):
    c = _case(dt, M, Cc, dev)
    ld = 2 * Cc if wide else Cc
    buf, y = _in_sentinels(M, Cc, ld, dt, dev)
    ops.bn_silu_fwd(c["z"], c["mr"], c["g"], c["b"], y, ld, M, Cc)
    close(y[:, :Cc], c["y"], dt, what="bn silu fwd")
    assert _sentinels_kept(buf, M, Cc), "bn_silu_fwd wrote outside its M x C view"


def _reduce_twice(ops, dev, c, dy, lddy, M, Cc, dt, dy_off=0):
    buf = torch.full((4, Cc), SENT, device=dev, dtype=torch.float64)
    red = buf[1:3]
    red.zero_()
    ops.bn_silu_bwd_reduce(dy, lddy, c["z"], c["mr"], c["g"], c["b"], red, M, Cc, dy_off=dy_off)
    one = red.clone()
    close(one, c["red"], dt, what="bn bwd sums")
    ops.bn_silu_bwd_reduce(dy, lddy, c["z"], c["mr"], c["g"], c["b"], red, M, Cc, dy_off=dy_off)
    # the second call adds the same f32 partials of the same workgroups; only the order of the f64 additions may differ:
    # at most a few thousand of them, each within 2^-53 of a running sum that sum |g| bounds
    err = float((red - 2 * one).abs().max())
    print(f"second call: |red - 2 red1| = {err:.3e}, sum |g| = {c['sumabs']:.3e}")
    assert err <= 1e-12 * max(c["sumabs"], 1e-30), "two calls on the same inputs must accumulate to twice the sums"
    assert bool((buf[0] == SENT).all()) and bool((buf[3] == SENT).all()), "bn_silu_bwd_reduce wrote outside red"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,Cc", SHAPES)
def test_bn_silu_bwd_reduce(ops, dev, dt, M, Cc):
    c = _case(dt, M, Cc, dev)
    _reduce_twice(ops, dev, c, c["dy"], Cc, M, Cc, dt)


@pytest.mark.parametrize("dt", DTS)
def test_bn_silu_bwd_reduce_dy_slice(ops, dev, dt):
    M, Cc = 257, 128
    c = _case(dt, M, Cc, dev)
    _reduce_twice(ops, dev, c, _dy_slice(c, M, Cc, dev), 2 * Cc, M, Cc, dt, dy_off=Cc)


def _apply(ops, dev, c, dy, lddy, M, Cc, dt, dy_off=0):
    red = c["red"].clone()
    buf, dz = _in_sentinels(M, Cc, Cc, dt, dev)
    dg0, db0 = rnd((Cc,), dev, torch.float32, 5), rnd((Cc,), dev, torch.float32, 6)
    dg, db = dg0.clone(), db0.clone()
    ops.bn_silu_bwd_apply(dy, lddy, c["z"], c["mr"], c["g"], c["b"], red, dz, dg, db, M, Cc, dy_off=dy_off)
    # close() scales its bound by max |reference|.  With one row the reference is identically zero (g - mean g and xhat both vanish)
    # while the kernel returns the f32 rounding of the two terms it subtracts, so there the scale is that of the terms, gamma rstd g
    close(dz, c["dz"], dt, scale=float(c["dz"].abs().max()) or c["terms"], what="bn dz")
    assert _sentinels_kept(buf, M, Cc), "bn_silu_bwd_apply wrote outside dz"
    assert torch.equal(red, c["red"]), "bn_silu_bwd_apply changed red"
    assert torch.equal(db, db0 + red[0].float()), "dbeta is not its old value plus (float)red[0], added once"
    assert torch.equal(dg, dg0 + red[1].float()), "dgamma is not its old value plus (float)red[1], added once"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,Cc", SHAPES)
def test_bn_silu_bwd_apply(ops, dev, dt, M, Cc):
    c = _case(dt, M, Cc, dev)
    _apply(ops, dev, c, c["dy"], Cc, M, Cc, dt)


@pytest.mark.parametrize("dt", DTS)
def test_bn_silu_bwd_apply_dy_slice(ops, dev, dt):
    M, Cc = 257, 128
    c = _case(dt, M, Cc, dev)
    _apply(ops, dev, c, _dy_slice(c, M, Cc, dev), 2 * Cc, M, Cc, dt, dy_off=Cc)
