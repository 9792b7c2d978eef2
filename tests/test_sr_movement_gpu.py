"""The data movement between the SR branch's convolutions (csrc/sr.hip), each kernel on its own through the C ABI: bilinear x2
(align_corners=True) and its adjoint, PixelShuffle(2) both ways, add_rows, and the (B, C, H, W) f32 <-> token-major converters that
tests/test_sr_gpu.py uses as helpers.  References are plain torch in float64 or exact torch permutations / casts; inputs come from
seeded CPU generators; every output buffer is pre-filled with a sentinel where the kernel must not write, and those regions are
compared too.

Which case fails for which fault (each claim was checked by handing the comparison a deliberately wrong result on the CPU):
* wrong corner alignment (align_corners=False map): every bilinear case with an extent >= 2; (1, 2, 2, 8) is the smallest - output 1
  reads the source at 1/3, the half-pixel map puts it at 1/4, an error of |x1 - x0| / 12.
* border clamp: with align_corners=True the last output of an axis sits exactly on the last input, so its "+ 1" neighbour carries the
  weight 0: a missing clamp changes no value, it READS outside x (one pixel, or one row past the last image).  x and dy therefore
  lie between rows of NaN (more than one image row on either side), and 0 * NaN = NaN fails every bilinear case; so does a missing
  o < 0 / o >= 2n test in the backward's scan.  The axis-of-length-1 cases (2, 1, 1, 8), (1, 1, 7, 8), (1, 6, 1, 16) are where BOTH
  neighbours clamp to pixel 0 and the map's 0 / 1 must not divide 0 by 0.
* swapped axes (wx <-> wy, or H <-> W in the map): the non-square cases (2, 5, 7, 24), (1, 3, 40, 64), (2, 6, 5, 32), (1, 64, 33, 64);
  a square grid such as (1, 2, 2, 8) cannot see it.
* missed adjoint term: test_bilinear_up2_bwd against float64 autograd element by element (one dropped term is a whole weight
  times dy, >= 1e-2 |dy| against a bound of 8e-5 max|dy|) and test_bilinear_adjoint_identity.
* sub-pixel order: test_pixel_shuffle2 (values distinct per element, compared bit for bit; (2, 3, 5) and (3, 7, 6) are non-square so
  that an i <-> j swap cannot hide).
* slice addressing: test_bilinear_up2_fwd_column_slice, test_bilinear_up2_bwd_column_slice, test_add_rows[slice],
  test_add_rows_short_f32_row (sentinels left and right of the slice, NaN in the columns that must not be read).
* grid-stride pass: the *_grid_stride cases (more than 8192 * 256 chunks; a kernel that does not stride leaves the sentinel in the
  tail, one that strides wrongly misplaces it).
* pad overwrite: the converter tests (pad columns must be written as +0, the row after the last and the element after the last keep
  their sentinel).
* rounding mode: test_rows_from_nchw_and_back (bf16 ties to even in both directions, the overflow to inf, NaN kept)."""
import pytest
import torch
import torch.nn.functional as F

from exact_cases import BF16, F32, IVIEW, bits_equal as _bits_equal, gen as _gen, values as _values

pytestmark = pytest.mark.gpu

DTS = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
SENT = 7.0


def _guarded(t, dev, rows=2):
    """t [M][C] on the device between `rows` rows of NaN: a read outside the tensor poisons the result"""
    M, C = t.shape
    buf = torch.full((M + 2 * rows, C), float("nan"), dtype=t.dtype)
    buf[rows: rows + M] = t
    return buf.to(dev)[rows: rows + M]


# ------------------------------------------------------------------------------------------------ bilinear x2
UP_SHAPES = [(2, 1, 1, 8), (1, 1, 7, 8), (1, 6, 1, 16), (1, 2, 2, 8), (2, 5, 7, 24), (1, 3, 40, 64), (2, 6, 5, 32), (1, 64, 33, 64)]
UP_BIG = (1, 256, 264, 64)          # 512 * 528 * 64 / 8 = 2.16 M bf16 chunks (4.3 M in f32) > 8192 * 256 = 2.10 M
UP_BWD_BIG = (1, 128, 264, 256)     # 128 * 264 * 256 / 4 = 2.16 M f32 input chunks


def _up_ref(x, B, H, W, C):
    """x [B*H*W][C] (any float dtype, any device) -> float64 [B*4HW][C]"""
    xn = x.double().view(B, H, W, C).permute(0, 3, 1, 2)
    y = F.interpolate(xn, scale_factor=2, mode="bilinear", align_corners=True)
    return y.permute(0, 2, 3, 1).reshape(B * 4 * H * W, C)


def _up_bwd_ref(dy, B, H, W, C):
    """float64 autograd of _up_ref: dy [B*4HW][C] -> [B*H*W][C]"""
    x = torch.zeros(B * H * W, C, dtype=torch.float64, device=dy.device, requires_grad=True)
    _up_ref(x, B, H, W, C).backward(dy.double())
    return x.grad


def _lerp_check(got, ref, amax, dt, n, what):
    """f32: |got - ref| <= 2e-5 * amax for extents n <= 64 (scaled by n / 64 above).  The source coordinate o (n - 1) / (2n - 1) has
    an exact product and a correctly rounded divide: half an ulp of a value below 64 = 1.9e-6 per axis, times a neighbour difference
    of at most 2 amax, on two axes, plus the three lerp roundings: under 1e-5 amax; the bound allows a factor two over that.
    bf16: one more rounding of the stored result, at most 2^-8 |ref| (half a bf16 ulp)."""
    bound = 2e-5 * max(1.0, n / 64.0) * amax + (2.0 ** -8 * ref.abs() if dt == BF16 else 0.0)
    err = (got.double() - ref).abs()
    assert not bool(err.isnan().any()), f"{what}: NaN in the result (a read outside the input, or an unwritten element)"
    ratio = float((err / bound).max())
    print(f"{what}: max |err| = {float(err.max()):.3e}, worst err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error is {ratio:.3f} x the bound"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,W,C", UP_SHAPES)
def test_bilinear_up2_fwd(ops, dev, B, H, W, C, dt):
    """sodt_bilinear_up2_fwd against float64 F.interpolate(align_corners=True) of the same (bf16-rounded) input.  Catches: corner
    alignment (every case with an extent >= 2), border clamp (x lies between NaN rows: an unclamped neighbour reads them; the
    length-1 axes clamp both neighbours), swapped axes (the non-square cases)."""
    x = torch.randn(B * H * W, C, generator=_gen(100 * H + W)).to(dt)
    Mo = B * 4 * H * W
    y = torch.full((Mo + 1, C), SENT, dtype=dt, device=dev)
    ops.bilinear_up2_fwd(_guarded(x, dev, W + 2), y[:Mo], B, H, W, C)
    y = y.cpu()
    _lerp_check(y[:Mo], _up_ref(x, B, H, W, C), float(x.abs().max()), dt, max(H, W), f"up2 fwd {(B, H, W, C)} {dt}")
    assert bool((y[Mo] == SENT).all()), "wrote past the last output row"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ycol", [0, 16])
def test_bilinear_up2_fwd_column_slice(ops, dev, ycol, dt):
    """y is columns [ycol, ycol + C) of a wider buffer (ldy = C + 16): the slice holds the result, every other column keeps its
    sentinel.  Catches slice addressing (ldy taken for C, or the column offset dropped)."""
    B, H, W, C = 2, 5, 7, 24
    ld = C + 16
    x = torch.randn(B * H * W, C, generator=_gen(3)).to(dt)
    Mo = B * 4 * H * W
    y = torch.full((Mo + 1, ld), SENT, dtype=dt, device=dev)
    ops.bilinear_up2_fwd(_guarded(x, dev, W + 2), y[:Mo], B, H, W, C, ldy=ld, ycol=ycol)
    y = y.cpu()
    _lerp_check(y[:Mo, ycol: ycol + C], _up_ref(x, B, H, W, C), float(x.abs().max()), dt, max(H, W), f"up2 fwd slice ycol={ycol} {dt}")
    outside = torch.ones(ld, dtype=torch.bool)
    outside[ycol: ycol + C] = False
    assert bool((y[:Mo, outside] == SENT).all()) and bool((y[Mo] == SENT).all()), "wrote outside the column slice"


@pytest.mark.parametrize("dt", DTS)
def test_bilinear_up2_fwd_grid_stride(ops, dev, dt):
    """More 16-byte chunks than the 8192 x 256 threads of the capped launch: in f32 (4.3 M chunks) every thread takes a second pass, in bf16 (2.16 M) the first 3 % do.  The float64
    reference is evaluated by torch on the device.  Extent 264 > 64: the f32 bound scales by 264 / 64 (the divide's half ulp grows
    with the coordinate)."""
    B, H, W, C = UP_BIG
    assert B * 4 * H * W * C // (4 if dt == F32 else 8) > 8192 * 256
    x = torch.randn(B * H * W, C, generator=_gen(11)).to(dt).to(dev)
    Mo = B * 4 * H * W
    y = torch.full((Mo + 1, C), SENT, dtype=dt, device=dev)
    ops.bilinear_up2_fwd(x, y[:Mo], B, H, W, C)
    _lerp_check(y[:Mo], _up_ref(x, B, H, W, C), float(x.abs().max()), dt, max(H, W), f"up2 fwd grid-stride {dt}")
    assert bool((y[Mo] == SENT).all())


def _relu_out(M, C, dt, seed):
    """the activation a ReLU left behind, with exact zeros AND (as a plain mask operand) negative values"""
    r = torch.randn(M, C, generator=_gen(seed))
    r[r.abs() < 0.4] = 0.0
    r.view(-1)[0], r.view(-1)[-1] = 0.0, -1.5
    return r.to(dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("B,H,W,C", UP_SHAPES)
def test_bilinear_up2_bwd(ops, dev, B, H, W, C, masked, dt):
    """sodt_bilinear_up2_bwd against float64 autograd of F.interpolate(align_corners=True), with and without the ReLU mask
    (reference: grad * (relu_out > 0); relu_out holds exact zeros and negative values, both of which must block).  Bound as for the
    forward with 4 max|dy| for max|x|: an input pixel collects at most 16 terms whose weights sum to 4 in the interior.  Catches a
    missed adjoint term (a whole weight times dy), the clamps at the border (length-1 axes: both neighbours are pixel 0 and the
    weight is 1, not 1 - w + w rounded twice) and swapped axes (non-square cases)."""
    Mo, Mi = B * 4 * H * W, B * H * W
    dy = torch.randn(Mo, C, generator=_gen(200 * H + W)).to(dt)
    r = _relu_out(Mi, C, dt, 7 * H + W) if masked else None
    dx = torch.full((Mi + 1, C), SENT, dtype=dt, device=dev)
    ops.bilinear_up2_bwd(_guarded(dy, dev, 4 * W + 4), dx[:Mi], B, H, W, C, relu_out=None if r is None else _guarded(r, dev))
    dx = dx.cpu()
    ref = _up_bwd_ref(dy, B, H, W, C)
    if masked:
        ref = ref * (r.double() > 0)
    _lerp_check(dx[:Mi], ref, 4 * float(dy.abs().max()), dt, max(H, W), f"up2 bwd {(B, H, W, C)} relu={masked} {dt}")
    assert bool((dx[Mi] == SENT).all())


@pytest.mark.parametrize("dt", DTS)
def test_bilinear_up2_bwd_column_slice(ops, dev, dt):
    """dy is columns [8, 8 + C) of a wider buffer (lddy = C + 8) whose other columns hold NaN: reading them poisons dx."""
    B, H, W, C = 2, 5, 7, 24
    ld, col = C + 8, 8
    Mo, Mi = B * 4 * H * W, B * H * W
    dy = torch.randn(Mo, C, generator=_gen(5)).to(dt)
    wide = torch.full((Mo, ld), float("nan"), dtype=dt)
    wide[:, col: col + C] = dy
    dx = torch.full((Mi + 1, C), SENT, dtype=dt, device=dev)
    ops.bilinear_up2_bwd(_guarded(wide, dev, 4 * W + 4), dx[:Mi], B, H, W, C, lddy=ld, dycol=col)
    dx = dx.cpu()
    _lerp_check(dx[:Mi], _up_bwd_ref(dy, B, H, W, C), 4 * float(dy.abs().max()), dt, max(H, W), f"up2 bwd slice {dt}")
    assert bool((dx[Mi] == SENT).all())


def test_bilinear_up2_bwd_grid_stride(ops, dev):
    """More input chunks than 8192 x 256 threads (f32); float64 autograd on the device; bound scaled by 264 / 64."""
    B, H, W, C = UP_BWD_BIG
    assert B * H * W * C // 4 > 8192 * 256
    Mo, Mi = B * 4 * H * W, B * H * W
    dy = torch.randn(Mo, C, generator=_gen(13)).to(dev)
    dx = torch.full((Mi + 1, C), SENT, device=dev)
    ops.bilinear_up2_bwd(dy, dx[:Mi], B, H, W, C)
    _lerp_check(dx[:Mi], _up_bwd_ref(dy, B, H, W, C), 4 * float(dy.abs().max()), F32, max(H, W), "up2 bwd grid-stride f32")
    assert bool((dx[Mi] == SENT).all())


@pytest.mark.parametrize("B,H,W,C", UP_SHAPES)
def test_bilinear_adjoint_identity(ops, dev, B, H, W, C):
    """<up(x), dy> = <x, up^T(dy)>, summed in float64 from the two kernels' own f32 outputs, within 1e-5 |up(x)| |dy| (each side
    carries a few f32 roundings per element, ~1e-7 relative).  The forward takes its stencil from the output pixel, the backward
    scans output pixels [2i - 2, 2i + 2] around the input pixel: a term that scan misses breaks the identity."""
    x = torch.randn(B * H * W, C, generator=_gen(31 * H + W))
    dy = torch.randn(B * 4 * H * W, C, generator=_gen(37 * H + W))
    up = torch.full((B * 4 * H * W, C), SENT, device=dev)
    dx = torch.full((B * H * W, C), SENT, device=dev)
    ops.bilinear_up2_fwd(x.to(dev), up, B, H, W, C)
    ops.bilinear_up2_bwd(dy.to(dev), dx, B, H, W, C)
    up, dx = up.cpu().double(), dx.cpu().double()
    lhs, rhs = float((up * dy.double()).sum()), float((x.double() * dx).sum())
    tol = 1e-5 * float(up.norm()) * float(dy.double().norm())
    print(f"adjoint {(B, H, W, C)}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {tol:.3e}")
    assert abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------ PixelShuffle(2)
def _distinct(n, dt):
    """n values, no two equal within any window of 32512 (bf16) / 2^24 (f32) consecutive elements, all finite and exact in dt"""
    if dt == BF16:
        return (torch.arange(n, dtype=torch.int32) % 32512).to(torch.int16).view(BF16)          # every finite positive bit pattern
    return (torch.arange(n, dtype=torch.int64) % (1 << 24)).float()


def _shuffle_ref(x, B, H, W, C):
    """x [B*H*W][4C] -> [B*2H*2W][C] as nn.PixelShuffle(2) on the NCHW view"""
    y = F.pixel_shuffle(x.view(B, H, W, 4 * C).permute(0, 3, 1, 2), 2)
    return y.permute(0, 2, 3, 1).reshape(B * 4 * H * W, C).contiguous()


def _unshuffle_ref(y, B, H, W, C):
    x = F.pixel_unshuffle(y.view(B, 2 * H, 2 * W, C).permute(0, 3, 1, 2), 2)
    return x.permute(0, 2, 3, 1).reshape(B * H * W, 4 * C).contiguous()


def _shuffle_case(ops, dev, B, H, W, C, dt):
    Ms, Ml = B * H * W, B * 4 * H * W
    x = _distinct(Ms * 4 * C, dt).view(Ms, 4 * C).to(dev)
    y = torch.full((Ml + 1, C), SENT, dtype=dt, device=dev)
    ops.pixel_shuffle2(x, y[:Ml], B, H, W, C)
    assert _bits_equal(y[:Ml], _shuffle_ref(x, B, H, W, C)), "forward differs from F.pixel_shuffle"
    assert bool((y[Ml] == SENT).all())
    back = torch.full((Ms + 1, 4 * C), SENT, dtype=dt, device=dev)
    ops.pixel_shuffle2(y[:Ml], back[:Ms], B, H, W, C, inverse=True)
    assert _bits_equal(back[:Ms], x), "inverse(forward(x)) != x"
    assert bool((back[Ms] == SENT).all())
    # the inverse on its own input (not a forward output): values in the order of the LARGE grid
    z = _distinct(Ml * C, dt).view(Ml, C).to(dev)
    back.fill_(SENT)
    ops.pixel_shuffle2(z, back[:Ms], B, H, W, C, inverse=True)
    assert _bits_equal(back[:Ms], _unshuffle_ref(z, B, H, W, C)), "inverse differs from F.pixel_unshuffle"
    assert bool((back[Ms] == SENT).all())


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 5), (3, 7, 6), (1, 16, 16)])
@pytest.mark.parametrize("dt,C", [pytest.param(BF16, c, id=f"bf16-C{c}") for c in (8, 64, 72)]
                         + [pytest.param(F32, c, id=f"f32-C{c}") for c in (4, 20, 64)])
def test_pixel_shuffle2(ops, dev, B, H, W, C, dt):
    """sodt_pixel_shuffle2 both ways, bit for bit against F.pixel_shuffle / F.pixel_unshuffle on the NCHW view, on values that are
    distinct per element.  Catches the sub-pixel order (2i + j against 2j + i; the non-square grids also catch y <-> x), the channel
    interleave 4c + s of one 16-byte chunk (C = 72 / 20: chunks per pixel no power of two), and B > 1 (the image stride)."""
    _shuffle_case(ops, dev, B, H, W, C, dt)


def test_pixel_shuffle2_grid_stride(ops, dev):
    """256 * 260 * 4 * 64 / 8 = 2.13 M chunks > 8192 * 256: a second grid-stride pass, both directions."""
    B, H, W, C = 1, 256, 260, 64
    assert B * H * W * 4 * C // 8 > 8192 * 256
    _shuffle_case(ops, dev, B, H, W, C, BF16)


# ------------------------------------------------------------------------------------------------ add_rows
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", ["full", "slice"])
def test_add_rows(ops, dev, form, dt):
    """dst[:, dcol : dcol + C] += src[:, scol : scol + C], bit for bit: f32 as torch's f32 add (the exact sum rounded once), bf16 as
    (dst.float() + src.float()).bfloat16().  "slice": ldd, dcol, lds, scol all non-trivial and different; the columns of dst outside
    the slice keep their sentinel, those of src hold NaN (reading them poisons the sum).  Catches slice addressing (a leading dimension or column offset of one side used for the other)."""
    M, C = 37, 24
    ldd, dcol, lds, scol = (C, 0, C, 0) if form == "full" else (C + 16, 8, C + 24, 16)
    g = _gen(17)
    d0, s0 = torch.randn(M, C, generator=g).to(dt), torch.randn(M, C, generator=g).to(dt)
    dst = torch.full((M + 1, ldd), SENT, dtype=dt)
    dst[:M, dcol: dcol + C] = d0
    src = torch.full((M, lds), float("nan"), dtype=dt)
    src[:, scol: scol + C] = s0
    dst = dst.to(dev)
    ops.add_rows(dst[:M], src.to(dev), M, C, ldd=ldd, dcol=dcol, lds=lds, scol=scol)
    dst = dst.cpu()
    ref = (d0.float() + s0.float()).to(dt)          # the f32 sum is the correctly rounded exact sum; bf16 rounds that once more
    assert _bits_equal(dst[:M, dcol: dcol + C].contiguous(), ref)
    outside = torch.ones(ldd, dtype=torch.bool)
    outside[dcol: dcol + C] = False
    assert bool((dst[:M, outside] == SENT).all()) and bool((dst[M] == SENT).all()), "wrote outside the slice"


@pytest.mark.parametrize("C", [1, 3, 63])
def test_add_rows_short_f32_row(ops, dev, C):
    """The one-row f32 path below the 16-byte granule (the bias gradient of a 3-channel convolution), with column offsets that are
    no multiple of 4: exactly C elements change."""
    dcol, scol, n = 5, 2, 80
    g = _gen(C)
    d0, s0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dst, src = d0.clone().to(dev), s0.to(dev)
    ops.add_rows(dst.view(1, n), src.view(1, n), 1, C, dcol=dcol, scol=scol)
    ref = d0.clone()
    ref[dcol: dcol + C] = d0[dcol: dcol + C] + s0[scol: scol + C]
    assert _bits_equal(dst, ref)


def test_add_rows_grid_stride(ops, dev):
    """40000 x 512 bf16 = 2.56 M chunks > 8192 * 256."""
    M, C = 40000, 512
    assert M * C // 8 > 8192 * 256
    g = _gen(19)
    d0, s0 = torch.randn(M, C, generator=g).bfloat16().to(dev), torch.randn(M, C, generator=g).bfloat16().to(dev)
    dst = torch.full((M + 1, C), SENT, dtype=BF16, device=dev)
    dst[:M] = d0
    ops.add_rows(dst[:M], s0, M, C)
    assert _bits_equal(dst[:M], (d0.float() + s0.float()).bfloat16())
    assert bool((dst[M] == SENT).all())


def test_add_rows_refusals(ops, dev):
    """What the 16-byte kernels cannot do is refused (RuntimeError from ops, nothing launched) - never done approximately."""
    def buf(n):
        return torch.zeros(n, device=dev)
    with pytest.raises(RuntimeError):                      # one f32 row just past the short path, not a multiple of 4
        ops.add_rows(buf(128).view(1, 128), buf(128).view(1, 128), 1, 65)
    with pytest.raises(RuntimeError):                      # the short path is for ONE row
        ops.add_rows(buf(16).view(2, 8), buf(16).view(2, 8), 2, 3)
    off = buf(64 + 4)[1: 65].view(8, 8)                    # a view offset by one element: 4-byte aligned only
    with pytest.raises(RuntimeError):
        ops.add_rows(off, buf(64).view(8, 8), 8, 8)
    with pytest.raises(RuntimeError):
        ops.add_rows(buf(64).view(8, 8), off, 8, 8)
    with pytest.raises(RuntimeError):                      # dcol not a multiple of the granule (4 f32 / 8 bf16)
        ops.add_rows(buf(128).view(8, 16), buf(64).view(8, 8), 8, 8, dcol=2)
    with pytest.raises(RuntimeError):
        ops.add_rows(buf(128).bfloat16().view(8, 16), buf(64).bfloat16().view(8, 8), 8, 8, dcol=4)
    ok = torch.full((8, 16), 1.0, device=dev)               # the same call with an aligned offset is accepted
    ops.add_rows(ok, torch.full((8, 8), 2.0, device=dev), 8, 8, dcol=8)
    assert bool((ok[:, 8:] == 3.0).all()) and bool((ok[:, :8] == 1.0).all())


# ------------------------------------------------------------------------------------------------ NCHW f32 <-> rows
def _convert_case(ops, dev, B, C, H, W, ld, dt, seed):
    M = B * H * W
    y = _values(B * C * H * W, seed).view(B, C, H, W)
    rows = torch.full((M + 1, ld), SENT, dtype=dt, device=dev)
    ops.rows_from_nchw_f32(y.to(dev), rows[:M], B, C, H, W)
    rows = rows.cpu()
    ref = y.permute(0, 2, 3, 1).reshape(M, C).to(dt)                 # torch: round to nearest even, NaN kept
    assert _bits_equal(rows[:M, :C].contiguous(), ref), "rows differ from the permuted tensor"
    assert bool((rows[:M, C:].contiguous().view(IVIEW[dt]) == 0).all()), "pad columns are not +0"
    assert bool((rows[M] == SENT).all()), "wrote past the last row"
    # back: pad columns hold NaN and must be ignored
    src = torch.full((M, ld), float("nan"), dtype=dt)
    src[:, :C] = ref
    out = torch.full((B * C * H * W + 1,), SENT, device=dev)
    ops.nchw_f32_from_rows(src.to(dev), out[:-1].view(B, C, H, W), B, C, H, W)
    out = out.cpu()
    assert _bits_equal(out[:-1].view(B, C, H, W), ref.float().view(B, H, W, C).permute(0, 3, 1, 2).contiguous())
    assert float(out[-1]) == SENT
    if dt == F32:                                                     # f32 -> rows(f32) -> f32 is the identity
        assert _bits_equal(out[:-1].view(B, C, H, W), y)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,ld", [(c, ld) for c in (3, 4, 13, 64) for ld in sorted({c, 8, 16, 72}) if ld >= c])
def test_rows_from_nchw_and_back(ops, dev, C, ld, dt):
    """sodt_rows_from_nchw_f32 / sodt_nchw_f32_from_rows - the helpers every SR test trusts - bit for bit against permute (f32) and
    .bfloat16() of the permuted tensor (bf16), for B in {1, 3} and 1 x 1, 5 x 7, 16 x 12 grids.  Catches the rounding mode (ties,
    overflow to inf, NaN), pad overwrite (pad columns are written +0 going to rows and ignored coming back) and H <-> W / C <-> ld
    mix-ups (C odd, ld > C, non-square grids)."""
    for B in (1, 3):
        for H, W in ((1, 1), (5, 7), (16, 12)):
            _convert_case(ops, dev, B, C, H, W, ld, dt, 1000 * C + 10 * H + B)


@pytest.mark.parametrize("dt", DTS)
def test_rows_from_nchw_grid_stride(ops, dev, dt):
    """3 x 64 x 128 x 96 = 2.36 M elements (2.65 M with ld = 72) > 2^21 = 8192 * 256: both converters stride their grid."""
    B, C, H, W, ld = 3, 64, 128, 96, 72
    assert B * C * H * W > 1 << 21
    _convert_case(ops, dev, B, C, H, W, ld, dt, 5)


def test_converter_refusals(ops, dev):
    """C > ld would write past each row"""
    y = torch.zeros(1, 13, 2, 2, device=dev)
    rows = torch.zeros(4, 8, device=dev)
    with pytest.raises(RuntimeError):
        ops.rows_from_nchw_f32(y, rows, 1, 13, 2, 2)
    with pytest.raises(RuntimeError):
        ops.nchw_f32_from_rows(rows, y, 1, 13, 2, 2)
