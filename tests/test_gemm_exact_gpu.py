"""Every GEMM kernel route, bit for bit.

The operands are small integers, so every product and partial sum a kernel forms is exact in f32 (tests/gemm_cases.py) and
the expected output is a pure function of the inputs: f64 reference -> f32 (exact) -> one round-to-nearest-even store.  Each
case asserts `torch.equal` on the raw bits, that nothing outside the output view was written (sentinel bit pattern), that no
NaN planted around the operand views reached a stored element, and - through the profiler - which kernel instantiation
served the call.  The activation epilogues are checked on exact arguments against the error bounds csrc/common.h documents.
Random-data cases stay in tests/test_kernels_gpu.py."""
import math

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
E = dict(BIAS=1, RESID=2, GELU_DUAL=4, DGELU=8, STATS=16, AFFINE_SILU=32, DETECT=64, OUT_F32=128, GELU=256, DGELU_RC=512,
         RELU=2048, DRELU=4096)
EXACT_FLAGS = {"0": 0, "BIAS": 1, "RESID": 2, "BIAS|RESID": 3, "RELU": 2048, "BIAS|RELU": 2049, "DRELU": 4096}
TAPS3 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
TAPS2 = [(0, 0), (1, 0), (0, 1), (1, 1)]

# Every kernel instantiation some case below asserts.  Each parametrize table goes through routed(), which records route(*row)
# for every row, and the case asserts that same route(*row): deleting a case or changing what it is written for changes this set
# with it.  test_engine_gemm_routes_are_covered compares the model's GEMM launches against it.
COVERED = set()


def routed(table, route):
    for row in table:
        COVERED.update(route(*(row if isinstance(row, tuple) else (row,))))
    return table


def _r8(n):
    return (n + 7) // 8 * 8


@pytest.fixture
def variant(ops):
    """Set the NT / TN route hook for one case; always back to automatic afterwards."""
    yield ops.gemm_set_variant
    ops.gemm_set_variant(0)
    ops.set_tn_scratch(None)


# ------------------------------------------------------------------ the NT harness
def make_a(dev, dt, M, K, *, lim=4, seed=1, coff=8, extra_cols=8, nseg=1, klens=None):
    """A as nseg segments, each a NaN-poisoned view [M][klen] at column coff of a wider [M + 3][ld] buffer (ld > coff + klen)."""
    klens = klens or [K // nseg] * nseg
    assert sum(klens) == K
    segs = []
    for i, kl in enumerate(klens):
        c0 = coff + 8 * (i % 3)
        buf, _ = G.poisoned(G.ints((M, kl), lim, seed + 17 * i, dev), dt, ld=c0 + kl + extra_cols + 8 * (i % 2), col0=c0)
        segs.append(dict(buf=buf, klen=kl, coff=c0))
    return segs


def make_w(dev, dt, N, K, *, lim=4, seed=2, row0=0, extra_cols=16):
    """W [N][K] inside a NaN buffer: rows before row0 (reached through w_off) and after N, columns after K (ldw > K)."""
    buf, view = G.poisoned(G.ints((N, K), lim, seed, dev), dt, ld=K + extra_cols, row0=row0)
    return buf, view


def nt_call(ops, segs, wbuf, out, M, N, K, *, w_row0=0, ldc=None, c_off=0, spatial=None, **kw):
    ops.gemm_nt(G.segspecs(ops, segs), wbuf, out, M, N, K, ldw=wbuf.shape[1], w_off=w_row0 * wbuf.shape[1], ldc=ldc, c_off=c_off,
                spatial=spatial, **kw)


def epilogue64(v, cf, bias=None, resid=None, aux=None):
    """epi_chunk's order (csrc/gemm_epi.h): bias, relu, drelu, resid - exact in f64 for the integer data here.  With integer data
    every order of the f32 adds gives the same bits, so these cases pin the single rounding at the store, not the order of the adds
    (gemm_nt3_kernel adds a residual before the bias)."""
    if cf & E["BIAS"]:
        v = v + bias.double()
    if cf & E["RELU"]:
        v = v.clamp(min=0)
    if cf & E["DRELU"]:
        v = torch.where(aux.double() > 0, v, torch.zeros_like(v))
    if cf & E["RESID"]:
        v = v + resid.double()
    return v


def run_nt_exact(ops, dev, dt, M, N, K, cf, expect, *, nseg=1, klens=None, resid_alias=False, ldc_pad=24, c_off=8, w_row0=3,
                 segs=None, spatial=None, lim=4, seed=0):
    """One exact NT case: flags cf from EXACT_FLAGS (+ STATS-free), output a [M][N] view at column c_off of an [M + 5][ldc]
    sentinel buffer, optionally aliased with the residual (the engine's resid=out form)."""
    segs = segs or make_a(dev, dt, M, K, nseg=nseg, klens=klens, seed=seed + 1, lim=lim)
    wbuf, wv = make_w(dev, dt, N, K, row0=w_row0, seed=seed + 2, lim=lim)
    ldc = c_off + N + ldc_pad + (-N) % 8          # (ldc stays a multiple of 16 bytes for any N)
    out = G.sentinel_buffer(M + 5, ldc, dt, dev)
    kw = {}
    bias = resid = aux = None
    if cf & E["BIAS"]:
        bias = G.ints((N,), 1000, seed + 3, dev)              # f32 integers that bf16 cannot hold: a bias rounded first fails
        kw["bias"] = bias
    if cf & E["RESID"]:
        resid = G.ints((M, N), 256, seed + 4, dev)            # |r| <= 256: exact in bf16
        if resid_alias:
            out[:M, c_off:c_off + N] = resid.to(dt)
            kw.update(resid=out, ldr=ldc, r_off=c_off)
        else:
            rbuf, _ = G.poisoned(resid, dt, ld=_r8(N) + 16, col0=8)
            kw.update(resid=rbuf, ldr=rbuf.shape[1], r_off=8)
    if cf & E["DRELU"]:
        aux = G.ints((M, N), 3, seed + 5, dev)
        abuf, _ = G.poisoned(aux, dt, ld=_r8(N) + 8, col0=0)
        kw.update(drelu_aux=abuf)
    if cf & E["RELU"]:
        kw["relu"] = True
    G.run_expecting(lambda: nt_call(ops, segs, wbuf, out, M, N, K, w_row0=w_row0, ldc=ldc, c_off=c_off, spatial=spatial, **kw),
                    expect)
    a64 = G.gather_a(segs, M, spatial)
    ref = G.rne(epilogue64(a64 @ wv.double().t(), cf, bias, resid, aux), dt)
    G.assert_bits(out[:M, c_off:c_off + N], ref, f"{expect} M={M} N={N} K={K}")
    G.assert_sentinel_outside(out, slice(0, M), slice(c_off, c_off + N), f"{expect} M={M} N={N} K={K}")


# ------------------------------------------------------------------ §2 gemm_nt3_kernel, NV = 3: the exact flag sets
NT3_SHAPES = [(256, 192, 192, 1), (257, 384, 640, 2), (511, 200, 512, 1), (300, 776, 576, 3)]   # segments: whole 64-column K-steps


def _nt3_flag_route(M, N, K, nseg, flag):
    return [G.nt3(EXACT_FLAGS[flag])]


@pytest.mark.parametrize("M,N,K,nseg,flag", routed([s + (f,) for s in NT3_SHAPES for f in EXACT_FLAGS], _nt3_flag_route))
def test_nt3_exact_flags(ops, dev, variant, M, N, K, nseg, flag):
    variant(0)
    if N % 192 and K < 512:
        pytest.fail("shape table error: a partial column tile needs K >= 512")
    run_nt_exact(ops, dev, BF, M, N, K, EXACT_FLAGS[flag], _nt3_flag_route(M, N, K, nseg, flag), nseg=nseg, resid_alias=(M == 257))


def _nt3_shape_route(M, N, K, cf, klens):
    return [G.nt3(cf)]


@pytest.mark.parametrize("M,N,K,cf,klens", routed([
    (257 * 256, 192, 192, 0, None),                          # 257 tiles on a 256-workgroup grid: a partial last persistent round
    (256, 1152, 192, 1, None),
    (256, 3072, 192, 1, None),                               # T3_MAXBIAS
    (256, 192, 3968, 2, None),                               # one segment of exactly T3_MAXKLEN
    (300, 192, 4096, 3, [3968, 128]),                        # K above it, split across segments
    (384, 384, 832, 1, [64, 128, 64, 192, 64, 64, 128, 64, 64]),   # SODT_MAX_SEG segments, different ld / coff
], _nt3_shape_route))
def test_nt3_shapes(ops, dev, variant, M, N, K, cf, klens):
    variant(0)
    lim = 4 if K <= 1024 else 2           # |a|, |w| <= 2 at K <= 4096: |sum| <= 2^14
    run_nt_exact(ops, dev, BF, M, N, K, cf, _nt3_shape_route(M, N, K, cf, klens), klens=klens, lim=lim)


def _spatial_segs(dev, dt, B, H, W, C, taps, *, mul=1, shr=0, Hi=None, Wi=None, seed=7, same=True):
    Hi, Wi = Hi or H, Wi or W
    rows = B * Hi * Wi
    if same:
        buf, _ = G.poisoned(G.ints((rows, C), 4, seed, dev), dt, ld=C + 16, col0=8)
        return [dict(buf=buf, klen=C, coff=8, dy=dy, dx=dx, mul=mul, shr=shr, Hi=Hi, Wi=Wi) for (dy, dx) in taps]
    out = []
    for i, (dy, dx) in enumerate(taps):
        buf, _ = G.poisoned(G.ints((rows, C), 4, seed + i, dev), dt, ld=C + 8 * (1 + i % 3), col0=8 * (i % 2))
        out.append(dict(buf=buf, klen=C, coff=8 * (i % 2), dy=dy, dx=dx, mul=mul, shr=shr, Hi=Hi, Wi=Wi))
    return out


def _taps_route(B, H, W, C, N, cf):
    return [G.nt3(cf)]


@pytest.mark.parametrize("B,H,W,C,N,cf", routed([(2, 12, 16, 64, 192, 1), (2, 1, 160, 64, 192, 3), (1, 300, 1, 64, 192, 0),
                                                (1, 16, 32, 64, 200, 2049)], _taps_route))
def test_nt3_conv3x3_taps_fast(ops, dev, variant, B, H, W, C, N, cf):
    """3x3 taps of one tensor on the output grid (taps_fast), including H = 1 / W = 1 images where taps leave the grid."""
    variant(0)
    segs = _spatial_segs(dev, BF, B, H, W, C, TAPS3)
    run_nt_exact(ops, dev, BF, B * H * W, N, 9 * C, cf, _taps_route(B, H, W, C, N, cf), segs=segs, spatial=(H, W))


GENERIC_SEG_ROUTE = [G.nt3(3)]
COVERED.update(GENERIC_SEG_ROUTE)


def test_nt3_generic_segment_table(ops, dev, variant):
    """Mixed tensors: a PatchMerging gather (mul = 2) of one tensor, an upsample (shr = 1) of another and negative taps of a
    third - the generic segment-table path of gemm_nt3_kernel."""
    variant(0)
    B, H, W = 2, 12, 16
    segs = _spatial_segs(dev, BF, B, H, W, 64, TAPS2, mul=2, Hi=2 * H, Wi=2 * W, same=False)
    segs += _spatial_segs(dev, BF, B, H, W, 128, [(0, 0)], shr=1, Hi=H // 2, Wi=W // 2, seed=30)
    segs += _spatial_segs(dev, BF, B, H, W, 64, [(-1, -1), (-1, 1), (1, -1)], seed=40, same=False)
    K = sum(s["klen"] for s in segs)
    run_nt_exact(ops, dev, BF, B * H * W, 384, K, 3, GENERIC_SEG_ROUTE, segs=segs, spatial=(H, W))


MERGE = [  # (Cc, H, W, dtype, route hook, the kernel the size selects)
    (192, 32, 32, BF, 0, G.nt3(0, True)),                 # pipelined sizes
    (64, 8, 12, BF, 0, G.bs(BF, False, -1, False)),       # short K: the generic weight-stationary kernel
    (64, 8, 12, BF, 1, G.ntk(BF, -1)),                    # the K-loop kernel
    (192, 32, 32, F32, 0, G.ntk(F32, -1)),
    (32, 8, 12, F32, 0, G.bs(F32, False, -1, False)),
]


def _merge_route(Cc, H, W, dt, hook, kernel):
    return [kernel] * 4


@pytest.mark.parametrize("Cc,H,W,dt,hook,kernel", routed(MERGE, _merge_route),
                         ids=[f"{r[0]}-{r[1]}x{r[2]}-{'bf16' if r[3] == BF else 'f32'}-v{r[4]}" for r in MERGE])
def test_nt_patch_merge_scatter(ops, dev, variant, Cc, H, W, dt, hook, kernel):
    """PatchMerging backward: four GEMMs whose output rows scatter to the stride-2 positions of the full grid (oscatter), on the
    pipelined kernel (gemm_nt3_kernel<0, true, 3>), the generic weight-stationary kernel and the K-loop kernel."""
    variant(hook)
    B = 2
    M2 = B * (H // 2) * (W // 2)
    dz_buf, dz = G.poisoned(G.ints((M2, 2 * Cc), 4, 3, dev), dt, ld=2 * Cc + 16, col0=8)
    WrT_buf, WrT = G.poisoned(G.ints((4 * Cc, 2 * Cc), 4, 4, dev), dt, ld=2 * Cc + 8)
    out = G.sentinel_buffer(B * H * W + 4, Cc + 16, dt, dev)
    expect = kernel

    def run():
        for tap, (dy, dxx) in enumerate(TAPS2):
            ops.gemm_nt([ops.SegSpec(dz_buf, 2 * Cc, 8, 0, 0, 1, 0, H // 2, W // 2)], WrT_buf, out, M2, Cc, 2 * Cc,
                        ldw=WrT_buf.shape[1], w_off=tap * Cc * WrT_buf.shape[1], ldc=Cc + 16, c_off=8, spatial=(H // 2, W // 2),
                        oscatter=(2, dy, dxx, H, W))
    G.run_expecting(run, _merge_route(Cc, H, W, dt, hook, kernel))
    full = dz.double() @ WrT.double().t()                 # [M2][4C]
    f4 = full.view(B, H // 2, W // 2, 4, Cc)
    ref = torch.zeros(B, H, W, Cc, device=dev, dtype=torch.float64)
    for tap, (dy, dxx) in enumerate(TAPS2):
        ref[:, dy::2, dxx::2] = f4[..., tap, :]
    G.assert_bits(out[:B * H * W, 8:8 + Cc], G.rne(ref.view(-1, Cc), dt), f"patch merge scatter {expect}")
    G.assert_sentinel_outside(out, slice(0, B * H * W), slice(8, 8 + Cc), "patch merge scatter")


# ------------------------------------------------------------------ §2 NV = 2 (thin outputs)
THIN = {"0": 0, "BIAS": 1, "BIAS|RESID": 3, "RESID": 2, "BIAS|RELU": 2049, "DRELU": 4096}


def _thin_route(N, flag):
    return [G.nt3(THIN[flag], nv=2)]


@pytest.mark.parametrize("N,flag", routed([(n, f) for n in (8, 32, 40, 64) for f in THIN], _thin_route))
def test_nt3_thin_flags(ops, dev, variant, N, flag):
    variant(0)
    run_nt_exact(ops, dev, BF, 300, N, 512, THIN[flag], _thin_route(N, flag), resid_alias=(N == 40))


def _stats_case(ops, dev, M, N, K, A, W, expect):
    stats = torch.zeros(16, 2, N, device=dev, dtype=torch.float64)
    out = G.sentinel_buffer(M + 3, N + 8, BF, dev)
    G.run_expecting(lambda: ops.gemm_nt([ops.SegSpec(A)], W, out, M, N, K, ldc=N + 8, stats=stats), [expect])
    v = A.double() @ W.double().t()
    return out, stats.sum(0), v


STATS_ROUTE = G.nt3(16, nv=2)
COVERED.add(STATS_ROUTE)


@pytest.mark.parametrize("N,K", routed([(8, 192), (32, 192), (40, 192), (64, 448)], lambda N, K: [STATS_ROUTE]))
def test_nt3_thin_stats_exact(ops, dev, variant, N, K):
    """SODT_EPI_STATS: |a|, |w| <= 1 and K <= 448 give |v| <= 448; a lane's f32 partial of v^2 covers at most 4 rows per tile
    and one tile per workgroup here (17 tiles), then 16 lanes are summed in f32: <= 64 * 448^2 < 2^24 - exact, so the f64
    column sums are bit-exact."""
    variant(0)
    M = 4096 + 37
    A = G.ints((M, K), 1, 11, dev, BF)
    W = G.ints((N, K), 1, 12, dev, BF)
    out, st, v = _stats_case(ops, dev, M, N, K, A, W, STATS_ROUTE)
    G.assert_bits(out[:M, :N], G.rne(v, BF), "stats output")
    G.assert_sentinel_outside(out, slice(0, M), slice(0, N), "stats output")
    assert torch.equal(st[0], v.sum(0)) and torch.equal(st[1], (v * v).sum(0)), "column statistics are not exact"


def test_nt3_thin_stats_large_offset(ops, dev, variant):
    """M > 10^6 rows, mean ~ 30 std: the variance bn_finalize derives from the statistics matches f64 to 1e-4 relative."""
    variant(0)
    M, N, K = 1_000_003, 64, 192
    g = torch.Generator(device="cpu").manual_seed(5)
    A = torch.randn(M, K, generator=g).to(dev).to(BF)
    A[:, 0] = 30.0
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev).to(BF)
    W[:, 0] = 1.0
    out, st, v = _stats_case(ops, dev, M, N, K, A, W, STATS_ROUTE)
    mean = st[0] / M
    var = st[1] / M - mean * mean
    rvar = v.var(0, unbiased=False)
    assert float((v.mean(0) / v.std(0)).abs().min()) > 20
    rel = float(((var - rvar).abs() / rvar).max())
    assert rel <= 1e-4, f"variance from the statistics: rel err {rel:.2e}"


# ------------------------------------------------------------------ §2 GELU family on exact data (data movement exact, activation bounded)
def _gelu_family_route(route, flag):
    cf = sum(E[f] for f in flag.split("|"))
    if route == "nt3":
        return [G.nt3(cf)]
    if route == "bs":
        return [G.bs(BF, False, cf, True) if cf != E["BIAS"] | E["GELU"] else G.bs(BF, False, -1, False)]
    return [G.ntk(BF, cf) if cf != E["BIAS"] | E["GELU"] else G.ntk(BF, -1)]


@pytest.mark.parametrize("route,flag", routed([(r, f) for r in ("nt3", "bs", "nt") for f in ("BIAS|GELU_DUAL", "BIAS|GELU", "DGELU")],
                                              _gelu_family_route))
def test_gelu_family_exact_data(ops, dev, variant, route, flag):
    """Integer A / W / bias: the pre-activation is exact, so GELU_DUAL's C must be bit-exact and every activation output within the
    documented bound of f at that exact argument."""
    cf = sum(E[f] for f in flag.split("|"))
    dt = BF
    variant(1 if route == "nt" else 0)
    M, N, K = (300, 384, 576) if route == "nt3" else (300, 136, 192)
    segs = make_a(dev, dt, M, K, lim=2)
    wbuf, wv = make_w(dev, dt, N, K, lim=1, row0=2)
    v = G.gather_a(segs, M, None) @ wv.double().t()
    out = G.sentinel_buffer(M + 3, N + 16, dt, dev)
    kw = {}
    if cf & E["BIAS"]:
        bias = G.ints((N,), 6, 3, dev)
        kw["bias"] = bias
        v = v + bias.double()
    if flag == "BIAS|GELU_DUAL":
        c2 = G.sentinel_buffer(M + 3, N, dt, dev)
        kw["gelu_out"] = c2
    elif flag == "BIAS|GELU":
        kw["gelu_only"] = True
    else:
        vals = torch.tensor([-1.5, -0.5, 0.0, 0.5, 1.0, 3.0], device=dev)       # gelu' pairwise >= 0.07 apart: a misread aux shows
        g = torch.Generator(device="cpu").manual_seed(9)
        x = vals[torch.randint(0, 6, (M, N), generator=g).to(dev)]
        abuf, _ = G.poisoned(x, dt, ld=N + 8)
        kw["dgelu_aux"] = abuf
    G.run_expecting(lambda: nt_call(ops, segs, wbuf, out, M, N, K, w_row0=2, ldc=N + 16, **kw), _gelu_family_route(route, flag))
    got = out[:M, :N]
    G.assert_sentinel_outside(out, slice(0, M), slice(0, N), flag)
    if flag == "BIAS|GELU_DUAL":
        G.assert_bits(got, G.rne(v, dt), "GELU_DUAL pre-activation")
        G.assert_within(c2[:M], G.gelu64(v), G.act_bound("gelu", dt, v), "GELU_DUAL activation")
        G.assert_sentinel_outside(c2, slice(0, M), slice(0, N), "GELU_DUAL C2")
    elif flag == "BIAS|GELU":
        G.assert_within(got, G.gelu64(v), G.act_bound("gelu", dt, v), "GELU")
    else:
        # v * gelu'(x): |v| times the gelu' error, plus the f32 product and the store
        want = v * G.dgelu64(x.double())
        e = v.abs() * (G.DGELU_BF16 + 2.0 ** -24 * G.dgelu64(x.double()).abs())
        G.assert_within(got, want, e + G.U_OUT[dt] * (want.abs() + e) + G.FTZ, "DGELU")


RC_ROUTE = [G.nt3(E["BIAS"] | E["DGELU_RC"])]
COVERED.update(RC_ROUTE)


def test_nt3_dgelu_recompute(ops, dev, variant):
    """SODT_EPI_DGELU_RC on integer xn, W1, b1 (h exact) and dy, W2 (dy W2 exact): dh = (dy W2) gelu'(h).  The kernel parks
    gelu'(h) as bf16 between the two K halves (csrc/gemm3.hip), one extra bf16 rounding (2^-8 relative) in the bound."""
    variant(0)
    M, Cc = 300, 192
    xn = G.ints((M, Cc), 1, 1, dev, BF)
    dy = G.ints((M, Cc), 2, 2, dev, BF)
    W1 = G.ints((4 * Cc, Cc), 1, 3, dev, BF)
    W2 = G.ints((Cc, 4 * Cc), 2, 4, dev, BF)
    b1 = G.ints((4 * Cc,), 3, 5, dev)
    Wcat = torch.cat([W1, W2.t()], 1).contiguous()
    out = G.sentinel_buffer(M + 3, 4 * Cc + 8, BF, dev)
    G.run_expecting(lambda: ops.gemm_nt([ops.SegSpec(xn), ops.SegSpec(dy)], Wcat, out, M, 4 * Cc, 2 * Cc, ldc=4 * Cc + 8, bias=b1,
                                        dgelu_rc=True), RC_ROUTE)
    h = xn.double() @ W1.double().t() + b1.double()
    d = dy.double() @ W2.double()
    gp = G.dgelu64(h)
    want = d * gp
    eg = G.DGELU_BF16 + G.U_OUT[BF] * (gp.abs() + G.DGELU_BF16)          # gelu'(h), then its bf16 parking
    e = d.abs() * eg
    G.assert_within(out[:M, :4 * Cc], want, e + G.U_OUT[BF] * (want.abs() + e) + G.FTZ, "DGELU_RC")
    G.assert_sentinel_outside(out, slice(0, M), slice(0, 4 * Cc), "DGELU_RC")


# ------------------------------------------------------------------ §2 the gemm.hip kernels, both dtypes
BS_SIMPLE = {"0": 0, "BIAS": 1, "RESID": 2, "BIAS|RESID": 3}
SHORT_K = {BF: 192, F32: 96}          # K * sizeof(T) = 384 bytes: the weight- / A-stationary kernels


def _dts(flags):
    return [(dt, f) for dt in (BF, F32) for f in flags]


def _ids(rows):
    return [f"{'bf16' if r[0] == BF else 'f32'}-{'-'.join(str(x) for x in r[1:])}" for r in rows]


def _bs_simple_route(dt, flag):
    return [G.bs(dt, False, BS_SIMPLE[flag], True)]


@pytest.mark.parametrize("dt,flag", routed(_dts(BS_SIMPLE), _bs_simple_route), ids=_ids(_dts(BS_SIMPLE)))
def test_bs_simple(ops, dev, variant, dt, flag):
    variant(0)
    cf = BS_SIMPLE[flag]
    run_nt_exact(ops, dev, dt, 300, 136, SHORT_K[dt], cf, _bs_simple_route(dt, flag), resid_alias=(cf == 3), w_row0=0 if dt == F32 else 3)


BS_GENERIC = _dts(["RELU", "BIAS|RELU", "DRELU", "0-segments"])


def _bs_generic_route(dt, flag):
    return [G.bs(dt, False, -1, False)]


@pytest.mark.parametrize("dt,flag", routed(BS_GENERIC, _bs_generic_route), ids=_ids(BS_GENERIC))
def test_bs_generic(ops, dev, variant, dt, flag):
    variant(0)
    if flag == "0-segments":
        cf, nseg = 0, 2
    else:
        cf, nseg = EXACT_FLAGS[flag], 1
    run_nt_exact(ops, dev, dt, 300, 136, SHORT_K[dt], cf, _bs_generic_route(dt, flag), nseg=nseg)


def _as_route(dt, flag):
    return [G.as_(dt)]


@pytest.mark.parametrize("dt,flag", routed(_dts(EXACT_FLAGS), _as_route), ids=_ids(_dts(EXACT_FLAGS)))
def test_as_kernel(ops, dev, variant, dt, flag):
    variant(2)
    cf = EXACT_FLAGS[flag]
    run_nt_exact(ops, dev, dt, 300, 136, SHORT_K[dt], cf, _as_route(dt, flag), nseg=2, resid_alias=(cf == 2))


NT_CASES = {"0": 0, "BIAS": 1, "RESID": 2, "BIAS|RESID": 3}


def _ntk_route(dt, flag):
    return [G.ntk(dt, EXACT_FLAGS[flag] if flag in NT_CASES else -1)]


@pytest.mark.parametrize("dt,flag", routed(_dts(EXACT_FLAGS), _ntk_route), ids=_ids(_dts(EXACT_FLAGS)))
def test_nt_kernel(ops, dev, variant, dt, flag):
    variant(1)
    cf = EXACT_FLAGS[flag]
    run_nt_exact(ops, dev, dt, 300, 200, 3 * SHORT_K[dt], cf, _ntk_route(dt, flag), nseg=3, resid_alias=(cf == 3))


TAIL = [(route, N, flag) for route in ("as", "nt") for N in (131, 77) for flag in ("0", "BIAS|RESID", "BIAS|RELU", "DRELU")]


def _tail_route(route, N, flag):
    return _as_route(BF, flag) if route == "as" else _ntk_route(BF, flag)


@pytest.mark.parametrize("route,N,flag", routed(TAIL, _tail_route))
def test_bf16_output_column_tail(ops, dev, variant, route, N, flag):
    """bf16 output with N % 8 != 0: the per-element store path of epi_chunk (the last chunk of a row is partial), on the two kernels
    that accept such widths (the A-stationary one at short K, the K-loop one)."""
    variant(2 if route == "as" else 1)
    cf = EXACT_FLAGS[flag]
    K = SHORT_K[BF] if route == "as" else 3 * SHORT_K[BF]
    run_nt_exact(ops, dev, BF, 300, N, K, cf, _tail_route(route, N, flag), nseg=1 if route == "as" else 3, resid_alias=(cf == 3))


def _drelu_resid_route(dt):
    return [G.as_(dt), G.ntk(dt, -1)]


@pytest.mark.parametrize("dt", routed([BF, F32], _drelu_resid_route), ids=["bf16", "f32"])
def test_engine_drelu_resid_route(ops, dev, variant, dt):
    """drelu_aux with resid (sr.py's dgrad of a ReLU conv into an accumulated input gradient): the A-stationary kernel at short K,
    the K-loop kernel otherwise - the weight-stationary one refuses the pair (it adds the residual first)."""
    variant(0)
    cf = E["DRELU"] | E["RESID"]
    short, long_ = _drelu_resid_route(dt)
    run_nt_exact(ops, dev, dt, 300, 64, SHORT_K[dt], cf, [short], resid_alias=True)
    run_nt_exact(ops, dev, dt, 300, 64, 2 * SHORT_K[dt] + 64, cf, [long_], resid_alias=True)


def _runtime_flags_route(dt, route):
    """STATS, RESID with rmod, OUT_F32, DETECT - in the order the case calls them."""
    if route == "bs":
        return [G.bs(dt, True, -1, False), G.bs(dt, False, 2, True), G.as_(dt), G.ntk(dt, -1)]
    return [G.ntk(dt, -1), G.ntk(dt, 2), G.ntk(dt, -1), G.ntk(dt, -1)]


@pytest.mark.parametrize("dt,route", routed(_dts(["bs", "nt"]), _runtime_flags_route), ids=_ids(_dts(["bs", "nt"])))
def test_stats_rmod_outf32_detect(ops, dev, variant, dt, route):
    """The run-time-flag epilogues of the gemm.hip kernels: STATS (launch_bs<.., true, ..> / gemm_nt_kernel<T, -1>), RESID with a
    row modulus, OUT_F32 and DETECT's (B, na, HW, no) store."""
    variant(0 if route == "bs" else 1)
    r_stats, r_rmod, r_out32, r_det = _runtime_flags_route(dt, route)
    M, N, K = 300, 136, SHORT_K[dt]
    segs = make_a(dev, dt, M, K, lim=1)
    wbuf, wv = make_w(dev, dt, N, K, lim=1)
    v = G.gather_a(segs, M, None) @ wv.double().t()
    # statistics: |v| <= K <= 192, per-workgroup f32 sums of v^2 over <= 300 rows stay below 2^24 - exact
    stats = torch.zeros(16, 2, N, device=dev, dtype=torch.float64)
    out = G.sentinel_buffer(M + 3, N + 8, dt, dev)
    G.run_expecting(lambda: nt_call(ops, segs, wbuf, out, M, N, K, ldc=N + 8, stats=stats),
                    [r_stats])
    G.assert_bits(out[:M, :N], G.rne(v, dt), "stats output")
    G.assert_sentinel_outside(out, slice(0, M), slice(0, N), "stats output")
    st = stats.sum(0)
    assert torch.equal(st[0], v.sum(0)) and torch.equal(st[1], (v * v).sum(0)), "column statistics are not exact"
    # RESID with rmod (pos_embed broadcast over the batch)
    r = G.ints((100, N), 64, 8, dev)
    out = G.sentinel_buffer(M + 3, N + 8, dt, dev)
    G.run_expecting(lambda: nt_call(ops, segs, wbuf, out, M, N, K, ldc=N + 8, resid=r.to(dt), rmod=100),
                    [r_rmod])
    G.assert_bits(out[:M, :N], G.rne(v + r.double()[torch.arange(M, device=dev) % 100], dt), "rmod residual")
    # OUT_F32 (A-stationary at short K, else the K-loop kernel) and DETECT (always the K-loop kernel)
    out = G.sentinel_buffer(M + 3, N + 4, F32, dev)
    G.run_expecting(lambda: nt_call(ops, segs, wbuf, out, M, N - 3, K, ldc=N + 4, out_f32=True), [r_out32])
    G.assert_bits(out[:M, :N - 3], G.rne(v[:, :N - 3], F32), "OUT_F32")
    G.assert_sentinel_outside(out, slice(0, M), slice(0, N - 3), "OUT_F32")
    B, na, no, hw = 3, 3, 17, 100
    det = G.sentinel_buffer(B * na * hw, no, F32, dev)
    wd = wv[:na * no]
    G.run_expecting(lambda: nt_call(ops, segs, wbuf, det, M, na * no, K, detect=(na, no, hw)), [r_det])
    ref = (G.gather_a(segs, M, None) @ wd.double().t()).view(B, hw, na, no).permute(0, 2, 1, 3).reshape(-1, no)
    G.assert_bits(det, G.rne(ref, F32), "DETECT")


# ------------------------------------------------------------------ §3 TN
def run_tn(ops, dev, dt, M, N, K, *, expect, splits=None, scratch=None, dbias=True, kperm=None, spatial=None, segs=None,
           y_off=8, ldy_pad=16, lddw_pad=8, acc=True, lim=4):
    """dW[N][K] (+)= dY^T X bit-exactly: |dy|, |x| <= 4 (2 at M > 1024) and M <= 4096 keep every partial sum <= 2^16."""
    lim = lim if M <= 1024 else 2
    ldy = y_off + N + ldy_pad
    ybuf, yv = G.poisoned(G.ints((M, N), lim, 21, dev), dt, ld=ldy, col0=y_off)
    segs = segs or make_a(dev, dt, M, K, nseg=2 if K % 16 == 0 else 1, lim=lim, seed=22)
    lddw = K + lddw_pad
    dW = G.sentinel_buffer(N + 2, lddw, F32, dev)
    dW0 = G.ints((N, K), 50, 23, dev) if acc else torch.zeros(N, K, device=dev)
    dW[:N, :K] = dW0
    db = None
    if dbias:
        db = G.sentinel_buffer(N + 4, 1, F32, dev).view(-1)
        db0 = G.ints((N,), 50, 24, dev) if acc else torch.zeros(N, device=dev)
        db[:N] = db0
    if scratch is not None:
        # NaN everywhere: slices past the live ones are never written, so a reduction that read them (or any stale slot) fails
        ops.set_tn_scratch(torch.full((scratch,), float("nan"), device=dev))
    G.run_expecting(lambda: ops.gemm_tn(ybuf, G.segspecs(ops, segs), dW, M, N, K, ldy=ldy, y_off=y_off, spatial=spatial, dbias=db,
                                        lddw=lddw, kperm=kperm, splits=splits), expect)
    x = G.gather_a(segs, M, spatial)
    g = yv.double().t() @ x                               # [N][K], column k = tap * C + ci
    if kperm is not None:
        c, t = kperm
        g = g.view(N, t, c).transpose(1, 2).reshape(N, K)
    G.assert_bits(dW[:N, :K], G.rne(dW0.double() + g, F32), f"dW {expect} M={M} N={N} K={K} splits={splits}", tile=(256, 192))
    G.assert_sentinel_outside(dW, slice(0, N), slice(0, K), "dW")
    if dbias:
        G.assert_bits(db[:N].view(1, -1), G.rne(db0.double() + yv.double().sum(0), F32).view(1, -1), f"dbias {expect}")
        assert bool((G.int_view(db[N:]) == G.F32_SENTINEL).all()), "dbias written past N"


def _live(M, splits):
    rows_per = -(-(-(-M // splits)) // 32) * 32
    return -(-M // rows_per)


def _swap(N, K):
    a = ((N + 255) // 256) * 256 * ((K + 191) // 192) * 192
    b = ((K + 255) // 256) * 256 * ((N + 191) // 192) * 192
    return b < a


TN3_CASES = [
    # (M, N, K, splits, scratch) - N and K on both sides of sodt_tn3_swap (192 x 256 swaps, 256 x 192 does not, 192 x 192 ties)
    (1025, 192, 256, 16, "fit"),        # live = 11 of 16 slices: empty trailing slices, reduced from the scratch
    (1025, 256, 192, 16, None),         # the same with atomics
    (1025, 192, 192, 32, "fit"),        # live = 17, the last live slice is exactly one row
    (2048, 192, 192, 1, None),          # splits = 1
    (1536, 192, 256, 8, "small"),       # scratch smaller than splits N K: atomics
    (1100, 136, 200, 4, "fit"),         # N, K not tile multiples (swap)
    (1100, 8, 192, 4, None),            # N = 8 (tie: no swap)
]


def _tn3_route(M, N, K, splits, scratch, dbias):
    return [G.tn3(_swap(N, K), False)] + ([G.TN3_REDUCE] if scratch == "fit" and splits > 1 else [])


TN3_ROWS = [c + (b,) for c in TN3_CASES for b in (True, False)]


@pytest.mark.parametrize("M,N,K,splits,scratch,dbias", routed(TN3_ROWS, _tn3_route))
def test_tn3(ops, dev, variant, M, N, K, splits, scratch, dbias):
    variant(0)
    need = splits * N * K
    expect = _tn3_route(M, N, K, splits, scratch, dbias)
    if M == 1025 and splits == 16:
        assert _live(M, splits) == 11
    if M == 1025 and splits == 32:
        assert _live(M, splits) == 17 and M - 16 * 64 == 1
    run_tn(ops, dev, BF, M, N, K, expect=expect, splits=splits,
           scratch=(need + 64 if scratch == "fit" else need // 2 if scratch == "small" else None), dbias=dbias)


def _tn3_conv_route(taps, N, C, scratch):
    return [G.tn3(_swap(N, len(taps) * C), True)] + ([G.TN3_REDUCE] if scratch else [])


@pytest.mark.parametrize("taps,N,C,scratch", routed([(TAPS2, 192, 64, True), (TAPS3, 64, 64, False), (TAPS3, 192, 64, True)],
                                                   _tn3_conv_route))
def test_tn3_conv_kperm(ops, dev, variant, taps, N, C, scratch):
    """Convolution weight gradients in the torch layout (kperm with 4 and 9 taps) through the spatial instantiations."""
    variant(0)
    B, H, W = 2, 16, 36
    M, K = B * H * W, len(taps) * C
    segs = _spatial_segs(dev, BF, B, H, W, C, taps)
    for s in segs:
        s["buf"] = s["buf"].clamp(-2, 2)
    splits = 4
    run_tn(ops, dev, BF, M, N, K, expect=_tn3_conv_route(taps, N, C, scratch), splits=splits, scratch=splits * N * K if scratch else None, kperm=(C, len(taps)),
           spatial=(H, W), segs=segs)


TN2 = [(dt,) + c for dt in (BF, F32) for c in [(700, 136, 200, 3, True), (700, 136, 200, 3, False), (300, 8, 192, 1, True),
                                                (1000, 192, 384, 5, False)]]


def _tn2_route(dt, M, N, K, splits, dbias):
    return [G.tn2(dt)]


@pytest.mark.parametrize("dt,M,N,K,splits,dbias", routed(TN2, _tn2_route), ids=_ids(TN2))
def test_tn2(ops, dev, variant, dt, M, N, K, splits, dbias):
    variant(0)
    run_tn(ops, dev, dt, M, N, K, expect=_tn2_route(dt, M, N, K, splits, dbias), splits=splits, dbias=dbias)


TNK = [(dt,) + c for dt in (BF, F32) for c in [(700, 200, 264, 3, True), (700, 200, 264, 3, False), (300, 8, 192, 1, True),
                                                (1000, 384, 384, 5, False)]]


def _tnk_route(dt, M, N, K, splits, dbias):
    return [G.tnk(dt)]


@pytest.mark.parametrize("dt,M,N,K,splits,dbias", routed(TNK, _tnk_route), ids=_ids(TNK))
def test_tn_kernel_128(ops, dev, variant, dt, M, N, K, splits, dbias):
    variant(1)
    run_tn(ops, dev, dt, M, N, K, expect=_tnk_route(dt, M, N, K, splits, dbias), splits=splits, dbias=dbias)


TN_CONV = [(dt, hook, N) for dt in (BF, F32) for (hook, N) in ((0, 64), (1, 200))]


def _tn_conv_route(dt, hook, N):
    return [G.tn2(dt) if hook == 0 else G.tnk(dt)]


@pytest.mark.parametrize("dt,hook,N", routed(TN_CONV, _tn_conv_route), ids=_ids(TN_CONV))
def test_tn_conv_kperm(ops, dev, variant, dt, hook, N):
    """3x3 convolution weight gradient in the torch layout (kperm, 9 taps) on launch_tn2 and the 128 x 128 kernel (M < 1024)."""
    variant(hook)
    B, H, W, C = 2, 8, 12, 32
    segs = _spatial_segs(dev, dt, B, H, W, C, TAPS3)
    run_tn(ops, dev, dt, B * H * W, N, 9 * C, expect=_tn_conv_route(dt, hook, N), splits=2, kperm=(C, 9), spatial=(H, W), segs=segs,
           dbias=(hook == 0))


# ------------------------------------------------------------------ §4 activation sweeps: every finite bf16 in [-16, 16]
def _sweep_x(dev):
    xs = G.finite_bf16_in(-16.0, 16.0, dev)
    return torch.cat([xs, torch.tensor([-300.0, -40.0, 40.0, 300.0, 3000.0], device=dev)])


SWEEP = [(k, r, d) for k in ("gelu_dual", "gelu", "dgelu", "silu")
         for (r, d) in (("nt3", BF), ("bs", BF), ("bs", F32), ("as", BF), ("as", F32), ("nt", BF), ("nt", F32))
         if not (k == "silu" and r == "nt3")]
SWEEP_CF = {"gelu_dual": 5, "gelu": 257, "dgelu": 8, "silu": 32}


def _sweep_route(kind, route, dt):
    cf = SWEEP_CF[kind]
    if route == "nt3":
        return [G.nt3(cf)]
    if route == "bs":
        return [G.bs(dt, False, cf, True) if cf in (5, 8) else G.bs(dt, False, -1, False)]
    if route == "as":
        return [G.as_(dt)]
    return [G.ntk(dt, cf if cf in (5, 8) else -1)]


@pytest.mark.parametrize("kind,route,dt", routed(SWEEP, _sweep_route), ids=[f"{k}-{r}-{'bf16' if d == BF else 'f32'}" for (k, r, d) in SWEEP])
def test_activation_sweep(ops, dev, variant, route, dt, kind):
    """One-hot A (one entry x per row) and identity W make the pre-activation exactly x; for DGELU, A W^T = 1 and aux = x.
    (AFFINE_SILU has no pipelined instantiation.)"""
    xs = _sweep_x(dev)
    K = N = {("nt3", BF): 192, ("bs", BF): 64, ("bs", F32): 32, ("as", BF): 64, ("as", F32): 32, ("nt", BF): 128,
             ("nt", F32): 64}[(route, dt)]
    M = (xs.numel() + 255) // 256 * 256
    x = torch.zeros(M, device=dev)
    x[:xs.numel()] = xs
    variant({"nt": 1, "as": 2}.get(route, 0))
    rows = torch.arange(M, device=dev)
    if kind == "dgelu":
        A = torch.zeros(M, K, device=dev, dtype=dt); A[:, 0] = 1
        Wm = torch.zeros(N, K, device=dev, dtype=dt); Wm[:, 0] = 1
        aux = x.view(-1, 1).expand(M, N).contiguous().to(dt)
        xm = aux.double()
    else:
        A = torch.zeros(M, K, device=dev, dtype=dt); A[rows, rows % K] = x.to(dt)
        Wm = torch.eye(N, K, device=dev, dtype=dt)
        xm = A.double()
    out = G.sentinel_buffer(M, N, dt, dev)
    zero = torch.zeros(N, device=dev)
    kw = {"gelu_dual": lambda: dict(bias=zero, gelu_out=out2), "gelu": lambda: dict(bias=zero, gelu_only=True),
          "dgelu": lambda: dict(dgelu_aux=aux), "silu": lambda: dict(affine=(torch.ones(N, device=dev), zero))}
    out2 = G.sentinel_buffer(M, N, dt, dev)
    expect = _sweep_route(kind, route, dt)
    G.run_expecting(lambda: ops.gemm_nt([ops.SegSpec(A)], Wm, out, M, N, K, **kw[kind]()), expect)
    got = out2 if kind == "gelu_dual" else out
    f = {"gelu_dual": G.gelu64, "gelu": G.gelu64, "dgelu": G.dgelu64, "silu": G.silu64}[kind]
    fk = {"gelu_dual": "gelu", "gelu": "gelu", "dgelu": "dgelu", "silu": "silu"}[kind]
    G.assert_within(got, f(xm), G.act_bound(fk, dt, xm), f"{kind} on {expect}")
    if kind == "gelu_dual":
        G.assert_bits(out, xm.to(dt), "GELU_DUAL pre-activation")


# ------------------------------------------------------------------ §5 the engine's GEMM routes are all covered above
@pytest.mark.parametrize("img,dt,sr", [(512, BF, False), (256, F32, False), (256, BF, True)], ids=["512-bf16", "256-f32", "sr-256-bf16"])
def test_engine_gemm_routes_are_covered(ops, dev, variant, img, dt, sr):
    from oracle import ref_torch as R
    if sr:
        from test_model_sr_gpu import build
    else:
        from test_model_gpu import build
    variant(0)
    model, _ = build(dev, img)
    model.compute_dtype = dt
    model.train()
    x_rgb, x_ir = R.synthetic_inputs(1, img, seed=2)

    def step():
        out = model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
        loss = 0
        stack = [out]
        while stack:
            o = stack.pop()
            if isinstance(o, (list, tuple)):
                stack.extend(o)
            elif torch.is_tensor(o) and o.requires_grad:
                loss = loss + o.float().square().mean()
        loss.backward()
    step()                                   # plans are recorded on the first call; the profiled step replays them
    used = set(G.gemm_kernels(G.launched_kernels(step)))
    assert used, "no GEMM kernel seen in a training step: the profiler did not see the library"
    missing = sorted(used - COVERED)
    assert not missing, f"GEMM instantiations the step launches that no exact case covers: {missing}"
