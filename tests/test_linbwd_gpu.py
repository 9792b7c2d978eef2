"""sodt_linear_bwd_sq (csrc/linbwd.hip): the backward of a square 192 -> 192 linear layer, dX and dW (+ dbias) from one read of dY.

Exact cases use the integer construction of tests/gemm_cases.py: |dy|, |x|, |w| <= 4 and M <= 4096, so every product is exact in
f32 and every partial sum stays below 2^24 (dX: |sum| <= 192 * 16; dW: |sum| <= 4096 * 16 plus a pre-fill <= 100; dbias: <= 4096 * 4
plus the pre-fill) whatever the summation order.  dX must then equal the f64 reference rounded once to bf16, dW / dbias the exact
f32 values, bit for bit - through the scratch (fixed-order reduction) and through the atomics fallback alike.  Operand rows beyond M
hold NaN: a stage that reads past the end of its slice poisons dW."""
import ctypes

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
C = 192


def _call(pkg, *, dY, ldy, X, ldx, wT, ldw, dX, lddx, dW, lddw, M, dbias=None, aux=None, ldaux=0, N=C, K=C, splits=1,
          scratch=None, dtype=None):
    L = pkg._lib
    g = L.LinBwdArgs()
    g.dY, g.ldy, g.X, g.ldx, g.wT, g.ldw = dY.data_ptr(), ldy, X.data_ptr(), ldx, wT.data_ptr(), ldw
    g.dX, g.lddx, g.dW, g.lddw = dX.data_ptr(), lddx, dW.data_ptr(), lddw
    g.dbias = None if dbias is None else dbias.data_ptr()
    if aux is not None:
        g.aux, g.ldaux, g.flags = aux.data_ptr(), ldaux, L.EPI_DGELU
    g.M, g.N, g.K, g.splits = M, N, K, splits
    if scratch is not None:
        g.partial, g.partial_floats = scratch.data_ptr(), scratch.numel()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.load().sodt_linear_bwd_sq(ctypes.byref(g), L.BF16 if dtype is None else dtype, st)
    torch.cuda.synchronize()
    return rc


def _exact_case(pkg, dev, M, splits, *, ldy=C, ycol=0, ldx=C, lddx=C, lddw=C, ldw=C, scratch="fits", bias=True, prefill=True, seed=0):
    """Runs one integer case and checks dX, dW, dbias and everything around them bit for bit; returns the operands."""
    dy = G.ints((M, C), 4, 11 + seed, dev)
    x = G.ints((M, C), 4, 12 + seed, dev)
    w = G.ints((C, C), 4, 13 + seed, dev)                     # W[n][k]
    dYb, dYv = G.poisoned(dy, BF, ld=ldy, col0=ycol)
    Xb, Xv = G.poisoned(x, BF, ld=ldx)
    wTb, wTv = G.poisoned(w.t().contiguous(), BF, ld=ldw, pad_rows=0)      # wT[k][n]
    dXb = G.sentinel_buffer(M + 3, lddx, BF, dev)
    dWb = G.sentinel_buffer(C, lddw, torch.float32, dev)
    w0 = G.ints((C, C), 100, 14 + seed, dev) if prefill else torch.zeros(C, C, device=dev)
    dWb[:, :C] = w0
    b0 = G.ints((C,), 100, 15 + seed, dev) if prefill else torch.zeros(C, device=dev)
    dbb = G.sentinel_buffer(1, C + 4, torch.float32, dev)
    dbb[0, :C] = b0
    if scratch == "fits":
        scr = torch.full((splits * C * (C + 1),), float("nan"), device=dev)
    elif scratch == "tiles":                                  # room for the dW tiles only: dbias keeps its atomics
        scr = torch.full((splits * C * C,), float("nan"), device=dev)
    elif scratch == "small":
        scr = torch.full((splits * C * C - 1,), float("nan"), device=dev)
    else:
        scr = None
    rc = _call(pkg, dY=dYv, ldy=ldy, X=Xv, ldx=ldx, wT=wTv, ldw=ldw, dX=dXb, lddx=lddx, dW=dWb, lddw=lddw, M=M,
               dbias=dbb if bias else None, splits=splits, scratch=scr)
    assert rc == 0
    what = f"M={M} splits={splits} scratch={scratch}"
    G.assert_bits(dXb[:M, :C], G.rne(dy.double() @ w.double(), BF), what + " dX", tile=(32, 32))
    G.assert_sentinel_outside(dXb, slice(0, M), slice(0, C), what + " dX")
    G.assert_bits(dWb[:, :C], G.rne(w0.double() + dy.double().t() @ x.double(), torch.float32), what + " dW", tile=(48, 96))
    G.assert_sentinel_outside(dWb, slice(0, C), slice(0, C), what + " dW")
    want_b = b0.double() + (dy.double().sum(0) if bias else 0.0)
    G.assert_bits(dbb[:, :C], G.rne(want_b.view(1, C), torch.float32), what + " dbias", tile=(1, 48))
    G.assert_sentinel_outside(dbb, slice(0, 1), slice(0, C), what + " dbias")


@pytest.mark.parametrize("M,splits", [(64, 1), (31, 1), (33, 1), (1025, 16), (1025, 32)])
def test_exact_slices(pkg, dev, M, splits):
    """one workgroup and two stages; a ragged only / last stage; 11 and 17 live slices of 16 and 32 (dead slices write no tile, the
    reduction reads the live ones only).  dW and dbias start from non-zero integers: += , not =."""
    _exact_case(pkg, dev, M, splits)


@pytest.mark.parametrize("scratch", ["small", "tiles", None])
def test_exact_atomics_fallback(pkg, dev, scratch):
    """scratch one float short of splits * N * K, scratch for the tiles alone (dbias by atomics), no scratch at all"""
    _exact_case(pkg, dev, 2048, 8, scratch=scratch)


def test_exact_leading_dimensions(pkg, dev):
    """every leading dimension independent of 192, dY at a column offset inside its buffer"""
    _exact_case(pkg, dev, 2048, 8, ldy=384, ycol=64, ldx=576, lddx=256, lddw=196, ldw=200)


def test_exact_without_dbias(pkg, dev):
    """dbias = NULL: the sentinel-guarded bias buffer is not handed over and must stay as it was"""
    _exact_case(pkg, dev, 1025, 16, bias=False)
    _exact_case(pkg, dev, 64, 1, bias=False, scratch=None)


@pytest.mark.parametrize("M,splits", [(33, 1), (1025, 4)])
def test_dgelu_form_matches_gemm_nt(pkg, ops, dev, M, splits):
    """SODT_EPI_DGELU: dX = (dY W) * gelu'(aux) with gemm_epi.h's own gelu' - the same function on the same exact f32 product as
    sodt_gemm_nt(..., dgelu_aux=...), so the two outputs agree bit for bit.  aux: multiples of 1/8 in [-5, 5] (bf16-exact, both
    sides of the polynomial's clamp at +-4), its own leading dimension.  dW / dbias are unaffected by the epilogue."""
    dy, x, w = G.ints((M, C), 4, 21, dev), G.ints((M, C), 4, 22, dev), G.ints((C, C), 4, 23, dev)
    aux = G.ints((M, C), 40, 24, dev) / 8.0
    dYb, dYv = G.poisoned(dy, BF, ld=200)
    Xb, Xv = G.poisoned(x, BF)
    auxb, auxv = G.poisoned(aux, BF, ld=208)
    wT = w.t().contiguous().to(BF)
    dXb = G.sentinel_buffer(M + 3, C, BF, dev)
    dW = torch.zeros(C, C, device=dev)
    db = torch.zeros(C, device=dev)
    scr = torch.full((splits * C * (C + 1),), float("nan"), device=dev)
    rc = _call(pkg, dY=dYv, ldy=200, X=Xv, ldx=C, wT=wT, ldw=C, dX=dXb, lddx=C, dW=dW, lddw=C, M=M, dbias=db, aux=auxv, ldaux=208,
               splits=splits, scratch=scr)
    assert rc == 0
    want = G.sentinel_buffer(M, C, BF, dev)
    ops.gemm_nt([ops.SegSpec(dYb, C, 0, ld=200)], wT, want, M, C, C, dgelu_aux=auxb)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    G.assert_bits(dXb[:M], want, f"M={M} dgelu dX vs sodt_gemm_nt", tile=(32, 32))
    G.assert_sentinel_outside(dXb, slice(0, M), slice(0, C), "dgelu dX")
    G.assert_bits(dW, G.rne(dy.double().t() @ x.double(), torch.float32), "dgelu dW", tile=(48, 96))
    G.assert_bits(db.view(1, C), G.rne(dy.double().sum(0).view(1, C), torch.float32), "dgelu dbias", tile=(1, 48))


def _dgelu_poly64(x):
    """dgelu_t<bf16> of csrc/common.h (the function gemm_epi.h's epilogue applies), evaluated in f64"""
    z = x.double().clamp(-4.0, 4.0)
    u = z * z
    p = torch.full_like(z, -1.642114889e-08)
    for c in (1.213881774e-06, -3.846123582e-05, 6.876639673e-04, -7.687550504e-03, 5.591514707e-02, -2.620302439e-01,
              7.967218161e-01):
        p = p * u + c
    return p * z + 0.5


@pytest.fixture(scope="module")
def random_case(dev):
    M = 4096
    g = torch.Generator(device="cpu").manual_seed(5)
    dy, x, aux = (torch.randn(M, C, generator=g).to(BF).to(dev) for _ in range(3))
    w = torch.randn(C, C, generator=g).to(BF).to(dev)          # W[n][k]
    d64, x64, w64 = dy.double(), x.double(), w.double()
    return dict(M=M, dy=dy, x=x, aux=aux, wT=w.t().contiguous(), dW=d64.t() @ x64, dWabs=d64.abs().t() @ x64.abs(),
                dX=d64 @ w64, dXabs=d64.abs() @ w64.abs(), db=d64.sum(0))


@pytest.mark.parametrize("form", ["plain", "dgelu"])
def test_random_data_against_f64(pkg, dev, random_case, form):
    """N(0,1) bf16 operands, M = 4096, splits = 16.  dW: f32 accumulation over M/32 stages per element, then the slices and the +=
    into dW: |err| <= (M/32 + splits + 1) 2^-24 sum|dy||x|.  dX: f32 accumulation over K = 192 and one bf16 rounding:
    |err| <= 2^-8 |ref| + 192 2^-24 sum|dy||w|.  (DGELU form: the reference multiplies by the epilogue's own gelu' polynomial.)"""
    r = random_case
    M, splits = r["M"], 16
    dX = G.sentinel_buffer(M, C, BF, dev)
    dW = torch.zeros(C, C, device=dev)
    db = torch.zeros(C, device=dev)
    scr = torch.empty(splits * C * (C + 1), device=dev)
    rc = _call(pkg, dY=r["dy"], ldy=C, X=r["x"], ldx=C, wT=r["wT"], ldw=C, dX=dX, lddx=C, dW=dW, lddw=C, M=M, dbias=db,
               aux=r["aux"] if form == "dgelu" else None, ldaux=C, splits=splits, scratch=scr)
    assert rc == 0
    G.assert_within(dW, r["dW"], (M / 32 + splits + 1) * 2.0 ** -24 * r["dWabs"], form + " dW")
    ref = r["dX"] * _dgelu_poly64(r["aux"]) if form == "dgelu" else r["dX"]
    G.assert_within(dX.float(), ref, 2.0 ** -8 * ref.abs() + 192 * 2.0 ** -24 * r["dXabs"], form + " dX")
    G.assert_within(db, r["db"], (M / 32 + splits + 1) * 2.0 ** -24 * r["dy"].double().abs().sum(0), form + " dbias")


def test_deterministic_with_scratch(pkg, dev, random_case):
    """scratch fits: two calls into zeroed dW (and dbias) give identical bits"""
    r = random_case
    M, splits = r["M"], 16
    outs = []
    for _ in range(2):
        dX = torch.empty(M, C, device=dev, dtype=BF)
        dW = torch.zeros(C, C, device=dev)
        db = torch.zeros(C, device=dev)
        scr = torch.empty(splits * C * (C + 1), device=dev)
        assert _call(pkg, dY=r["dy"], ldy=C, X=r["x"], ldx=C, wT=r["wT"], ldw=C, dX=dX, lddx=C, dW=dW, lddw=C, M=M, dbias=db,
                     splits=splits, scratch=scr) == 0
        outs.append((dX, dW, db.view(1, C)))
    for a, b, what in zip(outs[0], outs[1], ("dX", "dW", "dbias")):
        G.assert_bits(a, b, "second call " + what)


@pytest.mark.parametrize("bad", ["N=384", "f32", "ldy=196", "flags"])
def test_refusals_write_nothing(pkg, dev, bad):
    L = pkg._lib
    M = 64
    dY = torch.zeros(M, 392, device=dev, dtype=BF)
    X = torch.zeros(M, C, device=dev, dtype=BF)
    wT = torch.zeros(384, 384, device=dev, dtype=BF)
    dX = G.sentinel_buffer(M, 384, BF, dev)
    dW = G.sentinel_buffer(384, 384, torch.float32, dev)
    db = G.sentinel_buffer(1, 384, torch.float32, dev)
    kw = dict(dY=dY, ldy=392, X=X, ldx=C, wT=wT, ldw=384, dX=dX, lddx=384, dW=dW, lddw=384, M=M, dbias=db)
    if bad == "N=384":
        kw["N"] = 384
    elif bad == "f32":
        kw["dtype"] = L.F32
    elif bad == "ldy=196":
        kw["ldy"] = 196
    rc = _call(pkg, **kw) if bad != "flags" else None
    if bad == "flags":               # any epilogue but none / DGELU
        g = L.LinBwdArgs()
        g.dY, g.ldy, g.X, g.ldx, g.wT, g.ldw = dY.data_ptr(), 392, X.data_ptr(), C, wT.data_ptr(), 384
        g.dX, g.lddx, g.dW, g.lddw, g.dbias = dX.data_ptr(), 384, dW.data_ptr(), 384, db.data_ptr()
        g.M, g.N, g.K, g.splits, g.flags = M, C, C, 1, L.EPI_BIAS
        rc = L.load().sodt_linear_bwd_sq(ctypes.byref(g), L.BF16, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert rc == 1
    for buf, what in ((dX, "dX"), (dW, "dW"), (db, "dbias")):
        G.assert_sentinel_outside(buf, slice(0, 0), slice(0, 0), f"{bad}: {what}")


def test_engine_block_backward_switch(dev):
    """One stage-1 block (B = 1, 64 x 64 tokens, window 8, shift 2, the folded 2x2-conv MLP), bf16: Engine._block_bwd with
    use_fused_linbwd on and off.

    * The fused launch forms dX from the same f32 products and the same epilogue as sodt_gemm_nt, so every activation gradient of
      the block is IDENTICAL bits on the two paths: dc, dxm, dqkv and the block's input gradient dX.  Every other launch of the
      block therefore sees identical inputs.
    * The eight gradient tensors the switched launches write (attn.proj and mlp.fc2, weight and bias, on either path) are each
      checked against f64 (dxm^T ao, dY^T ca and the column sums, from the bf16 buffers the kernels read) within the random-data
      bound (M/32 + splits + 1) 2^-24 sum|dy||x|.  The builder does NOT match gemm_tn3's slice order (its own reduction sums the
      slices in its own fixed order), so the two paths are not compared bit for bit with each other.
    * attn.qkv.weight (gemm_tn3 through the scratch, fixed order) is deterministic and must be identical bits.  The remaining
      gradients of the block are accumulated with f32 atomics by kernels this change does not touch - norm1 / norm2 weight and bias
      (sodt_layernorm_bwd), attn.qkv.bias and the column sums behind conv1 / fc1 (gemm_tn3's dbias), the relative-position table
      (the attention backward) - so their bits vary from run to run on ONE path and are not compared; their inputs are, above."""
    from oracle import ref_torch as R
    from test_model_gpu import build
    S, B = 256, 1
    model, _ = build(dev, S)
    model.compute_dtype = BF
    model.train()
    x_rgb, x_ir = R.synthetic_inputs(B, S, seed=2)
    model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
    eng = model._get_engine()
    assert eng.use_fused_linbwd is True
    plan = next(p for p in eng.plans.values() if p.dt == BF and p.training)
    P = eng._prep_for(BF)
    tag, blk = "stage1.1", model.image_encoder.stage1[1]
    Bq, H, W, Cc, ws, shift = plan.saved[tag].geo
    assert (Bq, H, W, Cc, ws, shift) == (1, 64, 64, 192, 8, 2) and not blk.mlp.linear
    M = H * W
    gen = torch.Generator(device="cpu").manual_seed(9)
    dY = torch.randn(M, Cc, generator=gen).to(BF).to(dev)
    pre = "image_encoder." + tag + "."
    own = [pre + "attn.proj.weight", pre + "attn.proj.bias", pre + "mlp.fc2.weight", pre + "mlp.fc2.bias"]
    acts = [f"g.dxm.{M}x{Cc}", f"g.dc.{M}x{Cc}", f"g.dqkv.{M}x{3 * Cc}"]     # Plan.scratch: kind and shape
    res = {}
    for on in (True, False):
        eng.use_fused_linbwd = on
        eng.flat_grad.zero_()
        dX = torch.empty(M, Cc, device=dev, dtype=BF)
        names = G.launched_kernels(lambda: eng._block_bwd(plan, P, tag, blk, dY, dX))
        assert sum(n.startswith("linbwd_sq_kernel") for n in names) == (2 if on else 0), names
        res[on] = dict(dX=dX, g={n: eng.g[n].clone() for n in own + [pre + "attn.qkv.weight"]},
                       a={n: plan.bufs[n].clone() for n in acts})
    eng.use_fused_linbwd = True
    G.assert_bits(res[True]["dX"], res[False]["dX"], "block input gradient")
    for n in acts:
        G.assert_bits(res[True]["a"][n], res[False]["a"][n], n)
    G.assert_bits(res[True]["g"][pre + "attn.qkv.weight"], res[False]["g"][pre + "attn.qkv.weight"], "attn.qkv.weight")
    splits = max(1, min(M // 512, 256))
    k = (M / 32 + splits + 1) * 2.0 ** -24
    b = plan.bufs
    pairs = {pre + "attn.proj": (res[True]["a"][f"g.dxm.{M}x{Cc}"].double(), b[tag + ".ao"].double()),
             pre + "mlp.fc2": (dY.double(), b[tag + ".ca"].double())}
    for on in (True, False):
        for n in own:
            dy_, x_ = pairs[n.rsplit(".", 1)[0]]
            if n.endswith("weight"):
                ref, bound = dy_.t() @ x_, k * (dy_.abs().t() @ x_.abs())
            else:
                ref, bound = dy_.sum(0), k * dy_.abs().sum(0)
            assert float(ref.abs().max()) > 0
            G.assert_within(res[on]["g"][n], ref, bound, f"{n} (fused {'on' if on else 'off'})")
