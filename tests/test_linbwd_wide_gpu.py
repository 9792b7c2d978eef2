"""sodt_linear_bwd_wide (csrc/linbwd.hip): the backward of the 192 -> 576 linear layer (attn.qkv), dX, dW and dbias from one
launch: three sibling workgroups per M-slice, each owning a 64-column slab of K.

Exact cases use the integer construction of tests/gemm_cases.py: |dy|, |x|, |w| <= 4 and M <= 4096, so every product is exact in
f32 and every partial sum stays below 2^24 (dX: |sum| <= 576 * 16; dW: |sum| <= 4096 * 16 plus a pre-fill <= 100; dbias: <= 4096 * 4
plus the pre-fill) whatever the summation order.  dX must then equal the f64 reference rounded once to bf16, dW / dbias the exact
f32 values, bit for bit - through the scratch (fixed-order reduction) and through the atomics alike.  Operand rows and columns
outside the views hold NaN: a stage that reads past the end of its slice, or a column past 576, poisons an output.

Random data: dW and dbias sum M products in f32 in some order, then add the result to dW: the standard bound of recursive f32
summation, (M + 2) 2^-24 sum_m |dy||x| per element (M - 1 additions - the products round nowhere, bf16 x bf16 is exact in f32 -
the slice sum and the += into dW make it M + 1, and one more is the usual slack of the first-order bound).  Nothing in it comes
from a kernel."""
import ctypes
import types

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
N, K = 576, 192
WIDE, REDUCE = "linbwd_wide_kernel", "linbwd_reduce_kernel"


def _call(pkg, *, dY, ldy, X, ldx, wT, ldw, dX, lddx, dW, lddw, M, dbias=None, N=N, K=K, splits=1, scratch=None, dtype=None,
          flags=0, dx_byte_off=0):
    L = pkg._lib
    g = L.LinBwdArgs()
    g.dY, g.ldy, g.X, g.ldx, g.wT, g.ldw = dY.data_ptr(), ldy, X.data_ptr(), ldx, wT.data_ptr(), ldw
    g.dX, g.lddx, g.dW, g.lddw = dX.data_ptr() + dx_byte_off, lddx, dW.data_ptr(), lddw
    g.dbias = None if dbias is None else dbias.data_ptr()
    g.M, g.N, g.K, g.splits, g.flags = M, N, K, splits, flags
    if scratch is not None:
        g.partial, g.partial_floats = scratch.data_ptr(), scratch.numel()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.load().sodt_linear_bwd_wide(ctypes.byref(g), L.BF16 if dtype is None else dtype, st)
    torch.cuda.synchronize()
    return rc


def _scratch(kind, splits, dev):
    if kind == "fits":
        return torch.full((splits * N * (K + 1),), float("nan"), device=dev)
    if kind == "tiles":                                     # room for the dW tiles only: dbias keeps its atomics
        return torch.full((splits * N * K,), float("nan"), device=dev)
    if kind == "small":
        return torch.full((splits * N * K - 1,), float("nan"), device=dev)
    return None


def _exact_case(pkg, dev, M, splits, *, scratch="fits", bias=True, prefill=True, names=None):
    """One integer case, every leading dimension off its width: dY a 576-column window at column 16 of a NaN buffer with ldy = 600,
    X and dX with ld = 200, dW with lddw = 196, wT with ldw = 584.  Checks dX, dW, dbias and everything around them bit for bit."""
    ldy, ycol, ldx, lddx, lddw, ldw = 600, 16, 200, 200, 196, 584
    dy = G.ints((M, N), 4, 31, dev)
    x = G.ints((M, K), 4, 32, dev)
    w = G.ints((N, K), 4, 33, dev)                           # W[n][k]
    dYb, dYv = G.poisoned(dy, BF, ld=ldy, col0=ycol)
    Xb, Xv = G.poisoned(x, BF, ld=ldx)
    wTb, wTv = G.poisoned(w.t().contiguous(), BF, ld=ldw, pad_rows=0)       # wT[k][n]
    dXb = G.sentinel_buffer(M + 3, lddx, BF, dev)
    dWb = G.sentinel_buffer(N, lddw, torch.float32, dev)
    w0 = G.ints((N, K), 100, 34, dev) if prefill else torch.zeros(N, K, device=dev)
    dWb[:, :K] = w0
    b0 = G.ints((N,), 100, 35, dev) if prefill else torch.zeros(N, device=dev)
    dbb = G.sentinel_buffer(1, N + 4, torch.float32, dev)
    dbb[0, :N] = b0
    scr = _scratch(scratch, splits, dev)

    def run():
        assert _call(pkg, dY=dYv, ldy=ldy, X=Xv, ldx=ldx, wT=wTv, ldw=ldw, dX=dXb, lddx=lddx, dW=dWb, lddw=lddw, M=M,
                     dbias=dbb if bias else None, splits=splits, scratch=scr) == 0
    if names is None:
        run()
    else:
        names.extend(G.launched_kernels(run))
    what = f"M={M} splits={splits} scratch={scratch}"
    G.assert_bits(dXb[:M, :K], G.rne(dy.double() @ w.double(), BF), what + " dX", tile=(32, 64))
    G.assert_sentinel_outside(dXb, slice(0, M), slice(0, K), what + " dX")
    G.assert_bits(dWb[:, :K], G.rne(w0.double() + dy.double().t() @ x.double(), torch.float32), what + " dW", tile=(144, 64))
    G.assert_sentinel_outside(dWb, slice(0, N), slice(0, K), what + " dW")
    want_b = b0.double() + (dy.double().sum(0) if bias else 0.0)
    G.assert_bits(dbb[:, :N], G.rne(want_b.view(1, N), torch.float32), what + " dbias", tile=(1, 16))
    G.assert_sentinel_outside(dbb, slice(0, 1), slice(0, N), what + " dbias")


@pytest.mark.parametrize("M,splits", [(33, 1), (96 + 7, 3), (2048 + 5, 4), (1024, 85)])
def test_exact_slices(pkg, dev, M, splits):
    """a ragged second stage; a ragged last slice, a dead one and slices of one or two stages (shorter than the ring); 17 stages per
    slice (the steady-state ring); 32 live slices of 85 (dead slices write no tile, the reduction reads the live ones only).  dW and
    dbias start from non-zero integers: +=, not =."""
    _exact_case(pkg, dev, M, splits)


@pytest.mark.parametrize("scratch", ["fits", "tiles", "small", None])
def test_exact_scratch_arms(pkg, dev, scratch):
    """scratch for tiles and dbias rows (the kernel and its reduction run, no atomics); for the tiles alone (dbias by atomics); one
    float short of the tiles, and none at all (atomics, one launch)"""
    names = []
    _exact_case(pkg, dev, 2048 + 5, 4, scratch=scratch, names=names)
    base = [n.split("<")[0] for n in names]
    assert base == ([WIDE, REDUCE] if scratch in ("fits", "tiles") else [WIDE]), names


def test_exact_without_dbias(pkg, dev):
    """dbias = NULL: the sentinel-guarded bias buffer is not handed over and must stay as it was"""
    _exact_case(pkg, dev, 96 + 7, 3, bias=False)
    _exact_case(pkg, dev, 33, 1, bias=False, scratch=None)


def test_exact_into_zeroed_outputs(pkg, dev):
    """the same sums into zeroed dW / dbias (the pre-filled runs above check +=)"""
    _exact_case(pkg, dev, 96 + 7, 3, prefill=False)


@pytest.fixture(scope="module")
def random_case(dev):
    M = 4096 + 32
    g = torch.Generator(device="cpu").manual_seed(7)
    dy = torch.randn(M, N, generator=g).to(BF)
    x = torch.randn(M, K, generator=g).to(BF)
    w = torch.randn(N, K, generator=g).to(BF)                  # W[n][k]
    k = (M + 2) * 2.0 ** -24
    d64, x64 = dy.double(), x.double()
    ref = dict(dW=d64.t() @ x64, dWb=k * (d64.abs().t() @ x64.abs()), db=d64.sum(0), dbb=k * d64.abs().sum(0))
    # the bound against a plain f32 order on the CPU, before any kernel is asked: blocked f32 matmul and column sums
    G.assert_within(dy.float().t() @ x.float(), ref["dW"], ref["dWb"], "CPU f32 dW")
    G.assert_within(dy.float().sum(0), ref["db"], ref["dbb"], "CPU f32 dbias")
    out = {n: v.to(dev) for n, v in ref.items()}
    out.update(M=M, dy=dy.to(dev), x=x.to(dev), wT=w.t().contiguous().to(dev))
    return out


def _run_random(pkg, dev, r, splits=8):
    M = r["M"]
    dX = G.sentinel_buffer(M, K, BF, dev)
    dW = torch.zeros(N, K, device=dev)
    db = torch.zeros(N, device=dev)
    scr = torch.empty(splits * N * (K + 1), device=dev)
    assert _call(pkg, dY=r["dy"], ldy=N, X=r["x"], ldx=K, wT=r["wT"], ldw=N, dX=dX, lddx=K, dW=dW, lddw=K, M=M, dbias=db,
                 splits=splits, scratch=scr) == 0
    return dX, dW, db


def test_random_data_against_the_two_launches(pkg, ops, dev, random_case):
    """N(0,1) bf16 operands, M = 4096 + 32, 8 slices.  dX: bit-identical to sodt_gemm_nt's.  dW / dbias: within the summation bound of
    the f64 reference - and so are sodt_gemm_tn's own."""
    r = random_case
    M = r["M"]
    dX, dW, db = _run_random(pkg, dev, r)
    want = G.sentinel_buffer(M, K, BF, dev)
    ops.gemm_nt([ops.SegSpec(r["dy"], N, 0)], r["wT"], want, M, K, N)
    dW2 = torch.zeros(N, K, device=dev)
    db2 = torch.zeros(N, device=dev)
    ops.gemm_tn(r["dy"], [ops.SegSpec(r["x"])], dW2, M, N, K, dbias=db2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    G.assert_bits(dX, want, "dX vs sodt_gemm_nt", tile=(32, 64))
    G.assert_within(dW2, r["dW"], r["dWb"], "sodt_gemm_tn dW")
    G.assert_within(db2, r["db"], r["dbb"], "sodt_gemm_tn dbias")
    G.assert_within(dW, r["dW"], r["dWb"], "dW")
    G.assert_within(db, r["db"], r["dbb"], "dbias")


def test_deterministic_with_scratch(pkg, dev, random_case):
    """scratch fits: two calls into zeroed dW (and dbias) give identical bits"""
    a, b = _run_random(pkg, dev, random_case), _run_random(pkg, dev, random_case)
    for u, v, what in zip(a, b, ("dX", "dW", "dbias")):
        G.assert_bits(u.view(-1, u.shape[-1]), v.view(-1, v.shape[-1]), "second call " + what)


@pytest.mark.parametrize("bad", ["N=192", "N=768", "K=384", "f32", "ldy=604", "dX+8", "flags"])
def test_refusals_write_nothing(pkg, dev, bad):
    """(the N = 768 width is not built: it stays refused)"""
    L = pkg._lib
    M = 64
    dY = torch.zeros(M, 768, device=dev, dtype=BF)
    X = torch.zeros(M, 384, device=dev, dtype=BF)
    wT = torch.zeros(384, 768, device=dev, dtype=BF)
    dX = G.sentinel_buffer(M + 1, 384, BF, dev)
    dW = G.sentinel_buffer(768, 384, torch.float32, dev)
    db = G.sentinel_buffer(1, 768, torch.float32, dev)
    kw = dict(dY=dY, ldy=768, X=X, ldx=384, wT=wT, ldw=768, dX=dX, lddx=384, dW=dW, lddw=384, M=M, dbias=db)
    if bad.startswith("N="):
        kw["N"] = int(bad[2:])
    elif bad == "K=384":
        kw["K"] = 384
    elif bad == "f32":
        kw["dtype"] = L.F32
    elif bad == "ldy=604":
        kw["ldy"] = 604
    elif bad == "dX+8":
        kw["dx_byte_off"] = 8
    else:
        kw["flags"] = L.EPI_DGELU
    assert _call(pkg, **kw) == L.EINVAL
    for buf, what in ((dX, "dX"), (dW, "dW"), (db, "dbias")):
        G.assert_sentinel_outside(buf, slice(0, 0), slice(0, 0), f"{bad}: {what}")


@pytest.mark.parametrize("cid", ["s1.0-bf16", "s1.1-bf16"])
def test_engine_block_backward_route(dev, cid):
    """One stage-1 block at S = 256, B = 2 (M = 8192), bf16, both MLP kinds (block 1 is shifted):
    * default switches: M is below Engine.wide_linbwd_min_rows, the backward launches no linbwd_wide_kernel;
    * wide_linbwd_min_rows = 0 and a fresh route record: exactly one, with one gemm_tn and one gemm_nt launch fewer; the block's dX
      is the same bits (the launch forms d(xn1) as sodt_gemm_nt does, and everything downstream reads only that); every parameter
      gradient passes the gate of tests/test_block_routes_gpu.py for the arm; attn.qkv.weight / .bias stay within the summation
      bound of the module docstring of the switch-off run (from the dqkv and xn1 buffers the kernels read);
    * use_wide_linbwd = False: no such launch again;
    * a frozen attn.qkv.weight and bias: Engine._linear_bwd leaves the plain sodt_gemm_nt."""
    import block_cases as BC
    import test_block_routes_gpu as TB
    case = next(c for c in BC.CASES if c.id == cid)
    model, eng, plan, P = TB.engine_for(dev, case.S, case.B, case.dtype, dict(TB.PREP_SWITCHES))
    ref = BC.reference(case)
    g = BC.geometry(case.tag, case.S, case.B)
    M, Cc = g.B * g.H * g.W, g.C
    assert (M, Cc) == (8192, 192) and eng.use_wide_linbwd is True and eng.wide_linbwd_min_rows == 85 * 512
    sname, i = case.tag.split(".")
    blk = getattr(model.image_encoder, sname)[int(i)]
    x_in = BC.block_input(case.tag, case.S, case.B).to(case.dtype).to(dev)
    dY = BC.grad_output(M, Cc).to(case.dtype).to(dev)
    pre = BC.E + case.tag + "."
    pnames = BC.param_names(case.tag, g.linear)
    qw, qb = pre + "attn.qkv.weight", pre + "attn.qkv.bias"

    def backward():
        eng.flat_grad.zero_()
        dX = torch.empty(M, Cc, device=dev, dtype=case.dtype)
        names = G.launched_kernels(lambda: eng._block_bwd(plan, P, case.tag, blk, dY, dX))
        fam = TB.families(names)
        fam["wide"] = sum(n.split("<")[0] == WIDE for n in names)
        return dX, {n: eng.g[n].clone() for n in pnames}, fam

    try:
        eng._block_fwd(plan, P, case.tag, blk, x_in, g.B, g.H, g.W)
        assert plan.saved[case.tag].wide_ok is False
        dX0, g0, f0 = backward()
        assert f0["wide"] == 0, f0
        eng.wide_linbwd_min_rows = 0
        eng._block_fwd(plan, P, case.tag, blk, x_in, g.B, g.H, g.W)
        assert plan.saved[case.tag].wide_ok is True
        dX1, g1, f1 = backward()
        dqkv, xn1 = plan.bufs[f"g.dqkv.{M}x{3 * Cc}"].double(), plan.bufs[case.tag + ".xn1"].double()
        eng.use_wide_linbwd = False
        _, _, f2 = backward()
        eng.use_wide_linbwd = True
        frozen = types.SimpleNamespace(trainable=lambda *names: False)
        dxn = torch.empty(M, Cc, device=dev, dtype=case.dtype)
        fz = G.launched_kernels(lambda: eng._linear_bwd(P, pre + "attn.qkv", plan.bufs[f"g.dqkv.{M}x{3 * Cc}"],
                                                        plan.bufs[case.tag + ".xn1"], dxn, M, 3 * Cc, Cc, wide=True, plan=frozen))
    finally:
        eng.use_wide_linbwd, eng.wide_linbwd_min_rows = True, 85 * 512
        eng._block_fwd(plan, P, case.tag, blk, x_in, g.B, g.H, g.W)      # the default route record again
        eng.flat_grad.zero_()
    assert f1["wide"] == 1 and f1["gemm_tn"] == f0["gemm_tn"] - 1 and f1["gemm_nt"] == f0["gemm_nt"] - 1, (f0, f1)
    assert {k: v for k, v in f1.items() if k not in ("wide", "gemm_tn", "gemm_nt")} == \
        {k: v for k, v in f0.items() if k not in ("wide", "gemm_tn", "gemm_nt")}, (f0, f1)
    assert f2 == f0, (f0, f2)
    assert TB.families(fz) == {"gemm_nt": 1} and not any(n.split("<")[0] in (WIDE, REDUCE) for n in fz), fz
    G.assert_bits(dX1, dX0, "block input gradient")
    bad = []
    for n in pnames:
        short = n[len(pre):]
        err, lim = BC.rel_l2(g1[n], ref.A[short]), BC.gate(case, ref, short)
        print(f"WIDE {cid} {short} err {err:.3e} gate {lim:.3e}")
        if not err <= lim:
            bad.append(f"{short}: {err:.3e} > {lim:.3e}")
    assert not bad, bad
    k = (M + 2) * 2.0 ** -24
    G.assert_within(g1[qw], g0[qw].double(), k * (dqkv.abs().t() @ xn1.abs()), "attn.qkv.weight against the two launches")
    G.assert_within(g1[qb], g0[qb].double(), k * dqkv.abs().sum(0), "attn.qkv.bias against the two launches")
