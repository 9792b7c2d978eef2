"""sodt_mlp_bwd (csrc/mlpbwd.hip): the backward of the stage-1 linear MLP (fc1 192 -> 768, GELU, fc2 768 -> 192), dh, dW1 / db1 and
dW2 / db2 from one launch: eight sibling workgroups per M-slice, each owning a 96-column slab of the hidden dimension.

What is checked, and against what:
* dh: the bits of ops.gemm_nt(..., dgelu_rc=True) over [xn | dY] and [w1 | w2T] wherever that launch exists (M >= 256); below it,
  the f64 value (dY W2) gelu'(h) within the error of the documented arithmetic: the odd polynomial's 2.8e-4 on gelu' (common.h),
  one bf16 rounding of gelu' and one of dh (unit roundoff 2^-8 each), and the f32 accumulation of dA = dY W2 over K = 192.
* hact (the recomputed GELU(h)): within 2^-7 max|hact| of what sodt_mlp_fwd's training form writes for the same xn, the criterion of
  test_mlp_fused_matches_two_gemm_chain, no element excluded.
* dW1 / db1: the f64 products of the kernel's OWN dh bits with xn; dW2 / db2: of its own hact bits with dY.  Bound: recursive f32
  summation of M exact products (bf16 x bf16 is exact in f32), the slice sum and the += into a pre-filled dW, first-order slack of
  one: (M + 2) 2^-24 (sum_m |a||b| + |pre-fill|), the bound of tests/test_linbwd_wide_gpu.py with the pre-fill's share of the last
  addition written out.  A plain f32 matmul on the CPU is held to the same bound first.  Nothing in it comes from a kernel.
Operand rows and columns outside the views hold NaN, outputs sit in sentinel buffers with every leading dimension off its width."""
import ctypes

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
Cc, H4 = 192, 768
KERNEL, REDUCE = "mlp_bwd_kernel", "mlpbwd_reduce_kernel"
TILE = H4 * Cc


def _call(pkg, *, xn, ldxn, dY, ldy, w1, ldw1, b1, w2T, ldw2, dh, lddh, dW1, lddw1, db1, dW2, lddw2, db2, M, hact=None, ldha=0,
          C=Cc, splits=1, scratch=None, dtype=None, dh_byte_off=0):
    L = pkg._lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.load().sodt_mlp_bwd(xn.data_ptr(), ldxn, dY.data_ptr(), ldy, w1.data_ptr(), ldw1, b1.data_ptr(), w2T.data_ptr(), ldw2,
                               dh.data_ptr() + dh_byte_off, lddh, None if hact is None else hact.data_ptr(), ldha,
                               dW1.data_ptr(), lddw1, db1.data_ptr(), dW2.data_ptr(), lddw2, db2.data_ptr(), M, C, splits,
                               None if scratch is None else scratch.data_ptr(), 0 if scratch is None else scratch.numel(),
                               L.BF16 if dtype is None else dtype, st)
    torch.cuda.synchronize()
    return rc


def _scratch(kind, splits, dev):
    if kind == "fits":
        return torch.full((splits * (2 * TILE + H4 + Cc),), float("nan"), device=dev)
    if kind == "tiles":                                     # room for the two tiles only: the bias rows keep their atomics
        return torch.full((splits * 2 * TILE,), float("nan"), device=dev)
    if kind == "small":
        return torch.full((splits * 2 * TILE - 1,), float("nan"), device=dev)
    return None


def _operands(M, seed, wscale):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xn = torch.randn(M, Cc, generator=g).to(BF)
    dy = torch.randn(M, Cc, generator=g).to(BF)
    w1 = (torch.randn(H4, Cc, generator=g) * wscale).to(BF)             # fc1.weight
    w2T = (torch.randn(H4, Cc, generator=g) * wscale).to(BF)            # fc2.weight^T
    b1 = torch.randn(H4, generator=g) * 0.5
    return xn, dy, w1, w2T, b1


def _sum_bound(a64, b64, M, pre64=None):
    k = (M + 2) * 2.0 ** -24
    s = a64.abs().t() @ b64.abs()
    return k * (s if pre64 is None else s + pre64.abs())


def _dh_bound(xn, dy, w1, w2T, b1):
    """(reference, bound) of dh in f64 on the CPU"""
    h = xn.double() @ w1.double().t() + b1.double()
    dA = dy.double() @ w2T.double().t()
    gp = G.dgelu64(h)
    ref = dA * gp
    acc = (Cc + 2) * 2.0 ** -24 * (dy.double().abs() @ w2T.double().abs().t())
    # gelu' moves by at most 1.13 |dh| for an error dh of the recomputed pre-activation (max |gelu''| < 1.13)
    herr = 1.13 * (Cc + 2) * 2.0 ** -24 * (xn.double().abs() @ w1.double().abs().t() + b1.double().abs())
    gerr = 2.8e-4 + 2.0 ** -8 * (gp.abs() + 2.8e-4) + herr
    return ref, dA.abs() * gerr + acc * (gp.abs() + gerr) + 2.0 ** -8 * (ref.abs() + dA.abs() * gerr)


def _case(pkg, ops, dev, M, splits, *, scratch="fits", names=None, wscale=Cc ** -0.5):
    """One case with every leading dimension off its width and pre-filled gradients.  Returns nothing: asserts."""
    ldxn, ldy, ycol, ldw1, ldw2, lddh, ldha, lddw1, lddw2 = 200, 216, 16, 200, 208, 776, 784, 196, 772
    xn, dy, w1, w2T, b1 = _operands(M, 11 + M, wscale)
    xb, xv = G.poisoned(xn.to(dev), BF, ld=ldxn)
    yb, yv = G.poisoned(dy.to(dev), BF, ld=ldy, col0=ycol)
    w1b, w1v = G.poisoned(w1.to(dev), BF, ld=ldw1, pad_rows=0)
    w2b, w2v = G.poisoned(w2T.to(dev), BF, ld=ldw2, pad_rows=0)
    b1d = b1.to(dev)
    dhb = G.sentinel_buffer(M + 3, lddh, BF, dev)
    hab = G.sentinel_buffer(M + 3, ldha, BF, dev)
    dW1b = G.sentinel_buffer(H4, lddw1, torch.float32, dev)
    dW2b = G.sentinel_buffer(Cc, lddw2, torch.float32, dev)
    db1b = G.sentinel_buffer(1, H4 + 4, torch.float32, dev)
    db2b = G.sentinel_buffer(1, Cc + 4, torch.float32, dev)
    p1, p2 = G.ints((H4, Cc), 100, 34, dev), G.ints((Cc, H4), 100, 35, dev)
    q1, q2 = G.ints((H4,), 100, 36, dev), G.ints((Cc,), 100, 37, dev)
    dW1b[:, :Cc], dW2b[:, :H4], db1b[0, :H4], db2b[0, :Cc] = p1, p2, q1, q2
    scr = _scratch(scratch, splits, dev)

    def run():
        assert _call(pkg, xn=xv, ldxn=ldxn, dY=yv, ldy=ldy, w1=w1v, ldw1=ldw1, b1=b1d, w2T=w2v, ldw2=ldw2, dh=dhb, lddh=lddh,
                     hact=hab, ldha=ldha, dW1=dW1b, lddw1=lddw1, db1=db1b, dW2=dW2b, lddw2=lddw2, db2=db2b, M=M, splits=splits,
                     scratch=scr) == 0
    if names is None:
        run()
    else:
        names.extend(G.launched_kernels(run))
    what = f"M={M} splits={splits} scratch={scratch}"
    for buf, r, c, n in ((dhb, M, H4, "dh"), (hab, M, H4, "hact"), (dW1b, H4, Cc, "dW1"), (dW2b, Cc, H4, "dW2"), (db1b, 1, H4, "db1"),
                         (db2b, 1, Cc, "db2")):
        G.assert_sentinel_outside(buf, slice(0, r), slice(0, c), f"{what} {n}")
    dh, ha = dhb[:M, :H4], hab[:M, :H4]
    assert bool(torch.isfinite(dh.float()).all()) and bool(torch.isfinite(ha.float()).all()), what
    if M >= 256:
        want = G.sentinel_buffer(M, H4, BF, dev)
        wcat = torch.cat([w1, w2T], 1).contiguous().to(dev)
        ops.gemm_nt([ops.SegSpec(xn.to(dev)), ops.SegSpec(dy.to(dev))], wcat, want, M, H4, 2 * Cc, bias=b1d, dgelu_rc=True)
        torch.cuda.synchronize()
        G.assert_bits(dh, want, what + " dh vs sodt_gemm_nt(DGELU_RC)", tile=(32, 96))
    else:
        ref, bound = _dh_bound(xn, dy, w1, w2T, b1)
        G.assert_within(dh.cpu(), ref, bound, what + " dh")
    # hact against the forward's training form
    xo = torch.empty(M, Cc, device=dev, dtype=BF)
    haf = torch.empty(M, H4, device=dev, dtype=BF)
    ops.mlp_fwd(xn.to(dev), w1.to(dev), b1d, w2T.t().contiguous().to(dev), torch.zeros(Cc, device=dev), None, xo, haf, M, Cc)
    torch.cuda.synchronize()
    tol = 2.0 ** -7 * float(haf.float().abs().max())
    err = float((ha.float() - haf.float()).abs().max())
    print(f"MLPBWD {what} hact max err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (what, err, tol)
    # the weight gradients against the f64 products of the kernel's own dh / hact bits
    dh64, ha64, x64, y64 = dh.double(), ha.double(), xn.to(dev).double(), dy.to(dev).double()
    G.assert_within(dW1b[:, :Cc], p1.double() + dh64.t() @ x64, _sum_bound(dh64, x64, M, p1.double()), what + " dW1")
    G.assert_within(dW2b[:, :H4], p2.double() + y64.t() @ ha64, _sum_bound(y64, ha64, M, p2.double()), what + " dW2")
    k = (M + 2) * 2.0 ** -24
    G.assert_within(db1b[0, :H4], q1.double() + dh64.sum(0), k * (dh64.abs().sum(0) + q1.double().abs()), what + " db1")
    G.assert_within(db2b[0, :Cc], q2.double() + y64.sum(0), k * (y64.abs().sum(0) + q2.double().abs()), what + " db2")


@pytest.mark.parametrize("M,splits", [(33, 1), (96 + 7, 3), (2048 + 5, 4), (1024, 32)])
def test_slices(pkg, ops, dev, M, splits):
    """a ragged second stage; a ragged last slice, a dead one and slices of one or two stages (shorter than the ring); 17 stages per
    slice (the steady-state ring); 32 slices of one stage (1024 rows: all live) - and with splits = 3 at M = 103 the last is dead.
    dW and db start from non-zero integers: +=, not =."""
    _case(pkg, ops, dev, M, splits)


def test_dead_slices(pkg, ops, dev):
    """M = 96 in 32 slices: three live slices of one stage, 29 dead ones that write no tile (the reduction reads the live ones only)"""
    _case(pkg, ops, dev, 96, 32)


@pytest.mark.parametrize("scratch", ["fits", "tiles", "small", None])
def test_scratch_arms(pkg, ops, dev, scratch):
    """scratch for tiles and bias rows (the kernel and its reduction run, no atomics); for the tiles alone (biases by atomics); one
    float short of the tiles, and none at all (atomics, one launch)"""
    names = []
    _case(pkg, ops, dev, 2048 + 5, 4, scratch=scratch, names=names)
    base = [n.split("<")[0] for n in names]
    assert base == ([KERNEL, REDUCE] if scratch in ("fits", "tiles") else [KERNEL]), names


@pytest.fixture(scope="module")
def random_case(pkg, dev):
    """N(0,1) bf16 operands at M = 4128 (weights N(0,1) too: |h| ~ 14, gelu' mostly saturated - the slices above have h ~ N(0,1)),
    one call with 8 slices; the kernel's dh / hact bits come back to the CPU for the f32-order check."""
    M = 4096 + 32
    xn, dy, w1, w2T, b1 = _operands(M, 7, 1.0)
    d = {n: v.to(dev) for n, v in dict(xn=xn, dy=dy, w1=w1, w2T=w2T, b1=b1).items()}
    d["M"] = M
    return d


def _run_random(pkg, dev, r, splits=8):
    M = r["M"]
    dh = G.sentinel_buffer(M, H4, BF, dev)
    ha = G.sentinel_buffer(M, H4, BF, dev)
    dW1, dW2 = torch.zeros(H4, Cc, device=dev), torch.zeros(Cc, H4, device=dev)
    db1, db2 = torch.zeros(H4, device=dev), torch.zeros(Cc, device=dev)
    scr = torch.empty(splits * (2 * TILE + H4 + Cc), device=dev)
    assert _call(pkg, xn=r["xn"], ldxn=Cc, dY=r["dy"], ldy=Cc, w1=r["w1"], ldw1=Cc, b1=r["b1"], w2T=r["w2T"], ldw2=Cc, dh=dh, lddh=H4,
                 hact=ha, ldha=H4, dW1=dW1, lddw1=Cc, db1=db1, dW2=dW2, lddw2=H4, db2=db2, M=M, splits=splits, scratch=scr) == 0
    return dh, ha, dW1, db1.view(1, -1), dW2, db2.view(1, -1)


def test_random_data_against_the_three_launches(pkg, ops, dev, random_case):
    """dh: bit-identical to sodt_gemm_nt's SODT_EPI_BIAS | SODT_EPI_DGELU_RC.  dW1 / db1 / dW2 / db2: within the summation bound of
    the f64 products of the kernel's own dh / hact bits - and so is a plain f32 order on the CPU, asserted first."""
    r = random_case
    M = r["M"]
    dh, ha, dW1, db1, dW2, db2 = _run_random(pkg, dev, r)
    want = G.sentinel_buffer(M, H4, BF, dev)
    ops.gemm_nt([ops.SegSpec(r["xn"]), ops.SegSpec(r["dy"])], torch.cat([r["w1"], r["w2T"]], 1).contiguous(), want, M, H4, 2 * Cc,
                bias=r["b1"], dgelu_rc=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    G.assert_bits(dh, want, "dh vs sodt_gemm_nt(DGELU_RC)", tile=(32, 96))
    dhc, hac, xc, yc = dh.cpu(), ha.cpu(), r["xn"].cpu(), r["dy"].cpu()
    refs = {"dW1": (dhc, xc), "dW2": (yc, hac)}
    for name, got in (("dW1", dW1), ("dW2", dW2)):
        a, b = refs[name]
        ref, bound = a.double().t() @ b.double(), _sum_bound(a.double(), b.double(), M)
        G.assert_within(a.float().t() @ b.float(), ref, bound, "CPU f32 " + name)
        G.assert_within(got.cpu(), ref, bound, name)
    k = (M + 2) * 2.0 ** -24
    for name, got, a in (("db1", db1, dhc), ("db2", db2, yc)):
        ref, bound = a.double().sum(0), k * a.double().abs().sum(0)
        G.assert_within(a.float().sum(0), ref, bound, "CPU f32 " + name)
        G.assert_within(got.cpu().view(-1), ref, bound, name)


def test_deterministic_with_scratch(pkg, dev, random_case):
    """scratch fits: two calls into zeroed gradients give identical bits"""
    a, b = _run_random(pkg, dev, random_case), _run_random(pkg, dev, random_case)
    for u, v, what in zip(a, b, ("dh", "hact", "dW1", "db1", "dW2", "db2")):
        G.assert_bits(u, v, "second call " + what)


@pytest.mark.parametrize("bad", ["f32", "C=384", "hidden=384", "dh+8", "ldy=204"])
def test_refusals_write_nothing(pkg, ops, dev, bad):
    L = pkg._lib
    M = 64
    xn = torch.zeros(M, 384, device=dev, dtype=BF)
    dY = torch.zeros(M, 384, device=dev, dtype=BF)
    w1 = torch.zeros(H4, Cc, device=dev, dtype=BF)
    w2T = torch.zeros(H4, Cc, device=dev, dtype=BF)
    b1 = torch.zeros(H4, device=dev)
    dh = G.sentinel_buffer(M + 1, H4, BF, dev)
    ha = G.sentinel_buffer(M + 1, H4, BF, dev)
    dW1 = G.sentinel_buffer(H4, Cc, torch.float32, dev)
    dW2 = G.sentinel_buffer(Cc, H4, torch.float32, dev)
    db1 = G.sentinel_buffer(1, H4, torch.float32, dev)
    db2 = G.sentinel_buffer(1, Cc, torch.float32, dev)
    kw = dict(xn=xn, ldxn=384, dY=dY, ldy=384, w1=w1, ldw1=Cc, b1=b1, w2T=w2T, ldw2=Cc, dh=dh, lddh=H4, hact=ha, ldha=H4, dW1=dW1,
              lddw1=Cc, db1=db1, dW2=dW2, lddw2=H4, db2=db2, M=M)
    if bad == "hidden=384":       # the width of the hidden dimension is the shape of the weights: the wrapper refuses it
        w = torch.zeros(384, Cc, device=dev, dtype=BF)
        assert ops.mlp_bwd(xn, dY, w, b1[:384], w, dh, dW1, db1, dW2, db2, M, hact=ha) is False
    else:
        if bad == "f32":
            kw["dtype"] = L.F32
        elif bad == "C=384":
            kw["C"] = 384
        elif bad == "dh+8":
            kw["dh_byte_off"] = 8
        else:
            kw["ldy"] = 204
        assert _call(pkg, **kw) == L.EINVAL
    torch.cuda.synchronize()
    for buf, what in ((dh, "dh"), (ha, "hact"), (dW1, "dW1"), (dW2, "dW2"), (db1, "db1"), (db2, "db2")):
        G.assert_sentinel_outside(buf, slice(0, 0), slice(0, 0), f"{bad}: {what}")


def test_engine_block_backward_route(dev):
    """The unshifted stage-1 block at S = 256, B = 2 (M = 8192), bf16:
    * default switches: M is below Engine.mlp_bwd_min_rows, the block launches what it launched before (no mlp_bwd_kernel, GELU(h) kept);
    * mlp_bwd_min_rows = 0 and a fresh route record: exactly one mlp_bwd_kernel, two gemm_tn and one gemm_nt launch fewer; the
      forward runs the launch's inference form and writes no GELU(h) (the plan's buffer of the default route, which recorded
      launches hold, keeps a sentinel); the block's dX has the same bits (dh has, and everything downstream reads only dh); every
      parameter gradient passes the block's gate of tests/block_cases.py; fc1 / fc2 gradients stay within the summation bound
      of the module docstring of the switch-off run, from the dh, xn2, dY and GELU(h) buffers that run read;
    * a frozen fc1 or fc2 parameter: today's launches."""
    import block_cases as BC
    import test_block_routes_gpu as TB
    case = next(c for c in BC.CASES if c.id == "s1.0-bf16")
    model, eng, plan, P = TB.engine_for(dev, case.S, case.B, case.dtype, dict(TB.PREP_SWITCHES))
    ref = BC.reference(case)
    g = BC.geometry(case.tag, case.S, case.B)
    M = g.B * g.H * g.W
    assert (M, g.C) == (8192, 192) and eng.mlp_bwd_min_rows == 65536
    default_on = eng.use_fused_mlp_bwd
    blk = model.image_encoder.stage1[0]
    x_in = BC.block_input(case.tag, case.S, case.B).to(case.dtype).to(dev)
    dY = BC.grad_output(M, g.C).to(case.dtype).to(dev)
    pre = BC.E + case.tag + "."
    pnames = BC.param_names(case.tag, g.linear)
    hakey = case.tag + ".ha"

    def forward():
        """(launch families, the fused MLP kernel's instantiation, whether the GELU(h) buffer was written)"""
        G.int_view(plan.bufs[hakey]).fill_(G.BF16_SENTINEL)
        names = G.launched_kernels(lambda: eng._block_fwd(plan, P, case.tag, blk, x_in, g.B, g.H, g.W))
        mlp, = [n for n in names if n.split("<")[0] == "mlp_fwd_kernel"]
        return TB.families(names), mlp, not bool((G.int_view(plan.bufs[hakey]) == G.BF16_SENTINEL).all())

    def backward():
        eng.flat_grad.zero_()
        dX = torch.empty(M, g.C, device=dev, dtype=case.dtype)
        names = G.launched_kernels(lambda: eng._block_bwd(plan, P, case.tag, blk, dY, dX))
        fam = TB.families(names)
        fam["mlp_bwd"] = sum(n.split("<")[0] == KERNEL for n in names)
        return dX, {n: eng.g[n].clone() for n in pnames}, fam

    real_trainable = plan.trainable
    try:
        eng.use_fused_mlp_bwd = True
        fw0, k0, ha0 = forward()
        assert plan.saved[case.tag].mlp_bwd is False and ha0 and k0 == "mlp_fwd_kernel<true, true>", k0
        haf = plan.bufs[hakey].double()
        dX0, g0, f0 = backward()
        assert f0["mlp_bwd"] == 0, f0
        dh0 = plan.bufs[f"g.dh.{M}x{4 * g.C}"].double()
        xn2, dY64 = plan.bufs[case.tag + ".xn2"].double(), dY.double()
        eng.mlp_bwd_min_rows = 0
        fw1, k1, ha1 = forward()
        assert plan.saved[case.tag].mlp_bwd is True and not ha1 and fw1 == fw0 and k1 == "mlp_fwd_kernel<false, true>", (fw0, fw1, k1)
        dX1, g1, f1 = backward()
        G.assert_bits(plan.bufs[f"g.dh.{M}x{4 * g.C}"], dh0.to(case.dtype), "dh")
        # one frozen parameter of the four: the route falls back
        frozen = []
        for name in ("mlp.fc1.bias", "mlp.fc2.weight"):
            plan.trainable = lambda *ns, _n=pre + name: _n not in ns and real_trainable(*ns)
            frozen.append(eng._block_route(plan, P, case.tag, blk, x_in, g.B, g.H, g.W).mlp_bwd)
            plan.trainable = real_trainable
        eng.use_fused_mlp_bwd = False
        fw2, k2, ha2 = forward()
        assert plan.saved[case.tag].mlp_bwd is False and ha2 and k2 == k0
        _, _, f2 = backward()
    finally:
        plan.trainable = real_trainable
        eng.use_fused_mlp_bwd, eng.mlp_bwd_min_rows = default_on, 65536
        eng._block_fwd(plan, P, case.tag, blk, x_in, g.B, g.H, g.W)      # the default route record (and its GELU(h)) again
        eng.flat_grad.zero_()
    assert frozen == [False, False], frozen
    assert f1["mlp_bwd"] == 1 and f1["gemm_tn"] == f0["gemm_tn"] - 2 and f1["gemm_nt"] == f0["gemm_nt"] - 1, (f0, f1)
    rest = lambda f: {k: v for k, v in f.items() if k not in ("mlp_bwd", "gemm_tn", "gemm_nt")}
    assert rest(f1) == rest(f0), (f0, f1)
    assert f2 == f0, (f0, f2)
    G.assert_bits(dX1, dX0, "block input gradient")
    bad = []
    for n in pnames:
        short = n[len(pre):]
        err, lim = BC.rel_l2(g1[n], ref.A[short]), BC.gate(case, ref, short)
        print(f"MLPBWD s1.0-bf16 {short} err {err:.3e} gate {lim:.3e}")
        if not err <= lim:
            bad.append(f"{short}: {err:.3e} > {lim:.3e}")
    assert not bad, bad
    k = (M + 2) * 2.0 ** -24
    G.assert_within(g1[pre + "mlp.fc1.weight"], g0[pre + "mlp.fc1.weight"].double(), k * (dh0.abs().t() @ xn2.abs()), "fc1.weight vs the launches")
    G.assert_within(g1[pre + "mlp.fc1.bias"], g0[pre + "mlp.fc1.bias"].double(), k * dh0.abs().sum(0), "fc1.bias vs the launches")
    G.assert_within(g1[pre + "mlp.fc2.weight"], g0[pre + "mlp.fc2.weight"].double(), k * (dY64.abs().t() @ haf.abs()), "fc2.weight vs the launches")
    G.assert_within(g1[pre + "mlp.fc2.bias"], g0[pre + "mlp.fc2.bias"].double(), k * dY64.abs().sum(0), "fc2.bias vs the launches")
