"""Every Swin-block route of the engine against float64, one block at a time: Engine._block_fwd / _block_bwd on each arm that
Engine._block_route can choose (ATTN_FUSED_RC / FUSED_SAVED / PADDED / PLAIN x MLP_FUSED / LIN_RC / LIN_SAVED / FOLD / CONV, the
square linear backward on and off), compared with the exact block in float64 (tests/block_cases.py, reference A).

Gate.  bf16 routes: |T_gpu - T_A| / |T_A| <= 3 e_emul(T) + 1e-5, where e_emul(T) = |T_B - T_A| / |T_A| and B is the same float64
graph with a straight-through bf16 rounding wherever the bf16 route narrows a value (block_cases.narrow; the list is in
oracle.ref_torch.swin_block).  The margin 3 covers a second realisation of same-sized rounding noise and the approximate
placement of B's internal narrowing points (the fused arms narrow at fewer points); the floor covers f32 accumulation over at
most 16,384 rows (sqrt(M) 2^-24 = 8e-6).  f32 routes: 2e-3, test_model_gpu's f32 gradient gate.  Nothing in the gate comes from a
kernel.  xo and dX are also gated on row subsets (last grid row / column: the 2x2 convolution's pad border that
convmlp_border_fix corrects; the wrap region of a shifted block's mask; every other token), so that an error confined to a
border cannot dilute into the global norm.  mlp.fc2.bias: its gradient is the column sum of the given bf16 dY, which no narrowing
point touches, so e_emul is exactly 0 there and the gate is the floor.  On the conv-MLP blocks the convolution's pre-activation
cp, as the route stores it, is gated the same way: the residual sum hides that border in xo (skipping convmlp_border_fix moves
xo[border] by 7.4e-3 against a gate of 8.1e-3, cp[border] by 2.9e-2 against 1.0e-2).

Per case the test also pins the BlockRoute record, which kernels ran forward and backward (by family: a fused arm launches its
fused kernel and none of the launches it replaces), and that a second backward without clearing flat_grad doubles every
parameter gradient (every scratch a route expects to be zero is zero again).

x_in is the model's own activation in front of the block (the oracle's f32 encoder under R.synthetic_inputs, rounded to the run
dtype), the same tensor for every engine, so one reference serves every switch setting of a block.

Measured on an MI355X, worst tensor of each group as err / gate (3 e_emul + 1e-5, or 2e-3 on f32); per group and with e_emul per
tensor in DESIGN.md section 2, "Block routes against float64":

    case                   xo, cp (+subsets)    dX (+subsets)  weights, biases       bias table  second backward
    s1.0-bf16               3.0e-03/8.7e-03  3.0e-03/8.8e-03  4.4e-03/1.3e-02  6.1e-03/2.1e-02  4.4e-03/1.3e-02
    s1.0-bf16-mlp_off       3.0e-03/8.7e-03  3.0e-03/8.8e-03  4.4e-03/1.3e-02  6.1e-03/2.1e-02  4.4e-03/1.3e-02
    s1.0-bf16-wmsa_off      2.8e-03/8.7e-03  3.0e-03/8.8e-03  3.1e-03/8.6e-03  5.8e-03/2.1e-02  3.1e-03/8.6e-03
    s1.1-bf16               4.0e-03/1.0e-02  2.8e-03/8.5e-03  4.7e-03/1.4e-02  6.6e-03/2.4e-02  4.7e-03/1.4e-02
    s1.1-bf16-linbwd_off    4.0e-03/1.0e-02  2.8e-03/8.5e-03  4.7e-03/1.4e-02  6.6e-03/2.4e-02  4.7e-03/1.4e-02
    s1.1-bf16-fold_off      2.8e-03/8.1e-03  2.8e-03/8.5e-03  2.7e-03/7.6e-03  6.7e-03/2.3e-02  2.7e-03/7.6e-03
    s1.1-bf16-wmsa_off      3.8e-03/1.0e-02  2.7e-03/8.4e-03  2.7e-03/7.6e-03  6.7e-03/2.4e-02  2.7e-03/7.6e-03
    s2.0-bf16               2.8e-03/8.9e-03  2.9e-03/8.6e-03  2.7e-03/6.9e-03  9.1e-03/3.4e-02  2.7e-03/6.9e-03
    s2.1-bf16               3.7e-03/1.0e-02  2.7e-03/8.4e-03  2.0e-03/5.7e-03  1.2e-02/4.5e-02  2.0e-03/5.7e-03
    s3.0-bf16-S256          2.8e-03/8.7e-03  3.2e-03/8.4e-03  3.9e-03/8.8e-03  1.6e-02/4.9e-02  3.9e-03/8.8e-03
    s3.0-bf16-S512          2.8e-03/8.7e-03  3.2e-03/8.4e-03  4.5e-03/8.3e-03  1.8e-02/5.0e-02  4.5e-03/8.3e-03
    s3.0-bf16-S640          2.8e-03/8.8e-03  3.1e-03/8.6e-03  3.4e-03/8.1e-03  9.8e-03/3.0e-02  3.4e-03/8.1e-03
    s1.0-f32                2.9e-07/2.0e-03  3.6e-07/2.0e-03  8.3e-07/2.0e-03  9.2e-07/2.0e-03  9.8e-07/2.0e-03
    s1.1-f32                5.7e-07/2.0e-03  3.0e-07/2.0e-03  9.5e-07/2.0e-03  1.2e-06/2.0e-03  1.1e-06/2.0e-03
    s1.1-f32-wmsa_off       5.7e-07/2.0e-03  3.0e-07/2.0e-03  1.0e-06/2.0e-03  1.1e-06/2.0e-03  1.1e-06/2.0e-03
"""
import types
from collections import Counter

import pytest
import torch

import attn_cases as A
import block_cases as BC
import gemm_cases as G

pytestmark = pytest.mark.gpu
BF, F32 = BC.BF, BC.F32
HEADS = 12
PREP_SWITCHES = {"use_fused_wmsa": True, "convmlp_fold_maxc": 384}      # read when the parameter layouts are first prepared
NT = ("gemm_nt3_kernel", "gemm_nt_kernel", "gemm_as_kernel", "gemm_bs_kernel")
TN = ("gemm_tn3_kernel", "gemm_tn_kernel", "gemm_tn2_kernel")
SINGLE = BC.WATCHED_KERNELS

_engines = {}
_gpu_error = []      # a HIP error in one case: the cases after it launch nothing more


def engine_for(dev, S, B, dtype, prep):
    """(model, engine, plan, P) of a freshly built model with the given prepare-time switches, after one training forward."""
    from oracle import ref_torch as R
    from test_model_gpu import build
    key = (S, B, dtype, tuple(sorted(prep.items())))
    if key not in _engines:
        model, _ = build(dev, S)
        model.compute_dtype = dtype
        model.train()
        eng = model._get_engine()
        for k, v in prep.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
        x_rgb, x_ir = R.synthetic_inputs(B, S, seed=BC.SEED_X)
        model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
        plan = next(p for p in eng.plans.values() if p.dt == dtype and p.training and p.B == B and p.S == S)
        _engines[key] = (model, eng, plan, eng._prep_for(dtype))
    return _engines[key]


def family(name: str):
    base = name.split("<")[0]
    if base.startswith("attn_"):
        return name
    if base in NT:
        return "gemm_nt"
    if base in TN:
        return "gemm_tn"
    if base.startswith("ln_fwd"):
        return "ln_fwd"
    if base.startswith("ln_bwd"):
        return "ln_bwd"
    return base if base in SINGLE else None


def families(names):
    return dict(Counter(f for f in map(family, names) if f is not None))


def expected_fwd(case, hd, ws, shift):
    c = Counter()
    if case.attn == BC.FUSED_RC:
        c["wmsa_hg_kernel"] += 1
    elif case.attn == BC.FUSED_SAVED:
        c["wmsa_block_kernel"] += 1
    else:                                   # LayerNorm 1 and 2, the QKV and projection GEMMs, the attention kernel
        c["ln_fwd"] += 2
        c["gemm_nt"] += 2
        c.update(A.fwd_route(case.dtype, hd, ws, shift))
    if case.mlp == BC.M_FUSED:
        c["mlp_fwd_kernel"] += 1
    elif case.mlp in (BC.M_LIN_RC, BC.M_LIN_SAVED):
        c["gemm_nt"] += 2
    elif case.mlp == BC.M_FOLD:
        c["convmlp_compose_kernel"] += 1
        c["gemm_nt"] += 2
        c["convmlp_border_fix_kernel"] += 1
    else:
        c["gemm_nt"] += 3
    return dict(c)


def expected_bwd(case, hd, ws, shift, linbwd):
    c = Counter(ln_bwd=2)
    sq = linbwd and case.sq_ok

    def lin(one_launch):
        if one_launch:
            c["linbwd_sq_kernel"] += 1
        else:
            c["gemm_tn"] += 1
            c["gemm_nt"] += 1
    if case.mlp in (BC.M_FUSED, BC.M_LIN_RC, BC.M_LIN_SAVED):
        lin(False), lin(False)
    elif case.mlp == BC.M_FOLD:
        lin(sq)
        c["gemm_tn"] += 1
        c["convmlp_border_sums_kernel"] += 1
        c["convmlp_decompose_kernel"] += 1
        c["gemm_nt"] += 1
    else:
        lin(sq)
        c["gemm_tn"] += 1
        c["gemm_nt"] += 1
        lin(False)
    if case.attn == BC.PADDED:
        lin(False), lin(False)
        c.update(A.bwd_route(case.dtype, hd, ws, 0))
    else:
        lin(sq)
        c.update(A.RC_ROUTE if case.attn == BC.FUSED_RC else A.bwd_wm_route(case.dtype) if case.attn == BC.FUSED_SAVED
                 else A.bwd_route(case.dtype, hd, ws, shift))
        lin(False)
    return dict(c)


@pytest.mark.parametrize("case", BC.CASES, ids=[c.id for c in BC.CASES])
def test_block_route(dev, case):
    if _gpu_error:
        pytest.fail(f"not run: an earlier case ended in a GPU error ({_gpu_error[0]})")
    sw = dict(case.switches)
    prep = {k: sw.get(k, v) for k, v in PREP_SWITCHES.items()}
    live = {k: v for k, v in sw.items() if k not in PREP_SWITCHES}
    try:
        model, eng, plan, P = engine_for(dev, case.S, case.B, case.dtype, prep)
    except RuntimeError as e:
        _gpu_error.append(f"{case.id}: {e}")
        raise
    ref = BC.reference(case)
    BC.check_reference(case, ref)
    g = BC.geometry(case.tag, case.S, case.B)
    M = g.B * g.H * g.W
    ws = min(g.window, g.H)
    hd = g.C // HEADS
    sname, i = case.tag.split(".")
    blk = getattr(model.image_encoder, sname)[int(i)]
    x_in = BC.block_input(case.tag, case.S, case.B).to(case.dtype).to(dev)
    dY = BC.grad_output(M, g.C).to(case.dtype).to(dev)
    pre = BC.E + case.tag + "."
    pnames = BC.param_names(case.tag, g.linear)
    assert eng.use_fused_mlp is True and eng.use_fused_linbwd is True
    out = {}
    try:
        for k, v in live.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
        fwd_names = G.launched_kernels(lambda: out.__setitem__("xo", eng._block_fwd(plan, P, case.tag, blk, x_in, g.B, g.H, g.W)))
        r = plan.saved[case.tag]
        got = {"xo": out["xo"].clone()}
        if not g.linear:
            got["cp"] = plan.bufs[case.tag + ".cp"].clone()         # the convolution's pre-activation, as the route stores it
        eng.flat_grad.zero_()
        dX = torch.empty(M, g.C, device=dev, dtype=case.dtype)
        bwd_names = G.launched_kernels(lambda: eng._block_bwd(plan, P, case.tag, blk, dY, dX))
        got["dX"] = dX.clone()
        for n in pnames:
            got[n[len(pre):]] = eng.g[n].clone()
        dX2 = torch.empty(M, g.C, device=dev, dtype=case.dtype)
        eng._block_bwd(plan, P, case.tag, blk, dY, dX2)              # flat_grad NOT cleared: every parameter gradient doubles
        twice = {n[len(pre):]: eng.g[n].clone() for n in pnames}
        twice["dX"] = dX2
        torch.cuda.synchronize()
    except RuntimeError as e:
        _gpu_error.append(f"{case.id}: {e}")
        raise
    finally:
        eng.use_fused_mlp, eng.use_fused_linbwd = True, True
    eng.flat_grad.zero_()

    # ---- the route record and the launches (collected: every figure below is printed before anything is asserted)
    bad = []
    if (r.attn, r.mlp, r.sq_ok, r.zscratch, r.pad) != (case.attn, case.mlp, case.sq_ok, case.zscratch, case.pad):
        bad.append(f"route {r[2:]} where the case was written for {case[6:]}")
    if r.geo != (g.B, g.H, g.W, g.C, ws, g.shift):
        bad.append(f"geometry {r.geo}")
    if r.x_in is not x_in or (r.wpk is not None) != (case.attn in (BC.FUSED_RC, BC.FUSED_SAVED)):
        bad.append("route record: x_in / parameter pack")
    for what, names, want in (("forward", fwd_names, expected_fwd(case, hd, ws, g.shift)),
                              ("backward", bwd_names, expected_bwd(case, hd, ws, g.shift, live.get("use_fused_linbwd", True)))):
        if families(names) != want:
            bad.append(f"{what} launched {families(names)}, the arm is {want} (all kernels: {names})")

    # ---- values: every figure is printed before anything is asserted
    sub = BC.subsets(g)

    def measure(what, t, name, scale):
        a = ref.A[name] * scale
        err, lim = BC.rel_l2(t, a), BC.gate(case, ref, name)
        print(f"BLOCKROUTE {case.id} {what} {name} err {err:.3e} gate {lim:.3e} e_emul {ref.e_emul.get(name, float('nan')):.3e}")
        if not err <= lim:
            bad.append(f"{what} {name}: {err:.3e} > {lim:.3e}")

    def rows(t, name):
        return t if "[" not in name else t[sub[name[name.index("[") + 1:-1]].to(t.device)]
    for name in ref.A:
        base = name.split("[")[0]
        measure("once", rows(got[base], name), name, 1.0)
    for name in ref.A:
        base = name.split("[")[0]
        if base in ("xo", "cp"):
            continue
        measure("twice", rows(twice[base], name), name, 1.0 if base == "dX" else 2.0)
    assert not bad, f"{case.id}: " + "; ".join(bad)


# ------------------------------------------------------------------ the route table at the benchmark shape, without running it
def _routes(eng, model, dt, P, B, H1):
    plan = types.SimpleNamespace(dt=dt)
    enc = model.image_encoder
    table = {}
    for si, sname in enumerate(("stage1", "stage2", "stage3")):
        H = H1 >> si
        for i, blk in enumerate(getattr(enc, sname)):
            tag = f"{sname}.{i}"
            table[tag] = (blk, eng._block_route(plan, P, tag, blk, None, B, H, H))
    return table


def test_route_table_at_benchmark_shape(dev):
    """B = 8 @1024^2: 256 / 128 / 64 tokens a side in stages 1 / 2 / 3.  _block_route reads plan.dt, P and the geometry only, so the
    table is asked for without allocating a single activation.  A refactor that flips one condition drops a block to a slower,
    still correct arm: parity tests stay green, this does not.  (The fused W-MSA kernel exists for C = 192, window 8 only: stage 2
    and stage 3 run the plain arm - DESIGN.md, "Why stage 2 (C = 384) has no fused block kernel yet".)"""
    model, eng, _, Pb = engine_for(dev, 512, 1, BF, dict(PREP_SWITCHES))      # a 512-built model has the 32-token stage-3 window
    assert eng.use_fused_wmsa and eng.use_fused_mlp and eng.use_fused_linbwd and eng.convmlp_fold_maxc == 384
    bf = _routes(eng, model, BF, Pb, 8, 256)
    assert sorted(bf) == [f"stage1.{i}" for i in range(6)] + [f"stage2.{i}" for i in range(4)] + ["stage3.0"]
    for tag, (blk, r) in bf.items():
        s = int(tag[5])
        lin = blk.mlp.linear
        if s == 1:
            want = (BC.FUSED_RC, BC.M_FUSED if lin else BC.M_FOLD, True, False, None)
        elif s == 2:
            want = (BC.PLAIN, BC.M_LIN_RC if lin else BC.M_FOLD, False, False, None)
        else:
            want = (BC.PLAIN, BC.M_LIN_RC, False, True, None)
        assert (r.attn, r.mlp, r.sq_ok, r.zscratch, r.pad) == want, (tag, r[1:])
        assert (r.wpk is not None) == (s == 1) and r.x_in is None
        assert r.geo == (8, 256 >> (s - 1), 256 >> (s - 1), 192 << (s - 1), 32 if s == 3 else 8, blk.shift_size), (tag, r.geo)
    assert [bf[f"stage1.{i}"][0].mlp.linear for i in range(6)] == [True, False] * 3
    f32 = _routes(eng, model, F32, eng._prep_for(F32), 8, 256)
    for tag, (blk, r) in f32.items():
        s = int(tag[5])
        want = (BC.FUSED_SAVED if s == 1 else BC.PLAIN, BC.M_LIN_SAVED if blk.mlp.linear else BC.M_CONV, False, s == 3, None)
        assert (r.attn, r.mlp, r.sq_ok, r.zscratch, r.pad) == want, (tag, r[1:])
    # the two geometries the engine refuses, by name
    plan = types.SimpleNamespace(dt=BF)
    enc = model.image_encoder
    assert enc.stage1[1].shift_size > 0
    with pytest.raises(NotImplementedError, match="SHIFTED"):
        eng._block_route(plan, Pb, "stage1.1", enc.stage1[1], None, 1, 60, 60)       # 60 tokens: no multiple of the 8-token window
    with pytest.raises(NotImplementedError, match="ONE 4x4 window"):
        eng._block_route(plan, Pb, "stage3.0", enc.stage3[0], None, 1, 4, 4)         # a stage below 8 tokens a side
