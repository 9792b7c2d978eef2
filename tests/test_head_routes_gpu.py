"""The head's Conv+BN+SiLU / C3 / SPP units, PatchMerging and the whole head walk of the engine against float64, the way the
engine calls them: Engine._conv_fwd / _c3_fwd / _spp_fwd / _merge_fwd and their backwards on a Plan of their own, on every arm
they can take (the nine-segment and the direct 3x3, the merged and the two-launch C3 input gradient, the eval arm), and
Engine._head_fwd / _head_bwd over the default head and the 3x3-Conv head.  The counterpart of tests/test_block_routes_gpu.py.

Gate.  bf16 routes: |T_gpu - T_A| / |T_A| <= 3 e_emul(T) + 1e-5, where A is the exact unit in float64 on the operands the route
reads and e_emul(T) = |T_B - T_A| / |T_A| with B the same float64 graph with a straight-through bf16 rounding wherever the bf16
route stores a value (tests/head_cases.py; the list is in the docstrings of oracle.ref_torch.conv_bn_silu / c3 / spp /
patch_merging / head_graph).  f32 routes: 2e-3.  The constants are block_cases'; nothing in a gate comes from a kernel.  Gated:
the unit output, din, every parameter gradient, every BatchNorm's updated running statistics; out and din again on the first /
last grid row and column of the units with a 3x3, PatchMerging's dX on each of its four (y & 1, x & 1) parities.  Where no
narrowing point reaches a tensor (PatchMerging's norm.bias gradient; the running statistics of a convolution that reads the
unit's exact input, BatchNorm's statistics being those of the wide conv output) e_emul is 0 and the gate is the floor.  The bf16 SPP's
din and cv1 gradients (upstream of the pooling cascade, where exact bf16 ties route a maximum's gradient to another, equally
valid element) keep test_head_graph_gpu.py's norm-ratio gate instead.

Per case the test also pins the ConvRoute records and whether P["wT12"] holds the unit, the launches by family (an arm launches
its own kernel and none of the launches it replaces), the kernel kind of every statistics GEMM, and that a second backward
without clearing flat_grad doubles every parameter gradient and reproduces din.

The walk runs _head_fwd and _head_bwd on the model's own plan from given features (the oracle's encoder outputs rounded to the run
dtype) and a given gradient at the last unit's output: every unit output, every head parameter gradient, every running
statistic, d f0 / d f1 / d f2 and the gradient in front of each gather_sum_rows, by child parity, against head_graph in float64.

Measured on an MI355X, worst tensor of each group as err / gate (3 e_emul + 1e-5, or 2e-3 on f32; the floor where e_emul is 0);
with e_emul in DESIGN.md section 2, "Head units against float64".  The bf16 SPP's din / cv1 gradients: norm ratios 1.000 - 1.007
(relative L2 0.10 - 0.13 on din and cv1.conv.weight, where their own e_emul is 0.09 - 0.12).

    case                          out (+subsets)   din (+subsets)   conv / red. w    BN / LN w, b     running stats    second backward  
    conv0-B2-8x8-bf16             2.6e-03/7.9e-03  2.5e-03/7.4e-03  1.8e-03/5.4e-03  2.1e-03/6.3e-03  4.9e-08/1.0e-05  2.1e-03/6.3e-03
    conv4-B2-16x16-bf16           2.6e-03/7.8e-03  2.4e-03/7.2e-03  1.8e-03/5.3e-03  1.7e-03/5.0e-03  4.8e-08/1.0e-05  2.4e-03/7.2e-03
    conv3x3_4-B2-16x16-bf16       2.7e-03/8.1e-03  2.4e-03/7.3e-03  1.8e-03/5.3e-03  2.0e-03/6.1e-03  5.1e-08/1.0e-05  2.4e-03/7.3e-03
    conv3x3_4-B1-16x24-bf16       2.7e-03/8.0e-03  2.4e-03/7.3e-03  1.8e-03/5.4e-03  2.0e-03/5.9e-03  5.1e-08/1.0e-05  2.4e-03/7.3e-03
    conv0-B2-8x8-f32              4.7e-07/2.0e-03  3.6e-07/2.0e-03  3.0e-07/2.0e-03  4.8e-07/2.0e-03  5.2e-08/2.0e-03  4.8e-07/2.0e-03
    conv4-B2-16x16-f32            3.4e-07/2.0e-03  2.6e-07/2.0e-03  3.3e-07/2.0e-03  3.0e-07/2.0e-03  5.3e-08/2.0e-03  3.3e-07/2.0e-03
    conv3x3_4-B2-16x16-f32        9.6e-07/2.0e-03  7.2e-07/2.0e-03  4.9e-07/2.0e-03  1.1e-06/2.0e-03  5.4e-08/2.0e-03  1.1e-06/2.0e-03
    conv3x3_4-B1-16x24-f32        9.6e-07/2.0e-03  7.2e-07/2.0e-03  5.3e-07/2.0e-03  9.1e-07/2.0e-03  5.2e-08/2.0e-03  9.1e-07/2.0e-03
    c3_3-B1-24x24-bf16            5.0e-03/1.5e-02  5.6e-03/1.6e-02  4.1e-03/1.2e-02  8.5e-03/2.4e-02  4.3e-05/1.4e-04  8.5e-03/2.4e-02
    c3_3-B2-16x24-bf16            5.0e-03/1.5e-02  5.7e-03/1.6e-02  6.2e-03/1.9e-02  4.4e-03/1.2e-02  4.4e-05/1.4e-04  4.4e-03/1.2e-02
    c3_7-B2-16x16-bf16            4.9e-03/1.5e-02  5.4e-03/1.6e-02  6.2e-03/1.8e-02  7.0e-03/1.8e-02  4.4e-05/1.1e-04  7.0e-03/1.8e-02
    c3_7-B2-16x16-bf16-direct_off 4.8e-03/1.5e-02  5.3e-03/1.6e-02  6.3e-03/1.8e-02  7.2e-03/1.8e-02  4.4e-05/1.4e-04  7.2e-03/1.8e-02
    c3_7-B2-16x16-bf16-merged_off 4.9e-03/1.5e-02  5.5e-03/1.6e-02  6.2e-03/1.8e-02  7.0e-03/1.8e-02  4.4e-05/1.1e-04  7.0e-03/1.8e-02
    c3_7-B2-16x16-f32             7.1e-07/2.0e-03  7.3e-07/2.0e-03  9.7e-07/2.0e-03  1.2e-06/2.0e-03  6.0e-08/2.0e-03  1.2e-06/2.0e-03
    c3_7-B1-16x40-bf16            4.7e-03/1.4e-02  5.2e-03/1.5e-02  6.4e-03/1.9e-02  7.7e-03/2.0e-02  4.1e-05/1.2e-04  7.7e-03/2.0e-02
    c3_7-B1-16x40-bf16-direct_off 5.0e-03/1.5e-02  5.4e-03/1.5e-02  6.3e-03/1.9e-02  6.6e-03/1.7e-02  4.4e-05/1.4e-04  6.6e-03/1.7e-02
    c3_7-B1-16x40-bf16-merged_off 4.7e-03/1.4e-02  5.4e-03/1.5e-02  6.4e-03/1.9e-02  7.7e-03/2.0e-02  4.1e-05/1.2e-04  7.7e-03/2.0e-02
    c3_7-B1-16x40-f32             7.1e-07/2.0e-03  7.3e-07/2.0e-03  1.0e-06/2.0e-03  1.1e-06/2.0e-03  5.5e-08/2.0e-03  1.1e-06/2.0e-03
    spp-B1-16x24-bf16             1.1e-02/3.3e-02                   1.3e-02/3.9e-02  1.0e-02/3.1e-02  6.7e-04/2.0e-03  1.3e-02/3.9e-02
    spp-B2-8x8-bf16               1.1e-02/3.2e-02                   1.3e-02/3.6e-02  1.1e-02/3.3e-02  9.1e-04/2.7e-03  1.3e-02/3.6e-02
    spp-B1-16x24-f32              1.6e-06/2.0e-03  1.2e-06/2.0e-03  1.8e-06/2.0e-03  1.9e-06/2.0e-03  1.2e-07/2.0e-03  1.9e-06/2.0e-03
    spp-B2-8x8-f32                1.5e-06/2.0e-03  1.4e-06/2.0e-03  1.6e-06/2.0e-03  2.1e-06/2.0e-03  1.6e-07/2.0e-03  2.1e-06/2.0e-03
    pmerging1-B2-32x32-bf16       2.3e-03/7.0e-03  2.4e-03/7.1e-03  1.7e-03/5.0e-03  1.6e-03/4.8e-03                   2.4e-03/7.1e-03
    pmerging2-B2-16x16-bf16       2.4e-03/7.1e-03  2.3e-03/7.0e-03  1.7e-03/5.0e-03  1.6e-03/4.7e-03                   2.3e-03/7.0e-03
    pmerging2-B1-16x24-bf16       2.4e-03/7.1e-03  2.3e-03/7.0e-03  1.7e-03/5.0e-03  1.6e-03/4.9e-03                   1.6e-03/4.9e-03
    pmerging1-B2-32x32-f32        5.0e-07/2.0e-03  3.6e-07/2.0e-03  3.0e-07/2.0e-03  5.0e-07/2.0e-03                   5.1e-07/2.0e-03
    pmerging2-B2-16x16-f32        7.0e-07/2.0e-03  5.1e-07/2.0e-03  2.2e-07/2.0e-03  7.0e-07/2.0e-03                   7.0e-07/2.0e-03
    pmerging2-B1-16x24-f32        7.0e-07/2.0e-03  5.1e-07/2.0e-03  2.0e-07/2.0e-03  7.1e-07/2.0e-03                   7.0e-07/2.0e-03
    conv0-B2-8x8-bf16-eval        1.7e-03/5.1e-03
    c3_7-B2-16x16-bf16-eval       2.5e-03/7.6e-03
    conv0-B2-8x8-f32-eval         4.8e-07/2.0e-03
    c3_7-B2-16x16-f32-eval        4.8e-07/2.0e-03
    walk-base-bf16                1.3e-02/4.0e-02  2.6e-02/7.6e-02  3.0e-02/9.0e-02  2.1e-02/5.6e-02  5.2e-05/1.3e-04
    walk-base-f32                 3.9e-06/2.0e-03  5.7e-06/2.0e-03  6.5e-06/2.0e-03  6.8e-06/2.0e-03  6.1e-08/2.0e-03
    walk-conv3-bf16               1.3e-02/4.0e-02  1.5e-02/4.3e-02  3.1e-02/8.8e-02  8.0e-03/2.2e-02  2.3e-05/5.9e-05
    walk-conv3-f32                4.0e-06/2.0e-03  5.7e-06/2.0e-03  6.3e-06/2.0e-03  6.5e-06/2.0e-03  6.1e-08/2.0e-03
"""
import importlib
import statistics
from collections import Counter

import pytest
import torch

import gemm_cases as G
import head_cases as HC

pytestmark = pytest.mark.gpu
BF, F32 = HC.BF, HC.F32
PKG = HC.PKG
PREP_SWITCHES = {"use_merged_c3_din": True}          # read when the parameter layouts are first prepared
LIVE_SWITCHES = {"use_direct_conv3": True}
NT = ("gemm_nt3_kernel", "gemm_nt_kernel", "gemm_as_kernel", "gemm_bs_kernel")
TN = ("gemm_tn3_kernel", "gemm_tn_kernel", "gemm_tn2_kernel")
SINGLE = ("conv3_c64_kernel", "conv3_c64_wgrad_kernel", "col_stats_kernel", "bn_finalize_kernel", "bn_affine_kernel",
          "bn_silu_fwd_kernel", "bn_silu_bwd_reduce_kernel", "bn_silu_bwd_apply_kernel", "maxpool5_fwd_kernel",
          "maxpool5_bwd_kernel", "gather_sum_rows_kernel")

_engines = {}
_gpu_error = []      # a HIP error in one case: the cases after it launch nothing more


def engine_for(dev, head, dtype, prep):
    """(model, engine, plan, P, state dict) of a freshly built S=128 model with this head and the given prepare-time switches,
    after one training forward (which casts and lays out the weights)."""
    from oracle import ref_torch as R
    key = (head, dtype, tuple(sorted(prep.items())))
    if key not in _engines:
        model, sd = HC.build_model(head)
        model = model.to(dev)
        model.compute_dtype = dtype
        model.train()
        eng = model._get_engine()
        for k, v in prep.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
        x_rgb, x_ir = R.synthetic_inputs(HC.B_WALK, HC.S_MODEL, seed=HC.SEED_FEATS)
        model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
        plan = next(p for p in eng.plans.values() if p.dt == dtype and p.training and p.B == HC.B_WALK and p.S == HC.S_MODEL)
        _engines[key] = (model, eng, plan, eng._prep_for(dtype), sd)
    return _engines[key]


def reset_running(eng, sd, prefix):
    """the BatchNorm running statistics under `prefix` back to the state dict's (every forward moves them)"""
    for n, b in eng.buffers.items():
        if n.startswith(prefix) and n.endswith(("running_mean", "running_var")):
            b.copy_(sd[n])


def family(name: str):
    base = name.split("<")[0]
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


# ------------------------------------------------------------------ what an arm launches
def convs_of(kind, c1, c2, ksize, direct):
    """[(tag suffix, K, Cout, k, direct)] of the Conv2d+BN+SiLU launches of a unit, in forward order"""
    if kind == "Conv":
        return [("", c1 * ksize * ksize, c2, ksize, False)]
    if kind == "C3":
        c_ = c2 // 2
        return [(".cv1", c1, c_, 1, False), (".m1", c_, c_, 1, False), (".m2", 9 * c_, c_, 3, direct), (".cv2", c1, c_, 1, False),
                (".cv3", 2 * c_, c2, 1, False)]
    return [(".cv1", c1, c1 // 2, 1, False), (".cv2", 2 * c1, c2, 1, False)]


def stats_kernel(dtype, M, N, K):
    """The kernel of a forward GEMM with the BatchNorm statistics epilogue, as csrc/routes.h (nt_route) chooses it for the K-segments
    the head passes (whole 64-column steps): the thin pipelined kernel for a bf16 output of at most 64 columns from M >= 256 rows and
    K >= 192; the B-stationary statistics kernel for a contraction row of at most 384 bytes; else the tiled kernel."""
    if dtype == BF and N <= 64 and K >= 192 and K % 64 == 0 and M >= 256:
        return G.nt3(16, False, 2)
    kb = K * (2 if dtype == BF else 4)
    if kb % 128 == 0 and kb <= 384:
        return G.bs(dtype, True, -1, False)
    return G.ntk(dtype, -1)


def expected_unit(kind, c1, c2, ksize, dtype, M, training, direct, merged):
    """(forward families, backward families, forward NT kernels in order) of one head unit"""
    convs = convs_of(kind, c1, c2, ksize, direct)
    n, nd = len(convs), sum(1 for c in convs if c[4])
    f, b = Counter(), Counter()
    f["bn_finalize_kernel"] = n
    if not training:
        f["bn_affine_kernel"] = n
        f["gemm_nt"] = n
        if kind == "SPP":
            f["maxpool5_fwd_kernel"] = 3
        return dict(f), {}, None
    f["bn_silu_fwd_kernel"] = n
    f["gemm_nt"] = n - nd
    b["bn_silu_bwd_reduce_kernel"] = b["bn_silu_bwd_apply_kernel"] = n
    b["gemm_tn"] = n - nd
    if nd:                      # the direct 3x3: its own forward, statistics, input-gradient (the same kernel, flipped) and weight-gradient kernels
        f["conv3_c64_kernel"] = f["col_stats_kernel"] = nd
        b["conv3_c64_kernel"] = b["conv3_c64_wgrad_kernel"] = nd
    if kind == "Conv":
        b["gemm_nt"] = 1
    elif kind == "C3":          # dcat, d(m.0.cv2 input) unless direct, d(m.0.cv1 input), d(input): one merged GEMM or two
        b["gemm_nt"] = 1 + (0 if direct else 1) + 1 + (1 if merged else 2)
    else:
        f["maxpool5_fwd_kernel"] = b["maxpool5_bwd_kernel"] = 3
        b["gemm_nt"] = 2
    kinds = [stats_kernel(dtype, M, cout, K) for (_, K, cout, _, d) in convs if not d]
    return dict(f), dict(b), kinds


def expected_case(case):
    if case.kind == "merge":
        return {"gemm_nt": 1, "ln_fwd": 1}, {"ln_bwd": 1, "gemm_tn": 1, "gemm_nt": 4}, None
    u = HC.spec(case)
    return expected_unit(u.kind, u.c1, u.c2, u.ksize, case.dtype, case.B * case.H * case.W, case.training, case.direct, case.merged)


# ------------------------------------------------------------------ one unit as the engine calls it
def unit_fwd(eng, ops, plan, P, case, x):
    B, H, W = case.B, case.H, case.W
    M = B * H * W
    if case.kind == "merge":
        return eng._merge_fwd(plan, P, f"pmerging{case.row}", x, B, H, W, HC.MERGES[case.row])
    u = HC.spec(case)
    tag, pname = f"h{case.row}", f"detect.{case.row}."
    if u.kind == "Conv":            # (_head_fwd: a 1x1 on one dense tensor is a plain segment, a 3x3 is nine shifted ones)
        if u.ksize == 1:
            segs, spatial = [ops.SegSpec(x)], None
        else:
            segs, spatial = [ops.SegSpec(x, u.c1, 0, dy, dx, 1, 0, H, W) for (dy, dx) in ops.TAPS3], (H, W)
        return eng._conv_fwd(plan, P, tag, pname, segs, spatial, M, u.c1 * u.ksize ** 2, u.c2, u.ksize)
    if u.kind == "C3":
        return eng._c3_fwd(plan, P, tag, pname, [ops.SegSpec(x, u.c1, 0, 0, 0, 1, 0, H, W)], (H, W), M, u.c1, u.c2)
    return eng._spp_fwd(plan, P, tag, pname, [ops.SegSpec(x)], (H, W), M, u.c1, u.c2, B)


def unit_bwd(eng, ops, plan, P, case, dout):
    B, H, W = case.B, case.H, case.W
    M = B * H * W
    if case.kind == "merge":
        dX = torch.empty(M, HC.MERGES[case.row], device=dout.device, dtype=dout.dtype)
        eng._merge_bwd(plan, P, f"pmerging{case.row}", dout, dX)
        return dX
    u = HC.spec(case)
    tag, pname = f"h{case.row}", f"detect.{case.row}."
    if u.kind == "Conv":            # (the Conv arm of _head_bwd)
        dz = eng._conv_bwd(plan, tag, dout, u.c2, 0)
        din = plan.buf(tag + ".din", (M, u.c1))
        w_ = P["wT"][pname + "conv.weight"]
        if u.ksize == 1:
            ops.gemm_nt([ops.SegSpec(dz)], w_, din, M, u.c1, u.c2)
        else:
            segs = [ops.SegSpec(dz, u.c2, 0, -dy_, -dx_, 1, 0, H, W) for (dy_, dx_) in ops.TAPS3]
            ops.gemm_nt(segs, w_, din, M, u.c1, 9 * u.c2, spatial=(H, W))
        return din
    if u.kind == "C3":
        return eng._c3_bwd(plan, P, tag, dout, u.c2, 0)
    return eng._spp_bwd(plan, P, tag, dout, u.c2, 0)


class Measure:
    """prints every figure, collects what is out of its gate"""

    def __init__(self, cid, dtype, ref):
        self.cid, self.dtype, self.ref, self.bad = cid, dtype, ref, []

    def __call__(self, what, t, name, scale=1.0):
        a = self.ref.A[name] * scale
        err, lim = HC.rel_l2(t.reshape(a.shape), a), HC.gate(self.dtype, self.ref, name)
        print(f"HEADROUTE {self.cid} {what} {name} err {err:.3e} gate {lim:.3e} e_emul {self.ref.e_emul.get(name, float('nan')):.3e}")
        if not err <= lim:
            self.bad.append(f"{what} {name}: {err:.3e} > {lim:.3e}")

    def ratios(self, what, got, names, scale=1.0):
        """test_head_graph_gpu.py's gate on gradients upstream of the bf16 pooling cascade: the ratio of norms"""
        rs = []
        for name in names:
            a = self.ref.A[name] * scale
            r = float(got[name].double().norm()) / float(a.norm())
            err = HC.rel_l2(got[name].reshape(a.shape), a)
            print(f"HEADROUTE {self.cid} {what} {name} err {err:.3e} norm-ratio {r:.3f} e_emul {self.ref.e_emul.get(name, float('nan')):.3e}")
            rs.append(r)
            if not HC.RATIO_EACH[0] <= r <= HC.RATIO_EACH[1]:
                self.bad.append(f"{what} {name}: norm ratio {r:.3f}")
        med = statistics.median(rs)
        if not HC.RATIO_MEDIAN[0] <= med <= HC.RATIO_MEDIAN[1]:
            self.bad.append(f"{what}: median norm ratio {med:.3f}")


@pytest.mark.parametrize("case", HC.CASES, ids=[c.id for c in HC.CASES])
def test_head_route(dev, case):
    if _gpu_error:
        pytest.fail(f"not run: an earlier case ended in a GPU error ({_gpu_error[0]})")
    ops = importlib.import_module(PKG + ".ops")
    E = importlib.import_module(PKG + ".engine")
    prep = {k: dict(case.prep).get(k, v) for k, v in PREP_SWITCHES.items()}
    live = {k: dict(case.live).get(k, v) for k, v in LIVE_SWITCHES.items()}
    try:
        model, eng, _, P, sd = engine_for(dev, case.head, case.dtype, prep)
    except RuntimeError as e:
        _gpu_error.append(f"{case.id}: {e}")
        raise
    ref = HC.reference(case)
    HC.check_reference(case, ref)
    merge = case.kind == "merge"
    pre = f"{HC.E}pmerging{case.row}." if merge else f"detect.{case.row}."
    tag = f"pmerging{case.row}" if merge else f"h{case.row}"
    okey, dkey = ("y", "dX") if merge else ("out", "din")
    pnames = [n for n in eng.params if n.startswith(pre)]
    snames = [n for n in eng.buffers if n.startswith(pre) and n.endswith(("running_mean", "running_var"))]
    x = HC.unit_input(case).to(case.dtype).to(dev)
    dout = HC.grad_output(case).to(case.dtype).to(dev)
    plan = E.Plan(case.B, (4 * case.H, 4 * case.W), case.dtype, case.training, dev)
    out, got, twice, bwd_names = {}, {}, {}, []
    assert all(getattr(eng, k) is v for k, v in LIVE_SWITCHES.items())
    try:
        for k, v in live.items():
            setattr(eng, k, v)
        reset_running(eng, sd, pre)
        ops.zero_(plan.zpool("f"))
        fwd_names = G.launched_kernels(lambda: out.__setitem__("y", unit_fwd(eng, ops, plan, P, case, x)))
        got[okey] = out["y"].clone()
        got.update({n[len(pre):]: eng.buffers[n].clone() for n in snames if case.training})
        if case.training:
            eng.flat_grad.zero_()
            ops.zero_(plan.zpool("b"))
            bwd_names = G.launched_kernels(lambda: out.__setitem__("d", unit_bwd(eng, ops, plan, P, case, dout)))
            got[dkey] = out["d"].clone()
            got.update({n[len(pre):]: eng.g[n].clone() for n in pnames})
            ops.zero_(plan.zpool("b"))                                   # flat_grad NOT cleared: every parameter gradient doubles
            twice[dkey] = unit_bwd(eng, ops, plan, P, case, dout).clone()
            twice.update({n[len(pre):]: eng.g[n].clone() for n in pnames})
        torch.cuda.synchronize()
    except RuntimeError as e:
        _gpu_error.append(f"{case.id}: {e}")
        raise
    finally:
        for k, v in LIVE_SWITCHES.items():
            setattr(eng, k, v)
    eng.flat_grad.zero_()

    # ---- the route records and the launches (collected: every figure below is printed before anything is asserted)
    m = Measure(case.id, case.dtype, ref)
    bad = m.bad
    if not merge:
        u = HC.spec(case)
        for sfx, K, cout, k, direct in convs_of(u.kind, u.c1, u.c2, u.ksize, case.direct):
            r = plan.saved[tag + sfx]
            if (r.K, r.Cout, r.k, r.direct, r.M) != (K, cout, k, direct, case.B * case.H * case.W):
                bad.append(f"ConvRoute {tag + sfx}: {(r.K, r.Cout, r.k, r.direct, r.M)}, the case was written for {(K, cout, k, direct)}")
        if u.kind == "C3" and case.training and (pre in P["wT12"]) != case.merged:
            bad.append(f"P['wT12'] {'holds' if pre in P['wT12'] else 'lacks'} {pre}")
    want_f, want_b, kinds = expected_case(case)
    for what, names, want in (("forward", fwd_names, want_f), ("backward", bwd_names, want_b)):
        if families(names) != want:
            bad.append(f"{what} launched {families(names)}, the arm is {want} (all kernels: {names})")
    if kinds is not None:
        nt = [n for n in fwd_names if n.split("<")[0] in NT]
        if nt != kinds:
            bad.append(f"statistics GEMMs ran {nt}, the arm is {kinds}")

    # ---- values
    sub = HC.subsets(case)

    def rows(t, name):
        return t if "[" not in name else t[sub[name[name.index("[") + 1:-1]][1].to(t.device)]
    loose = [n for n in ref.A if HC.ratio_gated(case, n)]
    for name in ref.A:
        if name not in loose:
            m("once", rows(got[name.split("[")[0]], name), name)
    if loose:
        m.ratios("once", got, loose)
    for name in ref.A:
        base = name.split("[")[0]
        if base in twice and name not in loose:
            m("twice", rows(twice[base], name), name, 1.0 if base == dkey else 2.0)
    if loose and twice:
        m.ratios("twice", {n: twice[n] * (1.0 if n == dkey else 0.5) for n in loose}, loose)
    assert not bad, f"{case.id}: " + "; ".join(bad)


@pytest.mark.parametrize("head,dtype", HC.WALKS, ids=[f"{h}-{'bf16' if d == BF else 'f32'}" for h, d in HC.WALKS])
def test_head_walk(dev, head, dtype):
    """_head_fwd / _head_bwd over the whole head: what no unit contains - the up-sampled / concatenated A operand, the column-slice
    hand-over through gout, gather_sum_rows at the engine's own ld / d_off."""
    if _gpu_error:
        pytest.fail(f"not run: an earlier case ended in a GPU error ({_gpu_error[0]})")
    ops = importlib.import_module(PKG + ".ops")
    HG = importlib.import_module(PKG + ".headgraph")
    cid = f"walk-{head}-{'bf16' if dtype == BF else 'f32'}"
    try:
        model, eng, plan, P, sd = engine_for(dev, head, dtype, dict(PREP_SWITCHES))
    except RuntimeError as e:
        _gpu_error.append(f"{cid}: {e}")
        raise
    ref = HC.walk_reference(head, dtype)
    HC.check_reference(cid, ref, dtype)
    units = eng.head.units
    assert [(u.k, u.kind) for u in units] == HC.walk_units(head)
    last = units[-1]
    gbuf = HC.walk_grad(head).to(dtype).to(dev)
    got = {}
    try:
        for j, f in enumerate(HC.walk_features(head)):
            plan.bufs[f"f{j}"].copy_(HC.tok(f).to(dtype))
        reset_running(eng, sd, "detect.")
        ops.zero_(plan.zpool("f"))
        fwd_names = G.launched_kernels(lambda: eng._head_fwd(plan, P))
        for u in units:
            got[f"h{u.k}.out"] = plan.bufs[u.out_name].clone()
        eng.flat_grad.zero_()
        ops.zero_(plan.zpool("b"))
        res = {}
        bwd_names = G.launched_kernels(lambda: res.update(eng._head_bwd(plan, P, {last.ref: (gbuf, last.c2, 0)}, {})))
        for j, c in enumerate(HG.ENC_C):
            buf, ld, off = res[HG.Ref("enc", j)]
            assert buf.shape[-1] == ld
            got[f"df{j}"] = buf[:, off: off + c].clone()
        for n in ref.A:
            if n in eng.params:
                got[n] = eng.g[n].clone()
            elif n in eng.buffers:
                got[n] = eng.buffers[n].clone()
        ups = HC.walk_upsampled(head)
        for k, c in ups:
            got[f"h{k}.din"] = plan.bufs[f"h{k}.din"].clone()
        torch.cuda.synchronize()
    except RuntimeError as e:
        _gpu_error.append(f"{cid}: {e}")
        raise
    eng.flat_grad.zero_()

    m = Measure(cid, dtype, ref)
    want_f, want_b = Counter(), Counter({"gather_sum_rows_kernel": len(ups)})
    t = HC.S_MODEL // 4
    for u in units:
        bf7 = dtype == BF and u.kind == "C3" and u.c2 == 128
        f, b, _ = expected_unit(u.kind, u.c1, u.c2, u.ksize, dtype, HC.B_WALK * (t >> u.level) ** 2, True, bf7, bf7)
        want_f.update(f), want_b.update(b)
    for what, names, want in (("forward", fwd_names, dict(want_f)), ("backward", bwd_names, dict(want_b))):
        if families(names) != want:
            m.bad.append(f"{what} launched {families(names)}, the walk is {want} (all kernels: {names})")
    par = {k: (c, HC.parity_masks(HC.B_WALK, t >> eng.head.by_row[k].level, t >> eng.head.by_row[k].level)) for k, c in ups}
    for name in ref.A:
        base = name.split("[")[0]
        v = got[base]
        if "[" in name:
            c, masks = par[int(base[1:base.index(".")])]
            v = v[masks[name[name.index("[") + 1:-1]].to(v.device)][:, :c]
        m("walk", v, name)
    assert not m.bad, f"{cid}: " + "; ".join(m.bad)
