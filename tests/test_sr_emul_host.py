"""The conditions tests/test_sr_routes_gpu.py puts on its own float64 references, checked on the CPU (no GPU needed): for every
case and every gated tensor |T_A| > 0 and 0 < e_emul(T) <= 5e-2 (e_emul == 0 where no store point reaches the tensor;
tests/sr_cases.py), so that the bf16 gate 3 e_emul + 1e-5 is neither vacuous nor loose; that the factored oracle without a store
is, bit for bit, the statement it was before it took one; that the store points are the documented ones; and that the case and
kernel tables are complete."""
import importlib
import os

import pytest
import torch
import torch.nn.functional as F

import block_cases as BC
import sr_cases as SC

BF, F32 = SC.BF, SC.F32
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), SC.PKG, "libsodt_hip.so")


# ------------------------------------------------------------------ the oracle, as it was stated before it was factored
def _plain_decoder(sd, pfx, x, low, factor=2):
    lo = F.relu(F.conv2d(low, sd[pfx + "conv1.weight"]))
    xx = F.relu(F.conv2d(x, sd[pfx + "conv2.weight"]))
    size = [d * (factor // 2) for d in lo.shape[2:]]
    xx = F.interpolate(xx, size=size, mode="bilinear", align_corners=True)
    if factor > 1:
        lo = F.interpolate(lo, size=size, mode="bilinear", align_corners=True)
    z = torch.cat((xx, lo), 1)
    z = F.relu(F.conv2d(z, sd[pfx + "last_conv.0.weight"], None, padding=1))
    z = F.relu(F.conv2d(z, sd[pfx + "last_conv.2.weight"], None, padding=1))
    return F.conv2d(z, sd[pfx + "last_conv.4.weight"], sd[pfx + "last_conv.4.bias"])


def _plain_edsr(sd, pfx, x):
    def conv(name, t):
        return F.conv2d(t, sd[pfx + name + ".weight"], sd[pfx + name + ".bias"], padding=1)
    h = conv("head.0", x)
    r = h
    i = 0
    while f"{pfx}body.{i}.body.0.weight" in sd:
        r = r + conv(f"body.{i}.body.2", F.relu(conv(f"body.{i}.body.0", r)))
        i += 1
    r = conv(f"body.{i}", r) + h
    j = 0
    while f"{pfx}tail.0.{j}.weight" in sd:
        r = F.pixel_shuffle(conv(f"tail.0.{j}", r), 2)
        j += 2
    return conv("tail.1", r)


def _run(fn, dtype, **kw):
    """y, the input gradients and every parameter gradient of fn(sd, low, x) on fresh leaves"""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in SC.params(4).items()}
    B, H, W = 1, 6, 10
    low = SC._randn_seeded(1, B, SC.C1, H, W).to(dtype).requires_grad_(True)
    x = SC._randn_seeded(2, B, SC.C2, H // 2, W // 2).to(dtype).requires_grad_(True)
    y = fn(sd, low, x, **kw)
    y.backward(SC._randn_seeded(3, *y.shape).to(dtype))
    out = {"y": y.detach(), "d_low": low.grad, "d_x": x.grad}
    out.update({k: v.grad for k, v in sd.items() if v.grad is not None})
    return out


def _identity(t, name):
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_factored_oracle_without_a_store_is_the_plain_statement(dtype):
    """sr_decoder / edsr / deeplab_sr with store=None against the un-factored statements above: the same bits, forward and backward"""
    from oracle import ref_torch as R
    pairs = {
        "decoder": (lambda sd, low, x: R.sr_decoder(sd, SC.DEC, x, low, 2), lambda sd, low, x: _plain_decoder(sd, SC.DEC, x, low, 2)),
        "edsr": (lambda sd, low, x: R.edsr(sd, SC.ED, low[:, :64] + 0 * x.sum()),
                 lambda sd, low, x: _plain_edsr(sd, SC.ED, low[:, :64] + 0 * x.sum())),
        "deeplab": (lambda sd, low, x: R.deeplab_sr(sd, "", low, x, 2),
                    lambda sd, low, x: _plain_edsr(sd, SC.ED, _plain_decoder(sd, SC.DEC, x, low, 2))),
    }
    for name, (new, old) in pairs.items():
        a, b = _run(new, dtype), _run(old, dtype)
        assert set(a) == set(b) and len(a) > 5, name
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)


def test_store_hook_identity_and_narrow():
    """an explicit identity store is the same graph (the Upsampler stage then runs as its four planes: equal to rounding, 1e-12
    in float64); the narrowing store gives other values"""
    from oracle import ref_torch as R
    fn = lambda sd, low, x, **kw: R.deeplab_sr(sd, "", low, x, 2, **kw)
    a, b, c = _run(fn, torch.float64), _run(fn, torch.float64, store=_identity), _run(fn, torch.float64, store=SC.narrow)
    assert set(a) == set(b) == set(c)
    for k in a:
        assert SC.rel_l2(b[k], a[k]) <= 1e-12, k
        if k != SC.ED + "tail.1.bias":           # (the column sum of the given gradient, which is exact in bf16)
            assert 1e-4 < SC.rel_l2(c[k], a[k]) < 0.5, k


def test_store_points_are_the_documented_ones():
    from oracle import ref_torch as R
    seen = []

    def rec(t, name):
        seen.append(name)
        return t
    _run(lambda sd, low, x: R.deeplab_sr(sd, "", low, x, 2, store=rec), torch.float64)
    D, E = SC.DEC, SC.ED
    want = [D + n for n in ("low", "a", "x", "xr", "cat.x", "d1", "d2", "d3")] + [E + "x", E + "h", E + "body.in"]
    for i in range(SC.DEPTH):
        want += [f"{E}body.{i}.u", f"{E}body.{i}.r"]
    want += [E + "rb"]
    for j in range(3):
        want += [f"{E}tail.0.{2 * j}.acc{p}" for p in (3, 2, 1)] + [f"{E}p{j}"]
    want += [E + "y"]
    assert seen == want, seen


def test_narrow_grad_store_of_the_float32_output():
    """store_of: the closing convolution's "y" keeps its value and narrows its gradient where the route writes the float32 tensor
    itself, and narrows both ways above NCHW_DIRECT_MAX_CH"""
    v = (torch.arange(7, dtype=torch.float64) / 7 + 1e-3).requires_grad_(True)
    for ch, same in ((3, True), (4, True), (8, False), (12, False)):
        st = SC.store_of(SC._c("close", 1, 10, 36, BF, ch))
        y = st(v, SC.ED + "y")
        assert torch.equal(y.detach(), v.detach()) == same
        g, = torch.autograd.grad(y, v, v.detach())
        assert torch.equal(g, v.detach().bfloat16().double()) and not torch.equal(g, v.detach())
        assert not torch.equal(st(v, SC.ED + "h").detach(), v.detach())


REF_CASES = list(SC.CASES)


@pytest.mark.parametrize("case", REF_CASES, ids=[c.id for c in REF_CASES])
def test_reference_conditions(case):
    ref = SC.reference(case)
    SC.check_reference(case, ref)
    pre, names = SC.param_names(case)
    assert names and all(pre + n in SC.params(case.ch) for n in names)
    maps = {"dec_entry": ("cat.x", "cat.a", "d_low", "d_x"), "dec_entry_engine": ("cat.x", "cat.a", "d_low", "d_x"),
            "dec_tail": ("out", "g.cu", "g.a")}.get(case.kind, ("out", "din"))
    want = set(maps) | set(names)
    if case.kind in SC.HAS_3X3:
        want |= {f"{k}[{s}]" for k in maps for s in ("top", "bottom", "left", "right")}
    if case.kind == "up":
        want |= {f"{k}[p{a}{b}]" for k in ("out", "din", "tail.0.0.weight", "tail.0.0.bias") for a in (0, 1) for b in (0, 1)}
    assert set(ref.A) == want and (set(ref.e_emul) == want if case.dtype == BF else not ref.e_emul)
    if case.kind == "walk":
        assert len(names) == 2 * (1 + 2 * SC.DEPTH + 1 + 3 + 1)
        assert ref.A["out"].shape == (case.B * 64 * case.H * case.W, 4) and ref.A["din"].shape == (case.B * case.H * case.W, 64)
    for k, v in ref.e_emul.items():
        print(f"EMUL {case.id} {k} e_emul {v:.3e} gate {SC.MARGIN * v + SC.FLOOR:.3e}")


def test_untouched_tensors_are_named_by_reasoning():
    """every name of UNTOUCHED is a parameter of its unit; the closing output is untouched exactly where the route writes it itself"""
    for kind, names in SC.UNTOUCHED.items():
        assert kind in SC.KINDS
        have = SC.param_names(SC._c(kind, 1, 8, 12, BF))[1]
        assert all(n in have for n in names), kind
    assert [SC.untouched(SC._c("close", 1, 10, 36, BF, ch), "out[top]") for ch in (3, 4, 8, 12)] == [True, True, False, False]
    assert not SC.untouched(SC._c("walk", 1, 7, 6, BF), "out")


def test_subsets_cover_what_they_name():
    for c in SC.CASES:
        s = SC.out_scale(c)
        b = SC.border_masks(c.B, c.H, c.W)
        assert int(b["top"].sum()) == int(b["bottom"].sum()) == c.B * c.W and int(b["left"].sum()) == int(b["right"].sum()) == c.B * c.H
        assert bool(b["top"][: c.W].all()) and bool(b["right"][c.W - 1:: c.W].all()) and bool(b["bottom"][-c.W:].all())
        names = SC.subset_names(c, SC.reference(c).A)
        assert bool(names) == (c.kind in SC.HAS_3X3)
        if c.kind in SC.HAS_3X3:
            A = SC.reference(c).A
            assert A["out[top]"].shape[0] == c.B * s * c.W and A["out[left]"].shape[0] == c.B * s * c.H
        if c.kind == "up":
            p = SC.parity_masks(c.B, 2 * c.H, 2 * c.W)
            tot = sum(m.long() for m in p.values())
            assert sorted(p) == ["p00", "p01", "p10", "p11"] and int(tot.min()) == 1 == int(tot.max())
            A = SC.reference(c).A
            assert A["out[p10]"].shape == (c.B * c.H * c.W, 64) and A["tail.0.0.weight[p10]"].shape == (64, 64, 3, 3)
            assert torch.equal(A["tail.0.0.bias[p11]"], A["tail.0.0.bias"][3::4])
            # the plane runs add up to the whole input gradient
            assert SC.rel_l2(sum(A[f"din[{k}]"] for k in p), A["din"]) < 1e-12


def test_constants_are_block_cases():
    assert (SC.MARGIN, SC.FLOOR, SC.F32_GATE, SC.E_EMUL_MAX) == (BC.MARGIN, BC.FLOOR, BC.F32_GATE, BC.E_EMUL_MAX) == (3.0, 1e-5, 2e-3, 5e-2)
    assert SC.narrow is BC.narrow and SC.rel_l2 is BC.rel_l2


def test_case_matrix():
    ids = [c.id for c in SC.CASES]
    assert len(set(ids)) == len(ids) == 46
    have = {(c.kind, c.B, c.H, c.W, c.dtype, c.ch) for c in SC.CASES}
    grids3 = ((2, 7, 6), (1, 10, 36), (1, 18, 34))
    for dt in (BF, F32):
        for g in ((2, 8, 12), (1, 6, 10)):
            assert ("dec_entry", *g, dt, 4) in have and ("dec_tail", *g, dt, 4) in have
        assert ("dec_entry_engine", 2, 8, 12, dt, 4) in have
        for kind in ("head", "resblock", "body_close"):
            assert all((kind, *g, dt, 4) in have for g in grids3)
        assert all(("up", *g, dt, 4) in have for g in grids3[:2])
        assert all(("close", *g, dt, ch) in have for g in (grids3[0], grids3[2]) for ch in (3, 4))
        assert all(("walk", *g, dt, 4) in have for g in ((1, 7, 6), (2, 10, 12)))
    assert ("close", 1, 10, 36, BF, 8) in have and ("close", 1, 10, 36, BF, 12) in have
    assert {c.kind for c in SC.CASES} == set(SC.KINDS) and {c.dtype for c in SC.CASES} == {BF, F32}
    # the whole Decoder and EDSR(depth 16) are not cases: their own bf16 noise is above the cap
    assert SC.DEPTH == 2 and not any(c.kind in ("decoder", "edsr16") for c in SC.CASES)


def test_kernel_table():
    """every case has its launches stated; every arm of the branch appears among the cases; absent families are absent"""
    arms = set()
    for c in SC.CASES:
        f, b = SC.expected(c)
        assert f and b and all(v > 0 for v in list(f.values()) + list(b.values())), c.id
        arms |= {(c.dtype, k) for k in list(f) + list(b)}
        if c.dtype == F32:
            assert not any(k.startswith("conv3_") for k in list(f) + list(b)), c.id
    for k in ("conv3_c64_kernel", "conv3_c64_wgrad_kernel", "conv3_c64_wgrad_reduce_kernel", "conv3_n8_fwd_kernel", "conv3_n8_dgrad_kernel",
              "conv3_n8_wgrad_kernel", "nchw_from_rows_kernel", "rows_from_nchw_kernel", "add_rows_kernel", "gemm_nt", "gemm_tn",
              "bilinear_up2_fwd_kernel", "bilinear_up2_bwd_kernel"):
        assert (BF, k) in arms, k
    for k in ("pixel_shuffle2_kernel", "gemm_nt", "gemm_tn", "add_rows_kernel", "nchw_from_rows_kernel", "rows_from_nchw_kernel",
              "bilinear_up2_fwd_kernel", "bilinear_up2_bwd_kernel"):
        assert (F32, k) in arms, k
    E = SC.EXPECTED
    c64 = "conv3_c64_kernel"
    # a 64 -> 64 3x3 on bf16: the direct kernels each way, no GEMM
    assert E[("body_close", BF, None)] == ({c64: 1}, {c64: 1, "conv3_c64_wgrad_kernel": 1, "conv3_c64_wgrad_reduce_kernel": 1})
    # an Upsampler stage: four launches each way, four weight-gradient launches, no shuffle
    assert E[("up", BF, None)][0] == {c64: 4} and E[("up", BF, None)][1]["conv3_c64_wgrad_kernel"] == 4
    assert "pixel_shuffle2_kernel" not in E[("up", BF, None)][0] and E[("up", F32, None)][0]["pixel_shuffle2_kernel"] == 1
    # the closing convolution: its own kernels up to 8 channels, the layout kernels from 8, the GEMMs + add_rows at 12
    for ch in (3, 4):
        f, b = SC.expected(SC._c("close", 2, 7, 6, BF, ch))
        assert f == {"conv3_n8_fwd_kernel": 1} and "rows_from_nchw_kernel" not in b and "gemm_nt" not in b
    f, b = SC.expected(SC._c("close", 1, 10, 36, BF, 8))
    assert f == {"conv3_n8_fwd_kernel": 1, "nchw_from_rows_kernel": 1} and b["rows_from_nchw_kernel"] == 1 and "gemm_tn" not in b
    f, b = SC.expected(SC._c("close", 1, 10, 36, BF, 12))
    assert f == {"gemm_nt": 1, "nchw_from_rows_kernel": 1} and b["add_rows_kernel"] == 2 and b["gemm_tn"] == 1
    # the Decoder: GEMMs and exactly one resize each way
    f, b = SC.expected(SC._c("dec_entry", 2, 8, 12, BF))
    assert f == {"gemm_nt": 2, "bilinear_up2_fwd_kernel": 1} and b == {"gemm_nt": 2, "gemm_tn": 2, "bilinear_up2_bwd_kernel": 1}
    f, b = SC.expected(SC._c("walk", 1, 7, 6, BF))
    assert f == {c64: 18, "conv3_n8_fwd_kernel": 1} and b["add_rows_kernel"] == 1 and "gemm_nt" not in b
    f, b = SC.expected(SC._c("walk", 1, 7, 6, F32))
    assert f == {"gemm_nt": 10, "pixel_shuffle2_kernel": 3, "nchw_from_rows_kernel": 1}
    assert b == {"gemm_nt": 10, "gemm_tn": 10, "pixel_shuffle2_kernel": 3, "rows_from_nchw_kernel": 1, "add_rows_kernel": 3}


def test_case_table_is_the_module():
    """the parameter names and widths of sr_cases are sr.sr_param_shapes'; the per-unit methods the GPU test calls exist"""
    S = importlib.import_module(SC.PKG + ".sr")
    shapes = S.sr_param_shapes(4, SC.C1, SC.C2, SC.DEPTH)
    assert shapes[SC.DEC + "last_conv.0.weight"] == (256, SC.CX + SC.CA, 3, 3) and shapes[SC.DEC + "conv2.weight"][0] == SC.CX
    for kind, (pre, names) in SC.UNIT_PARAMS.items():
        assert all(pre + n in shapes for n in names), kind
    assert f"{SC.ED}body.{SC.DEPTH}.weight" in shapes and f"{SC.ED}body.{SC.DEPTH}.body.0.weight" not in shapes
    for m in ("_dec_entry_fwd", "_dec_entry_bwd", "_dec_tail_fwd", "_dec_tail_bwd", "_head_fwd", "_head_bwd", "_resblock_fwd",
              "_resblock_bwd", "_body_close_fwd", "_body_close_bwd", "_up_fwd", "_up_bwd", "_close_fwd", "_close_bwd"):
        assert callable(getattr(S.SRBranch, m)), m
    src = open(os.path.join(os.path.dirname(LIB), "sr.py")).read()
    assert f"ct.cout <= {SC.NCHW_DIRECT_MAX_CH}" in src


def test_watched_kernels_exist_in_the_library():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run build() first")
    with open(LIB, "rb") as f:
        blob = f.read()
    assert len(SC.SINGLE) == 13
    for n in SC.SINGLE + SC.ADD:
        assert n.encode() in blob, n
