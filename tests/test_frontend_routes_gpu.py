"""The front-end kernels against float64, element by element, with a check of which kernel ran: the fused window-1 kernels of
csrc/frontend.hip (sodt_frontend_fwd / _bwd on every launch shape of its dispatch) and the general form of csrc/cattn.hip
(sodt_patch_embed4_fwd / _bwd, sodt_cross_attn_ln_fwd / _bwd).  Cases, references, bounds and routes: tests/frontend_cases.py;
tests/test_frontend_ref_host.py holds the bounds against an f32 statement and ten mutated ones on the CPU.

Reference.  oracle.ref_torch.channel_embeds / cattention_block in float64 with autograd.  The four embedding planes are leaves, so
their gradient de is compared with the kernel's; dw / db of patch_embed4_bwd are compared on the reference's own de.

Bound.  Every kernel computes in f32 (U = 2^-24); the run dtype narrows only the store of `out` (U_T) and the read of dout, which
is exact.  A gated element must lie within  U_T |ref| + (first-order propagated f32 error) + 1e-30  of the reference, where the
second term carries, stage by stage, the operation counts of the kernels times the absolute-value companion of the same graph:

    e     = b + sum_k w p         16 multiply-adds: |de| <= K_E U (|b| + sum |w||p|), K_E = 17.
    score = (q.k - 100 m) / 2     the two operand errors, 5 U |q|.|k| for the dot product, U (|q|.|k| + 100) for the mask add and
                                  U |score| for the scale: E.
    p     = softmax               p_j (E_j + sum_i p_i E_i + (8 N + 4 (max - s_j) + 4 (max - min) + 8) U): at most N = 64 online
                                  steps of two __expf (relative error (2 |x| + 2) U at argument x; the arguments of one key's
                                  chain add up to at most (max - s_j) + (max - min)), a multiply and an add each for the
                                  denominator and the numerator, then the division.  The backward forms exp(s - max) / den
                                  directly and stays inside the same figure.
    o     = sum p v               the error of p times |v|, p times the error of v, (N + 2) U sum p |v|.
    s     = e_q + o               one more rounding.
    LN    = (s - mean) rstd g + b mean and variance are 48-term sums, the subtraction one rounding, rsqrtf one ulp: K_LN = 50;
                                  an error ds of s moves xhat by at most rstd (ds_i + mean ds + |xhat_i| mean(|xhat| ds))
                                  (the rstd amplification: up to 316 on a token whose 48 sums are equal), and rstd by the
                                  relative r = rstd mean(|xhat| ds) + 27 U.
    dgamma = sum_tok dy xhat      sum |dy| X (X the error of xhat) + (D + 2) U sum |dy xhat|;  dbeta = sum dy: D U sum |dy|.
    ds    = rstd (g - mean g - xhat mean(g xhat)), g = dy gamma:
                                  r |ds| + rstd (X |c2| + |xhat| mean(|g| X)) + (K_LN + 6) U A_ds, A_ds its absolute companion.
    de                            dp_j = ds.k_j, delta = sum p dp, dsc = p (dp - delta) / 2, dq = ds + sum dsc k,
                                  dkv_j = p_j ds + dsc_j q, each with the errors of its operands and its own 3 .. N + 6 roundings;
                                  2 N + 2 atomics at most land on one element of de.
    dw, db = sum_tok de p, de     sum (error of de) |p| + (D + 2) U sum |de||p|.

D is the depth of the longest chain of f32 additions an element of a sum can pass through, whatever the order of the atomics
(an addition chain of depth D has error at most D U sum |terms|): 64 tokens of an MFMA tile per trip of the grid-stride loop,
the permlane / shuffle folds, then one atomic per workgroup (one-stage), or 32 rows and one atomic per row group (two-stage);
one atomic per wave and min(ntok, 512) atomics in cross_attn_ln_bwd and patch_embed4_bwd (frontend_cases.fused_bwd_route,
general_depths).  Nothing in a bound comes from a kernel's output.

A gradient pre-filled with random values must come back as pre-fill + gradient within the same bound plus one rounding of the
sum.  Buffers carry quiet-NaN margins that must come back bit-identical, as must the rows of the workspace past the grid.

Exact cases: small-integer images, one-hot weights times a power of two, power-of-two biases: e is exact in f32 and compared
with torch.equal; at tokens whose 48 pair sums are equal the fused forward must return beta itself.

Measured on an MI355X, worst err / bound of each tensor; every ratio must be at most 1.  (The bf16 `out` sits at its store's own
half ulp.  The gradients sit far inside: their bound is the worst case over every order of the additions.  With the reduce
kernel made to drop the last workgroup's row, the two-stage cases fail at 10 to 900 times the bound; with the masked keys'
scores of cross_attn_ln_bwd's last loop off by 0.1 %, the finite-mask case fails on de at 540 times, and nothing else fails.)
ws / none / short: backward with a workspace, without one, with one a float short:

    case                              e        out      de       dgamma   dbeta    dw       db
    fused-1-4-4-f32 ws                         7.6e-03           7.3e-03  0.0e+00  3.9e-03  2.9e-03
    fused-1-4-4-bf16 ws                        9.5e-01           6.5e-03  0.0e+00  3.3e-03  2.6e-03
    fused-2-8-260-f32 ws                       1.8e-02           9.3e-04  6.5e-03  1.3e-03  2.4e-04
    fused-2-8-260-bf16 ws                      9.9e-01           7.1e-04  1.2e-03  1.1e-03  2.3e-04
    fused-1-256-256-f32 ws                     2.0e-02           3.2e-04  7.2e-04  2.2e-04  1.3e-04
    fused-1-256-256-bf16 ws                    9.9e-01           3.0e-04  3.0e-04  1.9e-04  9.8e-05
    fused-1-256-260-f32 ws                     1.9e-02           2.8e-04  1.5e-03  2.0e-04  6.4e-05
    fused-1-256-260-f32 none                                     2.5e-04  1.1e-03  2.0e-04  8.9e-05
    fused-1-256-260-f32 short                                    3.0e-04  6.6e-04  1.7e-04  9.6e-05
    fused-1-256-260-bf16 ws                    9.9e-01           3.3e-04  7.8e-04  1.7e-04  6.4e-05
    fused-1-256-260-bf16 none                                    3.2e-04  2.3e-04  1.8e-04  1.2e-04
    fused-1-256-260-bf16 short                                   3.7e-04  2.8e-04  1.8e-04  1.4e-04
    fused-3-420-420-f32 ws                     2.6e-02           8.0e-05  2.8e-04  7.7e-05  2.4e-05
    fused-3-420-420-f32 none                                     7.3e-05  1.6e-04  6.0e-05  4.7e-05
    fused-3-420-420-f32 short                                    1.0e-04  1.3e-04  7.0e-05  5.3e-05
    fused-3-420-420-bf16 ws                    9.9e-01           7.9e-05  1.6e-04  7.4e-05  3.1e-05
    fused-3-420-420-bf16 none                                    1.0e-04  1.2e-04  9.4e-05  3.5e-05
    fused-3-420-420-bf16 short                                   8.3e-05  1.2e-04  8.3e-05  4.3e-05
    fused-irstride-f32 one-plane               1.8e-02           7.5e-04  5.2e-03  1.3e-03  2.4e-04
    fused-irstride-f32 plane0                  1.8e-02           7.5e-04  3.6e-03  1.3e-03  2.5e-04
    fused-irstride-f32 plane2                  1.9e-02           8.5e-04  4.8e-03  1.4e-03  2.4e-04
    fused-irstride-bf16 one-plane              9.9e-01           7.1e-04  1.2e-03  1.1e-03  2.3e-04
    fused-irstride-bf16 plane0                 9.9e-01           7.1e-04  1.2e-03  1.1e-03  2.3e-04
    fused-irstride-bf16 plane2                 9.9e-01           9.5e-04  1.2e-03  1.1e-03  2.9e-04
    general-1-48-48-2-0-f32           1.8e-01  4.6e-03  2.0e-03  1.5e-04  3.0e-02  2.0e-02  1.0e-02
    general-1-48-48-2-0-bf16          1.8e-01  9.5e-01  2.1e-03  1.3e-04  2.4e-03  2.5e-02  9.6e-03
    general-1-48-48-2-1-f32           1.8e-01  3.7e-03  1.5e-03  1.8e-04  4.0e-02  2.4e-02  1.6e-02
    general-1-48-48-2-1-bf16          1.8e-01  9.5e-01  1.4e-03  1.8e-04  1.3e-03  2.6e-02  1.4e-02
    general-1-48-48-4-3-f32           1.9e-01  4.4e-03  1.5e-03  3.0e-04  3.8e-02  2.1e-02  1.1e-02
    general-1-48-48-4-3-bf16          1.9e-01  9.6e-01  1.6e-03  2.7e-04  0.0e+00  2.3e-02  1.5e-02
    general-1-32-32-8-7-f32           1.7e-01  3.2e-03  2.1e-03  3.2e-04  8.2e-02  3.9e-02  3.5e-02
    general-1-32-32-8-7-bf16          1.7e-01  9.4e-01  1.5e-03  3.0e-04  0.0e+00  3.9e-02  2.9e-02
    general-2-32-96-8-3-f32           2.0e-01  3.6e-03  2.3e-03  1.4e-04  1.4e-02  7.0e-03  4.1e-03
    general-2-32-96-8-3-bf16          2.0e-01  9.6e-01  1.5e-03  2.4e-04  4.0e-03  8.5e-03  4.2e-03
    general-3-16-24-2-1-f32           1.9e-01  4.3e-03  2.6e-03  1.7e-04  4.8e-02  4.5e-02  2.2e-02
    general-3-16-24-2-1-bf16          1.9e-01  9.4e-01  2.5e-03  1.9e-04  0.0e+00  3.5e-02  2.6e-02
    general-2-8-260-1-0-f32           1.8e-01  5.3e-03  3.4e-03  3.2e-04  2.3e-02  9.9e-03  4.9e-03
    general-2-8-260-1-0-bf16          1.8e-01  9.8e-01  3.8e-03  2.7e-04  2.8e-03  1.1e-02  6.3e-03
    finite-1-32-32-4-2-f32                     2.2e-02  1.8e-02  1.0e-03  7.4e-02
    finite-1-32-32-4-2-bf16                    9.7e-01  1.7e-02  9.7e-04  1.8e-02
    exact-frontend_fwd-f32                     3.0e-01
    exact-cross_attn_ln_fwd-f32                3.0e-01
    exact-frontend_fwd-bf16                    8.6e-01
    exact-cross_attn_ln_fwd-bf16               8.6e-01
    prefill-fused-2-8-260-f32                                    1.0e-03  4.6e-03  1.3e-03  3.8e-04
    prefill-fused-1-256-260-f32                                  3.0e-04  1.5e-03  2.1e-04  6.7e-05
    prefill-general-1-48-48-4-3-f32                     3.6e-03  3.0e-04  3.2e-02  1.9e-02  1.3e-02
    prefill-fused-2-8-260-bf16                                   7.3e-04  1.2e-03  1.1e-03  2.9e-04
    prefill-fused-1-256-260-bf16                                 3.2e-04  5.7e-04  1.9e-04  6.4e-05
    prefill-general-1-48-48-4-3-bf16                    2.2e-03  2.2e-04  1.3e-02  2.7e-02  1.4e-02
"""
import contextlib

import pytest
import torch

import attn_cases as A
import frontend_cases as FC
import gemm_cases as G

pytestmark = pytest.mark.gpu
BF, F32 = FC.BF, FC.F32
DTYPES = [F32, BF]
DT_IDS = ["f32", "bf16"]
FUSED_GATED = ("out", "dw", "db", "dgamma", "dbeta")
GENERAL_RUN = FC.GENERAL_CASES + [FC.STRIDE_CASE + (1, 0)]             # window 1 through the general route as well

_gpu_error = []      # a HIP error in one case: the cases after it launch nothing more
_dev_cache = {}


@contextlib.contextmanager
def gpu(cid):
    if _gpu_error:
        pytest.fail(f"not run: an earlier case ended in a GPU error ({_gpu_error[0]})")
    try:
        yield
        torch.cuda.synchronize()
    except RuntimeError as e:
        _gpu_error.append(f"{cid}: {e}")
        raise


def on_dev(su, dev):
    key = (su["kind"],) + su["case"]
    if key not in _dev_cache:
        _dev_cache.clear()                                               # one case's images at a time
        _dev_cache[key] = {k: su[k].to(dev) for k in ("rgb", "ir3", "w", "b", "gamma", "beta")}
    return _dev_cache[key]


def launched(fn):
    return FC.frontend_kernels(G.launched_kernels(fn))


def gate(tag, got, ref, bnd, names, prefill=None):
    """Print worst err / bound of every tensor, then require each to be at most 1.  prefill: the values the gradients were
    added onto (the reference becomes prefill + gradient, the bound grows by one rounding of the sum)."""
    ratios = {}
    for n in names:
        r, b = ref[n].double(), bnd[n]
        if prefill is not None and n in prefill:
            r = r.reshape(prefill[n].shape) + prefill[n].double().cpu()
            b = b.reshape(r.shape) + FC.U * r.abs()
        ratios[n] = FC.worst(got[n], r, b.reshape(r.shape))
    print(f"\n    {tag:<44}" + "  ".join(f"{n} {ratios[n]:.1e}" for n in names))
    bad = {n: v for n, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{tag}: err / bound over 1: {bad}"


def margins_intact(buf, mid_rows, pad=2):
    bits = A.sentinel_bits(buf)
    return bool(bits[:pad].all()) and bool(bits[pad + mid_rows:].all())


def grads(d, dev, prefill_seed=None):
    """dw, db, dgamma, dbeta: zeros, or random f32 values to be added onto."""
    shapes = dict(dw=(4, FC.CE, 16), db=(4, FC.CE), dgamma=(4, FC.CE), dbeta=(4, FC.CE))
    if prefill_seed is None:
        return {k: torch.zeros(s, device=dev) for k, s in shapes.items()}
    return {k: A.randn(s, prefill_seed + i, dev) for i, (k, s) in enumerate(shapes.items())}


def fused_bwd(ops, d, su, dout, g, ir, ir_bstride, ws):
    ops.frontend_bwd(d["rgb"], ir, ir_bstride, d["w"], d["b"], d["gamma"], d["beta"], dout, g["dw"], g["db"], g["dgamma"], g["dbeta"],
                     su["B"], su["H"], su["W"], ws=ws)


def fused_depth(route):
    return dict(gamma=route["depth"], de=3, embed=route["depth"])


# ------------------------------------------------------------------ fused route
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", FC.FUSED_CASES, ids=FC.case_id)
def test_fused_route(ops, dev, dt, case):
    su = FC.setup("fused", case)
    B, H, W, M = su["B"], su["H"], su["W"], su["M"]
    dout_c, ref = FC.dout_and_reference(su, dt)
    tag = f"fused-{FC.case_id(case)}-{DT_IDS[DTYPES.index(dt)]}"
    modes = ["ws"] + (["none", "short"] if case in FC.THREE_WAY else [])
    got = {}
    with gpu(tag):
        d = on_dev(su, dev)
        dout = dout_c.to(dev)
        ir = d["ir3"][:, 0]
        out_buf, out = A.nan_buffer(M, 192, dt, dev)
        names = launched(lambda: ops.frontend_fwd(d["rgb"], ir, 3 * H * W, d["w"], d["b"], d["gamma"], d["beta"], out, B, H, W))
        assert names == FC.fused_fwd_route(dt), f"{tag}: forward launched {names}"
        assert margins_intact(out_buf, M), f"{tag}: the forward wrote outside its {M} rows"
        got["ws"] = dict(out=out)
        for mode in modes:
            ws_buf, ws = A.nan_buffer(FC.FE_BWD_GRID, FC.FE_PART, F32, dev)
            wsv = {"ws": ws.view(-1), "none": None, "short": ws.view(-1)[:FC.WS_FLOATS - 1]}[mode]
            route = FC.fused_bwd_route(dt, M, None if wsv is None else wsv.numel())
            g = grads(d, dev)
            names = launched(lambda: fused_bwd(ops, d, su, dout, g, ir, 3 * H * W, wsv))
            assert names == route["kernels"], f"{tag} {mode}: backward launched {names}, the route table says {route['kernels']}"
            bits = A.sentinel_bits(ws_buf)
            touched = route["grid"] if route["two_stage"] else 0
            assert bool(bits[:2].all()) and bool(bits[2 + touched:].all()), f"{tag} {mode}: workspace written past row {touched}"
            assert not bool(bits[2:2 + touched].any()), f"{tag} {mode}: a workspace row of the grid was left unwritten"
            got.setdefault(mode, {}).update(g)
            got[mode]["route"] = route
    if case == (1, 256, 256):
        assert got["ws"]["route"]["kernels"] == [f"frontend_bwd_kernel<{FC._ty(dt)}, false>"]
    if case == (1, 256, 260):
        assert got["ws"]["route"]["kernels"] == [f"frontend_bwd_kernel<{FC._ty(dt)}, true>", "frontend_bwd_reduce_kernel"]
        assert got["short"]["route"]["kernels"] == got["none"]["route"]["kernels"] == [f"frontend_bwd_kernel<{FC._ty(dt)}, false>"]
    for mode in modes:
        bnd = FC.bounds_for(su, dt, fused_depth(got[mode]["route"]))
        gate(f"{tag} {mode}", got[mode], ref, bnd, FUSED_GATED if mode == "ws" else FUSED_GATED[1:])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_fused_ir_stride(ops, dev, dt):
    """The IR plane as a one-plane tensor (stride H W), as plane 0 and as plane 2 of a three-plane tensor (stride 3 H W, plane 2
    behind a pointer offset); the three planes hold different data."""
    su = FC.setup("fused", FC.STRIDE_CASE)
    B, H, W, M = su["B"], su["H"], su["W"], su["M"]
    dout_c, ref0 = FC.dout_and_reference(su, dt)
    ref2 = FC.reference(FC.x4_of(su["rgb"], su["ir3"][:, 2]), su["w"], su["b"], su["gamma"], su["beta"], 1, 0, dout_c)
    route = FC.fused_bwd_route(dt, M, FC.WS_FLOATS)
    depth = fused_depth(route)
    tag = f"fused-irstride-{DT_IDS[DTYPES.index(dt)]}"
    runs = {}
    with gpu(tag):
        d = on_dev(su, dev)
        dout = dout_c.to(dev)
        ws = torch.zeros(FC.WS_FLOATS, device=dev)
        one = d["ir3"][:, 0].contiguous()
        for name, ir, stride in (("one-plane", one, H * W), ("plane0", d["ir3"][:, 0], 3 * H * W), ("plane2", d["ir3"][:, 2], 3 * H * W)):
            out = torch.zeros(M, 192, device=dev, dtype=dt)
            ops.frontend_fwd(d["rgb"], ir, stride, d["w"], d["b"], d["gamma"], d["beta"], out, B, H, W)
            g = grads(d, dev)
            fused_bwd(ops, d, su, dout, g, ir, stride, ws)
            runs[name] = dict(g, out=out)
    su2 = dict(su, x4=FC.x4_of(su["rgb"], su["ir3"][:, 2]))
    bnd0 = FC.bounds_for(su, dt, depth)
    bnd2 = FC.bounds(su2["x4"], su["w"], su["b"], su["gamma"], su["beta"], 1, 0, dout_c, dt, ref2, depth)
    assert float((ref2["out"] - ref0["out"]).abs().max()) > 0.1                   # the planes do differ
    gate(f"{tag} one-plane", runs["one-plane"], ref0, bnd0, FUSED_GATED)
    gate(f"{tag} plane0", runs["plane0"], ref0, bnd0, FUSED_GATED)
    gate(f"{tag} plane2", runs["plane2"], ref2, bnd2, FUSED_GATED)


# ------------------------------------------------------------------ general route
def general_run(ops, d, su, dt, dout, de_ref, dev, e_given=None, prefill_seed=None):
    """patch_embed4_fwd -> cross_attn_ln_fwd -> cross_attn_ln_bwd, and patch_embed4_bwd on de_ref; returns the tensors, the kernel
    names per entry point and the sentinel buffers."""
    B, H, W, M, ws, shift = su["B"], su["H"], su["W"], su["M"], su["ws"], su["shift"]
    got, names, bufs = {}, {}, {}
    if e_given is None:
        bufs["e"], e = A.nan_buffer(M, 192, F32, dev)
        names["embed_fwd"] = launched(lambda: ops.patch_embed4_fwd(d["rgb"], d["ir3"][:, 0], 3 * H * W, d["w"], d["b"], e, B, H, W))
        got["e"] = e
    else:
        e = e_given
    bufs["out"], out = A.nan_buffer(M, 192, dt, dev)
    names["attn_fwd"] = launched(lambda: ops.cross_attn_ln_fwd(e, d["gamma"], d["beta"], out, B, H, W, ws, shift))
    bufs["de"], de = A.nan_buffer(M, 192, F32, dev)
    g = grads(d, dev, prefill_seed)
    pre = {k: v.clone() for k, v in g.items()}
    if prefill_seed is None:
        de.zero_()
    else:
        de.copy_(A.randn((M, 192), prefill_seed + 9, dev))
    pre["de"] = de.clone()
    names["attn_bwd"] = launched(lambda: ops.cross_attn_ln_bwd(e, d["gamma"], dout, de, g["dgamma"], g["dbeta"], B, H, W, ws, shift))
    if e_given is None:
        de_in = de_ref.float().to(dev)
        names["embed_bwd"] = launched(lambda: ops.patch_embed4_bwd(d["rgb"], d["ir3"][:, 0], 3 * H * W, de_in, g["dw"], g["db"], B, H, W))
    got.update(g, out=out, de=de)
    return got, names, bufs, pre


def check_general_names(tag, names, dt):
    want = dict(embed_fwd=["patch_embed4_fwd_kernel"], attn_fwd=[f"cross_attn_ln_fwd_kernel<{FC._ty(dt)}>"],
                attn_bwd=[f"cross_attn_ln_bwd_kernel<{FC._ty(dt)}>"], embed_bwd=["patch_embed4_bwd_kernel"])
    for k, v in names.items():
        assert v == want[k], f"{tag}: {k} launched {v}"


def general_bounds(su, dt):
    depth = FC.general_depths(su["M"], su["ws"] ** 2)
    bnd = FC.bounds_for(su, dt, depth)
    if su["e_given"] is None:                                            # dw / db: patch_embed4_bwd on the reference's de
        exact = FC.bounds_for(su, dt, depth, de_exact=True)
        bnd["dw"], bnd["db"] = exact["dw"], exact["db"]
    return bnd


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", GENERAL_RUN, ids=FC.case_id)
def test_general_route(ops, dev, dt, case):
    su = FC.setup("general", case)
    dout_c, ref = FC.dout_and_reference(su, dt)
    tag = f"general-{FC.case_id(case)}-{DT_IDS[DTYPES.index(dt)]}"
    with gpu(tag):
        d = on_dev(su, dev)
        got, names, bufs, _ = general_run(ops, d, su, dt, dout_c.to(dev), ref["de"], dev)
        for k, buf in bufs.items():
            assert margins_intact(buf, su["M"]), f"{tag}: {k} written outside its {su['M']} rows"
    check_general_names(tag, names, dt)
    gate(tag, got, ref, general_bounds(su, dt), ("e", "out", "de", "dgamma", "dbeta", "dw", "db"))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_finite_mask(ops, dev, dt):
    """Masked keys that win the softmax: -100 is added before the 1/sqrt(4) scale, and it is finite."""
    su = FC.setup("finite", FC.FINITE_CASE)
    dout_c, ref = FC.dout_and_reference(su, dt)
    tag = f"finite-{FC.case_id(FC.FINITE_CASE)}-{DT_IDS[DTYPES.index(dt)]}"
    with gpu(tag):
        d = on_dev(su, dev)
        got, names, bufs, _ = general_run(ops, d, su, dt, dout_c.to(dev), None, dev, e_given=su["e_given"].to(dev))
        for k, buf in bufs.items():
            assert margins_intact(buf, su["M"]), f"{tag}: {k} written outside its {su['M']} rows"
    check_general_names(tag, names, dt)
    gate(tag, got, ref, general_bounds(su, dt), ("out", "de", "dgamma", "dbeta"))


# ------------------------------------------------------------------ exact cases
def test_exact_patch_embed(ops, dev):
    """Plane routing, tap order, R's -1 shift and zero border, the IR stride: e equals the float64 embedding bit for bit."""
    from oracle import ref_torch as R
    B, H, W = FC.EXACT_CASE
    M = B * (H // 4) * (W // 4)
    inp = FC.exact_embed_inputs(B, H, W)
    sd = FC._sd(inp["w"].double(), inp["b"].double(), inp["gamma"].double(), inp["beta"].double())
    with gpu("exact-embed"):
        d = {k: v.to(dev) for k, v in inp.items()}
        for name, plane, ir, stride in (("plane0", 0, d["ir3"][:, 0], 3 * H * W), ("plane2", 2, d["ir3"][:, 2], 3 * H * W),
                                        ("one-plane", 1, d["ir3"][:, 1].contiguous(), H * W)):
            want = torch.cat(R.channel_embeds(sd, FC.x4_of(inp["rgb"], inp["ir3"][:, plane]).double()), -1).reshape(M, 192)
            assert torch.equal(want.float().double(), want)                       # exact in f32 by construction
            e_buf, e = A.nan_buffer(M, 192, F32, dev)
            ops.patch_embed4_fwd(d["rgb"], ir, stride, d["w"], d["b"], e, B, H, W)
            torch.cuda.synchronize()
            assert torch.equal(e.cpu(), want.float()), f"{name}: {int((e.cpu() != want.float()).sum())} elements differ"
            assert margins_intact(e_buf, M)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_exact_frontend_returns_beta_on_flat_tokens(ops, dev, dt):
    """gamma = 1, beta a distinct power of two per (pair, channel): where e_q + e_kv is the same in all 48 channels the output is
    beta itself (the centred value is an exact zero, and 1e-5 keeps rstd finite), which pins the pair-to-beta mapping."""
    B, H, W = FC.EXACT_CASE
    M = B * (H // 4) * (W // 4)
    inp = FC.exact_embed_inputs(B, H, W)
    x4 = FC.x4_of(inp["rgb"], inp["ir3"][:, 0])
    dout = torch.zeros(M, 192, dtype=dt)
    ref = FC.reference(x4, inp["w"], inp["b"], inp["gamma"], inp["beta"], 1, 0, dout)
    e3 = ref["e"].view(M, 4, FC.CE)
    s = e3 + e3[:, list(FC.PAIR_KV)]
    flat = (s.max(-1).values == s.min(-1).values)                                 # [M][4]
    assert all(int(flat[:, p].sum()) >= 2 for p in range(4)) and not bool(flat.all()), flat.sum(0)
    bnd = FC.bounds(x4, inp["w"], inp["b"], inp["gamma"], inp["beta"], 1, 0, dout, dt, ref, dict(gamma=1, de=3, embed=1))
    with gpu("exact-frontend"):
        d = {k: v.to(dev) for k, v in inp.items()}
        out = torch.zeros(M, 192, device=dev, dtype=dt)
        ops.frontend_fwd(d["rgb"], d["ir3"][:, 0], 3 * H * W, d["w"], d["b"], d["gamma"], d["beta"], out, B, H, W)
        out2 = torch.zeros(M, 192, device=dev, dtype=dt)
        e = torch.zeros(M, 192, device=dev)
        ops.patch_embed4_fwd(d["rgb"], d["ir3"][:, 0], 3 * H * W, d["w"], d["b"], e, B, H, W)
        ops.cross_attn_ln_fwd(e, d["gamma"], d["beta"], out2, B, H, W, 1, 0)
    want = inp["beta"].view(1, 4, FC.CE).expand(M, 4, FC.CE).to(dt)
    for name, o in (("frontend_fwd", out), ("cross_attn_ln_fwd", out2)):
        o3 = o.cpu().view(M, 4, FC.CE)
        assert torch.equal(o3[flat], want[flat]), f"{name}: {int((o3[flat] != want[flat]).sum())} flat elements differ from beta"
        gate(f"exact-{name}-{DT_IDS[DTYPES.index(dt)]}", dict(out=o), ref, bnd, ("out",))


# ------------------------------------------------------------------ contracts
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_gradients_accumulate_onto_what_is_there(ops, dev, dt):
    """dw, db, dgamma, dbeta (and de on the general route) pre-filled with random values: pre-fill + gradient comes back, on the
    one-stage, the two-stage and the general route."""
    for case, use_ws in ((FC.STRIDE_CASE, False), ((1, 256, 260), True)):
        su = FC.setup("fused", case)
        dout_c, ref = FC.dout_and_reference(su, dt)
        route = FC.fused_bwd_route(dt, su["M"], FC.WS_FLOATS if use_ws else None)
        assert route["two_stage"] == use_ws
        tag = f"prefill-fused-{FC.case_id(case)}-{DT_IDS[DTYPES.index(dt)]}"
        with gpu(tag):
            d = on_dev(su, dev)
            g = grads(d, dev, prefill_seed=77)
            pre = {k: v.clone() for k, v in g.items()}
            ws = torch.zeros(FC.WS_FLOATS, device=dev) if use_ws else None
            names = launched(lambda: fused_bwd(ops, d, su, dout_c.to(dev), g, d["ir3"][:, 0], 3 * su["H"] * su["W"], ws))
        assert names == route["kernels"]
        gate(tag, g, ref, FC.bounds_for(su, dt, fused_depth(route)), FUSED_GATED[1:], prefill=pre)
    case = (1, 48, 48, 4, 3)
    su = FC.setup("general", case)
    dout_c, ref = FC.dout_and_reference(su, dt)
    tag = f"prefill-general-{FC.case_id(case)}-{DT_IDS[DTYPES.index(dt)]}"
    with gpu(tag):
        got, names, bufs, pre = general_run(ops, on_dev(su, dev), su, dt, dout_c.to(dev), ref["de"], dev, prefill_seed=91)
        assert margins_intact(bufs["de"], su["M"])
    check_general_names(tag, names, dt)
    gate(tag, got, ref, general_bounds(su, dt), ("de", "dgamma", "dbeta", "dw", "db"), prefill=pre)


def test_window_entries_refuse_without_touching_their_outputs(ops, dev):
    """ws = 9, shift = ws, shift = -1, and ws = 1 with shift = 1: SODT_EINVAL, no launch, outputs untouched."""
    su = FC.setup("general", (1, 48, 48, 4, 3))
    M = 18 * 18                                  # rows of the largest grid named below (72 x 72: 9 divides its 18 x 18 tokens)
    nan = float("nan")
    with gpu("refusals"):
        d = on_dev(su, dev)
        e = torch.zeros(M, 192, device=dev)
        dout = torch.ones(M, 192, device=dev)
        out = torch.full((M, 192), nan, device=dev)
        de = torch.full((M, 192), nan, device=dev)
        dg, dbe = torch.full((4, FC.CE), nan, device=dev), torch.full((4, FC.CE), nan, device=dev)

        def attempts():
            for S, ws, shift in ((72, 9, 0), (48, 4, 4), (48, 2, 2), (48, 4, -1), (48, 1, 1)):
                with pytest.raises(RuntimeError, match="status 1"):
                    ops.cross_attn_ln_fwd(e, d["gamma"], d["beta"], out, 1, S, S, ws, shift)
                with pytest.raises(RuntimeError, match="status 1"):
                    ops.cross_attn_ln_bwd(e, d["gamma"], dout, de, dg, dbe, 1, S, S, ws, shift)
        assert launched(attempts) == []
        torch.cuda.synchronize()
        for t in (out, de, dg, dbe):
            assert bool(torch.isnan(t).all())
        ops.cross_attn_ln_fwd(e, d["gamma"], d["beta"], out, 1, 48, 48, 4, 3)         # and the shift below the window is accepted
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[:su["M"]]).all()) and bool(torch.isnan(out[su["M"]:]).all())
