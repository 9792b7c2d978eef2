"""Shared helpers of tests/test_block_routes_gpu.py and tests/test_block_emul_host.py: the case matrix of one Swin block through
Engine._block_fwd / _block_bwd, the two float64 references of a case and the gate that comes from them.

Reference A is the exact block: oracle.ref_torch.swin_block in float64 on the tensor the engine reads (x_in, already rounded to the
run dtype) with the parameters as the route reads them (GEMM weights rounded to bf16 on the bf16 path, everything else f32).
Reference B is the same graph with `store=narrow`: a straight-through rounding to bf16 (forward and gradient) at every point where
the bf16 route narrows a value - see swin_block's docstring for the list; the gradients dh / dc / du / dxn / dqkv / dxm / dX are
narrowed by the backward of the same function.  B says nothing about the kernels: it is float64 torch with roundings put in.

    e_emul(T) = |T_B - T_A|_2 / |T_A|_2          the reference's own measure of bf16 noise on tensor T
    gate(T)   = 3 e_emul(T) + 1e-5               bf16 routes;  2e-3 on the f32 routes (test_model_gpu's f32 gradient gate)

`python tests/block_cases.py` prints e_emul for every (reference, tensor) on the CPU; the same table with the routes' measured
errors beside it is in DESIGN.md section 2 ("Block routes against float64").
"""
from __future__ import annotations

import os
import sys
from typing import Dict, NamedTuple, Optional, Tuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BF, F32 = torch.bfloat16, torch.float32
E = "image_encoder."
MARGIN, FLOOR, F32_GATE, E_EMUL_MAX = 3.0, 1e-5, 2e-3, 5e-2
GEMM_WEIGHTS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight", "mlp.conv1.weight")
# the folded conv-MLP composes its weights from the f32 masters of fc1 / conv1 (csrc/convmlp.hip): it never reads them rounded
FOLD_F32 = ("mlp.fc1.weight", "mlp.conv1.weight")
# mlp.fc2.bias: its gradient is the column sum of dY, a tensor given in bf16 that no narrowing point touches, so B equals A on it
# and its gate is the floor alone (f32 accumulation); e_emul == 0 is asserted for it instead of e_emul > 0
UNTOUCHED = ("mlp.fc2.bias",)
SEED_X, SEED_DY = 2, 9

# route names as engine.py spells them (kept here so that a host test can state the table without importing the engine)
FUSED_RC, FUSED_SAVED, PADDED, PLAIN = "fused, q/k/v recomputed", "fused, q/k/v saved", "padded", "plain"
M_FUSED, M_LIN_RC, M_LIN_SAVED, M_FOLD, M_CONV = "fused linear", "linear, activation saved", "linear, pre-activation saved", \
    "folded conv", "three-GEMM conv"


# kernels with one instantiation family each that the route tests count by name (GEMM and attention families: gemm_cases / attn_cases)
WATCHED_KERNELS = ("wmsa_hg_kernel", "wmsa_block_kernel", "mlp_fwd_kernel", "linbwd_sq_kernel", "convmlp_compose_kernel",
                   "convmlp_border_fix_kernel", "convmlp_border_sums_kernel", "convmlp_decompose_kernel")


class _Narrow(torch.autograd.Function):
    """x -> bf16 -> x.dtype, and the same for the gradient on the way back (straight-through)."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


def narrow(x: torch.Tensor, name: str = "") -> torch.Tensor:
    """the `store=` callable of reference B (oracle.ref_torch.swin_block): every stored value alike"""
    return _Narrow.apply(x)


class Case(NamedTuple):
    id: str
    tag: str                        # "stage1.0"
    S: int
    B: int
    dtype: torch.dtype
    switches: Tuple[Tuple[str, object], ...]     # Engine attributes that differ from their defaults
    attn: str
    mlp: str
    sq_ok: bool
    zscratch: bool
    pad: Optional[Tuple[int, int]]


def _c(id, tag, S, B, dtype, attn, mlp, sq_ok=False, zscratch=False, pad=None, **switches):
    return Case(id, tag, S, B, dtype, tuple(sorted(switches.items())), attn, mlp, sq_ok, zscratch, pad)


CASES = (
    _c("s1.0-bf16", "stage1.0", 256, 2, BF, FUSED_RC, M_FUSED, sq_ok=True),
    _c("s1.0-bf16-mlp_off", "stage1.0", 256, 2, BF, FUSED_RC, M_LIN_RC, sq_ok=True, use_fused_mlp=False),
    _c("s1.0-bf16-wmsa_off", "stage1.0", 256, 2, BF, PLAIN, M_FUSED, sq_ok=True, use_fused_wmsa=False),
    _c("s1.1-bf16", "stage1.1", 256, 2, BF, FUSED_RC, M_FOLD, sq_ok=True),
    _c("s1.1-bf16-linbwd_off", "stage1.1", 256, 2, BF, FUSED_RC, M_FOLD, sq_ok=True, use_fused_linbwd=False),
    _c("s1.1-bf16-fold_off", "stage1.1", 256, 2, BF, FUSED_RC, M_CONV, sq_ok=True, convmlp_fold_maxc=0),
    _c("s1.1-bf16-wmsa_off", "stage1.1", 256, 2, BF, PLAIN, M_FOLD, sq_ok=True, use_fused_wmsa=False),
    _c("s2.0-bf16", "stage2.0", 256, 2, BF, PLAIN, M_LIN_RC),
    _c("s2.1-bf16", "stage2.1", 256, 2, BF, PLAIN, M_FOLD),
    _c("s3.0-bf16-S256", "stage3.0", 256, 2, BF, PLAIN, M_LIN_RC, zscratch=True),
    _c("s3.0-bf16-S512", "stage3.0", 512, 1, BF, PLAIN, M_LIN_RC, zscratch=True),
    _c("s3.0-bf16-S640", "stage3.0", 640, 1, BF, PADDED, M_LIN_RC, zscratch=True, pad=(64, 64)),
    _c("s1.0-f32", "stage1.0", 256, 2, F32, FUSED_SAVED, M_LIN_SAVED),
    _c("s1.1-f32", "stage1.1", 256, 2, F32, FUSED_SAVED, M_CONV),
    _c("s1.1-f32-wmsa_off", "stage1.1", 256, 2, F32, PLAIN, M_CONV, use_fused_wmsa=False),
)


# ------------------------------------------------------------------ geometry
class Geo(NamedTuple):
    B: int
    H: int
    W: int
    C: int
    window: int         # the block's constructor window (swin_block clamps it to the grid)
    shift: int
    linear: bool


def geometry(tag: str, S: int, B: int) -> Geo:
    from oracle import ref_torch as R
    si, i = int(tag[5]) - 1, int(tag.split(".")[1])
    H = (S // 4) >> si
    shift = R.SHIFTS[i] if H > R.STAGE_WINDOWS[si] else 0
    return Geo(B, H, H, R.STAGE_DIMS[si], R.STAGE_WINDOWS[si], shift, R.SHIFTS[i] == 0 or si == 2)


def subsets(g: Geo) -> Dict[str, torch.Tensor]:
    """Row masks over the B*H*W tokens: the last grid row / column (the 2x2 convolution's pad border), the wrap region of a
    shifted block's mask (y >= H - shift or x >= W - shift), and every other token."""
    y = torch.arange(g.H).view(1, g.H, 1).expand(g.B, g.H, g.W).reshape(-1)
    x = torch.arange(g.W).view(1, 1, g.W).expand(g.B, g.H, g.W).reshape(-1)
    border = (y == g.H - 1) | (x == g.W - 1)
    out = {"border": border}
    rest = ~border
    if g.shift:
        wrap = (y >= g.H - g.shift) | (x >= g.W - g.shift)
        out["wrap"] = wrap
        rest = rest & ~wrap
    out["rest"] = rest
    return out


# ------------------------------------------------------------------ inputs
_sd: Dict[int, dict] = {}
_acts: Dict[Tuple[int, int], Dict[str, torch.Tensor]] = {}


def state_dict(S: int) -> dict:
    from oracle import ref_torch as R
    if S not in _sd:
        _sd[S] = R.procedural_state_dict(S, 8)
    return _sd[S]


def block_input(tag: str, S: int, B: int) -> torch.Tensor:
    """The model's own activation in front of block `tag` under R.synthetic_inputs(B, S, seed=SEED_X): the oracle's f32 encoder
    run up to that block, [B*H*W][C] f32."""
    from oracle import ref_torch as R
    acts = _acts.setdefault((S, B), {})
    if tag in acts:
        return acts[tag]
    sd, pfx = state_dict(S), E
    with torch.no_grad():
        if "x" not in acts:
            x_rgb, x_ir = R.synthetic_inputs(B, S, seed=SEED_X)
            x = R.frontend(sd, torch.cat([x_rgb, x_ir[:, 0:1]], 1), pfx)
            acts["x"], acts["next"] = x.view(B, -1, x.shape[-1]), (0, 0)
        h = S // 4
        while tag not in acts:
            si, i = acts["next"]
            hs = h >> si
            name = f"stage{si + 1}.{i}"
            acts[name] = acts["x"].reshape(-1, acts["x"].shape[-1]).clone()
            if name == tag:
                break
            x = R.swin_block(sd, f"{pfx}{name}.", acts["x"], hs, hs, R.STAGE_WINDOWS[si], R.SHIFTS[i], R.SHIFTS[i] == 0 or si == 2)
            i += 1
            if i == R.STAGE_DEPTHS[si]:
                x = R.patch_merging(sd, f"{pfx}pmerging{si + 1}.", x, hs, hs)
                si, i = si + 1, 0
            acts["x"], acts["next"] = x, (si, i)
    return acts[tag]


def grad_output(M: int, C: int) -> torch.Tensor:
    """dY: N(0, 1) rounded to bf16 (exact in either run dtype), as f32."""
    gen = torch.Generator(device="cpu").manual_seed(SEED_DY)
    return torch.randn(M, C, generator=gen).to(BF).float()


def param_names(tag: str, linear: bool):
    pre = E + tag + "."
    names = [pre + f"norm{i}.{wb}" for i in (1, 2) for wb in ("weight", "bias")]
    names += [pre + f"attn.{l}.{wb}" for l in ("qkv", "proj") for wb in ("weight", "bias")]
    names += [pre + "attn.relative_position_bias_table"]
    names += [pre + f"mlp.{l}.{wb}" for l in (("fc1", "fc2") if linear else ("fc1", "conv1", "fc2")) for wb in ("weight", "bias")]
    return names


# ------------------------------------------------------------------ references
def run_reference(tag: str, S: int, B: int, dtype, fold: bool, store) -> Dict[str, torch.Tensor]:
    """One float64 forward and backward of the block; returns xo, dX ([M][C]) and the gradient of every parameter (short names)."""
    from oracle import ref_torch as R
    g = geometry(tag, S, B)
    pre = E + tag + "."
    sd = state_dict(S)
    params = {}
    for n in param_names(tag, g.linear):
        v, short = sd[n], n[len(pre):]
        if dtype == BF and short in GEMM_WEIGHTS and not (fold and short in FOLD_F32):
            v = v.to(BF)
        params[n] = v.double().clone().requires_grad_(True)
    x = block_input(tag, S, B).to(dtype).double().view(B, g.H * g.W, g.C).clone().requires_grad_(True)
    seen = {}

    def recording(t, name):         # the convolution's pre-activation as the route stores it (tag.cp), beside xo
        t = t if store is None else store(t, name)
        seen[name] = t.detach()
        return t
    xo = R.swin_block(params, pre, x, g.H, g.W, g.window, g.shift, g.linear, store=recording)
    xo.backward(grad_output(B * g.H * g.W, g.C).double().view_as(xo))
    out = {"xo": xo.detach().reshape(-1, g.C), "dX": x.grad.reshape(-1, g.C)}
    if not g.linear:
        out["cp"] = seen["cp"].reshape(-1, g.C)
    for n, p in params.items():
        out[n[len(pre):]] = p.grad
    return out


def rel_l2(t: torch.Tensor, ref: torch.Tensor) -> float:
    return float((t.double().cpu() - ref).norm() / ref.norm())


class Reference(NamedTuple):
    A: Dict[str, torch.Tensor]          # tensor name (subsets of xo / dX as "xo[border]", ...) -> float64 value
    e_emul: Dict[str, float]            # bf16 only


_refs: Dict[tuple, Reference] = {}


FIELDS = ("xo", "dX", "cp")          # [M][C] tensors, also gated on the row subsets


def with_subsets(t: Dict[str, torch.Tensor], g: Geo) -> Dict[str, torch.Tensor]:
    out = dict(t)
    for name, rows in subsets(g).items():
        for k in FIELDS:
            if k in t:
                out[f"{k}[{name}]"] = t[k][rows.to(t[k].device)]
    return out


def reference(case: Case) -> Reference:
    """References of a case, computed once per (block, S, B, dtype, folded or not) and shared by every case that reads them."""
    fold = case.mlp == M_FOLD
    key = (case.tag, case.S, case.B, case.dtype, fold)
    if key not in _refs:
        g = geometry(case.tag, case.S, case.B)
        A = with_subsets(run_reference(case.tag, case.S, case.B, case.dtype, fold, None), g)
        e = {}
        if case.dtype == BF:
            Bt = with_subsets(run_reference(case.tag, case.S, case.B, case.dtype, fold, narrow), g)
            e = {k: rel_l2(Bt[k], A[k]) for k in A}
        _refs[key] = Reference(A, e)
    return _refs[key]


def gate(case: Case, ref: Reference, name: str) -> float:
    return F32_GATE if case.dtype == F32 else MARGIN * ref.e_emul[name] + FLOOR


def check_reference(case: Case, ref: Reference) -> None:
    """The conditions on the reference alone: |T_A| > 0 and 0 < e_emul(T) <= 5e-2 for every tensor (e_emul == 0 where no narrowing
    point can reach the tensor: UNTOUCHED)."""
    for k, a in ref.A.items():
        assert float(a.norm()) > 0, (case.id, k)
        if case.dtype != BF:
            continue
        if k in UNTOUCHED:
            assert ref.e_emul[k] == 0.0, (case.id, k, ref.e_emul[k])
        else:
            assert 0 < ref.e_emul[k] <= E_EMUL_MAX, (case.id, k, ref.e_emul[k])


GROUPS = (("xo", ("xo",)), ("xo subsets", ("xo[",)), ("cp", ("cp",)), ("cp subsets", ("cp[",)), ("dX", ("dX",)), ("dX subsets", ("dX[",)),
          ("norm1/2", ("norm",)),
          ("attn.qkv/proj", ("attn.qkv", "attn.proj")), ("bias table", ("attn.relative",)), ("mlp", ("mlp.",)))


def group_of(name: str) -> str:
    if name in FIELDS:
        return name
    for gname, pres in GROUPS:
        if gname not in FIELDS and name.startswith(pres):
            return gname
    raise KeyError(name)


if __name__ == "__main__":
    import time
    seen = set()
    for c in CASES:
        key = (c.tag, c.S, c.B, c.dtype, c.mlp == M_FOLD)
        if key in seen or c.dtype != BF:
            continue
        seen.add(key)
        t0 = time.time()
        r = reference(c)
        check_reference(c, r)
        print(f"# {c.tag} S={c.S} B={c.B} {'folded' if key[4] else ''} ({time.time() - t0:.1f} s)")
        for k, v in r.e_emul.items():
            print(f"{k:42s} e_emul {v:.3e}   gate {MARGIN * v + FLOOR:.3e}")
