"""Shared helpers of tests/test_sr_routes_gpu.py and tests/test_sr_emul_host.py: the case matrix of the super-resolution branch's
units (sr.SRBranch: the Decoder's entry and its last_conv chain, EDSR's head convolution, one ResBlock, the body's closing
convolution + skip, one Upsampler stage, the closing convolution, and the EDSR(depth 2) walk), the two float64 references of a case
and the gate that comes from them.  The counterpart of tests/head_cases.py, with block_cases' narrow / MARGIN / FLOOR / F32_GATE /
E_EMUL_MAX / rel_l2 as they are.

Reference A is the exact unit: oracle.ref_torch.sr_decoder_entry / sr_decoder_tail / edsr_head / edsr_resblock / edsr_body_close /
edsr_upsampler_stage / edsr_close / edsr in float64 on the operands the route reads (inputs and incoming gradients N(0, 1) rounded
to bf16; on bf16 cases the convolution weights rounded to bf16, the composed wTp being a plain transpose of them; biases f32).
Reference B is the same graph with a straight-through bf16 rounding at the store points listed in the docstrings of
ref_torch.sr_decoder and ref_torch.edsr, which were read off sr.py and the kernels' epilogues.  B says nothing about the kernels.

    e_emul(T) = |T_B - T_A|_2 / |T_A|_2          the reference's own measure of bf16 noise on tensor T
    gate(T)   = 3 e_emul(T) + 1e-5               bf16 routes;  2e-3 on the f32 routes

The closing convolution's store point "y" depends on the form the route takes, and the table is stated here (NCHW_DIRECT_MAX_CH):
with at most 4 output channels the bf16 route writes the float32 NCHW output itself, unrounded, and reads the float32 gradient
narrowed; above that it goes through [M][Np] rows of the run dtype (sr.py: _close_fwd, the "e.o" / "g.o" buffers), which round
the output as well.

Gated per case: the unit output, every input gradient, every parameter gradient; the two slices of the concatenation and
g.cu / g.a separately; out and din again on the first / last grid row and column of every unit with a 3x3; the Upsampler
stage's output on each (y & 1, x & 1) parity of the fine grid, its weight / bias gradient rows 4 c + p of each plane p, and
the input gradient of an incoming gradient that lives on one parity alone ("din[pYX]": what one plane launch reads back).  Every
subset is gated with e_emul of that same subset.

Tensors no store point reaches have e_emul == 0 exactly and the floor as their gate (untouched()): the weight / bias gradient of a
convolution whose input and incoming gradient are both given (conv1 of the Decoder entry, the body's closing convolution, the
Upsampler stage, the closing convolution), the bias gradient of a unit's last convolution (the column sum of the given gradient:
last_conv.4, a ResBlock's body.2, the walk's tail.1), and the closing convolution's float32 output where the route writes it
itself.

`python tests/sr_cases.py` prints e_emul for every (case, tensor) on the CPU; the same table with the routes' measured errors
beside it is in DESIGN.md section 2 ("SR units against float64").
"""
from __future__ import annotations

import importlib
import os
import sys
from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from block_cases import BF, E_EMUL_MAX, F32, F32_GATE, FLOOR, MARGIN, narrow, rel_l2     # noqa: E402,F401

PKG = "small-object-detection-transformers_amd"
C1, C2, DEPTH = 128, 512, 2
CA, CX = C1 // 2, C2 // 2               # the concatenation: [x resized (CX) | low (CA)]
NCHW_DIRECT_MAX_CH = 4                  # bf16: the closing convolution writes / reads the float32 NCHW tensors itself up to here
SEED_X, SEED_X2, SEED_DY, SEED_DY2 = 5, 7, 6, 8
# added to the four seeds of a kind.  Under the base seeds two references stood above the 5e-2 cap on e_emul through ReLU inputs
# within bf16 rounding of zero (dec_tail B2 8x12: g.cu / g.a on the bottom row, 5.7e-2; walk B2 10x12: body.1.body.0, 5.6e-2 and
# 7.3e-2); the first of the shifts 100, 200, ... under which every case of the kind meets the condition is taken - a property of
# the references alone (worst e_emul then: dec_tail 4.9e-2, walk 2.5e-2).
SEED_SHIFT = {"dec_tail": 100, "walk": 200}
DEC, ED = "sr_decoder.", "edsr."

KINDS = ("dec_entry", "dec_entry_engine", "dec_tail", "head", "resblock", "body_close", "up", "close", "walk")
HAS_3X3 = ("dec_tail", "head", "resblock", "body_close", "up", "close", "walk")
# the parameters of a unit, relative to DEC / ED
UNIT_PARAMS = {
    "dec_entry": (DEC, ("conv1.weight", "conv2.weight")),
    "dec_entry_engine": (DEC, ("conv1.weight", "conv2.weight")),
    "dec_tail": (DEC, ("last_conv.0.weight", "last_conv.2.weight", "last_conv.4.weight", "last_conv.4.bias")),
    "head": (ED, ("head.0.weight", "head.0.bias")),
    "resblock": (ED, ("body.0.body.0.weight", "body.0.body.0.bias", "body.0.body.2.weight", "body.0.body.2.bias")),
    "body_close": (ED, (f"body.{DEPTH}.weight", f"body.{DEPTH}.bias")),
    "up": (ED, ("tail.0.0.weight", "tail.0.0.bias")),
    "close": (ED, ("tail.1.weight", "tail.1.bias")),
}
UNTOUCHED = {
    "dec_entry": ("conv1.weight",), "dec_entry_engine": ("conv1.weight",), "dec_tail": ("last_conv.4.bias",), "head": (),
    "resblock": ("body.0.body.2.bias",), "body_close": (f"body.{DEPTH}.weight", f"body.{DEPTH}.bias"),
    "up": ("tail.0.0.weight", "tail.0.0.bias"), "close": ("tail.1.weight", "tail.1.bias"), "walk": ("tail.1.bias",),
}


class Case(NamedTuple):
    id: str
    kind: str
    B: int
    H: int                          # the unit's own (input) grid
    W: int
    dtype: torch.dtype
    ch: int                         # output channels of the closing convolution of the parameter set


def _dt(dtype):
    return "bf16" if dtype == BF else "f32"


def _c(kind, B, H, W, dtype, ch=4):
    sfx = f"-ch{ch}" if kind == "close" else ""
    return Case(f"{kind}{sfx}-B{B}-{H}x{W}-{_dt(dtype)}", kind, B, H, W, dtype, ch)


def _cases():
    out = []
    for dt in (BF, F32):
        out += [_c("dec_entry", 2, 8, 12, dt), _c("dec_entry", 1, 6, 10, dt), _c("dec_entry_engine", 2, 8, 12, dt)]
        out += [_c("dec_tail", 2, 8, 12, dt), _c("dec_tail", 1, 6, 10, dt)]
        for kind in ("head", "resblock", "body_close"):
            out += [_c(kind, 2, 7, 6, dt), _c(kind, 1, 10, 36, dt), _c(kind, 1, 18, 34, dt)]
        out += [_c("up", 2, 7, 6, dt), _c("up", 1, 10, 36, dt)]
        for ch in (3, 4):
            out += [_c("close", 2, 7, 6, dt, ch), _c("close", 1, 18, 34, dt, ch)]
    out += [_c("close", 1, 10, 36, BF, 8), _c("close", 1, 10, 36, BF, 12)]
    for dt in (BF, F32):
        out += [_c("walk", 1, 7, 6, dt), _c("walk", 2, 10, 12, dt)]
    return tuple(out)


CASES = _cases()


# ------------------------------------------------------------------ which kernel ran: the launches of a unit, by family
NT = ("gemm_nt3_kernel", "gemm_nt_kernel", "gemm_as_kernel", "gemm_bs_kernel")
TN = ("gemm_tn3_kernel", "gemm_tn_kernel", "gemm_tn2_kernel")
SINGLE = ("conv3_c64_kernel", "conv3_c64_wgrad_kernel", "conv3_c64_wgrad_reduce_kernel", "conv3_n8_fwd_kernel", "conv3_n8_dgrad_kernel",
          "conv3_n8_wgrad_kernel", "conv3_n8_wgrad_reduce_kernel", "bilinear_up2_fwd_kernel", "bilinear_up2_bwd_kernel",
          "pixel_shuffle2_kernel", "nchw_from_rows_kernel", "rows_from_nchw_kernel", "gather_sum_rows_kernel")
ADD = ("add_rows_kernel", "add_small_f32_kernel")        # (the second: one f32 row shorter than 16 bytes, a 3-channel bias gradient)


def family(name: str) -> Optional[str]:
    base = name.split("<")[0]
    if base in NT:
        return "gemm_nt"
    if base in TN:
        return "gemm_tn"
    if base in ADD:
        return "add_rows_kernel"
    return base if base in SINGLE else None


def _c64(n):            # n 64 -> 64 convolutions on the direct kernels, each way: forward | input gradient, weight gradient + its reduce
    return ({"conv3_c64_kernel": n}, {"conv3_c64_kernel": n, "conv3_c64_wgrad_kernel": n, "conv3_c64_wgrad_reduce_kernel": n})


def _gemm(n, n_dx=None):
    return ({"gemm_nt": n}, {"gemm_tn": n, "gemm_nt": n if n_dx is None else n_dx})


def _plus(a, b):
    return tuple({k: x.get(k, 0) + y.get(k, 0) for k in set(x) | set(y)} for x, y in zip(a, b))


_N8 = ({"conv3_n8_fwd_kernel": 1}, {"conv3_n8_dgrad_kernel": 1, "conv3_n8_wgrad_kernel": 1, "conv3_n8_wgrad_reduce_kernel": 1})
_LAYOUT = ({"nchw_from_rows_kernel": 1}, {"rows_from_nchw_kernel": 1})
_PAD_ADD = ({}, {"add_rows_kernel": 2})                 # dw_pad and db_pad added to the gradients
_DEC_ENTRY = _plus(_gemm(2), ({"bilinear_up2_fwd_kernel": 1}, {"bilinear_up2_bwd_kernel": 1}))
_DEC_TAIL = _gemm(3, 4)                                 # input gradients: g.d2, g.d1 and the two slices g.cu, g.a
_CHAIN_ADD = ({}, {"add_rows_kernel": 1})               # add_rows(dr, d_rb)
_SHUFFLE = ({"pixel_shuffle2_kernel": 1}, {"pixel_shuffle2_kernel": 1})
_CLOSE_F32 = _plus(_plus(_gemm(1), _LAYOUT), _PAD_ADD)
# (kind, dtype, ch of a closing convolution or None) -> (forward launches, backward launches) by family; stated by hand from
# what each unit is, not from the route's predicates.  Families that are absent must not launch.
EXPECTED = {
    ("dec_entry", BF, None): _DEC_ENTRY, ("dec_entry", F32, None): _DEC_ENTRY,
    ("dec_entry_engine", BF, None): _DEC_ENTRY, ("dec_entry_engine", F32, None): _DEC_ENTRY,
    ("dec_tail", BF, None): _DEC_TAIL, ("dec_tail", F32, None): _DEC_TAIL,
    ("head", BF, None): _plus(_c64(1), _CHAIN_ADD), ("head", F32, None): _plus(_gemm(1), _CHAIN_ADD),
    ("resblock", BF, None): _c64(2), ("resblock", F32, None): _gemm(2),
    ("body_close", BF, None): _c64(1), ("body_close", F32, None): _gemm(1),
    ("up", BF, None): _c64(4), ("up", F32, None): _plus(_gemm(1), _SHUFFLE),
    ("close", BF, 3): _N8, ("close", BF, 4): _N8, ("close", BF, 8): _plus(_N8, _LAYOUT),
    ("close", BF, 12): _plus(_plus(_gemm(1), _LAYOUT), _PAD_ADD),
    ("close", F32, 3): _CLOSE_F32, ("close", F32, 4): _CLOSE_F32,
    # EDSR(depth 2): head, 2 x 2 ResBlock convolutions, the body's closing one, 3 stages (4 plane launches each), the closing one
    ("walk", BF, None): _plus(_plus(_c64(1 + 2 * DEPTH + 1 + 3 * 4), _N8), _CHAIN_ADD),
    ("walk", F32, None): _plus(_plus(_plus(_gemm(1 + 2 * DEPTH + 1 + 3), _plus(_plus(_SHUFFLE, _SHUFFLE), _SHUFFLE)), _CLOSE_F32),
                               _CHAIN_ADD),
}


def expected(case: Case):
    f, b = EXPECTED[(case.kind, case.dtype, case.ch if case.kind == "close" else None)]
    return {k: v for k, v in f.items() if v}, {k: v for k, v in b.items() if v}


# ------------------------------------------------------------------ parameters and inputs
_params: Dict[int, dict] = {}


def params(ch: int) -> dict:
    """the procedural f32 parameters of DeepLab(ch, 128, 512) with EDSR depth 2, names relative to the module"""
    if ch not in _params:
        from oracle import ref_torch as R
        S = importlib.import_module(PKG + ".sr")
        _params[ch] = R.procedural_from_shapes(S.sr_param_shapes(ch, C1, C2, DEPTH))
    return _params[ch]


def param_names(case: Case) -> Tuple[str, Tuple[str, ...]]:
    """(prefix, names below it) of the parameters the unit owns"""
    if case.kind == "walk":
        return ED, tuple(n[len(ED):] for n in params(case.ch) if n.startswith(ED))
    return UNIT_PARAMS[case.kind]


def ref_params(case: Case) -> Dict[str, torch.Tensor]:
    """float64 leaves under their full names, as the route reads them: weights rounded to bf16 on the bf16 path, biases f32"""
    pre, names = param_names(case)
    out = {}
    for n in names:
        v = params(case.ch)[pre + n]
        if case.dtype == BF and n.endswith(".weight"):
            v = v.to(BF)
        out[pre + n] = v.double().clone().requires_grad_(True)
    return out


def _randn_seeded(seed: int, *shape) -> torch.Tensor:
    """N(0, 1) rounded to bf16 (exact in either run dtype), as f32, from a seeded CPU generator"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=gen).to(BF).float()


def tok(t: torch.Tensor) -> torch.Tensor:          # NCHW -> token-major [B*H*W][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def nchw(t: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def up2(t: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """nearest x2 of a token-major [B*H*W][C] tensor, token-major on the 2H x 2W grid"""
    return t.view(B, H, W, -1).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(B * 4 * H * W, -1)


_inputs: Dict[tuple, dict] = {}


def inputs(case: Case) -> Dict[str, torch.Tensor]:
    """The operands of a case, token-major f32 (NCHW for the float32 output gradient "dy_nchw"), all exact in bf16."""
    key = (case.kind, case.B, case.H, case.W, case.dtype, case.ch)
    if key in _inputs:
        return _inputs[key]
    B, H, W = case.B, case.H, case.W
    M = B * H * W
    k = case.kind
    _randn = lambda seed, *shape: _randn_seeded(seed + SEED_SHIFT.get(k, 0), *shape)
    if k in ("dec_entry", "dec_entry_engine"):
        h, w = H // 2, W // 2
        if k == "dec_entry":
            t = {"low": _randn(SEED_X, M, C1), "x": _randn(SEED_X2, B * h * w, C2)}
        else:
            # the engine's taps for the default head: low = Upsample(128 @ H/2), x = Concat(Upsample(256 @ h/2), 256 @ h)
            t = {"low_half": _randn(SEED_X, B * h * w, C1), "xa_half": _randn(SEED_X2, B * (h // 2) * (w // 2), C2 // 2),
                 "xb": _randn(SEED_X2 + 10, B * h * w, C2 // 2)}
            t["low"] = up2(t["low_half"], B, h, w)
            t["x"] = torch.cat((up2(t["xa_half"], B, h // 2, w // 2), t["xb"]), 1)
        # the route hands g.a over behind the low-level ReLU's mask (the last_conv.0 launch applies it): the given gradient is
        # masked with the exact unit's own mask, which autograd then applies a second time without effect
        w1 = params(case.ch)[DEC + "conv1.weight"]
        w1 = (w1.to(BF) if case.dtype == BF else w1).double()
        mask = tok(F.conv2d(nchw(t["low"].double(), B, H, W), w1)) > 0
        t["dcu"] = _randn(SEED_DY, M, CX)
        t["da"] = _randn(SEED_DY2, M, CA) * mask
    elif k == "dec_tail":
        t = {"cat_x": _randn(SEED_X, M, CX).relu(), "a_pre": _randn(SEED_X2, M, CA), "dy": _randn(SEED_DY, M, 64)}
    elif k == "head":
        t = {"x": _randn(SEED_X, M, 64), "dr": _randn(SEED_DY, M, 64), "d_rb": _randn(SEED_DY2, M, 64)}
    elif k in ("resblock", "body_close"):
        t = {"x": _randn(SEED_X, M, 64), "dy": _randn(SEED_DY, M, 64)}
        if k == "body_close":
            t["h"] = _randn(SEED_X2, M, 64)
    elif k == "up":
        t = {"x": _randn(SEED_X, M, 64), "dy": _randn(SEED_DY, 4 * M, 64)}
    elif k == "close":
        t = {"x": _randn(SEED_X, M, 64), "dy_nchw": _randn(SEED_DY, B, case.ch, H, W)}
    else:
        t = {"x": _randn(SEED_X, M, 64), "dy_nchw": _randn(SEED_DY, B, case.ch, 8 * H, 8 * W)}
    _inputs[key] = t
    return t


# ------------------------------------------------------------------ subsets
def rows_yx(B: int, H: int, W: int):
    y = torch.arange(H).view(1, H, 1).expand(B, H, W).reshape(-1)
    x = torch.arange(W).view(1, 1, W).expand(B, H, W).reshape(-1)
    return y, x


def border_masks(B: int, H: int, W: int) -> Dict[str, torch.Tensor]:
    y, x = rows_yx(B, H, W)
    return {"top": y == 0, "bottom": y == H - 1, "left": x == 0, "right": x == W - 1}


def parity_masks(B: int, H: int, W: int) -> Dict[str, torch.Tensor]:
    y, x = rows_yx(B, H, W)
    return {f"p{py}{px}": ((y & 1) == py) & ((x & 1) == px) for py in (0, 1) for px in (0, 1)}


def out_scale(case: Case) -> int:
    """the output grid is the input grid times this"""
    return {"up": 2, "walk": 8}.get(case.kind, 1)


def map_fields(case: Case) -> Tuple[Tuple[str, ...], Tuple[str, ...]]:
    """(tensors on the output grid, tensors on the input grid) that take the border subsets"""
    if case.kind == "dec_tail":
        return ("out",), ("g.cu", "g.a")
    return ("out",), ("din",)


def subset(case: Case, base: str, sub: str, t: torch.Tensor) -> torch.Tensor:
    """the subset `sub` of tensor `base` of a case (t: the whole tensor, on any device)"""
    B, H, W = case.B, case.H, case.W
    if sub.startswith("p"):                         # Upsampler stage parities
        p = 2 * int(sub[1]) + int(sub[2])
        if base == "out":
            return t[parity_masks(B, 2 * H, 2 * W)[sub].to(t.device)]
        return t[p::4]                              # weight / bias gradient rows 4 c + p
    s = out_scale(case) if base in map_fields(case)[0] else 1
    return t[border_masks(B, s * H, s * W)[sub].to(t.device)]


def subset_names(case: Case, have) -> Tuple[str, ...]:
    out = []
    if case.kind in HAS_3X3:
        outs, ins = map_fields(case)
        out += [f"{k}[{s}]" for k in outs + ins if k in have for s in ("top", "bottom", "left", "right")]
    if case.kind == "up":
        out += [f"{k}[p{a}{b}]" for k in ("out", "tail.0.0.weight", "tail.0.0.bias") for a in (0, 1) for b in (0, 1)]
    return tuple(out)


def with_subsets(t: Dict[str, torch.Tensor], case: Case) -> Dict[str, torch.Tensor]:
    out = dict(t)
    for name in subset_names(case, t):
        base, sub = name[:-1].split("[")
        out[name] = subset(case, base, sub, t[base])
    return out


def untouched(case: Case, name: str) -> bool:
    """tensors that no store point of reference B can reach (see the module docstring)"""
    base = name.split("[")[0]
    if case.kind == "close" and base == "out":
        return case.ch <= NCHW_DIRECT_MAX_CH
    return base in UNTOUCHED[case.kind]


# ------------------------------------------------------------------ references of one unit
class _NarrowGrad(torch.autograd.Function):
    """the value as it is; its gradient through bf16 (a float32 tensor the route writes itself and whose gradient it reads narrowed)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


def store_of(case: Case):
    """the `store=` callable of reference B of this case: every store point narrows, the closing convolution's "y" by its form"""
    def store(t, name):
        if name == ED + "y" and case.ch <= NCHW_DIRECT_MAX_CH:
            return _NarrowGrad.apply(t)
        return narrow(t, name)
    return store


def run_reference(case: Case, store) -> Dict[str, torch.Tensor]:
    """One float64 forward and backward of the unit.  Maps are token-major; parameter gradients under their names below the prefix."""
    from oracle import ref_torch as R
    B, H, W = case.B, case.H, case.W
    t = {k: v.double() for k, v in inputs(case).items()}
    sd = ref_params(case)
    st = store if store is not None else (lambda v, name: v)
    k = case.kind
    leaf = lambda v, h=H, w=W: nchw(v, B, h, w).clone().requires_grad_(True)
    out = {}
    if k in ("dec_entry", "dec_entry_engine"):
        low, x = leaf(t["low"]), leaf(t["x"], H // 2, W // 2)
        cat = R.sr_decoder_entry(sd, DEC, x, low, 2, store)
        cat.backward(nchw(torch.cat((t["dcu"], t["da"]), 1), B, H, W))
        c = tok(cat.detach())
        out = {"cat.x": c[:, :CX], "cat.a": c[:, CX:], "d_low": tok(low.grad), "d_x": tok(x.grad)}
    elif k == "dec_tail":
        cx, ap = leaf(t["cat_x"]), leaf(t["a_pre"])
        y = R.sr_decoder_tail(sd, DEC, torch.cat((st(cx, DEC + "cat.x"), st(F.relu(ap), DEC + "a")), 1), store)
        y.backward(nchw(t["dy"], B, H, W))
        out = {"out": tok(y.detach()), "g.cu": tok(cx.grad), "g.a": tok(ap.grad)}
    elif k == "walk":
        x = leaf(t["x"])
        y = R.edsr(sd, ED, x, store)
        y.backward(t["dy_nchw"])
        out = {"out": tok(y.detach()), "din": tok(x.grad)}
    else:
        x = leaf(t["x"])
        if k == "head":
            y, g = R.edsr_head(sd, ED, x, store), t["dr"] + t["d_rb"]
        elif k == "resblock":
            y, g = R.edsr_resblock(sd, ED, 0, st(x, ED + "x"), store), t["dy"]
        elif k == "body_close":
            y, g = R.edsr_body_close(sd, ED, DEPTH, st(x, ED + "x"), nchw(t["h"], B, H, W), store), t["dy"]
        elif k == "up":
            y, g = R.edsr_upsampler_stage(sd, ED, 0, st(x, ED + "x"), store), t["dy"]
        else:
            y, g = R.edsr_close(sd, ED, st(x, ED + "x"), store), None
        s = out_scale(case)
        gy = t["dy_nchw"] if g is None else nchw(g, B, s * H, s * W)
        if k == "up":                               # the input gradient of each plane alone
            for name, rows in parity_masks(B, 2 * H, 2 * W).items():
                gp = nchw(t["dy"] * rows.view(-1, 1), B, 2 * H, 2 * W)
                out[f"din[{name}]"] = tok(torch.autograd.grad(y, x, gp, retain_graph=True)[0])
        y.backward(gy)
        out.update({"out": tok(y.detach()), "din": tok(x.grad)})
    pre, names = param_names(case)
    out.update({n: sd[pre + n].grad for n in names})
    return out


class Reference(NamedTuple):
    A: Dict[str, torch.Tensor]          # tensor name (subsets as "out[top]", "out[p01]", ...) -> float64 value
    e_emul: Dict[str, float]            # bf16 only


_refs: Dict[tuple, Reference] = {}


def reference(case: Case) -> Reference:
    key = (case.kind, case.B, case.H, case.W, case.dtype, case.ch)
    if key not in _refs:
        A = with_subsets(run_reference(case, None), case)
        e = {}
        if case.dtype == BF:
            Bt = with_subsets(run_reference(case, store_of(case)), case)
            e = {k: rel_l2(Bt[k], A[k]) for k in A}
        _refs[key] = Reference(A, e)
    return _refs[key]


def gate(case: Case, ref: Reference, name: str) -> float:
    return F32_GATE if case.dtype == F32 else MARGIN * ref.e_emul[name] + FLOOR


def check_reference(case: Case, ref: Reference) -> None:
    """The conditions on the reference alone: |T_A| > 0 and 0 < e_emul(T) <= 5e-2 for every gated tensor a store point
    reaches, e_emul == 0 for the others."""
    for k, a in ref.A.items():
        assert float(a.norm()) > 0, (case.id, k)
        if case.dtype != BF:
            continue
        if untouched(case, k):
            assert ref.e_emul[k] == 0.0, (case.id, k, ref.e_emul[k])
        else:
            assert 0 < ref.e_emul[k] <= E_EMUL_MAX, (case.id, k, ref.e_emul[k])


def group_of(name: str) -> str:
    """the column of the summary tables a tensor belongs to"""
    base = name.split("[")[0]
    if base in ("out", "cat.x", "cat.a"):
        return "out"
    if base in ("din", "d_low", "d_x", "g.cu", "g.a"):
        return "din"
    return "bias" if base.endswith(".bias") else "weight"


if __name__ == "__main__":
    import time
    for c in CASES:
        if c.dtype != BF:
            continue
        t0 = time.time()
        r = reference(c)
        check_reference(c, r)
        print(f"# {c.id} ({time.time() - t0:.1f} s)")
        for k, v in r.e_emul.items():
            print(f"{k:34s} e_emul {v:.3e}   gate {MARGIN * v + FLOOR:.3e}{'   (untouched)' if untouched(c, k) else ''}")
