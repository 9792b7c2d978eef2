"""Shared helpers of tests/test_gemm_exact_gpu.py: exact-arithmetic GEMM operands, NaN-poisoned operand views, sentinel-filled
output buffers, the bitwise f64 reference and the kernel-name probe.

Why bitwise equality holds: every operand is a small integer, so every product a kernel forms is exact in f32 and every
partial sum stays below 2^24 in magnitude whatever the accumulation order (the bound is written next to each generator).
The f64 reference is then the exact value, `.float()` is exact, and the output dtype cast is torch's round-to-nearest-even,
the same rule as the kernels' single store (v_cvt_pk_bf16_f32, csrc/common.h).  A kernel that drops, duplicates, misplaces
or double-rounds one element differs in its bits."""
from __future__ import annotations

import math
import re
from typing import List, Optional, Sequence, Tuple

import torch

BF16_SENTINEL = -0x4A3D            # 0xB5C3 as int16: a bf16 (-1.45e-6) no case here produces
F32_SENTINEL = -0x4A3C5A5B          # 0xB5C3A5A5 as int32

GEMM_KERNELS = ("gemm_nt3_kernel", "gemm_tn3_kernel", "tn3_reduce_kernel", "gemm_nt_kernel", "gemm_as_kernel", "gemm_bs_kernel",
                "gemm_tn_kernel", "gemm_tn2_kernel")


# ------------------------------------------------------------------ operands
def ints(shape, lim: int, seed: int, dev, dtype=torch.float32) -> torch.Tensor:
    """Uniform integers in [-lim, lim].  Exactness bound used by the callers: |a|, |w| <= 4 and K <= 4096 keep every partial
    sum of A @ W^T at |sum| <= 16 K <= 2^16, and integers of magnitude <= 256 are exact in bf16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).to(dtype).to(dev)


def poisoned(vals: torch.Tensor, dtype, *, ld: Optional[int] = None, col0: int = 0, row0: int = 0, pad_rows: int = 3):
    """A NaN-filled [row0 + rows + pad_rows][ld] buffer with vals at rows row0.., columns col0..; returns (buffer, view)."""
    rows, cols = vals.shape
    ld = cols + col0 if ld is None else ld
    assert col0 + cols <= ld
    buf = torch.full((row0 + rows + pad_rows, ld), float("nan"), device=vals.device, dtype=dtype)
    buf[row0:row0 + rows, col0:col0 + cols] = vals.to(dtype)
    return buf, buf[row0:row0 + rows, col0:col0 + cols]


def int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def sentinel_buffer(rows: int, ld: int, dtype, dev) -> torch.Tensor:
    buf = torch.empty((rows, ld), device=dev, dtype=dtype)
    int_view(buf).fill_(BF16_SENTINEL if buf.element_size() == 2 else F32_SENTINEL)
    return buf


def sentinel_of(buf: torch.Tensor) -> int:
    return BF16_SENTINEL if buf.element_size() == 2 else F32_SENTINEL


# ------------------------------------------------------------------ reference
def rne(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """f64 -> f32 (exact for the integer data here: asserted) -> dtype by torch's round-to-nearest-even."""
    r32 = ref64.float()
    ok = torch.isnan(ref64) | (r32.double() == ref64)
    assert bool(ok.all()), "reference is not exact in f32: the case breaks its own exactness bound"
    return r32.to(dtype)


def gather_a(segs: Sequence[dict], M: int, spatial: Optional[Tuple[int, int]]) -> torch.Tensor:
    """The implicit A[M][K] (f64) of a K-segment list (include/sodt_hip.h, sodt_seg): each dict has the SegSpec fields plus
    'buf' (the whole source buffer, rows x ld)."""
    cols = []
    dev = segs[0]["buf"].device
    m = torch.arange(M, device=dev)
    for s in segs:
        src = s["buf"].double()[:, s["coff"]:s["coff"] + s["klen"]]
        if spatial is None:
            cols.append(src[:M])
            continue
        Ho, Wo = spatial
        b, rem = m // (Ho * Wo), m % (Ho * Wo)
        y, x = rem // Wo, rem % Wo
        yy, xx = y * s.get("mul", 1) + s.get("dy", 0), x * s.get("mul", 1) + s.get("dx", 0)
        yi, xi = yy >> s.get("shr", 0), xx >> s.get("shr", 0)
        ok = (yy >= 0) & (xx >= 0) & (yi < s["Hi"]) & (xi < s["Wi"])
        row = torch.where(ok, (b * s["Hi"] + yi.clamp(min=0)) * s["Wi"] + xi.clamp(min=0), torch.zeros_like(m))
        g = src[row]
        g[~ok] = 0.0
        cols.append(g)
    return torch.cat(cols, 1)


def segspecs(ops, segs: Sequence[dict]):
    return [ops.SegSpec(s["buf"], s["klen"], s["coff"], s.get("dy", 0), s.get("dx", 0), s.get("mul", 1), s.get("shr", 0),
                        s.get("Hi", 0), s.get("Wi", 0)) for s in segs]


# ------------------------------------------------------------------ assertions
def first_mismatch(got: torch.Tensor, want: torch.Tensor, tile: Tuple[int, int]) -> str:
    gi, wi = int_view(got.contiguous()), int_view(want.contiguous())
    bad = (gi != wi).nonzero()
    r, c = int(bad[0, 0]), int(bad[0, 1])
    return (f"{bad.shape[0]} of {gi.numel()} elements differ; first at (row {r}, col {c}) = tile ({r // tile[0]}, {c // tile[1]}):"
            f" got {float(got[r, c])!r}, want {float(want[r, c])!r}")


def assert_bits(got: torch.Tensor, want: torch.Tensor, what: str, tile: Tuple[int, int] = (256, 192)) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(int_view(got.contiguous()), int_view(want.contiguous())):
        raise AssertionError(f"{what}: {first_mismatch(got, want, tile)}")


def assert_sentinel_outside(buf: torch.Tensor, rows: slice, cols: slice, what: str) -> None:
    """Every element of buf outside [rows, cols] still holds the sentinel bit pattern."""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[rows, cols] = False
    iv = int_view(buf)
    bad = (iv != sentinel_of(buf)) & mask
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements written outside the output view; first at buffer (row {r}, col {c})")


def assert_within(got: torch.Tensor, want64: torch.Tensor, bound64: torch.Tensor, what: str) -> None:
    """|got - want| <= bound element-wise (f64), with the worst element reported."""
    err = (got.double() - want64).abs()
    ok = err <= bound64
    if not bool(ok.all()):
        ratio = torch.where(ok, torch.zeros_like(err), err / bound64.clamp(min=1e-300))
        i = int(ratio.flatten().argmax())
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)]
        raise AssertionError(f"{what}: {int((~ok).sum())} elements outside the documented bound; worst at {idx}: got "
                             f"{float(got[tuple(idx)])!r}, want {float(want64[tuple(idx)])!r}, |err| {float(err[tuple(idx)]):.3e} > "
                             f"bound {float(bound64[tuple(idx)]):.3e}")


# ------------------------------------------------------------------ activations (f64) and their documented error
def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.special.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def silu64(x):
    return x * torch.sigmoid(x)


# unit roundoff of a round-to-nearest store: |RNE(y) - y| <= u |y| with u = 2^-p for p significand bits (bf16 8, f32 24).  (2^-9
# would be the half-ulp relative to the TOP of a binade; at the bottom, e.g. gelu(-1) = -0.15866 -> bf16 -0.15820, it is 2^-8.)
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
# the kernels' f32 arithmetic flushes subnormals (an f32-subnormal argument or result may come back as zero): an absolute floor
FTZ = 2.0 ** -126

# csrc/common.h:
#   bf16 path: erf_poly |err| <= 4.2e-5 for |x / sqrt 2| <= 2.7, <= 1.8e-4 on the clamped tail (both evaluated in f32);
#              dgelu_t<bf16> |err| <= 2.8e-4 (evaluated in f32, clamped tail included).
#   f32 path:  erf_gauss |err| <= 1.5e-7 + 2^-22 (A-S 7.1.26 plus its f32 evaluation), and gelu'(x) = (1 + erf)/2 + x phi(x) with
#              phi from the same exp, so |err| <= (1.5e-7 + 2^-22) / 2 + |x| phi(x) 2^-22.
#   sigmoid_f (both paths): v_exp_f32 / v_rcp_f32 at 1 ulp plus the rounding of the exp argument x log2(e): relative error of
#              sigmoid <= (1 - sigmoid) (|x| + 3) 2^-24, so |silu err| <= |silu(x)| (1 - sigmoid(x)) (|x| + 3) 2^-24 + |silu| 2^-24.
ERF_BF16_IN, ERF_BF16_TAIL, DGELU_BF16 = 4.2e-5, 1.8e-4, 2.8e-4
ERF_F32 = 1.5e-7 + 2.0 ** -22


def act_bound(kind: str, dtype, x: torch.Tensor) -> torch.Tensor:
    """documented_abs_err(f, x) + u_out (|f(x)| + documented_abs_err) for one activation evaluated at x (f64)."""
    x = x.double()
    ax = x.abs()
    f32ulp = 2.0 ** -24
    if kind == "gelu":
        f = gelu64(x)
        if dtype == torch.bfloat16:
            e_erf = torch.where(ax / math.sqrt(2.0) <= 2.7, torch.full_like(x, ERF_BF16_IN), torch.full_like(x, ERF_BF16_TAIL))
        else:
            e_erf = torch.full_like(x, ERF_F32)
        # gelu = x/2 (1 + erf): the erf error scaled by |x|/2, plus the f32 rounding of the products / sum (2 ulp of |x|)
        e = 0.5 * ax * e_erf + 2 * f32ulp * ax
    elif kind == "dgelu":
        f = dgelu64(x)
        if dtype == torch.bfloat16:
            e = torch.full_like(x, DGELU_BF16)
        else:
            e = 0.5 * ERF_F32 + ax * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi) * 2.0 ** -22 + 2 * f32ulp
    elif kind == "silu":
        f = silu64(x)
        s = torch.sigmoid(x)
        e = f.abs() * ((1 - s) * (ax + 3) * f32ulp + f32ulp)
    else:
        raise ValueError(kind)
    return e + U_OUT[dtype] * (f.abs() + e) + FTZ


def finite_bf16_in(lo: float, hi: float, dev) -> torch.Tensor:
    """Every finite bf16 value in [lo, hi] (as f32)."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    v = v[torch.isfinite(v) & (v >= lo) & (v <= hi)]
    return torch.unique(v).to(dev)


# ------------------------------------------------------------------ which kernel ran
def _demangle_args(s: str) -> List[str]:
    out, i = [], 0
    while i < len(s) and s[i] != "E":         # (the template argument list ends at a bare E)
        if s.startswith("DF16b", i):
            out.append("bf16"); i += 5
        elif s[i] == "f":
            out.append("float"); i += 1
        elif s.startswith("Lb", i):
            out.append("true" if s[i + 2] == "1" else "false"); i = s.index("E", i) + 1
        elif s.startswith("Li", i):
            v = s[i + 2:s.index("E", i)]
            out.append(str(-int(v[1:])) if v.startswith("n") else v); i = s.index("E", i) + 1
        else:
            raise ValueError(f"cannot read template arguments {s!r}")
    return out


# torch's demangler (the profiler's names) mis-reads the bf16 type (DF16b) in front of some integer template arguments and
# returns these strings instead of failing; they stand for exactly one instantiation each
_GARBLED = {"gemm_nt_kernel<bool _Accum, int, E>": "gemm_nt_kernel<bf16, 1>",
            "gemm_nt_kernel<bool _Accum, int, __int128, E>": "gemm_nt_kernel<bf16, -1>"}


def canonical_kernel(name: str) -> str:
    """'void (anonymous namespace)::gemm_nt3_kernel<0, false, 2>(sodt_gemm_args)' or its mangled form -> 'gemm_nt3_kernel<0, false, 2>'."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if m:
        n = int(m.group(1))
        rest = name[m.end():]
        base, rest = rest[:n], rest[n:]
        if rest.startswith("I"):
            return f"{base}<{', '.join(_demangle_args(rest[1:]))}>"
        return base
    m = re.search(r"(?:::)?(\w+)(<[^()]*>)?\(", name)
    if not m:
        return name
    base, targs = m.group(1), m.group(2) or ""
    targs = targs.replace("__bf16", "bf16")
    if "_Accum" in targs:        # (an unknown garbled GEMM name matches no expected instantiation, so its case fails by name)
        return _GARBLED.get(base + targs, base + "<unreadable>")
    return base + targs


def launched_kernels(fn) -> List[str]:
    """Canonical names of the GPU kernels fn launches (torch.profiler over HIP), in launch order."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [canonical_kernel(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def gemm_kernels(names: Sequence[str]) -> List[str]:
    return [n for n in names if n.split("<")[0] in GEMM_KERNELS]


def run_expecting(fn, expect: Sequence[str]) -> None:
    """Run fn once under the profiler and require its GEMM kernels to be exactly `expect` (in launch order)."""
    got = gemm_kernels(launched_kernels(fn))
    assert got == list(expect), f"GEMM route: launched {got}, the case was written for {list(expect)}"


# expected instantiation names (the template argument spelling of canonical_kernel)
def nt3(cf: int, osc: bool = False, nv: int = 3) -> str:
    return f"gemm_nt3_kernel<{cf}, {'true' if osc else 'false'}, {nv}>"


def tn3(swap: bool, spatial: bool) -> str:
    return f"gemm_tn3_kernel<{'true' if swap else 'false'}, {'true' if spatial else 'false'}>"


def _ty(dt) -> str:
    return "bf16" if dt == torch.bfloat16 else "float"


def bs(dt, stats: bool, cf: int, simple: bool) -> str:
    return f"gemm_bs_kernel<{_ty(dt)}, 128, {'true' if stats else 'false'}, {cf}, {'true' if simple else 'false'}>"


def as_(dt) -> str:
    return f"gemm_as_kernel<{_ty(dt)}, 128>"


def ntk(dt, cf: int) -> str:
    return f"gemm_nt_kernel<{_ty(dt)}, {cf}>"


def tn2(dt) -> str:
    return f"gemm_tn2_kernel<{_ty(dt)}>"


def tnk(dt) -> str:
    return f"gemm_tn_kernel<{_ty(dt)}>"


TN3_REDUCE = "tn3_reduce_kernel"
