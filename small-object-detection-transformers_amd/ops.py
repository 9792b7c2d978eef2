"""Thin Python wrappers over the C ABI (include/sodt_hip.h).

Every wrapper builds the argument record once, launches on torch's current stream and,
when a ``Recorder`` is active, also appends ``(cfunc, args)`` to it so that the engine
can replay a whole forward / backward with ~1 us of host work per kernel (shapes and
buffers are static per (batch, resolution, dtype) plan).  PyTorch is used only for
device memory and streams.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L

_lib = L.load()

_active_recorder: Optional[list] = None


class Recorder:
    """with Recorder() as rec: ...ops...  -> rec.calls can be replayed with replay()."""

    def __init__(self):
        self.calls: List[Tuple] = []
        self.keep: List = []       # tensors / structs that must outlive the plan

    def __enter__(self):
        global _active_recorder
        assert _active_recorder is None, "nested recorders are not supported"
        _active_recorder = self.calls
        return self

    def __exit__(self, *exc):
        global _active_recorder
        _active_recorder = None
        return False


def recorded_count() -> Optional[int]:
    """Launches recorded so far by the active Recorder (None outside one): lets the engine mark split points."""
    return None if _active_recorder is None else len(_active_recorder)


_tag: str = ""          # label attached to recorded launches (set by the engine, read by bench probes)


def set_tag(tag: str) -> None:
    global _tag
    _tag = tag


def replay(calls: Sequence[Tuple], stream: Optional[int] = None, probes: Optional[dict] = None,
           start: int = 0, end: Optional[int] = None) -> None:
    """Re-issue recorded launches [start, end).  probes: {call index: (start_event, end_event)} -> the events are
    recorded on the launch stream around that one kernel (bench.py's live roofline measurement)."""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    if start or end is not None:
        calls = calls[start:end]
    if probes:
        for i, (fn, args, name, tag) in enumerate(calls, start):
            pr = probes.get(i)
            if pr is not None:
                pr[0].record()
            rc = fn(*args, st)
            if pr is not None:
                pr[1].record()
            if rc != 0:
                raise RuntimeError(f"{name} failed with status {rc}")
        return
    for fn, args, name, tag in calls:
        rc = fn(*args, st)
        if rc != 0:
            raise RuntimeError(f"{name} [{tag}] failed with status {rc}")


def _launch(name: str, *args) -> None:
    fn = getattr(_lib, name)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = fn(*args, st)
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc} (unsupported shape/alignment, see include/sodt_hip.h)")
    if _active_recorder is not None:
        _active_recorder.append((fn, args, name, _tag))


def _ws_bytes(name: str, *args, hint: str = "see include/sodt_hip.h", msg: Optional[str] = None) -> int:
    """A ``sodt_*_workspace_bytes(..., size_t* bytes)`` query; a refusal raises ``msg``, or the status with ``hint``."""
    b = C.c_size_t(0)
    rc = getattr(_lib, name)(*args, C.byref(b))
    if rc != 0:
        raise RuntimeError(msg or f"{name} failed with status {rc}" + (f" ({hint})" if hint else ""))
    return int(b.value)


def dt_code(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return L.BF16
    if t.dtype == torch.float32:
        return L.F32
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class SegSpec:
    """One K-segment: a [rows][ld] token-major tensor view starting at channel ``coff``."""
    __slots__ = ("t", "klen", "coff", "dy", "dx", "mul", "shr", "Hi", "Wi", "ld")

    def __init__(self, t: torch.Tensor, klen: Optional[int] = None, coff: int = 0, dy: int = 0, dx: int = 0,
                 mul: int = 1, shr: int = 0, Hi: int = 0, Wi: int = 0, ld: Optional[int] = None):
        self.t = t
        self.ld = t.shape[-1] if ld is None else ld
        self.klen = (self.ld - coff) if klen is None else klen
        self.coff, self.dy, self.dx, self.mul, self.shr, self.Hi, self.Wi = coff, dy, dx, mul, shr, Hi, Wi


TAPS3 = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))     # (dy, dx) of a 3x3 convolution, kernel index (dy+1)*3 + dx+1


def _fill_aspec(a: L.ASpec, segs: Sequence[SegSpec], spatial: Optional[Tuple[int, int]]):
    assert 1 <= len(segs) <= L.MAX_SEG
    es = segs[0].t.element_size()
    for i, s in enumerate(segs):
        d = a.s[i]
        d.p = s.t.data_ptr() + s.coff * es
        d.ld, d.klen, d.dy, d.dx, d.mul, d.shr, d.Hi, d.Wi = s.ld, s.klen, s.dy, s.dx, s.mul, s.shr, s.Hi, s.Wi
    a.nseg = len(segs)
    if spatial is None:
        a.spatial, a.Ho, a.Wo = 0, 1, 1
    else:
        a.spatial, a.Ho, a.Wo = 1, spatial[0], spatial[1]


def gemm_nt(segs: Sequence[SegSpec], W: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, *,
            ldw: Optional[int] = None, ldc: Optional[int] = None, c_off: int = 0,
            spatial: Optional[Tuple[int, int]] = None, bias: Optional[torch.Tensor] = None,
            resid: Optional[torch.Tensor] = None, ldr: Optional[int] = None, r_off: int = 0, rmod: int = 0,
            gelu_out: Optional[torch.Tensor] = None, dgelu_aux: Optional[torch.Tensor] = None,
            stats: Optional[torch.Tensor] = None, affine: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
            out_f32: bool = False, detect: Optional[Tuple[int, int, int]] = None,
            oscatter: Optional[Tuple[int, int, int, int, int]] = None, w_off: int = 0,
            gelu_only: bool = False, dgelu_rc: bool = False, relu: bool = False, drelu_aux: Optional[torch.Tensor] = None, aux_off: int = 0) -> None:
    """out[M][N] = epilogue(concat_k(segs) @ W[N][K]^T); see SODT_EPI_* in include/sodt_hip.h."""
    g = L.GemmArgs()
    _fill_aspec(g.a, segs, spatial)
    es = W.element_size()
    g.W = W.data_ptr() + w_off * es
    g.ldw = W.shape[-1] if ldw is None else ldw
    oes = 4 if (out_f32 or detect is not None) else es
    g.C = out.data_ptr() + c_off * oes
    g.ldc = (out.shape[-1] if ldc is None else ldc)
    flags = 0
    if bias is not None:
        flags |= L.EPI_BIAS
        g.bias = bias.data_ptr()
    if resid is not None:
        flags |= L.EPI_RESID
        g.R = resid.data_ptr() + r_off * es
        g.ldr = resid.shape[-1] if ldr is None else ldr
        g.rmod = rmod
    if gelu_out is not None:
        flags |= L.EPI_GELU_DUAL
        g.C2 = gelu_out.data_ptr()
        g.ldc2 = gelu_out.shape[-1]
    if dgelu_aux is not None:
        flags |= L.EPI_DGELU
        g.aux = dgelu_aux.data_ptr()
        g.ldaux = dgelu_aux.shape[-1]
    if stats is not None:
        flags |= L.EPI_STATS
        g.stats = stats.data_ptr()
    if affine is not None:
        flags |= L.EPI_AFFINE_SILU
        g.scale, g.shift = affine[0].data_ptr(), affine[1].data_ptr()
    if out_f32:
        flags |= L.EPI_OUT_F32
    if detect is not None:
        flags |= L.EPI_DETECT
        g.det_na, g.det_no, g.det_hw = detect
    if oscatter is not None:
        g.oscatter = 1
        g.omul, g.ody, g.odx, g.OH, g.OW = oscatter
    if gelu_only:
        flags |= L.EPI_GELU
    if dgelu_rc:
        flags |= L.EPI_DGELU_RC
    if relu:
        flags |= L.EPI_RELU
    if drelu_aux is not None:       # gradient through a ReLU whose output is drelu_aux
        flags |= L.EPI_DRELU
        g.aux = drelu_aux.data_ptr() + aux_off * drelu_aux.element_size()
        g.ldaux = drelu_aux.shape[-1]
    g.M, g.N, g.K, g.flags = M, N, K, flags
    _launch("sodt_gemm_nt", C.byref(g), dt_code(W))


def mlp_recompute_ok(M: int, Cc: int, dtype: torch.dtype) -> bool:
    """Linear-GELU-Linear with only the activation saved (SODT_EPI_GELU forward, SODT_EPI_DGELU_RC backward): needs the
    pipelined bf16 kernel for N = 4C, K = 2C (csrc/gemm3.hip: N % 192 == 0, K-halves whole 64-wide steps, bias in LDS)."""
    return dtype == torch.bfloat16 and M >= 256 and (4 * Cc) % 192 == 0 and Cc % 64 == 0 and 4 * Cc <= 3072


def mlp_fused_ok(M: int, Cc: int, dtype: torch.dtype) -> bool:
    """sodt_mlp_fwd runs its fused kernel (csrc/mlp.hip) for this shape; otherwise it is the two-GEMM chain through hact."""
    return dtype == torch.bfloat16 and Cc == 192 and M >= 1


def mlp_fwd(xn: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
            resid: Optional[torch.Tensor], out: torch.Tensor, hact: Optional[torch.Tensor], M: int, Cc: int) -> None:
    """out = resid + fc2(GELU(fc1(xn))) (backbone_vit.py:884-890, :1128); hact (optional) receives GELU(fc1(xn)) [M][4C]."""
    assert xn.shape[-1] == Cc and out.shape[-1] == Cc and w1.shape == (4 * Cc, Cc) and w2.shape == (Cc, 4 * Cc)
    assert xn.is_contiguous() and out.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()
    assert w1.dtype == xn.dtype and w2.dtype == xn.dtype and b1.dtype == torch.float32 and b2.dtype == torch.float32
    assert resid is None or (resid.is_contiguous() and resid.shape[-1] == Cc and resid.dtype == xn.dtype)
    assert hact is None or (hact.is_contiguous() and hact.shape[-1] == 4 * Cc and hact.dtype == xn.dtype)
    _launch("sodt_mlp_fwd", _p(xn), _p(w1), _p(b1), _p(w2), _p(b2), _p(resid), _p(out), _p(hact), M, Cc, dt_code(xn))


# ---- 2x2-conv MLP with fc1 folded into the convolution (csrc/convmlp.hip)
def convmlp_compose(fc1_w, fc1_b, conv_w, conv_b, weff, weffT, beff, vtap, Cc):
    assert fc1_w.dtype == torch.float32 and conv_w.dtype == torch.float32 and fc1_w.is_contiguous() and conv_w.is_contiguous()
    assert tuple(conv_w.shape) == (Cc, Cc, 2, 2) and tuple(fc1_w.shape) == (Cc, Cc) and tuple(weff.shape) == (Cc, 4 * Cc) == tuple(weffT.shape)
    _launch("sodt_convmlp_compose", _p(fc1_w), _p(fc1_b), _p(conv_w), _p(conv_b), _p(weff), _p(weffT), _p(beff), _p(vtap), Cc, dt_code(weff))


def convmlp_border_fix(cp, ca, vtap, B, H, W, Cc):
    _launch("sodt_convmlp_border_fix", _p(cp), _p(ca), _p(vtap), B, H, W, Cc, dt_code(cp))


def convmlp_border_sums(dc, bs, B, H, W, Cc):
    _launch("sodt_convmlp_border_sums", _p(dc), _p(bs), B, H, W, Cc, dt_code(dc))


def convmlp_decompose(dweff, colsum, bs, fc1_w, fc1_b, conv_w, g_conv_w, g_conv_b, g_fc1_w, g_fc1_b, Cc):
    for t in (dweff, colsum, bs, fc1_w, fc1_b, conv_w, g_conv_w, g_conv_b, g_fc1_w, g_fc1_b):
        assert t.dtype == torch.float32 and t.is_contiguous()
    _launch("sodt_convmlp_decompose", _p(dweff), _p(colsum), _p(bs), _p(fc1_w), _p(fc1_b), _p(conv_w), _p(g_conv_w), _p(g_conv_b),
            _p(g_fc1_w), _p(g_fc1_b), Cc)


def tn_splits(M: int, N: int, K: int, bf16: bool = False) -> int:
    """M-slices per dW tile so that the grid is one full round of workgroups (no tail): 256 x 192 tiles at one
    workgroup per CU when the short side is <= 192, 128 x 128 tiles at two per CU otherwise (csrc/gemm.hip).
    bf16 (M >= 1024): the pipelined kernel of csrc/gemm3.hip - 256 x 192 tiles, the 256 side on whichever of
    N / K pads less, one workgroup per CU, at least 16 stages of 32 rows per workgroup."""
    if bf16 and M >= 1024 and N % 8 == 0 and K % 8 == 0:
        a = ((N + 255) // 256) * ((K + 191) // 192)
        b = ((K + 255) // 256) * ((N + 191) // 192)
        tiles = b if b * 256 * 192 < a * 256 * 192 else a
        return max(1, min(M // 512, max(1, 256 // tiles)))
    if N <= 192 or K <= 192:
        tiles, slots = ((N + 255) // 256) * ((K + 191) // 192), 256
    else:
        tiles, slots = ((N + 127) // 128) * ((K + 127) // 128), 1536
    return max(1, min(M // 256 if M >= 256 else 1, max(1, slots // tiles)))


_tn_scratch: Optional[torch.Tensor] = None


def set_tn_scratch(t: Optional[torch.Tensor]) -> None:
    """f32 device scratch for the weight-gradient partial tiles (sodt_gemm_tn_args.partial); kept alive here because
    recorded launch plans hold its address."""
    global _tn_scratch
    assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    _tn_scratch = t


def gemm_tn(dY: torch.Tensor, segs: Sequence[SegSpec], dW: torch.Tensor, M: int, N: int, K: int, *,
            ldy: Optional[int] = None, y_off: int = 0, spatial: Optional[Tuple[int, int]] = None,
            dbias: Optional[torch.Tensor] = None, lddw: Optional[int] = None, kperm: Optional[Tuple[int, int]] = None,
            splits: Optional[int] = None) -> None:
    """dW[N][K] (f32) += dY[M][N]^T @ concat_k(segs); dbias[N] += column sums of dY."""
    g = L.GemmTnArgs()
    g.dY = dY.data_ptr() + y_off * dY.element_size()
    g.ldy = dY.shape[-1] if ldy is None else ldy
    _fill_aspec(g.x, segs, spatial)
    assert dW.dtype == torch.float32
    g.dW = dW.data_ptr()
    g.lddw = K if lddw is None else lddw
    g.dbias = _p(dbias)
    g.M, g.N, g.K = M, N, K
    if kperm is not None:
        g.kperm_c, g.kperm_t = kperm
    g.splits = tn_splits(M, N, K, dY.dtype == torch.bfloat16) if splits is None else splits
    if _tn_scratch is not None and _tn_scratch.device == dY.device and g.splits > 1:
        g.partial, g.partial_floats = _tn_scratch.data_ptr(), _tn_scratch.numel()
    _launch("sodt_gemm_tn", C.byref(g), dt_code(dY))


def linear_bwd_sq(dY: torch.Tensor, X: torch.Tensor, wT: torch.Tensor, dX: torch.Tensor, dW: torch.Tensor, M: int, *,
                  dbias: Optional[torch.Tensor] = None, dgelu_aux: Optional[torch.Tensor] = None,
                  ldy: Optional[int] = None, y_off: int = 0, ldx: Optional[int] = None, lddx: Optional[int] = None,
                  lddw: Optional[int] = None, splits: Optional[int] = None) -> bool:
    """dX[M][192] = (dY @ W) [* gelu'(dgelu_aux)], dW[192][192] (f32) += dY^T @ X, dbias += column sums of dY, from ONE read of dY;
    wT is the [N][K] operand gemm_nt takes for the same dX.  One workgroup per M-slice, at least 16 stages of 32 rows each.
    Returns False, with nothing launched, written or recorded, when sodt_linear_bwd_sq does not take the layer (anything but bf16
    at 192 -> 192, a leading dimension or an address off its alignment: SODT_EINVAL): the caller then runs gemm_tn + gemm_nt."""
    ts = [dY, X, wT, dX] + ([dgelu_aux] if dgelu_aux is not None else [])
    if any(t.dtype != torch.bfloat16 for t in ts) or dW.dtype != torch.float32 or (dbias is not None and dbias.dtype != torch.float32):
        return False
    if tuple(wT.shape) != (192, 192) or X.shape[-1] < 192 or dX.shape[-1] < 192:
        return False
    g = L.LinBwdArgs()
    g.dY = dY.data_ptr() + y_off * dY.element_size()
    g.ldy = dY.shape[-1] if ldy is None else ldy
    g.X, g.ldx = X.data_ptr(), (X.shape[-1] if ldx is None else ldx)
    g.wT, g.ldw = wT.data_ptr(), wT.stride(0)
    g.dX, g.lddx = dX.data_ptr(), (dX.shape[-1] if lddx is None else lddx)
    g.dW, g.lddw = dW.data_ptr(), (192 if lddw is None else lddw)
    g.dbias = _p(dbias)
    g.M, g.N, g.K = M, 192, 192
    if dgelu_aux is not None:
        g.flags = L.EPI_DGELU
        g.aux, g.ldaux = dgelu_aux.data_ptr(), dgelu_aux.shape[-1]
    g.splits = linear_bwd_sq_splits(M) if splits is None else splits
    if _tn_scratch is not None and _tn_scratch.device == dY.device and g.splits > 1:
        g.partial, g.partial_floats = _tn_scratch.data_ptr(), _tn_scratch.numel()
    fn = _lib.sodt_linear_bwd_sq
    args = (C.byref(g), L.BF16)
    rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == L.EINVAL:              # refused before any launch (a failed launch is SODT_ELAUNCH and raises below)
        return False
    if rc != 0:
        raise RuntimeError(f"sodt_linear_bwd_sq failed with status {rc}")
    if _active_recorder is not None:
        _active_recorder.append((fn, args, "sodt_linear_bwd_sq", _tag))
    return True


def linear_bwd_sq_splits(M: int) -> int:
    """M-slices of sodt_linear_bwd_sq: one workgroup per CU, at least 16 stages of 32 rows per slice."""
    return max(1, min(M // 512, 256))


def linear_bwd_wide(dY: torch.Tensor, X: torch.Tensor, wT: torch.Tensor, dX: torch.Tensor, dW: torch.Tensor, M: int, *,
                    dbias: Optional[torch.Tensor] = None, ldy: Optional[int] = None, y_off: int = 0, ldx: Optional[int] = None,
                    lddx: Optional[int] = None, lddw: Optional[int] = None, splits: Optional[int] = None) -> bool:
    """dX[M][192] = dY[M][576] @ W, dW[576][192] (f32) += dY^T @ X, dbias[576] += column sums of dY, in ONE launch (plus the slice
    reduction); wT is the [192][576] operand gemm_nt takes for the same dX.  Three sibling workgroups per M-slice, one 64-column
    slab of K each (csrc/linbwd.hip).  Returns False, with nothing launched, written or recorded, when sodt_linear_bwd_wide does not
    take the layer (SODT_EINVAL): the caller then runs gemm_tn + gemm_nt."""
    if any(t.dtype != torch.bfloat16 for t in (dY, X, wT, dX)) or dW.dtype != torch.float32 or (dbias is not None and dbias.dtype != torch.float32):
        return False
    if tuple(wT.shape) != (192, 576) or X.shape[-1] < 192 or dX.shape[-1] < 192:
        return False
    g = L.LinBwdArgs()
    g.dY = dY.data_ptr() + y_off * dY.element_size()
    g.ldy = dY.shape[-1] if ldy is None else ldy
    g.X, g.ldx = X.data_ptr(), (X.shape[-1] if ldx is None else ldx)
    g.wT, g.ldw = wT.data_ptr(), wT.stride(0)
    g.dX, g.lddx = dX.data_ptr(), (dX.shape[-1] if lddx is None else lddx)
    g.dW, g.lddw = dW.data_ptr(), (192 if lddw is None else lddw)
    g.dbias = _p(dbias)
    g.M, g.N, g.K = M, 576, 192
    g.splits = linear_bwd_wide_splits(M) if splits is None else splits
    if _tn_scratch is not None and _tn_scratch.device == dY.device and g.splits > 1:
        g.partial, g.partial_floats = _tn_scratch.data_ptr(), _tn_scratch.numel()
    fn = _lib.sodt_linear_bwd_wide
    args = (C.byref(g), L.BF16)
    rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == L.EINVAL:              # refused before any launch
        return False
    if rc != 0:
        raise RuntimeError(f"sodt_linear_bwd_wide failed with status {rc}")
    if _active_recorder is not None:
        _active_recorder.append((fn, args, "sodt_linear_bwd_wide", _tag))
    return True


def linear_bwd_wide_splits(M: int) -> int:
    """M-slices of sodt_linear_bwd_wide: three workgroups per slice, 3 x 85 = 255 on 256 CUs, at least 16 stages of 32 rows per slice."""
    return max(1, min(M // 512, 85))


def mlp_bwd(xn: torch.Tensor, dY: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2T: torch.Tensor, dh: torch.Tensor,
            dW1: torch.Tensor, db1: torch.Tensor, dW2: torch.Tensor, db2: torch.Tensor, M: int, *,
            hact: Optional[torch.Tensor] = None, ldxn: Optional[int] = None, ldy: Optional[int] = None, lddh: Optional[int] = None,
            ldha: Optional[int] = None, lddw1: Optional[int] = None, lddw2: Optional[int] = None, splits: Optional[int] = None) -> bool:
    """Backward of fc2(GELU(fc1(xn))) at C = 192, hidden 768, in ONE launch (plus the slice reduction): dh[M][768] = (dY @ fc2.weight)
    * gelu'(xn @ w1^T + b1) with the bits of gemm_nt(dgelu_rc=True), dW1 += dh^T xn, db1 += column sums of dh, dW2 += dY^T GELU(h),
    db2 += column sums of dY; hact (optional) receives the recomputed GELU(h).  w1 is fc1.weight [768][192], w2T the [768][192]
    operand gemm_nt takes for dY @ fc2.weight.  Eight sibling workgroups per M-slice, one 96-column slab of the hidden dimension
    each (csrc/mlpbwd.hip).  Returns False, with nothing launched, written or recorded, when sodt_mlp_bwd does not take the layer
    (SODT_EINVAL): the caller then runs gemm_tn + gemm_nt(dgelu_rc) + gemm_tn."""
    bf = [xn, dY, w1, w2T, dh] + ([hact] if hact is not None else [])
    if any(t.dtype != torch.bfloat16 for t in bf) or any(t.dtype != torch.float32 for t in (b1, dW1, db1, dW2, db2)):
        return False
    if tuple(w1.shape) != (768, 192) or tuple(w2T.shape) != (768, 192) or b1.numel() != 768 or db1.numel() != 768 or db2.numel() != 192:
        return False
    if xn.shape[-1] < 192 or dY.shape[-1] < 192 or dh.shape[-1] < 768 or (hact is not None and hact.shape[-1] < 768):
        return False
    sp = mlp_bwd_splits(M) if splits is None else splits
    part, part_n = None, 0
    if _tn_scratch is not None and _tn_scratch.device == dY.device and sp > 1:
        part, part_n = _tn_scratch.data_ptr(), _tn_scratch.numel()
    fn = _lib.sodt_mlp_bwd
    args = (xn.data_ptr(), xn.shape[-1] if ldxn is None else ldxn, dY.data_ptr(), dY.shape[-1] if ldy is None else ldy,
            w1.data_ptr(), w1.stride(0), b1.data_ptr(), w2T.data_ptr(), w2T.stride(0),
            dh.data_ptr(), dh.shape[-1] if lddh is None else lddh, _p(hact), 0 if hact is None else (hact.shape[-1] if ldha is None else ldha),
            dW1.data_ptr(), 192 if lddw1 is None else lddw1, db1.data_ptr(), dW2.data_ptr(), 768 if lddw2 is None else lddw2,
            db2.data_ptr(), M, 192, sp, part, part_n, L.BF16)
    rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == L.EINVAL:              # refused before any launch
        return False
    if rc != 0:
        raise RuntimeError(f"sodt_mlp_bwd failed with status {rc}")
    if _active_recorder is not None:
        _active_recorder.append((fn, args, "sodt_mlp_bwd", _tag))
    return True


def mlp_bwd_splits(M: int) -> int:
    """M-slices of sodt_mlp_bwd: eight workgroups per slice, 8 x 32 = 256 on 256 CUs, at least 16 stages of 32 rows per slice."""
    return max(1, min(M // 512, 32))


def layernorm_fwd(x, gamma, beta, y, stats, M, Cc):
    _launch("sodt_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(stats), M, Cc, dt_code(x))


def layernorm_bwd(dy, x, stats, gamma, dres, dx, dgamma, dbeta, M, Cc):
    _launch("sodt_layernorm_bwd", _p(dy), _p(x), _p(stats), _p(gamma), _p(dres), _p(dx), _p(dgamma), _p(dbeta),
            M, Cc, dt_code(x))


def window_attn_fwd(qkv, bias_t, out, lse, B, H, W, Cc, heads, ws, shift):
    _launch("sodt_window_attn_fwd", _p(qkv), _p(bias_t), _p(out), _p(lse), B, H, W, Cc, heads, ws, shift, dt_code(qkv))


def window_attn_bwd(qkv, bias_t, out, dout, lse, dqkv, dbias_t, scratch, B, H, W, Cc, heads, ws, shift):
    _launch("sodt_window_attn_bwd", _p(qkv), _p(bias_t), _p(out), _p(dout), _p(lse), _p(dqkv), _p(dbias_t), _p(scratch),
            B, H, W, Cc, heads, ws, shift, dt_code(qkv))


def wmsa_pack_bytes(Cc: int, heads: int, ws: int, dtype_code: int) -> int:
    """0 when the fused block kernel does not take this geometry (csrc/wmsa_block.hip: C 192, 12 heads, 8x8 windows)."""
    return int(_lib.sodt_wmsa_pack_bytes(Cc, heads, ws, dtype_code))


def wmsa_pack(qkv_w, qkv_b, proj_w, proj_b, table, n1w, n1b, n2w, n2b, wpk, Cc, heads, ws):
    _launch("sodt_wmsa_pack", _p(qkv_w), _p(qkv_b), _p(proj_w), _p(proj_b), _p(table), _p(n1w), _p(n1b), _p(n2w), _p(n2b),
            _p(wpk), Cc, heads, ws, L.BF16 if wpk.dtype == torch.bfloat16 else L.F32)


def wmsa_block_fwd(x, wpk, xm, xn2, st1, st2, xn1, qkvw, lsew, ao, B, H, W, Cc, heads, ws, shift):
    """x_mid = x + Proj(W-MSA(LN1 x)), xn2 = LN2(x_mid) in one launch; xn1 .. ao are the save-for-backward outputs (None: inference)."""
    _launch("sodt_wmsa_block_fwd", _p(x), _p(wpk), _p(xm), _p(xn2), _p(st1), _p(st2), _p(xn1), _p(qkvw), _p(lsew), _p(ao),
            B, H, W, Cc, heads, ws, shift, dt_code(x))


def window_attn_sp_fwd(qkv, qkv_bias, bias_t, out, lse, B, H, W, Cc, heads, ws, shift):
    """shifted block on a zero-padded grid (csrc/attention_sp.hip): operands on the unpadded grid, a pad key reads qkv_bias"""
    _launch("sodt_window_attn_sp_fwd", _p(qkv), _p(qkv_bias), _p(bias_t), _p(out), _p(lse), B, H, W, Cc, heads, ws, shift, dt_code(qkv))


def window_attn_sp_bwd(qkv, qkv_bias, bias_t, out, dout, lse, dqkv, dqkv_bias, dbias_t, B, H, W, Cc, heads, ws, shift):
    _launch("sodt_window_attn_sp_bwd", _p(qkv), _p(qkv_bias), _p(bias_t), _p(out), _p(dout), _p(lse), _p(dqkv), _p(dqkv_bias),
            _p(dbias_t), B, H, W, Cc, heads, ws, shift, dt_code(qkv))


def window_attn_bwd_wm(qkvw, bias_t, dout, lsew, dqkv, dbias_t, B, H, W, Cc, heads, ws, shift):
    _launch("sodt_window_attn_bwd_wm", _p(qkvw), _p(bias_t), _p(dout), _p(lsew), _p(dqkv), _p(dbias_t),
            B, H, W, Cc, heads, ws, shift, dt_code(dout))


def wmsa_block_bwd(xn1, wpk, bias_t, dout, lsew, dqkv, dbias_t, B, H, W, Cc, heads, ws, shift):
    """Attention backward of the fused block (bf16) with q / k / v recomputed from the saved LN1 output and the parameter pack."""
    _launch("sodt_wmsa_block_bwd", _p(xn1), _p(wpk), _p(bias_t), _p(dout), _p(lsew), _p(dqkv), _p(dbias_t),
            B, H, W, Cc, heads, ws, shift, dt_code(dout))


# ---- super-resolution branch data movement (csrc/sr.hip)
def bilinear_up2_fwd(x, y, B, H, W, Cc, ldy=None, ycol=0):
    """y[:, ycol : ycol + C] = bilinear x2 (align_corners=True) of x [B*H*W][C]; y may be a wider [B*4HW][ldy] buffer."""
    ldy = y.shape[-1] if ldy is None else ldy
    _launch("sodt_bilinear_up2_fwd", x.data_ptr(), y.data_ptr() + ycol * y.element_size(), ldy, B, H, W, Cc, dt_code(x))


def bilinear_up2_bwd(dy, dx, B, H, W, Cc, lddy=None, dycol=0, relu_out=None):
    lddy = dy.shape[-1] if lddy is None else lddy
    _launch("sodt_bilinear_up2_bwd", dy.data_ptr() + dycol * dy.element_size(), lddy, dx.data_ptr(), _p(relu_out), B, H, W, Cc, dt_code(dx))


def pixel_shuffle2(src, dst, B, H, W, Cc, inverse=False):
    """forward: src [B*H*W][4C] -> dst [B*2H*2W][C] (nn.PixelShuffle(2)); inverse: src [B*2H*2W][C] -> dst [B*H*W][4C]."""
    _launch("sodt_pixel_shuffle2", src.data_ptr(), dst.data_ptr(), B, H, W, Cc, int(bool(inverse)), dt_code(src))


def conv3_n8_ok(t: torch.Tensor, cin: int, np_: int, k: int) -> bool:
    """EDSR's closing convolution (64 -> <= 8 channels, 3x3) has its own kernels in bf16 (csrc/conv3.hip)."""
    return t.dtype == torch.bfloat16 and cin == 64 and np_ == 8 and k == 3


def conv3_n8_fwd(x, w, bias, y, B, H, W, y_nchw=None, cout=8):
    """y [B*H*W][8] = conv3x3(x [B*H*W][64]; w [8][576] = [n][tap*64 + c]) + bias (f32[8] or None); y_nchw (B, cout, H, W) float32:
    the result goes there instead (unrounded) and y may be None."""
    _launch("sodt_conv3x3_c64n8_fwd", x.data_ptr(), w.data_ptr(), _p(bias), _p(y), _p(y_nchw), B, H, W, cout, dt_code(x))


def conv3_n8_dgrad(dy, wT, dx, B, H, W, dy_nchw=None, cout=8):
    """dx [B*H*W][64] = conv3x3^T(dy [B*H*W][8] or dy_nchw (B, cout <= 4, H, W) float32; wT [64][72] = [c][tap*8 + n])."""
    _launch("sodt_conv3x3_c64n8_dgrad", _p(dy), _p(dy_nchw), wT.data_ptr(), dx.data_ptr(), B, H, W, cout, dt_code(dx))


def conv3_n8_wgrad_scratch_floats() -> int:
    return int(_lib.sodt_conv3x3_c64n8_wgrad_scratch_bytes()) // 4


def conv3_n8_wgrad(dy, x, dw, db, scratch, B, H, W, cout, dy_nchw=None):
    """dw [cout][64][3][3] f32 += , db [cout] f32 += (or None); dy rows or dy_nchw float32; scratch: conv3_n8_wgrad_scratch_floats() float32."""
    assert dw.dtype == torch.float32 and dw.is_contiguous() and scratch.dtype == torch.float32
    _launch("sodt_conv3x3_c64n8_wgrad", _p(dy), _p(dy_nchw), x.data_ptr(), dw.data_ptr(), _p(db), scratch.data_ptr(), B, H, W, cout, dt_code(x))


def conv3_geo(w_row=(1, 0), inp=(1, 0, 0), out=(1, 0, 0)):
    """sodt_conv3_geo: output channel n <-> weight row w_row[0] * n + w_row[1]; input / output pixel (y, x) <-> (m y + i, m x + j)."""
    g = L.Conv3Geo()
    g.w_row_stride, g.w_row_off = w_row
    g.in_mul, g.in_i, g.in_j = inp
    g.out_mul, g.out_i, g.out_j = out
    return g


def conv3_c64_fwd(x, w, y, B, H, W, bias=None, relu=False, drelu_aux=None, resid=None, flip=False, geo=None):
    """y [B*H*W][64] = epilogue(conv3x3(x [B*H*W][64]; w [64][576] = [n][tap*64 + c])), bf16 (csrc/conv3.hip); flip: mirrored taps (the
    input gradient with the transposed weights); geo: conv3_geo(...) maps (H x W is the grid the kernel walks)."""
    flags = ((L.EPI_BIAS if bias is not None else 0) | (L.EPI_RELU if relu else 0) | (L.EPI_DRELU if drelu_aux is not None else 0)
             | (L.EPI_RESID if resid is not None else 0))
    _launch("sodt_conv3x3_c64_fwd", x.data_ptr(), w.data_ptr(), _p(bias), _p(resid), _p(drelu_aux), y.data_ptr(), B, H, W, flags,
            int(bool(flip)), C.byref(geo) if geo is not None else None, dt_code(x))


def conv3_c64_wgrad_scratch_floats() -> int:
    return int(_lib.sodt_conv3x3_c64_wgrad_scratch_bytes()) // 4


def conv3_c64_wgrad(dy, x, dw, db, scratch, B, H, W, geo=None):
    """dw [..][64][3][3] f32 +=, db f32 += (or None), bf16 operands; geo: dy through the out_* map, dw / db rows through w_row."""
    assert dw.dtype == torch.float32 and dw.is_contiguous() and scratch.dtype == torch.float32
    _launch("sodt_conv3x3_c64_wgrad", dy.data_ptr(), x.data_ptr(), dw.data_ptr(), _p(db), scratch.data_ptr(), B, H, W,
            C.byref(geo) if geo is not None else None, dt_code(dy))


def add_rows(dst, src, M, Cc, ldd=None, dcol=0, lds=None, scol=0):
    _launch("sodt_add_rows", dst.data_ptr(), dst.shape[-1] if ldd is None else ldd, dcol, src.data_ptr(),
            src.shape[-1] if lds is None else lds, scol, C.c_long(M), Cc, dt_code(dst))


def nchw_f32_from_rows(rows, y, B, Cc, H, W):
    _launch("sodt_nchw_f32_from_rows", rows.data_ptr(), rows.shape[-1], y.data_ptr(), B, Cc, H, W, dt_code(rows))


def rows_from_nchw_f32(y, rows, B, Cc, H, W):
    _launch("sodt_rows_from_nchw_f32", y.data_ptr(), rows.data_ptr(), rows.shape[-1], B, Cc, H, W, dt_code(rows))


def frontend_fwd(rgb, ir_plane, ir_bstride, w, b, gamma, beta, out, B, H, W, *, ca_ws=1):
    """The front end on an H x W image: out is [B * (H/4) * (W/4)][192], row (b * H/4 + y) * W/4 + x."""
    _launch("sodt_frontend_fwd", _p(rgb), _p(ir_plane), ir_bstride, _p(w), _p(b), _p(gamma), _p(beta), _p(out),
            B, H, W, ca_ws, dt_code(out))


def frontend_bwd_workspace_bytes(B: int, H: int, W: int) -> int:
    return int(_lib.sodt_frontend_bwd_workspace_bytes(B, H, W))


def frontend_bwd(rgb, ir_plane, ir_bstride, w, b, gamma, beta, dout, dw, db, dgamma, dbeta, B, H, W, *, ca_ws=1, ws=None):
    """``ws``: f32 scratch of ``frontend_bwd_workspace_bytes`` (two-stage reduction); None = direct atomics."""
    _launch("sodt_frontend_bwd", _p(rgb), _p(ir_plane), ir_bstride, _p(w), _p(b), _p(gamma), _p(beta), _p(dout),
            _p(dw), _p(db), _p(dgamma), _p(dbeta), B, H, W, ca_ws, _p(ws), 0 if ws is None else ws.numel() * ws.element_size(),
            dt_code(dout))


def patch_embed4_fwd(rgb, ir_plane, ir_bstride, w, b, e, B, H, W):
    _launch("sodt_patch_embed4_fwd", _p(rgb), _p(ir_plane), ir_bstride, _p(w), _p(b), _p(e), B, H, W)


def patch_embed4_bwd(rgb, ir_plane, ir_bstride, de, dw, db, B, H, W):
    _launch("sodt_patch_embed4_bwd", _p(rgb), _p(ir_plane), ir_bstride, _p(de), _p(dw), _p(db), B, H, W)


def cross_attn_ln_fwd(e, gamma, beta, out, B, H, W, ws, shift):
    _launch("sodt_cross_attn_ln_fwd", _p(e), _p(gamma), _p(beta), _p(out), B, H, W, ws, shift, dt_code(out))


def cross_attn_ln_bwd(e, gamma, dout, de, dgamma, dbeta, B, H, W, ws, shift):
    _launch("sodt_cross_attn_ln_bwd", _p(e), _p(gamma), _p(dout), _p(de), _p(dgamma), _p(dbeta), B, H, W, ws, shift, dt_code(dout))


def bn_finalize(stats, mean_rstd, running_mean, running_var, count, Cc, eps, momentum):
    _launch("sodt_bn_finalize", _p(stats), _p(mean_rstd), _p(running_mean), _p(running_var), count, Cc,
            C.c_float(eps), C.c_float(momentum))


def bn_affine(mean_rstd, gamma, beta, scale, shift, Cc):
    _launch("sodt_bn_affine", _p(mean_rstd), _p(gamma), _p(beta), _p(scale), _p(shift), Cc)


def bn_silu_fwd(z, mean_rstd, gamma, beta, y, ldy, M, Cc):
    _launch("sodt_bn_silu_fwd", _p(z), _p(mean_rstd), _p(gamma), _p(beta), _p(y), ldy, M, Cc, dt_code(z))


def col_stats(z, stats, M, Cc):
    """stats [STATS_REPL][2][C] f64 += column sums / sums of squares of z [M][ld] (BatchNorm batch statistics of a stored conv output)."""
    _launch("sodt_col_stats", z.data_ptr(), z.shape[-1], stats.data_ptr(), C.c_long(M), Cc, dt_code(z))


def bn_silu_bwd_reduce(dy, lddy, z, mean_rstd, gamma, beta, red, M, Cc, dy_off=0):
    _launch("sodt_bn_silu_bwd_reduce", dy.data_ptr() + dy_off * dy.element_size(), lddy, _p(z), _p(mean_rstd), _p(gamma),
            _p(beta), _p(red), M, Cc, dt_code(z))


def bn_silu_bwd_apply(dy, lddy, z, mean_rstd, gamma, beta, red, dz, dgamma, dbeta, M, Cc, dy_off=0, lddz=None, dz_off=0):
    """dz may be a column slice of a wider buffer: rows lddz elements apart, starting at column dz_off (dense: Cc, 0)."""
    _launch("sodt_bn_silu_bwd_apply", dy.data_ptr() + dy_off * dy.element_size(), lddy, _p(z), _p(mean_rstd), _p(gamma),
            _p(beta), _p(red), dz.data_ptr() + dz_off * dz.element_size(), _p(dgamma), _p(dbeta), M, Cc,
            Cc if lddz is None else lddz, dt_code(z))


def bn_silu_bwd_apply_sync(dy, lddy, z, mean_rstd, gamma, beta, red_local, red_global, count_total, dz, dgamma, dbeta, M, Cc,
                           dy_off=0, lddz=None, dz_off=0):
    """bn_silu_bwd_apply with the statistics of every data-parallel rank: the means of dz are red_global / count_total (the
    all-reduced sums over the rows of all ranks), dgamma / dbeta take this rank's red_local."""
    _launch("sodt_bn_silu_bwd_apply_sync", dy.data_ptr() + dy_off * dy.element_size(), lddy, _p(z), _p(mean_rstd), _p(gamma),
            _p(beta), _p(red_local), _p(red_global), count_total, dz.data_ptr() + dz_off * dz.element_size(), _p(dgamma),
            _p(dbeta), M, Cc, Cc if lddz is None else lddz, dt_code(z))


def copy_rows(src, lds, dst, ldd, B, Ho, Wo, shr, Cc, dst_off=0):
    _launch("sodt_copy_rows", _p(src), lds, dst.data_ptr() + dst_off * dst.element_size(), ldd, B, Ho, Wo, shr, Cc, dt_code(src))


def gather_sum_rows(d, ldd, dsrc, lds, B, Hs, Ws, shr, Cc, accumulate=False, d_off=0):
    _launch("sodt_gather_sum_rows", d.data_ptr() + d_off * d.element_size(), ldd, _p(dsrc), lds, B, Hs, Ws, shr, Cc,
            1 if accumulate else 0, dt_code(d))


def detect_unpermute(dpred, dz, ldz, B, HW, na, no):
    _launch("sodt_detect_unpermute", _p(dpred), _p(dz), ldz, B, HW, na, no, dt_code(dz))


def detect_splits(M: int, fwd: bool = False) -> int:
    """M-slices of sodt_detect_fwd / _bwd, at least 16 stages of 32 rows per slice: one workgroup per CU for the backward (its
    registers allow no second one), two for the forward (60 KiB of LDS each at K = 128: twice the rows in flight per CU)."""
    return max(1, min(M // 512, 512 if fwd else 256))


def detect_fused_ok(K: int, na: int, no: int, dtype: torch.dtype) -> bool:
    """the shapes sodt_detect_fwd / sodt_detect_bwd take (csrc/detect.hip); alignment is checked by the entry itself"""
    return dtype == torch.bfloat16 and K % 32 == 0 and 32 <= K <= 256 and 1 <= na * no <= 48


def _detect_args(X, W, B, HW, na, no, K, splits, fwd=False):
    g = L.DetectArgs()
    g.X, g.ldx = X.data_ptr(), X.shape[-1]
    g.W, g.ldw = W.data_ptr(), W.stride(0)
    g.B, g.HW, g.na, g.no, g.K = B, HW, na, no, K
    g.splits = detect_splits(B * HW, fwd) if splits is None else splits
    return g


def _detect_call(name, g) -> bool:
    fn = getattr(_lib, name)
    args = (C.byref(g), L.BF16)
    rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == L.EINVAL:              # refused before any launch
        return False
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc}")
    if _active_recorder is not None:
        _active_recorder.append((fn, args, name, _tag))
    return True


def detect_fwd(X: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], pred: torch.Tensor, B: int, HW: int, na: int, no: int,
               K: int, splits: Optional[int] = None) -> bool:
    """pred (B, na, HW, no) f32 = Detect's 1x1 convolution of X [B*HW][K] with W [>= na*no][K] (+ bias), in one pass (csrc/detect.hip).
    Returns False, with nothing launched, written or recorded, where sodt_detect_fwd does not take the call (SODT_EINVAL): the
    caller then runs gemm_nt(..., detect=...)."""
    if X.dtype != torch.bfloat16 or W.dtype != torch.bfloat16 or pred.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        return False
    g = _detect_args(X, W, B, HW, na, no, K, splits, fwd=True)
    g.bias, g.pred = _p(bias), pred.data_ptr()
    return _detect_call("sodt_detect_fwd", g)


def detect_bwd(dpred: torch.Tensor, X: torch.Tensor, W: torch.Tensor, dX: Optional[torch.Tensor], dW: Optional[torch.Tensor],
               dbias: Optional[torch.Tensor], B: int, HW: int, na: int, no: int, K: int, *, lddw: Optional[int] = None,
               splits: Optional[int] = None) -> bool:
    """Detect's backward from ONE read of dpred (B, na, HW, no) f32: dX [B*HW][K] bf16 = dZ @ W, dW [na*no][K] f32 += dZ^T @ X,
    dbias += column sums of dZ, with dZ = bf16(dpred).  dX None: no input gradient; dW None: no weight / bias gradient.  The
    slices' partials go through the weight-gradient scratch (set_tn_scratch).  Returns False, with nothing launched or written,
    where sodt_detect_bwd refuses (SODT_EINVAL): the caller then runs detect_unpermute + gemm_tn + gemm_nt."""
    ts = [X, W] + ([dX] if dX is not None else [])
    if any(t.dtype != torch.bfloat16 for t in ts) or dpred.dtype != torch.float32 or any(t is not None and t.dtype != torch.float32 for t in (dW, dbias)):
        return False
    g = _detect_args(X, W, B, HW, na, no, K, splits)
    g.pred = dpred.data_ptr()
    if dX is not None:
        g.dX, g.lddx = dX.data_ptr(), dX.shape[-1]
    else:
        g.flags |= L.DETECT_NO_DX
    if dW is not None:
        g.dW, g.lddw, g.dbias = dW.data_ptr(), (K if lddw is None else lddw), _p(dbias)
        if _tn_scratch is not None and _tn_scratch.device == X.device:
            g.partial, g.partial_floats = _tn_scratch.data_ptr(), _tn_scratch.numel()
    else:
        g.flags |= L.DETECT_NO_WGRAD
    return _detect_call("sodt_detect_bwd", g)


def detect_decode(raw, anchor_grid, z, B, na, ny, nx, no, stride):
    _launch("sodt_detect_decode", _p(raw), _p(anchor_grid), _p(z), B, na, ny, nx, no, C.c_float(stride))


def tta_scale(x, ir, passes):
    """Every augmented input of one call in one launch (model.py:161-162, torch_utils.py:249-259).  x f32 (B, c, H, W), ir the
    same with its own channel count or None; passes: up to four (out_rgb, out_ir | None, (h, w), flip) with out_* f32
    (B, c, Hp, Wp) - the input flipped (0, 2 = up-down, 3 = left-right), resized to (h, w) and padded with 0.447."""
    B, c1, H, W = x.shape
    tab = (L.TtaPass * len(passes))()
    for t, (o1, o2, (h, w), flip) in zip(tab, passes):
        t.out_rgb, t.out_ir, t.h, t.w, t.Hp, t.Wp, t.flip = _p(o1), _p(o2), h, w, o1.shape[2], o1.shape[3], flip
    _launch("sodt_tta_scale", _p(x), _p(ir), B, c1, 0 if ir is None else ir.shape[1], H, W, tab, len(passes))


def detect_decode_tta(raw, anchor_grid, z, B, na, ny, nx, no, stride, row_off, si, flip, img_h, img_w):
    """detect_decode of one augmented pass into rows row_off .. of z (B, rows_total, no), de-scaled and de-flipped
    (model.py:178-182)."""
    _launch("sodt_detect_decode_tta", _p(raw), _p(anchor_grid), _p(z), B, na, ny, nx, no, C.c_float(stride), row_off,
            z.shape[1], C.c_float(si), flip, img_h, img_w)


def nms_candidates(z_img, conf_thres, multi_label, class_allow, keys, count):
    """z_img (N, 5+nc) f32 of one image -> sort keys + device count (general.py:433-480)."""
    N, no = z_img.shape
    _launch("sodt_nms_candidates", _p(z_img), N, no - 5, C.c_float(conf_thres), int(bool(multi_label)),
            _p(class_allow) if class_allow is not None else None, _p(keys), keys.numel(), _p(count))


def nms_workspace_bytes(n_total: int) -> int:
    return _ws_bytes("sodt_nms_workspace_bytes", int(n_total), hint="")


def nms_select(z_img, keys, n_total, iou_thres, agnostic, ws, out, out_index, out_count):
    """Sort + NMS + max_det + merge-NMS of general.py:485-508 for one image."""
    _launch("sodt_nms_select", _p(z_img), z_img.shape[1] - 5, _p(keys), int(n_total), C.c_float(iou_thres),
            int(bool(agnostic)), _p(ws), ws.numel() * ws.element_size(), _p(out), _p(out_index), _p(out_count))


def nms_batch_workspace_bytes(B: int, rows: int, nc: int, multi_label) -> int:
    """Scratch bytes of nms_batch (general.py:425-512 for a batch): a function of B, rows = N + lab_cap, nc, multi_label."""
    return _ws_bytes("sodt_nms_batch_workspace_bytes", int(B), int(rows), int(nc), int(bool(multi_label)),
                     hint="B <= 4096, B * rows * nc < 2^31")


def nms_batch(z, labels, nlab, conf_thres, iou_thres, multi_label, class_allow, agnostic, ws, out_rows, out_index, out_off):
    """non_max_suppression of general.py:425-512 for all B images of z (B, N, 5+nc) in one launch sequence without a host
    read.  labels (B, lab_cap, 5) f32 / nlab (B) int32 or None: the autolabelling rows.  out_rows (B*300, 6) f32,
    out_index (B*300) int32, out_off (B+1) int32: the packed form eval_match / confusion_update take."""
    B, N, no = z.shape
    lab_cap = 0 if labels is None else labels.shape[1]
    _launch("sodt_nms_batch", _p(z), B, N, no - 5, _p(labels), _p(nlab), lab_cap, C.c_float(conf_thres),
            C.c_float(iou_thres), int(bool(multi_label)), _p(class_allow), int(bool(agnostic)), _p(ws),
            ws.numel() * ws.element_size(), _p(out_rows), _p(out_index), _p(out_off))


def wbf_candidates(z, conf_thres, image_size, boxes, scores, labels, src, counts):
    """z (B, N, 5+nc) f32 -> per-image compact candidates + device counts (general.py:523-544)."""
    B, N, no = z.shape
    _launch("sodt_wbf_candidates", _p(z), B, N, no - 5, C.c_float(conf_thres), C.c_float(image_size), _p(boxes), _p(scores),
            _p(labels), _p(src), _p(counts))


def wbf_fuse_workspace_bytes(B: int, cap: int) -> int:
    return _ws_bytes("sodt_wbf_fuse_workspace_bytes", int(B), int(cap), hint="B <= 65535, B * cap <= 2^30")


def wbf_fuse(boxes, scores, labels, model, src, counts, weights, iou_thr, skip_box_thr, conf_type, allows_overflow, ws,
             out_boxes, out_scores, out_labels, out_counts, member=None, scan_lanes=0):
    """weighted_boxes_fusion (ensemble_boxes_wbf.py:150-225) for B images: boxes (B, cap, 4), scores / labels / model / src
    (B, cap), counts (B); weights: host floats, one per model."""
    B, cap = scores.shape
    w = (C.c_double * len(weights))(*[float(v) for v in weights])
    _launch("sodt_wbf_fuse", _p(boxes), _p(scores), _p(labels), _p(model), _p(src), _p(counts), B, cap, w, len(weights),
            C.c_double(iou_thr), C.c_float(skip_box_thr), int(conf_type), int(bool(allows_overflow)), int(scan_lanes),
            _p(ws), ws.numel() * ws.element_size(), _p(out_boxes), _p(out_scores), _p(out_labels), _p(out_counts), _p(member))


def eval_match_workspace_bytes(B: int, n_det: int, nt: int) -> int:
    return _ws_bytes("sodt_eval_match_workspace_bytes", int(B), int(n_det), int(nt), hint="")


def eval_match(det, det_off, targets, geom, iouv, ws, correct, tcls_out):
    """Per-image true-positive matching of test.py:155-240 for one batch: det (n_det, 6) f32 packed NMS rows,
    det_off (B+1) int32, targets (nt, 6) f32 pixel-space, geom (B, 5) f32, iouv: 10 host floats."""
    B = det_off.numel() - 1
    thr = (C.c_float * 10)(*[float(v) for v in iouv])
    _launch("sodt_eval_match", _p(det), _p(det_off), B, det.shape[0], _p(targets), targets.shape[0], _p(geom), thr,
            _p(ws), ws.numel() * ws.element_size(), _p(correct), _p(tcls_out))


def ap_per_class_workspace_bytes(n: int, nt: int, nc: int) -> int:
    return _ws_bytes("sodt_ap_per_class_workspace_bytes", int(n), int(nt), int(nc), hint="nc must be in [1, 4096]")


def ap_per_class(tp, conf, pred_cls, target_cls, nc, ws, p, r, f1, ap, classes, nt_count, info):
    """ap_per_class + compute_ap of metrics.py:18-106 on the device (f64 outputs, first info[0] rows valid)."""
    _launch("sodt_ap_per_class", _p(tp), _p(conf), _p(pred_cls), tp.shape[0], _p(target_cls), target_cls.numel(), int(nc),
            _p(ws), ws.numel() * ws.element_size(), _p(p), _p(r), _p(f1), _p(ap), _p(classes), _p(nt_count), _p(info))


def confusion_workspace_bytes(B: int, n_det: int, nt: int) -> int:
    return _ws_bytes("sodt_confusion_update_workspace_bytes", int(B), int(n_det), int(nt), hint="")


def confusion_update(det, det_off, targets, geom, nc, conf, iou_thres, ws, matrix, info):
    """ConfusionMatrix.process_batch (metrics.py:117-155) for one batch, added into matrix ((nc+1)^2 int64) and info
    (int32[2]).  det / det_off / targets / geom as eval_match; geom None: boxes as given, targets [img cls x1 y1 x2 y2]."""
    B = det_off.numel() - 1
    _launch("sodt_confusion_update", _p(det), _p(det_off), B, det.shape[0], _p(targets), targets.shape[0],
            _p(geom), int(nc), C.c_float(conf), C.c_float(iou_thres),
            _p(ws), ws.numel() * ws.element_size(), _p(matrix), _p(info))


def prep_weights(table_dev, n, max_elems, dtype_code):
    _launch("sodt_prep_weights", _p(table_dev), n, max_elems, dtype_code)


class PrepTable:
    """A descriptor table of sodt_prep_weights: add() one permuted copy per destination, upload() once, run() per step."""

    def __init__(self):
        self.descs: List[L.PrepDesc] = []
        self.tab = None                 # (device table, descriptors, elements of the largest copy)

    def add(self, src, dst, dims, perm, dst_ld, inner_ld=0):
        d = L.PrepDesc()
        d.src, d.dst = src.data_ptr(), dst.data_ptr()
        d.d0, d.d1, d.d2 = dims
        d.p0, d.p1, d.p2 = perm
        d.dst_ld, d.inner_ld = dst_ld, inner_ld
        self.descs.append(d)

    def upload(self, dev):
        arr = (L.PrepDesc * len(self.descs))(*self.descs)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.tab = (host.to(dev), len(self.descs), max(d.d0 * d.d1 * d.d2 for d in self.descs))
        return self

    def run(self, dtype_code):
        prep_weights(*self.tab, dtype_code)


def transpose_f32(src, dst, rows, cols, accumulate=0):
    """accumulate: 0 store, 1 add, 2 add and clear src."""
    _launch("sodt_transpose_f32", _p(src), _p(dst), rows, cols, int(accumulate))


def zero_(t):
    _launch("sodt_memset_zero", _p(t), t.numel() * t.element_size())


def cast(src, dst, n):
    _launch("sodt_cast", _p(src), _p(dst), n, dt_code(src), dt_code(dst))


def batch_sum(d, out, B, RC):
    _launch("sodt_batch_sum", _p(d), _p(out), B, RC, dt_code(d))


def sgd_ema_step(p, g, mom, ema, p_cast, group_of_chunk, lr, momentum, weight_decay, nesterov, grad_scale=1.0, ema_decay=0.0):
    """One fused SGD(+nesterov, weight decay groups) + EMA + run-dtype cast pass over the flat buffers (csrc/optim.hip)."""
    ng = len(lr)
    arr = lambda v: (C.c_float * ng)(*[float(x) for x in v])
    code = L.F32 if p_cast is None else dt_code(p_cast)
    _launch("sodt_sgd_ema_step", _p(p), _p(g), _p(mom), _p(ema), _p(p_cast), code, _p(group_of_chunk), p.numel(), ng,
            arr(lr), arr(momentum), arr(weight_decay), int(bool(nesterov)), C.c_float(grad_scale), C.c_float(ema_decay))


def adam_ema_step(p, g, exp_avg, exp_avg_sq, ema, p_cast, group_of_chunk, lr, betas, eps, weight_decay, decoupled, step,
                  grad_scale=1.0, ema_decay=0.0):
    """One fused Adam / AdamW (decoupled) + EMA + run-dtype cast pass over the flat buffers (csrc/optim.hip); per-group
    hyper-parameters go down as doubles, `step` is torch's state['step'] after its increment (>= 1)."""
    ng = len(lr)
    arr = lambda v: (C.c_double * ng)(*[float(x) for x in v])
    code = L.F32 if p_cast is None else dt_code(p_cast)
    _launch("sodt_adam_ema_step", _p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), _p(ema), _p(p_cast), code, _p(group_of_chunk),
            p.numel(), ng, arr(lr), arr([b[0] for b in betas]), arr([b[1] for b in betas]), arr(eps), arr(weight_decay),
            int(bool(decoupled)), int(step), C.c_float(grad_scale), C.c_float(ema_decay))


def new_step_ctl(dev, step: int = 0):
    """A zeroed sodt_step_ctl record in device memory as eight f64 words (L.StepCtl names the fields)."""
    ctl = torch.zeros(C.sizeof(L.StepCtl) // 8, dtype=torch.float64, device=dev)
    ctl.view(torch.int64)[L.StepCtl.step.offset // 8] = int(step)
    return ctl


def step_ctl_field(ctl, name):
    """A one-element view of field `name` of a record made by new_step_ctl (no copy, no synchronisation)."""
    f = getattr(L.StepCtl, name)
    dt = {C.c_double: torch.float64, C.c_longlong: torch.int64, C.c_float: torch.float32, C.c_int: torch.int32,
          C.c_uint: torch.int32}[dict((n, t) for n, t in L.StepCtl._fields_)[name]]
    i = f.offset // f.size
    return ctl.view(dt)[i:i + 1]


def grad_stats(g, group_of_chunk, ctl, scale=None, found_inf=None, grad_scale=1.0, max_norm=None, skip_nonfinite=False):
    """One pass over the flat gradient that fills the control record of the next *_step_ctl launch (csrc/optim.hip):
    found_inf, the f64 norm, the clip coefficient, inv_scale_eff, the skip flag and the applied-step counter.  `scale` and
    `found_inf` are one-element f32 DEVICE tensors (torch.amp.GradScaler's) or None; nothing is read on the host."""
    for t in (scale, found_inf):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != g.device):
            raise TypeError("grad_stats: scale / found_inf must be one-element float32 tensors on the gradient's device")
    _launch("sodt_grad_stats", _p(g), _p(group_of_chunk), g.numel(), _p(scale), _p(found_inf), C.c_float(grad_scale),
            C.c_float(0.0 if max_norm is None else max_norm), int(bool(skip_nonfinite)), _p(ctl))


def sgd_ema_step_ctl(p, g, mom, ema, p_cast, group_of_chunk, lr, momentum, weight_decay, nesterov, ctl, ema_decay=0.0):
    """sgd_ema_step with the gradient factor and the skip decision read from the device record `ctl` (grad_stats)."""
    ng = len(lr)
    arr = lambda v: (C.c_float * ng)(*[float(x) for x in v])
    code = L.F32 if p_cast is None else dt_code(p_cast)
    _launch("sodt_sgd_ema_step_ctl", _p(p), _p(g), _p(mom), _p(ema), _p(p_cast), code, _p(group_of_chunk), p.numel(), ng,
            arr(lr), arr(momentum), arr(weight_decay), int(bool(nesterov)), _p(ctl), C.c_float(ema_decay))


def adam_ema_step_ctl(p, g, exp_avg, exp_avg_sq, ema, p_cast, group_of_chunk, lr, betas, eps, weight_decay, decoupled, ctl,
                      ema_decay=0.0):
    """adam_ema_step with the gradient factor, the skip decision and the step count t read from the device record `ctl`."""
    ng = len(lr)
    arr = lambda v: (C.c_double * ng)(*[float(x) for x in v])
    code = L.F32 if p_cast is None else dt_code(p_cast)
    _launch("sodt_adam_ema_step_ctl", _p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), _p(ema), _p(p_cast), code, _p(group_of_chunk),
            p.numel(), ng, arr(lr), arr([b[0] for b in betas]), arr([b[1] for b in betas]), arr(eps), arr(weight_decay),
            int(bool(decoupled)), _p(ctl), C.c_float(ema_decay))


def new_sam_rec(dev):
    """A zeroed record of sam_norm / sam_perturb in device memory as eight f64 words (L.SAM_REC names the fields)."""
    return torch.zeros(L.SAM_REC_BYTES // 8, dtype=torch.float64, device=dev)


def sam_rec_field(rec, name):
    """A one-element view of field `name` of a record made by new_sam_rec (no copy, no synchronisation)."""
    off, ct = L.SAM_REC[name]
    dt = {C.c_double: torch.float64, C.c_float: torch.float32, C.c_uint: torch.int32}[ct]
    i = off // C.sizeof(ct)
    return rec.view(dt)[i:i + 1]


def _sam_flags(adaptive):
    return (C.c_int * len(adaptive))(*[int(bool(a)) for a in adaptive])


def sam_norm(p, g, group_of_chunk, adaptive, rec, scale=None, grad_scale=1.0):
    """basics/utils/sam.py:49-59 in one pass over the flat gradient (csrc/sam.hip): the f64 norm of (|p| if adaptive else 1) * g
    over the owned chunks, the not-finite flag and 1 / (norm + 1e-12) left in the device record `rec`.  `adaptive`: one flag
    per group; `p` may be None when none is set.  `scale`: a one-element f32 DEVICE tensor (GradScaler's) or None."""
    if scale is not None and (scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != g.device):
        raise TypeError("sam_norm: scale must be a one-element float32 tensor on the gradient's device")
    _launch("sodt_sam_norm", _p(p), _p(g), _p(group_of_chunk), g.numel(), len(adaptive), _sam_flags(adaptive), _p(scale),
            C.c_float(grad_scale), _p(rec))


def sam_perturb(p, g, old_p, p_cast, group_of_chunk, rho, adaptive, rec):
    """basics/utils/sam.py:19-25 in one pass: old_p = p, p += (p*p if adaptive else 1) * g * inv_scale * rho[group] / norm with
    the norm read from `rec` (sam_norm), and the run-dtype mirror of the moved p (p_cast, nullable)."""
    ng = len(rho)
    assert len(adaptive) == ng
    code = L.F32 if p_cast is None else dt_code(p_cast)
    _launch("sodt_sam_perturb", _p(p), _p(g), _p(old_p), _p(p_cast), code, _p(group_of_chunk), p.numel(), ng,
            (C.c_float * ng)(*[float(x) for x in rho]), _sam_flags(adaptive), _p(rec))


def sam_restore(p, old_p, group_of_chunk):
    """basics/utils/sam.py:34: p = old_p on the owned chunks."""
    _launch("sodt_sam_restore", _p(p), _p(old_p), _p(group_of_chunk), p.numel())


def sr_l1_workspace_bytes(B: int, C_: int, H: int, W: int) -> int:
    return _ws_bytes("sodt_sr_l1_workspace_bytes", int(B), int(C_), int(H), int(W), hint="B * C <= 65535, H * W < 2^31")


def _sr_l1_args(sr, rgb, ir, mode):
    tgt = ir if rgb is None else rgb
    code = L.U8 if tgt.dtype == torch.uint8 else L.F32
    B, Cc, H, W = sr.shape
    return (_p(sr), _p(rgb), _p(ir), code, L.SR_MODES[mode], B, Cc, 0 if rgb is None else rgb.shape[1],
            0 if ir is None else ir.shape[1], H, W)


def sr_l1_fwd(sr, rgb, ir, mode, ws, loss):
    """The --super term of Train.py:420-427 in one pass (csrc/srloss.hip): sr f32 (B, C, H, W), rgb / ir uint8 (or f32 in
    [0, 1]) batches, either None where `mode` ('IR', 'RGB', 'RGB+IR') does not use it; loss: one f32 on the device."""
    _launch("sodt_sr_l1_fwd", *_sr_l1_args(sr, rgb, ir, mode), _p(ws), ws.numel() * ws.element_size(), _p(loss))


def sr_l1_bwd(sr, rgb, ir, mode, upstream, dsr):
    """dsr = upstream * w / n_group * sign(sr - target) in one pass; upstream is a one-element f32 DEVICE tensor."""
    _launch("sodt_sr_l1_bwd", *_sr_l1_args(sr, rgb, ir, mode), _p(upstream), _p(dsr))


def anchor_stats_workspace_bytes(N: int, S: int) -> int:
    return _ws_bytes("sodt_anchor_stats_workspace_bytes", int(N), int(S))


def anchor_stats(wh, sets, thr_inv, ws, out):
    """autoanchor.py:33-39, :80-96 for S anchor sets: wh (N, 2) f32, sets (S, n, 2) f32, thr_inv = 1 / anchor_t (rounded to f32
    here); out (S, 6) f64 = sum(best), sum(best [best > thr]), count(best > thr), count(x > thr), sum(x), sum(x [x > thr])."""
    S, n, _ = sets.shape
    _launch("sodt_anchor_stats", _p(wh), wh.shape[0], _p(sets), S, n, C.c_float(thr_inv), _p(ws),
            ws.numel() * ws.element_size(), _p(out))


def anchor_evolve_workspace_bytes(N: int) -> int:
    return _ws_bytes("sodt_anchor_evolve_workspace_bytes", int(N))


def anchor_evolve(wh, thr_inv, k, f, v, accepted, ws):
    """autoanchor.py:146-153 for the G = v.shape[0] generations, one launch each and no host read: k (n, 2) f64 and f (1) f64
    in and out, v (G, n, 2) f64, accepted (G) int32 or None - all on the device."""
    _launch("sodt_anchor_evolve", _p(wh), wh.shape[0], C.c_float(thr_inv), _p(k), k.shape[0], _p(f), _p(v), v.shape[0],
            _p(accepted), _p(ws), ws.numel() * ws.element_size())


def kmeans_lloyd_workspace_bytes(N: int, R: int, n: int) -> int:
    return _ws_bytes("sodt_kmeans_lloyd_workspace_bytes", int(N), int(R), int(n))


def kmeans_lloyd(obs, books, alive, prev, done, thresh, iters, ws):
    """`iters` iterations of the loop inside scipy.cluster.vq.kmeans for the R = books.shape[0] restarts: obs (N, 2) f64,
    books (R, n, 2) f64, alive (R, n) int32, prev (R) f64, done (R) int32, all on the device and updated in place."""
    R, n, _ = books.shape
    _launch("sodt_kmeans_lloyd", _p(obs), obs.shape[0], _p(books), _p(alive), _p(prev), _p(done), R, n, C.c_double(thresh),
            int(iters), _p(ws), ws.numel() * ws.element_size())


CHOICES_BLOCK = L.CHOICES_BLOCK         # weights per block of the scan of weighted_choices (SODT_CHOICES_BLOCK)
CLASS_COUNTS_GRID = 1024 * 256          # labels that one grid of class_counts covers with one thread each


def class_counts(cls, img, n_img, nc, counts, class_total, status):
    """np.bincount per image and overall (general.py:227, :241): cls, img (M) int32; counts (n_img, nc) int32 and class_total
    (nc) int64 are ADDED to, status (1) int32 gets SODT_SAMPLING_BAD_* ORed in - the caller zeroes all three."""
    _launch("sodt_class_counts", _p(cls), _p(img), cls.numel(), int(n_img), int(nc), _p(counts), _p(class_total), _p(status))


def image_weights(counts, cw, iw):
    """iw[i] = sum_c cw[c] * counts[i][c] in f64, classes ascending (general.py:242): counts (n_img, nc) int32, cw (nc) f64."""
    n_img, nc = counts.shape
    _launch("sodt_image_weights", _p(counts), _p(cw), n_img, nc, _p(iw))


def weighted_choices_workspace_bytes(n: int, k: int) -> int:
    return _ws_bytes("sodt_weighted_choices_workspace_bytes", int(n), int(k))


def weighted_choices(iw, u, idx, cum, status, ws):
    """random.choices(range(n), weights=iw, k=k) from the k uniform numbers u: iw, cum (n) f64, u (k) f64, idx (k) int32,
    status (1) int32 (SODT_SAMPLING_*_TOTAL are ORed in), all on the device; no host read."""
    _launch("sodt_weighted_choices", _p(iw), iw.numel(), _p(u), u.numel(), _p(idx), _p(cum), _p(status), _p(ws),
            ws.numel() * ws.element_size())


def maxpool5_fwd(x, y, argmax, B, H, W, Cc, ldx=None, ldy=None, x_off=0, y_off=0):
    """y = MaxPool2d(5, 1, 2)(x), token-major; x / y may be channel slices of wider tensors (ld*, *_off in elements)."""
    es = x.element_size()
    _launch("sodt_maxpool5_fwd", x.data_ptr() + x_off * es, x.shape[-1] if ldx is None else ldx, y.data_ptr() + y_off * es,
            y.shape[-1] if ldy is None else ldy, _p(argmax), B, H, W, Cc, dt_code(x))


def maxpool5_bwd(dy, argmax, dx, B, H, W, Cc, lddy=None, lddx=None, dy_off=0, dx_off=0, accumulate=False):
    es = dy.element_size()
    _launch("sodt_maxpool5_bwd", dy.data_ptr() + dy_off * es, dy.shape[-1] if lddy is None else lddy, _p(argmax),
            dx.data_ptr() + dx_off * es, dx.shape[-1] if lddx is None else lddx, int(bool(accumulate)), B, H, W, Cc, dt_code(dy))


def gemm_set_variant(v) -> None:
    """Test hook (SODT_VARIANT_* in include/sodt_hip.h).  0/False: automatic; 1/True: the K-loop NT and the 128 x 128 TN kernel;
    2: A-stationary NT instead of B-stationary, no pipelined kernel; 3: NT as automatic, TN without the pipelined kernel."""
    _lib.sodt_gemm_set_variant(int(v))


def version() -> str:
    """Version string of the loaded library; a non-default library path (SODT_LIB_PATH) is part of it."""
    v = _lib.sodt_version().decode()
    ov = L.overrides() if hasattr(L, "overrides") else {}
    return v + (" [" + ", ".join(f"{k}={x}" for k, x in sorted(ov.items())) + "]" if ov else "")
