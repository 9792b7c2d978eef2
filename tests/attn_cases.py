"""Shared helpers of tests/test_attention_routes_gpu.py: the window-attention route table, the float64 reference with its
per-element error bounds, and the structured inputs whose answers are exact.  The bound derivation is in that module's
docstring; the constants here carry the same names."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24                                     # unit roundoff of the kernels' f32 arithmetic
U_T = {BF: 2.0 ** -8, F32: 2.0 ** -24}             # unit roundoff of a store to the run dtype
TINY = 1e-30                                       # absolute floor: f32 subnormal flushing of exp() results and products
NAN16, NAN32 = 0x7FC1, 0x7FC0A5A5                  # quiet-NaN sentinels (bit patterns no kernel produces)

# waves per workgroup of each (dtype, head dim) instantiation: sodt_window_attn_fwd / _bwd (csrc/attention.hip)
NW_FWD = {(BF, 16): 4, (BF, 32): 4, (BF, 64): 2, (F32, 16): 4, (F32, 32): 2, (F32, 64): 2}
NW_BWD = {(BF, 16): 4, (BF, 32): 2, (BF, 64): 1, (F32, 16): 2, (F32, 32): 2, (F32, 64): 1}
# instantiations whose 8x8-window (single 64-token tile) launches take the register-resident kernels: launch_fwd's
# 3 * DCH <= 12 and launch_bwd's PFOK (4 * DCH <= 16), DCH = 16-byte chunks per head row
FAST = {(BF, 16), (BF, 32), (F32, 16)}


def _ty(dt) -> str:
    return "bf16" if dt == BF else "float"


# ------------------------------------------------------------------ routes (re-derived from launch_fwd / launch_bwd / _wm / _rc)
def fwd_route(dt, hd: int, ws: int, shift: int) -> List[str]:
    t, nw = _ty(dt), NW_FWD[(dt, hd)]
    if ws == 8:
        if (dt, hd) in FAST:
            return [f"attn_fwd_fast_kernel<{t}, {hd}, {nw}>"]
        return [f"attn_fwd_kernel<{t}, {hd}, {nw}>"]
    if (dt, hd) == (BF, 16):                       # DCH = 2: neither multi-tile kernel is built for it
        return [f"attn_fwd_kernel<{t}, {hd}, {nw}>"]
    if shift == 0 and ws <= 32:
        return [f"attn_fwd_mt2_kernel<{t}, {hd}>"]
    return [f"attn_fwd_mt_kernel<{t}, {hd}>"]


def bwd_route(dt, hd: int, ws: int, shift: int) -> List[str]:
    t, nw = _ty(dt), NW_BWD[(dt, hd)]
    if ws == 8:
        if (dt, hd) in FAST:
            return [f"attn_bwd_fast2_kernel<{t}, {hd}, {nw}, false, false>"]
        return [f"attn_bwd_kernel<{t}, {hd}, {nw}, false>"]
    seq = [f"attn_delta_kernel<{t}>"]
    if (dt, hd) != (BF, 16) and shift == 0 and ws <= 32:
        return seq + [f"attn_bwd_dkv_kernel<{t}, {hd}>", f"attn_bwd_dq_kernel<{t}, {hd}>"]
    return seq + [f"attn_bwd_mt_kernel<{t}, {hd}, {nw}>", f"attn_dq_finish_kernel<{t}>"]


def bwd_wm_route(dt) -> List[str]:
    return [f"attn_bwd_fast2_kernel<{_ty(dt)}, 16, {4 if dt == BF else 2}, true, false>"]


RC_ROUTE = ["attn_bwd_fast2_kernel<bf16, 16, 4, true, true>"]


def attention_kernels(names: Sequence[str]) -> List[str]:
    """The kernels defined in csrc/attention.hip (all named attn_*) among canonical kernel names."""
    return [n for n in names if n.startswith("attn_")]


# ------------------------------------------------------------------ persistent grids (launch_fwd, bwd_persistent_grid, launch_bwd_rc)
def fwd_fast_grid(nwin: int) -> int:
    return min(nwin, 512)


def bwd_persistent_grid(nwin: int, ngroups: int, nw: int) -> int:
    resident = 256 * (2 if nw in (2, 4) else 4)
    return min(nwin, max(1, resident // max(ngroups, 1)))


def rc_grid(nwin: int) -> int:
    gx = bwd_persistent_grid(nwin, 3, 4)
    return gx // 8 * 8 if gx >= 8 else 8


# ------------------------------------------------------------------ geometry
class Geo:
    """Window bookkeeping of the reference: rows[w, n] is the token row of window-local position n of window w (windows in
    (b, wy, wx) order of the rolled frame, tokens row-major), region[w, n] its SW-MSA mask region (backbone_vit.py:1058-1077),
    rel[n, m] the relative-position index (backbone_vit.py:940-951)."""

    def __init__(self, B, H, W, C, heads, ws, shift, dev):
        from oracle import ref_torch as R
        self.B, self.H, self.W, self.C, self.heads, self.ws, self.shift = B, H, W, C, heads, ws, shift
        self.hd, self.N, self.M = C // heads, ws * ws, B * H * W
        self.nwy, self.nwx = H // ws, W // ws
        self.nwin = B * self.nwy * self.nwx
        idx = torch.arange(self.M, dtype=torch.float64).view(B, H, W, 1)
        if shift:
            idx = torch.roll(idx, (-shift, -shift), (1, 2))
        self.rows = R.window_partition(idx, ws).view(self.nwin, self.N).long().to(dev)
        img = torch.zeros((1, H, W, 1), dtype=torch.float64)
        if shift:
            cnt = 0
            for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                    img[:, hs, wsl, :] = cnt
                    cnt += 1
        reg = R.window_partition(img, ws).view(-1, self.N)                       # [nWy * nWx][N], the same for every b
        self.region = reg.repeat(B, 1).long().to(dev)
        self.rel = R.relative_position_index(ws).to(dev)
        self.L2 = (2 * ws - 1) ** 2

    def split(self, t: torch.Tensor, part: int) -> torch.Tensor:
        """[M][3C] (part 0/1/2 = q/k/v) or [M][C] (part None) -> [nwin][heads][N][hd] float64."""
        c0 = 0 if part is None else part * self.C
        x = t.double()[:, c0:c0 + self.C][self.rows]                               # [nwin][N][C]
        return x.view(self.nwin, self.N, self.heads, self.hd).permute(0, 2, 1, 3)

    def merge(self, x: torch.Tensor) -> torch.Tensor:
        """[nwin][heads][N][hd] -> [M][C] in natural token order."""
        out = torch.empty(self.M, self.C, dtype=x.dtype, device=x.device)
        out[self.rows] = x.permute(0, 2, 1, 3).reshape(self.nwin, self.N, self.C)
        return out

    def per_row(self, x: torch.Tensor) -> torch.Tensor:
        """[nwin][heads][N] -> [M][heads]."""
        out = torch.empty(self.M, self.heads, dtype=x.dtype, device=x.device)
        out[self.rows] = x.permute(0, 2, 1)
        return out

    def windows_of(self, x: torch.Tensor) -> torch.Tensor:
        """[M][heads] -> [nwin][heads][N]."""
        return x.double()[self.rows].permute(0, 2, 1)

    def mask(self) -> torch.Tensor:
        """[nwin][1][N][N] bool: query and key in different regions (the reference adds -100 there)."""
        r = self.region
        return (r[:, :, None] != r[:, None, :]).unsqueeze(1)


# ------------------------------------------------------------------ float64 reference and bounds
def reference(g: Geo, qkv: torch.Tensor, bias_t: torch.Tensor, dt, *, eta: float = 0.0, q_eff: Optional[torch.Tensor] = None,
              k_eff: Optional[torch.Tensor] = None, v_eff: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Forward reference and its per-element bounds from the kernel's actual (dtype-rounded) inputs.  eta: relative
    uncertainty of the operands themselves (the recomputing backward rounds q / k / v it forms itself)."""
    scale = g.hd ** -0.5
    q = g.split(qkv, 0) if q_eff is None else q_eff
    k = g.split(qkv, 1) if k_eff is None else k_eff
    v = g.split(qkv, 2) if v_eff is None else v_eff
    bias = bias_t.double()[:, g.rel]                                                # [heads][N][N]
    msk = g.mask().double()
    S = scale * (q @ k.transpose(-1, -2)) + bias.unsqueeze(0) - 100.0 * msk
    A = scale * (q.abs() @ k.abs().transpose(-1, -2)) + bias.abs().unsqueeze(0) + 100.0 * msk
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.unsqueeze(-1))
    O = P @ v
    E = (g.hd + 8) * U * A + 4 * U * (lse.abs().unsqueeze(-1) + 1) + 2 * eta * scale * (q.abs() @ k.abs().transpose(-1, -2))
    Ebar = (P * E).sum(-1, keepdim=True)
    uP = U_T[dt] if dt == BF else 0.0
    Pv = P @ v.abs()
    out_bound = (P * (E + Ebar + uP)) @ v.abs() + ((g.N + 8) * U + eta) * Pv + U_T[dt] * O.abs() + TINY
    lse_bound = Ebar.squeeze(-1) + (g.N + 8) * U + 4 * U * lse.abs() + TINY
    return dict(q=q, k=k, v=v, S=S, P=P, O=O, lse=lse, E=E, out_bound=out_bound, lse_bound=lse_bound, scale=scale, eta=eta)


def reference_bwd(g: Geo, f: Dict[str, torch.Tensor], dt, dout: torch.Tensor, out_k: Optional[torch.Tensor], lse_k: torch.Tensor,
                  prefill: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Backward reference (analytic, float64) and its bounds, given the kernel's own log-sum-exp and, when the route reads it
    (ws > 8: attn_delta_kernel), its forward output; and the dbias_t prefill it must accumulate onto.  out_k None: the route
    forms delta itself from the P it recomputes."""
    q, k, v, P, scale, eta = f["q"], f["k"], f["v"], f["P"], f["scale"], f["eta"]
    dO = g.split(dout, None)
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * f["O"]).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dV = P.transpose(-1, -2) @ dO
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    rho = f["E"] + (g.windows_of(lse_k) - f["lse"]).abs().unsqueeze(-1) + 4 * U * (f["lse"].abs().unsqueeze(-1) + 1)
    e_dP = ((g.hd + 4) * U + 2 * eta) * (dO.abs() @ v.abs().transpose(-1, -2))
    if out_k is not None:
        ok = g.split(out_k, None)
        d_delta = ((dO * (ok - f["O"])).sum(-1, keepdim=True)).abs() + (g.hd + 4) * U * (dO.abs() * ok.abs()).sum(-1, keepdim=True)
    else:
        d_delta = (P * (rho + (g.N + g.hd + 8) * U + 2 * eta) * (dO.abs() @ v.abs().transpose(-1, -2))).sum(-1, keepdim=True)
    eS = P * (rho * (dP - delta).abs() + e_dP + d_delta) * (1 + 2 * rho)
    uP, uT, acc = (U_T[dt] if dt == BF else 0.0), U_T[dt], (g.N + 8) * U
    aS = dS.abs()
    dSerr = eS + uP * aS
    dV_b = (P * (rho + uP)).transpose(-1, -2) @ dO.abs() + acc * (P.transpose(-1, -2) @ dO.abs()) + uT * dV.abs() + TINY
    dQ_b = scale * (dSerr @ k.abs() + (acc + eta) * (aS @ k.abs())) + uT * dQ.abs() + TINY
    dK_b = scale * (dSerr.transpose(-1, -2) @ q.abs() + (acc + eta) * (aS.transpose(-1, -2) @ q.abs())) + uT * dK.abs() + TINY
    # the relative-position-bias gradient: every (window, query, key) with the same table entry, summed in some order
    idx = g.rel.view(-1)
    H = g.heads

    def scatter(x):                                                      # [nwin][heads][N][N] -> [heads][L2]
        s = x.sum(0).reshape(H, -1)
        return torch.zeros(H, g.L2, dtype=x.dtype, device=x.device).index_add_(1, idx, s)
    cnt = torch.zeros(g.L2, dtype=torch.float64, device=dS.device).index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
    cnt = cnt * g.nwin + 2
    db = scatter(dS)
    db_b = scatter(dSerr) + cnt * U * (scatter(aS) + prefill.double().abs()) + TINY
    dqkv = torch.cat((g.merge(dQ), g.merge(dK), g.merge(dV)), 1)
    dqkv_b = torch.cat((g.merge(dQ_b), g.merge(dK_b), g.merge(dV_b)), 1)
    return dict(dqkv=dqkv, dqkv_bound=dqkv_b, dbias=db, dbias_bound=db_b, dS=dS)


# ------------------------------------------------------------------ inputs
def randn(shape, seed: int, dev, scale=1.0, dtype=torch.float32) -> torch.Tensor:
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(tuple(shape), generator=gen) * scale).to(dtype).to(dev)


def nan_buffer(rows: int, cols: int, dtype, dev, pad: int = 2):
    """A [pad + rows + pad][cols] buffer of quiet NaN sentinels and its middle view."""
    buf = torch.empty((rows + 2 * pad, cols), device=dev, dtype=dtype)
    iv = buf.view(torch.int16) if buf.element_size() == 2 else buf.view(torch.int32)
    iv.fill_(NAN16 if buf.element_size() == 2 else NAN32)
    return buf, buf[pad:pad + rows]


def sentinel_bits(buf: torch.Tensor) -> torch.Tensor:
    iv = buf.view(torch.int16) if buf.element_size() == 2 else buf.view(torch.int32)
    want = NAN16 if buf.element_size() == 2 else NAN32
    return iv == want


def code_bits(n: torch.Tensor, nb: int) -> torch.Tensor:
    """[..] window-local positions -> [..][nb] +-1 codes (binary digits)."""
    sh = torch.arange(nb, device=n.device)
    return ((n.unsqueeze(-1) >> sh) & 1).double() * 2 - 1


# selection codes: q . k is gamma^2 (nb - 2 hamming) - gamma^2 nb, so the target logit is 0 and every other key of the same
# region sits at scale * -2 gamma^2 * hamming <= -40; gamma per head dim keeps 2 gamma^2 scale >= 40 with integer codes
GAMMA = {16: 9, 32: 11, 64: 13}


def selection_inputs(g: Geo, dt, seed: int, dev, cross: bool):
    """q / k / v / dout for the selection case and the chosen target key (window-local) of each query.  Each window and mask
    region gets a random permutation of its keys as targets.  cross: in each window with two or more regions, two queries of
    different regions swap their targets and win them through a boost channel by 160 logits (> 100 + 40)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    N, hd, H = g.N, g.hd, g.heads
    nb = max(1, int(math.ceil(math.log2(N))))
    gam = GAMMA[hd]
    assert nb + 3 <= hd
    tgt = torch.empty(g.nwin, H, N, dtype=torch.long)
    reg = g.region.cpu()
    boost = []                                       # (window, head, query a, query b)
    for w in range(g.nwin):
        for h in range(H):
            for r in torch.unique(reg[w]).tolist():
                mem = (reg[w] == r).nonzero().flatten()
                tgt[w, h, mem] = mem[torch.randperm(mem.numel(), generator=gen)]
            if cross and torch.unique(reg[w]).numel() > 1:
                a = int(torch.randint(N, (1,), generator=gen))
                others = (reg[w] != reg[w, a]).nonzero().flatten()
                b = int(others[torch.randint(others.numel(), (1,), generator=gen)])
                tgt[w, h, a], tgt[w, h, b] = int(tgt[w, h, b]), int(tgt[w, h, a])
                boost.append((w, h, a, b))
    tgt = tgt.to(dev)
    n = torch.arange(N, device=dev)
    kcode = torch.zeros(g.nwin, H, N, hd, dtype=torch.float64, device=dev)
    kcode[..., :nb] = gam * code_bits(n, nb)
    kcode[..., hd - 1] = gam
    qcode = torch.zeros_like(kcode)
    qcode[..., :nb] = gam * code_bits(tgt, nb)
    qcode[..., hd - 1] = -gam * nb
    # boost: query a gets channel hd-2, query b channel hd-3; their targets carry the matching key value
    bq, bk = {16: (40, 16), 32: (40, 23), 64: (40, 32)}[hd]        # scale * bq * bk >= 160
    for (w, h, a, b) in boost:
        qcode[w, h, a, hd - 2] = bq
        kcode[w, h, int(tgt[w, h, a]), hd - 2] = bk
        qcode[w, h, b, hd - 3] = bq
        kcode[w, h, int(tgt[w, h, b]), hd - 3] = bk
    # v: small non-zero integers identifying the source token's row; dout likewise (exact in bf16: |x| <= 256)
    rows = torch.arange(g.M, device=dev).unsqueeze(1)
    c = torch.arange(g.C, device=dev).unsqueeze(0)
    vrow = ((rows * (2 * c + 3) + 7 * c) % 61 + 1) * (1 - 2 * ((rows + c) % 2))
    dorow = ((rows * (c + 5) + 3 * c) % 29 + 1) * (1 - 2 * ((rows // 3 + c) % 2))
    qkv = torch.cat((g.merge(qcode), g.merge(kcode), vrow.double()), 1).to(dt)
    return qkv, dorow.double().to(dt), tgt, boost


def onehot_bias_inputs(g: Geo, dt, dev, beta: float = 60.0):
    """q = k = 0; head h's bias table is beta on one relative offset (different per head) and 0 elsewhere.  Returns qkv,
    bias_t and the offsets (dy, dx) = query - key."""
    offs = [(0, 1), (1, 0), (-1, -1), (2, -3), (-3, 2), (1, 1), (0, -2), (-2, 0)]
    bias_t = torch.zeros(g.heads, g.L2, device=dev)
    L = 2 * g.ws - 1
    for h in range(g.heads):
        dy, dx = offs[h % len(offs)]
        bias_t[h, (dy + g.ws - 1) * L + dx + g.ws - 1] = beta
    rows = torch.arange(g.M, device=dev).unsqueeze(1)
    c = torch.arange(g.C, device=dev).unsqueeze(0)
    v = ((rows * (2 * c + 3) + 5 * c) % 61 + 1).double()
    qkv = torch.cat((torch.zeros(g.M, 2 * g.C, device=dev, dtype=torch.float64), v), 1).to(dt)
    return qkv, bias_t, [offs[h % len(offs)] for h in range(g.heads)]
