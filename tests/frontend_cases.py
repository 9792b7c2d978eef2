"""Shared helpers of tests/test_frontend_routes_gpu.py and tests/test_frontend_ref_host.py: the case tables and the route table
of the front-end kernels (csrc/frontend.hip, csrc/cattn.hip), the float64 reference (oracle/ref_torch.py) with its
per-element error bounds, the mutated statements the host test holds the bounds against, and the structured inputs whose
answers are exact.  The bound derivation is in the docstring of tests/test_frontend_routes_gpu.py; the constants here carry the
same names."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

import attn_cases as A

BF, F32 = A.BF, A.F32
U, U_T, TINY = A.U, A.U_T, A.TINY
CE, NH, HD = 48, 12, 4
PAIR_KV = (1, 2, 3, 1)                              # key/value plane of pair p (query plane p): backbone_vit.py:508-521
FE_PART = 4 * CE * 19                               # csrc/frontend.hip: floats per workgroup row of the workspace
FE_BWD_GRID = 512
FE_RG = 32
WS_FLOATS = FE_BWD_GRID * FE_PART                   # sodt_frontend_bwd_workspace_bytes / 4
K_E = 17                                            # an embedding: 16 multiply-adds onto the bias (and one spare)
K_LN = 50                                           # a 48-term sum or sum of squares, the subtraction, rsqrtf


def w_scale_general(ws: int) -> float:
    """The general cases scale the embedding weights by 3 (score standard deviation about 2): the median largest attention
    probability is then at least 3 / N for N >= 16.  With the four keys of ws = 2 that takes 0.75, which takes a scale of 5."""
    return 5.0 if ws == 2 else 3.0


# ------------------------------------------------------------------ cases, read as (B, H, W)
FUSED_CASES = [(1, 4, 4), (2, 8, 260), (1, 256, 256), (1, 256, 260), (3, 420, 420)]
THREE_WAY = [(1, 256, 260), (3, 420, 420)]          # backward with ws=None / a NaN workspace / a workspace one float short
STRIDE_CASE = (2, 8, 260)                           # the IR stride cases and window 1 through both routes
# (B, H, W, ws, shift)
GENERAL_CASES = [(1, 48, 48, 2, 0), (1, 48, 48, 2, 1), (1, 48, 48, 4, 3), (1, 32, 32, 8, 7), (2, 32, 96, 8, 3), (3, 16, 24, 2, 1)]
FINITE_CASE = (1, 32, 32, 4, 2)
EXACT_CASE = (2, 8, 12)

MUTANTS = {1: "pair 3 reads B where the reference reads G", 2: "mask added after the scale", 3: "mask as -inf",
           4: "R read without its -1 shift", 5: "taps transposed within the patch", 6: "beta of pair p from pair (p + 1) % 4",
           7: "scale 1/sqrt(48)", 8: "db credited to the query plane only", 9: "dsc factor 0.5 dropped in de",
           10: "ir_bstride ignored"}
_EMBED = [("fused",) + STRIDE_CASE, ("general", 1, 48, 48, 4, 3), ("general", 3, 16, 24, 2, 1)]
_WINDOWED = [("general",) + c for c in GENERAL_CASES]
# mutant -> the cases that must catch it (1 % of the elements of a gated tensor over the bound of both dtypes)
MUTANT_CASES = {1: _EMBED, 4: _EMBED, 5: _EMBED, 6: _EMBED, 8: _EMBED,
                10: [("fused",) + STRIDE_CASE, ("general", 3, 16, 24, 2, 1), ("general", 2, 32, 96, 8, 3)],
                2: [("finite",) + FINITE_CASE], 3: [("finite",) + FINITE_CASE],
                7: _WINDOWED + [("finite",) + FINITE_CASE], 9: _WINDOWED + [("finite",) + FINITE_CASE]}


def case_id(c) -> str:
    return "-".join(str(v) for v in c)


def _ty(dt) -> str:
    return "bf16" if dt == BF else "float"


# ------------------------------------------------------------------ routes (re-derived from sodt_frontend_bwd and cattn.hip's entries)
def fused_bwd_route(dt, ntok: int, ws_floats: Optional[int]) -> Dict:
    """sodt_frontend_bwd's dispatch: two stages when a workspace of at least WS_FLOATS floats is given and there are more than
    64 blocks of 64 tokens; the grid is capped at 512 (two stages) or 256.  trips: the most grid-stride trips of one workgroup;
    depth: the longest chain of f32 additions one gradient element can pass through (see the bound derivation)."""
    nblk = (ntok + 63) // 64
    two = ws_floats is not None and ws_floats >= WS_FLOATS and nblk > 64
    grid = min(nblk, FE_BWD_GRID if two else FE_BWD_GRID // 2)
    trips = (nblk + grid - 1) // grid
    t = _ty(dt)
    if two:
        groups = (grid + FE_RG - 1) // FE_RG
        return dict(kernels=[f"frontend_bwd_kernel<{t}, true>", "frontend_bwd_reduce_kernel"], two_stage=True, nblk=nblk, grid=grid,
                    trips=trips, reduce_grid=(FE_PART // 64, groups), depth=64 * trips + 8 + FE_RG + 3 * groups)
    return dict(kernels=[f"frontend_bwd_kernel<{t}, false>"], two_stage=False, nblk=nblk, grid=grid, trips=trips,
                reduce_grid=None, depth=64 * trips + 8 + 3 * grid)


def fused_fwd_route(dt) -> List[str]:
    return [f"frontend_fwd_kernel<{_ty(dt)}>"]


GENERAL_FWD = lambda dt: ["patch_embed4_fwd_kernel", f"cross_attn_ln_fwd_kernel<{_ty(dt)}>"]      # noqa: E731
GENERAL_BWD = lambda dt: [f"cross_attn_ln_bwd_kernel<{_ty(dt)}>", "patch_embed4_bwd_kernel"]      # noqa: E731


def general_depths(ntok: int, N: int) -> Dict[str, int]:
    """cross_attn_ln_bwd: four shuffles, then one atomic per wave (16 tokens) and pair; de: one query-path atomic and N key-path
    atomics for each of at most two pairs that read the plane as key/value.  patch_embed4_bwd: grid.y = min(ntok, 512) threads
    walk the tokens of one output, then one atomic each."""
    gy = min(ntok, 512)
    return dict(gamma=5 + (ntok + 15) // 16, de=2 * N + 2, embed=(ntok + gy - 1) // gy + gy)


# torch's demangler (the profiler's names) mis-reads the bf16 type in front of a bool template argument; of the front-end
# kernels that happens to this one instantiation alone (tests/test_frontend_ref_host.py checks every symbol of the library)
_UNREADABLE = {"frontend_bwd_kernel<unreadable>": "frontend_bwd_kernel<bf16, true>"}


def canonical(name: str) -> str:
    """gemm_cases.canonical_kernel on a kernel name of csrc/frontend.hip / csrc/cattn.hip."""
    import gemm_cases as G
    n = G.canonical_kernel(name)
    return _UNREADABLE.get(n, n)


def frontend_kernels(names: Sequence[str]) -> List[str]:
    """The kernels of csrc/frontend.hip and csrc/cattn.hip among canonical kernel names."""
    return [_UNREADABLE.get(n, n) for n in names if n.startswith(("frontend_", "patch_embed4_", "cross_attn_ln_"))]


ALL_ROUTE_NAMES = sorted({n for dt in (BF, F32) for n in fused_fwd_route(dt) + GENERAL_FWD(dt) + GENERAL_BWD(dt)
                          + fused_bwd_route(dt, 65 * 64, WS_FLOATS)["kernels"] + fused_bwd_route(dt, 64, None)["kernels"]})


# ------------------------------------------------------------------ inputs
def rand_inputs(B: int, H: int, W: int, seed: int, w_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """U[0,1) images (rgb and a three-plane IR tensor whose planes differ), normal parameters; all f32 on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return dict(rgb=torch.rand(B, 3, H, W, generator=g), ir3=torch.rand(B, 3, H, W, generator=g),
                w=torch.randn(4, CE, 16, generator=g) * (0.25 * w_scale), b=torch.randn(4, CE, generator=g) * 0.1,
                gamma=1.0 + 0.2 * torch.randn(4, CE, generator=g), beta=0.3 * torch.randn(4, CE, generator=g))


def rand_dout(M: int, dt, seed: int) -> torch.Tensor:
    return A.randn((M, 4 * CE), seed, "cpu").to(dt)


def x4_of(rgb: torch.Tensor, ir_plane: torch.Tensor) -> torch.Tensor:
    return torch.cat((rgb, ir_plane.unsqueeze(1)), 1)


def finite_mask_e(B: int, H: int, W: int, ws: int, shift: int, seed: int) -> torch.Tensor:
    """e [M][192] f32 for the finite-mask case.  Within one window the mask region of a token is one of at most four, told
    apart by (last row band, last column band); u is the one-hot 4-vector of that code.  R = -11 u, G = +11 u, B = -11 u and
    IR = -11 u in the even heads, +11 u in the odd ones (+ U(-0.5, 0.5) noise everywhere), so that before the mask a key of the
    query's own region scores about -121 and a key of another region about 0 in every head of pairs 0 and 1, in the even heads
    of pair 3 and the odd heads of pair 2: after (score - 100) / 2 the masked keys win by about e^10.  (No sign of IR serves
    both pair 2, where it is the key, and pair 3, where it is the query of G: in the other heads the query's own region wins.)"""
    th, tw = H // 4, W // 4
    g = torch.Generator(device="cpu").manual_seed(seed)
    y = (torch.arange(th) - shift) % th
    x = (torch.arange(tw) - shift) % tw
    code = 2 * (y >= th - shift).long().view(th, 1) + (x >= tw - shift).long().view(1, tw)          # [th][tw]
    u = F.one_hot(code, 4).float().view(1, th, tw, 1, 1, 4).expand(B, th, tw, 4, NH, 4).clone()
    sign = torch.tensor([-1.0, 1.0, -1.0, -1.0]).view(1, 1, 1, 4, 1, 1).expand(1, 1, 1, 4, NH, 1).clone()
    sign[..., 3, 1::2, :] = 1.0
    e = 11.0 * sign * u + (torch.rand(B, th, tw, 4, NH, 4, generator=g) - 0.5)
    return e.reshape(B * th * tw, 4 * CE).contiguous()


def exact_embed_inputs(B: int, H: int, W: int) -> Dict[str, torch.Tensor]:
    """Small-integer images; channel ch of plane p reads tap (5 ch + 3 p) % 16 alone, times 2^p; the bias of plane p is
    2^-(p + 1): every embedding is exact in f32.  Columns 0..7 of every plane are constant (a different small integer per plane
    and image), which makes e constant over the channels at the tokens whose whole patch lies there."""
    g = torch.Generator(device="cpu").manual_seed(H * 7 + W)
    rgb = torch.randint(0, 16, (B, 3, H, W), generator=g).float()
    ir3 = torch.randint(0, 16, (B, 3, H, W), generator=g).float()
    for t, off in ((rgb, 1), (ir3, 7)):
        for bi in range(B):
            for p in range(3):
                t[bi, p, :, :8] = float(off + 3 * p + 5 * bi)
    w = torch.zeros(4, CE, 16)
    for p in range(4):
        for ch in range(CE):
            w[p, ch, (5 * ch + 3 * p) % 16] = 2.0 ** p
    b = torch.stack([torch.full((CE,), 2.0 ** -(p + 1)) for p in range(4)])
    beta = (2.0 ** (torch.arange(4 * CE, dtype=torch.float64) - 96)).float().view(4, CE)            # exact in bf16 as well
    return dict(rgb=rgb, ir3=ir3, w=w, b=b, gamma=torch.ones(4, CE), beta=beta)


# ------------------------------------------------------------------ float64 reference (oracle/ref_torch.py)
def _sd(w, b, gamma, beta) -> Dict[str, torch.Tensor]:
    sd = {}
    for p, c in enumerate("rgbi"):
        sd[f"image_encoder.channel_embed_{c}.proj.weight"] = w[p].reshape(CE, 1, 4, 4)
        sd[f"image_encoder.channel_embed_{c}.proj.bias"] = b[p]
        sd[f"image_encoder.chan_block.norm{p + 1}.weight"] = gamma[p]
        sd[f"image_encoder.chan_block.norm{p + 1}.bias"] = beta[p]
    return sd


def reference(x4, w, b, gamma, beta, ws: int, shift: int, dout, dtype=torch.float64, e_given=None) -> Dict[str, torch.Tensor]:
    """channel_embeds -> cattention_block -> cat, and the gradients by autograd, all in `dtype` on the CPU.  The four embedding
    planes are leaves of the attention graph: de is their gradient, and dw / db come from a second graph (the embeddings
    alone) fed with de.  e_given [M][192]: the embeddings themselves (no dw / db)."""
    from oracle import ref_torch as R
    w, b, gamma, beta = (t.detach().to(dtype).clone().requires_grad_() for t in (w, b, gamma, beta))
    sd = _sd(w, b, gamma, beta)
    if e_given is None:
        Bn, _, H, W = x4.shape
        planes = R.channel_embeds(sd, x4.to(dtype))
        e = torch.cat(planes, -1)
    else:
        Bn, H, W = x4
        e = e_given.to(dtype).view(Bn, H // 4, W // 4, 4 * CE)
    el = e.detach().clone().requires_grad_()
    out = torch.cat(R.cattention_block(sd, *el.split(CE, -1), window_size=ws, shift=shift), -1).reshape(-1, 4 * CE)
    out.backward(dout.to(dtype))
    res = dict(e=e.detach().reshape(-1, 4 * CE), out=out.detach(), de=el.grad.reshape(-1, 4 * CE), dgamma=gamma.grad, dbeta=beta.grad)
    if e_given is None:
        e.backward(el.grad)
        res["dw"], res["db"] = w.grad, b.grad
    return res


def patches_of(x4: torch.Tensor, r_pad: int = 1, transpose: bool = False) -> torch.Tensor:
    """[M][4][16] float64: the 4 x 4 patch of every plane at every token, taps row-major; R with padding r_pad."""
    Bn = x4.shape[0]
    ps = []
    for p in range(4):
        u = F.unfold(x4[:, p:p + 1].double(), 4, stride=4, padding=r_pad if p == 0 else 0)          # [B][16][L]
        u = u.permute(0, 2, 1).reshape(-1, 4, 4)
        ps.append((u.transpose(1, 2) if transpose else u).reshape(-1, 16))
    assert ps[0].shape[0] == Bn * (x4.shape[2] // 4) * (x4.shape[3] // 4)
    return torch.stack(ps, 1)


def statement(x4, w, b, gamma, beta, ws: int, shift: int, dout, mutant: Optional[int] = None, e_given=None) -> Dict[str, torch.Tensor]:
    """The same statement written out (float64), with the knobs of MUTANTS.  mutant None reproduces reference() (the host test
    checks that), so that a mutant differs from the reference by its one change alone."""
    if e_given is None:
        Bn, _, H, W = x4.shape
        x4 = x4.double()
        if mutant == 10:
            x4 = torch.cat((x4[:, :3], x4[:1, 3:].expand(Bn, 1, H, W)), 1)
        pt = patches_of(x4, r_pad=0 if mutant == 4 else 1)
        wd = w.double()
        if mutant == 5:
            wd = wd.view(4, CE, 4, 4).transpose(2, 3).reshape(4, CE, 16)
        e = (torch.einsum("mpk,pjk->mpj", pt, wd) + b.double()).reshape(-1, 4 * CE)
    else:
        Bn, H, W = x4
        e = e_given.double()
    g = A.Geo(Bn, H // 4, W // 4, CE, NH, ws, shift, "cpu")
    eq = e.detach().clone().requires_grad_()
    ekv = e.detach().clone().requires_grad_()
    gam = gamma.double().clone().requires_grad_()
    bet = beta.double().clone().requires_grad_()
    msk = g.mask()
    outs = []
    for p in range(4):
        kvp = 2 if (mutant == 1 and p == 3) else PAIR_KV[p]
        q = g.split(eq[:, p * CE:(p + 1) * CE], None)
        k = g.split(ekv[:, kvp * CE:(kvp + 1) * CE], None)
        s = q @ k.transpose(-1, -2)
        scale = 1.0 / math.sqrt(CE) if mutant == 7 else 0.5
        if mutant == 2:
            s = s * scale - 100.0 * msk
        elif mutant == 3:
            s = s.masked_fill(msk, float("-inf")) * scale
        else:
            s = s - 100.0 * msk
            s = (s.detach() * scale + (s - s.detach())) if mutant == 9 else s * scale
        o = g.merge(torch.softmax(s, -1) @ k)
        bp = (p + 1) % 4 if mutant == 6 else p
        outs.append(F.layer_norm(eq[:, p * CE:(p + 1) * CE] + o, (CE,), gam[p], bet[bp], 1e-5))
    out = torch.cat(outs, -1)
    out.backward(dout.double())
    de = eq.grad + ekv.grad
    dbeta = bet.grad if mutant != 6 else torch.roll(bet.grad, -1, 0)      # (the mutant reads another beta; it still writes dbeta[p])
    res = dict(e=e.detach(), out=out.detach(), de=de, dgamma=gam.grad, dbeta=dbeta)
    if e_given is None:
        d3 = de.view(-1, 4, CE)
        res["dw"] = torch.einsum("mpj,mpk->pjk", d3, pt)
        res["db"] = (eq.grad if mutant == 8 else de).view(-1, 4, CE).sum(0)
    return res


# ------------------------------------------------------------------ bounds
def bounds(x4, w, b, gamma, beta, ws: int, shift: int, dout, dt, ref: Dict[str, torch.Tensor], depth: Dict[str, int],
           e_given=None, de_exact: bool = False) -> Dict[str, torch.Tensor]:
    """Per-element bounds of every gated tensor around `ref` (see the derivation in tests/test_frontend_routes_gpu.py).
    depth: the addition-chain depths of the route's sums, keys gamma (dgamma / dbeta), de, embed (dw / db).  de_exact: dw / db
    are computed from a stored de that is the reference's own (patch_embed4_bwd judged on its own input)."""
    gam, bet, dy = gamma.double(), beta.double(), dout.double().view(-1, 4, CE)
    e = ref["e"].double()
    M = e.shape[0]
    if e_given is None:
        Bn, _, H, W = x4.shape
        pt = patches_of(x4).abs()                                                                     # [M][4][16]
        Ae = torch.einsum("mpk,pjk->mpj", pt, w.double().abs()) + b.double().abs()                   # [M][4][48]
        dE = K_E * U * Ae
    else:
        Bn, H, W = x4
        pt, dE = None, torch.zeros(M, 4, CE, dtype=torch.float64)
    g = A.Geo(Bn, H // 4, W // 4, CE, NH, ws, shift, "cpu")
    N = g.N
    msk = g.mask().double()
    e3 = e.view(M, 4, CE)
    s3, ds_err3 = torch.empty_like(e3), torch.empty_like(e3)
    fw = []
    for p in range(4):
        kvp = PAIR_KV[p]
        q, k = g.split(e3[:, p], None), g.split(e3[:, kvp], None)
        dq_e, dk_e = g.split(dE[:, p], None), g.split(dE[:, kvp], None)
        qk = q @ k.transpose(-1, -2)
        aqk = q.abs() @ k.abs().transpose(-1, -2)
        S = 0.5 * (qk - 100.0 * msk)
        Es = 0.5 * (dq_e @ k.abs().transpose(-1, -2) + q.abs() @ dk_e.transpose(-1, -2) + 5 * U * aqk + U * (aqk + 100.0) * msk) + U * S.abs()
        P = torch.softmax(S, -1)
        top = S.max(-1, keepdim=True).values
        rng = top - S.min(-1, keepdim=True).values
        rho = Es + (P * Es).sum(-1, keepdim=True) + (8 * N + 4 * (top - S) + 4 * rng + 8) * U
        Pv = P @ k.abs()
        o = P @ k
        do = (P * rho) @ k.abs() + P @ dk_e + (N + 2) * U * Pv
        s = q + o
        s3[:, p] = g.merge(s)
        ds_err3[:, p] = g.merge(dq_e + do + U * s.abs())
        fw.append(dict(q=q, k=k, dq_e=dq_e, dk_e=dk_e, P=P, rho=rho))
    # LayerNorm forward
    mean = s3.mean(-1, keepdim=True)
    d = s3 - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    xh = d * rstd
    dsn = ds_err3 + U * d.abs() + (K_LN - 1) * U * s3.abs().mean(-1, keepdim=True)
    mxd = (xh.abs() * dsn).mean(-1, keepdim=True)
    X = rstd * (dsn + dsn.mean(-1, keepdim=True) + xh.abs() * mxd) + 32 * U * xh.abs()
    out = xh * gam + bet
    out_b = (gam.abs() * X + 2 * U * ((xh * gam).abs() + bet.abs())) * (1 + U_T[dt]) + U_T[dt] * out.abs() + TINY
    res = dict(out=out_b.reshape(M, 4 * CE))
    if e_given is None:
        res["e"] = (dE + TINY).reshape(M, 4 * CE)
    # LayerNorm backward
    Dg = depth["gamma"]
    res["dgamma"] = (dy.abs() * X).sum(0) + (Dg + 2) * U * (dy * xh).abs().sum(0) + TINY
    res["dbeta"] = Dg * U * dy.abs().sum(0) + TINY
    gg = dy * gam
    c2 = (gg * xh).mean(-1, keepdim=True)
    ds = rstd * (gg - gg.mean(-1, keepdim=True) - xh * c2)
    A_ds = rstd * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
    r = rstd * mxd + 27 * U
    dds = r * ds.abs() + rstd * (X * c2.abs() + xh.abs() * (gg.abs() * X).mean(-1, keepdim=True)) + (K_LN + 6) * U * A_ds
    # attention backward
    de_b = torch.zeros_like(e3)
    A_de = torch.zeros_like(e3)
    for p in range(4):
        kvp, f = PAIR_KV[p], fw[p]
        q, k, P, rho, dq_e, dk_e = f["q"], f["k"], f["P"], f["rho"], f["dq_e"], f["dk_e"]
        dO, ddO = g.split(ds[:, p], None), g.split(dds[:, p], None)
        kT, akT = k.transpose(-1, -2), k.abs().transpose(-1, -2)
        dp = dO @ kT
        adp = dO.abs() @ akT
        ddp = ddO @ akT + dO.abs() @ dk_e.transpose(-1, -2) + 5 * U * adp
        delta = (P * dp).sum(-1, keepdim=True)
        ddelta = (P * (rho * dp.abs() + ddp)).sum(-1, keepdim=True) + (N + 2) * U * (P * dp.abs()).sum(-1, keepdim=True)
        dsc = 0.5 * P * (dp - delta)
        ddsc = 0.5 * P * (rho * (dp - delta).abs() + ddp + ddelta + 3 * U * (dp.abs() + delta.abs()))
        a_dq = dO.abs() + dsc.abs() @ k.abs()
        b_dq = ddO + ddsc @ k.abs() + dsc.abs() @ dk_e + (N + 3) * U * a_dq
        PT, dscT = P.transpose(-1, -2), dsc.abs().transpose(-1, -2)
        a_dkv = PT @ dO.abs() + dscT @ q.abs()
        b_dkv = (P * rho).transpose(-1, -2) @ dO.abs() + PT @ ddO + ddsc.transpose(-1, -2) @ q.abs() + dscT @ dq_e + (N + 6) * U * a_dkv
        de_b[:, p] += g.merge(b_dq)
        A_de[:, p] += g.merge(a_dq)
        de_b[:, kvp] += g.merge(b_dkv)
        A_de[:, kvp] += g.merge(a_dkv)
    res["de"] = (de_b + depth["de"] * U * A_de + TINY).reshape(M, 4 * CE)
    if e_given is None:
        De = depth["embed"]
        if de_exact:
            de_b, A_de = torch.zeros_like(e3), ref["de"].double().abs().view(M, 4, CE)
        else:
            de_b = de_b + depth["de"] * U * A_de
        x = 1 if de_exact else 0                                         # (the reference's de is rounded to f32 on its way in)
        res["dw"] = torch.einsum("mpj,mpk->pjk", de_b, pt) + (De + 2 + x) * U * torch.einsum("mpj,mpk->pjk", A_de, pt) + TINY
        res["db"] = de_b.sum(0) + (De + x) * U * A_de.sum(0) + TINY
    return res


def probabilities(e: torch.Tensor, Bn: int, H: int, W: int, ws: int, shift: int):
    """[4 pairs] of (P [nwin][heads][N][N], masked [nwin][1][N][N] bool) of the reference's attention on embeddings e."""
    g = A.Geo(Bn, H // 4, W // 4, CE, NH, ws, shift, "cpu")
    msk = g.mask()
    out = []
    for p in range(4):
        q, k = g.split(e[:, p * CE:(p + 1) * CE], None), g.split(e[:, PAIR_KV[p] * CE:(PAIR_KV[p] + 1) * CE], None)
        out.append((torch.softmax(0.5 * (q @ k.transpose(-1, -2) - 100.0 * msk.double()), -1), msk))
    return g, out


def worst(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - ref| / bound; inf on a non-finite value."""
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref.double()).abs() / bound).max())


def share_over(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """Share of the elements with |got - ref| > bound (a non-finite value counts)."""
    err = (got.detach().double().reshape(ref.shape) - ref.double()).abs()
    return float((~(err <= bound)).double().mean())


# ------------------------------------------------------------------ a case, its reference and its bounds (computed once per process)
_setups: Dict = {}
_refs: Dict = {}


def setup(kind: str, case) -> Dict:
    """Inputs of a case.  kind: fused (B, H, W), general (B, H, W, ws, shift; embedding weights x 3), finite (the finite-mask
    case: hand-built embeddings, no images)."""
    key = (kind,) + tuple(case)
    if key not in _setups:
        B, H, W = case[:3]
        ws, shift = (1, 0) if kind == "fused" else case[3:5]
        seed = 1000 * B + 31 * H + 7 * W + 3 * ws + shift
        su = dict(kind=kind, case=tuple(case), B=B, H=H, W=W, ws=ws, shift=shift, M=B * (H // 4) * (W // 4), seed=seed, e_given=None)
        su.update(rand_inputs(B, H, W, seed, w_scale_general(ws) if kind == "general" else 1.0))
        if kind == "finite":
            su["e_given"] = finite_mask_e(B, H, W, ws, shift, seed)
            su["x4"] = (B, H, W)
        else:
            su["x4"] = x4_of(su["rgb"], su["ir3"][:, 0])
        _setups[key] = su
    return _setups[key]


def dout_and_reference(su: Dict, dt):
    key = (su["kind"],) + su["case"] + (dt,)
    if key not in _refs:
        dout = rand_dout(su["M"], dt, su["seed"] + 5)
        _refs[key] = (dout, reference(su["x4"], su["w"], su["b"], su["gamma"], su["beta"], su["ws"], su["shift"], dout, e_given=su["e_given"]))
    return _refs[key]


def bounds_for(su: Dict, dt, depth: Dict[str, int], de_exact: bool = False) -> Dict[str, torch.Tensor]:
    dout, ref = dout_and_reference(su, dt)
    return bounds(su["x4"], su["w"], su["b"], su["gamma"], su["beta"], su["ws"], su["shift"], dout, dt, ref, depth,
                  e_given=su["e_given"], de_exact=de_exact)


def tightest_depth(su: Dict, dt) -> Dict[str, int]:
    """The smallest depths any route of the case has (the host test holds the f32 statement to these)."""
    if su["kind"] == "fused":
        dd = min(fused_bwd_route(dt, su["M"], wsf)["depth"] for wsf in (None, WS_FLOATS))
        return dict(gamma=dd, de=3, embed=dd)
    return general_depths(su["M"], su["ws"] ** 2)
