"""Every window-attention route (csrc/attention.hip) against float64, element by element, with the kernel that ran pinned.

Each case states, through the profiler, the exact sequence of attention kernels its call launched (tests/attn_cases.py holds
the route table re-derived from launch_fwd / launch_bwd / launch_bwd_wm / launch_bwd_rc), and COVERED collects those names from
the same parametrize tables; test_engine_attention_routes_are_covered requires every attention kernel a training step launches
to be in it.  Inputs and outputs sit in quiet-NaN-filled buffers: every output element must be written, nothing around the
views may change, and a read outside the inputs shows up as NaN.  dbias_t is pre-filled and must come back as prefill +
gradient; the dq_acc scratch (ws > 8) starts with NaN in its delta half and must leave its first M * C floats exactly zero.

Bounds (u = 2^-24, the f32 unit roundoff; u_T = 2^-8 for bf16, 2^-24 for f32, the unit roundoff of a store to the run dtype;
u_P = u_T for bf16, where P and dS are rounded to bf16 to feed the MFMAs, else 0; N keys per window; hd the head dim).  The
reference is float64 on the kernel's actual inputs: S = hd^-1/2 q k^T + bias[index] - 100 [different region], lse, P, O, and
the analytic dP = dO V^T, delta = rowsum(dO o O), dS = P o (dP - delta), dV = P^T dO, dQ = hd^-1/2 dS K, dK = hd^-1/2 dS^T Q,
dbias = sum of dS over the entries sharing a table index.

  logit / p:  A_ij = hd^-1/2 |q_i||k_j| + |bias_ij| + 100 [masked].  The kernel's logit is an f32 dot product of hd exact
              products plus two adds (scale, bias / mask) and the log2 e scaling some kernels apply: |err| <= (hd + 8) u A_ij.
              exp / exp2 and the final m + log(l) add a few ulp relative to |lse|: E_ij = (hd + 8) u A_ij + 4 u (|lse_i| + 1)
              bounds the relative error of each p_ij; the normaliser l carries the P-weighted mean Ebar_i = sum_j P_ij E_ij.
  out:        |out - O| <= (P o (E + Ebar + u_P)) |V| + (N + 8) u P|V| + u_T |O|   (f32 accumulation over N keys, worst case).
  lse:        |lse_k - lse| <= Ebar + (N + 8) u + 4 u |lse|   (l summed over N keys; the m + log l add).
  backward:   rho_ij = E_ij + |lse_k,i - lse_i| + 4 u (|lse_i| + 1) bounds the recomputed p (it reads the kernel's lse);
              e_dP = (hd + 4) u |dO||V|^T; delta read from the stored output o_k (ws > 8): |dO.(o_k - O)| + (hd + 4) u |dO||o_k|,
              delta formed in-kernel from P: sum_j P_ij (rho_ij + (N + hd + 8) u) (|dO||V|^T)_ij;
              e_dS = P o (rho |dP - delta| + e_dP + e_delta) (1 + 2 rho) + u_P |dS|.
  dV:         (P o (rho + u_P))^T |dO| + (N + 8) u P^T|dO| + u_T |dV|.
  dQ, dK:     hd^-1/2 (e_dS |K| + (N + 8) u |dS||K|) + u_T |dQ|   and the same with e_dS^T, |Q|.
  dbias:      scatter(e_dS) + n_t u (scatter|dS| + |prefill|), n_t = nwin x (pairs per entry) + 2: f32 atomics in any order.
  recompute:  the fused-block backward forms q / k / v itself (bf16 of an f32 GEMM, one bf16 ulp from the reference's
              rounding): eta = 2^-7 relative on q / k / v adds 2 eta hd^-1/2 |q||k| to E and eta to the accumulation terms.

Measured on one MI355X (the module prints the worst err / bound per route and quantity under `pytest -s`): bf16 out, dqkv
and the multi-tile dbias reach 0.5 - 0.98, so u_P is the bound that binds.  The f32 routes sit at 0.01 - 0.1: their bound is
the worst-case accumulation term (hd + 8) u, (N + 8) u, while random data errs like sqrt(N) u.  The ws-8 dbias sits far
lower (1e-4 - 5e-2): the bound charges u_P and the n_t u atomics term to every dS, while those kernels sum the bias
gradient of a window in f32 before one flush.  The sparse-dout cases are what pin that dbias, window by window.

Structural cases have exact answers: selection codes make one key per query win by >= 40 nats (out must equal V[target]
bitwise in bf16), a one-hot relative-position table makes a query select the key at one offset, and a sparse dout must leave
every token outside its windows exactly zero and dbias equal to those windows' contribution."""
import json
import os

import pytest
import torch

import attn_cases as A
import gemm_cases as G

pytestmark = pytest.mark.gpu

BF, F32 = A.BF, A.F32

COVERED = set()
RATIOS = {}


def routed(table, route):
    for row in table:
        COVERED.update(route(*row))
    return table


def _fb(dt, hd, heads, B, H, W, ws, shift, *rest):
    return A.fwd_route(dt, hd, ws, shift) + A.bwd_route(dt, hd, ws, shift)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        for k in sorted(RATIOS):
            print(f"[attn bounds] {k}: worst err/bound {RATIOS[k]:.3g}")
        path = os.environ.get("ATTN_BOUND_REPORT")
        if path:
            with open(path, "w") as f:
                json.dump(RATIOS, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------ harness
def check(got, want, bound, what, key):
    got = got.double()
    err = (got - want).abs()
    ratio = float((err / bound).max()) if err.numel() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    G.assert_within(got, want, bound, what)


def _nan_free(view, what):
    bad = torch.isnan(view.float())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements not written (NaN sentinel left), first at {bad.nonzero()[0].tolist()}"


def _pads_intact(buf, pad, rows, what):
    s = A.sentinel_bits(buf)
    assert bool(s[:pad].all()) and bool(s[pad + rows:].all()), f"{what}: written outside its view"


def _route(fn, expect, what):
    got = A.attention_kernels(G.launched_kernels(fn))
    assert got == list(expect), f"{what}: launched {got}, the case was written for {list(expect)}"


def _inputs(g, dt, dev, seed, qk_scale=1.5):
    M, C, heads = g.M, g.C, g.heads
    qkv_buf, qkv = A.nan_buffer(M, 3 * C, dt, dev)
    qkv.copy_(torch.cat((A.randn((M, 2 * C), seed, dev, qk_scale), A.randn((M, C), seed + 1, dev)), 1).to(dt))
    bias_t = A.randn((heads, g.L2), seed + 2, dev, 0.7)
    do_buf, dout = A.nan_buffer(M, C, dt, dev)
    dout.copy_(A.randn((M, C), seed + 3, dev).to(dt))
    return qkv, bias_t, dout


def run_fwd(ops, g, dt, qkv, bias_t, f, tag):
    """Forward through the C ABI into NaN-filled views; route pinned; bounds against the reference dict f."""
    M, C, heads = g.M, g.C, g.heads
    out_buf, out = A.nan_buffer(M, C, dt, qkv.device)
    lse_buf, lse = A.nan_buffer(M, heads, torch.float32, qkv.device)
    route = A.fwd_route(dt, g.hd, g.ws, g.shift)
    _route(lambda: ops.window_attn_fwd(qkv, bias_t, out, lse, g.B, g.H, g.W, C, heads, g.ws, g.shift), route, tag)
    _nan_free(out, f"{tag} out"); _nan_free(lse, f"{tag} lse")
    _pads_intact(out_buf, 2, M, f"{tag} out"); _pads_intact(lse_buf, 2, M, f"{tag} lse")
    key = f"{route[0]} ws{g.ws}"
    check(out, g.merge(f["O"]), g.merge(f["out_bound"]), f"{tag} out", key + " out")
    check(lse, g.per_row(f["lse"]), g.per_row(f["lse_bound"]), f"{tag} lse", key + " lse")
    return out, lse


def run_bwd(ops, g, dt, qkv, bias_t, out, dout, lse, f, tag, seed, *, twice=False):
    M, C, heads = g.M, g.C, g.heads
    dev = qkv.device
    prefill = A.randn((heads, g.L2), seed + 7, dev, 0.5)
    r = A.reference_bwd(g, f, dt, dout, out if g.ws > 8 else None, lse, prefill)
    scratch = None
    if g.ws * g.ws > 64:
        scratch = torch.zeros(M * (C + heads), device=dev)
        scratch[M * C:] = float("nan")                    # the delta half needs no initialisation
    route = A.bwd_route(dt, g.hd, g.ws, g.shift)
    results = []
    for call in range(2 if twice else 1):
        dq_buf, dqkv = A.nan_buffer(M, 3 * C, dt, dev)
        dbt = prefill.clone()
        _route(lambda: ops.window_attn_bwd(qkv, bias_t, out, dout, lse, dqkv, dbt, scratch, g.B, g.H, g.W, C, heads, g.ws,
                                           g.shift), route, tag)
        _nan_free(dqkv, f"{tag} dqkv"); _pads_intact(dq_buf, 2, M, f"{tag} dqkv")
        if scratch is not None:
            nz = int((scratch[:M * C] != 0).sum())
            assert nz == 0, f"{tag}: dq_acc left {nz} non-zero floats (must be zero on exit)"
        key = f"{route[-2] if len(route) > 1 else route[0]} ws{g.ws}"
        check(dqkv, r["dqkv"], r["dqkv_bound"], f"{tag} dqkv (call {call})", key + " dqkv")
        check(dbt, prefill.double() + r["dbias"], r["dbias_bound"], f"{tag} dbias_t (call {call})", key + " dbias")
        results.append(dqkv)
    return results[-1], r


def _geo(dt, hd, heads, B, H, W, ws, shift, dev):
    return A.Geo(B, H, W, hd * heads, heads, ws, shift, dev)


# ------------------------------------------------------------------ §2 dense random cases, every route
# (dt, head dim, heads, B, H, W, ws, shift): window counts 1, 3, 7, 9, 21, 169, 171, 259, 513 cross the persistent grids
# (attn_fwd_fast_kernel walks above 512 windows; bwd_persistent_grid: 512 / (heads / NW) workgroup columns)
DENSE = routed([
    (BF, 16, 12, 1, 72, 152, 8, 3),      # 171 windows, fast2 grid 170
    (BF, 16, 4, 1, 152, 216, 8, 0),      # 513 windows: the fast forward walks (512), fast2 grid 512
    (BF, 32, 12, 1, 72, 152, 8, 4),      # stage 2: 171 windows, fast2<bf16, 32, 2> grid 85
    (BF, 64, 4, 1, 56, 8, 8, 7),         # stage 3 at S = 128: generic forward, attn_bwd_kernel, 7 windows
    (F32, 16, 4, 1, 56, 296, 8, 1),      # 259 windows, fast2<float, 16, 2> grid 256
    (F32, 16, 12, 1, 104, 104, 8, 0),    # 169 windows, grid 85
    (F32, 32, 24, 1, 24, 24, 8, 4),      # 24 heads
    (F32, 64, 4, 1, 8, 8, 8, 0),         # one window
    (BF, 16, 4, 1, 48, 48, 16, 8),       # bf16 hd 16 multi-tile: generic forward (nqt 4) + attn_bwd_mt_kernel, shifted 16x16
    (BF, 32, 12, 1, 16, 48, 16, 0),      # mt2 + dkv / dq
    (BF, 64, 4, 1, 48, 16, 16, 8),       # mt + mt
    (F32, 16, 4, 1, 16, 48, 16, 0),
    (F32, 32, 4, 1, 48, 16, 16, 15),
    (F32, 64, 4, 1, 16, 16, 16, 0),
    (BF, 64, 12, 1, 32, 32, 32, 0),      # stage 3
    (BF, 16, 4, 1, 32, 64, 32, 16),
    (F32, 32, 4, 1, 32, 32, 32, 0),
    (BF, 32, 4, 1, 64, 32, 32, 1),
    (F32, 16, 4, 1, 32, 32, 32, 5),
    (BF, 16, 4, 1, 64, 64, 64, 0),       # ws 64
    (F32, 64, 4, 1, 64, 64, 64, 32),
    (BF, 32, 4, 1, 64, 64, 64, 0),
], _fb)


@pytest.mark.parametrize("dt,hd,heads,B,H,W,ws,shift", DENSE)
def test_dense_route(ops, dev, dt, hd, heads, B, H, W, ws, shift):
    g = _geo(dt, hd, heads, B, H, W, ws, shift, dev)
    seed = hd * 7 + ws + shift
    qkv, bias_t, dout = _inputs(g, dt, dev, seed)
    f = A.reference(g, qkv, bias_t, dt)
    tag = f"{dt} hd{hd} h{heads} {H}x{W} ws{ws} shift{shift}"
    out, lse = run_fwd(ops, g, dt, qkv, bias_t, f, tag)
    run_bwd(ops, g, dt, qkv, bias_t, out, dout, lse, f, tag, seed, twice=(ws > 8 and heads == 12 or ws == 64 and dt == F32))


# ------------------------------------------------------------------ §3 selection: one key per query wins by >= 40 nats
SELECT = routed([
    (BF, 16, 4, 1, 24, 24, 8, 4),
    (F32, 32, 4, 1, 16, 24, 8, 0),
    (BF, 64, 4, 1, 16, 8, 8, 3),
    (BF, 32, 4, 1, 16, 32, 16, 0),
    (F32, 16, 4, 1, 32, 16, 16, 15),
    (F32, 64, 4, 1, 32, 32, 32, 16),
    (BF, 16, 4, 1, 32, 32, 32, 8),
    (BF, 64, 4, 1, 64, 64, 64, 0),
    (BF, 16, 4, 1, 64, 64, 64, 32),
], _fb)


def _exact_rows(got, want, dt, what):
    """bf16: bitwise.  f32: within 2^-16 relative and the same nearest integer (the answers are integers)."""
    if dt == BF:
        G.assert_bits(got.to(dt).contiguous(), want.to(dt).contiguous(), what)
        return
    g, w = got.double(), want.double()
    bad = ((g - w).abs() > 2.0 ** -16 * w.abs()) | (g.round() != w)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements do not select their target; first {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dt,hd,heads,B,H,W,ws,shift", SELECT)
def test_selection(ops, dev, dt, hd, heads, B, H, W, ws, shift):
    g = _geo(dt, hd, heads, B, H, W, ws, shift, dev)
    qkv_vals, dout_vals, tgt, boost = A.selection_inputs(g, dt, 11 + ws + shift, dev, cross=shift > 0)
    assert boost or not shift
    _, qkv = A.nan_buffer(g.M, 3 * g.C, dt, dev); qkv.copy_(qkv_vals)
    _, dout = A.nan_buffer(g.M, g.C, dt, dev); dout.copy_(dout_vals)
    bias_t = torch.zeros(heads, g.L2, device=dev)
    f = A.reference(g, qkv, bias_t, dt)
    tag = f"selection {dt} hd{hd} ws{ws} shift{shift}"
    out, lse = run_fwd(ops, g, dt, qkv, bias_t, f, tag)
    # out[query] = V[target]; lse = the target's logit (0, or 160 - 100 for the boosted cross-region queries)
    v = g.split(qkv, 2)
    sel = torch.gather(v, 2, tgt.unsqueeze(-1).expand(-1, -1, -1, hd))
    _exact_rows(out, g.merge(sel), dt, f"{tag}: out != V[target]")
    st = torch.gather(f["S"], 3, tgt.unsqueeze(-1)).squeeze(-1)
    lse_b = 16 * A.U * (1 + st.abs() + 100) + 1e-12
    G.assert_within(lse, g.per_row(st), g.per_row(lse_b), f"{tag}: lse != target logit")
    if boost:
        wb, hb, a, _ = boost[0]
        assert abs(float(st[wb, hb, a]) - 60.0) < 5, "the boosted cross-region target must win through the -100 mask"
    # backward: dV[target] = dO[query] (each key is exactly one query's target); dQ, dK, dbias stay within the tiny bound
    dqkv, r = run_bwd(ops, g, dt, qkv, bias_t, out, dout, lse, f, tag, 3)
    dO = g.split(dout, None)
    inv = torch.empty_like(tgt).scatter_(2, tgt, torch.arange(g.N, device=dev).expand_as(tgt).contiguous())
    dv_want = torch.gather(dO, 2, inv.unsqueeze(-1).expand(-1, -1, -1, hd))
    _exact_rows(dqkv[:, 2 * g.C:], g.merge(dv_want), dt, f"{tag}: dV[target] != dO[query]")
    # dQ / dK: the target's dS is exactly 0 (p = 1, dP and delta are exact integer sums), every other p <= e^-40, so
    # |dQ| <= 4 hd^-1/2 |dS||K| of the reference, below 1e-6 here.  A boosted cross-region query rounds its logit 60 through
    # log2 e, so its p is 1 - O(2^-24): its row and its target key are held to the dense bound above only.
    dS = r["dS"]
    tiny_q = 4 * f["scale"] * (dS.abs() @ f["k"].abs()) + 1e-30
    tiny_k = 4 * f["scale"] * (dS.abs().transpose(-1, -2) @ f["q"].abs()) + 1e-30
    keep_q = torch.ones(g.nwin, heads, g.N, dtype=torch.bool, device=dev)
    keep_k = keep_q.clone()
    for (w, h, a, b) in boost:
        keep_q[w, h, a] = keep_q[w, h, b] = False
        keep_k[w, h, tgt[w, h, a]] = keep_k[w, h, tgt[w, h, b]] = False
    assert float(tiny_q[keep_q].max()) < 1e-6 and float(tiny_k[keep_k].max()) < 1e-6
    G.assert_within(g.split(dqkv, 0)[keep_q], torch.zeros_like(tiny_q[keep_q]), tiny_q[keep_q], f"{tag}: dQ not ~0")
    G.assert_within(g.split(dqkv, 1)[keep_k], torch.zeros_like(tiny_k[keep_k]), tiny_k[keep_k], f"{tag}: dK not ~0")


# ------------------------------------------------------------------ §3 one-hot relative-position bias
ONEHOT = routed([(BF, 16, 4, 1, 16, 24, 8, 4), (F32, 32, 4, 1, 32, 16, 16, 0), (BF, 32, 4, 1, 32, 32, 32, 16),
                 (F32, 16, 8, 1, 16, 16, 8, 0)], _fb)


@pytest.mark.parametrize("dt,hd,heads,B,H,W,ws,shift", ONEHOT)
def test_onehot_bias(ops, dev, dt, hd, heads, B, H, W, ws, shift):
    g = _geo(dt, hd, heads, B, H, W, ws, shift, dev)
    qkv_vals, bias_t, offs = A.onehot_bias_inputs(g, dt, dev)
    _, qkv = A.nan_buffer(g.M, 3 * g.C, dt, dev); qkv.copy_(qkv_vals)
    _, dout = A.nan_buffer(g.M, g.C, dt, dev); dout.copy_(A.randn((g.M, g.C), 5, dev).to(dt))
    f = A.reference(g, qkv, bias_t, dt)
    tag = f"one-hot bias {dt} hd{hd} ws{ws} shift{shift}"
    out, lse = run_fwd(ops, g, dt, qkv, bias_t, f, tag)
    n = torch.arange(g.N, device=dev)
    iy, ix = n // ws, n % ws
    v = g.split(qkv, 2)
    got = g.split(out, None)
    checked = 0
    for h, (dy, dx) in enumerate(offs):
        ky, kx = iy - dy, ix - dx
        ok = (ky >= 0) & (ky < ws) & (kx >= 0) & (kx < ws)
        key = (ky.clamp(0, ws - 1) * ws + kx.clamp(0, ws - 1))
        same = g.region.gather(1, key.expand(g.nwin, -1)) == g.region
        sel = ok.unsqueeze(0) & same                                           # [nwin][N]
        want = v[:, h].gather(1, key.view(1, -1, 1).expand(g.nwin, -1, hd))
        _exact_rows(got[:, h][sel], want[sel], dt, f"{tag} head {h}: query does not select the key at offset {(dy, dx)}")
        checked += int(sel.sum())
    assert checked > 0
    run_bwd(ops, g, dt, qkv, bias_t, out, dout, lse, f, tag, 9)


# ------------------------------------------------------------------ §3 sparse dout: only chosen windows carry a gradient
def _walk_windows(dt, hd, heads, nwin, ws):
    gx = A.bwd_persistent_grid(nwin, heads // A.NW_BWD[(dt, hd)], A.NW_BWD[(dt, hd)]) if ws == 8 else min(nwin * ws * ws // 64, 1024) // (ws * ws // 64)
    return sorted({w for w in (0, gx - 1, gx, 2 * gx, nwin - 1) if 0 <= w < nwin})


SPARSE = routed([(BF, 16, 12, 1, 152, 152, 8, 0), (BF, 32, 12, 1, 72, 152, 8, 2), (F32, 16, 12, 1, 72, 152, 8, 0),
                 (BF, 16, 4, 1, 272, 256, 16, 0)], _fb)


def _sparse_dout(g, dt, dev, wins, seed):
    dout_full = A.randn((g.M, g.C), seed, dev).to(dt)
    keep = torch.zeros(g.M, dtype=torch.bool, device=dev)
    keep[g.rows[wins].flatten()] = True
    _, dout = A.nan_buffer(g.M, g.C, dt, dev)
    dout.copy_(torch.where(keep.unsqueeze(1), dout_full, torch.zeros_like(dout_full)))
    return dout, keep


def _zero_outside(dqkv, keep, what):
    nz = int((dqkv[~keep] != 0).sum())
    assert nz == 0, f"{what}: {nz} gradient elements non-zero on tokens whose windows carry no dout"


@pytest.mark.parametrize("dt,hd,heads,B,H,W,ws,shift", SPARSE)
def test_sparse_dout(ops, dev, dt, hd, heads, B, H, W, ws, shift):
    g = _geo(dt, hd, heads, B, H, W, ws, shift, dev)
    wins = _walk_windows(dt, hd, heads, g.nwin, ws)
    qkv, bias_t, _ = _inputs(g, dt, dev, 21)
    dout, keep = _sparse_dout(g, dt, dev, wins, 22)
    f = A.reference(g, qkv, bias_t, dt)
    tag = f"sparse dout {dt} hd{hd} windows {wins} of {g.nwin}"
    out, lse = run_fwd(ops, g, dt, qkv, bias_t, f, tag)
    dqkv, _ = run_bwd(ops, g, dt, qkv, bias_t, out, dout, lse, f, tag, 23)
    _zero_outside(dqkv, keep, tag)


# ------------------------------------------------------------------ the window-major backward (sodt_window_attn_bwd_wm)
WM = routed([(BF, 12, 1, 72, 152, 3, False), (F32, 12, 1, 72, 152, 0, False), (BF, 4, 1, 24, 24, 4, False),
             (BF, 12, 1, 152, 152, 2, True)], lambda dt, *r: A.bwd_wm_route(dt))


@pytest.mark.parametrize("dt,heads,B,H,W,shift,sparse", WM)
def test_bwd_window_major(ops, dev, dt, heads, B, H, W, shift, sparse):
    from oracle import ref_torch as R
    g = _geo(dt, 16, heads, B, H, W, 8, shift, dev)
    qkv, bias_t, dout = _inputs(g, dt, dev, 31)
    keep = None
    if sparse:
        nw = A.NW_BWD[(dt, 16)] if dt == F32 else 4
        gx = A.bwd_persistent_grid(g.nwin, heads // nw, nw)
        dout, keep = _sparse_dout(g, dt, dev, sorted({0, gx - 1, gx, 2 * gx, g.nwin - 1}), 32)
    f = A.reference(g, qkv, bias_t, dt)
    tag = f"bwd_wm {dt} h{heads} {H}x{W} shift{shift}"
    out, lse = run_fwd(ops, g, dt, qkv, bias_t, f, tag)
    qkvw = qkv[g.rows].view(g.nwin, 64, 3, heads, 16).permute(0, 3, 2, 1, 4).contiguous()
    lsew = lse[g.rows].permute(0, 2, 1).contiguous()
    prefill = A.randn((heads, g.L2), 33, dev, 0.5)
    r = A.reference_bwd(g, f, dt, dout, None, lse, prefill)
    dq_buf, dqkv = A.nan_buffer(g.M, 3 * g.C, dt, dev)
    dbt = prefill.clone()
    _route(lambda: ops.window_attn_bwd_wm(qkvw, bias_t, dout, lsew, dqkv, dbt, B, H, W, g.C, heads, 8, shift),
           A.bwd_wm_route(dt), tag)
    _nan_free(dqkv, tag); _pads_intact(dq_buf, 2, g.M, tag)
    key = A.bwd_wm_route(dt)[0]
    check(dqkv, r["dqkv"], r["dqkv_bound"], f"{tag} dqkv", key + " dqkv")
    check(dbt, prefill.double() + r["dbias"], r["dbias_bound"], f"{tag} dbias_t", key + " dbias")
    if keep is not None:
        _zero_outside(dqkv, keep, tag)


# ------------------------------------------------------------------ the fused block's recomputing backward (sodt_wmsa_block_bwd)
RC = routed([(1, 56, 8, 0, False), (1, 72, 152, 2, False), (1, 152, 152, 0, True)], lambda *r: A.RC_ROUTE)


@pytest.mark.parametrize("B,H,W,shift,sparse", RC)
def test_bwd_recompute(ops, dev, B, H, W, shift, sparse):
    import importlib
    from test_wmsa_block_gpu import _pack, _params
    L = importlib.import_module("small-object-detection-transformers_amd._lib")
    C, heads, hd, dt = 192, 12, 16, BF
    g = A.Geo(B, H, W, C, heads, 8, shift, dev)
    sd = _params(dev, seed=5 + shift)
    x = (A.randn((g.M, C), 41, dev) * 1.3 + 0.2).to(dt)
    wpk = _pack(ops, L, sd, dev, dt)
    xm, xn2, xn1, ao = (torch.zeros(g.M, C, device=dev, dtype=dt) for _ in range(4))
    st1, st2 = torch.zeros(g.M, 2, device=dev), torch.zeros(g.M, 2, device=dev)
    lsew = torch.zeros(g.nwin, heads, 64, device=dev)
    ops.wmsa_block_fwd(x, wpk, xm, xn2, st1, st2, xn1, None, lsew, ao, B, H, W, C, heads, 8, shift)
    # the operands the kernel forms: q_s = bf16(xn1 bf16(Wq hd^-1/2 log2 e)^T + bq hd^-1/2 log2 e), k, v = bf16(xn1 W^T + b)
    s2 = hd ** -0.5 * 1.4426950408889634
    Wb, bb = sd["attn.qkv.weight"], sd["attn.qkv.bias"]
    xd = xn1.double()
    qs = (xd @ (Wb[:C] * s2).to(dt).double().t() + bb[:C].double() * s2).float().to(dt).double()
    kk = (xd @ Wb[C:2 * C].to(dt).double().t() + bb[C:2 * C].double()).float().to(dt).double()
    vv = (xd @ Wb[2 * C:].to(dt).double().t() + bb[2 * C:].double()).float().to(dt).double()
    qkv64 = torch.cat((qs / s2, kk, vv), 1)
    bias_t = sd["attn.relative_position_bias_table"].t().contiguous()
    f = A.reference(g, qkv64, bias_t, dt, eta=2.0 ** -7)
    lse_nat = g.per_row(lsew.view(g.nwin, heads, 64))
    check(lse_nat, g.per_row(f["lse"]), g.per_row(f["lse_bound"] + 2.0 ** -7 * f["lse"].abs() + 2 * 2.0 ** -7 * 10), "rc lse",
          "wmsa_block_fwd lsew")
    if sparse:
        gx = A.rc_grid(g.nwin)
        dout, keep = _sparse_dout(g, dt, dev, sorted({0, gx - 1, gx, 2 * gx, g.nwin - 1}), 42)
    else:
        _, dout = A.nan_buffer(g.M, C, dt, dev); dout.copy_(A.randn((g.M, C), 43, dev).to(dt))
        keep = None
    prefill = A.randn((heads, g.L2), 44, dev, 0.5)
    r = A.reference_bwd(g, f, dt, dout, None, lse_nat, prefill)
    dq_buf, dqkv = A.nan_buffer(g.M, 3 * C, dt, dev)
    dbt = prefill.clone()
    tag = f"wmsa_block_bwd {H}x{W} shift{shift}"
    _route(lambda: ops.wmsa_block_bwd(xn1, wpk, bias_t, dout, lsew, dqkv, dbt, B, H, W, C, heads, 8, shift), A.RC_ROUTE, tag)
    _nan_free(dqkv, tag); _pads_intact(dq_buf, 2, g.M, tag)
    check(dqkv, r["dqkv"], r["dqkv_bound"], f"{tag} dqkv", A.RC_ROUTE[0] + " dqkv")
    check(dbt, prefill.double() + r["dbias"], r["dbias_bound"], f"{tag} dbias_t", A.RC_ROUTE[0] + " dbias")
    if keep is not None:
        _zero_outside(dqkv, keep, tag)


# ------------------------------------------------------------------ §4 refusals: SODT_EINVAL through ops._launch, nothing written
# (dtype, head dim, heads, H, W, ws, shift, why)
REFUSED = [
    (BF, 16, 4, 16, 16, 4, 0, "ws 4"),
    (BF, 16, 4, 48, 48, 24, 0, "ws 24"),
    (F32, 32, 4, 24, 16, 16, 0, "ws does not divide H"),
    (BF, 32, 4, 16, 24, 16, 0, "ws does not divide W"),
    (BF, 16, 4, 16, 16, 8, 8, "shift == ws"),
    (F32, 16, 4, 32, 32, 16, 17, "shift > ws"),
    (BF, 48, 4, 16, 16, 8, 0, "head dim 48"),
    (BF, 16, 6, 16, 16, 8, 0, "heads % NW (bf16, 6 heads, head dim 16)"),
    (BF, 32, 3, 16, 16, 8, 0, "heads % NW (bf16, 3 heads, head dim 32)"),
]


@pytest.mark.parametrize("dt,hd,heads,H,W,ws,shift,why", REFUSED, ids=[r[-1] for r in REFUSED])
def test_refused_geometry(ops, dev, dt, hd, heads, H, W, ws, shift, why):
    B, C = 1, hd * heads
    M = B * H * W
    L2 = (2 * max(ws, 1) - 1) ** 2
    qkv = A.randn((M, 3 * C), 1, dev).to(dt)
    bias_t = torch.zeros(heads, L2, device=dev)
    out_buf, out = A.nan_buffer(M, C, dt, dev)
    lse_buf, lse = A.nan_buffer(M, heads, torch.float32, dev)
    with pytest.raises(RuntimeError, match="sodt_window_attn_fwd failed"):
        ops.window_attn_fwd(qkv, bias_t, out, lse, B, H, W, C, heads, ws, shift)
    dq_buf, dqkv = A.nan_buffer(M, 3 * C, dt, dev)
    dbt = torch.full((heads, L2), 3.0, device=dev)
    scratch = torch.zeros(M * (C + heads), device=dev)
    dout = torch.zeros(M, C, device=dev, dtype=dt)
    ref_out = torch.zeros(M, C, device=dev, dtype=dt)
    with pytest.raises(RuntimeError, match="sodt_window_attn_bwd failed"):
        ops.window_attn_bwd(qkv, bias_t, ref_out, dout, lse, dqkv, dbt, scratch, B, H, W, C, heads, ws, shift)
    torch.cuda.synchronize()
    for buf, what in ((out_buf, "out"), (lse_buf, "lse"), (dq_buf, "dqkv")):
        assert bool(A.sentinel_bits(buf).all()), f"{why}: a refused call wrote {what}"
    assert bool((dbt == 3.0).all()) and bool((scratch == 0).all()), f"{why}: a refused call wrote dbias_t / dq_acc"


def test_refused_null_scratch_and_dtype(ops, dev):
    import importlib
    L = importlib.import_module("small-object-detection-transformers_amd._lib")
    B, H, W, heads, hd, ws = 1, 16, 16, 4, 32, 16
    C, M = heads * hd, B * H * W
    qkv = A.randn((M, 3 * C), 1, dev).to(BF)
    bias_t = torch.zeros(heads, (2 * ws - 1) ** 2, device=dev)
    out = torch.zeros(M, C, device=dev, dtype=BF)
    lse = torch.zeros(M, heads, device=dev)
    ops.window_attn_fwd(qkv, bias_t, out, lse, B, H, W, C, heads, ws, 0)
    dq_buf, dqkv = A.nan_buffer(M, 3 * C, BF, dev)
    dbt = torch.full_like(bias_t, 3.0)
    with pytest.raises(RuntimeError, match="sodt_window_attn_bwd failed"):          # ws > 8 needs dq_acc
        ops.window_attn_bwd(qkv, bias_t, out, out, lse, dqkv, dbt, None, B, H, W, C, heads, ws, 0)
    p = lambda t: t.data_ptr()
    out_buf, out2 = A.nan_buffer(M, C, BF, dev)
    bad = 7
    assert bad not in (L.BF16, L.F32)
    with pytest.raises(RuntimeError, match="sodt_window_attn_fwd failed"):
        ops._launch("sodt_window_attn_fwd", p(qkv), p(bias_t), p(out2), p(lse), B, H, W, C, heads, 8, 0, bad)
    with pytest.raises(RuntimeError, match="sodt_window_attn_bwd failed"):
        ops._launch("sodt_window_attn_bwd", p(qkv), p(bias_t), p(out), p(out), p(lse), p(dqkv), p(dbt), None, B, H, W, C, heads,
                    8, 0, bad)
    torch.cuda.synchronize()
    assert bool(A.sentinel_bits(dq_buf).all()) and bool(A.sentinel_bits(out_buf).all()) and bool((dbt == 3.0).all())


# ------------------------------------------------------------------ the engine's attention routes are all covered above
@pytest.mark.parametrize("img,dt", [(512, BF), (256, F32), (128, BF)], ids=["512-bf16", "256-f32", "128-bf16"])
def test_engine_attention_routes_are_covered(ops, dev, img, dt):
    from oracle import ref_torch as R
    from test_model_gpu import build
    model, _ = build(dev, img)
    model.compute_dtype = dt
    model.train()
    x_rgb, x_ir = R.synthetic_inputs(1, img, seed=2)

    def step():
        out = model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
        loss = 0
        stack = [out]
        while stack:
            o = stack.pop()
            if isinstance(o, (list, tuple)):
                stack.extend(o)
            elif torch.is_tensor(o) and o.requires_grad:
                loss = loss + o.float().square().mean()
        loss.backward()
    step()                                   # plans are recorded on the first call; the profiled step replays them
    used = set(A.attention_kernels(G.launched_kernels(step)))
    assert used, "no attention kernel seen in a training step: the profiler did not see the library"
    missing = sorted(used - COVERED)
    assert not missing, f"attention kernels the step launches that no case covers: {missing}"
