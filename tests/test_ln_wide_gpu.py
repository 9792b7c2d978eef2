"""Wide-row LayerNorm (C = 384 and 768: ln_fwd_kernel / ln_bwd_kernel of csrc/norm.hip, one wave per row) on its own through the C
ABI.  At C = 768 ln_bwd_kernel keeps two rows of a wave in flight and runs on a small grid, so the row counts are chosen around that
walk: M = 1 (one wave of one workgroup has a row, and only the first of its rows), 5 (a ragged last trip: an odd row count, the last wave
holds one row of its pair), 263 (several workgroups, odd), 4101 (more rows than one trip of the whole grid: the grid stride in use).

Every operand lies between two rows of NaN (tests/test_sr_movement_gpu.py::_guarded), so a read outside a view poisons the result;
y, dx and the statistics lie inside buffers of sentinels that are compared afterwards.

The reference is float64 autograd of F.layer_norm on the very tensors the kernel reads.  The gates are those of
tests/block_cases.py (imported, not restated): relative L2 error at most F32_GATE on f32, MARGIN * e_emul + FLOOR on bf16, where
e_emul is the relative L2 distance between that reference and the same float64 graph with a straight-through bf16 rounding
(block_cases.narrow) wherever the kernel stores bf16: y on the way forward, dx on the way back.  mean / rstd and dgamma / dbeta are
stored in f32, no rounding point reaches them, so their e_emul is 0 and their gate is the floor, as for block_cases.UNTOUCHED.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import block_cases as BC
from test_sr_movement_gpu import _guarded

pytestmark = pytest.mark.gpu

SENT = 7.0
CASES = [pytest.param(BC.BF, M, Cc, id=f"bf16-{M}x{Cc}") for M in (1, 5, 263, 4101) for Cc in (384, 768)] + \
        [pytest.param(BC.F32, 263, Cc, id=f"f32-263x{Cc}") for Cc in (384, 768)]


def _cpu(shape, dt, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dt)


def _graph(x, dy, dres, gamma, beta, store):
    """float64 LayerNorm forward and backward; store() is applied wherever the kernel writes the run dtype"""
    xr = x.double().requires_grad_(True)
    g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = store(F.layer_norm(xr, (x.shape[-1],), g, b, 1e-5))
    y.backward(dy.double())
    dx = xr.grad if dres is None else xr.grad + dres.double()
    return dict(y=y.detach(), dx=store(dx).detach(), dgamma=g.grad, dbeta=b.grad)


@functools.lru_cache(maxsize=None)
def _case(dt, M, Cc, dev):
    """guarded inputs on the device, the float64 reference with and without the residual operand, and e_emul; never modified"""
    x = _guarded(_cpu((M, Cc), dt, 1, 1.3, 0.2), dev)
    dy = _guarded(_cpu((M, Cc), dt, 2), dev)
    dres = _guarded(_cpu((M, Cc), dt, 3), dev)
    gamma = _cpu((Cc,), torch.float32, 4, 0.2, 1.0).to(dev)
    beta = _cpu((Cc,), torch.float32, 5, 0.2).to(dev)
    xd = x.double()
    mean = xd.mean(-1)
    stats = torch.stack([mean, 1 / torch.sqrt(xd.var(-1, unbiased=False) + 1e-5)], -1)
    c = dict(x=x, dy=dy, dres=dres, gamma=gamma, beta=beta, stats=stats, ref={}, gate={})
    for res in (False, True):
        A = _graph(x, dy, dres if res else None, gamma, beta, lambda t: t)
        c["ref"][res] = A
        if dt == BC.BF:
            Bt = _graph(x, dy, dres if res else None, gamma, beta, BC.narrow)
            c["gate"][res] = {k: BC.MARGIN * BC.rel_l2(Bt[k], A[k].cpu()) + BC.FLOOR for k in A}
        else:
            c["gate"][res] = {k: BC.F32_GATE for k in A}
    c["gate"]["stats"] = BC.FLOOR if dt == BC.BF else BC.F32_GATE
    return c


def _check(what, got, ref, gate):
    err = BC.rel_l2(got, ref.cpu())
    print(f"{what}: rel l2 err {err:.3e}, gate {gate:.3e}")
    assert err <= gate, f"{what}: {err:.3e} above the gate {gate:.3e}"       # (NaN fails too)


def _in_sentinels(M, Cc, dt, dev, rows=2):
    buf = torch.full((M + 2 * rows, Cc), SENT, device=dev, dtype=dt)
    return buf, buf[rows: rows + M]


def _kept(buf, M, rows=2):
    return bool((buf[:rows] == SENT).all()) and bool((buf[rows + M:] == SENT).all())


@pytest.mark.parametrize("dt,M,Cc", CASES)
def test_layernorm_fwd_wide(ops, dev, dt, M, Cc):
    c = _case(dt, M, Cc, dev)
    ybuf, y = _in_sentinels(M, Cc, dt, dev)
    sbuf, stats = _in_sentinels(M, 2, torch.float32, dev)
    ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], y, stats, M, Cc)
    _check("y", y, c["ref"][False]["y"], c["gate"][False]["y"])
    _check("mean, rstd", stats, c["stats"], c["gate"]["stats"])
    assert _kept(ybuf, M) and _kept(sbuf, M), "layernorm_fwd wrote outside y / stats"


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("dt,M,Cc", CASES)
def test_layernorm_bwd_wide(ops, dev, dt, M, Cc, res):
    c = _case(dt, M, Cc, dev)
    ref, gate = c["ref"][res], c["gate"][res]
    stats = _guarded(c["stats"].float().cpu(), dev)
    dbuf, dx = _in_sentinels(M, Cc, dt, dev)
    pbuf = torch.full((4, Cc), SENT, device=dev)
    dg, db = pbuf[1], pbuf[2]
    dg.zero_(); db.zero_()
    for n in (1, 2):                              # dgamma / dbeta accumulate: the second call doubles them
        ops.layernorm_bwd(c["dy"], c["x"], stats, c["gamma"], c["dres"] if res else None, dx, dg, db, M, Cc)
        _check(f"dx (call {n})", dx, ref["dx"], gate["dx"])
        _check(f"dgamma (call {n})", dg, n * ref["dgamma"], gate["dgamma"])
        _check(f"dbeta (call {n})", db, n * ref["dbeta"], gate["dbeta"])
    assert _kept(dbuf, M), "layernorm_bwd wrote outside dx"
    assert bool((pbuf[0] == SENT).all()) and bool((pbuf[3] == SENT).all()), "layernorm_bwd wrote outside dgamma / dbeta"
