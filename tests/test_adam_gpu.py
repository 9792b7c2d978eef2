"""optim.FusedAdam (+ optim.ModelEMA; one fused kernel over the flat buffers, csrc/optim.hip, sodt_adam_ema_step) against
torch.optim.Adam as Train.py:148 builds it under --adam (betas=(hyp['momentum'], 0.999)) and against torch.optim.AdamW
(decoupled=True), both over the reference's two weight-decay groups (basics/optimizer.py:35-49) and followed by the
reference's ModelEMA update loop; four steps, so bias correction runs at t = 1..4, with per-group learning rates that
change every step as the warm-up of Train.py:384-392 does.  Then the optimizer's own behaviour (skipped step, resume,
one launch per step, refusals) and a short training loop with focal loss.

Tolerance of the comparison with torch: 2e-6 * (max|ref| + 1e-5) per tensor, the figure tests/test_optim_gpu.py uses for
"same arithmetic, different fma grouping".  Next to it the test steps a float64 restatement of the update on float64
copies of the same parameters and gradients and prints how far torch's float32 optimizer and the fused kernel each are
from it (DESIGN.md section 7 records the figures)."""
import ctypes as C
import importlib

import pytest
import torch

from test_model_gpu import build
from test_optim_gpu import _RefEMA, _build

pytestmark = pytest.mark.gpu
PKG = "small-object-detection-transformers_amd"
BETAS = (0.937, 0.999)          # Train.py:148 with hyp['momentum'] of models/hyp.scratch.yaml
EPS = 1e-8


def _group_of(name, p):         # basics/optimizer.py:41-47
    return 1 if p.dim() == 1 or name.endswith(".bias") else 0


class _Adam64:
    """The update of include/sodt_hip.h (sodt_adam_ema_step) restated in float64, one tensor at a time, with the EMA."""

    def __init__(self, model, ema_model):
        self.p = {k: p.detach().double().clone() for k, p in model.named_parameters()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.e = {k: p.detach().double().clone() for k, p in ema_model.named_parameters()}
        self.group = {k: _group_of(k, p) for k, p in model.named_parameters()}
        self.t = 0

    def step(self, grads, lr, wd, decoupled, ema_decay):
        self.t += 1
        b1, b2 = BETAS
        bc1, sqrt_bc2 = 1 - b1 ** self.t, (1 - b2 ** self.t) ** 0.5
        for k, p in self.p.items():
            g, l, w = grads[k].double(), lr[self.group[k]], wd[self.group[k]]
            if decoupled:
                d, p0 = g, p * (1 - l * w)
            else:
                d, p0 = g + w * p, p
            self.m[k] = b1 * self.m[k] + (1 - b1) * d
            self.v[k] = b2 * self.v[k] + (1 - b2) * d * d
            self.p[k] = p0 - (l / bc1) * self.m[k] / (self.v[k].sqrt() / sqrt_bc2 + EPS)
            self.e[k] = self.e[k] * ema_decay + (1 - ema_decay) * self.p[k]


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_fused_adam_ema_matches_torch(dev, dt, decoupled):
    O = importlib.import_module(PKG + ".optim")
    ma, mb = _build(dev), _build(dev)
    ma.compute_dtype = mb.compute_dtype = dt
    ema_a = O.ModelEMA(ma)
    ema_b = _RefEMA(mb)
    wd = (0.00048, 0.0)
    opt_a = O.FusedAdam(O.set_weight_decay(ma, weight_decay=wd[0]), model=ma, lr=1e-3, betas=BETAS, decoupled=decoupled, ema=ema_a)
    opt_b = (torch.optim.AdamW if decoupled else torch.optim.Adam)(O.set_weight_decay(mb, weight_decay=wd[0]), lr=1e-3, betas=BETAS)
    assert [g["weight_decay"] for g in opt_a.param_groups] == list(wd) == [g["weight_decay"] for g in opt_b.param_groups]
    ref64 = _Adam64(ma, ema_a.ema)
    g = torch.Generator().manual_seed(5)
    x, ir = torch.rand(2, 3, 128, 128, generator=g).to(dev), torch.rand(2, 3, 128, 128, generator=g).to(dev)
    worst = dict(fused_torch=0.0, torch_f64=0.0, fused_f64=0.0)
    for step in range(4):
        lr = (0.0005 * (step + 1), 0.004 - 0.0009 * step)          # warm-up style per-group schedules (Train.py:384-392)
        for opt in (opt_a, opt_b):
            opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lr
        # one forward / backward (model A); model B steps on a COPY of A's gradients and running statistics, so that the
        # comparison is the optimizer + EMA arithmetic and not the run-to-run summation order of the gradient kernels
        pred, _ = ma(x, ir, "RGB+IR")
        pred[0].float().square().mean().backward()
        pa = dict(ma.named_parameters())
        grads = {k: p.grad.detach().clone() for k, p in pa.items()}
        for k, p in mb.named_parameters():
            p.grad = grads[k].clone()
        ba = dict(ma.named_buffers())
        with torch.no_grad():
            for k, bfr in mb.named_buffers():
                bfr.copy_(ba[k])
        ref64.step(grads, lr, wd, decoupled, ema_a.next_decay())
        for m, opt, ema in ((ma, opt_a, ema_a), (mb, opt_b, ema_b)):
            opt.step()
            opt.zero_grad(set_to_none=True)
            ema.update(m)
        torch.cuda.synchronize()
        assert opt_a.state_dict()["step"] == step + 1
        tol = 2e-6
        sa, sb = ma.state_dict(), mb.state_dict()
        ea, eb = ema_a.ema.state_dict(), ema_b.ema.state_dict()
        bad = []
        for k in sa:
            if not sa[k].dtype.is_floating_point:
                continue
            for what, a, b, r64 in (("parameter", sa[k], sb[k], ref64.p.get(k)), ("EMA of", ea[k], eb[k], ref64.e.get(k))):
                s = float(b.abs().max()) + 1e-5
                err = float((a - b).abs().max())
                worst["fused_torch"] = max(worst["fused_torch"], err / s)
                if r64 is not None:
                    worst["torch_f64"] = max(worst["torch_f64"], float((b.double() - r64).abs().max()) / s)
                    worst["fused_f64"] = max(worst["fused_f64"], float((a.double() - r64).abs().max()) / s)
                if err > tol * s:
                    bad.append(f"step {step}: {what} {k}: {err:.3e} > {tol * s:.3e}")
        print(f"adam decoupled={decoupled} {dt} step {step}: worst so far, relative to max|ref| + 1e-5: "
              + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
        assert not bad, bad[:8]
        if dt == torch.bfloat16:      # the bf16 mirror written by the fused step is what a re-cast of the masters gives
            eng = ma._get_engine()
            assert eng.param_cast_fresh and torch.equal(eng.flat_cast[dt], eng.flat_param.to(dt))
    assert ema_a.updates == 4


def _one_backward(m, x, ir):
    m(x, ir, "RGB+IR")[0][0].float().square().mean().backward()


def test_fused_adam_skips_without_gradients(dev):
    O = importlib.import_module(PKG + ".optim")
    m = _build(dev)
    opt = O.FusedAdam(m.parameters(), model=m, lr=0.1)
    eng = m._get_engine()
    before = eng.flat_param.clone()
    opt.step()                                          # no backward yet: torch.optim.Adam would skip every parameter
    assert torch.equal(before, eng.flat_param) and opt.state_dict()["step"] == 0
    g = torch.Generator().manual_seed(2)
    x, ir = torch.rand(1, 3, 128, 128, generator=g).to(dev), torch.rand(1, 3, 128, 128, generator=g).to(dev)
    _one_backward(m, x, ir)
    opt.step()
    assert not torch.equal(before, eng.flat_param) and opt.state_dict()["step"] == 1
    opt.zero_grad(set_to_none=True)
    after = eng.flat_param.clone()
    opt.step()                                          # gradients were dropped and no backward ran: nothing moves
    assert torch.equal(after, eng.flat_param) and opt.state_dict()["step"] == 1


def test_fused_adam_resumes_from_state_dict_bit_for_bit(dev):
    """Train.py:173-174: optimizer.load_state_dict(ckpt['optimizer']).  Two steps on model 1; model 2 takes model 1's weights
    and a new optimizer takes its state_dict; a third step on the same gradients gives the same parameters."""
    O = importlib.import_module(PKG + ".optim")
    g = torch.Generator().manual_seed(9)
    x, ir = torch.rand(1, 3, 128, 128, generator=g).to(dev), torch.rand(1, 3, 128, 128, generator=g).to(dev)
    m1, m2 = _build(dev), _build(dev)
    kw = dict(lr=2e-3, betas=BETAS, weight_decay=0.00048)
    opt1 = O.FusedAdam(O.set_weight_decay(m1), model=m1, **kw)
    for _ in range(2):
        _one_backward(m1, x, ir)
        opt1.step()
        opt1.zero_grad(set_to_none=True)
    sd = opt1.state_dict()
    assert sd["step"] == 2 and sd["exp_avg_flat"].abs().max() > 0 and sd["exp_avg_sq_flat"].abs().max() > 0
    m2.load_state_dict(m1.state_dict())
    opt2 = O.FusedAdam(O.set_weight_decay(m2), model=m2, lr=1.0, betas=(0.5, 0.5))      # every hyper-parameter comes from sd
    opt2.load_state_dict(sd)
    assert "exp_avg_flat" in sd and opt2.param_groups[0]["lr"] == 2e-3 and tuple(opt2.param_groups[0]["betas"]) == BETAS
    _one_backward(m1, x, ir)
    _one_backward(m2, x, ir)                            # (claims m2's gradient views; the values are replaced by m1's)
    e1, e2 = m1._get_engine(), m2._get_engine()
    e2.flat_grad.copy_(e1.flat_grad)
    opt1.step()
    opt2.step()
    torch.cuda.synchronize()
    assert opt2.state_dict()["step"] == 3
    assert torch.equal(e1.flat_param, e2.flat_param)
    assert torch.equal(opt1.state_dict()["exp_avg_sq_flat"], opt2.state_dict()["exp_avg_sq_flat"])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_fused_adam_is_one_launch_per_step(dev, dt):
    O = importlib.import_module(PKG + ".optim")
    ops = importlib.import_module(PKG + ".ops")
    m = _build(dev)
    m.compute_dtype = dt
    ema = O.ModelEMA(m)
    opt = O.FusedAdam(O.set_weight_decay(m), model=m, ema=ema)
    g = torch.Generator().manual_seed(4)
    x, ir = torch.rand(1, 3, 128, 128, generator=g).to(dev), torch.rand(1, 3, 128, 128, generator=g).to(dev)
    for _ in range(2):
        _one_backward(m, x, ir)
        with ops.Recorder() as rec:
            opt.step()
        assert [name for _, _, name, _ in rec.calls] == ["sodt_adam_ema_step"]
        assert ema._fused_pending                       # the parameter average rode in that launch
        opt.zero_grad(set_to_none=True)
        ema.update(m)
        assert not ema._fused_pending
    assert m._get_engine().param_cast_fresh == (dt == torch.bfloat16)


def test_fused_adam_refusals(dev):
    O = importlib.import_module(PKG + ".optim")
    L = importlib.import_module(PKG + "._lib")
    m = _build(dev)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        O.FusedAdam(m.parameters(), model=m, amsgrad=True)
    # the C entry: invalid ARGUMENTS only, each refused before anything is launched
    lib = L.load()
    n = 1024
    p, gr, ea, es = (torch.zeros(n + 4, device=dev) for _ in range(4))
    d5 = lambda v: (C.c_double * 5)(*([v] * 5))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pp=p.data_ptr(), ng=2, eps=1e-8, b1=0.9, b2=0.999, step=1, nel=n):
        return lib.sodt_adam_ema_step(pp, gr.data_ptr(), ea.data_ptr(), es.data_ptr(), None, None, L.F32, None, nel, ng, d5(1e-3),
                                      d5(b1), d5(b2), d5(eps), d5(0.0), 0, step, C.c_float(1.0), C.c_float(0.0), st)
    assert call() == 0
    assert call(pp=p.data_ptr() + 4) != 0               # misaligned
    assert call(ng=5) != 0 and call(ng=0) != 0
    assert call(eps=0.0) != 0 and call(b1=1.0) != 0 and call(b2=-0.1) != 0 and call(step=0) != 0 and call(nel=n + 2) != 0
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(es.abs().max()) == 0.0      # zero gradients: the one valid call moved nothing


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_loss_falls_with_fused_adam_focal_loss_and_ema(dev, dt):
    """The shape of test_train_loop_gpu.test_loss_falls_with_fused_optimizer_and_ema with --adam and fl_gamma = 1.5."""
    O = importlib.import_module(PKG + ".optim")
    LS = importlib.import_module(PKG + ".loss")
    S, B = 256, 2
    model, _ = build(dev, S)
    model.compute_dtype = dt
    model.train()
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP, fl_gamma=1.5), 1.0, 8
    ema = O.ModelEMA(model)
    opt = O.FusedAdam(O.set_weight_decay(model), model=model, lr=1e-3, ema=ema)
    compute_loss = LS.ComputeLoss(model)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    ir = torch.rand(B, 3, S, S, generator=g).to(dev)
    targets = LS.synthetic_targets(B, 16, 8, seed=1).to(dev)
    ls = []
    for _ in range(16):
        pred, _ = model(x, ir, "RGB+IR")
        loss = compute_loss(pred, targets)[0]
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        ema.update(model)
        ls.append(float(loss.detach()) / B)
    print(f"adam + focal loop {dt}: first {ls[0]:.6f} last {ls[-1]:.6f} all {[round(v, 5) for v in ls]}")
    assert all(v == v and abs(v) != float("inf") for v in ls), ls
    assert ls[-1] < ls[0], ls
    assert ema.updates == 16
    ema.ema.eval()
    with torch.no_grad():
        z = ema.ema(x, ir, "RGB+IR")[0]
    assert torch.isfinite(z).all()
