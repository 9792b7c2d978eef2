"""tests/test_train_loop_gpu.py's loop (2 x 256 x 256, a fixed batch, 16 steps) with optim.FusedSAM: step(closure) as the reference
drives basics/utils/sam.py, with bypass_bn's disable_running_stats / enable_running_stats around the closure's forward so that
only the first forward of a step moves the BatchNorm running statistics.  The loss per image at w (the first forward of a
step) must be lower at the last step than at the first; nothing is claimed against plain SGD.

Measured on an MI355X (first -> last loss per image): see DESIGN.md section 5, round 17."""
import importlib

import pytest
import torch

from test_model_gpu import build

pytestmark = pytest.mark.gpu
PKG = "small-object-detection-transformers_amd"


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_loss_falls_with_fused_sam(dev, dt, kind):
    O = importlib.import_module(PKG + ".optim")
    LS = importlib.import_module(PKG + ".loss")
    BN = importlib.import_module(PKG + ".bypass_bn")
    S, B = 256, 2
    model, _ = build(dev, S)
    model.compute_dtype = dt
    model.train()
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    ema = O.ModelEMA(model)
    if kind == "sgd":
        opt = O.FusedSAM(O.set_weight_decay(model), O.FusedSGD, model, rho=0.05, lr=0.01, momentum=0.937, nesterov=True, ema=ema)
    else:
        opt = O.FusedSAM(O.set_weight_decay(model), O.FusedAdam, model, rho=0.05, lr=1e-3, ema=ema)
    compute_loss = LS.ComputeLoss(model)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    ir = torch.rand(B, 3, S, S, generator=g).to(dev)
    targets = LS.synthetic_targets(B, 16, 8, seed=1).to(dev)
    bn = next(m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))

    def closure():
        BN.disable_running_stats(model)
        seen = bn.running_mean.clone()
        loss2 = compute_loss(model(x, ir, "RGB+IR")[0], targets)[0]
        loss2.backward()
        BN.enable_running_stats(model)
        assert torch.equal(bn.running_mean, seen)       # the second forward left the running statistics alone
        return loss2

    ls = []
    for _ in range(16):
        pred, _ = model(x, ir, "RGB+IR")
        loss = compute_loss(pred, targets)[0]
        loss.backward()
        opt.step(closure)
        opt.zero_grad(set_to_none=True)
        ema.update(model)
        ls.append(float(loss.detach()) / B)
    print(f"sam loop {kind} {dt}: loss per image first {ls[0]:.6f} last {ls[-1]:.6f} all {[round(v, 5) for v in ls]}")
    assert all(v == v for v in ls), ls
    assert ls[-1] < ls[0], ls
    assert ema.updates == 16 and bn.momentum == 0.03
    assert float(opt.sam_info()[0]) == 0.0
    ema.ema.eval()
    with torch.no_grad():
        z = ema.ema(x, ir, "RGB+IR")[0]
    assert torch.isfinite(z).all()
