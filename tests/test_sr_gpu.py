"""The super-resolution branch on the HIP kernels (sr.py: Decoder + EDSR = DeepLab, basics/models/deeplabedsr.py:35-73,
sr_decoder_noBN_noD.py:6-45, edsr.py:55-102) against tests/golden/sr.pt, which holds what the reference's own classes produce on the
procedural weights (oracle/gen_golden.py --only-sr): outputs, input gradients, every parameter's gradient norm and 64 strided gradient
values.  f32 is the parity run (tight); bf16 is the throughput dtype (loose).
The layout converters behind the _rows / _nchw helpers are pinned bit for bit by tests/test_sr_movement_gpu.py."""
import importlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# f32: (output / input-gradient max error over the tensor's max magnitude, gradient-norm relative error) against the goldens.
# bf16 is calibrated instead: see _oracle_runs / _check_bf16.
TOL = {torch.float32: (2e-4, 2e-4), torch.bfloat16: (None, None)}
TOL_DEEP = {torch.float32: (1e-3, 1e-3), torch.bfloat16: (None, None)}       # 37 convolutions in sequence


def _setup(name, dev, dt):
    from oracle import ref_torch as R
    S = importlib.import_module("small-object-detection-transformers_amd.sr")
    g = torch.load(os.path.join(GOLD, "sr.pt"))[name]
    _rel.l2 = dt == torch.bfloat16
    sd = {k: v.float().contiguous().to(dev) for k, v in R.procedural_from_shapes(g["shapes"]).items()}
    return R, S, g, sd


def _rows(ops, x, dev, dt):
    B, C, H, W = x.shape
    r = torch.zeros(B * H * W, C, device=dev, dtype=dt)
    ops.rows_from_nchw_f32(x.to(dev).contiguous(), r, B, C, H, W)
    return r


def _nchw(ops, r, B, C, H, W):
    y = torch.empty(B, C, H, W, device=r.device, dtype=torch.float32)
    ops.nchw_f32_from_rows(r, y, B, C, H, W)
    return y


def _rel(a, b):
    """f32: max error over the tensor's max magnitude.  bf16: relative L2 error - single elements move by whole terms when a
    ReLU input within bf16 rounding of zero changes sign, which says nothing about the kernels."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if _rel.l2:
        return float((a - b).norm()) / max(1e-9, float(b.norm()))
    return float((a - b).abs().max()) / max(1e-9, float(b.abs().max()))


_rel.l2 = False


class _RoundBf16(torch.autograd.Function):
    """identity that rounds to bf16 on the way forward AND on the way back: what a bf16 tensor in HBM does to a value / gradient."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


def _oracle_runs(R, name, g, monkeypatch):
    """The oracle on the CPU twice: float32 (pinned to the reference's classes by tests/test_oracle_golden.py) and with every
    convolution's operands and result rounded to bf16 both ways - the storage rounding of the bf16 run, ReLU inputs within
    rounding of zero changing sign included.  The second calibrates what a correct bf16 implementation can deliver:
    returns ({tensor name: f32 result}, {tensor name: rel. L2 error of the emulated bf16 run})."""
    def run(emulate):
        sd = {k: v.clone().requires_grad_(True) for k, v in R.procedural_from_shapes(g["shapes"]).items()}
        ins = [t.clone().requires_grad_(True) for t in g["inputs"]]
        with monkeypatch.context() as mp:
            if emulate:
                conv = R.F.conv2d
                rq = _RoundBf16.apply
                mp.setattr(R.F, "conv2d", lambda x, w, b=None, *a, **k: rq(conv(rq(x), rq(w), b, *a, **k)))
            if name == "decoder":
                y = R.sr_decoder(sd, "sr_decoder.", ins[1], ins[0], 2)
            elif name == "edsr":
                y = R.edsr(sd, "edsr.", ins[0])
            else:
                y = R.deeplab_sr(sd, "model_up.", ins[0], ins[1], 2)
        gsel = R._hash01("sr:" + name, y.numel()).view(y.shape).float()
        (y * gsel).sum().backward()
        out = {"y": y.detach()}
        out.update({f"din{i}": t.grad for i, t in enumerate(ins)})
        out.update({k: v.grad for k, v in sd.items()})
        return out
    ref, emu = run(False), run(True)
    return ref, {k: float((emu[k].double() - ref[k].double()).norm()) / max(1e-12, float(ref[k].double().norm())) for k in ref}


def _check_bf16(got, ref, emu_err, what):
    """ours vs the f32 oracle: no worse than 1.5 x the emulated-bf16 oracle's own distance from it (+ 1 %)"""
    for k, v in got.items():
        e = float((v.detach().double().cpu() - ref[k].double()).norm()) / max(1e-12, float(ref[k].double().norm()))
        assert e <= 1.5 * emu_err[k] + 1e-2, f"{what} {k}: rel. L2 error {e:.3e}, emulated bf16 oracle {emu_err[k]:.3e}"


def _check_grads(br, g, tol, what):
    worst = 0.0
    for k, v in g["gnorm"].items():
        got = br.g[k]
        n = float(got.double().norm())
        assert abs(n - v) <= tol * (v + 1e-9), f"{what} {k}: grad norm {n:.6e} vs {v:.6e}"
        sub = got.reshape(-1)[::max(1, got.numel() // 64)][:64]
        e = _rel(sub, g["gsub"][k])
        worst = max(worst, e)
        assert e <= 4 * tol, f"{what} {k}: strided gradient values off by {e:.3e}"
    return worst


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_sr_decoder_matches_reference_golden(ops, dev, dt, monkeypatch):
    R, S, g, sd = _setup("decoder", dev, dt)
    low, x = g["inputs"]                        # (2, 16, 12, 10), (2, 32, 6, 5)
    B, c1, H, W = low.shape
    br = S.SRBranch(sd, dt)
    d3 = br.decoder_forward([ops.SegSpec(_rows(ops, low, dev, dt))], [ops.SegSpec(_rows(ops, x, dev, dt))], B, H, W)
    y = _nchw(ops, d3, B, 64, H, W)
    to, tg = TOL[dt]
    st = g["y_step"]
    gsel = R._hash01("sr:decoder", y.numel()).view(y.shape).float()
    d_low, d_x = br.decoder_backward(_rows(ops, gsel, dev, dt))
    torch.cuda.synchronize()
    d_low, d_x = _nchw(ops, d_low, B, c1, H, W), _nchw(ops, d_x, B, x.shape[1], H // 2, W // 2)
    if dt == torch.bfloat16:
        ref, emu = _oracle_runs(R, "decoder", g, monkeypatch)
        _check_bf16(dict(y=y, din0=d_low, din1=d_x, **br.g), ref, emu, "decoder")
        return
    assert _rel(y[..., ::st, ::st], g["y_sub"]) <= to
    assert _rel(d_low, g["dinputs"][0]) <= to
    assert _rel(d_x, g["dinputs"][1]) <= to
    _check_grads(br, g, tg, "decoder")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_sr_edsr_matches_reference_golden(ops, dev, dt, monkeypatch):
    R, S, g, sd = _setup("edsr", dev, dt)
    (x,) = g["inputs"]                          # (1, 64, 7, 6) -> (1, 4, 56, 48)
    B, _, H, W = x.shape
    br = S.SRBranch(sd, dt)
    y = br.edsr_forward(_rows(ops, x, dev, dt), B, H, W)
    to, tg = TOL[dt]
    st = g["y_step"]
    assert tuple(y.shape) == (B, 4, 8 * H, 8 * W)
    gsel = R._hash01("sr:edsr", y.numel()).view(y.shape).float().to(dev)
    dx = br.edsr_backward(gsel.contiguous())
    torch.cuda.synchronize()
    dx = _nchw(ops, dx, B, 64, H, W)
    if dt == torch.bfloat16:
        ref, emu = _oracle_runs(R, "edsr", g, monkeypatch)
        _check_bf16(dict(y=y, din0=dx, **br.g), ref, emu, "edsr")
        return
    assert _rel(y[..., ::st, ::st], g["y_sub"]) <= to
    assert _rel(dx, g["dinputs"][0]) <= to
    _check_grads(br, g, tg, "edsr")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_sr_deeplab_matches_reference_golden(ops, dev, dt, monkeypatch):
    """DeepLab(4, 128, 512, factor 2) as model.py:113-115 builds it (EDSR depth 16, 2.9 M parameters): 128 @ 16 x 16 and
    512 @ 8 x 8 in, (1, 4, 128, 128) out; twice over, to show that the gradients accumulate and the buffers are reused."""
    R, S, g, sd = _setup("deeplab", dev, dt)
    low, x = g["inputs"]
    B, c1, H, W = low.shape
    br = S.SRBranch(sd, dt, dec="model_up.sr_decoder.", edsr="model_up.edsr.")
    assert br.depth == 16
    lr, xr = _rows(ops, low, dev, dt), _rows(ops, x, dev, dt)
    to, tg = TOL_DEEP[dt]
    st = g["y_step"]
    if dt == torch.bfloat16:
        ref, emu = _oracle_runs(R, "deeplab", g, monkeypatch)
    for rep in range(2):
        y = br.forward([ops.SegSpec(lr)], [ops.SegSpec(xr)], B, H, W)
        assert tuple(y.shape) == (B, 4, 8 * H, 8 * W)
        gsel = R._hash01("sr:deeplab", y.numel()).view(y.shape).float().to(dev)
        d_low, d_x = br.backward(gsel.contiguous())
        torch.cuda.synchronize()
        d_low, d_x = _nchw(ops, d_low, B, c1, H, W), _nchw(ops, d_x, B, x.shape[1], H // 2, W // 2)
        if dt == torch.bfloat16:
            _check_bf16(dict(y=y, din0=d_low, din1=d_x, **(br.g if rep == 0 else {})), ref, emu, "deeplab")
        else:
            assert _rel(y[..., ::st, ::st], g["y_sub"]) <= to
            assert _rel(d_low, g["dinputs"][0]) <= to
            assert _rel(d_x, g["dinputs"][1]) <= to
        if rep == 0:
            if dt == torch.float32:
                _check_grads(br, g, tg, "deeplab")
            first = {k: v.clone() for k, v in br.g.items()}
    for k, v in br.g.items():                    # the second pass added the same gradients again
        assert float((v - 2 * first[k]).abs().max()) <= 1e-3 * (float(first[k].abs().max()) + 1e-9), k


def test_sr_upsampled_low_level_view(ops, dev):
    """The low-level input may be an upsampling VIEW (y[8] = Upsample(y7) in the head graph): SegSpec(shr=1) over the half-size
    tensor equals materialising the nearest x2 copy first."""
    S = importlib.import_module("small-object-detection-transformers_amd.sr")
    from oracle import ref_torch as R
    dt = torch.float32
    _rel.l2 = False
    shapes = {"sr_decoder." + k[len("sr_decoder."):]: v for k, v in S.sr_param_shapes(4, 16, 32).items() if k.startswith("sr_decoder.")}
    sd = {k: v.float().contiguous().to(dev) for k, v in R.procedural_from_shapes(shapes).items()}
    B, H, W = 2, 8, 12
    g = torch.Generator().manual_seed(5)
    half = torch.randn(B, 16, H // 2, W // 2, generator=g)
    x = torch.randn(B, 32, H // 2, W // 2, generator=g)
    full = half.repeat_interleave(2, 2).repeat_interleave(2, 3)
    a, b = S.SRBranch(sd, dt), S.SRBranch(sd, dt)
    ya = a.decoder_forward([ops.SegSpec(_rows(ops, full, dev, dt))], [ops.SegSpec(_rows(ops, x, dev, dt))], B, H, W)
    hv = _rows(ops, half, dev, dt)
    yb = b.decoder_forward([ops.SegSpec(hv, 16, 0, 0, 0, 1, 1, H // 2, W // 2)], [ops.SegSpec(_rows(ops, x, dev, dt))], B, H, W)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb)
    dy = torch.randn(B * H * W, 64, generator=g).to(dev)
    da, _ = a.decoder_backward(dy)
    db, _ = b.decoder_backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(da, db)
    for k in a.g:
        assert _rel(b.g[k], a.g[k]) <= 1e-5, k
