"""Host-side checks of the --super loss term (no GPU): forward and backward of csrc/srloss.hip share their leading
arguments; the constants agree with the header; SRLoss names each bad input in a ValueError before anything
reaches the library; the entries themselves refuse bad arguments before a launch (exercised with host memory); and the
two-FMA form of float(k) / 255.0f the kernels use equals the IEEE quotient for every byte value."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

PKG = "small-object-detection-transformers_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_declared_exported_and_bound(pkg, ops):
    L = pkg._lib                    # (declared, exported, bound type for type: tests/test_abi_and_host.py, for every entry)
    hdr = open(os.path.join(ROOT, "include", "sodt_hip.h")).read()
    assert "Train.py:420-427" in hdr
    define = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)", hdr).group(1))
    assert define("SODT_U8") == L.U8 and define("SODT_F32") == L.F32
    assert {"IR": define("SODT_SR_IR"), "RGB": define("SODT_SR_RGB"), "RGB+IR": define("SODT_SR_RGB_IR")} == L.SR_MODES
    # forward and backward take the same leading description of the tensors
    assert L.SIGNATURES["sodt_sr_l1_fwd"][:11] == L.SIGNATURES["sodt_sr_l1_bwd"][:11]
    assert callable(ops.sr_l1_fwd) and callable(ops.sr_l1_bwd)
    # [ticket, 16 bytes] + one f64 per block of the form with the most blocks (the element-wise one: a block per 1024
    # elements of a plane), never more than 2048 blocks in all
    assert ops.sr_l1_workspace_bytes(2, 4, 40, 36) == 16 + 8 * 8 * 2
    assert ops.sr_l1_workspace_bytes(1, 4, 7, 5) == 16 + 8 * 4
    assert ops.sr_l1_workspace_bytes(2, 4, 256, 256) == 16 + 8 * 8 * 64
    assert ops.sr_l1_workspace_bytes(4, 4, 4096, 4096) == 16 + 8 * 2048
    for bad in ((0, 4, 8, 8), (2, 4, 0, 8), (65536, 1, 8, 8), (1, 1, 65536, 32768)):
        with pytest.raises(RuntimeError):
            ops.sr_l1_workspace_bytes(*bad)


def test_srloss_names_each_bad_input_before_any_library_call(monkeypatch):
    LS = importlib.import_module(PKG + ".loss")
    ops = importlib.import_module(PKG + ".ops")

    def no_call(*a, **k):
        raise AssertionError("a bad input reached the library")
    monkeypatch.setattr(ops, "_launch", no_call)
    monkeypatch.setattr(ops, "sr_l1_workspace_bytes", no_call)
    o = torch.zeros(2, 4, 8, 12)
    rgb, ir = torch.zeros(2, 3, 8, 12, dtype=torch.uint8), torch.zeros(2, 2, 8, 12, dtype=torch.uint8)
    fn = LS.SRLoss("RGB+IR")
    bad = [
        ("contiguous", (o.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), rgb, ir)),
        ("GPU", (o, rgb, ir)),                                              # a CPU tensor: every other property is right
        ("spatial", (o, rgb[:, :, :, :-1].contiguous(), ir)),
        ("spatial", (o, rgb, ir[:1])),
        ("C = 3", (o[:, :3].contiguous(), rgb, ir)),
        ("float32", (o.double(), rgb, ir)),
        ("float32", (o.bfloat16(), rgb, ir)),
        ("uint8", (o, rgb.long(), ir.long())),
        ("same dtype", (o, rgb, ir.float())),
        ("3 channels", (o, ir, ir)),
        ("ir must be contiguous", (o, rgb, torch.zeros(2, 2, 12, 8, dtype=torch.uint8).transpose(2, 3))),
        ("ir must be", (o, rgb, None)),
        ("rgb must be", (o, None, ir)),
        ("output_sr must be", (o[0], rgb, ir)),
    ]
    for word, args in bad:
        with pytest.raises(ValueError, match=word):
            fn(*args)
    with pytest.raises(ValueError, match="1 channel"):
        LS.SRLoss("IR")(o, None, ir)
    with pytest.raises(ValueError, match="GPU"):
        LS.SRLoss("IR")(o[:, :1].contiguous(), None, ir)                    # rgb is not needed in this mode
    with pytest.raises(ValueError, match="GPU"):
        LS.SRLoss("RGB")(o[:, :3].contiguous(), rgb, None)
    with pytest.raises(ValueError, match="input_mode"):
        LS.SRLoss("rgb+ir")


def test_entries_refuse_bad_arguments_before_a_launch(pkg):
    """Argument checks come before the memset and the launch, so they can be exercised with host memory and no device."""
    L = pkg._lib
    lib = L.load()
    B, Cc, H, W = 2, 4, 4, 8
    n = B * Cc * H * W
    f = [(C.c_float * (n + 8))() for _ in range(3)]
    sr, dsr, scal = [(C.addressof(b) + 15) & ~15 for b in f]
    u = [(C.c_ubyte * (n + 8))() for _ in range(2)]
    rgb, ir = [(C.addressof(b) + 15) & ~15 for b in u]
    nb = C.c_size_t(0)
    assert lib.sodt_sr_l1_workspace_bytes(B, Cc, H, W, C.byref(nb)) == 0 and nb.value == 16 + 8 * 8
    assert lib.sodt_sr_l1_workspace_bytes(B, Cc, H, W, None) != 0
    ws_buf = (C.c_char * (nb.value + 16))()
    ws = (C.addressof(ws_buf) + 15) & ~15

    def fwd(sr=sr, rgb=rgb, ir=ir, code=L.U8, mode=2, Cx=Cc, c_rgb=3, c_ir=1, Hx=H, ws=ws, wsb=nb.value, loss=scal):
        return lib.sodt_sr_l1_fwd(sr, rgb, ir, code, mode, B, Cx, c_rgb, c_ir, Hx, W, ws, wsb, loss, None)

    def bwd(sr=sr, ir=ir, code=L.U8, mode=2, Cx=Cc, c_rgb=3, up=scal, d=dsr):
        return lib.sodt_sr_l1_bwd(sr, rgb, ir, code, mode, B, Cx, c_rgb, 1, H, W, up, d, None)
    common = open(os.path.join(ROOT, "include", "sodt_hip.h")).read()
    einval = int(re.search(r"#define\s+SODT_EINVAL\s+(-?\d+)", common).group(1))
    for rc in (fwd(sr=None), fwd(sr=sr + 2), fwd(rgb=None), fwd(ir=None), fwd(code=L.BF16), fwd(code=L.F32, rgb=rgb + 1),
               fwd(mode=3), fwd(mode=-1), fwd(mode=0), fwd(mode=1), fwd(Cx=3), fwd(Cx=5), fwd(c_rgb=1), fwd(c_ir=0), fwd(Hx=0),
               fwd(Hx=-4), fwd(ws=None), fwd(ws=ws + 8), fwd(wsb=nb.value - 1), fwd(loss=None), fwd(loss=scal + 1),
               bwd(sr=None), bwd(ir=None), bwd(code=7), bwd(mode=5), bwd(Cx=1), bwd(c_rgb=4), bwd(up=None), bwd(up=scal + 2),
               bwd(d=None), bwd(d=dsr + 1)):
        assert rc == einval
    assert all(v == 0.0 for v in f[1]) and bytes(ws_buf) == bytes(len(ws_buf))          # nothing was written


def test_two_fma_quotient_is_the_ieee_division_for_every_byte():
    """csrc/srloss.hip forms float(k) / 255.0f as q = k * r, q + (k - q * 255) * r with r = RN(1 / 255) and fused multiply-adds
    (an FMA rounds once: restated here in f64 - the remainder k - q * 255 is exact there - and rounded to f32; on the device
    tests/test_sr_loss_gpu.py compares the uint8 route bit for bit with f32 targets divided on the host)."""
    src = open(os.path.join(ROOT, PKG, "csrc", "srloss.hip")).read()
    r = np.float32(float.fromhex(re.search(r"r = (0x[0-9a-f.]+p-?\d+)f", src).group(1)))
    assert r == np.float32(1.0) / np.float32(255.0)
    k = np.arange(256, dtype=np.float32)
    q = k * r                                                               # one f32 rounding
    e = (k.astype(np.float64) - q.astype(np.float64) * 255.0).astype(np.float32)          # fmaf(-q, 255, k): exact in f64
    got = (q.astype(np.float64) + e.astype(np.float64) * float(r)).astype(np.float32)     # fmaf(e, r, q)
    want = k / np.float32(255.0)
    assert np.array_equal(got, want)
    assert int((q != want).sum()) > 100            # the plain product with the reciprocal is NOT the quotient
    assert np.array_equal(want, (torch.arange(256, dtype=torch.uint8).float() / 255).numpy())
