"""ComputeLoss of the reference's training step (basics/utils/loss.py:90-224) on the device: build_targets, CIoU box loss,
objectness and class BCE and their gradient with respect to the head output in four small launches (csrc/loss.hip,
``sodt_yolo_loss``) - no autograd graph over ~60 ATen kernels, no host synchronisation.  Same constructor, call
signature and return tuple as the reference class, so ``compute_loss = ComputeLoss(model)`` /
``loss, lbox, lobj, lcls = compute_loss(pred, targets)`` (Train.py:281,418) port unchanged.

``hyp['fl_gamma'] > 0`` (off in models/hyp.scratch.yaml, mutated in (0, 2] by ``--evolve``, Train.py:720) wraps the class
and the objectness BCE in the reference's ``FocalLoss(BCEWithLogitsLoss(pos_weight), gamma, alpha=0.25)``
(basics/utils/loss.py:36-62, :103-108), value and gradient, inside the same four launches (``sodt_yolo_loss_fl``);
``fl_gamma == 0`` calls ``sodt_yolo_loss`` as before.

``SRLoss`` is the term ``--super`` adds to that loss (Train.py:420-427), computed from ``output_sr`` and the uint8 batches
the dataloader delivers in one pass forward and one pass backward (csrc/srloss.hip, ``sodt_sr_l1_fwd`` / ``_bwd``):
``loss += SRLoss(opt.input_mode)(output_sr, imgs_u8, irs_u8)`` replaces the three branches, and the full-resolution f32
``image`` / ``ir_image`` of Train.py:364-365 are no longer needed for it.

Not carried over: ``autobalance`` (off in Train.py:281) and label smoothing other than the reference's hard-coded
``smooth_BCE(eps=0.0)`` (loss.py:104); asking for them raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import ops


DEFAULT_HYP = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0)   # models/hyp.scratch.yaml


def synthetic_targets(B: int, per_image: int = 32, nc: int = 8, seed: int = 0) -> torch.Tensor:
    """Benchmark targets: per image `per_image` boxes, class ~U{0..nc-1}, centre ~U(0.05, 0.95),
    size ~U(0.01, 0.05); rows (image, class, x, y, w, h) as Train.py:362 delivers them."""
    g = torch.Generator().manual_seed(seed)
    n = B * per_image
    img = torch.arange(B).repeat_interleave(per_image).float()
    cls = torch.randint(0, nc, (n,), generator=g).float()
    xy = 0.05 + 0.9 * torch.rand(n, 2, generator=g)
    wh = 0.01 + 0.04 * torch.rand(n, 2, generator=g)
    return torch.cat((img[:, None], cls[:, None], xy, wh), 1)


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, targets, anchors, hyp, gr, nc):
        B, na, ny, nx, no = pred.shape
        nt = int(targets.shape[0])
        dpred = torch.empty_like(pred)
        out = torch.empty(4, device=pred.device, dtype=torch.float32)
        nbytes = ops._ws_bytes("sodt_yolo_loss_workspace_bytes", B * na * ny * nx, nt, nc,
                               msg="sodt_yolo_loss_workspace_bytes: unsupported shape (nc <= 32)")
        ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
        focal = hyp["fl_gamma"] > 0
        ops._launch("sodt_yolo_loss_fl" if focal else "sodt_yolo_loss", pred.data_ptr(), targets.data_ptr() if nt else None, nt,
                    anchors.data_ptr(), B, na, ny, nx, nc, C.c_float(hyp["box"]), C.c_float(hyp["cls"]), C.c_float(hyp["cls_pw"]),
                    C.c_float(hyp["obj"]), C.c_float(hyp["obj_pw"]), C.c_float(hyp["anchor_t"]), C.c_float(gr),
                    *((C.c_float(hyp["fl_gamma"]),) if focal else ()), ws.data_ptr(), nbytes, dpred.data_ptr(), out.data_ptr())
        ctx.save_for_backward(dpred)
        # independent tensors, not slices of `out`: views of one buffer returned by a multi-output Function are
        # MULTI_OUTPUT_NODE views on which the reference loop's in-place `loss *= opt.world_size` (Train.py:440),
        # `loss *= 4.` and `loss += sr_loss` raise
        loss, lbox, lobj, lcls = (out[i:i + 1].clone() for i in range(4))
        ctx.mark_non_differentiable(lbox, lobj, lcls)
        return loss, lbox, lobj, lcls

    @staticmethod
    def backward(ctx, g_loss, g_box, g_obj, g_cls):
        (dpred,) = ctx.saved_tensors
        # only the total is differentiated by the training loop (Train.py:445); the three components are reporting values
        return dpred * g_loss.to(dpred.dtype).reshape(()), None, None, None, None, None


class ComputeLoss:
    def __init__(self, model, autobalance: bool = False):
        if autobalance:
            raise NotImplementedError("autobalance is off in the reference's training loop (Train.py:281)")
        h = model.hyp
        det = model.module.detect[-1] if hasattr(model, "module") else model.detect[-1]
        if det.nl != 1:
            raise NotImplementedError("one detection layer (models/model.yaml)")
        self.hyp, self.gr, self.autobalance = h, model.gr, False
        self.cp, self.cn = 1.0, 0.0                 # smooth_BCE(eps=0.0), loss.py:104
        self.balance = [4.0, 1.0, 0.25, 0.06, .02]  # loss.py:110 for nl == 1
        for k in ("na", "nc", "nl", "anchors"):
            setattr(self, k, getattr(det, k))

    def __call__(self, p, targets):
        pred = p[0] if isinstance(p, (list, tuple)) else p
        if not pred.is_cuda:
            raise RuntimeError("ComputeLoss needs the head output on the GPU: there is no CPU fallback")
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        targets = targets.to(device=pred.device, dtype=torch.float32).contiguous()
        anchors = self.anchors[0].to(device=pred.device, dtype=torch.float32).contiguous()
        hyp = {k: float(self.hyp[k]) for k in ("box", "cls", "cls_pw", "obj", "obj_pw", "anchor_t")}
        hyp["fl_gamma"] = float(self.hyp.get("fl_gamma", 0.0))      # read per call, like the rest: --evolve rewrites hyp
        return _LossFn.apply(pred, targets, anchors, hyp, float(self.gr), int(self.nc))


class _SRLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output_sr, rgb, ir, mode):
        B, Cc, H, W = output_sr.shape
        ws = torch.empty(ops.sr_l1_workspace_bytes(B, Cc, H, W), device=output_sr.device, dtype=torch.uint8)
        loss = torch.empty((), device=output_sr.device, dtype=torch.float32)
        ops.sr_l1_fwd(output_sr, rgb, ir, mode, ws, loss)
        # references to the inputs, not copies: the backward reads output_sr and the targets again
        ctx.save_for_backward(output_sr, rgb, ir)
        ctx.mode = mode
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        output_sr, rgb, ir = ctx.saved_tensors
        # the incoming gradient stays on the device: it carries GradScaler's scale, the world size and the --quad factor
        upstream = g_loss.to(torch.float32).contiguous()
        dsr = torch.empty_like(output_sr)
        ops.sr_l1_bwd(output_sr, rgb, ir, ctx.mode, upstream, dsr)
        return dsr, None, None, None


class SRLoss:
    """The super-resolution term of Train.py:420-427 (``--super``) for ``input_mode`` 'IR', 'RGB' or 'RGB+IR':

        0.5 * L1(output_sr, ir)   |   0.5 * L1(output_sr, rgb)   |   0.1 * (L1(output_sr[:, :3], rgb) + L1(output_sr[:, 3:], ir[:, :1]))

    ``SRLoss(input_mode)(output_sr, rgb, ir)`` -> 0-dim f32 device tensor with autograd.  ``output_sr``: f32 (B, C, H, W)
    contiguous, as the engine returns it; ``rgb`` / ``ir``: the uint8 (B, c, H, W) batches as the dataloader delivers them
    (``t = u8 / 255`` is formed per element, as ``imgs.float() / 255.0`` does), or f32 tensors already in [0, 1]; of ``ir``
    only plane 0 is read; the batch a mode does not use may be None.  Anything else raises ValueError before a launch."""

    def __init__(self, input_mode: str = "RGB+IR"):
        if input_mode not in L.SR_MODES:
            raise ValueError(f"SRLoss: input_mode must be one of {sorted(L.SR_MODES)}, not {input_mode!r}")
        self.input_mode = input_mode

    def _check(self, output_sr, rgb, ir):
        mode = self.input_mode
        if not isinstance(output_sr, torch.Tensor) or output_sr.dim() != 4:
            raise ValueError("SRLoss: output_sr must be a (B, C, H, W) tensor")
        if output_sr.dtype != torch.float32:
            raise ValueError(f"SRLoss: output_sr must be float32, not {output_sr.dtype}")
        if not output_sr.is_contiguous():
            raise ValueError("SRLoss: output_sr must be contiguous (NCHW)")
        B, Cc, H, W = output_sr.shape
        if output_sr.numel() == 0 or B * Cc > 65535 or H * W >= 2 ** 31:
            raise ValueError(f"SRLoss: unsupported output_sr shape {tuple(output_sr.shape)}")
        want = {"IR": (1, None), "RGB": (Cc, Cc), "RGB+IR": (4, 3)}[mode]
        if Cc != want[0]:
            raise ValueError(f"SRLoss: input_mode {mode!r} needs output_sr with {want[0]} channel(s), got C = {Cc}")
        used = {"IR": (("ir", ir),), "RGB": (("rgb", rgb),), "RGB+IR": (("rgb", rgb), ("ir", ir))}[mode]
        for name, t in used:
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"SRLoss: {name} must be a (B, c, H, W) tensor for input_mode {mode!r}")
            if t.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"SRLoss: {name} must be uint8 (or float32 in [0, 1]), not {t.dtype}")
            if t.dtype != used[0][1].dtype:
                raise ValueError("SRLoss: rgb and ir must have the same dtype")
            if t.shape[0] != B or tuple(t.shape[2:]) != (H, W):
                raise ValueError(f"SRLoss: {name} has shape {tuple(t.shape)}, output_sr {tuple(output_sr.shape)}: "
                                 "batch and spatial size must agree")
            if name == "rgb" and t.shape[1] != want[1]:
                raise ValueError(f"SRLoss: rgb must have {want[1]} channels for input_mode {mode!r}, got {t.shape[1]}")
            if t.shape[1] < 1:
                raise ValueError(f"SRLoss: {name} has no channel")
            if not t.is_contiguous():
                raise ValueError(f"SRLoss: {name} must be contiguous")
        if not output_sr.is_cuda:
            raise ValueError("SRLoss: output_sr must be on the GPU device: there is no CPU fallback")
        for name, t in used:
            if t.device != output_sr.device:
                raise ValueError(f"SRLoss: {name} is on device {t.device}, output_sr on {output_sr.device}")
        return dict(used)

    def __call__(self, output_sr, rgb=None, ir=None):
        used = self._check(output_sr, rgb, ir)
        return _SRLossFn.apply(output_sr, used.get("rgb"), used.get("ir"), self.input_mode)
