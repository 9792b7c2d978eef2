"""Fused optimizer step + EMA for the training loop around the hot path.

The reference steps with ``optim.SGD(pg0, lr=hyp['lr0'], momentum=hyp['momentum'], nesterov=True)`` over the two
weight-decay groups of ``basics/optimizer.py:35-49`` (Train.py:139-150), calls ``scaler.step(optimizer)`` every
``accumulate`` batches (Train.py:448-450) and then ``ema.update(model)`` - a Python loop over the 273 state_dict tensors
(basics/utils/torch_utils.py:291-301).  Here the engine keeps parameters, gradients, momentum and the EMA in flat f32
buffers of one layout, so all of it - plus the cast of the updated masters to the bf16 copy the GEMM kernels read - is
ONE streaming kernel (csrc/optim.hip, ``sodt_sgd_ema_step``).

``FusedAdam`` is the same for Train.py's ``--adam`` (Train.py:147-148: ``optim.Adam(pg0, lr=hyp['lr0'],
betas=(hyp['momentum'], 0.999))``) and, with ``decoupled=True``, for the AdamW that ``basics/optimizer.py:11-33`` names:
``sodt_adam_ema_step``, one launch with the same EMA and cast tail.

``FusedSGD`` is a ``torch.optim.Optimizer``: param groups, ``lr`` / ``momentum`` / ``weight_decay`` per group (the
warm-up of Train.py:375-385 writes them every iteration), LR schedulers and ``zero_grad`` behave as with torch's SGD.
``ModelEMA`` mirrors the reference class (``.ema``, ``.updates``, ``.decay``, ``update``, ``update_attr``); attached to
the optimizer (``FusedSGD(..., ema=ema)`` / ``FusedAdam(..., ema=ema)``) its parameter average rides in the fused
kernel and ``ema.update(model)`` only handles the few non-parameter buffers.

The control path.  Both optimizers declare ``_step_supports_amp_scaling``, so ``torch.amp.GradScaler.step`` (Train.py:285,
:445-450) hands its scale and found-inf DEVICE tensors to ``step()`` instead of unscaling 273 gradient views and reading
``found_inf`` on the host.  ``step()`` then issues two launches: ``sodt_grad_stats`` (one pass over the flat gradient that
leaves found_inf, the f64 gradient norm, the clip coefficient and the effective gradient factor in a small device record)
and the ``_ctl`` sibling of the step kernel, which reads that record.  The same path serves ``skip_nonfinite=True`` (a
step whose gradient holds an inf / NaN changes neither parameters nor optimizer state; the EMA average and the run-dtype
mirror still run, as ``ema.update`` after a skipped ``scaler.step`` does in the reference) and ``max_grad_norm``
(``torch.nn.utils.clip_grad_norm_`` over every owned parameter, applied to the unscaled gradient).  No host read happens
on this path.  With neither option and no scaler, ``step()`` is the one launch it always was.

Data parallel: ``ddp.attach`` all-reduces the flat gradient before the step, so every rank sees the same gradient and
takes the same skip and clip decisions; no collective is added for them.

``FusedSAM`` wraps either of them with the reference's sharpness-aware steps (basics/utils/sam.py: ``first_step`` /
``second_step`` / ``step(closure)``): the gradient norm and the perturbation with its ``old_p`` copy and mirror are two launches,
the restore a third, and the base optimizer's step runs unchanged after it (csrc/sam.hip).
"""
from __future__ import annotations

import math
from copy import deepcopy
from typing import Optional

import torch

from . import ops


def set_weight_decay(model, skip_list=(), skip_keywords=(), weight_decay: float = 0.00048):
    """basics/optimizer.py:35-49: 1-D parameters and biases are not decayed."""
    has_decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.dim() == 1 or name.endswith(".bias") or name in skip_list or any(k in name for k in skip_keywords):
            no_decay.append(p)
        else:
            has_decay.append(p)
    return [{"params": has_decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0.0}]


class ModelEMA:
    """basics/utils/torch_utils.py:271-301 with the parameter average kept in one flat f32 buffer (the EMA module's
    parameters are views of it, so ``ema.ema`` is an ordinary Model for evaluation and checkpoints)."""

    def __init__(self, model, decay: float = 0.9999, updates: int = 0):
        model._get_engine()                 # (parameters of `model` live in its engine's flat buffer from here on)
        self.ema = deepcopy(model).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / 2000))
        for p in self.ema.parameters():
            p.requires_grad_(False)
        # the copy's own engine re-homes ITS parameters into a flat buffer of the same layout: that buffer is the average
        self.flat = self.ema._get_engine().flat_param
        self._fused_pending = False        # set by FusedSGD / FusedAdam.step when the parameter average was done in the fused kernel

    def next_decay(self) -> float:
        return self.decay(self.updates + 1)

    def update(self, model):
        with torch.no_grad():
            self.updates += 1
            d = self.decay(self.updates)
            msd = model.state_dict()
            if self._fused_pending:          # parameters already averaged with this d by the optimizer's kernel
                self._fused_pending = False
                names = [k for k, _ in self.ema.named_buffers()]
            else:
                names = list(self.ema.state_dict().keys())
            esd = self.ema.state_dict()
            dst = [esd[k] for k in names if esd[k].dtype.is_floating_point]
            src = [msd[k].detach() for k in names if esd[k].dtype.is_floating_point]
            if dst:
                torch._foreach_mul_(dst, d)
                torch._foreach_add_(dst, src, alpha=1.0 - d)
            if self.ema._engine is not None:
                self.ema._engine.invalidate_params()

    def update_attr(self, model, include=(), exclude=("process_group", "reducer")):
        for k, v in model.__dict__.items():
            if (len(include) and k not in include) or k.startswith("_") or k in exclude:
                continue
            setattr(self.ema, k, v)


class _FusedOptimizer(torch.optim.Optimizer):
    """What FusedSGD and FusedAdam share: the engine binding with the chunk -> group map, the skipped step when no backward
    ran, the attached-EMA protocol and the freshness of the run-dtype mirror around the one kernel `_launch_step` issues."""

    _entry = ""            # the C entry, for messages
    _n_state = 0           # flat f32 state buffers of the parameters' layout (momentum; exp_avg and exp_avg_sq)
    _step_supports_amp_scaling = True      # GradScaler.step sets .grad_scale / .found_inf (device tensors) and calls step()

    def __init__(self, params, defaults, model, ema, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (a positive number, or None for no clipping)")
        super().__init__(params, defaults)
        if len(self.param_groups) > 4:
            raise ValueError(f"at most 4 parameter groups ({self._entry})")
        self.model, self.ema = model, ema
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ctl = None           # the device control record (ops.new_step_ctl), made at the first control-path step
        self._eng = None
        self._state = None
        self._groups = None
        self._sig = None

    def _bind(self):
        eng = self.model._get_engine()
        if eng is not self._eng:
            self._eng, self._state, self._sig = eng, [torch.zeros_like(eng.flat_param) for _ in range(self._n_state)], None
        # (the requires_grad bits are part of the signature: a parameter frozen after the optimizer was built - Train.py:328-333 -
        #  has no gradient, and torch's optimizers pass over a parameter whose .grad is None: no decay, no momentum, no moment update)
        sig = tuple(tuple((id(p), p.requires_grad) for p in g["params"]) for g in self.param_groups)
        if sig != self._sig:       # chunk -> group map (255: padding / frozen parameters / parameters this optimizer does not own)
            gmap = torch.full((eng.flat_param.numel() // 4,), 255, dtype=torch.uint8)
            off_of = {id(eng.params[n]): (eng.grad_offsets[n], eng.params[n].numel()) for n in eng.grad_order}
            for gi, g in enumerate(self.param_groups):
                for p in g["params"]:
                    if id(p) not in off_of:
                        raise ValueError(f"{type(self).__name__}: a parameter does not belong to the model's engine")
                    o, n = off_of[id(p)]
                    gmap[o // 4: (o + n + 3) // 4] = gi if p.requires_grad else 255
            self._groups, self._sig = gmap.to(eng.dev), sig
        return eng

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        eng = self._bind()
        eng._check_param_views()
        if eng._claim_grads():              # no backward since zero_grad(set_to_none=True): torch skips parameters without a gradient
            eng.flat_grad.zero_()
            return loss
        self._check_groups()
        ema_flat, d = None, 0.0
        if self.ema is not None:
            ema_eng = self.ema.ema._get_engine()
            if self.ema.flat is not ema_eng.flat_param:       # the EMA model's engine was rebuilt (fuse(), unpickled / assigned model)
                self.ema.flat = ema_eng.flat_param
            ema_eng._check_param_views()
            ema_flat, d = self.ema.flat, self.ema.next_decay()
            self.ema._fused_pending = True
        cast = next(iter(eng.flat_cast.values())) if eng.flat_cast else None
        # torch.amp.GradScaler.step sets these two attributes around its call of step(): the scale (None after
        # scaler.unscale_: the gradients are already unscaled) and the found-inf sum, both f32 tensors on the device
        amp_scale, amp_found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        amp = amp_scale is not None or amp_found is not None
        if amp or self.skip_nonfinite or self.max_grad_norm is not None:
            ctl = self._ctl_record(eng)
            ops.grad_stats(eng.flat_grad, self._groups, ctl, amp_scale, amp_found, grad_scale, self.max_grad_norm,
                           amp or self.skip_nonfinite)
            self._launch_step_ctl(eng, ema_flat, cast, ctl, d)
        else:
            self._launch_step(eng, ema_flat, cast, grad_scale, d)
        if cast is not None:
            eng.mark_cast_fresh()
        else:
            eng.invalidate_params()         # (no mirror to keep fresh; the engine still has to know the masters moved: _param_epoch)
        return loss

    def _check_groups(self):
        pass

    def _ctl_record(self, eng):
        if self._ctl is None or self._ctl.device != eng.flat_grad.device:
            self._ctl = ops.new_step_ctl(eng.flat_grad.device)
        return self._ctl

    def last_step_info(self):
        """``(found_inf, grad_norm)`` of the last control-path step as one-element DEVICE tensors (f32 0 / 1; f64 norm of the
        unscaled gradient before clipping), or ``(None, None)`` before the first one.  Copies made on the device: reading
        them later (``.item()`` at a logging interval) is the caller's synchronisation, this call forces none."""
        if self._ctl is None:
            return None, None
        return ops.step_ctl_field(self._ctl, "found_inf").clone(), ops.step_ctl_field(self._ctl, "grad_norm").clone()


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD(momentum, nesterov, weight_decay) semantics (dampening 0) over the engine's flat buffers."""

    _entry, _n_state = "sodt_sgd_ema_step", 1

    def __init__(self, params, model, lr: float = 0.01, momentum: float = 0.937, weight_decay: float = 0.0,
                 nesterov: bool = True, ema: Optional[ModelEMA] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov), model, ema,
                         max_grad_norm, skip_nonfinite)

    @property
    def _mom(self):
        return None if self._state is None else self._state[0]

    def _check_groups(self):
        if len({bool(g["nesterov"]) for g in self.param_groups}) != 1:
            raise ValueError("FusedSGD: nesterov must be the same for every group")

    def _launch_step(self, eng, ema_flat, cast, grad_scale, ema_decay):
        gs = self.param_groups
        ops.sgd_ema_step(eng.flat_param, eng.flat_grad, self._mom, ema_flat, cast, self._groups,
                         [g["lr"] for g in gs], [g["momentum"] for g in gs], [g["weight_decay"] for g in gs],
                         gs[0]["nesterov"], grad_scale, ema_decay)

    def _launch_step_ctl(self, eng, ema_flat, cast, ctl, ema_decay):
        gs = self.param_groups
        ops.sgd_ema_step_ctl(eng.flat_param, eng.flat_grad, self._mom, ema_flat, cast, self._groups,
                             [g["lr"] for g in gs], [g["momentum"] for g in gs], [g["weight_decay"] for g in gs],
                             gs[0]["nesterov"], ctl, ema_decay)

    def state_dict(self):
        sd = super().state_dict()
        sd["momentum_flat"] = None if self._mom is None else self._mom.clone()
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)                       # the caller's dict keeps its "momentum_flat" entry
        mom = sd.pop("momentum_flat", None)
        super().load_state_dict(sd)
        if mom is not None:
            self._bind()
            self._mom.copy_(mom.to(self._mom.device))


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam (``decoupled=False``: weight decay added to the gradient, what Train.py:148 builds under --adam) or
    torch.optim.AdamW (``decoupled=True``) semantics over the engine's flat buffers, ``amsgrad=False``.  ``lr``, ``betas``,
    ``eps`` and ``weight_decay`` are read per group at every step.  One step counter serves every parameter: they all step
    together, and a step without gradients advances nothing, as torch leaves ``state['step']`` of such parameters alone.
    On the control path the counter lives in the device record and advances only when the step is applied, so the step after
    a skipped one takes the bias correction of t, not t + 1; ``_step`` (and ``state_dict()['step']``) read it back, which
    synchronises - at checkpoint time, not in the loop."""

    _entry, _n_state = "sodt_adam_ema_step", 2

    def __init__(self, params, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, decoupled: bool = False, ema: Optional[ModelEMA] = None,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False):
        if amsgrad:
            raise NotImplementedError("FusedAdam: amsgrad=True is not built (the reference never sets it)")
        if not eps > 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), model, ema, max_grad_norm,
                         skip_nonfinite)
        self.decoupled = bool(decoupled)
        self._step_host = 0        # the count as the host knows it; stale while _step_on_device
        self._step_on_device = False

    @property
    def _step(self) -> int:
        if self._step_on_device:            # control-path steps advanced (or skipped) on the device since the last read
            self._step_host = int(ops.step_ctl_field(self._ctl, "step").item())
            self._step_on_device = False
        return self._step_host

    @_step.setter
    def _step(self, v: int):
        self._step_host, self._step_on_device = int(v), False
        if self._ctl is not None:
            ops.step_ctl_field(self._ctl, "step").fill_(int(v))

    def _ctl_record(self, eng):
        if self._ctl is None or self._ctl.device != eng.flat_grad.device:
            self._ctl = ops.new_step_ctl(eng.flat_grad.device, self._step)
        return self._ctl

    def _launch_step_ctl(self, eng, ema_flat, cast, ctl, ema_decay):
        gs = self.param_groups
        ops.adam_ema_step_ctl(eng.flat_param, eng.flat_grad, self._state[0], self._state[1], ema_flat, cast, self._groups,
                              [g["lr"] for g in gs], [g["betas"] for g in gs], [g["eps"] for g in gs],
                              [g["weight_decay"] for g in gs], self.decoupled, ctl, ema_decay)
        self._step_on_device = True

    def _launch_step(self, eng, ema_flat, cast, grad_scale, ema_decay):
        gs = self.param_groups
        ops.adam_ema_step(eng.flat_param, eng.flat_grad, self._state[0], self._state[1], ema_flat, cast, self._groups,
                          [g["lr"] for g in gs], [g["betas"] for g in gs], [g["eps"] for g in gs],
                          [g["weight_decay"] for g in gs], self.decoupled, self._step + 1, grad_scale, ema_decay)
        self._step += 1                     # (after the launch: a refused one, e.g. a group's eps set to 0, is not a step)

    def state_dict(self):
        sd = super().state_dict()
        bound = self._state is not None
        sd["exp_avg_flat"] = self._state[0].clone() if bound else None
        sd["exp_avg_sq_flat"] = self._state[1].clone() if bound else None
        sd["step"] = self._step
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)                       # the caller's dict keeps its entries
        m, v, step = sd.pop("exp_avg_flat", None), sd.pop("exp_avg_sq_flat", None), sd.pop("step", 0)
        super().load_state_dict(sd)
        self._step = int(step)
        if m is not None and v is not None:
            self._bind()
            self._state[0].copy_(m.to(self._state[0].device))
            self._state[1].copy_(v.to(self._state[1].device))


class FusedSAM(torch.optim.Optimizer):
    """Sharpness-aware minimisation (basics/utils/sam.py: ``SAM.first_step`` / ``second_step`` / ``step(closure)``) around
    ``FusedSGD`` or ``FusedAdam``, over the engine's flat buffers (csrc/sam.hip).  The constructor mirrors the reference's,
    with the model the fused optimizers need::

        FusedSAM(params, base_optimizer, model, rho=0.05, adaptive=False, **kwargs)

    ``base_optimizer`` is the CLASS; it is built on this optimizer's ``param_groups`` with ``**kwargs`` (``lr``, ``momentum``,
    ``ema=``, ``max_grad_norm=``, ``skip_nonfinite=`` ...), and the groups are shared: ``rho`` and ``adaptive`` are per-group
    keys read at every call, next to the base's own.

    ``first_step`` is two launches - ``sodt_sam_norm`` (the f64 norm of the owned gradient and a not-finite flag, left in a
    device record) and ``sodt_sam_perturb`` (``old_p = p``, ``p += e_w``, the run-dtype mirror of the moved ``p``) - and
    ``second_step`` is ``sodt_sam_restore`` followed by the base optimizer's unchanged ``step()``.  Where the reference
    re-points ``p.data`` at a clone, the restore copies into the flat buffer, so the parameters stay the views the engine
    checks for.  Nothing on the way reads the device.

    Deviations from the reference: the norm is accumulated in float64 over the flat buffer (the reference: one float32 norm per
    tensor and a float32 norm of those), and a first gradient that is not finite leaves the weights unperturbed (the
    reference writes NaN into every weight and restores it afterwards); ``sam_info()`` reports the flag.

    With a ``GradScaler``: ``scaler.scale(loss).backward(); opt.first_step(zero_grad=True, scaler=scaler);
    scaler.scale(loss2).backward(); scaler.step(opt); scaler.update()`` - the closure-less ``step()`` acts as ``second_step()``
    when a first step is pending, and the scale / found-inf tensors ``GradScaler.step`` sets go through to the base."""

    _step_supports_amp_scaling = True

    def __init__(self, params, base_optimizer, model, rho: float = 0.05, adaptive: bool = False, **kwargs):
        if not rho >= 0.0:
            raise ValueError(f"Invalid rho, should be non-negative: {rho}")
        if not (isinstance(base_optimizer, type) and issubclass(base_optimizer, _FusedOptimizer)):
            raise TypeError("FusedSAM: base_optimizer is the class FusedSGD or FusedAdam")
        super().__init__(params, dict(rho=rho, adaptive=adaptive))
        self.base_optimizer = base_optimizer(self.param_groups, model, **kwargs)
        self.param_groups = self.base_optimizer.param_groups
        self.defaults.update(self.base_optimizer.defaults)
        self.model = model
        self._rec = None           # the device record of sodt_sam_norm (ops.new_sam_rec), made at the first first_step
        self._old = None           # old_p: scratch of the flat parameters' layout, never saved
        self._pending = None       # (engine, chunk -> group map) of a first_step whose second_step has not run

    def _hyp(self):
        rho, adaptive = [float(g["rho"]) for g in self.param_groups], [bool(g["adaptive"]) for g in self.param_groups]
        if not all(r >= 0.0 for r in rho):
            raise ValueError(f"Invalid rho, should be non-negative: {rho}")
        return rho, adaptive

    @torch.no_grad()
    def first_step(self, zero_grad: bool = False, scaler=None):
        base = self.base_optimizer
        rho, adaptive = self._hyp()
        scale = None
        if scaler is not None and scaler.is_enabled():
            scale = scaler._scale            # the device tensor; get_scale() would synchronise
            if scale is None:
                raise RuntimeError("FusedSAM.first_step: the GradScaler has no scale yet (scaler.scale(loss).backward() comes first)")
        if self._pending is not None:
            raise RuntimeError("FusedSAM.first_step: the previous first_step has not been followed by second_step / step")
        eng = base._bind()
        eng._check_param_views()
        if eng._claim_grads():              # no backward since zero_grad(set_to_none=True): nothing to climb along, nothing pending
            # _FusedOptimizer.step keeps the views it has just claimed and zeroes the buffer under them.  Here the views are handed
            # back instead, so that the base step that follows also sees that no backward ran and skips (with the views kept it
            # would step on a zero gradient: decay and momentum would move the weights).  The buffer needs no zeroing then:
            # nothing reads it before the next backward claims the views afresh, and that backward zeroes it first.
            for _, p, _, ptr in eng._claim:
                if p.grad is not None and p.grad.data_ptr() == ptr:
                    p.grad = None
            return
        dev = eng.flat_param.device
        if self._rec is None or self._rec.device != dev:
            self._rec = ops.new_sam_rec(dev)
        if self._old is None or self._old.shape != eng.flat_param.shape or self._old.device != dev:
            self._old = torch.empty_like(eng.flat_param)
        cast = next(iter(eng.flat_cast.values())) if eng.flat_cast else None
        # the perturbation writes the mirror of the chunks it owns only: the mirror is whole afterwards if it was whole before
        whole = cast is not None and eng.param_cast_fresh and eng._cast_version == eng.params_version()
        ops.sam_norm(eng.flat_param if any(adaptive) else None, eng.flat_grad, base._groups, adaptive, self._rec, scale)
        ops.sam_perturb(eng.flat_param, eng.flat_grad, self._old, cast, base._groups, rho, adaptive, self._rec)
        self._pending = (eng, base._groups)
        if whole:
            eng.mark_cast_fresh()
        else:
            eng.invalidate_params()
        if zero_grad:
            self.zero_grad(set_to_none=True)      # the weight-gradient kernels accumulate: the second backward starts from zero

    @torch.no_grad()
    def second_step(self, zero_grad: bool = False):
        base = self.base_optimizer
        if self._pending is not None:
            eng, groups = self._pending
            self._pending = None
            eng._check_param_views()
            ops.sam_restore(eng.flat_param, self._old, groups)
            eng.invalidate_params()         # (the base step rewrites the mirror and marks it fresh; a step without gradients does not)
        amp = {k: getattr(self, k) for k in ("grad_scale", "found_inf") if hasattr(self, k)}     # set by GradScaler.step
        for k, v in amp.items():
            setattr(base, k, v)
        try:
            base.step()
        finally:
            for k in amp:
                delattr(base, k)
        if zero_grad:
            self.zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is None:
            if self._pending is None:
                raise RuntimeError("Sharpness Aware Minimization requires closure, but it was not provided")
            self.second_step()
            return None
        self.first_step(zero_grad=True)
        with torch.enable_grad():           # (step() itself runs under no_grad; the closure's forward and backward must not)
            closure()
        self.second_step()
        return None

    def sam_info(self):
        """``(found, norm)`` of the last ``first_step`` as one-element DEVICE tensors (f32 0 / 1: the gradient was not finite and
        the weights were left unperturbed; f64 norm of the unscaled gradient, weighted by |p| in adaptive groups), or
        ``(None, None)`` before the first one.  Copies made on the device; this call forces no synchronisation."""
        if self._rec is None:
            return None, None
        return ops.sam_rec_field(self._rec, "found").clone(), ops.sam_rec_field(self._rec, "norm").clone()

    def last_step_info(self):
        return self.base_optimizer.last_step_info()

    def state_dict(self):
        return self.base_optimizer.state_dict()          # (rho / adaptive ride in the shared param_groups; old_p is scratch)

    def load_state_dict(self, sd):
        self.base_optimizer.load_state_dict(sd)
        self.param_groups = self.base_optimizer.param_groups
