"""Hold the BatchNorm running statistics still for SAM's second forward (the role of basics/utils/bypass_bn.py).

A SAM step runs two forward passes over the same batch, the second one at the perturbed weights ``w + e(w)``.  Only the
first should move ``running_mean`` / ``running_var``: ``disable_running_stats(model)`` before the second forward sets every
batch-norm layer's ``momentum`` to 0 after noting what it was, ``enable_running_stats(model)`` afterwards puts it back.  The
engine reads each ``Conv``'s ``bn.momentum`` at every training forward (Engine._conv_fwd), so with momentum 0 the running
statistics come back bit for bit while the batch statistics still normalise the activations::

    def closure():
        disable_running_stats(model)
        loss = compute_loss(model(imgs, irs, 'RGB+IR')[0], targets)[0]
        loss.backward()
        enable_running_stats(model)
    optimizer.step(closure)                 # optim.FusedSAM
"""
from torch.nn.modules.batchnorm import _BatchNorm

_KEPT = "backup_momentum"       # the attribute the reference keeps the value under: a model that went through either is restored by both


def _batch_norms(model):
    return [m for m in model.modules() if isinstance(m, _BatchNorm)]


def disable_running_stats(model):
    """Set every batch-norm layer's momentum to 0, remembering the current value.  Calling it twice in a row keeps the value
    of the first call (the reference would remember the 0)."""
    for m in _batch_norms(model):
        if not (m.momentum == 0 and hasattr(m, _KEPT)):
            setattr(m, _KEPT, m.momentum)
        m.momentum = 0


def enable_running_stats(model):
    """Give every batch-norm layer that disable_running_stats touched its momentum back."""
    for m in _batch_norms(model):
        if hasattr(m, _KEPT):
            m.momentum = getattr(m, _KEPT)
