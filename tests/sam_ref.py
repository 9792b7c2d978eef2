"""basics/utils/sam.py restated, for the tests of optim.FusedSAM and for tools/mb_optim.py --sam.

Two forms of the same arithmetic:

``Sam64``        float64, one tensor at a time, around torch.optim.SGD(nesterov, dampening 0) or torch.optim.Adam (weight decay
                 added to the gradient, amsgrad off): what tests/golden/sam.pt pins against the reference's own class run on
                 float64 tensors (tests/test_sam_host.py), and what the GPU tests hold the kernels against.
``PerTensorSAM`` the reference's loop on the parameters as they are (float32, on their device): one norm per tensor, a stack and
                 a norm of norms, one clone and one add_ per tensor.  It differs from the reference in one line: second_step
                 copies old_p back INTO p (``p.copy_(old_p)``) where the reference re-points ``p.data`` at the clone, which
                 would take the parameter out of the engine's flat buffer.

A group is a dict with ``rho``, ``adaptive`` and the base optimizer's keys (``lr``, ``weight_decay``, ``momentum`` / ``betas``,
``eps``)."""
import torch


def split(flat, sizes):
    """the tensors tests/golden/sam.pt stores end to end"""
    return [t.clone() for t in torch.split(flat, list(sizes))]


def grad_norm(ps, gs, group_of, groups):
    """sam.py:49-59 in the dtype of its inputs: the norm of the per-tensor norms of (|p| if adaptive else 1) * g."""
    return torch.stack([((p.abs() if groups[k]["adaptive"] else 1.0) * g).norm(p=2) for p, g, k in zip(ps, gs, group_of)]).norm(p=2)


def e_w(p, g, grp, norm):
    """sam.py:18-24: (p^2 if adaptive else 1) * g * rho / (norm + 1e-12)"""
    return (p * p if grp["adaptive"] else 1.0) * g * (grp["rho"] / (norm + 1e-12))


class Sam64:
    def __init__(self, kind, params, group_of, groups):
        assert kind in ("sgd", "adam")
        self.kind, self.group_of, self.groups = kind, list(group_of), [dict(g) for g in groups]
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = 0
        self.old = None

    def first_step(self, grads, inv_scale=1.0):
        """returns the norm; self.p is w + e(w) afterwards"""
        g = [x.detach().double().cpu() * inv_scale for x in grads]
        norm = grad_norm(self.p, g, self.group_of, self.groups)
        self.old = [p.clone() for p in self.p]
        self.p = [p + e_w(p, gi, self.groups[k], norm) for p, gi, k in zip(self.p, g, self.group_of)]
        return norm

    def second_step(self, grads, inv_scale=1.0):
        """back to w, then the base optimizer's step with the gradient taken at w + e(w)"""
        self.p, self.old = self.old, None
        self.base_step(grads, inv_scale)

    def base_step(self, grads, inv_scale=1.0):
        self.t += 1
        for i, (p, g, k) in enumerate(zip(self.p, grads, self.group_of)):
            h = self.groups[k]
            d = g.detach().double().cpu() * inv_scale + h["weight_decay"] * p
            if self.kind == "sgd":
                mu = h["momentum"]
                self.m[i] = mu * self.m[i] + d            # (the first step's "buf = d" is m = 0)
                self.p[i] = p - h["lr"] * (d + mu * self.m[i])
            else:
                b1, b2 = h["betas"]
                self.m[i] = self.m[i] + (1 - b1) * (d - self.m[i])
                self.v[i] = b2 * self.v[i] + (1 - b2) * d * d
                denom = self.v[i].sqrt() / (1 - b2 ** self.t) ** 0.5 + h["eps"]
                self.p[i] = p - (h["lr"] / (1 - b1 ** self.t)) * self.m[i] / denom


class PerTensorSAM:
    """The reference's per-tensor loop around any optimizer with ``param_groups`` whose groups carry ``rho`` / ``adaptive``."""

    def __init__(self, base):
        self.base = base
        self.old = {}

    @torch.no_grad()
    def first_step(self, zero_grad=False):
        owned = [(g, p) for g in self.base.param_groups for p in g["params"] if p.grad is not None]
        # one norm per tensor, then the norm of those (float32 on float32 parameters, in this order: the host test holds the bits)
        per_tensor = [torch.linalg.vector_norm(p.abs() * p.grad if g["adaptive"] else p.grad) for g, p in owned]
        norm = torch.linalg.vector_norm(torch.stack(per_tensor))
        for g, p in owned:
            step = g["rho"] / (norm + 1e-12)
            self.old[p] = p.detach().clone()
            p.add_((p * p * p.grad if g["adaptive"] else p.grad) * step)
        if zero_grad:
            self.base.zero_grad()
        return norm

    @torch.no_grad()
    def restore(self):
        for g in self.base.param_groups:
            for p in g["params"]:
                if p in self.old:
                    p.copy_(self.old[p])          # (the reference: p.data = old_p)

    def second_step(self, zero_grad=False):
        self.restore()
        self.base.step()
        if zero_grad:
            self.base.zero_grad()
