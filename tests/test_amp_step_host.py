"""Host-side checks of the optimizers' control path (no GPU): the _ctl steps take the plain steps' arguments with one record
pointer; the ctypes record matches the layout the header documents; the constructors refuse a max_grad_norm that
is not positive; both optimizers tell torch.amp.GradScaler that they take its scale and found-inf tensors themselves; Adam's
step count travels in state_dict(); the entries refuse null or misaligned control pointers before anything is launched."""
import ctypes as C
import importlib
import os
import re
import types

import pytest
import torch

PKG = "small-object-detection-transformers_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_control_entries_declared_exported_and_bound(pkg):
    L = pkg._lib                    # (declared, exported, bound type for type: tests/test_abi_and_host.py, for every entry)
    # the _ctl steps are the plain ones with (grad_scale) / (step, grad_scale) replaced by one record pointer
    sgd, sgd_c = L.SIGNATURES["sodt_sgd_ema_step"], L.SIGNATURES["sodt_sgd_ema_step_ctl"]
    assert len(sgd) == 16 and sgd_c[:13] + sgd_c[14:] == sgd[:13] + sgd[14:] and sgd_c[13] is C.c_void_p
    adam, adam_c = L.SIGNATURES["sodt_adam_ema_step"], L.SIGNATURES["sodt_adam_ema_step_ctl"]
    assert len(adam) == 20 and adam_c[:16] + adam_c[17:] == adam[:16] + adam[18:] and adam_c[16] is C.c_void_p


def test_control_record_layout_matches_the_header(pkg):
    L = pkg._lib
    hdr = open(os.path.join(ROOT, "include", "sodt_hip.h")).read()
    assert C.sizeof(L.StepCtl) == 64
    documented = dict(acc_sumsq=0, acc_found=8, ticket=12, sumsq=16, grad_norm=24, step=32, found_inf=40, inv_scale_eff=44,
                      clip_coef=48, skip=52, reserved=56)
    for name, off in documented.items():
        assert getattr(L.StepCtl, name).offset == off, name
        assert re.search(rf"\b{off}\s+[\w ]+?\s+{name}\b", hdr), f"offset {off} of {name} is not documented in the header"


class _FakeEngine:
    """Just enough of engine.Engine for _bind on the CPU: two parameters in a flat buffer."""

    def __init__(self):
        self.flat_param = torch.zeros(16)
        self.dev = torch.device("cpu")
        self.params = {"w": torch.nn.Parameter(self.flat_param[0:8].view(2, 4)), "b": torch.nn.Parameter(self.flat_param[8:10])}
        self.grad_order = ["w", "b"]
        self.grad_offsets = {"w": 0, "b": 8}


def _fake_model():
    eng = _FakeEngine()
    return types.SimpleNamespace(_get_engine=lambda: eng), eng


@pytest.mark.parametrize("cls", ["FusedSGD", "FusedAdam"])
def test_constructors_take_the_control_options_and_refuse_a_bad_norm(cls):
    O = importlib.import_module(PKG + ".optim")
    model, eng = _fake_model()
    ctor = getattr(O, cls)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            ctor(list(eng.params.values()), model=model, max_grad_norm=bad)
    opt = ctor(list(eng.params.values()), model=model)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False          # both off by default
    assert opt.last_step_info() == (None, None)
    opt = ctor(list(eng.params.values()), model=model, max_grad_norm=10, skip_nonfinite=True)
    assert opt.max_grad_norm == 10.0 and opt.skip_nonfinite is True
    # torch.amp.GradScaler.step reads this attribute to decide whether it unscales and reads found_inf on the host itself
    assert getattr(opt, "_step_supports_amp_scaling", False) is True


def test_adam_state_dict_carries_the_step_with_control_options():
    O = importlib.import_module(PKG + ".optim")
    model, eng = _fake_model()
    opt = O.FusedAdam(list(eng.params.values()), model=model, max_grad_norm=1.0, skip_nonfinite=True)
    opt._bind()
    sd = opt.state_dict()
    assert sd["step"] == 0 and opt._step == 0
    sd["step"] = 11
    opt2 = O.FusedAdam(list(eng.params.values()), model=model, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert opt2._step == 11 and opt2.state_dict()["step"] == 11
    # a record that exists follows the host's writes of the counter (resume), and is what _step reads after device-side steps
    ops = importlib.import_module(PKG + ".ops")
    opt2._ctl = ops.new_step_ctl(torch.device("cpu"), opt2._step)
    assert int(ops.step_ctl_field(opt2._ctl, "step")) == 11
    opt2._step = 5
    assert int(ops.step_ctl_field(opt2._ctl, "step")) == 5
    ops.step_ctl_field(opt2._ctl, "step").fill_(6)        # what an applied control-path step does on the device
    opt2._step_on_device = True
    assert opt2._step == 6 and opt2.state_dict()["step"] == 6


def test_entries_refuse_null_and_misaligned_control_pointers(pkg):
    """Argument checks come before any launch, so they can be exercised with host memory and no device."""
    L = pkg._lib
    lib = L.load()
    n = 64
    bufs = [(C.c_float * (n + 8))() for _ in range(5)]
    base = [(C.addressof(b) + 15) & ~15 for b in bufs]            # 16-byte aligned starts
    p, g, m, v = base[:4]
    ctl_buf = (C.c_char * 96)()
    ctl = (C.addressof(ctl_buf) + 15) & ~15
    f3, d3 = (C.c_float * 4)(0.01, 0.01, 0.01, 0.01), lambda x: (C.c_double * 4)(x, x, x, x)

    def stats(gp=g, cp=ctl, nel=n, scale=None, found=None, gs=1.0, mx=0.0):
        return lib.sodt_grad_stats(gp, None, nel, scale, found, C.c_float(gs), C.c_float(mx), 1, cp, None)

    def sgd(cp):
        return lib.sodt_sgd_ema_step_ctl(p, g, m, None, None, L.F32, None, n, 1, f3, f3, f3, 1, cp, C.c_float(0.0), None)

    def adam(cp):
        return lib.sodt_adam_ema_step_ctl(p, g, m, v, None, None, L.F32, None, n, 1, d3(1e-3), d3(0.9), d3(0.999), d3(1e-8),
                                          d3(0.0), 0, cp, C.c_float(0.0), None)
    for rc in (stats(cp=None), stats(cp=ctl + 8), stats(gp=None), stats(gp=g + 4), stats(nel=n + 2), stats(scale=base[4] + 2),
               stats(found=base[4] + 1), stats(gs=float("nan")), stats(mx=float("nan")),
               sgd(None), sgd(ctl + 4), sgd(ctl + 8), adam(None), adam(ctl + 8)):
        assert rc != 0
    common = open(os.path.join(ROOT, "include", "sodt_hip.h")).read()
    einval = int(re.search(r"#define\s+SODT_EINVAL\s+(-?\d+)", common).group(1))
    assert stats(cp=None) == einval and sgd(ctl + 8) == einval and adam(None) == einval
