"""engine.Plan on the CPU: the buffer cache refuses a name reused with another shape or dtype, the zero pools hand out 256-byte
aligned views, and every attribute the engine sets later exists from the start."""
import importlib
import inspect
import re

import pytest
import torch

E = importlib.import_module("small-object-detection-transformers_amd.engine")
BF, F32 = torch.bfloat16, torch.float32


def _plan():
    return E.Plan(2, 128, BF, True, torch.device("cpu"))


def test_buf_same_request_same_tensor():
    plan = _plan()
    a = plan.buf("x", (4, 6))
    assert a.dtype == BF and tuple(a.shape) == (4, 6) and plan.buf("x", (4, 6)) is a and plan.buf("x", [4, 6], BF) is a
    z = plan.buf("z", (3,), F32, zero=True)
    assert z.dtype == F32 and not z.any() and plan.buf("z", (3,), F32) is z
    assert set(plan.bufs) == {"x", "z"}


@pytest.mark.parametrize("shape,dtype", [((4, 7), None), ((24,), None), ((6, 4), None), ((4, 6), F32)])
def test_buf_other_shape_or_dtype_raises(shape, dtype):
    plan = _plan()
    plan.buf("x", (4, 6))
    with pytest.raises(RuntimeError, match="plan buffer 'x'"):
        plan.buf("x", shape, dtype)


def test_scratch_is_named_by_kind_and_shape():
    plan = _plan()
    a = plan.scratch("dxn", (2048, 192))
    assert plan.scratch("dxn", (2048, 192)) is a and plan.bufs["g.dxn.2048x192"] is a
    b = plan.scratch("dxn", (512, 384))                     # another shape: another buffer, never the first one back
    assert b is not a and tuple(b.shape) == (512, 384) and plan.bufs["g.dxn.512x384"] is b
    assert plan.scratch("dbt", (12, 225), F32, zero=True).dtype == F32


def test_zbuf_carves_aligned_views_of_one_pool():
    plan = _plan()
    a = plan.zbuf("f", "a", (3, 5), torch.float64)          # 120 bytes: the next view starts at 256
    b = plan.zbuf("f", "b", (2, 64), F32)                   # 512 bytes
    c = plan.zbuf("f", "c", (1,), F32)
    pool = plan.zpool("f")
    assert pool.dtype == torch.uint8 and pool.numel() == 1 << 21
    assert [t.data_ptr() - pool.data_ptr() for t in (a, b, c)] == [0, 256, 768] and plan.zused["f"] == 1024
    assert a.dtype == torch.float64 and tuple(a.shape) == (3, 5) and tuple(b.shape) == (2, 64)
    assert plan.zbuf("f", "a", (3, 5), torch.float64) is a and plan.zused["f"] == 1024
    b.fill_(1.0)
    pool.zero_()                                            # the single memset of a forward clears every accumulator
    assert not b.any()
    with pytest.raises(RuntimeError, match="plan buffer 'a'"):
        plan.zbuf("f", "a", (3, 5), F32)
    with pytest.raises(RuntimeError, match="plan buffer 'a'"):
        plan.zbuf("f", "a", (5, 3), torch.float64)
    d = plan.zbuf("b", "d", (4,), F32)                      # the backward's pool is another tensor
    assert d.data_ptr() == plan.zpool("b").data_ptr() and plan.zused == {"f": 1024, "b": 256}


def test_zbuf_exhaustion():
    plan = _plan()
    plan.zbuf("b", "big", ((1 << 21) - 256,), torch.uint8)
    plan.zbuf("b", "last", (256,), torch.uint8)
    with pytest.raises(RuntimeError, match="zero pool exhausted"):
        plan.zbuf("b", "over", (1,), torch.uint8)


def test_every_attribute_exists_after_init():
    plan = _plan()
    assert (plan.B, plan.S, plan.dt, plan.training, plan.dev) == (2, 128, BF, True, torch.device("cpu"))
    assert plan.bufs == {} and plan.saved == {} and plan.graphs == {} and plan.zused == {} and plan.bwd_marks == [] and plan.gen == 0
    for name in ("fwd_pre", "fwd_main", "bwd_main", "sr", "enc_bwd_start", "enc_gin"):
        assert getattr(plan, name) is None, name
    src = inspect.getsource(E)                              # whatever the engine assigns on a plan is declared by __init__
    assigned = set(re.findall(r"\bplan\.(\w+)\s*=[^=]", src)) | set(re.findall(r"\bplan\.(\w+)\s*\+=", src))
    assert assigned and assigned <= set(vars(plan)), assigned - set(vars(plan))
