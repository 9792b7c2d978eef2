"""Synchronised BatchNorm through the real engine: two gloo ranks on ONE GPU (the pattern and the model of tests/test_ddp_gpu.py)
with ddp.attach(average=False) and ddp.convert_sync_batchnorm run two images each; a model without a reducer runs the same four
images as one batch.  With the loss pred[0].float().square().sum() the two must agree on both steps - the first records the
plans and issues the statistics collectives inline, the second replays them in segments around the collectives:

* pred of a rank = its half of the whole batch's pred,
* flat_grad (the SUM over the ranks) = the whole batch's gradient,
* every BatchNorm's running statistics = the whole batch's, and the same bits on both ranks.

The gate is tests/test_ddp_gpu.py's: 2e-4 of max |reference|.  The same two ranks WITHOUT the flag must miss that gate on pred:
per-rank statistics are what the test exists to catch.

One rank, and no reducer at all: with the flag set the recorded launch lists are those of a run without it, name for name, and
ddp.GradReducer.all_reduce_stats is never called.

Three processes use the GPU at most (this one and the two ranks).  Every rank reports in a `finally`, the group's collectives
time out after 120 s, the parent waits with timeouts, terminates what is still alive and starts nothing afterwards.
"""
import importlib
import os
import traceback
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_ddp_gpu import PKG, _build, _free_port

pytestmark = pytest.mark.gpu
GATE = 2e-4
STEPS = 2


def _four_images(dev):
    g = torch.Generator().manual_seed(1234)
    return torch.rand(4, 3, 128, 128, generator=g).to(dev), torch.rand(4, 3, 128, 128, generator=g).to(dev)


def _running(model):
    return {n: b.detach().clone() for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))}


def _steps(model, x, ir):
    """[(pred, flat_grad, running statistics)] of STEPS training steps without an optimizer (the weights stay; the running
    statistics move on)"""
    out = []
    for _ in range(STEPS):
        for p in model.parameters():
            p.grad = None
        pred, _ = model(x, ir, "RGB+IR")
        pred[0].float().square().sum().backward()
        torch.cuda.synchronize()
        out.append((pred[0].detach().float().clone(), model._get_engine().flat_grad.clone(), _running(model)))
    return out


def _rel(got, want):
    return float((got.double() - want.double()).abs().max()) / max(float(want.double().abs().max()), 1e-30)


def _count_calls(red):
    """counts the calls of red.all_reduce_stats (the feature's one collective call site)"""
    calls = []
    inner = red.all_reduce_stats

    def counted(t):
        calls.append(tuple(t.shape))
        return inner(t)
    red.all_reduce_stats = counted
    return calls


def _worker(rank, world, port, q):
    res = {"rank": rank, "error": "did not finish"}
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
        ddp = importlib.import_module(PKG + ".ddp")
        x, ir = _four_images(dev)
        want = _steps(_build(dev), x, ir)                        # no reducer: one process, the four images as one batch
        mine = slice(2 * rank, 2 * rank + 2)
        for flag in (True, False):
            model = _build(dev)
            ddp.attach(model, average=False)
            if flag:
                assert ddp.convert_sync_batchnorm(model) is model
            calls = _count_calls(model.grad_reducer)
            got = _steps(model, x[mine], ir[mine])
            key = "sync" if flag else "local"
            res[key + ".pred"] = [_rel(g[0], w[0][mine]) for g, w in zip(got, want)]
            res[key + ".grad"] = [_rel(g[1], w[1]) for g, w in zip(got, want)]
            res[key + ".running"] = [max(_rel(g[2][n], w[2][n]) for n in w[2]) for g, w in zip(got, want)]
            res[key + ".calls"] = len(calls)
            if flag:
                plan = next(iter(model._get_engine().plans.values()))
                res["marks"] = (len(plan.bn_marks), len(plan.sbn_fwd), len(plan.sbn_bwd), len(plan.bwd_marks))
                # small, and as bytes (no tensor handle crosses the queue): compared between the ranks, bit for bit
                res["stats"] = {n: t.cpu().numpy().tobytes() for n, t in got[-1][2].items()}
                res["nbn"] = len(want[0][2]) // 2
        res["error"] = ""
    except BaseException:
        res["error"] = traceback.format_exc()
    finally:
        q.put(res)
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_match_the_whole_batch():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = []
    try:
        for _ in ps:
            res.append(q.get(timeout=420))
            if res[-1]["error"]:
                break                                            # the other rank would wait in a collective: do not wait for it
    finally:
        for p in ps:
            p.join(30 if len(res) == len(ps) and not any(r["error"] for r in res) else 1)
        for p in ps:
            if p.is_alive():
                p.terminate()
    assert len(res) == 2 and not any(r["error"] for r in res), [r["error"] for r in res]
    res.sort(key=lambda r: r["rank"])
    for r in res:
        print({k: v for k, v in r.items() if k != "stats"})
    for r in res:
        nbn = r["nbn"]
        assert nbn == 12 and r["marks"] == (nbn, nbn, nbn, 2), r["marks"]
        assert r["sync.calls"] == STEPS * 2 * nbn and r["local.calls"] == 0, (r["sync.calls"], r["local.calls"])
        for what in ("pred", "grad", "running"):
            assert all(e < GATE for e in r["sync." + what]), (what, r["sync." + what])
        # the check has teeth: statistics over the rank's own two images miss the same gate
        assert all(e >= GATE for e in r["local.pred"]), r["local.pred"]
    a, b = res[0]["stats"], res[1]["stats"]
    assert a.keys() == b.keys() and all(a[n] == b[n] for n in a), "the ranks' running statistics differ"


def _recorded_names(model, dev):
    x, ir = _four_images(dev)
    for p in model.parameters():
        p.grad = None
    pred, _ = model(x[:2], ir[:2], "RGB+IR")
    pred[0].float().square().sum().backward()
    torch.cuda.synchronize()
    plans = list(model._get_engine().plans.values())
    assert len(plans) == 1
    plan = plans[0]
    assert not plan.sbn_fwd and not plan.sbn_bwd
    return [c[2] for c in plan.fwd_main], [c[2] for c in plan.bwd_main]


def test_one_rank_and_no_reducer_run_as_without_the_flag(dev, monkeypatch):
    ddp = importlib.import_module(PKG + ".ddp")
    calls = []
    monkeypatch.setattr(ddp.GradReducer, "all_reduce_stats", lambda self, t: calls.append(tuple(t.shape)))
    plain = _recorded_names(_build(dev), dev)
    assert "sodt_bn_silu_bwd_apply" in plain[1] and "sodt_bn_finalize" in plain[0]
    # the flag with no reducer at all (what an EMA copy is)
    model = ddp.convert_sync_batchnorm(_build(dev))
    assert _recorded_names(model, dev) == plain
    assert model._get_engine().sync_bn is True and model._get_engine()._sbn_on is False
    # the flag under a group of one rank; setting it on a model that has run drops its plans and records the same lists again
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            timeout=timedelta(seconds=120))
    try:
        model = ddp.attach(_build(dev), average=False)
        assert _recorded_names(model, dev) == plain
        ddp.convert_sync_batchnorm(model)
        assert _recorded_names(model, dev) == plain
        assert model._get_engine().sync_bn is True and model._get_engine()._sbn_on is False
    finally:
        dist.destroy_process_group()
    assert not calls, calls
