"""tests/optim_ref.py checked without a GPU: the float64 restatements of the fused optimizer steps are torch's optimizers, the
per-element bound holds for an unfused float32 evaluation of every case of the shared matrix, each named mutant of the
statements breaks it, and grad_stats64 is clip_grad_norm_ and GradScaler's unscale.  The GPU test
(tests/test_optim_kernels_gpu.py) holds the kernels of csrc/optim.hip to the same references and the same bound."""
import math

import pytest
import torch

import optim_ref as R


# ---- (a) the references are torch's optimizers ------------------------------------------------------------------------------
SIZES_A = (36, 8, 52, 20)                      # elements per group (multiples of four: one parameter each)


def _ema_loop(ema, params, d):
    """ModelEMA.update's loop (basics/utils/torch_utils.py:298-301)"""
    for v, p in zip(ema, params):
        v *= d
        v += (1.0 - d) * p.detach()


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


@pytest.mark.parametrize("ng", [3, 4])
@pytest.mark.parametrize("nesterov", [True, False])
def test_sgd64_is_torch_sgd_then_model_ema(ng, nesterov):
    gen = torch.Generator().manual_seed(100 + ng)
    params = [torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_() for n in SIZES_A[:ng]]
    groups = [{"params": [p], "lr": R.SGD_HYP["lr"][k], "momentum": R.SGD_HYP["momentum"][k], "weight_decay": R.SGD_HYP["wd"][k]}
              for k, p in enumerate(params)]
    opt = torch.optim.SGD(groups, lr=0.01, momentum=0.9, nesterov=nesterov, foreach=False)
    ema = [p.detach().clone() for p in params]
    eg = torch.cat([torch.full((n,), k, dtype=torch.long) for k, n in enumerate(SIZES_A[:ng])])
    p, m, e = _flat(params).clone(), torch.zeros(int(eg.numel()), dtype=torch.float64), _flat(ema).clone()
    for step in range(5):
        warm = (step + 1) / 5.0                              # Train.py's warm-up: lr and momentum move every iteration
        for k, grp in enumerate(opt.param_groups):
            grp["lr"] = R.SGD_HYP["lr"][k] * (0.1 + warm)
            grp["momentum"] = R.SGD_HYP["momentum"][k] * (0.85 + 0.1 * warm)
        hyp = {"lr": [g["lr"] for g in opt.param_groups], "momentum": [g["momentum"] for g in opt.param_groups],
               "wd": [g["weight_decay"] for g in opt.param_groups], "nesterov": nesterov, "grad_scale": 1.0,
               "ema_decay": 0.9999 * (1 - math.exp(-(step + 1) / 2000))}
        grads = [torch.randn(n, generator=gen, dtype=torch.float64) for n in SIZES_A[:ng]]
        for q, g in zip(params, grads):
            q.grad = g.clone()
        opt.step()
        _ema_loop(ema, params, hyp["ema_decay"])
        out = R.sgd64(p, _flat(grads), m, e, eg, hyp, exact=True)
        p, m, e = out["p"], out["m"], out["e"]
        tol = 1e-12 * float(_flat(params).abs().max())
        assert float((p - _flat(params)).abs().max()) <= tol, step
        assert float((e - _flat(ema)).abs().max()) <= tol, step
        for k, q in enumerate(params):                       # (torch keeps no buffer for a group whose momentum is 0)
            if opt.param_groups[k]["momentum"] != 0:
                assert float((m[eg == k] - opt.state[q]["momentum_buffer"]).abs().max()) <= tol, (step, k)


@pytest.mark.parametrize("ng", [3, 4])
@pytest.mark.parametrize("decoupled", [False, True])
def test_adam64_is_torch_adam_and_adamw_then_model_ema(ng, decoupled):
    gen = torch.Generator().manual_seed(200 + ng)
    params = [(0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).requires_grad_() for n in SIZES_A[:ng]]
    H = R.ADAM_HYP
    groups = [{"params": [p], "lr": H["lr"][k], "betas": (H["b1"][k], H["b2"][k]), "eps": H["eps"][k], "weight_decay": H["wd"][k]}
              for k, p in enumerate(params)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=1e-3, foreach=False)
    ema = [p.detach().clone() for p in params]
    eg = torch.cat([torch.full((n,), k, dtype=torch.long) for k, n in enumerate(SIZES_A[:ng])])
    n = int(eg.numel())
    p, m, v, e = _flat(params).clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), _flat(ema).clone()
    for step in range(5):
        for k, grp in enumerate(opt.param_groups):
            grp["lr"] = H["lr"][k] * (0.1 + (step + 1) / 5.0)
        hyp = {"lr": [g["lr"] for g in opt.param_groups], "b1": list(H["b1"][:ng]), "b2": list(H["b2"][:ng]),
               "eps": list(H["eps"][:ng]), "wd": list(H["wd"][:ng]), "decoupled": decoupled, "t": step + 1, "grad_scale": 1.0,
               "ema_decay": 0.9999 * (1 - math.exp(-(step + 1) / 2000))}
        grads = [torch.randn(k_, generator=gen, dtype=torch.float64) for k_ in SIZES_A[:ng]]
        for q, g in zip(params, grads):
            q.grad = g.clone()
        opt.step()
        _ema_loop(ema, params, hyp["ema_decay"])
        out = R.adam64(p, _flat(grads), m, v, e, eg, hyp, exact=True)
        p, m, v, e = out["p"], out["m"], out["v"], out["e"]
        tol = 1e-12 * float(_flat(params).abs().max())
        assert float((p - _flat(params)).abs().max()) <= tol, step
        assert float((e - _flat(ema)).abs().max()) <= tol, step
        assert float((m - _flat([opt.state[q]["exp_avg"] for q in params])).abs().max()) <= tol, step
        assert float((v - _flat([opt.state[q]["exp_avg_sq"] for q in params])).abs().max()) <= tol, step


# ---- the matrix itself ------------------------------------------------------------------------------------------------------
def test_matrix_covers_every_axis_and_the_inputs_are_as_described():
    cs = R.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    for kind in ("sgd", "adam"):
        mine = [c for c in cs if c["kind"] == kind]
        assert {c["nchunk"] for c in mine} == set(R.SIZES) and {c["layout"] for c in mine} == {"null", "mixed"}
        assert {c["ng"] for c in mine} == {1, 2, 3, 4}
        assert {c["hyp"]["grad_scale"] for c in mine} == set(R.GRAD_SCALES)
        assert {c["hyp"]["ema_decay"] for c in mine} == set(R.EMA_DECAYS)
        assert {c["mirror"] for c in mine} == set(R.MIRRORS)
    assert {(c["hyp"]["decoupled"], c["hyp"]["t"]) for c in cs if c["kind"] == "adam"} == {(d, t) for d in (True, False) for t in R.ADAM_T}
    assert {c["hyp"]["nesterov"] for c in cs if c["kind"] == "sgd"} == {True, False}
    assert 0.0 in R.SGD_HYP["momentum"] and 0.0 in R.ADAM_HYP["b1"] and 0.0 in R.SGD_HYP["wd"] and 0.0 in R.ADAM_HYP["wd"]
    for name in ("lr", "momentum", "wd"):
        assert len(set(R.SGD_HYP[name])) == 4
    for name in ("lr", "b1", "b2", "eps", "wd"):
        assert len(set(R.ADAM_HYP[name])) == 4
    tiny = 2.0 ** -126
    for c in cs:
        b = R.build(c)
        own = b["own"]
        assert bool(torch.isfinite(b["g"][own]).all())
        if c["nchunk"] > 1:
            if c["layout"] == "mixed":
                assert set(b["gmap"].tolist()) == set(range(c["ng"])) | {255}
                assert bool(torch.isnan(b["g"][~own]).any()) and bool(torch.isinf(b["g"][~own]).any())
            allz = (b["p"] == 0) & (b["g"] == 0) & (b["m"] == 0) & (b["v"] == 0)
            assert c["nchunk"] < 255 or bool((allz & own).any())
            for x in (b["p"], b["g"], b["m"], b["v"]):
                assert bool((x[own] == 0).any()) and bool((x[own] != 0).any())
        ref, _ = R.ref_and_bound(c["kind"], b, c["hyp"])
        for x in list(ref.values()) + [b["p"], b["g"], b["m"], b["v"], b["e"]]:      # nothing in the float32 denormal range
            x = x[own].abs()
            assert not bool(((x > 0) & (x < tiny)).any()), c["name"]
    for c in cs:                                              # lr * |update| against |p|: between 1e-3 and 1 for most elements
        if c["nchunk"] < 255:
            continue
        b = R.build(c)
        ref, _ = R.ref_and_bound(c["kind"], b, c["hyp"])
        sel = b["own"] & (b["p"] != 0)
        rel = ((ref["p"] - b["p"].double()).abs() / b["p"].double().abs())[sel]
        frac = float(((rel >= 1e-3) & (rel <= 1.0)).float().mean())
        assert frac > 0.5, (c["name"], frac)


# ---- (b) the bound holds for float32 ----------------------------------------------------------------------------------------
def test_float32_arm_is_inside_the_bound_on_every_element():
    worst = {}
    for c in R.cases():
        b = R.build(c)
        ref, bound = R.ref_and_bound(c["kind"], b, c["hyp"])
        got = R.f32_arm(c["kind"], b, c["hyp"])
        assert set(got) == set(ref) == set(bound)
        for name in ref:
            ratio, out = R.worst_ratio(got[name], ref[name], bound[name])
            key = (c["kind"], name)
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert out == 0 and ratio <= 1.0, (c["name"], name, ratio, out)
            un = ~b["own"]
            if name != "e":
                assert torch.equal(got[name][un], b[name][un]) and torch.equal(ref[name][un], b[name][un].double())
    for key, ratio in sorted(worst.items()):
        print(f"float32 arm, {key[0]} {key[1]}': worst error / bound {ratio:.3f}")


# ---- (c) the bound bites ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mutant", [("sgd", m) for m in R.SGD_MUTANTS] + [("adam", m) for m in R.ADAM_MUTANTS])
def test_every_mutant_leaves_the_bound(kind, mutant):
    best = (0, None, None)
    caught = 0
    for c in R.cases():
        if c["kind"] != kind:
            continue
        b = R.build(c)
        got, bound = R.ref_and_bound(kind, b, c["hyp"], mutant=mutant)
        ref, _ = R.ref_and_bound(kind, b, c["hyp"])
        hit = False
        for name in ref:
            _, out = R.worst_ratio(got[name], ref[name], bound[name], sel=b["own"])
            hit |= out >= 10
            if out > best[0]:
                best = (out, name, c["name"])
        caught += hit
    print(f"mutant {kind}/{mutant}: caught in {caught} cases; most in {best[2]}: {best[0]} owned elements of {best[1]}' outside the bound")
    assert best[0] >= 10, (mutant, best)


# ---- (d) grad_stats64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.stats_cases() if c["nchunk"] != R.STATS_LARGE], ids=lambda c: c["name"])
def test_grad_stats64_is_clip_grad_norm_and_the_scaler_unscale(case):
    g, gm, eg = R.build_stats(case)
    max_norm = R.stats_max_norm(case, g, eg)
    st = R.grad_stats64(g, eg, case["scale"], case["found_in"], case["grad_scale"], max_norm, case["skip_nonfinite"], case["step0"])
    own = eg < 4
    bad_owned = case["bad"] is not None and case["bad"][1] != "unowned"
    found = bad_owned or (case["found_in"] or 0.0) != 0.0
    assert st["found_inf"] == float(found) and st["skip"] == int(found) and st["step"] == case["step0"] + (0 if found else 1)
    if bad_owned:
        return
    # GradScaler._unscale_grads_: inv_scale = scale.double().reciprocal().float(), grads multiplied by it
    inv_scale = 1.0 if case["scale"] is None else float(torch.tensor(case["scale"]).double().reciprocal().float())
    unscaled = g.double()[own] * inv_scale * R.f32(case["grad_scale"])
    params = [torch.zeros_like(t).requires_grad_() for t in torch.split(unscaled, 8)]
    for q, t in zip(params, torch.split(unscaled, 8)):
        q.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm if max_norm is not None else float("inf"), foreach=False)
    assert abs(st["grad_norm"] - float(total)) <= 1e-12 * float(total)
    assert abs(st["sumsq"] - float((g.double()[own] ** 2).sum())) <= 1e-12 * st["sumsq"]
    clipped = torch.cat([q.grad for q in params])
    mine = g.double()[own] * st["inv_scale_eff"]
    assert float((mine - clipped).abs().max()) <= 1e-12 * float(clipped.abs().max())
    if case["max_norm"] is None or case["max_norm"] == 2.0:
        assert st["clip_coef"] == 1.0
    elif case["max_norm"] == 1.0:
        assert 1.0 - 1e-5 < st["clip_coef"] < 1.0                  # just below 1: the + 1e-6
    else:
        assert abs(st["clip_coef"] - 0.5) < 1e-5
    assert (st["inv_scale_eff"] < 0) == (case["grad_scale"] < 0) and st["grad_norm"] > 0


def test_stats_matrix_covers_what_it_says():
    cs = R.stats_cases()
    assert {c["nchunk"] for c in cs} == set(R.STATS_SIZES) | {R.STATS_LARGE}
    assert {c["scale"] for c in cs} == {None, 65536.0, 3.0} and {c["grad_scale"] for c in cs} == {0.5, -0.5}
    clean = [c for c in cs if c["bad"] is None and not c["found_in"]]
    assert {c["max_norm"] for c in clean} == {None, 0.5, 1.0, 2.0}
    assert {c["bad"][1] for c in cs if c["bad"]} == {"first", "last", "tail", "unowned"}
    assert any(c["found_in"] == 1.0 and c["bad"] is None for c in cs) and any(c["step0"] == 41 for c in cs)
    vals = [c["bad"][0] for c in cs if c["bad"]]
    assert any(math.isnan(x) for x in vals) and float("inf") in vals and float("-inf") in vals
