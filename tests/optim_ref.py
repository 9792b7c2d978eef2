"""The fused optimizer steps of csrc/optim.hip restated, with the error an honest float32 evaluation may make.

``sgd64`` / ``adam64``  include/sodt_hip.h's formulas for sodt_sgd_ema_step / sodt_adam_ema_step in float64 over whole flat buffers.
                        ``elem_group`` (the chunk map repeated four times; all zeros for a null map) picks the hyper-parameters:
                        a byte below 4 is trained, with slot 0's hyper-parameters when it is not below ngroups (the launchers fill
                        the unused slots of their 4-entry tables from slot 0); any other byte keeps p, m and v.  The EMA runs on
                        every element, on the new p.  Constants enter as the kernel receives them: the SGD tables, grad_scale and
                        ema_decay rounded to float32; Adam's 1 - b1, b2, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t), eps, wd and
                        1 - lr * wd formed in double and then rounded; 1 - ema_decay formed from the float32 ema_decay.
                        ``exact=True`` keeps every constant in double (the comparison with torch.optim on float64 tensors).
``sgd32`` / ``adam32``  the same statements, one float32 torch op per operation, nothing fused.
``*_bound``             per-element absolute bounds on p', m', v', e' (below).
``grad_stats64``        every documented field of sodt_step_ctl after a sodt_grad_stats call.
``cases`` / ``stats_cases``  the case matrices the host and the GPU test share; ``build`` / ``build_stats`` make a case's buffers.
``SGD_MUTANTS`` / ``ADAM_MUTANTS``  wrong statements of the two references, by name (``mutant=``).

The bound.  First order, one u = 2^-24 per rounding of an UNFUSED float32 evaluation (a fused multiply-add rounds once where
this counts twice), evaluated in float64 from the reference's own intermediate magnitudes, s = grad_scale:

  SGD    E_d = u (|wd p| + |g s| + |d|)
         E_m = u |mu m| + E_d + u |m'|
         E_u = E_d + |mu| E_m + u |mu m'| + u |u|                       (nesterov; otherwise E_u = E_m)
         E_p = |lr| E_u + u |lr u| + u |p'|
  Adam   E_d as above (wd = 0 in the decoupled form)
         E_t = E_d + u |d - m|
         E_m = |1-b1| E_t + u |(1-b1)(d-m)| + u |m'|
         E_v = 2 |(1-b2) d| E_d + 3u |(1-b2) d^2| + u |b2 v| + u |v'|
         r_v = E_v / v' (0 where v' = 0);  E_sq = (r_v / 2 + u) sqrt(v')
         E_den = (E_sq + 2u sqrt(v')) / sbc2 + u den                    den = sqrt(v') / sbc2 + eps
         E_q = E_m / den + |m'| E_den / den^2 + u |q|                   q = m' / den
         E_p = u |p dm| + step E_q + 2u |step q| + u |p'|               dm = 1 - lr wd (decoupled) or 1
         (the second u on step and on sbc2 pays for the _ctl kernel forming them on the device: its b^t by squaring may land
         one float32 away from the host's pow)
  EMA    E_e = u |e a| + u |(1-a) p'| + |1-a| E_p + u |e'|

enlarged by SLACK = 1 + 2^-6 for the second-order terms and by nothing else.  An element that is not trained has E_p = E_m =
E_v = 0.  No constant here comes from a kernel or from a measurement."""
import math

import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -6

SGD_MUTANTS = ("no_weight_decay", "dampening", "no_nesterov", "decoupled_decay", "ema_on_old_p", "group_plus1_mod4",
               "group_plus1_modng")
ADAM_MUTANTS = ("t_plus_1", "omb2_from_f32_b2", "omb1_from_f32_b1", "no_sqrt_bc2", "coupled_decoupled_swapped", "eps_in_sqrt",
                "group_plus1_mod4", "group_plus1_modng")


def f32(x):
    """the float32 nearest to the Python float x, as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float64).float())


def _slots(vals, ng):
    """the 4-entry table sgd_launch / adam_launch build: the unused slots repeat slot 0"""
    return [float(vals[i if i < ng else 0]) for i in range(4)]


def _group_index(elem_group, ng, mutant):
    k = elem_group.clamp(max=3)
    if mutant == "group_plus1_mod4":
        k = (k + 1) % 4
    elif mutant == "group_plus1_modng":
        k = (torch.where(k < ng, k, torch.zeros_like(k)) + 1) % ng
    return k


def _ema(e, p1, Ep, a, oma, dt, want_bound):
    e1 = e * a + oma * p1
    if not want_bound:
        return e1, None
    return e1, U * (e * a).abs() + U * (oma * p1).abs() + abs(oma) * Ep + U * e1.abs()


def _sgd(p, g, m, e, elem_group, hyp, dt, exact=False, mutant=None):
    ng = len(hyp["lr"])
    R = (lambda x: float(x)) if exact else f32
    own = elem_group < 4
    k = _group_index(elem_group, ng, mutant)
    tab = lambda name: torch.tensor([R(x) for x in _slots(hyp[name], ng)], dtype=torch.float64).to(dt)[k]
    lr, mu, wd = tab("lr"), tab("momentum"), tab("wd")
    s = R(hyp.get("grad_scale", 1.0))
    p, m = p.to(dt), m.to(dt)
    g = torch.where(own, g.to(dt), torch.zeros((), dtype=dt))
    coupled_wd = torch.zeros_like(wd) if mutant in ("no_weight_decay", "decoupled_decay") else wd
    wdp, gs = coupled_wd * p, g * s
    d = wdp + gs
    mum = mu * m
    m1 = mum + (d * (1 - mu) if mutant == "dampening" else d)
    nesterov = bool(hyp["nesterov"]) and mutant != "no_nesterov"
    if nesterov:
        mum1 = mu * m1
        u = d + mum1
    else:
        u = m1
    lru = lr * u
    p1 = (p * (1 - lr * wd) if mutant == "decoupled_decay" else p) - lru
    out = {"p": torch.where(own, p1, p), "m": torch.where(own, m1, m)}
    bound = None
    if dt == torch.float64:
        Ed = U * (wdp.abs() + gs.abs() + d.abs())
        Em = U * mum.abs() + Ed + U * m1.abs()
        Eu = Ed + mu.abs() * Em + U * mum1.abs() + U * u.abs() if nesterov else Em
        Ep = lr.abs() * Eu + U * lru.abs() + U * p1.abs()
        zero = torch.zeros_like(Ep)
        bound = {"p": torch.where(own, Ep, zero), "m": torch.where(own, Em, zero)}
    if e is not None and hyp.get("ema_decay") is not None:
        a = R(hyp["ema_decay"])
        oma = 1.0 - a if exact else f32(1.0 - a)
        src = p if mutant == "ema_on_old_p" else out["p"]
        out["e"], Ee = _ema(e.to(dt), src, bound["p"] if bound else None, a, oma, dt, bound is not None)
        if bound is not None:
            bound["e"] = Ee
    if bound is not None:
        bound = {k_: v * SLACK for k_, v in bound.items()}
    return out, bound


def adam_constants(hyp, exact=False, mutant=None):
    """per table slot, what adam_launch hands the kernel: step = lr / (1 - b1^t), omb1, b2, omb2, sbc2, eps, wd, dm"""
    ng = len(hyp["lr"])
    R = (lambda x: float(x)) if exact else f32
    t = int(hyp["t"]) + (1 if mutant == "t_plus_1" else 0)
    decoupled = bool(hyp["decoupled"]) != (mutant == "coupled_decoupled_swapped")
    lr, b1, b2, eps, wd = (_slots(hyp[n], ng) for n in ("lr", "b1", "b2", "eps", "wd"))
    c = {n: [] for n in ("step", "omb1", "b2", "omb2", "sbc2", "eps", "wd", "dm")}
    for j in range(4):
        c["step"].append(R(lr[j] / (1.0 - math.pow(b1[j], t))))
        c["omb1"].append(R(1.0 - (f32(b1[j]) if mutant == "omb1_from_f32_b1" else b1[j])))
        c["b2"].append(R(b2[j]))
        c["omb2"].append(R(1.0 - (f32(b2[j]) if mutant == "omb2_from_f32_b2" else b2[j])))
        c["sbc2"].append(1.0 if mutant == "no_sqrt_bc2" else R(math.sqrt(1.0 - math.pow(b2[j], t))))
        c["eps"].append(R(eps[j]))
        c["wd"].append(0.0 if decoupled else R(wd[j]))
        c["dm"].append(R(1.0 - lr[j] * wd[j]) if decoupled else 1.0)
    return c


def _adam(p, g, m, v, e, elem_group, hyp, dt, exact=False, mutant=None):
    ng = len(hyp["lr"])
    R = (lambda x: float(x)) if exact else f32
    own = elem_group < 4
    k = _group_index(elem_group, ng, mutant)
    c = {n: torch.tensor(x, dtype=torch.float64).to(dt)[k] for n, x in adam_constants(hyp, exact, mutant).items()}
    s = R(hyp.get("grad_scale", 1.0))
    p, m, v = p.to(dt), m.to(dt), v.to(dt)
    g = torch.where(own, g.to(dt), torch.zeros((), dtype=dt))
    wdp, gs = c["wd"] * p, g * s
    d = wdp + gs
    dmm = d - m
    x = c["omb1"] * dmm
    m1 = m + x
    y = c["omb2"] * d * d
    bv = c["b2"] * v
    v1 = bv + y
    if mutant == "eps_in_sqrt":
        sq = (v1 / (c["sbc2"] * c["sbc2"]) + c["eps"]).sqrt()
        den = sq
    else:
        sq = v1.sqrt()
        den = sq / c["sbc2"] + c["eps"]
    q = m1 / den
    pdm, sq_ = p * c["dm"], c["step"] * q
    p1 = pdm - sq_
    out = {"p": torch.where(own, p1, p), "m": torch.where(own, m1, m), "v": torch.where(own, v1, v)}
    bound = None
    if dt == torch.float64:
        Ed = U * (wdp.abs() + gs.abs() + d.abs())
        Et = Ed + U * dmm.abs()
        Em = c["omb1"].abs() * Et + U * x.abs() + U * m1.abs()
        Ev = 2 * (c["omb2"] * d).abs() * Ed + 3 * U * y.abs() + U * bv.abs() + U * v1.abs()
        rv = torch.where(v1 > 0, Ev / v1.clamp(min=1e-300), torch.zeros_like(v1))
        Esq = (rv / 2 + U) * sq
        Eden = (Esq + 2 * U * sq) / c["sbc2"] + U * den
        Eq = Em / den + m1.abs() * Eden / (den * den) + U * q.abs()
        Ep = U * pdm.abs() + c["step"] * Eq + 2 * U * sq_.abs() + U * p1.abs()
        zero = torch.zeros_like(Ep)
        bound = {"p": torch.where(own, Ep, zero), "m": torch.where(own, Em, zero), "v": torch.where(own, Ev, zero)}
    if e is not None and hyp.get("ema_decay") is not None:
        a = R(hyp["ema_decay"])
        oma = 1.0 - a if exact else f32(1.0 - a)
        out["e"], Ee = _ema(e.to(dt), out["p"], bound["p"] if bound else None, a, oma, dt, bound is not None)
        if bound is not None:
            bound["e"] = Ee
    if bound is not None:
        bound = {k_: b * SLACK for k_, b in bound.items()}
    return out, bound


def sgd64(p, g, m, e, elem_group, hyp, exact=False, mutant=None):
    return _sgd(p, g, m, e, elem_group, hyp, torch.float64, exact, mutant)[0]


def sgd_bound(p, g, m, e, elem_group, hyp):
    return _sgd(p, g, m, e, elem_group, hyp, torch.float64)[1]


def sgd32(p, g, m, e, elem_group, hyp):
    return _sgd(p, g, m, e, elem_group, hyp, torch.float32)[0]


def adam64(p, g, m, v, e, elem_group, hyp, exact=False, mutant=None):
    return _adam(p, g, m, v, e, elem_group, hyp, torch.float64, exact, mutant)[0]


def adam_bound(p, g, m, v, e, elem_group, hyp):
    return _adam(p, g, m, v, e, elem_group, hyp, torch.float64)[1]


def adam32(p, g, m, v, e, elem_group, hyp):
    return _adam(p, g, m, v, e, elem_group, hyp, torch.float32)[0]


def ref_and_bound(kind, b, hyp, mutant=None):
    """(float64 outputs, bounds) of one case's buffers `b` (build()); the bounds are those of the unmutated statement"""
    if kind == "sgd":
        return sgd64(b["p"], b["g"], b["m"], b["e"], b["elem_group"], hyp, mutant=mutant), \
            sgd_bound(b["p"], b["g"], b["m"], b["e"], b["elem_group"], hyp)
    return adam64(b["p"], b["g"], b["m"], b["v"], b["e"], b["elem_group"], hyp, mutant=mutant), \
        adam_bound(b["p"], b["g"], b["m"], b["v"], b["e"], b["elem_group"], hyp)


def f32_arm(kind, b, hyp):
    if kind == "sgd":
        return sgd32(b["p"], b["g"], b["m"], b["e"], b["elem_group"], hyp)
    return adam32(b["p"], b["g"], b["m"], b["v"], b["e"], b["elem_group"], hyp)


def worst_ratio(got, ref, bound, sel=None):
    """(largest error / bound over the elements, how many are outside); a zero bound asks for equality"""
    err = (got.double().cpu() - ref).abs()
    if sel is not None:
        err, bound = err[sel], bound[sel]
    if err.numel() == 0:
        return 0.0, 0
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                           torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    return float(ratio.max()), int((ratio > 1.0).sum())


def grad_stats64(g, elem_group, scale, found_in, grad_scale, max_norm, skip_nonfinite, step0):
    """sodt_step_ctl after sodt_grad_stats(g, map, scale, found_in, grad_scale, max_norm, skip_nonfinite) on a record whose step
    was step0.  g as stored (float32), scale / found_in the values of the one-element device tensors or None, max_norm None or
    a float (<= 0: no clipping)."""
    own = elem_group < 4
    go = g.double()[own]
    sumsq = float((go * go).sum())
    found = bool((~torch.isfinite(go)).any()) or (found_in is not None and float(found_in) != 0.0)
    inv_scale = 1.0 if scale is None else f32(1.0 / f32(scale))          # GradScaler: scale.double().reciprocal().float()
    mul = inv_scale * f32(grad_scale)
    norm = math.sqrt(sumsq) * abs(mul) if sumsq == sumsq and sumsq >= 0 else float("nan")
    coef = 1.0
    if max_norm is not None and f32(max_norm) > 0.0:
        coef = f32(max_norm) / (norm + 1e-6)                             # clip_grad_norm_
        if coef > 1.0:
            coef = 1.0
    skip = int(found and bool(skip_nonfinite))
    return {"sumsq": sumsq, "grad_norm": norm, "step": int(step0) + (0 if skip else 1), "found_inf": 1.0 if found else 0.0,
            "inv_scale_eff": mul * coef, "clip_coef": coef, "skip": skip}


# ---- the case matrix ------------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 1025)                       # chunks: one lane, a block less / exactly / plus one chunk, five blocks
NG = {1: 1, 255: 3, 256: 4, 257: 2, 1025: 4}           # ngroups, rotated over the sizes
SGD_HYP = {"lr": (0.01, 0.0032, 0.02, 0.0007), "momentum": (0.937, 0.8, 0.0, 0.5), "wd": (0.0, 5e-4, 1e-3, 3e-4)}
ADAM_HYP = {"lr": (1e-3, 3e-4, 2e-3, 5e-4), "b1": (0.9, 0.99, 0.0, 0.937), "b2": (0.999, 0.99, 0.95, 0.9999),
            "eps": (1e-8, 1e-6, 1e-7, 1e-5), "wd": (0.0, 5e-4, 1e-2, 1e-3)}
ADAM_T = (1, 2, 7, 1000, 10 ** 6)
GRAD_SCALES = (1.0, 1.0 / 65536, 0.37)
EMA_DECAYS = (0.9999, 0.5, 0.0, None)                  # None: no EMA buffer
MIRRORS = ("bf16", "f32", None)


def cases():
    """Every size with both layouts; SGD with nesterov on and off, Adam coupled and decoupled; t, grad_scale, ema_decay and the
    mirror rotate over the cases so that every value of each meets every size class."""
    out, i = [], 0
    for kind, flag in (("sgd", "nesterov"), ("adam", "decoupled")):
        for on in (True, False):
            for nchunk in SIZES:
                for layout in ("null", "mixed"):
                    ng = NG[nchunk]
                    hyp = {n: list(v[:ng]) for n, v in (SGD_HYP if kind == "sgd" else ADAM_HYP).items()}
                    hyp[flag] = on
                    hyp["grad_scale"] = GRAD_SCALES[i % 3]
                    hyp["ema_decay"] = EMA_DECAYS[(i // 3) % 4]
                    if kind == "adam":
                        hyp["t"] = ADAM_T[(i // 2) % 5]
                    name = f"{kind}-{flag if on else 'no_' + flag}-{nchunk}-{layout}"
                    out.append({"name": name, "kind": kind, "nchunk": nchunk, "layout": layout, "ng": ng, "hyp": hyp,
                                "mirror": MIRRORS[(i // 4) % 3], "seed": 7919 * i + nchunk})
                    i += 1
    return out


def gmap(nchunk, ng, layout, gen):
    """None (every chunk is group 0), or groups 0..ng-1 with chunks marked 255 at both ends and interleaved"""
    if layout == "null":
        return None
    m = torch.randint(0, ng, (nchunk,), generator=gen).to(torch.uint8)
    if nchunk == 1:
        m[0] = ng - 1
        return m
    m[torch.rand(nchunk, generator=gen) < 0.25] = 255
    m[:2] = 255
    m[-3:] = 255
    for k in range(ng):                                 # (every group owns at least one chunk)
        m[2 + k] = k
    m[nchunk // 2] = ng - 1
    return m


def _zeros(x, gen, frac=0.03):
    x[torch.rand(x.numel(), generator=gen) < frac] = 0.0
    return x


def build(case, nchunk=None, gm="layout"):
    """The float32 CPU buffers of a case: p, g, m, v, e, the chunk map (uint8 or None) and elem_group.  Per group the scale of p
    puts lr * |update| between 1e-3 and 1 of |p| for most elements; |g * grad_scale| is log-uniform over 1e-3..10 (g is stored
    divided by grad_scale); m ~ 0.1 N(0,1), v the square of such a draw; each holds exact zeros, 1 % of the elements in all of
    them together.  The gradient of every chunk that is not trained holds NaN, +inf and -inf."""
    kind, hyp, ng = case["kind"], case["hyp"], case["ng"]
    nchunk = case["nchunk"] if nchunk is None else nchunk
    gen = torch.Generator().manual_seed(case["seed"])
    n = 4 * nchunk
    if isinstance(gm, str):
        gm = gmap(nchunk, ng, case["layout"], gen)
    eg = torch.zeros(n, dtype=torch.long) if gm is None else gm.long().repeat_interleave(4)
    own = eg < 4
    lr = torch.tensor(_slots(hyp["lr"], ng), dtype=torch.float64)[eg.clamp(max=3)]
    p = (torch.randn(n, generator=gen, dtype=torch.float64) * lr * (10.0 if kind == "sgd" else 30.0)).float()
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 4.0 - 3.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g = (mag * sign / f32(hyp["grad_scale"])).float()
    m = (0.1 * torch.randn(n, generator=gen)).float()
    v = (0.1 * torch.randn(n, generator=gen)).float().square()
    e = (p.double() * (1.0 + 0.05 * torch.randn(n, generator=gen, dtype=torch.float64))).float()
    for x in (p, g, m, v):
        _zeros(x, gen)
    allz = torch.rand(n, generator=gen) < 0.01
    for x in (p, g, m, v):
        x[allz] = 0.0
    un = torch.nonzero(~own).flatten()
    g[un[0::2]] = float("nan")
    g[un[1::4]] = float("inf")
    g[un[3::4]] = float("-inf")
    return {"p": p, "g": g, "m": m, "v": v, "e": e, "gmap": gm, "elem_group": eg, "own": own, "n": n}


STATS_SIZES = (1, 255, 256, 257, 1023, 1024, 1025)
STATS_LARGE = 1048576 + 262144 + 3                     # a second trip of the four-chunk loop, with a ragged tail


def stats_cases():
    """sodt_grad_stats: every size with both layouts, the arguments rotating over them.  max_norm is a factor of the float64
    norm (None: no clipping); bad = (value, where) puts one non-finite value into the first / last owned chunk, 'tail' (the last
    owned chunk of the large size: the tail trip) or 'unowned' (a chunk that is not owned: not found)."""
    scales = (None, 65536.0, 3.0)
    gscales = (0.5, -0.5)
    maxn = (None, 0.5, 1.0, 2.0)
    bads = (None, (float("nan"), "first"), (float("inf"), "last"), None, None, (float("nan"), "unowned"), (float("-inf"), "first"),
            None)
    out, i = [], 0
    for nchunk in STATS_SIZES + (STATS_LARGE,):
        for layout in ("null", "mixed"):
            bad = bads[i % 8]
            if nchunk == STATS_LARGE:
                bad = None if layout == "null" else (float("-inf"), "tail")
            out.append({"name": f"stats-{nchunk}-{layout}", "nchunk": nchunk, "layout": layout, "scale": scales[i % 3],
                        "grad_scale": gscales[(i // 3) % 2], "max_norm": maxn[(i // 2) % 4], "bad": bad,
                        "found_in": 1.0 if i % 7 == 4 else (0.0 if i % 2 else None), "skip_nonfinite": 1,
                        "step0": 41 if i % 5 == 3 else 0, "seed": 104729 + 31 * i})
            i += 1
    out.append(dict(out[-1], name=f"stats-{STATS_LARGE}-mixed-finite", bad=None, scale=65536.0, max_norm=0.5, seed=out[-1]["seed"] + 1))
    return out


def stats_max_norm(case, g, elem_group):
    """the case's max_norm as the float32 the entry takes: its factor times the float64 norm of the finite owned gradient after
    unscaling (None: no clipping)"""
    if case["max_norm"] is None:
        return None
    go = g.double()[(elem_group < 4).to(g.device)]
    go = go[torch.isfinite(go)]
    inv = 1.0 if case["scale"] is None else f32(1.0 / case["scale"])
    return f32(case["max_norm"] * math.sqrt(float((go * go).sum())) * abs(inv * f32(case["grad_scale"])))


def build_stats(case, dev="cpu"):
    """(g float32 with norm about |grad_scale| after unscaling, chunk map or None, elem_group): built on `dev` (the large size)"""
    gen = torch.Generator().manual_seed(case["seed"])
    nchunk = case["nchunk"]
    n = 4 * nchunk
    gm = None
    if case["layout"] == "mixed":
        gm = torch.randint(0, 4, (nchunk,), generator=gen).to(torch.uint8)
        if nchunk > 1:
            gm[torch.rand(nchunk, generator=gen) < 0.25] = 255
            gm[0], gm[-1] = 255, 255
            if nchunk > 2:
                gm[1], gm[-2] = 3, 2
    g = torch.randn(n, generator=gen) * ((case["scale"] or 1.0) / math.sqrt(n))
    eg = torch.zeros(n, dtype=torch.long) if gm is None else gm.long().repeat_interleave(4)
    own_chunks = torch.nonzero(eg[::4] < 4).flatten()
    if case["bad"] is not None and own_chunks.numel():
        value, where = case["bad"]
        if where == "unowned":
            un = torch.nonzero(eg >= 4).flatten()
            g[un[::3]] = value
        else:
            c = int(own_chunks[0] if where == "first" else own_chunks[-1])
            g[4 * c + (1 if where == "first" else 3)] = value
    return g.to(dev), (None if gm is None else gm.to(dev)), eg
