"""The five C entries of csrc/optim.hip (sodt_sgd_ema_step, sodt_adam_ema_step, sodt_grad_stats, sodt_sgd_ema_step_ctl,
sodt_adam_ema_step_ctl) called directly on flat buffers, element by element against the float64 restatement and the derived
per-element bound of tests/optim_ref.py (the bound's derivation is that module's docstring; tests/test_optim_ref_host.py shows
that it holds for unfused float32 arithmetic and that fifteen wrong formulas break it).  The optimizer state (the SGD momentum,
exp_avg, exp_avg_sq) is read back and gated like p and the EMA.  No element is excluded anywhere.

Every buffer (p, g, m, v, e, the mirror, the map) is carved out of a larger sentinel-filled one with 64 elements of guard on
either side; the gradient of every chunk that is not trained holds NaN, +inf and -inf.  After every call the guards and g are
bit for bit what they were, chunks that are not trained keep their p, m and v bits, and - this entry's contract, unlike SAM's -
they DO get the EMA and the cast of their unchanged p.

sodt_grad_stats: sumsq within n * 2^-53 relative of the float64 sum over the owned elements (n float64 additions in any
order), grad_norm within (n / 2 + 4) * 2^-53 (the square root halves it; the product with |grad_scale / scale|, the root and
their roundings are the 4), clip_coef and inv_scale_eff within one float32 ulp of the float64 formula rounded to float32,
found_inf, skip and step exact.

Map bytes: a byte below 4 is trained (with group 0's hyper-parameters when it is not below ngroups), every other byte is what
255 is, for the step kernels and for sodt_grad_stats alike."""
import ctypes as C
import math

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
SENT = -7776.0                             # (exact in bfloat16 too)
PAD = 64                                   # elements of sentinel on either side of every carved buffer
MAP_SENT = 0x5A
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.float64: torch.int64}


def _carve(dev, n, dtype=torch.float32, fill=SENT):
    big = torch.full((n + 2 * PAD,), fill, device=dev, dtype=dtype)
    return big, big[PAD: PAD + n]


def _same_bits(a, b):
    return torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


class _Bufs:
    """a case's buffers on the device, carved; `start` keeps what they held before the call"""

    def __init__(self, dev, b, mirror):
        self.n, self.own, self.b = b["n"], b["own"].to(dev), b
        self.big, self.t = {}, {}
        for name in ("p", "g", "m", "v", "e"):
            self.big[name], self.t[name] = _carve(dev, self.n)
            self.t[name].copy_(b[name].to(dev))
        self.mirror = None
        if mirror is not None:
            self.big["mirror"], self.mirror = _carve(dev, self.n, torch.bfloat16 if mirror == "bf16" else torch.float32)
        self.gmap = None
        if b["gmap"] is not None:
            self.big["gmap"], self.gmap = _carve(dev, self.n // 4, torch.uint8, MAP_SENT)
            self.gmap.copy_(b["gmap"].to(dev))
        self.start = {k: v.clone() for k, v in self.big.items()}

    def check_untouched(self, ema_ran, skipped=False):
        """guards; g and the map bit for bit; p, m, v of the chunks that are not trained (of every chunk, after a skipped step);
        e when no EMA buffer went down; the mirror is the cast of p everywhere"""
        for name, big in self.big.items():
            was = self.start[name]
            assert _same_bits(big[:PAD], was[:PAD]) and _same_bits(big[-PAD:], was[-PAD:]), f"guard of {name}"
        assert _same_bits(self.big["g"], self.start["g"])
        if self.gmap is not None:
            assert torch.equal(self.big["gmap"], self.start["gmap"])
        keep = torch.ones_like(self.own) if skipped else ~self.own
        for name in ("p", "m", "v"):
            assert _same_bits(self.t[name][keep], self.start[name][PAD:-PAD][keep]), f"{name} of chunks that are not trained"
        if not ema_ran:
            assert _same_bits(self.big["e"], self.start["e"])
        if self.mirror is not None:
            want = self.t["p"].to(torch.bfloat16) if self.mirror.dtype == torch.bfloat16 else self.t["p"]
            assert _same_bits(self.mirror, want), "mirror"


def _gate(what, got, ref, bound):
    bad = []
    for name in sorted(ref):
        ratio, out = R.worst_ratio(got[name], ref[name], bound[name])
        print(f"{what} {name}': worst error / bound {ratio:.3f}, {out} of {ref[name].numel()} outside")
        if out or not ratio <= 1.0:
            bad.append((name, ratio, out))
    assert not bad, (what, bad)


def _run_plain(ops, case, B):
    kind, hyp = case["kind"], case["hyp"]
    e = B.t["e"] if hyp["ema_decay"] is not None else None
    a = hyp["ema_decay"] or 0.0
    if kind == "sgd":
        ops.sgd_ema_step(B.t["p"], B.t["g"], B.t["m"], e, B.mirror, B.gmap, hyp["lr"], hyp["momentum"], hyp["wd"], hyp["nesterov"],
                         hyp["grad_scale"], a)
    else:
        ops.adam_ema_step(B.t["p"], B.t["g"], B.t["m"], B.t["v"], e, B.mirror, B.gmap, hyp["lr"], list(zip(hyp["b1"], hyp["b2"])),
                          hyp["eps"], hyp["wd"], hyp["decoupled"], hyp["t"], hyp["grad_scale"], a)
    torch.cuda.synchronize()


def _run_ctl(ops, case, B, ctl):
    kind, hyp = case["kind"], case["hyp"]
    e = B.t["e"] if hyp["ema_decay"] is not None else None
    a = hyp["ema_decay"] or 0.0
    if kind == "sgd":
        ops.sgd_ema_step_ctl(B.t["p"], B.t["g"], B.t["m"], e, B.mirror, B.gmap, hyp["lr"], hyp["momentum"], hyp["wd"],
                             hyp["nesterov"], ctl, a)
    else:
        ops.adam_ema_step_ctl(B.t["p"], B.t["g"], B.t["m"], B.t["v"], e, B.mirror, B.gmap, hyp["lr"], list(zip(hyp["b1"], hyp["b2"])),
                              hyp["eps"], hyp["wd"], hyp["decoupled"], ctl, a)


def _outputs(case, B):
    names = ("p", "m") + (("v",) if case["kind"] == "adam" else ()) + (("e",) if case["hyp"]["ema_decay"] is not None else ())
    return {k: B.t[k] for k in names}


# ---- the plain entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c["name"])
def test_plain_step_against_float64(dev, ops, case):
    b = R.build(case)
    ref, bound = R.ref_and_bound(case["kind"], b, case["hyp"])
    B = _Bufs(dev, b, case["mirror"])
    _run_plain(ops, case, B)
    _gate(case["name"], _outputs(case, B), ref, bound)
    B.check_untouched(ema_ran=case["hyp"]["ema_decay"] is not None)
    if case["nchunk"] > 1:
        assert not torch.equal(B.t["p"][B.own], B.start["p"][PAD:-PAD][B.own])
    if case["hyp"]["ema_decay"] == 0.0:
        assert _same_bits(B.t["e"], B.t["p"])
    if case["hyp"]["ema_decay"] is not None and not bool(B.own.all()):      # the EMA reaches the chunks that are not trained
        assert not torch.equal(B.t["e"][~B.own], B.start["e"][PAD:-PAD][~B.own])
    if case["kind"] == "sgd":
        assert _same_bits(B.big["v"], B.start["v"])


# ---- the _ctl entries -------------------------------------------------------------------------------------------------------
def _ctl_case(kind, on, step0, clip):
    hyp = {n: list(v) for n, v in (R.SGD_HYP if kind == "sgd" else R.ADAM_HYP).items()}
    hyp["nesterov" if kind == "sgd" else "decoupled"] = on
    hyp["grad_scale"] = (0.5 if clip else 1.0) * 0.37 / 65536.0      # (about what the record will hold: build() sizes g by it)
    hyp["ema_decay"] = 0.9999
    hyp["t"] = step0 + 1
    return {"name": f"ctl-{kind}-{on}-{step0}", "kind": kind, "nchunk": 1025, "layout": "mixed", "ng": 4, "hyp": hyp,
            "mirror": "bf16", "seed": 31337 + step0 + (7 if on else 0)}


@pytest.mark.parametrize("kind,on,step0,clip", [("sgd", True, 0, True), ("sgd", False, 3, False), ("adam", False, 0, False),
                                                ("adam", True, 1, True), ("adam", False, 6, True)])
def test_ctl_step_applied_four_groups(dev, ops, kind, on, step0, clip):
    """the record is filled by sodt_grad_stats on the same stream; four groups with four distinct (lr, b1, b2) reach lanes 2, 3,
    6 and 7 of the Adam kernel's eight-lane shuffle"""
    case = _ctl_case(kind, on, step0, clip)
    b = R.build(case)
    assert set(b["gmap"].tolist()) == {0, 1, 2, 3, 255}
    B = _Bufs(dev, b, case["mirror"])
    scale = torch.full((1,), 65536.0, device=dev)
    free = R.grad_stats64(b["g"], b["elem_group"], 65536.0, None, 0.37, None, 1, step0)
    max_norm = R.f32(0.5 * free["grad_norm"]) if clip else None
    want = R.grad_stats64(b["g"], b["elem_group"], 65536.0, None, 0.37, max_norm, 1, step0)
    ctl = ops.new_step_ctl(dev, step0)
    ops.grad_stats(B.t["g"], B.gmap, ctl, scale, None, 0.37, max_norm, True)
    _run_ctl(ops, case, B, ctl)
    torch.cuda.synchronize()
    f = lambda name: ops.step_ctl_field(ctl, name).item()
    assert f("skip") == 0 and f("found_inf") == 0.0 and f("step") == step0 + 1
    s = float(f("inv_scale_eff"))
    assert abs(s - R.f32(want["inv_scale_eff"])) <= abs(s) * 2.0 ** -23
    case["hyp"]["grad_scale"], case["hyp"]["t"] = s, int(f("step"))
    ref, bound = R.ref_and_bound(kind, b, case["hyp"])
    _gate(case["name"], _outputs(case, B), ref, bound)
    B.check_untouched(ema_ran=True)
    for k in range(4):                                        # every group moved
        sel = (b["elem_group"] == k).to(dev)
        assert not torch.equal(B.t["p"][sel], B.start["p"][PAD:-PAD][sel])


@pytest.mark.parametrize("kind,step0", [("sgd", 0), ("adam", 0), ("adam", 5)])
def test_ctl_step_skipped(dev, ops, kind, step0):
    """inf in one owned gradient element: p, m, v bit for bit, the EMA moves on the unchanged p within E_e, the mirror is the cast
    of the unchanged p, step stays (0: the very first step skipped, the kernel's t < 1 clamp), nothing NaN anywhere"""
    case = _ctl_case(kind, True, step0, False)
    b = R.build(case)
    at = int(torch.nonzero(b["own"])[-1])
    b["g"][at] = float("inf")
    B = _Bufs(dev, b, case["mirror"])
    ctl = ops.new_step_ctl(dev, step0)
    ops.grad_stats(B.t["g"], B.gmap, ctl, torch.full((1,), 65536.0, device=dev), None, 0.37, None, True)
    _run_ctl(ops, case, B, ctl)
    torch.cuda.synchronize()
    f = lambda name: ops.step_ctl_field(ctl, name).item()
    assert f("skip") == 1 and f("found_inf") == 1.0 and f("step") == step0
    frozen = dict(b, elem_group=torch.full_like(b["elem_group"], 255))        # the reference of a step nobody takes
    ref, bound = R.ref_and_bound(kind, frozen, case["hyp"])
    assert float(bound["p"].max()) == 0.0
    _gate(case["name"] + " skipped", {"e": B.t["e"]}, {"e": ref["e"]}, {"e": bound["e"]})
    B.check_untouched(ema_ran=True, skipped=True)
    for name in ("p", "m", "v", "e"):
        assert bool(torch.isfinite(B.t[name]).all()), name
    assert bool(torch.isfinite(B.mirror.float()).all())


# ---- position independence: the grid-stride loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_one_launch_past_the_block_cap_equals_two_split_launches(dev, ops, kind):
    """2,097,152 + 257 chunks: just past 8192 blocks of 256, so some threads make a second trip.  Bit-identical in p, state, EMA
    and mirror to the same buffers processed in two launches split at an arbitrary chunk (a pure device comparison)."""
    nchunk, split = 2097152 + 257, 777778
    n = 4 * nchunk
    gen = torch.Generator(device=dev).manual_seed(5)
    gm = torch.randint(0, 4, (nchunk,), generator=gen, device=dev).to(torch.uint8)
    gm[torch.rand(nchunk, generator=gen, device=dev) < 0.25] = 255
    gm[:2], gm[-3:] = 255, 255
    p = torch.randn(n, generator=gen, device=dev) * 0.03
    g = torch.randn(n, generator=gen, device=dev)
    g[(gm == 255).repeat_interleave(4)] = float("nan")
    m = torch.randn(n, generator=gen, device=dev) * 0.1
    v = (torch.randn(n, generator=gen, device=dev) * 0.1).square()
    e = p * 1.01
    hyp = {k: list(x) for k, x in (R.SGD_HYP if kind == "sgd" else R.ADAM_HYP).items()}

    def run(lo, hi, bufs):
        s = slice(4 * lo, 4 * hi)
        P, M, V, E, Mi = (x[s] for x in bufs)
        if kind == "sgd":
            ops.sgd_ema_step(P, g[s], M, E, Mi, gm[lo:hi], hyp["lr"], hyp["momentum"], hyp["wd"], True, 0.37, 0.9999)
        else:
            ops.adam_ema_step(P, g[s], M, V, E, Mi, gm[lo:hi], hyp["lr"], list(zip(hyp["b1"], hyp["b2"])), hyp["eps"], hyp["wd"],
                              False, 7, 0.37, 0.9999)

    one = [p.clone(), m.clone(), v.clone(), e.clone(), torch.full((n,), SENT, device=dev, dtype=torch.bfloat16)]
    two = [x.clone() for x in one]
    run(0, nchunk, one)
    run(0, split, two)
    run(split, nchunk, two)
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "e", "mirror"), one, two):
        assert _same_bits(a, b), name
    assert not torch.equal(one[0], p) and not bool((one[4] == SENT).any())
    tail = slice(4 * 2097152, n)                                # the second trip did its work
    own_tail = (gm[2097152:] < 4).repeat_interleave(4)
    assert bool((one[0][tail][own_tail] != p[tail][own_tail]).any())


# ---- sodt_grad_stats --------------------------------------------------------------------------------------------------------
def _stats_call(dev, ops, g, gm, ctl, **kw):
    """g and the map carved: NaN guards around g and owned (0) guards around the map, so a read past either end shows"""
    n = g.numel()
    g_big, gc = _carve(dev, n, fill=float("nan"))
    gc.copy_(g)
    mc = None
    if gm is not None:
        m_big, mc = _carve(dev, n // 4, torch.uint8, 0)
        mc.copy_(gm)
    ops.grad_stats(gc, mc, ctl, **kw)
    return gc


def _check_stats(ops, ctl, want, n, what):
    f = lambda name: ops.step_ctl_field(ctl, name).item()
    got = {k: f(k) for k in want}
    print(what, {k: (got[k], want[k]) for k in want})
    assert got["found_inf"] == want["found_inf"] and got["skip"] == want["skip"] and got["step"] == want["step"]
    if not math.isfinite(want["sumsq"]):
        return got
    eps = 2.0 ** -53
    assert abs(got["sumsq"] - want["sumsq"]) <= n * eps * want["sumsq"]
    assert abs(got["grad_norm"] - want["grad_norm"]) <= (n / 2 + 4) * eps * want["grad_norm"]
    for k in ("clip_coef", "inv_scale_eff"):
        r = R.f32(want[k])
        assert abs(got[k] - r) <= abs(r) * 2.0 ** -23, k
    return got


@pytest.mark.parametrize("case", R.stats_cases(), ids=lambda c: c["name"])
def test_grad_stats_against_float64(dev, ops, case):
    g, gm, eg = R.build_stats(case)
    max_norm = R.stats_max_norm(case, g, eg)
    if case["nchunk"] == R.STATS_LARGE:                       # (its float64 sum is formed on the device)
        gd = g.to(dev).double()[(eg < 4).to(dev)]
        big_sum = float((gd * gd).sum())
    want = R.grad_stats64(g, eg, case["scale"], case["found_in"], case["grad_scale"], max_norm, case["skip_nonfinite"], case["step0"])
    bad_owned = case["bad"] is not None and case["bad"][1] != "unowned"
    assert (want["found_inf"] == 1.0) == (bad_owned or bool(case["found_in"]))
    if case["nchunk"] == R.STATS_LARGE and math.isfinite(big_sum):
        assert abs(big_sum - want["sumsq"]) <= 1e-12 * big_sum
    scale = None if case["scale"] is None else torch.full((1,), case["scale"], device=dev)
    found_in = None if case["found_in"] is None else torch.full((1,), case["found_in"], device=dev)
    ctl = ops.new_step_ctl(dev, case["step0"])
    _stats_call(dev, ops, g.to(dev), None if gm is None else gm.to(dev), ctl, scale=scale, found_inf=found_in,
                grad_scale=case["grad_scale"], max_norm=max_norm, skip_nonfinite=True)
    torch.cuda.synchronize()
    got = _check_stats(ops, ctl, want, g.numel(), case["name"])
    if math.isfinite(want["sumsq"]):
        assert got["grad_norm"] > 0 and (got["inv_scale_eff"] < 0) == (case["grad_scale"] < 0)
        if case["scale"] == 3.0 and case["max_norm"] is None:  # the double reciprocal rounded to f32, then the host factor
            assert got["inv_scale_eff"] == R.f32(R.f32(1.0 / 3.0) * case["grad_scale"])
        if case["max_norm"] == 1.0:
            assert got["clip_coef"] < 1.0                      # max_norm == norm: just below 1, the + 1e-6
        if case["max_norm"] in (None, 2.0):
            assert got["clip_coef"] == 1.0


def test_grad_stats_without_skip_reuse_of_a_record_and_a_preset_step(dev, ops):
    """skip_nonfinite = 0 with a NaN: found, not skipped, step + 1.  Then two more calls on the same record, back to back with
    different gradients and no synchronisation: the last result stands alone and step advanced each time from the preset 41."""
    case = dict(R.stats_cases()[9], scale=None, found_in=None, bad=(float("nan"), "last"), max_norm=None, step0=41)
    g1, gm, eg = R.build_stats(case)
    g2, _, _ = R.build_stats(dict(case, bad=None, seed=case["seed"] + 1))
    g3, _, _ = R.build_stats(dict(case, bad=None, seed=case["seed"] + 2))
    g3 = g3 * 0.25
    gmd = None if gm is None else gm.to(dev)
    ctl = ops.new_step_ctl(dev, 41)
    _stats_call(dev, ops, g1.to(dev), gmd, ctl, grad_scale=0.5, skip_nonfinite=False)
    torch.cuda.synchronize()
    f = lambda name: ops.step_ctl_field(ctl, name).item()
    assert f("found_inf") == 1.0 and f("skip") == 0 and f("step") == 42
    keep = [_stats_call(dev, ops, g2.to(dev), gmd, ctl, grad_scale=0.5, skip_nonfinite=True),
            _stats_call(dev, ops, g3.to(dev), gmd, ctl, grad_scale=0.5, max_norm=0.05, skip_nonfinite=True)]
    torch.cuda.synchronize()
    want = R.grad_stats64(g3, eg, None, None, 0.5, 0.05, 1, 43)
    assert want["step"] == 44 and want["clip_coef"] < 1.0
    _check_stats(ops, ctl, want, g3.numel(), "third call on one record")
    del keep


# ---- map bytes --------------------------------------------------------------------------------------------------------------
MAP_BYTES = (0, 1, 2, 3, 4, 254, 255)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_map_bytes_outside_the_groups_of_the_call(dev, ops, kind):
    """ngroups = 2: bytes 2 and 3 are trained with group 0's hyper-parameters, bytes 4 and 254 are what 255 is"""
    case = dict([c for c in R.cases() if c["kind"] == kind and c["nchunk"] == 257 and c["layout"] == "mixed"][0])
    assert case["ng"] == 2
    gm = torch.tensor(MAP_BYTES, dtype=torch.uint8).repeat(37)[:257]
    b = R.build(case, gm=gm)
    ref, bound = R.ref_and_bound(kind, b, case["hyp"])
    as0, _ = R.ref_and_bound(kind, dict(b, elem_group=torch.where(b["elem_group"] < 4, 0, 255)), case["hyp"])
    sel23 = (b["elem_group"] == 2) | (b["elem_group"] == 3)
    assert torch.equal(ref["p"][sel23], as0["p"][sel23])       # (the reference's reading: slot 0)
    B = _Bufs(dev, b, "bf16")
    _run_plain(ops, case, B)
    _gate(case["name"] + " map bytes", _outputs(case, B), ref, bound)
    B.check_untouched(ema_ran=case["hyp"]["ema_decay"] is not None)
    p0 = B.start["p"][PAD:-PAD]
    for byte in MAP_BYTES:
        sel = (b["elem_group"] == byte).to(dev)
        assert torch.equal(B.t["p"][sel], p0[sel]) == (byte >= 4), byte


def test_map_bytes_grad_stats(dev, ops):
    """sodt_grad_stats owns exactly the chunks the step kernels train: bytes 0..3; a NaN under byte 4, 254 or 255 is not found"""
    gm = torch.tensor(MAP_BYTES, dtype=torch.uint8).repeat(37)[:257]
    eg = gm.long().repeat_interleave(4)
    g = torch.randn(4 * 257, generator=torch.Generator().manual_seed(3)) * 0.1
    for byte, value in ((4, float("nan")), (254, float("inf")), (255, float("-inf"))):
        g[torch.nonzero(eg == byte).flatten()[::2]] = value
    ctl = ops.new_step_ctl(dev)
    _stats_call(dev, ops, g.to(dev), gm.to(dev), ctl, grad_scale=1.0, skip_nonfinite=True)
    torch.cuda.synchronize()
    _check_stats(ops, ctl, R.grad_stats64(g, eg, None, None, 1.0, None, 1, 0), g.numel(), "map bytes")
    for byte in (2, 3):
        g2 = g.clone()
        g2[int(torch.nonzero(eg == byte)[0])] = float("inf")
        _stats_call(dev, ops, g2.to(dev), gm.to(dev), ctl, grad_scale=1.0, skip_nonfinite=True)
        torch.cuda.synchronize()
        assert ops.step_ctl_field(ctl, "found_inf").item() == 1.0 and ops.step_ctl_field(ctl, "skip").item() == 1, byte


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_touch_nothing(dev, pkg):
    """what tests/test_amp_step_host.py does not hold for the two plain entries: SODT_EINVAL, and NaN-filled buffers that come
    back bit for bit"""
    L = pkg._lib
    lib = L.load()
    n = 64
    nan = lambda dt=torch.float32: torch.full((n + 8,), float("nan"), device=dev, dtype=dt)
    p, g, m, v, e, cast = nan(), nan(), nan(), nan(), nan(), nan(torch.bfloat16)
    gmap = torch.zeros(n // 4, dtype=torch.uint8, device=dev)
    bufs = (p, g, m, v, e, cast)
    before = [b.clone() for b in bufs]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: None if t is None else t.data_ptr() + off
    fl = lambda *a: (C.c_float * len(a))(*a)
    db = lambda *a: (C.c_double * len(a))(*a)
    F = C.c_float

    def sgd(p_=P(p), g_=P(g), m_=P(m), e_=P(e), c_=P(cast), code=L.BF16, n_=n, ng=2):
        return lib.sodt_sgd_ema_step(p_, g_, m_, e_, c_, code, P(gmap), n_, ng, fl(.01, .02, 0, 0, 0), fl(.9, .8, 0, 0, 0),
                                     fl(0, 5e-4, 0, 0, 0), 1, F(1.0), F(0.9999), st)

    def adam(p_=P(p), g_=P(g), m_=P(m), v_=P(v), e_=P(e), c_=P(cast), code=L.BF16, n_=n, ng=2, b1=(.9, .8), b2=(.999, .99),
             eps=(1e-8, 1e-6), step=1):
        pad = (0.5, 0.5, 0.5)
        return lib.sodt_adam_ema_step(p_, g_, m_, v_, e_, c_, code, P(gmap), n_, ng, db(1e-3, 2e-3, *pad), db(*b1, *pad),
                                      db(*b2, *pad), db(*eps, *pad), db(0, 5e-4, *pad), 0, step, F(1.0), F(0.9999), st)

    calls = {
        "sgd: misaligned p": lambda: sgd(p_=P(p, 4)), "sgd: misaligned g": lambda: sgd(g_=P(g, 8)),
        "sgd: misaligned momentum": lambda: sgd(m_=P(m, 4)), "sgd: misaligned ema": lambda: sgd(e_=P(e, 12)),
        "sgd: misaligned p_cast": lambda: sgd(c_=P(cast, 2)), "sgd: n % 4": lambda: sgd(n_=n - 1),
        "sgd: ngroups 0": lambda: sgd(ng=0), "sgd: ngroups 5": lambda: sgd(ng=5), "sgd: unknown cast_dtype": lambda: sgd(code=7),
        "adam: misaligned p": lambda: adam(p_=P(p, 8)), "adam: misaligned g": lambda: adam(g_=P(g, 4)),
        "adam: misaligned exp_avg": lambda: adam(m_=P(m, 4)), "adam: misaligned exp_avg_sq": lambda: adam(v_=P(v, 4)),
        "adam: misaligned ema": lambda: adam(e_=P(e, 4)), "adam: misaligned p_cast": lambda: adam(c_=P(cast, 2)),
        "adam: n % 4": lambda: adam(n_=n - 2), "adam: ngroups 0": lambda: adam(ng=0), "adam: ngroups 5": lambda: adam(ng=5),
        "adam: unknown cast_dtype": lambda: adam(code=7), "adam: step 0": lambda: adam(step=0),
        "adam: eps 0": lambda: adam(eps=(1e-8, 0.0)), "adam: beta1 1": lambda: adam(b1=(.9, 1.0)),
        "adam: beta2 1": lambda: adam(b2=(1.0, .99)),
    }
    for what, call in calls.items():
        assert call() == L.EINVAL, what
    torch.cuda.synchronize()
    for b, was in zip(bufs, before):
        assert _same_bits(b, was)
    assert sgd() == 0 and adam() == 0                          # (the same calls with nothing wrong are accepted)
    torch.cuda.synchronize()
