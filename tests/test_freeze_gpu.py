"""requires_grad honoured by the engine (freeze.py, engine.py, optim.py, ddp.py): a frozen parameter has no gradient (.grad None, a
zero slice of the flat buffer), a unit whose output needs no gradient has no backward launch and saves nothing in the forward,
the fused optimizers leave a frozen parameter and its state alone, and a data-parallel step reduces the trainable tail only.

Everything at S = 128, B = 2: the smallest size at which all three stages, both block kinds and the whole head graph run.  The
reference of every step is the CPU oracle with the SAME requires_grad flags, computed once per freeze case and shared; the gates
are those of tests/test_model_gpu.py::test_train_step_vs_oracle (logits 1e-3 / gradients 2e-3 in f32, 0.30 / 0.17 in bf16, the
same floor on the gradient norm).  Before the engine read requires_grad, the `.grad is None` / zero-slice checks of every row with a
frozen parameter, the launch-list, workspace and data-parallel range checks and the bit-for-bit checks of the optimizer test failed."""
import functools
import importlib

import pytest
import torch

from freeze_cases import E, PKG, ROWS, apply, build

pytestmark = pytest.mark.gpu
S, B, NC = 128, 2, 8
F32, BF = torch.float32, torch.bfloat16
GATES = {F32: (1e-3, 2e-3), BF: (0.30, 0.17)}
ZERO_GRAD = E + "stage3.0.mlp.fc2.bias"          # zero in exact arithmetic (tests/test_model_gpu.py)
# what the backward of an encoder unit reads back from its forward (engine._attn_fwd / _mlp_fwd / _merge_fwd)
ENC_SAVES = (".xn1", ".st1", ".st2", ".xm", ".xn2", ".ao", ".aop", ".qkv", ".qkvw", ".lse", ".lsew", ".ha", ".hp", ".u", ".cp", ".ca")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()), float(b.abs().max())


@functools.lru_cache(maxsize=None)
def oracle(case, seed=1):
    """One CPU step of the oracle with the case's requires_grad flags: logits, the compared features, gradients, new running
    statistics.  Cached: the f32 and the bf16 run of a case (and the toggling test) share it; nobody writes to it."""
    from oracle import ref_torch as R
    from freeze_cases import CASES
    sd = R.procedural_state_dict(S, NC)
    x_rgb, x_ir = R.synthetic_inputs(B, S, seed=seed)
    osd = {}
    for k, v in sd.items():
        leaf = v.dtype.is_floating_point and "running" not in k and "anchor" not in k
        osd[k] = v.clone().requires_grad_(bool(leaf and not CASES[case](k, v)))
    ns = {}
    opred, oy = R.model_forward(osd, x_rgb, x_ir, True, ns)
    gsel = R._hash01("gsel", opred[0].numel()).view(opred[0].shape).float()
    loss = (opred[0] * gsel).sum()
    if loss.requires_grad:
        loss.backward()
    return dict(pred=opred[0].detach(), feats={i: oy[i].detach() for i in (0, 1, 2, 10)}, grads={k: v.grad for k, v in osd.items()},
                stats={k: v.detach() for k, v in ns.items()}, gsel=gsel, n_sd=len(osd), x=(x_rgb, x_ir))


def gmed_floor():
    """the floor of tests/test_model_gpu.py: the lower-quartile gradient norm of the step with nothing frozen"""
    ref = oracle("nothing")
    return sorted(float(g.double().norm()) for g in ref["grads"].values() if g is not None)[ref["n_sd"] // 4]


def step(model, dev, seed=1):
    ref = oracle("nothing", seed)
    x_rgb, x_ir = ref["x"]
    pred, y = model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
    (pred[0] * ref["gsel"].to(dev)).sum().backward()
    return pred, y


def check_step(model, pred, y, case, dtype, frozen, running=True):
    """the gates of test_train_step_vs_oracle on the trainable parameters; None and an all-zero slice for the frozen ones"""
    tol_logit, tol_grad = GATES[dtype]
    ref = oracle(case)
    err, scale = rel(pred[0], ref["pred"])
    print(f"{case} {dtype}: logits max abs err {err:.3e} (|logit| max {scale:.2f})")
    assert err <= tol_logit, f"logits max abs err {err:.3e} (|logit| max {scale:.2f})"
    for i in (0, 1, 2, 10):
        e, s = rel(y[i], ref["feats"][i])
        assert e <= tol_logit * max(1.0, s), f"feature {i}: {e:.3e} / {s:.2f}"
    gmed = gmed_floor()
    eng = model._get_engine()
    allr = []
    for n, p in model.named_parameters():
        og = ref["grads"][n]
        if n in frozen:
            assert og is None, n
            assert p.grad is None, f"{n}: frozen, .grad is {type(p.grad).__name__}"
            o = eng.grad_offsets[n]
            assert not bool(eng.flat_grad[o: o + p.numel()].any()), f"{n}: frozen, its slice of the flat gradient is not zero"
            continue
        assert p.grad is not None and og is not None, n
        gn = float(og.double().norm())
        d = float((p.grad.double().cpu() - og.double()).norm())
        if n == ZERO_GRAD:
            assert d <= max(tol_grad, 0.05) * gmed, (n, d, gmed)
            continue
        allr.append((d / (gn + 1e-2 * gmed + 1e-12), n))
    allr.sort(reverse=True)
    print(f"{case} {dtype}: worst relative gradient errors {allr[:3]}")
    assert not allr or allr[0][0] <= tol_grad, f"worst relative gradient errors {allr[:6]}"
    if running:
        bufs = dict(model.named_buffers())
        for k, v in ref["stats"].items():
            e, s = rel(bufs[k], v)
            assert e <= (1e-4 if dtype == F32 else 3e-2) * max(1.0, s), k


def fresh(dev, dtype, case="nothing"):
    model, _ = build(dev, S, NC)
    model.compute_dtype = dtype
    model.train()
    return model, apply(model, case)


def sig(calls):
    """A launch list without its addresses: (kernel, tag, which arguments are absent, the scalar arguments).  The launches at the
    head of a list, before the engine sets its first tag, carry the tag of whatever was recorded last (ops.set_tag is global):
    that leading run of equal tags is blanked."""
    out = []
    lead = calls[0][3] if calls else ""
    for fn, args, name, tag in calls:
        if tag != lead:
            lead = None
        tag = "" if lead is not None else tag
        shape = []
        for a in args:
            a = getattr(a, "value", a)
            if a is None or isinstance(a, float):
                shape.append(a)
            elif isinstance(a, int):
                shape.append("ptr" if a > (1 << 24) else a)
            else:
                shape.append("ref")
        out.append((name, tag, tuple(shape)))
    return out


def train_plan(model, dtype=F32):
    eng = model._get_engine()
    return eng.plans[(B, S, dtype, True, eng.freeze_record().signature)]


# ---------------------------------------------------------------- 1. a training step against the oracle
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ROWS)
def test_train_step_vs_oracle(dev, case, dtype):
    model, frozen = fresh(dev, dtype, case)
    pred, y = step(model, dev)
    check_step(model, pred, y, case, dtype, frozen)
    assert (len(frozen) > 0) == (case != "nothing") and (case != "everything" or len(frozen) == len(list(model.parameters())))
    if case == "everything":                              # backward() completes and the recorded backward was never entered
        assert train_plan(model, dtype).bwd_main is None


# ---------------------------------------------------------------- 2. launch lists
def test_encoder_frozen_backward_is_the_head_alone(dev, ops):
    full, _ = fresh(dev, F32)
    step(full, dev)
    pf = train_plan(full)
    head_part = [(c[2], c[3]) for c in pf.bwd_main[: pf.enc_bwd_start]]
    model, frozen = fresh(dev, F32, "encoder")
    step(model, dev)
    plan = train_plan(model)
    got = [(c[2], c[3]) for c in plan.bwd_main]
    names = [n for n, _ in got]
    for bad in ("sodt_wmsa_block_bwd", "sodt_window_attn_bwd", "sodt_window_attn_bwd_wm", "sodt_window_attn_sp_bwd", "sodt_layernorm_bwd",
                "sodt_linear_bwd_sq", "sodt_transpose_f32", "sodt_batch_sum", "sodt_convmlp_decompose"):
        assert bad not in names, bad
    assert not [g for g in got if g[1].startswith(("stage", "pmerging"))], "an encoder launch in the backward of a frozen encoder"
    n_w = sum(1 for n, p in model.named_parameters() if n.startswith("detect.") and p.dim() > 1)       # 12 convolutions + Detect
    assert n_w == 13 and names.count("sodt_gemm_tn") == n_w
    # it is the head's part of the full backward, minus the one input-gradient GEMM toward the encoder that stood alone (the first
    # head Conv reads y[2] only; the C3 units' input gradient still serves their head-side input)
    want = list(head_part)
    want.remove(("sodt_gemm_nt", "h0.bwd"))
    assert got == want
    assert plan.enc_bwd_start is None and plan.enc_gin is None and plan.bwd_marks and all(lo >= plan.fz.first_trainable_offset for _, lo, _ in plan.bwd_marks)
    # the live part of a replayed backward: Detect's un-permute; no front-end backward
    for p in model.parameters():
        p.grad = None
    ref = oracle("nothing")
    pred, _ = model(ref["x"][0].to(dev), ref["x"][1].to(dev), "RGB+IR")
    with ops.Recorder() as rec:
        (pred[0] * ref["gsel"].to(dev)).sum().backward()
    assert [c[2] for c in rec.calls] == ["sodt_memset_zero", "sodt_detect_unpermute"]       # (the reset gradient buffer, Detect)
    for p in full.parameters():
        p.grad = None
    pred, _ = full(ref["x"][0].to(dev), ref["x"][1].to(dev), "RGB+IR")
    with ops.Recorder() as rec:
        (pred[0] * ref["gsel"].to(dev)).sum().backward()
    assert [c[2] for c in rec.calls] == ["sodt_memset_zero", "sodt_detect_unpermute", "sodt_frontend_bwd"]
    x = ref["x"]
    with pytest.raises(RuntimeError, match="the encoder's backward was not recorded on this plan: frozen parameters"):
        model._get_engine().replay_encoder_backward(plan, x[0].to(dev), x[1].to(dev))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_nothing_frozen_lists_are_those_of_a_model_never_frozen(dev, dtype):
    a, _ = fresh(dev, dtype)
    step(a, dev)
    pa = train_plan(a, dtype)
    b, _ = fresh(dev, dtype, "encoder")
    step(b, dev)
    apply(b, "through_stage1")
    step(b, dev)
    apply(b, "nothing")
    for p in b.parameters():
        p.grad = None
    step(b, dev)
    pb = train_plan(b, dtype)
    assert pb.fz.signature == 0 and pb is b._get_engine().plans[(B, S, dtype, True)]
    assert sig(pa.fwd_main) == sig(pb.fwd_main) and sig(pa.bwd_main) == sig(pb.bwd_main) and sig(pa.fwd_pre) == sig(pb.fwd_pre)
    assert {k: (tuple(v.shape), v.dtype) for k, v in pa.bufs.items()} == {k: (tuple(v.shape), v.dtype) for k, v in pb.bufs.items()}
    assert pa.bwd_marks == pb.bwd_marks and len(pa.bwd_marks) == 2 and pa.enc_bwd_start == pb.enc_bwd_start
    assert {k: type(v).__name__ for k, v in pa.saved.items()} == {k: type(v).__name__ for k, v in pb.saved.items()}
    routes = lambda pl: {k: (r.geo, r.pad, r.attn, r.mlp, r.zscratch, r.sq_ok) for k, r in pl.saved.items() if k.startswith("stage")}   # noqa: E731
    assert routes(pa) == routes(pb) and len(routes(pa)) == 11


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_frozen_stage1_forward_is_the_eval_plan_s(dev, dtype):
    model, frozen = fresh(dev, dtype, "through_stage1")
    step(model, dev)
    plan = train_plan(model, dtype)
    ref = oracle("nothing")
    model.eval()
    with torch.no_grad():
        model(ref["x"][0].to(dev), ref["x"][1].to(dev), "RGB+IR")
    model.train()
    eng = model._get_engine()
    ev = eng.plans[(B, S, dtype, False)]
    s1 = lambda calls: [c for c in sig(calls) if c[1].startswith("stage1.")]           # noqa: E731
    assert s1(plan.fwd_main) and s1(plan.fwd_main) == s1(ev.fwd_main)
    # ... and not the training form, which also writes what the backward reads
    apply(model, "nothing")
    for p in model.parameters():
        p.grad = None
    step(model, dev)
    assert s1(train_plan(model, dtype).fwd_main) != s1(ev.fwd_main)
    # the eval plan is one plan whatever the flags
    apply(model, "encoder")
    model.eval()
    with torch.no_grad():
        model(ref["x"][0].to(dev), ref["x"][1].to(dev), "RGB+IR")
    assert eng.plans[(B, S, dtype, False)] is ev and sum(1 for k in eng.plans if not k[3]) == 1


# ---------------------------------------------------------------- 3. workspace
def _plan_bytes(plan):
    seen, tot = set(), 0
    for t in plan.bufs.values():
        st = t.untyped_storage()
        if st.data_ptr() not in seen:
            seen.add(st.data_ptr())
            tot += st.nbytes()
    return tot


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_frozen_encoder_saves_nothing(dev, dtype):
    full, _ = fresh(dev, dtype)
    step(full, dev)
    model, _ = fresh(dev, dtype, "encoder")
    step(model, dev)
    pf, plan = train_plan(full, dtype), train_plan(model, dtype)
    kept = [k for k in plan.bufs if k.startswith(("stage", "pmerging")) and (k.endswith(ENC_SAVES) or k.endswith((".z", ".st")))]
    assert not kept, kept
    assert [k for k in pf.bufs if k.startswith("stage1.0") and k.endswith(ENC_SAVES)], "the unfrozen plan keeps them under these names"
    assert not [k for k in plan.bufs if k.startswith("g.dA") or k.startswith("g.dB") or k == "g.dx0" or k == "fe.ws"]
    print(f"{dtype}: plan bytes frozen encoder {_plan_bytes(plan)}, nothing frozen {_plan_bytes(pf)}")
    assert _plan_bytes(plan) < _plan_bytes(pf)
    # the head still saves: its backward runs
    assert "h0.z" in plan.bufs and "h7.cv3.z" in plan.bufs


# ---------------------------------------------------------------- 4. toggling on one model
def _accumulated(model, times):
    """every listed parameter's gradient is times[name] x the oracle's, inside the f32 gradient gate of test 1"""
    ref, gmed = oracle("nothing"), gmed_floor()
    named = dict(model.named_parameters())
    for n, k in times.items():
        og = k * ref["grads"][n].double()
        d = float((named[n].grad.double().cpu() - og).norm())
        if n == ZERO_GRAD:
            assert d <= 0.05 * k * gmed, n
        else:
            assert d / (float(og.norm()) + 1e-2 * gmed + 1e-12) <= GATES[F32][1], (n, d)


def test_toggling_on_one_model(dev):
    model, _ = fresh(dev, F32)
    pred, y = step(model, dev)
    check_step(model, pred, y, "nothing", F32, set(), running=False)
    was = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is not None for g in was.values())
    frozen = apply(model, "encoder")                      # no zero_grad: the newly frozen parameters still hold their views
    pred, y = step(model, dev)
    for n, p in model.named_parameters():
        assert (p.grad is None) == (n in frozen), n
    # the head accumulated a second gradient (the gate of test 1 on twice the oracle's), the encoder's slices were cleared
    eng = model._get_engine()
    _accumulated(model, {n: 2 for n, _ in model.named_parameters() if n not in frozen})
    assert not bool(eng.flat_grad[: eng.freeze_record().first_trainable_offset].any())
    for p in model.parameters():
        p.grad = None
    pred, y = step(model, dev)
    check_step(model, pred, y, "encoder", F32, frozen, running=False)
    g1 = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    pred, y = step(model, dev)                            # accumulate: twice the single gradient, the frozen slices stay zero
    for n, p in model.named_parameters():
        if n in frozen:
            assert p.grad is None, n
        else:
            assert torch.allclose(p.grad, 2 * g1[n], rtol=2e-3, atol=1e-6), n
    assert not bool(eng.flat_grad[: eng.freeze_record().first_trainable_offset].any())
    apply(model, "nothing")
    for p in model.parameters():
        p.grad = None
    pred, y = step(model, dev)
    check_step(model, pred, y, "nothing", F32, set(), running=False)
    # unfreezing in the middle of an accumulation keeps what the head has accumulated
    for p in model.parameters():
        p.grad = None
    apply(model, "encoder")
    step(model, dev)
    apply(model, "nothing")
    step(model, dev)
    _accumulated(model, {n: 1 if n in frozen else 2 for n, _ in model.named_parameters()})


# ---------------------------------------------------------------- 5. optimizers
def _ref_optimizer(kind, model, wd):
    """torch's optimizer over clones of every parameter, in the two groups of optim.set_weight_decay"""
    ref = {n: torch.nn.Parameter(p.detach().clone()) for n, p in model.named_parameters()}
    decay = [ref[n] for n, p in model.named_parameters() if not (p.dim() == 1 or n.endswith(".bias"))]
    rest = [ref[n] for n, p in model.named_parameters() if p.dim() == 1 or n.endswith(".bias")]
    groups = [{"params": decay, "weight_decay": wd}, {"params": rest, "weight_decay": 0.0}]
    if kind == "sgd":
        return ref, torch.optim.SGD(groups, lr=0.01, momentum=0.937, nesterov=True)
    return ref, torch.optim.Adam(groups, lr=1e-3, betas=(0.937, 0.999))


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_fused_optimizers_leave_frozen_parameters_alone(dev, kind, clip):
    """Built over ALL parameters, one step with everything trainable (so that the encoder has momentum / moments), then the encoder
    is frozen (Train.py:328-333) and the next step must pass over it as torch does over a parameter whose .grad is None: no weight
    decay, no momentum, no moment update - bit for bit.  Bounds: tests/test_optim_gpu.py / test_adam_gpu.py (2e-6 of max|ref| +
    1e-5 per tensor); the norm of last_step_info() against the float64 norm over the trainable gradients, 1e-8 relative (the float64
    summation bound of tests/test_amp_step_gpu.py)."""
    O = importlib.import_module(PKG + ".optim")
    wd = 0.00048
    model, _ = fresh(dev, F32)
    kw = dict(max_grad_norm=1e9) if clip else {}
    if kind == "sgd":
        opt = O.FusedSGD(O.set_weight_decay(model, weight_decay=wd), model=model, lr=0.01, momentum=0.937, nesterov=True, **kw)
    else:
        opt = O.FusedAdam(O.set_weight_decay(model, weight_decay=wd), model=model, lr=1e-3, betas=(0.937, 0.999), **kw)
    assert [g["weight_decay"] for g in opt.param_groups] == [wd, 0.0] and sum(len(g["params"]) for g in opt.param_groups) == len(list(model.parameters()))
    ref, ropt = _ref_optimizer(kind, model, wd)
    eng = model._get_engine()
    frozen = set()
    for it in range(2):
        if it == 1:
            frozen = apply(model, "encoder")
            for n in frozen:
                ref[n].requires_grad_(False)
        step(model, dev)
        train = [n for n, p in model.named_parameters() if n not in frozen]
        for n, p in model.named_parameters():
            ref[n].grad = p.grad.detach().clone() if n in train else None
        norm64 = float(torch.sqrt(sum(ref[n].grad.double().square().sum() for n in train)))
        if clip:
            opt.max_grad_norm = 0.5 * norm64
            torch.nn.utils.clip_grad_norm_([ref[n] for n in train], 0.5 * norm64)
        before = [eng.flat_param.clone()] + [s.clone() for s in (opt._state or [])]
        opt.step()
        ropt.step()
        opt.zero_grad(set_to_none=True)
        ropt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        if clip:
            gn = float(opt.last_step_info()[1])
            print(f"{kind} step {it}: kernel norm {gn:.9e}, f64 norm over the trainable gradients {norm64:.9e}")
            assert abs(gn - norm64) <= 1e-8 * norm64
        after = [eng.flat_param] + list(opt._state)
        for n in frozen:
            o, k = eng.grad_offsets[n], ref[n].numel()
            for what, a, b_ in zip(("parameter", "state 1", "state 2"), before, after):
                assert torch.equal(a[o: o + k], b_[o: o + k]), f"step {it}: {what} of frozen {n} moved"
        if it == 1:       # ... and they did have a state to move
            o = eng.grad_offsets[E + "stage1.0.attn.qkv.weight"]
            assert bool(opt._state[0][o: o + 64].any())
        worst = 0.0
        for n, p in model.named_parameters():
            s = float(ref[n].abs().max()) + 1e-5
            err = float((p.detach() - ref[n].detach()).abs().max())
            worst = max(worst, err / s)
            assert err <= 2e-6 * s, f"step {it}: parameter {n}: {err:.3e} > {2e-6 * s:.3e}"
        print(f"{kind} clip={clip} step {it}: worst parameter error relative to max|ref| + 1e-5: {worst:.3e}")


# ---------------------------------------------------------------- 6. the SR branch
@pytest.mark.parametrize("case", ["model_up", "encoder"])
def test_sr_model_frozen(dev, case, ops):
    """Model(sr=True) at f32, both outputs in the loss: the gates of tests/test_model_sr_gpu.py::test_sr_train_step_vs_oracle
    (outputs 1e-3 relative l2, gradients 1e-2 with its floor)."""
    from oracle import ref_torch as R
    from freeze_cases import CASES
    from test_model_sr_gpu import rel_l2
    model, sd = build(dev, S, NC, sr=True)
    model.compute_dtype = F32
    model.train()
    frozen = apply(model, case)
    x_rgb, x_ir = R.synthetic_inputs(B, S, seed=1)
    pred, out_sr, y = model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
    gsel = R._hash01("gsel", pred[0].numel()).view(pred[0].shape).float()
    ssel = R._hash01("ssel", out_sr.numel()).view(out_sr.shape).float() * 0.05
    ((pred[0] * gsel.to(dev)).sum() + (out_sr * ssel.to(dev)).sum()).backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    # the live launches of a second, replayed backward (the SR branch, Detect's un-permute, the front end)
    for p in model.parameters():
        p.grad = None
    pred2, out_sr2, _ = model(x_rgb.to(dev), x_ir.to(dev), "RGB+IR")
    with ops.Recorder() as rec:
        ((pred2[0] * gsel.to(dev)).sum() + (out_sr2 * ssel.to(dev)).sum()).backward()
    live = [c[2] for c in rec.calls]
    for n, p in model.named_parameters():
        p.grad = grads.get(n)
    osd = {}
    for k, v in sd.items():
        leaf = v.dtype.is_floating_point and "running" not in k and "anchor" not in k
        osd[k] = v.clone().requires_grad_(bool(leaf and not CASES[case](k, v)))
    opred, oy = R.model_forward(osd, x_rgb, x_ir, True, {})
    osr = R.deeplab_sr(osd, "model_up.", oy[8], oy[5], 2)
    ((opred[0] * gsel).sum() + (osr * ssel).sum()).backward()
    assert rel_l2(out_sr.detach(), osr.detach()) <= 1e-3 and rel_l2(pred[0].detach(), opred[0].detach()) <= 1e-3
    og_all = {k: v.grad for k, v in osd.items() if v.requires_grad}
    gmed = sorted(float(v.double().norm()) for v in og_all.values())
    gmed = gmed[len(gmed) // 4]
    eng = model._get_engine()
    allr = []
    for n, p in model.named_parameters():
        if n in frozen:
            o = eng.grad_offsets[n]
            assert p.grad is None and not bool(eng.flat_grad[o: o + p.numel()].any()), n
            continue
        og = og_all[n]
        assert p.grad is not None, n
        if n == ZERO_GRAD:
            continue
        den = float(og.double().norm()) + 1e-2 * gmed + 1e-12
        allr.append((float((p.grad.double().cpu() - og.double()).norm()) / den, n))
    allr.sort(reverse=True)
    print(f"sr, {case} frozen: worst gradient errors {allr[:3]}")
    assert allr and allr[0][0] <= 1e-2, allr[:6]
    if case == "model_up":      # the branch runs for its input gradients only: no weight-gradient launch of its 41 convolutions
        assert "sodt_gemm_tn" not in live and not [n for n in live if "wgrad" in n] and "sodt_gemm_nt" in live, sorted(set(live))
        assert "sodt_frontend_bwd" in live
    else:
        assert "sodt_frontend_bwd" not in live and "sodt_gemm_tn" in live


# ---------------------------------------------------------------- 7. data parallel
def test_ddp_reduces_the_trainable_tail_only(dev, tmp_path):
    """One process, world size 1 (gloo over a file store).  The reducer is handed flat_grad[first_trainable_offset:] - as ONE slice
    on the step that records, as the recorded buckets plus the closing slice on a replayed step (world forced to 2 so that the
    collectives are issued: the sum over one rank is the identity) - and the gradients are those of a model without a reducer."""
    import torch.distributed as dist
    ddp = importlib.import_module(PKG + ".ddp")
    solo, frozen = fresh(dev, F32, "encoder")
    step(solo, dev)
    want = solo._get_engine().flat_grad.clone()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        model, frozen = fresh(dev, F32, "encoder")
        ddp.attach(model, average=False)
        eng = model._get_engine()
        red = eng.ddp
        red.world = 2
        seen = []
        base = eng.flat_grad.data_ptr()
        for name in ("reduce", "reduce_async", "finish"):
            def wrapped(t, name=name, inner=getattr(red, name)):
                seen.append((name, (t.data_ptr() - base) // 4 if t.numel() else None, t.numel()))
                return inner(t)
            setattr(red, name, wrapped)
        first, total = eng.freeze_record().first_trainable_offset, eng.flat_grad.numel()
        assert 0 < first == eng.grad_offsets["detect.0.conv.weight"] < total
        step(model, dev)                                  # records: one reduce of the tail
        assert seen == [("reduce", first, total - first)], seen
        torch.cuda.synchronize()
        assert float((eng.flat_grad - want).abs().max()) <= 2e-4 * float(want.abs().max())
        del seen[:]
        for p in model.parameters():
            p.grad = None
        step(model, dev)                                  # replays in segments: the buckets that have a backward, then the rest
        torch.cuda.synchronize()
        plan = train_plan(model)
        asyncs = [s for s in seen if s[0] == "reduce_async"]
        assert [s[0] for s in seen] == ["reduce_async"] * len(plan.bwd_marks) + ["finish"] and asyncs
        covered = sorted((s[1], s[1] + s[2]) for s in seen if s[2])
        assert covered[0][0] == first and covered[-1][1] == total and all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1)), covered
        assert float((eng.flat_grad - want).abs().max()) <= 2e-4 * float(want.abs().max())
        assert not bool(eng.flat_grad[:first].any())
        # nothing frozen: the whole buffer, in the two buckets and the closing slice as before
        apply(model, "nothing")
        for p in model.parameters():
            p.grad = None
        del seen[:]
        step(model, dev)
        assert seen == [("reduce", 0, total)], seen
        del seen[:]
        for p in model.parameters():
            p.grad = None
        step(model, dev)
        torch.cuda.synchronize()
        assert [(s[0], s[1], s[2]) for s in seen] == [("reduce_async", eng.ddp_split3, total - eng.ddp_split3),
                                                      ("reduce_async", eng.ddp_split, eng.ddp_split3 - eng.ddp_split), ("finish", 0, eng.ddp_split)]
    finally:
        dist.destroy_process_group()
