"""loss.ComputeLoss and the two C entries behind it (csrc/loss.hip, sodt_yolo_loss / sodt_yolo_loss_fl) away from the one
configuration of test_loss_gpu.py and test_loss_focal_gpu.py: rectangular grids, gr < 1, anchor_t of 2 / 4 / 8, nc of
1 / 2 / 32 with 1 / 3 / 8 anchors, pos-weights without focal loss, thresholds hit exactly, a crowded grid, image indices out
of range, tiny and ragged launches, bf16 / non-contiguous / device-scalar use of the wrapper, argument rejection, large
logits.  Inputs come from tests/loss_cases.py; test_loss_ref_host.py shows on the CPU that each does what it is for.

Every case is held against the float64 restatement of tests/loss_ref.py and, where the reference's own class can run it,
against its outputs in tests/golden/loss_edges.pt (tools/gen_loss_edges_golden.py), at the gates of test_loss_focal_gpu.py:
2e-5 * max(1, |ref|) on each of the four losses, 2e-6 + 2e-5 * max|dpred| on the gradient.  Every gradient element must be
finite; calls through the C entries start from a dpred full of NaN.  Every comparison prints its figures before it asserts."""
import functools
import importlib
import os

import pytest
import torch

import loss_cases as LC
import loss_ref as LR

pytestmark = pytest.mark.gpu
PKG = LC.PKG
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = LC.case(name)
    *out, n, dpred = LR.compute_loss_f64(c["pred"], c["targets"], c["anchors"], c["hyp"], c["gr"], c["nc"])
    return out, n, dpred


@functools.lru_cache(maxsize=None)
def _goldens():
    g = torch.load(os.path.join(GOLD, "loss_edges.pt"))
    return {c["name"]: dict(c, **g["inputs"][c["input"]]) for c in g["cases"]}


def _wrapper(c, dev, pred=None, scale=1.0):
    """The case through loss.ComputeLoss: (four outputs on the CPU in float64, d(scale * loss) / d(pred))."""
    Lm = importlib.import_module(PKG + ".loss")
    cl = Lm.ComputeLoss(LC.fake_model(c["anchors"], c["hyp"], c["gr"], dev, c["nc"]))
    pg = (c["pred"] if pred is None else pred).to(dev).requires_grad_(True)
    out = cl([pg], c["targets"].to(dev))
    (out[0] * scale).backward()
    torch.cuda.synchronize()
    return [o.detach().cpu().double().reshape(-1) for o in out], pg.grad.cpu()


def _entry(c, dev, **kw):
    gamma = c["hyp"]["fl_gamma"]
    name = "sodt_yolo_loss_fl" if gamma > 0 else "sodt_yolo_loss"
    rc, out, dpred = LC.call_entry(name, c, dev, gamma=gamma if gamma > 0 else None, **kw)
    assert rc == 0
    return [o.reshape(-1) for o in out.cpu().double()], dpred.cpu()


def _check(tag, out, dpred, ref, refd, gate_out=None, gate_d=None):
    """Print, then assert: all finite, the four losses and the gradient inside the gates (the project's unless given)."""
    g_out, g_d = LR.gates(ref, refd)
    g_out, g_d = gate_out or g_out, gate_d or g_d
    errs = [float((a.double().reshape(-1) - b.double().reshape(-1)).abs().max()) for a, b in zip(out, ref)]
    derr = float((dpred.double() - refd.double()).abs().max())
    print(f"{tag}: loss errs {[f'{e:.2e}' for e in errs]} (gates {[f'{g:.1e}' for g in g_out]}) of "
          f"{[f'{float(b):.4f}' for b in ref]}; dpred err {derr:.3e} (gate {g_d:.2e}) of max {float(refd.abs().max()):.3e}")
    assert bool(torch.isfinite(dpred).all()), f"{tag}: dpred has non-finite elements"
    assert all(bool(torch.isfinite(o).all()) for o in out), tag
    for e, g in zip(errs, g_out):
        assert e <= g, (tag, errs, g_out)
    assert derr <= g_d, (tag, derr, g_d)


def _check_case(name, out, dpred, how):
    ref, n, refd = _ref(name)
    _check(f"{name} [{how}] vs f64 ({n} matches)", out, dpred, ref, refd)
    gold = _goldens().get(name)
    assert (gold is not None) == LC.case(name)["golden"]
    if gold is not None:
        _check(f"{name} [{how}] vs reference golden", out, dpred, gold["out"], gold["dpred"])


def _run(name, dev, entry=False):
    c = LC.case(name)
    out, dpred = _wrapper(c, dev)
    _check_case(name, out, dpred, "ComputeLoss")
    if entry:
        out, dpred = _entry(c, dev)
        _check_case(name, out, dpred, "C entry")
    return out, dpred


def _match_count(ws, c):
    """The match count the kernels accumulated: sums[3] of the workspace (csrc/loss.hip: the winner table of ncells ints
    rounded up to 256 bytes, then four doubles: box, cls, obj, n)."""
    B, na, ny, nx, _ = c["pred"].shape
    win = (B * na * ny * nx * 4 + 255) & ~255
    return float(ws[win:win + 32].view(torch.float64)[3])


# ---- 1. rectangular grids
@pytest.mark.parametrize("name", ["rect_12x20_plain", "rect_12x20_focal", "rect_20x12_plain", "rect_20x12_focal"])
def test_rectangular_grid(dev, name):
    _run(name, dev, entry=True)


# ---- 2. gr and anchor_t
@pytest.mark.parametrize("name", ["gr0.0_t4", "gr0.5_t2", "gr0.5_t4", "gr0.5_t8"])
def test_gr_and_anchor_t(dev, name):
    out, dpred = _run(name, dev)
    if name == "gr0.0_t4":
        # gr == 0: every matched cell's objectness target is exactly 1, whatever its IoU: d BCE(x, 1) / dx = -(1 - sigmoid(x))
        c = LC.case(name)
        ref, n, refd = _ref(name)
        B, na, ny, nx, _ = c["pred"].shape
        cells = sorted({k[:4] for k in LR.candidates(c["pred"].shape, c["targets"], c["anchors"], c["hyp"]["anchor_t"])})
        b, a, gj, gi = (torch.tensor(v) for v in zip(*cells))
        x = c["pred"][b, a, gj, gi, 4].double()
        want = -(1.0 - x.sigmoid()) * c["hyp"]["obj"] * 4.0 * B / (B * na * ny * nx)
        assert float((refd[b, a, gj, gi, 4] - want).abs().max()) < 1e-15
        err = float((dpred[b, a, gj, gi, 4].double() - want).abs().max())
        print(f"{name}: objectness gradient of {len(cells)} matched cells against target 1: err {err:.3e}")
        assert err <= LR.gates(ref, refd)[1]


# ---- 3. class count, anchor count, workspace size
@pytest.mark.parametrize("name", ["nc1", "nc2", "nc32_na1", "nc32_na3", "nc32_na8"])
def test_class_and_anchor_count(dev, name):
    out, dpred = _run(name, dev, entry=True)
    if name == "nc1":
        assert float(out[3]) == 0.0 and float(_ref(name)[0][3]) == 0.0
        assert bool((dpred[..., 5:] == 0).all()) and dpred.shape[-1] == 6


def test_workspace_of_exactly_the_reported_size(dev):
    """nc = 32, na = 8: the largest record and the most candidates per target.  The workspace is a slice of exactly
    sodt_yolo_loss_workspace_bytes inside a larger buffer; the bytes on either side must come back unchanged.  (With 192
    cells and 8 targets the winner table and the records fill their 256-byte roundings completely.)"""
    c = LC.case("nc32_na8")
    need, guard = LC.workspace_bytes(c), 8192
    big = torch.full((need + 2 * guard,), 0xA5, device=dev, dtype=torch.uint8)          # 0xA5A5A5A5 is no NaN
    ws = big[guard:guard + need]
    assert ws.data_ptr() % 256 == 0
    out, dpred = _entry(c, dev, ws=ws, ws_bytes=need)
    _check_case("nc32_na8", out, dpred, "C entry, exact workspace")
    assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + need:] == 0xA5).all())
    assert _match_count(ws, c) == _ref("nc32_na8")[1]


# ---- 4. pos-weights without focal loss
@pytest.mark.parametrize("name", ["posw_rand_1.3_0.8", "posw_rand_0.5_2.0"])
def test_pos_weights_plain_path(dev, name):
    ops = importlib.import_module(PKG + ".ops")
    with ops.Recorder() as rec:
        _run(name, dev)
    assert [n for _, _, n, _ in rec.calls] == ["sodt_yolo_loss"]


# ---- 5. thresholds hit exactly
def test_thresholds_hit_exactly(dev):
    _run("thresholds", dev, entry=True)


# ---- 6. crowded cells
@pytest.mark.parametrize("name", ["crowded_plain", "crowded_focal"])
def test_crowded_cells(dev, name):
    """64 targets on a 4 x 4 grid: box and class gradients of a cell are sums over its candidates, its objectness target is
    the last candidate's, and n counts every candidate."""
    c = LC.case(name)
    _run(name, dev)
    ws = torch.empty(LC.workspace_bytes(c), device=dev, dtype=torch.uint8)
    out, dpred = _entry(c, dev, ws=ws, ws_bytes=ws.numel())
    _check_case(name, out, dpred, "C entry")
    assert _match_count(ws, c) == _ref(name)[1]


# ---- 7. image index out of range
def test_image_index_out_of_range(dev):
    """Rows with image index -1, B and B + 3 among valid rows: skipped.  The result is the result on the valid rows alone."""
    mixed, valid = LC.case("oor_mixed"), LC.case("oor_valid")
    ws_m = torch.empty(LC.workspace_bytes(mixed), device=dev, dtype=torch.uint8)
    ws_v = torch.empty(LC.workspace_bytes(valid), device=dev, dtype=torch.uint8)
    out_m, d_m = _entry(mixed, dev, ws=ws_m, ws_bytes=ws_m.numel())
    out_v, d_v = _entry(valid, dev, ws=ws_v, ws_bytes=ws_v.numel())
    _check_case("oor_mixed", out_m, d_m, "C entry")
    _check_case("oor_valid", out_v, d_v, "C entry")
    ref, n, refd = _ref("oor_valid")
    _check("oor_mixed against the kernel on the valid rows alone", out_m, d_m, out_v, d_v, *LR.gates(ref, refd))
    assert _match_count(ws_m, mixed) == _match_count(ws_v, valid) == n > 0
    _run("oor_mixed", dev)


def test_all_rows_out_of_range_is_no_targets(dev):
    c = LC.case("oor_all")
    none = dict(c, targets=torch.zeros(0, 6))
    ref, n, refd = _ref("oor_all")
    assert n == 0
    ws = torch.empty(LC.workspace_bytes(c), device=dev, dtype=torch.uint8)
    out_a, d_a = _entry(c, dev, ws=ws, ws_bytes=ws.numel())
    out_0, d_0 = _entry(none, dev)
    _check_case("oor_all", out_a, d_a, "C entry")
    _check("no targets [C entry] vs f64", out_0, d_0, ref, refd)
    _check("oor_all against the kernel without targets", out_a, d_a, out_0, d_0, *LR.gates(ref, refd))
    assert _match_count(ws, c) == 0.0 and float(out_a[1]) == 0.0 and float(out_a[3]) == 0.0
    assert bool((d_a[..., :4] == 0).all()) and bool((d_a[..., 5:] == 0).all())
    _run("oor_all", dev)


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_no_targets_through_the_focal_entry(dev, gamma):
    base = LC.case("oor_all")
    c = dict(base, targets=torch.zeros(0, 6), hyp=dict(base["hyp"], fl_gamma=gamma))
    *ref, n, refd = LR.compute_loss_f64(c["pred"], c["targets"], c["anchors"], c["hyp"], c["gr"], c["nc"])
    assert n == 0 and float(ref[1]) == 0.0 and float(ref[3]) == 0.0
    out, dpred = _entry(c, dev)
    _check(f"nt = 0, gamma {gamma} [C entry] vs f64", out, dpred, ref, refd)
    out, dpred = _wrapper(c, dev)
    _check(f"nt = 0, gamma {gamma} [ComputeLoss] vs f64", out, dpred, ref, refd)
    assert float(out[1]) == 0.0 and float(out[3]) == 0.0


# ---- 8. tiny and ragged launches
@pytest.mark.parametrize("name", ["tiny_3x5", "tiny_ncand130", "tiny_cells257"])
def test_tiny_and_ragged_launches(dev, name):
    _run(name, dev, entry=True)


# ---- 9. the wrapper
BF16_U = 2.0 ** -8          # unit roundoff of bfloat16 (8 significant bits): |round(v) - v| <= u |v|


def test_wrapper_bf16_pred(dev):
    """pred in bf16 with requires_grad: ComputeLoss reads pred.float(), so the restatement is evaluated on those values, and
    the losses meet the usual gates.  The gradient comes back through the .float() as bf16, i.e. the kernel's float32
    gradient rounded to nearest: per element the usual gate plus bf16's unit roundoff 2^-8 times the value."""
    c = LC.case("rect_12x20_plain")
    pb = c["pred"].bfloat16()
    *ref, n, refd = LR.compute_loss_f64(pb.float(), c["targets"], c["anchors"], c["hyp"], c["gr"], c["nc"])
    out, grad = _wrapper(c, dev, pred=pb)
    assert grad.dtype == torch.bfloat16 and grad.shape == pb.shape and grad.is_contiguous()
    g_out, g_d = LR.gates(ref, refd)
    errs = [float((a - b.reshape(-1)).abs().max()) for a, b in zip(out, ref)]
    excess = float(((grad.double() - refd).abs() - BF16_U * refd.abs()).max())
    print(f"bf16 pred ({n} matches): loss errs {[f'{e:.2e}' for e in errs]}; dpred err beyond bf16 rounding {excess:.3e} "
          f"(gate {g_d:.2e}) of max {float(refd.abs().max()):.3e}")
    assert bool(torch.isfinite(grad).all()) and n > 0
    assert all(e <= g for e, g in zip(errs, g_out)), (errs, g_out)
    assert excess <= g_d


def test_wrapper_non_contiguous_pred(dev):
    """pred as the permuted view of a (B, na, no, ny, nx) parent, the way Detect produces it: the gradient arrives in the
    parent's layout."""
    c = LC.case("rect_20x12_focal")
    Lm = importlib.import_module(PKG + ".loss")
    cl = Lm.ComputeLoss(LC.fake_model(c["anchors"], c["hyp"], c["gr"], dev, c["nc"]))
    parent = c["pred"].permute(0, 1, 4, 2, 3).contiguous().to(dev).requires_grad_(True)
    view = parent.permute(0, 1, 3, 4, 2)
    assert not view.is_contiguous() and view.shape == c["pred"].shape
    out = cl([view], c["targets"].to(dev))
    out[0].backward()
    torch.cuda.synchronize()
    assert parent.grad.dtype == torch.float32 and parent.grad.shape == parent.shape and parent.grad.is_contiguous()
    _check_case("rect_20x12_focal", [o.detach().cpu().double() for o in out], parent.grad.permute(0, 1, 3, 4, 2).cpu(), "permuted view")


def test_wrapper_device_scalar_and_retain_graph(dev):
    """loss * (a 0-dim device tensor), backpropagated twice with retain_graph: the incoming gradient is a tensor, not a Python
    scalar, and the second pass adds the same gradient again, exactly."""
    c = LC.case("gr0.5_t4")
    ref, n, refd = _ref("gr0.5_t4")
    Lm = importlib.import_module(PKG + ".loss")
    cl = Lm.ComputeLoss(LC.fake_model(c["anchors"], c["hyp"], c["gr"], dev, c["nc"]))
    pg = c["pred"].to(dev).requires_grad_(True)
    out = cl([pg], c["targets"].to(dev))
    total = out[0] * torch.tensor(1.5, device=dev)
    total.backward(retain_graph=True)
    g1 = pg.grad.clone()
    total.backward(retain_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(pg.grad, 2.0 * g1)
    _check("gr0.5_t4 * 1.5 (device scalar) vs f64", [o.detach().cpu().double() for o in out], g1.cpu(), ref, 1.5 * refd)


# ---- 10. argument rejection: bad arguments only, every buffer is real and large enough for the shape it is called with
def _rejected(entry, c, dev, **kw):
    pred = c["pred"].to(dev)
    dpred, out = torch.full_like(pred, 7.0), torch.full((4,), -3.0, device=dev)
    rc, out, dpred = LC.call_entry(entry, c, dev, gamma=1.5 if entry.endswith("_fl") else None, dpred=dpred, out=out, **kw)
    assert rc != 0, (entry, kw)
    assert bool((dpred == 7.0).all()) and bool((out == -3.0).all()), (entry, kw)


@pytest.mark.parametrize("entry", ["sodt_yolo_loss", "sodt_yolo_loss_fl"])
def test_argument_rejection(dev, entry):
    import ctypes as C
    lib = importlib.import_module(PKG + "._lib").load()
    tiny = LC.case("tiny_3x5")
    roomy = torch.zeros(1 << 20, device=dev, dtype=torch.uint8)
    g = torch.Generator().manual_seed(10)
    tg = LC.case("nc2")["targets"][:2]
    nbytes = C.c_size_t(0)
    assert lib.sodt_yolo_loss_workspace_bytes(48, 2, 33, C.byref(nbytes)) != 0 and nbytes.value == 0
    assert lib.sodt_yolo_loss_workspace_bytes(48, 2, 32, C.byref(nbytes)) == 0 and 0 < nbytes.value < roomy.numel()
    nc33 = dict(tiny, pred=torch.randn(1, 3, 4, 4, 38, generator=g), targets=tg, anchors=LC.YAML_ANCHORS)
    _rejected(entry, nc33, dev, ws=roomy, ws_bytes=roomy.numel())
    na9 = dict(tiny, pred=torch.randn(1, 9, 4, 4, 13, generator=g), targets=tg, anchors=torch.cat((LC.ANCHORS8, LC.ANCHORS8[:1])))
    _rejected(entry, na9, dev, ws=roomy, ws_bytes=roomy.numel())
    need = LC.workspace_bytes(tiny)
    _rejected(entry, tiny, dev, ws=roomy, ws_bytes=need - 1)
    _rejected(entry, tiny, dev, null_targets=True)
    rc, out, dpred = LC.call_entry(entry, tiny, dev, gamma=1.5 if entry.endswith("_fl") else None, ws=roomy, ws_bytes=need)
    assert rc == 0 and bool(torch.isfinite(dpred).all())             # and the same call with the size it asks for runs


# ---- 11. large logits
def test_large_logits(dev):
    """Box logits uniform in [-12, 12], objectness and class logits in [-30, 30]: tiny and huge decoded boxes, atan of
    extreme ratios, saturated BCE; plain and gamma = 2.  No one had measured a bound here, so the gate comes from the
    reference's arithmetic: e32 = |float32 restatement - float64 restatement| on the same inputs (CPU), and the kernel is
    held to 4 * e32 plus the usual gate - forward-mode and autograd derivatives round in different orders.

    Measured (float32 reference error e32 | kernel error on an MI355X; losses: worst of the four, the total):
      large_rand_plain   losses 3.46e-06 | 4.17e-06 of 68.35, dpred 3.742e-06 | 3.742e-06 of max 5.2e-03
      large_rand_focal2  losses 2.45e-06 | 1.37e-06 of 49.70, dpred 3.742e-06 | 3.742e-06 of max 4.4e-03
    The gradient figure is the same on both sides: it comes from one cell whose decoded box is so small that
    (x + w / 2) - (x - w / 2) loses w in float32, whichever way the derivative is taken."""
    for name in ("large_rand_plain", "large_rand_focal2"):
        c = LC.case(name)
        ref, n, refd = _ref(name)
        *o32, n32, d32 = LR.compute_loss_f32(c["pred"], c["targets"], c["anchors"], c["hyp"], c["gr"], c["nc"])
        e32 = [float((a.double() - b).abs().max()) for a, b in zip(o32, ref)]
        e32d = float((d32.double() - refd).abs().max())
        g_out, g_d = LR.gates(ref, refd)
        print(f"{name} ({n} matches): float32 reference vs f64: losses {[f'{e:.2e}' for e in e32]}, dpred {e32d:.3e}")
        assert n == n32 > 0 and bool(torch.isfinite(refd).all()) and bool(torch.isfinite(d32).all())
        out, dpred = _wrapper(c, dev)
        _check(f"{name} [ComputeLoss] vs f64", out, dpred, ref, refd, [4 * e + g for e, g in zip(e32, g_out)], 4 * e32d + g_d)
