"""tests/loss_ref.py and tests/loss_cases.py checked on the CPU, before test_loss_edges_gpu.py relies on them:

(a) compute_loss_f64 against the reference's own ComputeLoss outputs in tests/golden/loss.pt, loss_focal.pt and
    loss_edges.pt (values and dpred).  Bounds: for loss.pt what oracle/gen_golden.py asserts when it writes the file (1e-5,
    1e-6); for the other two the error each case records for the reference against itself (float32 against float64), plus
    1e-12 for the float64 rounding of the restatement; and 1e-12-close to the recorded float64 outputs themselves.
(b) for every case of loss_cases.py, build_targets takes identical decisions in float32 and float64: the same candidates in
    the same order.  A condition, not a measurement.
(c) every case exercises what it is for (its `claims`)."""
import os
from collections import Counter

import pytest
import torch

from oracle import ref_torch as R
import loss_cases as LC
import loss_ref as LR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64_SLACK = 1e-12


def _errs(c, nc=8):
    *ref, n, dpred = LR.compute_loss_f64(c["pred"], c["targets"], c["anchors"], c["hyp"], c["gr"], nc)
    errs = [float((a.reshape(-1).double() - b.reshape(-1)).abs().max()) for a, b in zip(c["out"], ref)]
    return errs, float((c["dpred"].double() - dpred).abs().max()), ref, dpred


def test_restatement_vs_loss_pt():
    for c in torch.load(os.path.join(GOLD, "loss.pt")):
        errs, derr, _, _ = _errs(c)
        print(f"loss.pt {c['targets'].shape[0]} targets: loss errs {[f'{e:.2e}' for e in errs]}, dpred err {derr:.2e}")
        assert max(errs) < 1e-5 and derr < 1e-6


@pytest.mark.parametrize("fixture", ["loss_focal.pt", "loss_edges.pt"])
def test_restatement_vs_recorded_reference_error(fixture):
    cases = torch.load(os.path.join(GOLD, fixture))
    if isinstance(cases, dict):
        cases = [dict(c, **cases["inputs"][c["input"]]) for c in cases["cases"]]
    for c in cases:
        errs, derr, ref, dpred = _errs(c, c.get("nc", 8))
        e64 = float((c["out64"] - torch.cat([r.reshape(-1) for r in ref])).abs().max())
        print(f"{fixture} {c.get('name', '')} gamma {c['hyp']['fl_gamma']}: loss errs {[f'{e:.2e}' for e in errs]} (recorded "
              f"{c['out_ref_err']:.2e}), dpred err {derr:.2e} (recorded {c['dpred_ref_err']:.2e}), vs float64 outputs {e64:.1e}")
        assert max(errs) <= c["out_ref_err"] + F64_SLACK
        assert derr <= c["dpred_ref_err"] + F64_SLACK
        assert e64 <= F64_SLACK
        if "dpred64" in c:
            assert float((c["dpred64"] - dpred).abs().max()) <= F64_SLACK


def test_golden_inputs_are_the_builders():
    """loss_edges.pt holds exactly the cases loss_cases.py marks, on exactly the inputs its builders produce."""
    g = torch.load(os.path.join(GOLD, "loss_edges.pt"))
    assert [c["name"] for c in g["cases"]] == LC.GOLDEN_NAMES
    for gc in g["cases"]:
        c, inp = LC.case(gc["name"]), g["inputs"][gc["input"]]
        assert all(torch.equal(inp[k], c[k]) for k in ("pred", "targets", "anchors")), gc["name"]
        assert gc["hyp"] == c["hyp"] and gc["gr"] == c["gr"] and gc["nc"] == c["nc"]
        assert gc["dpred"].shape == c["pred"].shape and max(c["pred"].shape[2:4]) <= 20 or gc["name"] == "tiny_cells257"


def test_f32_mode_is_the_oracle():
    """compute_loss_f32 with fl_gamma == 0 is oracle.ref_torch.compute_loss, value for value."""
    for name in ("rect_12x20_plain", "gr0.5_t8", "nc1", "posw_rand_1.3_0.8", "crowded_plain"):
        c = LC.case(name)
        *mine, n, dpred = LR.compute_loss_f32(c["pred"], c["targets"], c["anchors"], c["hyp"], c["gr"], c["nc"])
        p = c["pred"].clone().requires_grad_(True)
        ref = R.compute_loss(p, c["targets"], c["anchors"], c["hyp"], c["gr"], c["nc"])
        ref[0].backward()
        assert all(torch.equal(a, b.detach()) for a, b in zip(mine, ref)), name
        assert torch.equal(dpred, p.grad), name


@pytest.mark.parametrize("name", LC.NAMES)
def test_f32_and_f64_decisions_agree(name):
    c = LC.case(name)
    c32 = LR.candidates(c["pred"].shape, c["targets"], c["anchors"], c["hyp"]["anchor_t"], torch.float32)
    c64 = LR.candidates(c["pred"].shape, c["targets"], c["anchors"], c["hyp"]["anchor_t"], torch.float64)
    assert c32 == c64, sorted(set(c32) ^ set(c64))


def _cands(c, targets=None, shape=None):
    return LR.candidates(shape or c["pred"].shape, c["targets"] if targets is None else targets, c["anchors"], c["hyp"]["anchor_t"])


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_exercises_what_it_is_for(name):
    c = LC.case(name)
    assert c["golden"] == (name in LC.GOLDEN_NAMES)
    cl, cand = c["claims"], _cands(c)
    B, na, ny, nx, no = c["pred"].shape
    tg = c["targets"]
    assert no == c["nc"] + 5 and c["pred"].dtype == torch.float32 and tg.dtype == torch.float32
    n = LR.compute_loss_f64(c["pred"], tg, c["anchors"], c["hyp"], c["gr"], c["nc"])[4]
    assert n == len(cand)
    if cl.get("n0"):
        assert n == 0 and tg.shape[0] > 0
        return
    assert n >= 1
    cells = Counter(k[:4] for k in cand)
    if cl.get("dup"):
        assert max(cells.values()) >= 2
    if cl.get("crowd"):
        assert max(cells.values()) >= cl["crowd"] and len(cells) < n / 2
    if cl.get("all_pass"):
        assert tg.shape[0] == 64 and n > na * tg.shape[0]
        assert all(len(_cands(c, tg[i:i + 1])) >= na for i in range(tg.shape[0]))
    if cl.get("corners"):
        for gj, gi in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)):
            assert any(k[2] == gj and k[3] == gi for k in cand), (gj, gi)
    if cl.get("borders"):
        gx, gy = tg[:, 2] * nx, tg[:, 3] * ny
        for near in (gx < 0.5, nx - gx < 0.5, gy < 0.5, ny - gy < 0.5):
            assert any(len(_cands(c, tg[i:i + 1])) > 0 for i in near.nonzero().flatten().tolist())
    if cl.get("swap"):
        assert ny != nx
        swapped = _cands(c, shape=(B, na, nx, ny, no))
        assert set(swapped) != set(cand)
    if cl.get("per_target"):
        for i, want in enumerate(cl["per_target"]):
            assert len(_cands(c, tg[i:i + 1])) == want, (i, tg[i])
    if cl.get("clamp_hi"):
        i = int(((tg[:, 2] * nx >= nx) & (tg[:, 3] * ny >= ny)).nonzero()[0])
        assert all(k[2] == ny - 1 and k[3] == nx - 1 for k in _cands(c, tg[i:i + 1])) and _cands(c, tg[i:i + 1])
    if cl.get("clamp_lo"):
        i = int(((tg[:, 2] * nx <= -1) & (tg[:, 3] * ny <= -1)).nonzero()[0])
        assert all(k[2] == 0 and k[3] == 0 for k in _cands(c, tg[i:i + 1])) and _cands(c, tg[i:i + 1])
    if name.startswith("oor_"):
        b = tg[:, 0].long()
        assert name != "oor_mixed" or {-1, B, B + 3} <= set(b.tolist()) and bool(((b >= 0) & (b < B)).any())


def test_anchor_t_family_grows():
    sets = [set(_cands(LC.case(f"gr0.5_t{t}"))) for t in (2, 4, 8)]
    assert sets[0] < sets[1] < sets[2]
    assert all(torch.equal(LC.case("gr0.0_t4")["pred"], LC.case(f"gr0.5_t{t}")["pred"]) for t in (2, 4, 8))


def test_out_of_range_rows_are_removed():
    a, b, z = LC.case("oor_mixed"), LC.case("oor_valid"), LC.case("oor_all")
    ra = LR.compute_loss_f64(a["pred"], a["targets"], a["anchors"], a["hyp"], a["gr"], a["nc"])
    rb = LR.compute_loss_f64(b["pred"], b["targets"], b["anchors"], b["hyp"], b["gr"], b["nc"])
    rz = LR.compute_loss_f64(z["pred"], z["targets"], z["anchors"], z["hyp"], z["gr"], z["nc"])
    r0 = LR.compute_loss_f64(z["pred"], torch.zeros(0, 6), z["anchors"], z["hyp"], z["gr"], z["nc"])
    assert ra[4] == rb[4] > 0 and all(torch.equal(x, y) for x, y in zip(ra[:4] + ra[5:], rb[:4] + rb[5:]))
    assert rz[4] == r0[4] == 0 and all(torch.equal(x, y) for x, y in zip(rz[:4] + rz[5:], r0[:4] + r0[5:]))
    assert float(rz[1]) == 0.0 and float(rz[3]) == 0.0


def test_tiny_launch_shapes():
    for name, ncells, ncand in (("tiny_3x5", 15, 5), ("tiny_ncand130", 64, 130), ("tiny_cells257", 257, 15)):
        c = LC.case(name)
        B, na, ny, nx, _ = c["pred"].shape
        assert B * na * ny * nx == ncells and 5 * na * c["targets"].shape[0] == ncand
