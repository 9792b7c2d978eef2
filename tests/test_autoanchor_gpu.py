"""Autoanchor on the GPU (csrc/autoanchor.hip, autoanchor.py): the three entries against the numpy restatement of
tests/autoanchor_ref.py and against the vectors captured from the reference and scipy (tests/golden/autoanchor.pt), and
check_anchors end to end on the small Model.  Nothing here reads the reference or scipy.

Tolerances: counts are integers and must be equal.  Sums are float64 sums of float32 values added in another order than
numpy's: 1e-12 relative (N * n <= 1.1e6 terms of equal sign, so the worst case is far below that).  Code books are means
in float64 after at most a few dozen iterations: 1e-9 relative, as the issue sets it.  Against the reference's stored
anchors 1e-6 relative."""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import autoanchor_ref as AR  # noqa: E402
from test_model_gpu import build  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "small-object-detection-transformers_amd"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "autoanchor.pt")
EVOLVE_TAGS = ["evolve_n9_thr4.0", "evolve_n9_thr2.91", "evolve_n3_thr4.0", "evolve_n3_thr2.91"]
N_TWICE = 33000            # above 128 blocks x 256 threads: the grid-stride loop of the metric kernels runs twice


@pytest.fixture(scope="module")
def AA(pkg):
    return importlib.import_module(PKG + ".autoanchor")


@pytest.fixture(scope="module")
def cases():
    return {c["tag"]: c for c in torch.load(GOLD, weights_only=False)["cases"]}


@pytest.fixture(scope="module")
def restated(cases):
    """The restatement of every golden case, computed once: tag -> (k or None, info)."""
    out = {}
    for tag, c in cases.items():
        if c["book"] is None:
            continue
        np.random.seed(c["seed"])
        np.random.uniform(0.9, 1.1, size=(len(c["shapes"]), 1))
        out[tag] = AR.kmean_anchors(c["shapes"].numpy(), [l.numpy() for l in c["labels"]], c["n"], c["imgsz"], c["thr"], c["gen"])
    return out


def labels_wh(N, seed):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(2.0), np.log(500.0), (N, 2))).astype(np.float32)


def anchor_sets(S, n, seed):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(3.0), np.log(400.0), (S, n, 2))).astype(np.float32)


def run_stats(ops, dev, wh, sets, thr_inv, fill=None):
    w = torch.from_numpy(np.ascontiguousarray(wh, dtype=np.float32)).to(dev).reshape(-1, 2)
    s = torch.from_numpy(np.ascontiguousarray(sets, dtype=np.float32)).to(dev)
    out = torch.full((s.shape[0], 6), -7.0 if fill is None else fill, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.anchor_stats_workspace_bytes(w.shape[0], s.shape[0]), dtype=torch.uint8, device=dev)
    ops.anchor_stats(w, s, thr_inv, ws, out)
    return out.cpu().numpy()


def rel_close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= tol * np.abs(b)).all())


# ---- sodt_anchor_stats ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1025, N_TWICE])
def test_stats_match_the_restatement(ops, dev, N):
    wh = labels_wh(N, N)
    for n in (1, 3, 9, 32):
        for S in (1, 30):
            for thr in (4.0, 2.91):
                if thr == 2.91 and (N == N_TWICE or S == 30) and n != 9:
                    continue                                   # the second threshold on every N, n and S, not on every product
                sets = anchor_sets(S, n, 100 * n + S)
                got = run_stats(ops, dev, wh, sets, 1.0 / thr)
                again = run_stats(ops, dev, wh, sets, 1.0 / thr, fill=3.0)
                assert np.array_equal(got, again), (N, n, S)                       # bit-identical on a second run
                for s in range(S):
                    want = AR.stats(wh, sets[s], 1.0 / thr)
                    assert (got[s, 2], got[s, 3]) == (want[2], want[3]), (N, n, S, s, thr, got[s], want)
                    assert rel_close(got[s, [0, 1, 4, 5]], [want[0], want[1], want[4], want[5]], 1e-12), (N, n, S, s, got[s], want)


def test_stats_boundaries(ops, dev):
    # exactly on the threshold: 4 / 16 = 0.25 is not > 0.25
    got = run_stats(ops, dev, [[4.0, 4.0]], [[[16.0, 16.0]]], 0.25)[0]
    assert got.tolist() == [0.25, 0.0, 0.0, 0.0, 0.25, 0.0]
    # one float32 step inside it
    got = run_stats(ops, dev, [[np.nextafter(np.float32(4), np.float32(5)), 4.5]], [[[16.0, 16.0]]], 0.25)[0]
    assert got[2] == 1 and got[3] == 1
    # two anchors with the same ratio 0.5, one from above and one from below
    got = run_stats(ops, dev, [[8.0, 8.0]], [[[16.0, 16.0], [4.0, 4.0]]], 0.25)[0]
    assert got.tolist() == [0.5, 0.5, 1.0, 2.0, 1.0, 1.0]
    # 1 / 2.91 is inexact in float32 and rounds UP: a ratio equal to float32(1 / 2.91) is past the float64 quotient, and
    # not past the threshold torch compares with
    t = 1.0 / 2.91
    t32 = np.float32(t)
    assert float(t32) > t
    got = run_stats(ops, dev, [[t32 * np.float32(16), 16.0]], [[[16.0, 16.0]]], t)[0]
    assert got[2] == 0 and got[3] == 0 and got[0] == float(t32)
    got = run_stats(ops, dev, [[np.nextafter(t32, np.float32(1)) * np.float32(16), 16.0]], [[[16.0, 16.0]]], t)[0]
    assert got[2] == 1 and got[3] == 1


def test_stats_refuses_33_anchors(ops, dev):
    wh = labels_wh(100, 1)
    with pytest.raises(RuntimeError, match="sodt_anchor_stats failed with status 1"):
        run_stats(ops, dev, wh, anchor_sets(1, 33, 0), 0.25)
    w = torch.from_numpy(wh).to(dev)
    s = torch.from_numpy(anchor_sets(1, 33, 0)).to(dev)
    out = torch.full((1, 6), -7.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    rc = ops._lib.sodt_anchor_stats(w.data_ptr(), 100, s.data_ptr(), 1, 33, 0.25, ws.data_ptr(), 4096, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 1 and out.cpu().tolist() == [[-7.0] * 6]


def test_anchor_metric(AA, dev):
    wh = labels_wh(500, 2)
    sets = anchor_sets(4, 5, 3)
    bpr, aat = AA.anchor_metric(torch.from_numpy(wh).to(dev), torch.from_numpy(sets).to(dev), thr=4.0)
    for s in range(4):
        want = AR.stats(wh, sets[s], 0.25)
        assert float(bpr[s]) == want[2] / 500 and float(aat[s]) == want[3] / 500
    b0, a0 = AA.anchor_metric(torch.from_numpy(wh).to(dev), sets[0], thr=4.0)
    assert b0.dim() == 0 and float(b0) == float(bpr[0]) and float(a0) == float(aat[0])


# ---- sodt_anchor_evolve --------------------------------------------------------------------------------------------
def run_evolve(ops, dev, wh, k0, thr_inv, v):
    """The call under sync debug mode "error": any host read inside it raises."""
    w = torch.from_numpy(np.ascontiguousarray(wh, dtype=np.float32)).to(dev)
    k = torch.from_numpy(np.array(k0, dtype=np.float64)).to(dev)
    n, G = k.shape[0], len(v)
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).reshape(G, n, 2)).to(dev)
    st = torch.empty(1, 6, dtype=torch.float64, device=dev)
    ws0 = torch.empty(ops.anchor_stats_workspace_bytes(len(wh), 1), dtype=torch.uint8, device=dev)
    ops.anchor_stats(w, k.float().view(1, n, 2), thr_inv, ws0, st)
    f = (st[0, 1:2] / torch.tensor(float(len(wh)), dtype=torch.float64, device=dev)).contiguous()      # a true division
    acc = torch.full((max(G, 1),), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.anchor_evolve_workspace_bytes(len(wh)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.anchor_evolve(w, thr_inv, k, f, vd, acc, ws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return k.cpu().numpy(), float(f.cpu()), acc.cpu().numpy()[:G]


@pytest.mark.parametrize("tag", EVOLVE_TAGS)
def test_evolve_golden(ops, dev, cases, restated, tag):
    c = cases[tag]
    k_ref, info = restated[tag]
    k, f, acc = run_evolve(ops, dev, info["wh"], info["k0"], 1.0 / c["thr"], info["v"])
    assert np.array_equal(acc.astype(bool), info["accepted"]), np.nonzero(acc.astype(bool) != info["accepted"])
    assert rel_close(k, info["k_unsorted"], 1e-12) and rel_close(f, info["f"], 1e-12)
    ks = k[np.argsort(k.prod(1))]
    assert rel_close(ks, c["k"].numpy(), 1e-6)


def test_evolve_zero_and_one_generation(ops, dev):
    wh = labels_wh(300, 7)
    k0 = anchor_sets(1, 5, 8)[0].astype(np.float64)
    k, f, acc = run_evolve(ops, dev, wh, k0, 0.25, np.zeros((0, 5, 2)))
    assert np.array_equal(k, k0) and f == pytest.approx(AR.fitness(wh, k0, 0.25), rel=1e-12) and len(acc) == 0
    np.random.seed(3)
    v = AR.draw_mutations(6, (5, 2))
    for g in range(6):                                           # G = 1, taken or not
        want_k, want_f, want_acc, _ = AR.evolve(wh, k0, 0.25, v[g:g + 1])
        k, f, acc = run_evolve(ops, dev, wh, k0, 0.25, v[g:g + 1])
        assert acc.tolist() == want_acc.astype(int).tolist() and rel_close(k, want_k, 1e-12) and rel_close(f, want_f, 1e-12)


def test_evolve_clip_engages(ops, dev):
    """Anchors near 2.0: the mutated anchors are clipped from below, in float64, before they are rounded to float32."""
    rng = np.random.default_rng(11)
    wh = np.exp(rng.uniform(np.log(1.0), np.log(3.0), (400, 2))).astype(np.float32)       # labels the smallest anchors fit best
    k0 = np.array([[2.0, 2.05], [2.1, 3.0], [4.0, 2.02]])
    np.random.seed(4)
    v = AR.draw_mutations(40, (3, 2))
    want_k, want_f, want_acc, _ = AR.evolve(wh, k0, 0.25, v)
    assert (k0 * v < 2.0).any((1, 2)).sum() >= 10               # already from the start anchors many proposals go below 2.0
    assert (want_k == 2.0).any() and want_acc.sum() >= 3        # and clipped proposals were taken
    k, f, acc = run_evolve(ops, dev, wh, k0, 0.25, v)
    assert np.array_equal(acc.astype(bool), want_acc) and rel_close(k, want_k, 1e-12) and rel_close(f, want_f, 1e-12)
    assert (k >= 2.0).all() and (k == 2.0).any()


def test_evolve_many_blocks(ops, dev):
    wh = labels_wh(N_TWICE, 12)
    k0 = anchor_sets(1, 9, 13)[0].astype(np.float64)
    np.random.seed(6)
    v = AR.draw_mutations(20, (9, 2))
    want_k, want_f, want_acc, margins = AR.evolve(wh, k0, 1.0 / 2.91, v)
    assert margins.min() > 1e-9                                  # the order of addition cannot turn a decision
    k, f, acc = run_evolve(ops, dev, wh, k0, 1.0 / 2.91, v)
    k2, f2, acc2 = run_evolve(ops, dev, wh, k0, 1.0 / 2.91, v)
    assert np.array_equal(acc.astype(bool), want_acc) and rel_close(k, want_k, 1e-12) and rel_close(f, want_f, 1e-12)
    assert np.array_equal(k, k2) and f == f2 and np.array_equal(acc, acc2)


# ---- sodt_kmeans_lloyd ---------------------------------------------------------------------------------------------
def run_kmeans(AA, dev, obs, idx, chunk):
    o = torch.from_numpy(np.ascontiguousarray(obs)).to(dev)
    books, alive, curs, live = AA._kmeans_device(o, torch.from_numpy(np.ascontiguousarray(idx)).to(dev), chunk)
    return books.cpu().numpy(), alive.cpu().numpy().astype(bool), curs, live


@pytest.mark.parametrize("tag", EVOLVE_TAGS + ["fewer_n9"])
def test_kmeans_golden(AA, dev, cases, restated, tag):
    c = cases[tag]
    info = restated[tag][1]
    want = c["book"].numpy()
    books, alive, curs, live = run_kmeans(AA, dev, info["obs"], info["idx"], 8)
    win = int(np.argmin(curs))
    # (a distortion that is zero in exact arithmetic is a few 1e-17 here or there: hence the absolute term)
    assert win == info["winner"] and np.allclose(curs, info["curs"], rtol=1e-9, atol=1e-12)
    assert live[win] == len(want) and rel_close(books[win][alive[win]], want, 1e-9)
    if tag == "fewer_n9":
        assert live[win] == c["n"] - 1                           # a centre died; the others keep scipy's order
    # chunks of 1 and of 8 iterations: a restart that is done is not touched again
    books1, alive1, curs1, live1 = run_kmeans(AA, dev, info["obs"], info["idx"], 1)
    assert np.array_equal(books, books1) and np.array_equal(alive, alive1) and np.array_equal(curs, curs1)
    # the winning restart alone
    b, a, cur, lv = run_kmeans(AA, dev, info["obs"], info["idx"][win:win + 1], 8)
    assert np.array_equal(b[0], books[win]) and cur[0] == curs[win] and rel_close(b[0][a[0]], want, 1e-9)


def test_kmeans_done_restart_is_frozen(ops, dev, restated):
    info = restated["evolve_n9_thr4.0"][1]
    obs = torch.from_numpy(info["obs"]).to(dev)
    idx = torch.from_numpy(info["idx"][:4]).to(dev)
    books = obs[idx].contiguous()
    before = books.clone()
    alive = torch.ones(4, 9, dtype=torch.int32, device=dev)
    prev = torch.full((4,), float("inf"), dtype=torch.float64, device=dev)
    done = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.kmeans_lloyd_workspace_bytes(obs.shape[0], 4, 9), dtype=torch.uint8, device=dev)
    ops.kmeans_lloyd(obs, books, alive, prev, done, 1e-5, 3, ws)
    assert torch.equal(books[1], before[1]) and torch.equal(books[3], before[3])
    assert not torch.equal(books[0], before[0]) and prev.cpu().tolist()[1] == float("inf")
    want = info["obs"][info["idx"][0]].copy()
    al, p = np.ones(9, bool), np.inf
    for _ in range(3):
        p, _ = AR.lloyd_step(info["obs"], want, al, p)
    assert rel_close(books[0].cpu().numpy(), want, 1e-9) and rel_close(float(prev[0]), p, 1e-9)


def test_kmeans_tie_goes_to_the_lowest_live_index(ops, dev):
    """Two centres on the same point: the first takes every member, the second dies and keeps its slot."""
    obs = torch.tensor([[0.0, 0.0], [0.0, 1.0], [4.0, 4.0], [4.0, 5.0], [0.0, 0.5]], dtype=torch.float64, device=dev)
    books = torch.tensor([[[0.0, 0.0], [0.0, 0.0], [4.0, 4.0]]], dtype=torch.float64, device=dev)
    alive = torch.ones(1, 3, dtype=torch.int32, device=dev)
    prev = torch.full((1,), float("inf"), dtype=torch.float64, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.kmeans_lloyd_workspace_bytes(5, 1, 3), dtype=torch.uint8, device=dev)
    ops.kmeans_lloyd(obs, books, alive, prev, done, 1e-5, 1, ws)
    assert alive.cpu().tolist() == [[1, 0, 1]] and done.cpu().tolist() == [0]
    assert books.cpu().tolist() == [[[0.0, 0.5], [0.0, 0.0], [4.0, 4.5]]]
    assert float(prev) == (0.0 + 1.0 + 0.0 + 1.0 + 0.5) / 5


# ---- check_anchors end to end --------------------------------------------------------------------------------------
def dataset_of(c):
    return types.SimpleNamespace(shapes=c["shapes"].numpy(), labels=[l.numpy() for l in c["labels"]])


def quiet_check(AA, c, model):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        AA.check_anchors(dataset_of(c), model, thr=c["thr"], imgsz=c["imgsz"])
    return buf.getvalue()


def test_check_anchors_keeps_fitting_anchors(AA, dev, cases):
    c = cases["keep_n3"]
    model, _ = build(dev, 128)
    det = model.detect[-1]
    a0, g0 = det.anchors.clone(), det.anchor_grid.clone()
    np.random.seed(c["seed"])
    out = quiet_check(AA, c, model)
    state = np.random.get_state()
    assert torch.equal(det.anchors, a0) and torch.equal(det.anchor_grid, g0) and "Attempting to improve" not in out
    np.random.seed(c["seed"])
    np.random.uniform(0.9, 1.1, size=(len(c["shapes"]), 1))
    want = np.random.get_state()
    assert state[0] == want[0] and np.array_equal(state[1], want[1]) and state[2:] == want[2:]      # only the scale draw


def test_check_anchors_replaces_anchors_everywhere(AA, dev, cases, monkeypatch):
    from oracle import ref_torch as R
    LS = importlib.import_module(PKG + ".loss")
    c = cases["evolve_n3_thr4.0"]
    real = AA.kmean_anchors
    monkeypatch.setattr(AA, "kmean_anchors", lambda path, **kw: real(path, **dict(kw, gen=c["gen"])))
    model, _ = build(dev, 128)
    model.compute_dtype = torch.float32
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    det = model.detect[-1]
    loss_before = LS.ComputeLoss(model)                          # built before the anchors change
    x_rgb, x_ir = R.synthetic_inputs(1, 128, seed=2)
    xr, xi = x_rgb.to(dev), x_ir.to(dev)
    model.eval()
    with torch.no_grad():
        z_old, praw_old, _ = model(xr, xi, "RGB+IR")             # the engine exists, and has decoded with the old anchors
    g0 = det.anchor_grid.clone()
    np.random.seed(c["seed"])
    out = quiet_check(AA, c, model)
    assert "New anchors saved to model" in out
    got = det.anchor_grid.view(-1, 2).cpu().numpy()
    assert rel_close(got, c["anchor_grid"].view(-1, 2).numpy(), 1e-6) and not torch.equal(det.anchor_grid, g0)
    assert rel_close(det.anchors.cpu().numpy(), c["anchors"].numpy(), 1e-6)
    assert torch.equal(det.anchors, det.anchor_grid.view(1, -1, 2) / model.stride.to(dev).view(-1, 1, 1))
    # the eval forward decodes with the new anchor_grid: the engine holds no stale copy
    with torch.no_grad():
        z, praw, _ = model(xr, xi, "RGB+IR")
    want = R.detect_decode(praw[0].float().cpu(), det.anchor_grid.cpu())
    stale = R.detect_decode(praw[0].float().cpu(), g0.cpu())
    err = float((z.cpu() - want).abs().max() / want.abs().max())
    # f32 decode with the hardware exp / rcp: a few 1e-7 relative per factor; the stale anchors would be off by O(1)
    assert err < 1e-4 and float((z.cpu() - stale).abs().max()) > 1e-2 * float(want.abs().max()), err
    # a ComputeLoss built before the call sees the new anchors
    targets = LS.synthetic_targets(1, 16, 8, seed=1).to(dev)
    pred = praw[0].float().contiguous()
    l_before = [t.detach().cpu() for t in loss_before(pred, targets)]
    l_after = [t.detach().cpu() for t in LS.ComputeLoss(model)(pred, targets)]
    assert all(torch.equal(a, b) for a, b in zip(l_before, l_after))
    assert loss_before.anchors.data_ptr() == det.anchors.data_ptr()


def test_check_anchors_keeps_originals_when_the_new_ones_are_worse(AA, dev, cases, monkeypatch):
    c = cases["evolve_n3_thr2.91"]
    monkeypatch.setattr(AA, "kmean_anchors", lambda path, **kw: np.array([[2.0, 2.0], [2.0, 3.0], [3.0, 2.0]]))
    model, _ = build(dev, 128)
    det = model.detect[-1]
    a0, g0 = det.anchors.clone(), det.anchor_grid.clone()
    out = quiet_check(AA, c, model)
    assert torch.equal(det.anchors, a0) and torch.equal(det.anchor_grid, g0) and "Original anchors better" in out


def test_check_anchors_keeps_originals_when_a_centre_dies(AA, dev, cases):
    c = cases["fewer_n9"]
    a = c["anchors0"].clone().view(1, -1, 2).to(dev)
    m = types.SimpleNamespace(anchors=a / c["stride"], anchor_grid=a.clone().view(1, 1, -1, 1, 1, 2),
                              stride=torch.tensor([c["stride"]]))
    np.random.seed(c["seed"])
    out = quiet_check(AA, c, types.SimpleNamespace(detect=[m]))
    assert "requested 9 points but returned only 8" in out and "Original anchors better" in out
    assert torch.equal(m.anchor_grid.view(-1, 2).cpu(), c["anchors0"])
