"""--image-weights without a GPU: the restatement of tests/sampling_ref.py against the reference's recorded results
(tests/golden/sampling.pt, written by tools/gen_sampling_golden.py), `broadcast_indices` between two gloo ranks, the
refusals of sampling.py that need no device, and the new prototypes in header and ABI table.

Bounds (u = 2^-53).  The fixture stores the reference's float64 results, and the restatement performs the reference's numpy
operations, so class weights, cw and image weights must come out with the stored bits; the tests still only ask for the
bound that holds for ANY order of the sums, which is the one the device is held to in tests/test_sampling_gpu.py:
  class weights   2 nc u relative: two orders of the nc-term sum of reciprocals differ by 2 (nc - 1) u, each quotient rounds once;
  image weights   4 nc u relative to the stored value: non-negative terms, (nc - 1) u each way, doubled for two orders."""
import importlib
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as SR  # noqa: E402
from test_abi_and_host import header_prototypes  # noqa: E402

PKG = "small-object-detection-transformers_amd"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling.pt")
CASES = torch.load(GOLDEN)["cases"]
U = SR.U


def case_labels(c):
    """The fixture's labels as the loader holds them: one (m, 5) array per image."""
    return np.split(c["labels"].numpy(), np.cumsum(c["lens"].numpy())[:-1])


def test_the_fixture_covers_what_the_feature_must_handle():
    assert sorted({c["nc"] for c in CASES}) == [1, 8, 80]
    assert sorted({len(c["lens"]) for c in CASES}) == [1, 2, 65, 1025, 3077]
    assert any(c["k"] < len(c["lens"]) for c in CASES) and any(c["k"] > len(c["lens"]) for c in CASES)
    big = [c for c in CASES if len(c["lens"]) > 2]
    assert all(c["lens"][0] == 0 and c["lens"][-1] == 0 for c in big)                   # images without labels
    assert all(len(set(c["labels"][:, 0].tolist())) < c["nc"] for c in big)             # a class without labels
    assert all(0.0 in c["maps"].tolist() and 1.0 in c["maps"].tolist() for c in big)


@pytest.mark.parametrize("c", CASES, ids=[c["tag"] for c in CASES])
def test_restatement_reproduces_the_reference(c):
    labels, nc = case_labels(c), c["nc"]
    cwt = SR.labels_to_class_weights(labels, nc)
    ref = c["class_weights"].numpy()
    assert cwt.dtype == np.float64 and np.all(np.abs(cwt - ref) <= 2 * nc * U * ref)
    random.seed(c["seed"])
    cw, iw, idx = SR.epoch(labels, nc, c["model_class_weights"].numpy(), c["maps"].numpy(), c["k"])
    assert np.array_equal(cw, c["cw"].numpy())                                           # Train.py:339, the same expression
    ref = c["image_weights"].numpy()
    assert iw.shape == (len(labels),) and np.all(np.abs(iw - ref) <= 4 * nc * U * ref)
    assert idx == c["indices"].tolist()
    assert random.getstate() == c["state"]


def test_restated_choices_is_the_stdlibs():
    w = [0.0, 0.5, 0.0, 0.0, 0.25, 1.25, 0.0]
    random.seed(7)
    want = random.choices(range(len(w)), weights=w, k=50)
    state = random.getstate()
    random.seed(7)
    got, cum = SR.choices(w, 50)
    assert got == want and random.getstate() == state and cum[-1] == 2.0
    assert not {0, 2, 3, 6} & set(got)                                                   # zero-weight entries are never drawn
    for bad, msg in (([0.0, 0.0], "greater than zero"), ([1.0, float("inf")], "finite"), ([1.0, float("nan")], "finite")):
        with pytest.raises(ValueError, match=msg):
            SR.choices(bad, 1)
        with pytest.raises(ValueError, match=msg):
            random.choices(range(2), weights=bad, k=1)


def test_device_cum_is_a_prefix_sum_in_another_order():
    """The documented scan order, recomputed on the host, against np.cumsum: exact on integers, within the bound otherwise."""
    W = importlib.import_module(PKG + "._lib").CHOICES_BLOCK
    for n in (1, 2, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5):
        a = torch.arange(1, n + 1, dtype=torch.float64)
        assert torch.equal(SR.device_cum(a, W), torch.cumsum(a, 0))
        a = torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
        ref = np.cumsum(a.numpy())
        assert np.all(np.abs(SR.device_cum(a, W).numpy() - ref) <= 2 * max(n - 1, 0) * U * ref)


def test_python_layer_refusals_that_need_no_device():
    S = importlib.import_module(PKG + ".sampling")
    out = S.labels_to_class_weights([None], 8)                                           # general.py:222-223
    assert isinstance(out, torch.Tensor) and out.numel() == 0
    for bad in ([], [None]):
        with pytest.raises(ValueError, match="loaded labels"):
            S.ImageWeights(bad, 8)
    with pytest.raises(ValueError, match="nc must be"):
        S.ImageWeights([np.zeros((1, 5))], 0)
    with pytest.raises(ValueError, match=r"shape \(3,\), expected \(8,\)"):
        S._host_f64(np.ones(3), 8, "maps")
    with pytest.raises(ValueError, match="shape"):
        S._host_f64(torch.ones(2, 8), 8, "class_weights")
    assert S._host_f64(torch.ones(8), 8, "maps").dtype == np.float64
    with pytest.raises(RuntimeError, match="process group"):
        S.broadcast_indices([0, 1], 2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.ImageWeights([np.zeros((1, 5))], 8)
    # the normalising sum of the class weights: a tree of element-wise additions, exact on integers
    for n in (1, 2, 3, 8, 80):
        assert float(S.tree_sum(torch.arange(1, n + 1, dtype=torch.float64))) == n * (n + 1) / 2


def test_new_entries_are_in_the_header_and_the_table(pkg):
    protos, L = header_prototypes(), pkg._lib
    for name in ("sodt_class_counts", "sodt_image_weights", "sodt_weighted_choices"):
        assert name in protos and name in L.SIGNATURES
        assert len(protos[name][1]) == len(L.SIGNATURES[name])
        assert hasattr(L.load(), name)
    assert "sodt_weighted_choices_workspace_bytes" in protos and "sodt_weighted_choices_workspace_bytes" in L.SIGNATURES
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "sodt_hip.h")).read()
    assert f"#define SODT_CHOICES_BLOCK {L.CHOICES_BLOCK}\n" in src
    for name in ("BAD_CLASS", "BAD_IMAGE", "ZERO_TOTAL", "NONFINITE_TOTAL"):
        assert f"#define SODT_SAMPLING_{name} {getattr(L, 'SAMPLING_' + name)}\n" in src


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    S = importlib.import_module(PKG + ".sampling")
    want = [5, 0, 5, 3, 2, 16777215, 1]
    got = S.broadcast_indices(want if rank == 0 else None, len(want))
    ok = got == want and all(type(i) is int for i in got)
    got = S.broadcast_indices(want[::-1] if rank == 1 else None, len(want), src=1)      # another source rank
    ok = ok and got == want[::-1]
    if rank == 0:                                                                        # refused before the collective
        try:
            S.broadcast_indices(want, len(want) + 1)
            ok = False
        except ValueError:
            pass
    q.put((rank, ok))
    dist.destroy_process_group()


def test_broadcast_indices_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in ps:
        p.join(60)
    assert res == {0: True, 1: True}
