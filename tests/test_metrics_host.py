"""CPU checks of the validation statistics: the numpy restatement (tests/metrics_ref.py) reproduces every case of
tests/golden/metrics.pt (written by tools/gen_metrics_golden.py from the reference's own helpers), and the host-side
refusals of sodt_amd.metrics."""
import importlib
import os

import numpy as np
import pytest
import torch

import metrics_ref as MR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "metrics.pt")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLD)


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module(pkg.__name__ + ".metrics")


def test_fixture_covers_the_cases(cases):
    tags = {c["tag"] for c in cases}
    assert {"letterbox_clip", "iou_straddle", "duplicate", "duplicate_row_order", "equidistant",
            "class_only_pred_or_label", "empty_images", "nc1", "random"} <= tags
    for c in cases:
        assert len(np.unique(c["det"][:, 4].numpy())) == c["det"].shape[0], "confidences must be distinct"


def test_restatement_reproduces_golden(cases):
    iouv = MR.iouv_np()
    for c in cases:
        correct, tcls = MR.match_np(c["det"].numpy(), c["det_off"].numpy(), c["targets"].numpy(), c["geom"].numpy(), iouv)
        assert np.array_equal(correct, c["correct"].numpy()), c["tag"]
        assert np.array_equal(tcls, c["tcls"].numpy()), c["tag"]
        det = c["det"].numpy()
        p, r, ap, f1, cls = MR.ap_per_class_np(correct.astype(bool), det[:, 4], det[:, 5], tcls)
        for name, v in (("p", p), ("r", r), ("ap", ap), ("f1", f1)):
            assert np.array_equal(v, c[name].numpy()), (c["tag"], name)
        assert np.array_equal(cls, c["ap_class"].numpy()), c["tag"]
        assert np.array_equal(np.bincount(tcls.astype(np.int64), minlength=c["nc"]), c["nt"].numpy()), c["tag"]


def test_golden_pins_the_traps(cases):
    by = {c["tag"]: c for c in cases}
    # a second detection of a matched target is a false positive, whatever its IoU
    for tag in ("duplicate", "duplicate_row_order"):
        d, cls = by[tag]["correct"].numpy(), by[tag]["det"][:, 5].numpy()
        assert d[cls == 0].any(1).sum() == 1 and d[cls == 1].any(1).sum() == 1, tag
    # the walk follows row order, not confidence: the first row wins even with the lower confidence
    ro = by["duplicate_row_order"]
    first = {int(c): i for i, c in reversed(list(enumerate(ro["det"][:, 5].tolist())))}
    assert all(ro["correct"][i].any() for i in first.values())
    # equidistant prediction: the lower target index is taken, the second identical prediction finds it taken
    assert by["equidistant"]["correct"].numpy()[:2].any(1).tolist() == [True, False]
    # a class without predictions keeps an all-zero AP row that still counts
    c5 = by["class_only_pred_or_label"]
    assert c5["ap_class"].tolist() == [0, 1, 2] and not c5["ap"][2].any() and not c5["p"][2]
    # the target row of no image in the batch is not a label
    e = by["empty_images"]
    assert len(e["tcls"]) == len(e["targets"]) - 1


def test_workspace_refusals(ops):
    with pytest.raises(RuntimeError):
        ops.ap_per_class_workspace_bytes(10, 10, 4097)                            # nc above the cap
    with pytest.raises(RuntimeError):
        ops.eval_match_workspace_bytes(0, 10, 10)                                 # no image


def test_ap_per_class_plot_raises(metrics):
    tp = np.zeros((3, 10), bool)
    with pytest.raises(NotImplementedError):
        metrics.ap_per_class(tp, np.ones(3, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32), plot=True)


def test_detection_metrics_refuses_cpu_and_bad_nc(metrics):
    with pytest.raises(RuntimeError):
        metrics.DetectionMetrics(8, "cpu")
    with pytest.raises(ValueError):
        metrics.DetectionMetrics(0, "cuda:0")


def test_geometry_matches_scale_coords(metrics):
    # ratio_pad None: gain and pad computed in double as scale_coords does (general.py:325-327)
    g = metrics._geometry((640, 640), ((375, 500), None))
    assert g == [375.0, 500.0, 1.28, 0.0, (640 - 375 * 1.28) / 2]
    g = metrics._geometry((640, 640), ((375, 500), ((480 / 375, 1.28), (0.0, 80.0))))
    assert g == [375.0, 500.0, 480 / 375, 0.0, 80.0]
