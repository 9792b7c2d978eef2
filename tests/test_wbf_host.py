"""Weighted boxes fusion, host side: the numpy restatement of tests/wbf_ref.py against the reference's own results
(tests/golden/wbf.pt, written by tools/gen_wbf_golden.py), and the argument handling of wbf.py that needs no GPU.

The restatement follows the reference's number formats operation by operation, so every comparison here is exact:
boxes, scores, labels, the number of clusters, and the match decision taken for every candidate."""
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

import wbf_ref as WR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "wbf.pt")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


@pytest.fixture(scope="module")
def wbf(pkg):
    return importlib.import_module(pkg.__name__ + ".wbf")


def test_golden_holds_every_case(gold):
    tags = {c["tag"] for c in gold["weighted_boxes"]}
    assert {"exact_thr_no_match", "exact_thr_step_below", "equal_iou_left_first", "equal_iou_right_first",
            "drift_matches_fused_only", "drift_matches_fused_not_first", "drift_matches_member_only", "zero_intersection", "empty", "rand_nc1_b1",
            "rand_nc3_b3"} <= tags
    by = {c["tag"]: c for c in gold["weighted_boxes"]}
    assert [len(o) for o in by["exact_thr_no_match"]["out"]] == [2] and [len(o) for o in by["exact_thr_step_below"]["out"]] == [1]
    assert tuple(by["empty"]["out"][0].shape) == (0, 6)
    assert by["rand_nc3_b3"]["prediction"].shape[0] == 3 and len(by["rand_nc3_b3"]["out"][1]) == 0
    # the drift chains: the third box joins the fused cluster in two, starts its own in the third
    assert by["drift_matches_fused_only"]["trace"][:3, 1].tolist() == [-1, 0, 0]
    g = next(g for g in gold["fusion"] if g["tag"] == "hand_drift_matches_fused_only")
    a, b, c = g["boxes_list"][0].numpy()[:3]
    thr = g["iou_thr"]
    assert WR.iou_many(a[None], b)[0] > thr > max(WR.iou_many(a[None], c)[0], WR.iou_many(b[None], c)[0])   # neither member alone
    assert g["runs"][0]["trace"][:3, 1].tolist() == [-1, 0, 0] and len(g["runs"][0]["scores"]) == 2
    assert by["drift_matches_fused_not_first"]["trace"][:3, 1].tolist() == [-1, 0, 0]
    assert by["drift_matches_member_only"]["trace"][:3, 1].tolist() == [-1, 0, -1]
    # equal IoU: the candidate goes to the cluster created first, whichever side that one is on
    assert by["equal_iou_left_first"]["trace"][:, 1].tolist() == [-1, -1, 0]
    assert by["equal_iou_right_first"]["trace"][:, 1].tolist() == [-1, -1, 0]
    groups = {g["tag"]: g for g in gold["fusion"]}
    for m in (1, 2, 3):
        runs = groups[f"models_{m}"]["runs"]
        assert {(r["conf_type"], r["allows_overflow"]) for r in runs} == {(c, o) for c in WR.CONF_TYPES for o in (False, True)}


def test_restatement_weighted_boxes_matches_reference(gold):
    for c in gold["weighted_boxes"]:
        trace = []
        out = WR.weighted_boxes(c["prediction"].numpy(), c["image_size"], c["conf_thres"], c["iou_thres"], trace=trace)
        assert len(out) == len(c["out"]), c["tag"]
        for (rows, _), ref in zip(out, c["out"]):
            assert rows.shape == tuple(ref.shape), c["tag"]
            assert np.array_equal(rows, ref.numpy()), c["tag"]
        assert WR.by_label(trace) == WR.by_label(c["trace"].tolist()), c["tag"]


def test_restatement_fusion_matches_reference(gold):
    for g in gold["fusion"]:
        boxes = np.concatenate([b.numpy() for b in g["boxes_list"]])
        scores = np.concatenate([s.numpy() for s in g["scores_list"]])
        labels = np.concatenate([l.numpy() for l in g["labels_list"]])
        models = np.concatenate([np.full(len(s), t) for t, s in enumerate(g["scores_list"])])
        for r in g["runs"]:
            trace = []
            b, s, l, member = WR.fuse(boxes, scores, labels, models, g["weights"], g["iou_thr"], g["skip_box_thr"],
                                      r["conf_type"], r["allows_overflow"], trace=trace)
            tag = (g["tag"], r["conf_type"], r["allows_overflow"])
            assert np.array_equal(b.astype(np.float64), r["boxes"].numpy()), tag
            assert np.array_equal(s, r["scores"].numpy()), tag
            assert np.array_equal(l.astype(np.float64), r["labels"].numpy()), tag
            assert WR.by_label(trace) == WR.by_label(r["trace"].tolist()), tag
            assert (member >= 0).sum() == len(r["trace"]) and member.max() == len(s) - 1


def test_restatement_xyxy_is_the_same_clusters(gold):
    c = next(c for c in gold["weighted_boxes"] if c["tag"] == "rand_nc3_b3")
    a = WR.weighted_boxes(c["prediction"].numpy(), c["image_size"], c["conf_thres"], c["iou_thres"])
    b = WR.weighted_boxes(c["prediction"].numpy(), c["image_size"], c["conf_thres"], c["iou_thres"], xyxy=True)
    for (ra, ma), (rb, mb) in zip(a, b):
        assert np.array_equal(ma, mb) and np.array_equal(ra[:, 4:], rb[:, 4:])
        assert np.allclose((rb[:, 0] + rb[:, 2]) / 2, ra[:, 0], rtol=1e-6) and np.allclose(rb[:, 3] - rb[:, 1], ra[:, 3], rtol=1e-5)


def test_signatures_are_the_reference_s(wbf):
    p = inspect.signature(wbf.weighted_boxes).parameters
    assert list(p) == ["prediction", "image_size", "conf_thres", "iou_thres", "classes", "agnostic", "multi_label", "labels", "xyxy"]
    assert (p["conf_thres"].default, p["iou_thres"].default, p["classes"].default, p["agnostic"].default,
            p["multi_label"].default, p["labels"].default, p["xyxy"].default) == (0.25, 0.45, None, False, False, (), False)
    q = inspect.signature(wbf.weighted_boxes_fusion).parameters
    assert list(q) == ["boxes_list", "scores_list", "labels_list", "weights", "iou_thr", "skip_box_thr", "conf_type",
                           "allows_overflow"]
    assert (q["weights"].default, q["iou_thr"].default, q["skip_box_thr"].default, q["conf_type"].default,
            q["allows_overflow"].default) == (None, 0.55, 0.0, "avg", False)
    for name in ("classes", "agnostic", "multi_label", "labels", "general.py:515"):
        assert name in wbf.weighted_boxes.__doc__


def test_argument_validation(wbf):
    b, s, l = torch.zeros(2, 4), torch.zeros(2), torch.zeros(2)
    with pytest.raises(ValueError, match="conf_type"):
        wbf.weighted_boxes_fusion([b], [s], [l], conf_type="median")
    with pytest.raises(ValueError, match="models"):
        wbf.weighted_boxes_fusion([b] * 33, [s] * 33, [l] * 33)
    with pytest.raises(ValueError, match="models"):
        wbf.weighted_boxes_fusion([], [], [])
    with pytest.raises(ValueError, match="scores"):
        wbf.weighted_boxes_fusion([b], [torch.zeros(3)], [l])
    with pytest.raises(ValueError, match="labels"):
        wbf.weighted_boxes_fusion([b], [s], [torch.zeros(1)])
    with pytest.raises(ValueError, match="per model"):
        wbf.weighted_boxes_fusion([b, b], [s], [l, l])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wbf.weighted_boxes_fusion([b], [s], [l])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wbf.weighted_boxes(torch.zeros(1, 4, 6), 512)


def test_abi_rejects_bad_arguments_without_a_gpu(pkg):
    """SODT_EINVAL paths return before anything is launched, so they can be exercised on the host."""
    import ctypes as C
    lib = pkg._lib.load()
    n = C.c_size_t(0)
    assert lib.sodt_wbf_fuse_workspace_bytes(0, 8, C.byref(n)) != 0
    assert lib.sodt_wbf_fuse_workspace_bytes(1, 0, C.byref(n)) != 0
    assert lib.sodt_wbf_fuse_workspace_bytes(70000, 8, C.byref(n)) != 0
    assert lib.sodt_wbf_fuse_workspace_bytes(2, 1 << 30, C.byref(n)) != 0
    assert lib.sodt_wbf_fuse_workspace_bytes(1, 8, None) != 0
    assert lib.sodt_wbf_candidates(None, 1, 8, 1, 0.25, 512.0, None, None, None, None, None, None) != 0
    w = (C.c_double * 1)(1.0)
    assert lib.sodt_wbf_fuse(None, None, None, None, None, None, 1, 8, w, 1, 0.5, 0.0, 0, 0, 0, None, 0,
                             None, None, None, None, None, None) != 0
