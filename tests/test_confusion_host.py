"""CPU checks of the confusion matrix: the numpy restatement (tests/confusion_ref.py) reproduces every matrix of
tests/golden/confusion.pt (written by tools/gen_confusion_golden.py from the reference's own ConfusionMatrix) with
integer equality, the fixture covers the cases it was built for, and the workspace query answers and refuses."""
import os

import numpy as np
import pytest
import torch

import confusion_ref as CR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "confusion.pt")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLD)


def _restated(c):
    m = np.zeros((c["nc"] + 1, c["nc"] + 1), np.int64)
    for det, lab in c["images"]:
        CR.process_batch_np(m, det.numpy(), lab.numpy(), c["nc"], c["conf"], c["iou_thres"])
    return m


def test_restatement_reproduces_golden(cases):
    for c in cases:
        for det, lab in c["images"]:
            assert CR.tie_free(det.numpy(), lab.numpy(), c["conf"], c["iou_thres"]), c["tag"]
        assert np.array_equal(_restated(c), c["matrix"].numpy()), c["tag"]


def test_fixture_covers_the_cases(cases):
    by = {c["tag"]: c for c in cases}
    assert {"vedai_mix", "nc1", "labels_no_detection_above_conf", "detections_no_labels", "all_miss",
            "detection_over_two_labels", "two_detections_one_label", "reduction_order", "wrong_class", "at_conf",
            "iou_ulp", "iou_ulp_06"} <= set(by)
    assert by["vedai_mix"]["nc"] == 8 and len(by["vedai_mix"]["images"]) > 1 and by["nc1"]["nc"] == 1
    nc = 8
    # labels and no detection above conf: both labels of the first image are missed, nothing else is counted for it
    m = by["labels_no_detection_above_conf"]["matrix"]
    assert m[nc, 2] == 1 and m[nc, 3] == 1 and m[2, 2] == 1 and m.sum() == 3
    # detections and no labels: the first image adds nothing
    assert by["detections_no_labels"]["matrix"].sum() == 1
    # every detection misses: no [dc, nc] count at all, although three detections are kept (metrics.py:152)
    m = by["all_miss"]["matrix"]
    assert m[:, nc].sum() == 0 and m[nc].sum() == 3
    # a detection over two labels keeps the closer one
    m = by["detection_over_two_labels"]["matrix"]
    assert m[3, 3] == 1 and m[nc, 4] == 1 and m.sum() == 2
    # two detections on a label: one match, the others background
    m = by["two_detections_one_label"]["matrix"]
    assert m[2, 2] == 1 and m[2, nc] == 1 and m[7, nc] == 1 and m.sum() == 3
    # reduction order: A loses L1 to B in the second pass and does not fall back to L2
    m = by["reduction_order"]["matrix"]
    assert m[1, 5] == 1 and m[nc, 6] == 1 and m[1, nc] == 1 and m.sum() == 3
    # wrong classes land off the diagonal at [gt class, detection class]
    m = by["wrong_class"]["matrix"]
    assert m[1, 0] == 1 and m[2, 7] == 1 and m[6, 6] == 1
    # conf and iou_thres are strict, in float32
    for tag in ("at_conf", "iou_ulp", "iou_ulp_06"):
        m = by[tag]["matrix"]
        assert m.diagonal()[:nc].sum() == 1 and m[nc].sum() == 2 and m.sum() == 3, tag


def test_tie_rule_of_the_restatement():
    # one detection exactly as close to two labels: the lower label index; two identical detections: the lower one
    lab = np.array([[1, 100, 100, 124, 120], [2, 116, 100, 140, 120]], np.float32)
    det = np.array([[100, 100, 140, 120, 0.9, 3], [100, 100, 140, 120, 0.8, 4]], np.float32)
    assert not CR.tie_free(det, lab)
    m = np.zeros((9, 9), np.int64)
    CR.process_batch_np(m, det, lab, 8)
    assert m[1, 3] == 1 and m[8, 2] == 1 and m[4, 8] == 1 and m.sum() == 3


def test_new_symbols_exported(pkg, ops):
    assert callable(ops.confusion_update) and callable(ops.confusion_workspace_bytes)
    assert ops.confusion_workspace_bytes(8, 2400, 300) > 0
    with pytest.raises(RuntimeError):
        ops.confusion_workspace_bytes(0, 10, 10)                                  # no image
