"""Write tests/golden/autoanchor.pt: the reference's own `check_anchors` / `kmean_anchors` (basics/utils/autoanchor.py) run
on small synthetic data sets.  Runs only where the reference source tree and scipy are importable (the build machine);
it reads oracle.gen_golden.import_reference() for the module stubs, as tools/gen_wbf_golden.py does, and changes nothing
under oracle/.

The fixture holds inputs and results only.  Per case: the seed given to np.random.seed before the call, `shapes`
(n_img, 2), `labels` (one (m, 5) array per image), `thr`, `imgsz`, `n`, `gen`, the starting `anchors0` (n, 2) in pixels and
`stride`; the reference's `bpr` / `aat` of the starting anchors; `book`, the code book scipy.cluster.vq.kmeans returned
(captured by wrapping the module's `kmeans`; None where k-means never ran); `k`, the anchors kmean_anchors returned (None
where it raised or never ran); `anchors` / `anchor_grid` of the Detect stand-in afterwards; and `stdout`, what the call
printed.  The random state after the call is not stored: tests/test_autoanchor_host.py re-runs the reference for it.

Cases: n = 9 and n = 3 (the `na` of models/model.yaml) with thr 4.0 and 2.91, gen = 300, 200-260 labels; one case whose
starting anchors already reach BPR >= 0.98 (nothing recomputed); one whose labels repeat n - 1 points, so that a centre
dies and k-means returns fewer than n centres.

A seed is taken only if, measured on the restatement of tests/autoanchor_ref.py (which must first reproduce the
reference's code book and anchors exactly):
  * every generation has |fg - f| >= 1e-6 (the reference forms the fitness mean in float32, the device in float64);
  * every k-means stop decision has |diff - 1e-5| >= 1e-9;
  * the winning restart beats every other by >= 1e-9 in its final distortion (the device adds in another order, and two
    restarts that reach the same minimum would otherwise leave the winner to rounding).
The margins found are printed.

usage: python tools/gen_autoanchor_golden.py
"""
from __future__ import annotations

import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import autoanchor_ref as AR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "autoanchor.pt")
ANCHORS9 = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
ANCHORS3 = [10, 13, 16, 30, 33, 23]                       # models/model.yaml
STRIDE = 4.0


def dataset(rng, n_img, per_img, lo, hi, aspect):
    """Images of mixed shapes with log-uniform label sizes (normalised) of log-uniform aspect ratio."""
    shapes = np.stack([rng.choice([384, 480, 512, 640], n_img), rng.choice([384, 480, 512, 640], n_img)], 1).astype(np.float64)
    labels = []
    for _ in range(n_img):
        m = int(rng.integers(per_img[0], per_img[1] + 1))
        size = np.exp(rng.uniform(np.log(lo), np.log(hi), m))
        asp = np.exp(rng.uniform(-np.log(aspect), np.log(aspect), m))
        l = np.zeros((m, 5))
        l[:, 0] = rng.integers(0, 8, m)
        l[:, 1:3] = rng.uniform(0.1, 0.9, (m, 2))
        l[:, 3] = np.minimum(size * np.sqrt(asp), 0.95)
        l[:, 4] = np.minimum(size / np.sqrt(asp), 0.95)
        labels.append(l)
    return shapes, labels


def repeated_dataset(rng, n_img, per_img, points):
    """Square images whose labels are drawn from a few fixed sizes (so k-means meets duplicate centres)."""
    shapes = np.full((n_img, 2), 512.0)
    pts = np.array(points, dtype=np.float64) / 512.0
    labels = []
    for _ in range(n_img):
        m = int(rng.integers(per_img[0], per_img[1] + 1))
        l = np.zeros((m, 5))
        l[:, 1:3] = 0.5
        l[:, 3:5] = pts[rng.integers(0, len(pts), m)]
        labels.append(l)
    return shapes, labels


def detect_stub(anchors_px):
    a = torch.tensor(anchors_px, dtype=torch.float32).view(1, -1, 2)
    return types.SimpleNamespace(anchors=a / STRIDE, anchor_grid=a.clone().view(1, 1, -1, 1, 1, 2), stride=torch.tensor([STRIDE]))


def run_reference(A, seed, shapes, labels, anchors_px, thr, imgsz, gen):
    """The reference's check_anchors (with kmean_anchors at `gen` generations) on a Detect stand-in."""
    got = {}
    kmeans0, kmean_anchors0 = A.kmeans, A.kmean_anchors

    def kmeans(*a, **k):
        got["book"], got["dist"] = kmeans0(*a, **k)
        return got["book"].copy(), got["dist"]

    def kmean_anchors(path, **kw):                     # check_anchors asks for 1000 generations
        got["k"] = kmean_anchors0(path, **dict(kw, gen=gen))
        return got["k"]
    m = detect_stub(anchors_px)
    model = types.SimpleNamespace(detect=[m])
    ds = types.SimpleNamespace(shapes=shapes.copy(), labels=[l.copy() for l in labels])
    A.kmeans, A.kmean_anchors = kmeans, kmean_anchors
    buf = io.StringIO()
    try:
        np.random.seed(seed)
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
            A.check_anchors(ds, model, thr=thr, imgsz=imgsz)
    finally:
        A.kmeans, A.kmean_anchors = kmeans0, kmean_anchors0
    return m, got, buf.getvalue(), np.random.get_state()


def restate(seed, shapes, labels, anchors_px, thr, imgsz, n, gen):
    """The same call on the restatement.  Returns (bpr, aat, k, info, random state afterwards)."""
    np.random.seed(seed)
    scale = np.random.uniform(0.9, 1.1, size=(shapes.shape[0], 1))
    wh = AR.label_wh(shapes, labels, imgsz, scale)
    st = AR.stats(wh, np.array(anchors_px, dtype=np.float32).reshape(-1, 2), 1.0 / thr)
    bpr, aat = st[2] / len(wh), st[3] / len(wh)
    k, info = None, {}
    if np.float32(bpr) < 0.98:
        k, info = AR.kmean_anchors(shapes, labels, n, imgsz, thr, gen)
    return bpr, aat, k, info, np.random.get_state()


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def main():
    import_reference()
    A = importlib.import_module("reference.basics.utils.autoanchor")
    cases = []

    def attempt(tag, seed, shapes, labels, anchors_px, thr, imgsz, gen, want):
        n = len(anchors_px) // 2
        m, got, out, state = run_reference(A, seed, shapes, labels, anchors_px, thr, imgsz, gen)
        bpr, aat, k, info, rstate = restate(seed, shapes, labels, anchors_px, thr, imgsz, n, gen)
        assert same_state(state, rstate), f"{tag}: the restatement leaves another random state"
        ran = "book" in got
        if want == "keep":
            if ran:
                return None
        else:
            if not ran:
                return None
            assert np.array_equal(info["book"], got["book"]), f"{tag}: restated code book differs from scipy's"
            stops = min(abs(d - 1e-5) for d in info["diffs"])
            curs = sorted(info["curs"])
            lead = curs[1] - curs[0]
            if stops < 1e-9 or lead < 1e-9:
                return None
            if want == "fewer":
                if len(got["book"]) != n - 1 or "k" in got:
                    return None
                print(f"[autoanchor golden] {tag}: seed {seed}, {len(got['book'])} of {n} centres, stop margin {stops:.2e}, "
                      f"winner {info['winner']} leads by {lead:.2e}")
            else:
                if "k" not in got or len(got["book"]) != n:
                    return None
                assert np.array_equal(k, got["k"]), f"{tag}: restated anchors differ from the reference's"
                margin = float(info["margins"].min())
                replaced = not torch.equal(m.anchor_grid.view(-1), torch.tensor(anchors_px, dtype=torch.float32))
                if margin < 1e-6 or not replaced:
                    return None
                print(f"[autoanchor golden] {tag}: seed {seed}, {sum(len(l) for l in labels)} labels, bpr {bpr:.4f}, "
                      f"{int(info['accepted'].sum())} of {gen} accepted, min |fg - f| {margin:.2e}, stop margin {stops:.2e}, "
                      f"winner {info['winner']} leads by {lead:.2e}")
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
        return dict(tag=tag, seed=seed, shapes=t(shapes), labels=[t(l) for l in labels], thr=thr, imgsz=imgsz, n=n, gen=gen,
                    anchors0=torch.tensor(anchors_px, dtype=torch.float32).view(-1, 2), stride=STRIDE, bpr=float(bpr),
                    aat=float(aat), book=t(got.get("book")), k=t(got.get("k")), anchors=m.anchors.clone(),
                    anchor_grid=m.anchor_grid.clone(), stdout=out)

    def search(tag, make, anchors_px, thr, imgsz, gen, want, seed):
        while True:
            shapes, labels = make(np.random.default_rng(seed))
            c = attempt(tag, seed, shapes, labels, anchors_px, thr, imgsz, gen, want)
            if c is not None:
                cases.append(c)
                return
            seed += 1

    wide = lambda rng: dataset(rng, 40, (4, 8), 0.004, 0.7, 8.0)
    for n, anchors in ((9, ANCHORS9), (3, ANCHORS3)):
        for thr in (4.0, 2.91):
            search(f"evolve_n{n}_thr{thr}", wide, anchors, thr, 512, 300, "evolve", 1000 * n + int(thr * 100))
    # labels that the starting anchors already fit: nothing is recomputed, only the scale draw is consumed
    fit = lambda rng: dataset(rng, 40, (4, 8), 0.03, 0.12, 1.5)
    search("keep_n3", fit, ANCHORS3, 4.0, 512, 300, "keep", 50)
    # n - 1 = 8 distinct label sizes, none of which the starting anchors fit
    pts = [(3, 40), (40, 3), (5, 90), (90, 5), (4, 200), (200, 4), (6, 300), (300, 7)]
    rep = lambda rng: repeated_dataset(rng, 40, (4, 8), pts)
    search("fewer_n9", rep, ANCHORS9, 4.0, 512, 300, "fewer", 70)
    torch.save(dict(cases=cases), OUT)
    print(f"[autoanchor golden] wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
