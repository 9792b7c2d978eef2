"""Autoanchor on the GPU - the drop-in for `check_anchors` and `kmean_anchors` (`utils/autoanchor.py:24-158`), which
Train.py:259-261 runs on every fresh run unless --noautoanchor is given.

The ratio metric of every label against every anchor, the 30 restarts of k-means and the generations of
mutate-and-evaluate run in HIP kernels (csrc/autoanchor.hip) behind the C ABI (`sodt_anchor_stats`, `sodt_kmeans_lloyd`,
`sodt_anchor_evolve`).  Each label set goes to the device once; the host reads the BPR decision of `check_anchors`, the
done flags of k-means once per chunk of iterations (with the distortions and the live-centre counts beside them), the
final anchors together with the figures of the two summaries, and with verbose=True the figures of the accepted
generations.  Per label the metric is float32 exactly as torch forms it; sums and the fitness are float64 and
`fg > f` is decided in float64, where the reference's float32 mean decides the same unless the two differ by less than
about 1e-6.  The numpy global random stream is consumed exactly as the reference consumes it
(the scale draw of check_anchors, one `choice` per restart, then the mutation draws), so `np.random.get_state()` after a
call equals the reference's.  Neither scipy, tqdm nor cv2 is imported.

Differences from the reference, all documented in DESIGN.md:
  * when k-means returns fewer than `n` centres the reference asserts; its check_anchors catches that, prints the error
    and goes on to compare the old anchors with themselves.  Here `kmean_anchors` raises the same AssertionError, and
    `check_anchors` prints the same message and keeps the original anchors explicitly.
  * check_anchors rates the new anchors with the same float32 device metric as the old ones; the reference divides by the
    float64 array kmean_anchors returned, which promotes that one evaluation to float64.
  * there is no progress bar, and the summaries of accepted generations (verbose=True) are printed after the evolution,
    in generation order, not during it.
  * a `str` path (a dataset *.yaml) raises NotImplementedError: datasets are out of scope; pass the
    loaded dataset, any object with `.shapes` (n_img, 2) and `.labels` (a list of (m_i, 5) arrays).
  * the printed summary lines keep the reference's wording; `check_anchor_order` (model.py) reorders without the
    reference's "Reversing anchor order" notice.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import ops
from .model import check_anchor_order

PREFIX = "\033[34m\033[1mautoanchor: \033[0m"           # colorstr('autoanchor: ')
RESTARTS = 30                                         # kmeans(wh / s, n, iter=30)
KMEANS_THRESH = 1e-5                                  # scipy.cluster.vq.kmeans' default
KMEANS_CHUNK = 8                                      # Lloyd iterations between two reads of the done flags
MAX_ANCHORS = 32
_F = np.float32


def _device_of(dev=None) -> torch.device:
    if dev is not None and torch.device(dev).type == "cuda":
        return torch.device(dev)
    if not torch.cuda.is_available():
        raise RuntimeError("autoanchor: the metric, k-means and the evolution run on the GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _on(dev: torch.device):
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def _label_wh(dataset, img_size, scale=None) -> np.ndarray:
    """autoanchor.py:29-31 / :110-111: label sizes in pixels of the letterboxed images, float64 on the host."""
    shapes = np.asarray(dataset.shapes, dtype=np.float64)
    shapes = img_size * shapes / shapes.max(1, keepdims=True)
    if scale is not None:
        shapes = shapes * scale
    return np.concatenate([np.asarray(l)[:, 3:5] * s for s, l in zip(shapes, dataset.labels)]).reshape(-1, 2)


def _stats(wh: torch.Tensor, sets: torch.Tensor, thr: float) -> torch.Tensor:
    """(S, 6) f64 on the device for wh (N, 2) f32 and sets (S, n, 2) f32; no host read."""
    S = sets.shape[0]
    out = torch.empty(S, 6, dtype=torch.float64, device=wh.device)
    ws = torch.empty(ops.anchor_stats_workspace_bytes(wh.shape[0], S), dtype=torch.uint8, device=wh.device)
    ops.anchor_stats(wh, sets, 1.0 / thr, ws, out)
    return out


def _count(n: int, dev) -> torch.Tensor:
    """n as a float64 device tensor: tensor / tensor is an IEEE division, where tensor / python_number multiplies by the
    rounded reciprocal on the device - and the fitness the evolution starts from must be the quotient its kernel forms."""
    return torch.tensor(float(n), dtype=torch.float64, device=dev)


def _as_sets(anchors, dev) -> torch.Tensor:
    a = torch.as_tensor(anchors).detach().to(device=dev, dtype=torch.float32)
    a = a.reshape(1, -1, 2) if a.dim() <= 2 else a.reshape(a.shape[0], -1, 2)
    if not 1 <= a.shape[1] <= MAX_ANCHORS:
        raise ValueError(f"an anchor set has 1 to {MAX_ANCHORS} anchors, got {a.shape[1]}")
    return a.contiguous()


def anchor_metric(wh, anchors, thr: float = 4.0):
    """The device metric on its own (autoanchor.py:33-39): wh (N, 2) label sizes and anchors (n, 2), or (S, n, 2) for S
    sets at once, in pixels.  Returns (bpr, aat) as float64 device tensors, scalars for one set and (S) for several:
    the fraction of labels whose best anchor is within `thr` and the mean number of anchors within `thr` per label."""
    dev = _device_of(wh.device if torch.is_tensor(wh) else None)
    with _on(dev):
        w = torch.as_tensor(wh).detach().to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
        single = torch.as_tensor(anchors).dim() <= 2
        out = _stats(w, _as_sets(anchors, dev), thr)
        n = _count(max(w.shape[0], 1), dev)
        bpr, aat = out[:, 2] / n, out[:, 3] / n
        return (bpr[0], aat[0]) if single else (bpr, aat)


def _bpr32(count: float, n: int):
    """(best > thr).float().mean(): a float32 quotient of two integers."""
    return _F(count) / _F(n)


def check_anchors(dataset, model, thr: float = 4.0, imgsz: int = 640):
    """autoanchor.py:24-60: check the anchor fit to the data and recompute the anchors if the best possible recall is
    below 0.98.  `m.anchors` and `m.anchor_grid` of the Detect module are updated in place, so a ComputeLoss and an engine
    built before the call see the new anchors."""
    print(f"\n{PREFIX}Analyzing anchors... ", end="")
    m = model.module.detect[-1] if hasattr(model, "module") else model.detect[-1]
    scale = np.random.uniform(0.9, 1.1, size=(len(dataset.shapes), 1))                 # augment scale
    dev = _device_of(m.anchors.device)
    with _on(dev):
        wh = torch.from_numpy(_label_wh(dataset, imgsz, scale)).to(dev).float()        # the labels go up once
        n_lab = wh.shape[0]

        def counts(a):                                                                  # one host read: [n_best_thr, n_x_thr]
            return _stats(wh, _as_sets(a, dev), thr)[0, 2:4].tolist()
        old = m.anchor_grid.detach().clone().view(-1, 2)
        cb, cx = counts(old)
        bpr, aat = _bpr32(cb, n_lab), _F(cx) / _F(n_lab)
        print(f"anchors/target = {aat:.2f}, Best Possible Recall (BPR) = {bpr:.4f}", end="")
        if bpr < _F(0.98):                                                              # threshold to recompute
            print(". Attempting to improve anchors, please wait...")
            na = m.anchor_grid.numel() // 2
            new = None
            try:
                new = kmean_anchors(dataset, n=na, img_size=imgsz, thr=thr, gen=1000, verbose=False)
            except Exception as e:
                print(f"{PREFIX}ERROR: {e}")
            # (the reference goes on with the old anchors here and finds them no better than themselves)
            new_bpr = bpr if new is None else _bpr32(counts(new)[0], n_lab)
            if new_bpr > bpr:
                anchors = torch.as_tensor(new, device=m.anchors.device).type_as(m.anchors)
                m.anchor_grid[:] = anchors.clone().view_as(m.anchor_grid)              # for inference
                m.anchors[:] = anchors.clone().view_as(m.anchors) / m.stride.to(m.anchors.device).view(-1, 1, 1)   # loss
                check_anchor_order(m)
                print(f"{PREFIX}New anchors saved to model. Update model *.yaml to use these anchors in the future.")
            else:
                print(f"{PREFIX}Original anchors better than new anchors. Proceeding with original anchors.")
    print("")


def _kmeans_device(obs: torch.Tensor, idx: torch.Tensor, chunk: int = KMEANS_CHUNK):
    """The restarts of scipy.cluster.vq.kmeans from the initial rows idx (R, n) of obs (N, 2) f64.  Returns
    (books (R, n, 2), alive (R, n) int32) on the device and, on the host, the final distortion and the number of live
    centres of every restart.  One host read per chunk of iterations."""
    R, n = idx.shape
    dev = obs.device
    books = obs[idx].contiguous()
    alive = torch.ones(R, n, dtype=torch.int32, device=dev)
    prev = torch.full((R,), float("inf"), dtype=torch.float64, device=dev)
    done = torch.zeros(R, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.kmeans_lloyd_workspace_bytes(obs.shape[0], R, n), dtype=torch.uint8, device=dev)
    for _ in range(100000 // chunk):
        ops.kmeans_lloyd(obs, books, alive, prev, done, KMEANS_THRESH, chunk, ws)
        flags = torch.stack((done.double(), prev, alive.sum(1).double())).cpu()        # the read of this chunk
        if bool(flags[0].all()):
            return books, alive, flags[1].numpy(), flags[2].numpy().astype(np.int64)
    raise RuntimeError("k-means did not converge")


def _summary(n, img_size, thr_inv, k, st, n0):
    """The two lines of print_results (autoanchor.py:94-98) from the six figures `st` of the sorted anchors k."""
    sb, _, cb, cx, sx, sxt = st
    bpr, aat = _bpr32(cb, n0), _F(cx) / _F(n0 * n) * n
    past = sxt / cx if cx else float("nan")
    lines = f"{PREFIX}thr={thr_inv:.2f}: {bpr:.4f} best possible recall, {aat:.2f} anchors past thr\n"
    lines += (f"{PREFIX}n={n}, img_size={img_size}, metric_all={sx / (n0 * n):.3f}/{sb / n0:.3f}-mean/best, "
              f"past_thr={past:.3f}-mean: ")
    lines += ",  ".join("%i,%i" % (round(x[0]), round(x[1])) for x in k)
    return lines


def kmean_anchors(path, n: int = 9, img_size: int = 640, thr: float = 4.0, gen: int = 1000, verbose: bool = True):
    """autoanchor.py:63-158: k-means evolved anchors (n, 2) of a loaded dataset, a float64 numpy array sorted by area.

        path: a loaded dataset (`.shapes`, `.labels`); a str path is refused
        n: number of anchors;  img_size: image size used for training
        thr: anchor-label wh ratio threshold hyp['anchor_t'];  gen: generations of the genetic algorithm
        verbose: also print the summary of every accepted generation
    """
    if isinstance(path, str):
        raise NotImplementedError(f"kmean_anchors({path!r}): loading a dataset from a *.yaml path is out of scope; "
                                  "pass the loaded dataset (an object with .shapes and .labels)")
    if not 1 <= n <= MAX_ANCHORS:
        raise ValueError(f"kmean_anchors builds 1 to {MAX_ANCHORS} anchors, got n={n}")
    dataset = path
    thr_inv = 1.0 / thr
    wh0 = _label_wh(dataset, img_size)
    i = (wh0 < 3.0).any(1).sum()
    if i:
        print(f"{PREFIX}WARNING: Extremely small objects found. {i} of {len(wh0)} labels are < 3 pixels in size.")
    wh = wh0[(wh0 >= 2.0).any(1)]                                                       # filter > 2 pixels
    print(f"{PREFIX}Running kmeans for {n} anchors on {len(wh)} points...")
    s = wh.std(0)                                                                       # sigmas for whitening
    # scipy draws the initial code book of every restart with one `choice`; the draws do not depend on the restarts
    idx = np.stack([np.random.choice(len(wh), size=n, replace=False) for _ in range(RESTARTS)])
    dev = _device_of()
    with _on(dev):
        n0, nf = len(wh0), len(wh)
        up = torch.from_numpy(np.concatenate([wh0, wh, wh / s])).to(dev)                # the labels go up once
        wh0_d, wh_d, obs = up[:n0].float(), up[n0:n0 + nf].float(), up[n0 + nf:]
        s_d = torch.from_numpy(s).to(dev)
        books, alive, curs, live = _kmeans_device(obs, torch.from_numpy(idx).to(dev))
        win = int(np.argmin(curs))                                                      # the first strictly smallest distortion
        if live[win] != n:                                                              # the reference's `assert cond, print(...)`
            print(f"{PREFIX}ERROR: scipy.cluster.vq.kmeans requested {n} points but returned only {live[win]}")
            raise AssertionError(None)
        k = books[win] * s_d
        k = k[torch.argsort(k.prod(1), stable=True)]                                    # print_results sorts small to large
        st_kmeans = _stats(wh0_d, k.float().view(1, n, 2), thr)
        k0 = k.clone()

        # Evolve: the mutation factors depend on the random stream only, so all of them are drawn up front
        sh, mp, sg = (n, 2), 0.9, 0.1
        v = np.empty((gen, n, 2))
        for g in range(gen):
            vg = np.ones(sh)
            while (vg == 1).all():                                                      # mutate until a change occurs
                vg = ((np.random.random(sh) < mp) * np.random.random() * np.random.randn(*sh) * sg + 1).clip(0.3, 3.0)
            v[g] = vg
        f = _stats(wh_d, k.float().view(1, n, 2), thr)[0, 1:2] / _count(nf, dev)        # anchor_fitness(k), on the device
        accepted = torch.zeros(max(gen, 1), dtype=torch.int32, device=dev)
        if gen:
            ws = torch.empty(ops.anchor_evolve_workspace_bytes(nf), dtype=torch.uint8, device=dev)
            ops.anchor_evolve(wh_d, thr_inv, k, f, torch.from_numpy(v).to(dev), accepted, ws)
        k = k[torch.argsort(k.prod(1), stable=True)]
        st_final = _stats(wh0_d, k.float().view(1, n, 2), thr)
        # the one read at the end: both anchor sets, their figures and the acceptance mask
        host = torch.cat((k0.reshape(-1), k.reshape(-1), st_kmeans.reshape(-1), st_final.reshape(-1),
                          accepted.double())).cpu().numpy()
        k0_h, k_h = host[:2 * n].reshape(n, 2), host[2 * n:4 * n].reshape(n, 2)
        st0_h, st1_h, acc_h = host[4 * n:4 * n + 6], host[4 * n + 6:4 * n + 12], host[4 * n + 12:4 * n + 12 + gen] != 0
        print(_summary(n, img_size, thr_inv, k0_h, st0_h, n0))
        if verbose and acc_h.any():
            # the anchors of every accepted generation follow from k0 and the factors in float64 on the host, bit for
            # bit as the device formed them; their figures come from one more launch over all of them
            cur, steps = k0_h, []
            for g in np.nonzero(acc_h)[0]:
                cur = np.maximum(cur * v[g], 2.0)
                steps.append(cur[np.argsort(cur.prod(1))])
            sets = torch.from_numpy(np.stack(steps)).to(dev).float()
            for kk, st in zip(steps, _stats(wh0_d, sets, thr).cpu().numpy()):
                print(_summary(n, img_size, thr_inv, kk, st, n0))
        print(_summary(n, img_size, thr_inv, k_h, st1_h, n0))
    return k_h
