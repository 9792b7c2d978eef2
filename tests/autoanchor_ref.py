"""A numpy restatement of the three pieces of autoanchor (basics/utils/autoanchor.py) that run on the device, written from
their behaviour: the ratio metric, the Lloyd loop inside scipy.cluster.vq.kmeans, and the anchor evolution.  Shared by
tests/test_autoanchor_host.py, tests/test_autoanchor_gpu.py, tools/gen_autoanchor_golden.py and tools/mb_autoanchor.py.
It needs neither scipy nor the reference, and draws from the numpy global random stream exactly where the reference does.

Precision: per label `x` and `best` are float32, formed as torch forms them (one IEEE division per ratio and per
reciprocal); every sum, the fitness mean and the `fg > f` decision are float64.  Thresholds are compared in float32 with
the inverted threshold rounded to float32, which is what torch does for `float32_tensor > python_float`.
"""
from __future__ import annotations

import numpy as np

F = np.float32
STAT_NAMES = ("sum_best", "sum_best_thr", "n_best_thr", "n_x_thr", "sum_x", "sum_x_thr")


def label_wh(shapes, labels, img_size, scale=None):
    """wh of all labels in pixels (float64): shapes (n_img, 2), labels a list of (m_i, 5) arrays [cls x y w h] normalised."""
    shapes = np.asarray(shapes, dtype=np.float64)
    s = img_size * shapes / shapes.max(1, keepdims=True)
    if scale is not None:
        s = s * scale
    return np.concatenate([np.asarray(l)[:, 3:5] * r for r, l in zip(s, labels)])


def metric_x(wh, k):
    """x (N, n) and best (N) in float32 for wh (N, 2) and anchors k (n, 2), both rounded to float32 first."""
    wh = np.asarray(wh).astype(F)
    k = np.asarray(k).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = wh[:, None, :] / k[None, :, :]
        x = np.minimum(r, F(1.0) / r).min(2)
    best = x.max(1) if len(x) else np.zeros(0, F)
    return x, best


def stats(wh, k, thr_inv):
    """The six figures of one anchor set, sums in float64 and counts as ints, in STAT_NAMES order."""
    t = F(thr_inv)
    x, best = metric_x(wh, k)
    xb, xx = best.astype(np.float64), x.astype(np.float64)
    return (float(xb.sum()), float(xb[best > t].sum()), int((best > t).sum()), int((x > t).sum()), float(xx.sum()),
            float(xx[x > t].sum()))


def fitness(wh, k, thr_inv):
    """mean(best * [best > thr]) with the mean in float64."""
    t = F(thr_inv)
    _, best = metric_x(wh, k)
    return float(best.astype(np.float64)[best > t].sum() / len(best))


def draw_mutations(gen, sh, mp=0.9, s=0.1):
    """The `gen` mutation factors, drawn from the numpy global stream in the reference's order: per attempt random(sh),
    random(), randn(*sh); an attempt that changes nothing is redrawn.  They do not depend on the anchors."""
    npr = np.random
    out = np.empty((gen,) + tuple(sh))
    for g in range(gen):
        v = np.ones(sh)
        while (v == 1).all():
            v = ((npr.random(sh) < mp) * npr.random() * npr.randn(*sh) * s + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(wh, k, thr_inv, v):
    """k (n, 2) float64 evolved through the factors v (G, n, 2).  Returns (k, f, accepted (G) bool, margins (G) = |fg - f|)."""
    k = np.array(k, dtype=np.float64)
    f = fitness(wh, k, thr_inv)
    accepted = np.zeros(len(v), bool)
    margins = np.zeros(len(v))
    for g in range(len(v)):
        kg = np.maximum(k * v[g], 2.0)
        fg = fitness(wh, kg, thr_inv)
        margins[g] = abs(fg - f)
        if fg > f:
            f, k = fg, kg
            accepted[g] = True
    return k, f, accepted, margins


def lloyd_step(obs, book, alive, prev):
    """One iteration on book (n, 2) float64 and alive (n) bool, both updated in place.  Returns (cur, |prev - cur|)."""
    d = obs[:, None, :] - book[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    d2[:, ~alive] = np.inf
    code = d2.argmin(1)                                      # the first of equal minima
    cur = float(np.sqrt(d2[np.arange(len(obs)), code]).mean())
    for c in np.nonzero(alive)[0]:
        m = code == c
        if m.any():
            # members are added one by one in their order, then divided by their number
            book[c] = np.add.accumulate(obs[m], 0)[-1] / m.sum()
        else:
            alive[c] = False                                 # a centre without members takes no further part
    return cur, abs(prev - cur)


def lloyd(obs, book, thresh=1e-5):
    """One restart.  Returns (book of the live centres in their order, cur, alive (n) bool, diffs of every stop decision)."""
    obs = np.asarray(obs, dtype=np.float64)
    book = np.array(book, dtype=np.float64)
    alive = np.ones(len(book), bool)
    prev, diffs = np.inf, []
    while True:
        prev, diff = lloyd_step(obs, book, alive, prev)
        diffs.append(diff)
        if diff <= thresh:                                   # the book has been moved once more after this distortion
            return book[alive], prev, alive, diffs


def initial_rows(n_obs, n, restarts=30):
    """The rows (restarts, n) of the initial code books, one `choice` draw from the numpy global stream per restart."""
    return np.stack([np.random.choice(n_obs, size=n, replace=False) for _ in range(restarts)])


def kmeans(obs, n, restarts=30, thresh=1e-5):
    """scipy.cluster.vq.kmeans(obs, n, iter=restarts).  Returns (book, dist, info) with info = dict(winner, curs, diffs, idx)."""
    best_book, best_dist, winner = None, np.inf, -1
    curs, diffs = [], []
    obs = np.asarray(obs, dtype=np.float64)
    idx = initial_rows(len(obs), n, restarts)
    for r in range(restarts):
        book, cur, _, dd = lloyd(obs, obs[idx[r]], thresh)
        curs.append(cur)
        diffs += dd
        if cur < best_dist:
            best_book, best_dist, winner = book, cur, r
    return best_book, best_dist, dict(winner=winner, curs=curs, diffs=diffs, idx=idx)


def kmean_anchors(shapes, labels, n, img_size, thr, gen):
    """kmean_anchors on a dataset, consuming the random stream as the reference does.  Returns (k or None when k-means
    gives fewer than n centres, info)."""
    thr_inv = 1.0 / thr
    wh0 = label_wh(shapes, labels, img_size)
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    book, _, info = kmeans(wh / s, n)
    info.update(book=book, obs=wh / s, s=s, wh=wh, wh0=wh0)
    if len(book) != n:
        return None, info
    k = book * s
    k = k[np.argsort(k.prod(1))]
    v = draw_mutations(gen, k.shape)
    k_end, f, accepted, margins = evolve(wh, k, thr_inv, v)
    info.update(accepted=accepted, margins=margins, f=f, v=v, wh=wh, k0=k, k_unsorted=k_end)
    return k_end[np.argsort(k_end.prod(1))], info
