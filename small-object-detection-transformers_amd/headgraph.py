"""The head graph: ``model.detect`` (parse_model's nn.Sequential with the reference's ``.f`` wiring, model.py:268-281) parsed into
the records the engine plans its launches from.  Pure Python over the module tree: no device, no kernels."""
from __future__ import annotations

import warnings
from dataclasses import dataclass, field
from typing import Dict, NamedTuple, Optional, Tuple

from . import _lib as L

ENC_C = (256, 256, 512)                                   # neck widths (backbone_vit.py:167-187), levels 0, 1, 2


class Ref(NamedTuple):
    """A tensor that exists in the workspace: encoder output y[index] (kind "enc") or the output of head row index (kind "unit")."""
    kind: str
    index: int


class Part(NamedTuple):
    """One channel segment of a virtual tensor: `channels` columns of `ref`, seen through `shr` nearest x2 upsamples."""
    ref: Ref
    channels: int
    shr: int


class Unit(NamedTuple):
    """One compute row of the head (Conv, C3 or SPP): reads the concatenation of `parts` on the grid t >> level."""
    k: int
    kind: str
    parts: Tuple[Part, ...]
    level: int
    c1: int
    c2: int
    ksize: int

    @property
    def ref(self) -> Ref:
        return Ref("unit", self.k)

    @property
    def out_name(self) -> str:
        """plan buffer that holds the unit's output"""
        return f"h{self.k}" + {"Conv": ".y", "C3": ".cv3.y", "SPP": ".cv2.y"}[self.kind]


@dataclass(frozen=True)
class HeadGraph:
    units: Tuple[Unit, ...]
    rules: Dict[int, tuple]                     # feature-list index -> ("up", src) | ("cat", [srcs]): the rows that move no data
    head_out: Tuple[int, int]                   # (unit row, channels) that Detect reads
    nd: int                                     # row of Detect
    sr_taps: Optional[Tuple[int, int]]          # feature-list entries model_up reads (sr=True), on the stride-4 / stride-8 grid
    sr_parts: Optional[Tuple[Tuple[Part, ...], Tuple[Part, ...]]]
    by_row: Dict[int, Unit] = field(init=False, repr=False, compare=False)      # head row -> its unit

    def __post_init__(self):
        object.__setattr__(self, "by_row", {u.k: u for u in self.units})


def parse_head(model) -> HeadGraph:
    """Accepted: any CHAIN of compute units - Conv (1x1 or 3x3, stride 1), C3 (n = 1), SPP - in which every unit reads ONE
    feature-list entry, possibly through nn.Upsample(x2, nearest) and Concat rows (their inputs: the previous rows or encoder
    outputs y[0..2]), ending in a one-layer Detect; every unit output and every encoder output is consumed exactly once.  That
    covers models/model.yaml:65-74, the identical head of SRyolo_MF.yaml:52-71, and variants with extra Conv / SPP
    (common.py:129-140) rows.  Upsample and Concat never move data: they become the K-segments (source + spatial map) of the
    consuming unit's first GEMM."""
    from . import model as M
    d = model.detect
    # virtual tensor: (parts, level); resolution t >> level
    vals = {j: ((Part(Ref("enc", j), ENC_C[j], 0),), j) for j in range(3)}
    units, rules = [], {}
    uses: Dict[Ref, int] = {}
    head_out = None

    def resolve(f, yi):
        j = yi - 1 if f == -1 else f
        if not isinstance(j, int) or j not in vals or j >= yi:
            raise NotImplementedError(f"head row {yi - 3}: input {f!r} does not name an earlier feature-list entry")
        return j
    if not isinstance(d[-1], M.Detect) or d[-1].nl != 1:
        raise NotImplementedError("the head must end in a one-layer Detect (models/model.yaml:74)")
    for k, m in enumerate(d):
        yi, kind = 3 + k, type(m).__name__
        if kind in ("Conv", "C3", "SPP"):
            if not isinstance(m.f, int):
                raise NotImplementedError(f"head row {k}: {kind} takes one input")
            parts, level = vals[resolve(m.f, yi)]
            c1 = sum(p.channels for p in parts)
            if kind == "Conv":
                kk, c2, cin = m.conv.kernel_size[0], m.conv.out_channels, m.conv.in_channels
            elif kind == "C3":
                if len(m.m) != 1 or m.m[0].add:
                    raise NotImplementedError("C3 with n=1, shortcut=False only (models/model.yaml:68,73)")
                kk, c2, cin = 1, m.cv3.conv.out_channels, m.cv1.conv.in_channels
            else:
                kk, c2, cin = 1, m.cv2.conv.out_channels, m.cv1.conv.in_channels
            if cin != c1:
                raise NotImplementedError(f"head row {k}: {kind} expects {cin} channels, graph gives {c1}")
            if kk == 3 and len(parts) * 9 > L.MAX_SEG:
                raise NotImplementedError(f"head row {k}: a 3x3 Conv on a concatenation needs {len(parts) * 9} K-segments (max {L.MAX_SEG})")
            for p in parts:
                uses[p.ref] = uses.get(p.ref, 0) + 1
            units.append(Unit(k, kind, parts, level, c1, c2, kk))
            vals[yi] = ((Part(Ref("unit", k), c2, 0),), level)
        elif kind == "Upsample":
            parts, level = vals[resolve(m.f, yi)]
            if level == 0:
                raise NotImplementedError(f"head row {k}: Upsample above the stride-4 grid of Detect (model.py:130)")
            vals[yi] = (tuple(Part(p.ref, p.channels, p.shr + 1) for p in parts), level - 1)
            rules[yi] = ("up", resolve(m.f, yi))
        elif kind == "Concat":
            srcs = [resolve(f, yi) for f in m.f]
            if len({vals[j][1] for j in srcs}) != 1:
                raise NotImplementedError(f"head row {k}: Concat of different resolutions")
            vals[yi] = (sum((vals[j][0] for j in srcs), ()), vals[srcs[0]][1])
            rules[yi] = ("cat", srcs)
        elif kind == "Detect":
            if k != len(d) - 1 or len(m.f) != 1:
                raise NotImplementedError("Detect must be the last row with one input")
            parts, level = vals[resolve(m.f[0], yi)]
            if len(parts) != 1 or parts[0].ref.kind != "unit" or parts[0].shr != 0 or level != 0:
                raise NotImplementedError("Detect reads one unit output on the stride-4 grid (model.py:130: stride = [4.])")
            uses[parts[0].ref] = uses.get(parts[0].ref, 0) + 1
            head_out = (parts[0].ref.index, parts[0].channels)
        else:
            raise NotImplementedError(f"head row {k}: module {kind} is outside the hot path (SURVEY.md section 8)")
    for ref in [Ref("enc", j) for j in range(3)] + [u.ref for u in units]:
        if uses.get(ref, 0) != 1:
            raise NotImplementedError(f"head: {tuple(ref)} is consumed {uses.get(ref, 0)} times; the hand-written backward routes every "
                                      "feature to exactly one consumer")
    sr_taps = sr_parts = None
    if getattr(model, "sr", False):
        # model_up(y[l1], y[l2]) (model.py:286) cannot run with the yaml's l1 / l2 = 4 / 8 (256 channels into the 128-channel
        # conv1); the taps are the first feature-list entries with the channel counts and grids DeepLab(ch, c1, c2) needs:
        # c1 on the stride-4 grid (low-level) and c2 on the stride-8 grid - y[8] and y[5] in models/model.yaml
        mu = model.model_up

        def fits(yi, cn, level):
            return yi in vals and vals[yi][1] == level and sum(p.channels for p in vals[yi][0]) == cn

        def first(cn, level):
            for yi in sorted(vals):
                if fits(yi, cn, level):
                    return yi
            raise NotImplementedError(f"sr=True: no feature-list entry has {cn} channels on the stride-{4 << level} grid")
        l1, l2 = getattr(model, "l1", None), getattr(model, "l2", None)
        if fits(l1, mu.c1, 0) and fits(l2, mu.c2, 1):
            sr_taps = (l1, l2)                      # the yaml's own taps (model.py:286: model_up(y[l1], y[l2])) are usable
        else:
            sr_taps = (first(mu.c1, 0), first(mu.c2, 1))
            warnings.warn(f"sr=True: y[l1={l1}] / y[l2={l2}] of the yaml do not have {mu.c1} channels on the stride-4 grid / {mu.c2} on the "
                          f"stride-8 grid that DeepLab(c1, c2) takes; tapping y[{sr_taps[0]}] / y[{sr_taps[1]}] instead "
                          "(DESIGN.md section 4.3: graph parity unpinned)")
        sr_parts = (vals[sr_taps[0]][0], vals[sr_taps[1]][0])
    return HeadGraph(tuple(units), rules, head_out, len(d) - 1, sr_taps, sr_parts)
