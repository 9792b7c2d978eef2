"""What a set of frozen parameters (``requires_grad == False``: Train.py:115-121, :328-333) leaves of the backward: autograd's rule on
the model's unit graph.  Pure Python over names: no device, no kernels, no torch.

A *unit* is what the engine runs as one piece in each direction - the front end, patch embed / pos_embed, the attention half and the
MLP half of every Swin block, every PatchMerging, every neck, every head unit of ``headgraph``, Detect, the SR branch.  A tensor
needs a gradient when it is the output of a unit with at least one trainable parameter or of a unit one of whose inputs needs one;
the model's inputs need none.  ``propagate`` turns that into one ``UnitRecord`` per unit; the engine reads nothing else to decide
which backward launches run, which gradients it computes and which activations the forward keeps."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Iterable, Mapping, NamedTuple, Optional, Sequence, Tuple

E = "image_encoder."
ATTN_PARAMS = ("norm1.", "attn.")          # a block's attention half: x -> xm = x + proj(attention(LN1 x)); the rest (norm2., mlp.) is
#                                            its MLP half: xm -> xm + MLP(LN2 xm)


class UnitSpec(NamedTuple):
    """One node of the unit graph: `inputs` name the units whose outputs it reads (none: it reads the model's inputs)."""
    name: str
    inputs: Tuple[str, ...]
    params: Tuple[str, ...]


@dataclass(frozen=True)
class UnitRecord:
    name: str
    runs_bwd: bool                          # its output needs a gradient: its backward runs
    needs_dx: Mapping[str, bool]            # input unit -> that input needs a gradient
    wgrad: Mapping[str, bool]               # parameter -> requires_grad
    saves: bool                             # the forward keeps what the backward reads (== runs_bwd)

    @property
    def any_dx(self) -> bool:
        return any(self.needs_dx.values())

    @property
    def any_wgrad(self) -> bool:
        return any(self.wgrad.values())


@dataclass(frozen=True)
class FreezeRecord:
    units: Mapping[str, UnitRecord]         # in forward order
    first_trainable_offset: int             # into the flat gradient buffer (its size when nothing is trainable)
    signature: int                          # bit i set: parameter i of the gradient order is frozen
    frozen: frozenset = field(repr=False, compare=False)
    frozen_runs: Tuple[Tuple[int, int], ...] = field(repr=False, compare=False)     # see dirty_runs

    def trainable(self, *names: str) -> bool:
        """whether any of these parameters is trainable"""
        return any(n not in self.frozen for n in names)

    @property
    def any_bwd(self) -> bool:
        return any(u.runs_bwd for u in self.units.values())

    def dirty_runs(self, lo: int = 0, hi: Optional[int] = None) -> Tuple[Tuple[int, int], ...]:
        """The maximal contiguous runs [first, last + 1) of the flat gradient buffer that hold only frozen parameters and at least one
        parameter of a unit whose backward runs (a launch that fuses the input gradient with parameter gradients may have written
        there), clipped to [lo, hi)."""
        out = []
        for a, b in self.frozen_runs:
            a, b = max(a, lo), b if hi is None else min(b, hi)
            if a < b:
                out.append((a, b))
        return tuple(out)

    def summary(self):
        """[(unit, runs_bwd, saves, trainable parameters, frozen parameters)] in forward order (Model.freeze_summary)"""
        return [(u.name, u.runs_bwd, u.saves, sum(u.wgrad.values()), len(u.wgrad) - sum(u.wgrad.values())) for u in self.units.values()]


def grad_layout(sizes: Mapping[str, int]) -> Tuple[list, Dict[str, int], int]:
    """(order, offsets, size) of the engine's flat gradient / parameter buffers from {parameter name: numel} in the model's own
    order.  The front end's sixteen tensors come first (its one backward launch writes four contiguous groups); the rest lies in
    REVERSE order of completion in the backward, so that the buckets that become final first are contiguous slices at the end of
    the buffer (ddp.py) - and a frozen forward prefix is the buffer's head: [front end | pos/patch embed | stage 1 |
    PatchMerging 1, neck 1 | stage 2 | PatchMerging 2, neck 2 | stage 3 | neck 3 | head | SR branch]."""
    order = [E + f"channel_embed_{c}.proj.weight" for c in "rgbi"] + [E + f"channel_embed_{c}.proj.bias" for c in "rgbi"]
    order += [E + f"chan_block.norm{i}.weight" for i in range(1, 5)] + [E + f"chan_block.norm{i}.bias" for i in range(1, 5)]
    groups = [E + "pos_embed", E + "patch_embed.", E + "stage1.", E + "pmerging1.", E + "neck1.", E + "stage2.",
              E + "pmerging2.", E + "neck2.", E + "stage3.", E + "neck3.", "detect.", "model_up."]
    seen = set(order)
    rest = []
    for gname in groups:
        rest += [n for n in sizes if n.startswith(gname) and n not in seen]
        seen.update(rest)
    rest += [n for n in sizes if n not in seen]      # nothing today; keeps unknown parameters reducible
    order = order + rest
    offs, tot = {}, 0
    for n in order:
        offs[n] = tot
        tot += (sizes[n] + 7) // 8 * 8                # every view 16-byte aligned in f32 AND in the bf16 mirror
    return order, offs, tot


def block_halves(prefix: str, names: Iterable[str]) -> Tuple[Tuple[str, ...], Tuple[str, ...]]:
    """(attention half, MLP half) of the parameters under one block's prefix"""
    mine = [n for n in names if n.startswith(prefix)]
    attn = tuple(n for n in mine if n[len(prefix):].startswith(ATTN_PARAMS))
    return attn, tuple(n for n in mine if n not in attn)


def unit_graph(param_names: Sequence[str], head, sr: bool = False) -> Tuple[UnitSpec, ...]:
    """The model's units in forward order.  param_names: every parameter name of the model; head: its headgraph.HeadGraph (units
    with their `parts`, the unit Detect reads, the SR taps).  The encoder's shape is read off the names: stage{1,2,3}.{i}. blocks,
    stage 1 feeding neck 1 from its last two blocks (backbone_vit.py:236-246) and PatchMerging 1 from its last."""
    names = list(param_names)

    def under(*prefixes):
        return tuple(n for n in names if n.startswith(prefixes))
    units = [UnitSpec("frontend", (), under(E + "channel_embed_", E + "chan_block.")),
             UnitSpec("embed", ("frontend",), under(E + "patch_embed.", E + "pos_embed"))]
    last = "embed"
    outs = {}
    for s in (1, 2, 3):
        depth = 1 + max((int(n[len(E) + 7:].split(".")[0]) for n in names if n.startswith(f"{E}stage{s}.")), default=-1)
        for i in range(depth):
            attn, mlp = block_halves(f"{E}stage{s}.{i}.", names)
            units.append(UnitSpec(f"stage{s}.{i}.attn", (last,), attn))
            units.append(UnitSpec(f"stage{s}.{i}.mlp", (f"stage{s}.{i}.attn",), mlp))
            last = f"stage{s}.{i}.mlp"
            outs[(s, i)] = last
        if s == 1:
            units.append(UnitSpec("neck1", (outs[(1, depth - 2)], outs[(1, depth - 1)]), under(E + "neck1.")))
        else:
            units.append(UnitSpec(f"neck{s}", (last,), under(E + f"neck{s}.")))
        if s < 3:
            units.append(UnitSpec(f"pmerging{s}", (last,), under(E + f"pmerging{s}.")))
            last = f"pmerging{s}"

    def producer(ref):
        return f"neck{ref.index + 1}" if ref.kind == "enc" else f"h{ref.index}"
    for u in head.units:
        units.append(UnitSpec(f"h{u.k}", tuple(producer(p.ref) for p in u.parts), under(f"detect.{u.k}.")))
    units.append(UnitSpec("detect", (f"h{head.head_out[0]}",), under(f"detect.{head.nd}.")))
    if sr:
        taps = tuple(dict.fromkeys(producer(p.ref) for parts in head.sr_parts for p in parts))
        units.append(UnitSpec("model_up", taps, under("model_up.")))
    owned = [n for u in units for n in u.params]
    if len(owned) != len(set(owned)) or set(owned) != set(names):
        raise ValueError(f"unit graph: parameters outside every unit or in two: {sorted(set(names) ^ set(owned))[:4]}")
    return tuple(units)


def propagate(graph: Sequence[UnitSpec], frozen: Iterable[str], grad_order: Sequence[str], grad_offsets: Mapping[str, int],
              grad_size: int) -> FreezeRecord:
    """frozen: the names of the parameters with requires_grad == False; grad_order / grad_offsets / grad_size: the layout of the
    engine's flat gradient buffer (Engine.grad_order, .grad_offsets, .flat_grad.numel())."""
    frozen = frozenset(frozen)
    out_needs: Dict[str, bool] = {}
    units: Dict[str, UnitRecord] = {}
    for u in graph:
        wgrad = {n: n not in frozen for n in u.params}
        needs_dx = {i: out_needs[i] for i in u.inputs}
        runs = any(wgrad.values()) or any(needs_dx.values())
        out_needs[u.name] = runs
        units[u.name] = UnitRecord(u.name, runs, needs_dx, wgrad, runs)
    first = next((grad_offsets[n] for n in grad_order if n not in frozen), grad_size)
    sig = sum(1 << i for i, n in enumerate(grad_order) if n in frozen)
    # frozen runs that a backward launch may have written: neighbours in the buffer merge into one run
    dirty = {n for u in units.values() if u.runs_bwd for n, t in u.wgrad.items() if not t}
    runs, start, hot = [], None, False
    for n in list(grad_order) + [None]:
        if n is not None and n in frozen:
            if start is None:
                start, hot = grad_offsets[n], False
            hot = hot or n in dirty
        elif start is not None:
            if hot:
                runs.append((start, grad_size if n is None else grad_offsets[n]))
            start = None
    return FreezeRecord(units, first, sig, frozen, tuple(runs))
