"""Execution engine: the whole forward AND backward of Model(model.yaml) as a fixed
sequence of HIP kernels (C ABI, include/sodt_hip.h), token-major activations.

* One ``Plan`` per (batch, resolution, dtype, mode) - and, in training mode, per set of
  ``requires_grad`` flags (freeze.py: frozen units have no backward launch and save nothing):
  every activation / gradient buffer is allocated once; the first run records every launch,
  later runs replay the list.
* Backward is hand-written (no torch autograd inside): ``_EngineFn`` is a single
  autograd node whose backward runs the recorded reverse sequence and deposits parameter
  gradients into one flat f32 buffer (``param.grad`` are views of it), the layout a
  bucketed RCCL all-reduce wants (ddp.py).
* Reference lines each phase replaces are cited in the kernel sources and
  include/sodt_hip.h; the graph is backbone_vit.py:190-272 + models/model.yaml:65-74.
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib as L
from . import ops
from . import freeze
from .ddp import sync_bn_in_force
from .headgraph import Ref, parse_head
from .ops import TAPS3, SegSpec

HEADS = 12
E = "image_encoder."
TAPS2 = ((0, 0), (0, 1), (1, 0), (1, 1))                       # (dy, dx) of the 2x2 conv, kernel index kh*2+kw
MERGE = ((0, 0), (1, 0), (0, 1), (1, 1))                        # PatchMerging gather order (backbone_vit.py:850-853)
USE_HIPGRAPH = os.environ.get("SODT_HIPGRAPH", "0") == "1"     # opt-in: see Engine._replay


class _Yes:
    def __getitem__(self, key):
        return True


class _EveryUnit:
    """the freeze.UnitRecord of a plan without one (eval plans, plans built by hand): nothing is frozen"""
    runs_bwd = saves = any_dx = any_wgrad = True
    needs_dx = wgrad = _Yes()


class Plan:
    def __init__(self, B, S, dt, training, dev, fz=None):
        # S: the side of a square input, or (H, W).  plan.S stays the int for a square plan and is the tuple for H != W
        H, W = (S, S) if isinstance(S, int) else (int(S[0]), int(S[1]))
        S = H if H == W else (H, W)
        self.B, self.S, self.H, self.W, self.dt, self.training, self.dev = B, S, H, W, dt, training, dev
        self.fz: Optional[freeze.FreezeRecord] = fz     # what the requires_grad flags leave of the backward (training plans of Engine.run)
        self.bufs: Dict[str, torch.Tensor] = {}
        self.bwd_marks: List[Tuple[int, int, int]] = []   # (index in bwd_main, first, last+1 element of flat_grad) of the
        #                                                   gradient buckets that are final at that launch (ddp overlap)
        self.gen = 0                              # bumped by every forward that overwrites the saved activations
        self.fwd_pre: Optional[list] = None
        self.fwd_main: Optional[list] = None
        self.bwd_main: Optional[list] = None
        self.saved: dict = {}                     # tag -> BlockRoute / ConvRoute / dict: what the forward chose, for the backward
        self.graphs: dict = {}                    # hipGraph of a recorded list (captured on its first replay)
        self.zused: Dict[str, int] = {}           # bytes handed out of each zero pool (zbuf)
        self.sr = None                            # this plan's sr.SRBranch (Engine._sr_forward)
        self.enc_bwd_start: Optional[int] = None  # index in bwd_main where the head's backward ends and the encoder's begins
        self.enc_gin: Optional[list] = None       # [(buf, ld, off, c)]: where the head leaves d(f0), d(f1), d(f2)
        self.det_fused: Optional[bool] = None     # Detect's backward is the live one-pass launch, not part of bwd_main (set with bwd_main)
        self.bn_marks: List[list] = []            # [index in fwd_main, BatchNorm2d, its name, momentum recorded] of every sodt_bn_finalize
        # synchronised BatchNorm (Engine.sync_bn with more than one rank; empty otherwise): where a replay stops for a collective
        self.sbn_fwd: List[Tuple[int, torch.Tensor]] = []                 # (a bn_marks index, the conv's stats) - all-reduced in place
        self.sbn_bwd: List[Tuple[int, torch.Tensor, torch.Tensor]] = []   # (index in bwd_main of the apply launch, red, red_all)

    def unit(self, name):
        """the freeze.UnitRecord of unit `name`"""
        return _EveryUnit if self.fz is None else self.fz.units[name]

    def trainable(self, *names):
        """whether any of these parameters takes a gradient"""
        return True if self.fz is None else self.fz.trainable(*names)

    def saves(self, name):
        """whether the forward of unit `name` keeps what its backward reads"""
        return self.training and self.unit(name).saves

    def keep(self, save, name, kind, shape, dtype=None):
        """A forward intermediate the backward reads back: the unit's own buffer `name` when it is saved (and in an eval plan, as
        ever); in a training plan whose unit saves nothing, one scratch per kind and shape that every such unit shares (one unit's
        forward runs at a time)."""
        if save or not self.training:
            return self.buf(name, shape, dtype)
        return self.scratch("fwd." + kind, shape, dtype)

    def _cached(self, name, shape, dtype):
        """the buffer already allocated under `name`, or None; a hit with another shape or dtype is a bug of the caller"""
        t = self.bufs.get(name)
        if t is not None and (tuple(t.shape) != tuple(shape) or t.dtype != dtype):
            raise RuntimeError(f"plan buffer {name!r} is {tuple(t.shape)} {t.dtype}, requested as {tuple(shape)} {dtype}")
        return t

    def zbuf(self, pool, name, shape, dtype):
        """Small accumulator that must be zero at the start of every forward (pool "f") or backward (pool "b"): carved out of
        one 2 MiB pool per direction that a single memset clears (24 tiny memset launches per step otherwise)."""
        t = self._cached(name, shape, dtype)
        if t is None:
            pbuf = self.zpool(pool)
            n = 1
            for d in shape:
                n *= d
            nbytes = n * torch.empty((), dtype=dtype).element_size()
            off = self.zused[pool]
            if off + nbytes > pbuf.numel():
                raise RuntimeError("zero pool exhausted")
            t = pbuf[off: off + nbytes].view(dtype).view(shape)
            self.zused[pool] = (off + nbytes + 255) // 256 * 256
            self.bufs[name] = t
        return t

    def zpool(self, pool):
        pbuf = self.bufs.get("zpool." + pool)
        if pbuf is None:
            pbuf = self.bufs["zpool." + pool] = torch.zeros(1 << 21, device=self.dev, dtype=torch.uint8)
            self.zused[pool] = 0
        return pbuf

    def buf(self, name, shape, dtype=None, zero=False):
        dtype = self.dt if dtype is None else dtype
        t = self._cached(name, shape, dtype)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, device=self.dev, dtype=dtype)
            self.bufs[name] = t
        return t

    def scratch(self, kind, shape, dtype=None, zero=False):
        """Backward scratch that every user of the same kind AND shape shares (one block's backward runs at a time)."""
        return self.buf(f"g.{kind}.{'x'.join(str(d) for d in shape)}", shape, dtype, zero)


class _Plans(dict):
    """Engine.plans: (B, S, dt, False) -> eval plan, (B, S, dt, True, freeze signature) -> training plan.  The four-entry key of a
    training plan reads the plan with nothing frozen (signature 0), which is what it named before plans knew about freezing.
    S is the side of a square input; an H x W input with H != W has (H, W) in that slot."""

    def __missing__(self, key):
        if len(key) == 4 and key[3] and key + (0,) in self:
            return self[key + (0,)]
        raise KeyError(key)


# what _block_route chooses among (BlockRoute.attn / .mlp)
ATTN_FUSED_RC, ATTN_FUSED_SAVED, ATTN_PADDED, ATTN_PLAIN = "fused, q/k/v recomputed", "fused, q/k/v saved", "padded", "plain"
ATTN_SHIFT_PAD = "shifted, padded"      # only with Engine.pad_shifted_blocks (Model.pad_shifted_blocks)
MLP_FUSED, MLP_LIN_RC, MLP_LIN_SAVED, MLP_FOLD, MLP_CONV = "fused linear", "linear, activation saved", "linear, pre-activation saved", \
    "folded conv", "three-GEMM conv"


class BlockRoute(NamedTuple):
    """Everything one Swin block's forward chose (_block_route): the backward selects its launches from this alone."""
    x_in: torch.Tensor
    geo: tuple                          # (B, H, W, C, ws, shift)
    pad: Optional[Tuple[int, int]]      # the padded grid (Hp, Wp) of a resolution that is no multiple of the window
    attn: str                           # ATTN_*
    wpk: Optional[torch.Tensor]         # parameter pack of the fused W-MSA kernel
    mlp: str                            # MLP_*
    zscratch: bool                      # window above 64 tokens: the five-launch attention backward needs its zeroed scratch
    sq_ok: bool                         # attn.proj / fc2 backward may take the square one-launch form (use_fused_linbwd permitting)
    wide_ok: bool                       # attn.qkv backward may take the wide one-launch form (use_wide_linbwd permitting)
    mlp_bwd: bool = False               # MLP_FUSED only: the backward is sodt_mlp_bwd's one launch and the forward keeps no GELU(h)


class ConvRoute(NamedTuple):
    """One head Conv2d+BN+SiLU as _conv_fwd ran it."""
    segs: list
    spatial: Optional[Tuple[int, int]]
    M: int
    K: int
    Cout: int
    k: int
    pname: str
    direct: bool                        # the 3x3 at 64 -> 64 channels on the direct kernels (csrc/conv3.hip)


class _LazyFeatures(list):
    """forward_once's feature list `y` (model.py:268-281).  Entries produced by nn.Upsample(x2, nearest) and Concat
    (models/model.yaml:66-67,71-72: y[4], y[5], y[8], y[9]) are index arithmetic inside the GEMM loaders and never exist in
    the workspace; they are computed on first access.  rules: {index: ("up", src) | ("cat", [srcs])} from the head plan."""

    def __init__(self, items=(), rules=None):
        super().__init__(items)
        self._rules = dict(rules or {})

    def _fill(self, i):
        if list.__getitem__(self, i) is None and i in self._rules:
            r = self._rules[i]
            if r[0] == "up":
                v = torch.nn.functional.interpolate(self[r[1]].float(), scale_factor=2, mode="nearest")
            else:
                v = torch.cat([self[j].float() for j in r[1]], 1)
            list.__setitem__(self, i, v)

    def __getitem__(self, i):
        if isinstance(i, int):
            j = i + len(self) if i < 0 else i
            self._fill(j)
        else:
            for j in sorted(self._rules):
                self._fill(j)
        return list.__getitem__(self, i)

    def __iter__(self):
        for j in sorted(self._rules):
            self._fill(j)
        return list.__iter__(self)

    def __add__(self, other):       # Model.forward appends the head output: stay lazy
        out = _LazyFeatures(list.__iter__(self), self._rules)
        list.extend(out, other)
        return out


class _EngineFn(torch.autograd.Function):
    """One autograd node for the whole model.  Parameter gradients are written straight into
    ``param.grad`` (views of the engine's flat buffer), so the node returns None for them."""

    @staticmethod
    def forward(ctx, engine, plan, x_rgb, x_ir, anchor):
        ctx.engine, ctx.plan = engine, plan
        ctx.inputs = (x_rgb, x_ir)
        ctx.set_materialize_grads(False)         # an unused output (detection-only or SR-only loss) arrives as None, not zeros
        pred = engine._forward(plan, x_rgb, x_ir)
        ctx.gen = plan.gen
        if engine.sr:
            return pred, engine._sr_forward(plan)
        return pred

    @staticmethod
    def backward(ctx, dpred, dsr=None):
        if ctx.gen != ctx.plan.gen:
            raise RuntimeError("the activations this backward needs were overwritten by a later forward of the same "
                               "(batch, resolution, dtype, mode): call backward() before the next forward, or run the "
                               "extra forward under model.eval() / torch.no_grad() with a different mode")
        ctx.engine._backward(ctx.plan, ctx.inputs[0], ctx.inputs[1], None if dpred is None else dpred.contiguous().float(),
                             None if dsr is None else dsr.contiguous().float())
        return None, None, None, None, None


class Engine:
    def __init__(self, model):
        self.model = model
        self.params: Dict[str, torch.nn.Parameter] = dict(model.named_parameters())
        self.buffers: Dict[str, torch.Tensor] = dict(model.named_buffers())
        p0 = next(iter(self.params.values()))
        if not p0.is_cuda:
            raise RuntimeError("move the model to the GPU first: the engine has no CPU path")
        for n, p in self.params.items():
            if p.dtype != torch.float32:
                raise RuntimeError(f"master parameters must be float32 (got {p.dtype} for {n}); call model.float()")
        self.dev = p0.device
        enc = model.image_encoder
        self.img_t = enc.pos_embed.shape[1]
        det = model.detect[-1]
        self.na, self.no, self.nc = det.na, det.no, det.nc
        self.det_np = (det.na * det.no + 15) // 16 * 16      # Detect GEMM width, zero-padded to a multiple of 16 (39 -> 48 at nc = 8)
        self.fused = not any(type(m).__name__ == "BatchNorm2d" for m in model.detect.modules())
        self.sr = bool(getattr(model, "sr", False))
        self.head = parse_head(model)             # headgraph.HeadGraph: units, Upsample / Concat rules, Detect's input, SR taps
        self.det_name = f"detect.{self.head.nd}."
        self.plans: Dict[Tuple, Plan] = _Plans()
        self.unit_graph = freeze.unit_graph(list(self.params), self.head, self.sr)
        self.unit_inputs = {u.name: u.inputs for u in self.unit_graph}
        self._fz: Dict[tuple, freeze.FreezeRecord] = {}           # requires_grad bits (gradient order) -> record
        self._was_frozen: frozenset = frozenset()                  # the frozen set of the latest backward (_claim_grads)
        self.probes_fwd: Optional[dict] = None    # bench.py: {call index: (start event, end event)}
        self.probes_bwd: Optional[dict] = None
        self.prep: Dict[torch.dtype, dict] = {}
        self._build_grad_buffer()
        self._build_param_buffer()
        # anchor that makes the autograd node require grad even if the caller froze everything else
        self._anchor = torch.zeros(1, device=self.dev, requires_grad=True)
        self.ddp = None     # set by ddp.attach()
        # Shifted blocks on a grid that is no multiple of their window (S % 64 == 32: stage 2) run csrc/attention_sp.hip instead of
        # being refused.  Opt-in; run() copies Model.pad_shifted_blocks here and drops the cached plans when it changes.
        self.pad_shifted_blocks = False
        # torch.nn.SyncBatchNorm's semantics for the head's BatchNorms (ddp.convert_sync_batchnorm): run() copies Model.sync_bn here
        # and drops the cached plans when it - or whether it is in force - changes.  In force (_sbn_on) only with a reducer of more
        # than one rank: otherwise every launch list is what it is without the flag.
        self.sync_bn = False
        self._sbn_on = False
        self.use_fused_wmsa = True     # tests / tools may switch the fused block kernel off to compare with the four launches it replaces
        self.use_fused_mlp = True      # the same for the fused linear MLP (csrc/mlp.hip) against its two GEMM launches
        # bf16, C = 192: backward of attn.proj and of the conv-MLP's fc2 as ONE launch each (csrc/linbwd.hip: dX and dW from one read
        # of dY) against the sodt_gemm_tn + sodt_gemm_nt pair
        self.use_fused_linbwd = True
        # bf16, C = 192: backward of attn.qkv (192 -> 576) as ONE launch, three sibling workgroups per M-slice (csrc/linbwd.hip,
        # sodt_linear_bwd_wide), against the sodt_gemm_tn + sodt_gemm_nt pair.  The switch is read live in the backward; the row
        # threshold is read when a block's route is recorded.  Below 85 slices x 16 stages of 32 rows the launch cannot give its
        # 255 workgroups a full pipeline and would occupy a fraction of the CUs the pair fills (derived, not measured).
        self.use_wide_linbwd = True
        self.wide_linbwd_min_rows = 85 * 512
        # bf16, C = 192, MLP_FUSED: dh, dW1 / db1 and dW2 / db2 from ONE launch that recomputes GELU(h) (csrc/mlpbwd.hip, sodt_mlp_bwd:
        # eight sibling workgroups per M-slice, one 96-column slab of the hidden dimension each) against sodt_gemm_tn +
        # sodt_gemm_nt(DGELU_RC) + sodt_gemm_tn; the forward then writes no GELU(h).  Both the switch and the threshold are read when a
        # block's route is recorded (the forward has to know whether GELU(h) is kept).  Below 32 slices x 64 stages of 32 rows the
        # one-off 72 KiB load of the weight slabs is not amortised (derived, not measured).
        self.use_fused_mlp_bwd = True
        self.mlp_bwd_min_rows = 32 * 64 * 32
        # bf16: the Detect level as one pass each way (csrc/detect.hip) against sodt_gemm_nt with the Detect epilogue and
        # sodt_detect_unpermute + sodt_gemm_tn + sodt_gemm_nt; read when a plan's backward is first recorded and at every forward
        self.use_fused_detect = True
        # bf16: the stride-4 C3 forms d(input) of cv1 and cv2 in one GEMM over their concatenated dz (read when the weights are prepared)
        self.use_merged_c3_din = True
        # 2x2-conv MLPs (bf16): fc1 folded into the convolution's weights (csrc/convmlp.hip) - no fc1 GEMM, and in the backward no
        # d(x) = du W1 and no dW1 GEMM; widths above this run the three-GEMM form (the composition kernels are plain f32 loops)
        self.convmlp_fold_maxc = 384
        self.use_direct_conv3 = True   # the head's 3x3 Conv at 64 -> 64 channels on the direct kernels (csrc/conv3.hip) against the nine-segment GEMM
        # 64 MiB of f32 for the per-slice partial tiles of the bf16 weight-gradient GEMMs (largest need: 12.5 M floats)
        self._tn_scratch = torch.empty(16 << 20, dtype=torch.float32, device=self.dev)
        ops.set_tn_scratch(self._tn_scratch)

    # ------------------------------------------------------------------ gradients: one flat f32 buffer
    def _build_grad_buffer(self):
        # layout: freeze.grad_layout ([front end | pos/patch embed | stage 1 | ... | head | SR branch], reverse order of completion)
        self.grad_order, offs, tot = freeze.grad_layout({n: p.numel() for n, p in self.params.items()})
        self.fe_end = offs[self.grad_order[16]]          # the front end's sixteen gradients: [0, fe_end)
        self.flat_grad = torch.zeros(tot, device=self.dev, dtype=torch.float32)
        self.g: Dict[str, torch.Tensor] = {}
        for n in self.grad_order:
            p = self.params[n]
            self.g[n] = self.flat_grad[offs[n]: offs[n] + p.numel()].view(p.shape)
        self.grad_offsets = offs
        self._claim = [(n, p, self.g[n], self.g[n].data_ptr()) for n, p in self.params.items()]      # _claim_grads walks this
        self._ordered = [self.params[n] for n in self.grad_order]                                    # freeze_record reads these
        # first element of the buffer's tail that is complete before the stage-1 backward (see _backward_main)
        self.ddp_split = offs[next(n for n in self.grad_order if n.startswith(E + "pmerging1."))]
        self.ddp_split3 = offs[next(n for n in self.grad_order if n.startswith(E + "stage3."))]
        assert self.ddp_split < self.ddp_split3 and all(
            n.startswith((E + "stage3.", E + "neck3.", "detect.", "model_up.")) for n in self.grad_order if offs[n] >= self.ddp_split3)
        assert all(not n.startswith((E + "stage1.", E + "patch_embed.", E + "pos_embed", E + "channel_embed", E + "chan_block"))
                   for n in self.grad_order if offs[n] >= self.ddp_split)
        fe = offs[E + "channel_embed_r.proj.weight"]
        self.g_fe_w = self.flat_grad[fe: fe + 4 * 48 * 16]
        self.g_fe_b = self.flat_grad[offs[E + "channel_embed_r.proj.bias"]:][: 4 * 48]
        self.g_fe_g = self.flat_grad[offs[E + "chan_block.norm1.weight"]:][: 4 * 48]
        self.g_fe_be = self.flat_grad[offs[E + "chan_block.norm1.bias"]:][: 4 * 48]

    def _build_param_buffer(self):
        """Re-home every parameter into ONE flat f32 buffer with the layout of the gradient buffer (`p.data` become views),
        so that the optimizer step, the EMA and the cast to the run dtype are one streaming kernel over
        (flat_param, flat_grad, momentum, ema) - optim.FusedSGD, csrc/optim.hip - instead of 273 small launches."""
        self.flat_param = torch.zeros_like(self.flat_grad)
        with torch.no_grad():
            for n in self.grad_order:
                p = self.params[n]
                v = self.flat_param[self.grad_offsets[n]: self.grad_offsets[n] + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
        self.flat_cast: Dict[torch.dtype, torch.Tensor] = {}     # run-dtype mirror of flat_param (bf16 path)
        self.param_cast_fresh = False     # True: flat_cast == cast(flat_param) (set by optim.FusedSGD.step, cleared by invalidate_params)
        self._cast_version = -1           # params_version() at the moment the mirror was last made fresh
        self._param_epoch = 0             # bumped by every write params_version() cannot see (optim.FusedSGD.step, invalidate_params)

    def params_version(self) -> int:
        """Sum of the parameters' autograd version counters: every in-place write through the Parameter objects
        (load_state_dict's copy_, a torch optimizer's add_, p.mul_() under no_grad) bumps it.  Writes through `p.data`
        aliases and raw kernels do not: those callers use invalidate_params()."""
        return sum(p._version for p in self.params.values())

    def mark_cast_fresh(self):
        """optim.FusedSGD.step: the fused kernel has just written cast(flat_param) into the mirror."""
        self.param_cast_fresh = True
        self._cast_version = self.params_version()
        self._param_epoch += 1

    def invalidate_params(self):
        """Tell the engine the f32 masters were changed by something other than optim.FusedSGD (load_state_dict, a torch
        optimizer, manual edits): the run-dtype mirror is re-cast at the next forward.  In-place writes through the
        Parameter objects are also detected by their version counters (params_version)."""
        self.param_cast_fresh = False
        self._param_epoch += 1

    def _check_param_views(self):
        for n in self.grad_order:
            p = self.params[n]
            if p.data_ptr() != self.flat_param.data_ptr() + 4 * self.grad_offsets[n]:
                raise RuntimeError(f"{n} no longer lives in the engine's flat parameter buffer (model.to()/.float()/.half() after the "
                                   "first forward re-allocates parameters): rebuild the engine with model._engine = None")

    def freeze_record(self) -> freeze.FreezeRecord:
        """freeze.propagate for the parameters' requires_grad flags as they are now (one record per distinct set of flags)."""
        bits = tuple([p.requires_grad for p in self._ordered])
        fz = self._fz.get(bits)
        if fz is None:
            if len(self._fz) >= 64:
                self._fz.clear()
            frozen = [n for n, b in zip(self.grad_order, bits) if not b]
            fz = self._fz[bits] = freeze.propagate(self.unit_graph, frozen, self.grad_order, self.grad_offsets, self.flat_grad.numel())
        return fz

    def _claim_grads(self, frozen=None):
        """Make the trainable parameters' .grad the views of the flat buffer; returns whether the gradients were reset (the caller
        zeroes the buffer).  frozen: the names the coming backward treats as frozen (default: requires_grad as it is now).  A
        frozen parameter's .grad is never a view: torch leaves it None, so a view left from the time the parameter was trainable
        is dropped and its slice of the buffer cleared.  Every frozen slice is zero when a backward returns, so a parameter that
        was frozen at the latest backward takes its view back without counting as a reset."""
        if frozen is None:
            frozen = self.freeze_record().frozen
        fresh = False
        dropped = []
        held = claimed = 0
        for n, p, v, ptr in self._claim:
            g = p.grad
            if n in frozen:
                if g is not None and g.data_ptr() == ptr:
                    p.grad = None
                    dropped.append(n)
            elif g is None:
                p.grad = v
                claimed += 1
                fresh = fresh or n not in self._was_frozen
            elif g.data_ptr() != ptr:
                raise RuntimeError(f"{n}.grad is not the engine's flat-buffer view; use optimizer.zero_grad(set_to_none=True) "
                                   "or leave .grad untouched between steps")
            else:
                held += 1
        fresh = fresh or (claimed > 0 and held == 0)      # no trainable parameter held a gradient: nothing is being accumulated
        self._was_frozen = frozen
        if dropped and not fresh:
            drop = set(dropped)
            start = None
            for n in self.grad_order + [None]:            # neighbours in the buffer: one memset per run
                if n in drop:
                    start = self.grad_offsets[n] if start is None else start
                elif start is not None:
                    ops.zero_(self.flat_grad[start: self.flat_grad.numel() if n is None else self.grad_offsets[n]])
                    start = None
        return fresh

    # ------------------------------------------------------------------ prepared parameters
    def _prep_for(self, dt):
        P = self.prep.get(dt)
        if P is not None:
            return P
        dev = self.dev
        w: Dict[str, torch.Tensor] = {}
        wT: Dict[str, torch.Tensor] = {}
        tab_t, tab_f = ops.PrepTable(), ops.PrepTable()       # run-dtype destinations / f32 destinations

        # run-dtype mirror of the whole parameter buffer: every weight whose GEMM layout [N][K] IS its storage layout (all
        # nn.Linear and 1x1 Conv2d weights, pos_embed) is a VIEW of it - no per-step permute / cast launch for them; f32 runs
        # view the masters themselves
        if dt == torch.float32:
            mirror = self.flat_param
        else:
            mirror = self.flat_cast.get(dt)
            if mirror is None:
                mirror = self.flat_cast[dt] = torch.zeros_like(self.flat_param, dtype=dt)

        def mview(n, shape):
            o = self.grad_offsets[n]
            return mirror[o: o + self.params[n].numel()].view(shape)
        for n, p in self.params.items():
            if p.dim() < 2 or "relative_position_bias_table" in n or "channel_embed" in n or n.startswith("model_up."):
                continue        # (model_up: sr.SRBranch lays its own weights out)
            if n == E + "pos_embed":
                t = p.shape[1]
                w[n] = mview(n, (t * t, 192))
                continue
            N, K = p.shape[0], p.shape[1]
            taps = p.numel() // (N * K)
            Np = (N + 15) // 16 * 16 if n.startswith(self.det_name) else N     # Detect: 39 -> 48 zero-padded
            if taps == 1 and Np == N:
                w[n] = mview(n, (N, K))
            else:
                w[n] = torch.zeros(Np, taps * K, device=dev, dtype=dt)       # [N][tap*K + k]
                tab_t.add(p, w[n], (N, K, taps), (0, 2, 1), taps * K)
            wT[n] = torch.zeros(K, taps * Np, device=dev, dtype=dt)          # [K][tap*N + n]
            tab_t.add(p, wT[n], (N, K, taps), (1, 2, 0), taps * Np)
        # C3 units whose cv1 / cv2 input gradient runs as one GEMM (_c3_bwd): [cv1.weight^T | cv2.weight^T], [c1][2 c_].  bf16 rows of
        # at most 384 bytes only - the B-stationary kernel's range, the route the two separate launches take today
        wT12: Dict[str, torch.Tensor] = {}
        if dt == torch.bfloat16 and self.use_merged_c3_din:
            for u in self.head.units:
                if u.kind == "C3" and 2 * u.c2 <= 384 and u.c2 % 64 == 0:
                    pn = f"detect.{u.k}."
                    p1, p2 = self.params[pn + "cv1.conv.weight"], self.params[pn + "cv2.conv.weight"]
                    c_, c1 = p1.shape[0], p1.shape[1]
                    w12 = torch.zeros(c1, 2 * c_, device=dev, dtype=dt)
                    tab_t.add(p1, w12, (c_, c1, 1), (1, 2, 0), 2 * c_)
                    tab_t.add(p2, w12[:, c_:], (c_, c1, 1), (1, 2, 0), 2 * c_)
                    wT12[pn] = w12
        # Linear MLPs on the bf16 path keep only the activation: the backward GEMM recomputes the pre-activation from
        # [fc1.weight | fc2.weight^T] ([4C][2C]) in its first K half (SODT_EPI_DGELU_RC)
        wcat: Dict[str, torch.Tensor] = {}
        if dt == torch.bfloat16:
            for n, p in self.params.items():
                if n.endswith("mlp.fc1.weight") and p.dim() == 2 and p.shape[0] == 4 * p.shape[1]:
                    Cc = p.shape[1]
                    p2 = self.params[n.replace("fc1", "fc2")]
                    wc = torch.zeros(4 * Cc, 2 * Cc, device=dev, dtype=dt)
                    tab_t.add(p, wc, (4 * Cc, Cc, 1), (0, 2, 1), 2 * Cc)
                    tab_t.add(p2, wc[:, Cc:], (Cc, 4 * Cc, 1), (1, 2, 0), 2 * Cc)
                    wcat[n] = wc
        # 2x2-conv MLPs with fc1 folded into the convolution: composed weights (re-made every forward by sodt_convmlp_compose)
        cmlp: Dict[str, Dict[str, torch.Tensor]] = {}
        if dt == torch.bfloat16:
            for n, p in self.params.items():
                if n.endswith("mlp.conv1.weight") and p.dim() == 4 and tuple(p.shape[2:]) == (2, 2) and p.shape[0] == p.shape[1]:
                    Cc = p.shape[0]
                    if Cc <= self.convmlp_fold_maxc and Cc % 64 == 0:
                        cmlp[n[: -len("mlp.conv1.weight")]] = dict(
                            weff=torch.zeros(Cc, 4 * Cc, device=dev, dtype=dt), weffT=torch.zeros(Cc, 4 * Cc, device=dev, dtype=dt),
                            beff=torch.zeros(Cc, device=dev), vtap=torch.zeros(4, Cc, device=dev))
        # f32 side: transposed relative-position tables, packed front-end parameters
        bias_t: Dict[str, torch.Tensor] = {}
        for n, p in self.params.items():
            if "relative_position_bias_table" in n:
                bias_t[n] = torch.zeros(p.shape[1], p.shape[0], device=dev, dtype=torch.float32)
                tab_f.add(p, bias_t[n], (p.shape[0], p.shape[1], 1), (1, 0, 2), p.shape[0])
        fe = {k: torch.zeros(4 * 48 * (16 if k == "w" else 1), device=dev, dtype=torch.float32) for k in ("w", "b", "g", "be")}
        for ci, c in enumerate("rgbi"):
            tab_f.add(self.params[E + f"channel_embed_{c}.proj.weight"], fe["w"][ci * 768:], (48, 16, 1), (0, 1, 2), 16)
            tab_f.add(self.params[E + f"channel_embed_{c}.proj.bias"], fe["b"][ci * 48:], (48, 1, 1), (0, 1, 2), 1)
            tab_f.add(self.params[E + f"chan_block.norm{ci + 1}.weight"], fe["g"][ci * 48:], (48, 1, 1), (0, 1, 2), 1)
            tab_f.add(self.params[E + f"chan_block.norm{ci + 1}.bias"], fe["be"][ci * 48:], (48, 1, 1), (0, 1, 2), 1)

        # fused W-MSA block kernel (csrc/wmsa_block.hip): one stage-ordered parameter pack per eligible block
        wmsa: Dict[str, torch.Tensor] = {}
        code = L.BF16 if dt == torch.bfloat16 else L.F32
        enc = self.model.image_encoder
        for sname in ("stage1", "stage2", "stage3"):
            for i, blk in enumerate(getattr(enc, sname)):
                nb = ops.wmsa_pack_bytes(blk.dim, HEADS, blk.window_size, code) if self.use_fused_wmsa else 0
                if nb > 0:
                    wmsa[E + f"{sname}.{i}."] = torch.zeros(nb // (2 if dt == torch.bfloat16 else 4), device=dev, dtype=dt)

        P = dict(w=w, wT=wT, wT12=wT12, wcat=wcat, cmlp=cmlp, bias_t=bias_t, fe=fe, tab_t=tab_t.upload(dev), tab_f=tab_f.upload(dev), dt=dt,
                 ones={}, wmsa=wmsa)
        self.prep[dt] = P
        return P

    def _run_prep(self, P):
        P["tab_t"].run(L.BF16 if P["dt"] == torch.bfloat16 else L.F32)
        P["tab_f"].run(L.F32)
        p = self.params
        for pre, wpk in P["wmsa"].items():
            ops.wmsa_pack(p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"], p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"],
                          p[pre + "attn.relative_position_bias_table"], p[pre + "norm1.weight"], p[pre + "norm1.bias"],
                          p[pre + "norm2.weight"], p[pre + "norm2.bias"], wpk, p[pre + "attn.qkv.weight"].shape[1], HEADS, 8)

    # ------------------------------------------------------------------ public entry
    MAX_PLANS = 4      # each plan owns a full activation workspace (31 GB at B=8 @1024^2 bf16): least recently used goes

    def run(self, x_rgb, x_ir, dt, training):
        if x_rgb.dim() != 4 or x_rgb.shape[1] != 3 or x_ir.dim() != 4:
            raise ValueError("expected x_rgb (B,3,H,W) and x_ir (B,>=1,H,W)")
        B, _, H, W = x_rgb.shape
        if H % 32 or W % 32:
            raise ValueError(f"H and W must be multiples of 32 (4x patch stride, 8x8 windows on t/2 .. even t/4), got {H} x {W}")
        if x_ir.shape[0] != B or x_ir.shape[1] < 1 or tuple(x_ir.shape[-2:]) != (H, W):
            raise ValueError(f"x_ir must be (B={B}, >=1, {H}, {W}) like x_rgb, got {tuple(x_ir.shape)}")
        if H != W and self.sr:
            raise NotImplementedError(f"Model(sr=True) runs square inputs only: the super-resolution branch is not built for {H} x {W}")
        if H // 4 == self.img_t and W // 4 != self.img_t:
            # backbone_vit.py:215-217 compares the ROWS alone and then fails to broadcast; say so before any launch
            raise ValueError(f"pos_embed is {self.img_t} x {self.img_t} tokens: a {H} x {W} input has its {H // 4} rows and {W // 4} columns, "
                             "which the reference adds and cannot broadcast (backbone_vit.py:215-217); use another height")
        S = H if H == W else (H, W)
        if x_rgb.device != self.dev or x_ir.device != self.dev:
            raise ValueError(f"inputs must be on the model's device {self.dev} (got {x_rgb.device}, {x_ir.device}): "
                             "the kernels take raw device pointers")
        x_rgb = x_rgb.float().contiguous()
        x_ir = x_ir.float().contiguous()
        psb = bool(getattr(self.model, "pad_shifted_blocks", False))
        if psb != self.pad_shifted_blocks:
            self.pad_shifted_blocks = psb
            self.plans.clear()                                   # recorded launch lists hold the routes of the other setting
        sbn = bool(getattr(self.model, "sync_bn", False))
        sbn_on = sync_bn_in_force(sbn, self.ddp)
        if sbn != self.sync_bn or sbn_on != self._sbn_on:
            self.sync_bn, self._sbn_on = sbn, sbn_on
            self.plans.clear()                                   # the launch lists of the other setting stop elsewhere, for other collectives
        # a training plan belongs to one set of requires_grad flags (its launch lists and its workspace follow them), read here at
        # every forward: freezing at an epoch boundary (Train.py:328-333) needs no call.  Eval plans save nothing and have no
        # backward: one plan whatever the flags (an EMA copy is frozen throughout).
        fz = self.freeze_record() if training else None
        key = (B, S, dt, training, fz.signature) if training else (B, S, dt, training)
        plan = self.plans.pop(key, None)
        if plan is None:
            while len(self.plans) >= self.MAX_PLANS:
                self.plans.pop(next(iter(self.plans)))          # dicts keep insertion order: the first key is the LRU one
            if training and self._sbn_on:
                self._check_rank_shapes(B, H, W)
            plan = Plan(B, S, dt, training, self.dev, fz)
        self.plans[key] = plan                                   # (re)insert as most recently used
        out_sr = None
        if training and torch.is_grad_enabled():
            pred = _EngineFn.apply(self, plan, x_rgb, x_ir, self._anchor)
            if self.sr:
                pred, out_sr = pred
        else:
            pred = self._forward(plan, x_rgb, x_ir)
            if self.sr and training:                              # model.py:284-287: the branch runs in training mode only
                out_sr = self._sr_forward(plan)
        return pred, self._features(plan), out_sr

    def _check_rank_shapes(self, B, H, W):
        """Synchronised BatchNorm counts M * world rows and gives every rank's sums the same weight: every rank must run the same
        per-rank batch.  One all_gather per new training plan, so a mismatch raises on every rank, before any statistics
        collective of the plan (a rank that stopped alone would leave the others waiting in theirs)."""
        shapes = self.ddp.gather_shapes(B, H, W)
        if any(s != shapes[0] for s in shapes):
            raise RuntimeError(f"sync_bn: the ranks run different per-rank batches (B, H, W) = {shapes}: synchronised BatchNorm "
                               "needs the same batch size and image size on every rank (uneven batches are not built)")

    def _sbn_fwd_collective(self, stats):
        """the conv's f64 column sums [SODT_STATS_REPL][2][C] (one contiguous slice of zero pool "f") become those of every rank"""
        self.ddp.all_reduce_stats(stats)

    def _sbn_bwd_collective(self, red, red_all):
        """red_all = sum over the ranks of red, the BN-backward sums [2][C] f64; red stays this rank's own (dgamma / dbeta)"""
        red_all.copy_(red)
        self.ddp.all_reduce_stats(red_all)

    def decode(self, pred):
        B, na, ny, nx, no = pred.shape
        z = torch.empty(B, na * ny * nx, no, device=pred.device, dtype=torch.float32)
        ag = self.buffers[self.det_name + "anchor_grid"].reshape(-1).contiguous().float()
        ops.detect_decode(pred, ag, z, B, na, ny, nx, no, 4.0)
        return z

    def decode_tta(self, pred, z, row_off, si, flip, img_h, img_w):
        """decode of one pass of the augmented forward into rows row_off .. row_off + na * ny * nx of z (B, rows, no), with the
        de-scale and de-flip of model.py:178-182; returns the row after the slice."""
        B, na, ny, nx, no = pred.shape
        ag = self.buffers[self.det_name + "anchor_grid"].reshape(-1).contiguous().float()
        ops.detect_decode_tta(pred, ag, z, B, na, ny, nx, no, 4.0, row_off, si, flip, img_h, img_w)
        return row_off + na * ny * nx

    def _features(self, plan):
        """y[0..10] of forward_once (model.py:246,281) as NCHW *views* of the workspace (valid until the
        next forward).  y4, y5, y8, y9 (upsample / concat) are never materialised by the kernels: the list
        builds them with torch on first access (``_LazyFeatures``), so callers that index them get tensors
        as in the reference and nobody else pays for them."""
        B, th, tw = plan.B, plan.H // 4, plan.W // 4
        b = plan.bufs

        def nchw(name, level, c):
            return b[name].view(B, th >> level, tw >> level, c).permute(0, 3, 1, 2)
        items = [nchw("f0", 0, 256), nchw("f1", 1, 256), nchw("f2", 2, 512)] + [None] * self.head.nd
        for u in self.head.units:
            items[3 + u.k] = nchw(u.out_name, u.level, u.c2)
        y = _LazyFeatures(items, self.head.rules)
        if self.model.materialize_features:
            for i in sorted(self.head.rules):
                y[i]
        return y

    # ================================================================== forward
    def _forward(self, plan: Plan, x_rgb, x_ir):
        P = self._prep_for(plan.dt)
        B, H, W = plan.B, plan.H, plan.W
        th, tw = H // 4, W // 4
        T1 = B * th * tw
        plan.gen += 1          # the saved activations of an earlier forward on this plan are gone (see _EngineFn.backward)
        # (0) run-dtype mirror of the masters: written by the fused optimizer step; re-cast here when anything else may have
        #     changed them (live call: the decision is per step)
        if plan.dt != torch.float32:
            ver = self.params_version()
            if not self.param_cast_fresh or ver != self._cast_version:
                ops.cast(self.flat_param, self.flat_cast[plan.dt], self.flat_param.numel())
                # stays valid until the masters change: fresh only when an optimizer that maintains the mirror is stepping
                self._cast_version = ver
        # (1) parameter preparation (recorded)
        if plan.fwd_pre is None:
            with ops.Recorder() as rec:
                self._run_prep(P)
            plan.fwd_pre = rec.calls
        else:
            ops.replay(plan.fwd_pre)
        # (2) front end: live call (input pointers change per step)
        x0 = plan.buf("x0", (T1, 192))
        fe = P["fe"]
        cb = self.model.image_encoder.chan_block
        ca_ws, ca_shift = int(cb.window_size), int(cb.shift_size)
        irs = x_ir.shape[1] * H * W
        if ca_ws == 1:      # the shipped configuration (backbone_vit.py:438): fused kernel
            ops.frontend_fwd(x_rgb, x_ir, irs, fe["w"], fe["b"], fe["g"], fe["be"], x0, B, H, W)
        else:               # general window / shift form of CAttentionBlock
            e = plan.buf("fe.e", (T1, 192), torch.float32)
            ops.patch_embed4_fwd(x_rgb, x_ir, irs, fe["w"], fe["b"], e, B, H, W)
            ops.cross_attn_ln_fwd(e, fe["g"], fe["be"], x0, B, H, W, ca_ws, ca_shift)
        # (3) encoder + head (recorded)
        if plan.fwd_main is None:
            with ops.Recorder() as rec:
                self._forward_main(plan, P)
            plan.fwd_main = rec.calls
        else:
            self._sync_bn_momentum(plan)
            if plan.sbn_fwd:
                # synchronised BatchNorm: replay in segments that end in front of every sodt_bn_finalize, whose statistics are
                # all-reduced there (the recording issued the same collectives inline, in the same order)
                pos = 0
                for idx, stats in plan.sbn_fwd:
                    ops.replay(plan.fwd_main, probes=self.probes_fwd, start=pos, end=idx)
                    self._sbn_fwd_collective(stats)
                    pos = idx
                ops.replay(plan.fwd_main, probes=self.probes_fwd, start=pos)
            else:
                self._replay(plan, "fwd_main", plan.fwd_main, self.probes_fwd)
        # (4) Detect: live (fresh output tensor every call)
        pred = torch.empty(B, self.na, th, tw, self.no, device=self.dev, dtype=torch.float32)
        hrow, hc = self.head.head_out
        hx, wd, bd = self._ref_buf(plan, Ref("unit", hrow)), P["w"][self.det_name + "m.0.weight"], self.params[self.det_name + "m.0.bias"]
        if not (self.use_fused_detect and ops.detect_fused_ok(hc, self.na, self.no, plan.dt)
                and ops.detect_fwd(hx, wd, bd, pred, B, th * tw, self.na, self.no, hc)):
            ops.gemm_nt([SegSpec(hx)], wd, pred, T1, self.na * self.no, hc, bias=bd, detect=(self.na, self.no, th * tw))
        return pred

    @staticmethod
    def _bn_momentum(bn, name):
        """bn.momentum as sodt_bn_finalize takes it (bypass_bn.disable_running_stats sets 0: the running statistics stand still)"""
        m = bn.momentum
        if m is None:
            raise NotImplementedError(f"{name}: BatchNorm2d(momentum=None), the cumulative moving average, is not built")
        return float(m)

    def _sync_bn_momentum(self, plan: Plan):
        """Every Conv's bn.momentum is read at every training forward: a recorded sodt_bn_finalize whose BatchNorm2d has
        another momentum now than at its recording is re-recorded with the new one (its last argument).  A hipGraph captured
        from the list holds the arguments of its capture, so it is set aside under the momenta it was captured with and taken
        back when they return (bypass_bn alternates between two sets: one capture each, nothing re-captured per step and no
        graph destroyed while a replay of it may still run)."""
        was_sig = None
        for mk in plan.bn_marks:
            idx, bn, name, was = mk
            if bn.momentum != was:
                m = self._bn_momentum(bn, name)
                if was_sig is None:
                    was_sig = tuple(k[3] for k in plan.bn_marks)
                fn, args, cname, tag = plan.fwd_main[idx]
                assert cname == "sodt_bn_finalize", cname
                plan.fwd_main[idx] = (fn, args[:-1] + (C.c_float(m),), cname, tag)
                mk[3] = m
        if was_sig is None or not any(k == "fwd_main" or (isinstance(k, tuple) and k[0] == "fwd_main") for k in plan.graphs):
            return
        g = plan.graphs.pop("fwd_main", None)
        if g is not None:
            kept = [k for k in plan.graphs if isinstance(k, tuple) and k[0] == "fwd_main"]
            if len(kept) >= 4:              # a momentum that keeps moving: let the oldest capture go, once nothing can be replaying it
                torch.cuda.current_stream().synchronize()
                del plan.graphs[kept[0]]
            plan.graphs[("fwd_main", was_sig)] = g
        g = plan.graphs.pop(("fwd_main", tuple(k[3] for k in plan.bn_marks)), None)
        if g is not None:
            plan.graphs["fwd_main"] = g

    def _replay(self, plan: Plan, key: str, calls, probes):
        """Re-issue a recorded launch list.  With SODT_HIPGRAPH=1 (single-process runs without probes) the list is captured
        into a hipGraph on its first replay - every launch goes to the caller's stream and all pointers are plan-owned, so the
        capture is exact - and the graph is launched from then on: one host call instead of ~350 ctypes calls per list.
        Off by default: the step is GPU-bound (43 ms of kernels against ~0.5 ms of host replay that runs ahead of the GPU;
        185.6 vs 185.3 img/s measured), and the data-parallel path replays in segments around its all-reduce buckets."""
        if probes or not USE_HIPGRAPH or self.ddp is not None:
            ops.replay(calls, probes=probes)
            return
        g = plan.graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(g, stream=side):
                ops.replay(calls)
            torch.cuda.current_stream().wait_stream(side)
            plan.graphs[key] = g
        g.replay()

    def _forward_main(self, plan: Plan, P):
        B = plan.B
        H, W = plan.H // 4, plan.W // 4
        p, w = self.params, P["w"]
        T1 = B * H * W
        x0 = plan.bufs["x0"]
        if plan.training and not self.fused:
            ops.zero_(plan.zpool("f"))               # BatchNorm column-statistics accumulators of every head conv
        # 1x1 token-mixing conv + bias + pos_embed (only when the rows match: backbone_vit.py:215-217; rows that match with columns
        # that do not were refused by run())
        x = plan.buf("xe", (T1, 192))
        use_pos = (H == self.img_t and W == self.img_t)
        plan.saved["use_pos"] = use_pos
        ops.gemm_nt([SegSpec(x0)], w[E + "patch_embed.proj.weight"], x, T1, 192, 192, bias=p[E + "patch_embed.proj.bias"],
                    resid=w[E + "pos_embed"] if use_pos else None, rmod=H * W if use_pos else 0)
        enc = self.model.image_encoder
        outs = {}
        for i, blk in enumerate(enc.stage1):
            x = self._block_fwd(plan, P, f"stage1.{i}", blk, x, B, H, W)
            outs[i] = x
        f0 = plan.buf("f0", (T1, 256))
        ops.gemm_nt([SegSpec(outs[4]), SegSpec(outs[5])], w[E + "neck1.weight"], f0, T1, 256, 384)
        x = self._merge_fwd(plan, P, "pmerging1", x, B, H, W, 192)
        H, W = H // 2, W // 2
        for i, blk in enumerate(enc.stage2):
            x = self._block_fwd(plan, P, f"stage2.{i}", blk, x, B, H, W)
        T2 = B * H * W
        f1 = plan.buf("f1", (T2, 256))
        ops.gemm_nt([SegSpec(x)], w[E + "neck2.weight"], f1, T2, 256, 384)
        x = self._merge_fwd(plan, P, "pmerging2", x, B, H, W, 384)
        H, W = H // 2, W // 2
        for i, blk in enumerate(enc.stage3):
            x = self._block_fwd(plan, P, f"stage3.{i}", blk, x, B, H, W)
        T3 = B * H * W
        f2 = plan.buf("f2", (T3, 512))
        ops.gemm_nt([SegSpec(x)], w[E + "neck3.weight"], f2, T3, 512, 768)
        # ---- head (models/model.yaml:65-74 and the variants headgraph.parse_head accepts), token-major
        self._head_fwd(plan, P)

    def _head_fwd(self, plan: Plan, P):
        B, th, tw = plan.B, plan.H // 4, plan.W // 4
        for u in self.head.units:
            H, W = th >> u.level, tw >> u.level
            M = B * H * W
            tag, pname = f"h{u.k}", f"detect.{u.k}."
            plain = all(p.shr == 0 for p in u.parts) and ((u.kind == "Conv" and u.ksize == 1) or u.kind == "SPP")
            segs = []
            for ref, c, shr in u.parts:
                src = self._ref_buf(plan, ref)
                segs.append(SegSpec(src) if plain else SegSpec(src, c, 0, 0, 0, 1, shr, H >> shr, W >> shr))
            if u.kind == "Conv":
                if u.ksize == 3:
                    segs = [SegSpec(s_.t, s_.klen, 0, dy, dx, 1, s_.shr, s_.Hi, s_.Wi) for (dy, dx) in TAPS3 for s_ in segs]
                self._conv_fwd(plan, P, tag, pname, segs, None if plain else (H, W), M, u.c1 * u.ksize ** 2, u.c2, u.ksize)
            elif u.kind == "C3":
                self._c3_fwd(plan, P, tag, pname, segs, (H, W), M, u.c1, u.c2)
            else:
                self._spp_fwd(plan, P, tag, pname, segs, (H, W), M, u.c1, u.c2, B)

    def _ref_buf(self, plan, ref):
        """the plan buffer a headgraph.Ref names: an encoder output or a head unit's output"""
        return plan.bufs[f"f{ref.index}" if ref.kind == "enc" else self.head.by_row[ref.index].out_name]

    # ------------------------------------------------------------------ Swin block
    def _block_geo(self, blk, H, W):
        ws, shift = blk.window_size, blk.shift_size
        if min(H, W) <= ws:
            ws, shift = min(H, W), 0
            if ws < 8 or 64 % ws:
                raise NotImplementedError(f"a {H}x{W}-token stage is ONE {ws}x{ws} window (backbone_vit.py:1042-1045: no partition below "
                                          "the window size); the attention kernels walk 64-token tiles of whole window rows (window "
                                          "side 8, 16 or 32): below S = 576 use S = 128, 256 or 512 (from 576 on every multiple of 64 runs); "
                                          "an H x W input takes min(H, W) for S here")
        L2 = 2 * ws - 1
        if blk.attn.relative_position_bias_table.shape[0] != L2 * L2:
            raise ValueError(f"input resolution gives a {ws}x{ws} window but the model was built with a "
                             f"{blk.attn.window_size[0]}-window bias table; build Model with the matching img_size")
        return ws, shift

    def _block_route(self, plan, P, tag, blk, x_in, B, H, W) -> BlockRoute:
        """Decide, once, which launches run this block: the forward follows the record and the backward reads it back."""
        pre = E + tag + "."
        Cc, M = blk.dim, B * H * W
        ws, shift = self._block_geo(blk, H, W)
        # Resolution not a multiple of the window: the reference zero-pads AFTER norm1 and crops after the attention
        # (backbone_vit.py:619-672, window_partition / window_unpartition), so a pad token enters the attention as the qkv BIAS.
        # Unshifted blocks (stage 3 at S = 640, 768, ...: 40 x 40, 48 x 48 tokens against the 32-token window) run through the
        # spatial K-segments: the QKV GEMM writes the padded grid (rows outside read zeros), the attention runs on it, the
        # projection reads it back cropped.  Shifted blocks also need the reference's roll and mask of the UNPADDED grid: with
        # pad_shifted_blocks they run on the unpadded tensors, the padded grid being index arithmetic inside
        # sodt_window_attn_sp_fwd / _bwd (8-token windows: stage 2 at S % 64 == 32); without the switch they are refused.
        Hp, Wp = H + (-H) % ws, W + (-W) % ws
        pad = (Hp, Wp) if (Hp, Wp) != (H, W) else None
        if pad and shift > 0 and not (self.pad_shifted_blocks and ws == 8):
            raise NotImplementedError(f"{tag}: {H}x{W} tokens are not a multiple of the {ws}-token window of a SHIFTED block (the "
                                      "reference's zero padding, backbone_vit.py:619-643, is built for unshifted blocks only): choose "
                                      "an input size S that is a multiple of 64")
        wpk = P["wmsa"].get(pre) if (ws == 8 and H % 8 == 0 and W % 8 == 0) else None
        if wpk is not None:
            # q / k / v are saved by the f32 parity kernel only (sodt_window_attn_bwd_wm reads them back); the bf16 backward
            # recomputes them from xn1 and the parameter pack (sodt_wmsa_block_bwd): 604 MB less written per launch
            attn = ATTN_FUSED_SAVED if plan.dt == torch.float32 else ATTN_FUSED_RC
        else:
            attn = (ATTN_SHIFT_PAD if shift > 0 else ATTN_PADDED) if pad else ATTN_PLAIN
        if blk.mlp.linear:
            # Linear MLPs on the bf16 path keep only GELU(h): the backward recomputes h inside the dh GEMM
            rc = ops.mlp_recompute_ok(M, Cc, plan.dt) and (pre + "mlp.fc1.weight") in P["wcat"]
            if rc and self.use_fused_mlp and ops.mlp_fused_ok(M, Cc, plan.dt):
                mlp = MLP_FUSED
            else:
                mlp = MLP_LIN_RC if rc else MLP_LIN_SAVED
        else:
            mlp = MLP_FOLD if pre in P["cmlp"] else MLP_CONV
        # the one-launch MLP backward accumulates all four of fc1 / fc2 weight and bias: one frozen parameter keeps today's launches
        T = getattr(plan, "trainable", None)
        mlp_bwd = mlp == MLP_FUSED and self.use_fused_mlp_bwd and Cc == 192 and M >= self.mlp_bwd_min_rows and \
            (T is None or all(T(pre + n) for n in ("mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")))
        return BlockRoute(x_in, (B, H, W, Cc, ws, shift), pad, attn, wpk, mlp, zscratch=wpk is None and ws * ws > 64,
                          sq_ok=pad is None and plan.dt == torch.bfloat16 and Cc == 192,
                          wide_ok=plan.dt == torch.bfloat16 and Cc == 192 and attn != ATTN_PADDED and M >= self.wide_linbwd_min_rows,
                          mlp_bwd=mlp_bwd)

    def _block_fwd(self, plan, P, tag, blk, x_in, B, H, W):
        ops.set_tag(tag)
        r = plan.saved[tag] = self._block_route(plan, P, tag, blk, x_in, B, H, W)
        xm, xn2 = self._attn_fwd(plan, P, tag, r)
        return self._mlp_fwd(plan, P, tag, r, xm, xn2)

    def _attn_fwd(self, plan, P, tag, r: BlockRoute):
        """xm = x_in + proj(attention(LN1(x_in))), xn2 = LN2(xm); returns (xm, xn2)."""
        p, w = self.params, P["w"]
        pre = E + tag + "."
        x_in, (B, H, W, Cc, ws, shift) = r.x_in, r.geo
        M = B * H * W
        bias_t = P["bias_t"][pre + "attn.relative_position_bias_table"]
        # what the backward of the attention half (sa) and of the MLP half (sm) read back: kept per block only where that half's
        # backward runs (freeze.py); a frozen block below every trainable parameter runs the eval plan's launches
        sa, sm = plan.saves(tag + ".attn"), plan.saves(tag + ".mlp")
        if r.attn in (ATTN_FUSED_RC, ATTN_FUSED_SAVED) and plan.training and not (sa or sm):
            xm = plan.keep(False, tag + ".xm", "xm", (M, Cc))
            xn2 = plan.keep(False, tag + ".xn2", "xn2", (M, Cc))
            ops.wmsa_block_fwd(x_in, r.wpk, xm, xn2, None, None, None, None, None, None, B, H, W, Cc, HEADS, ws, shift)
            return xm, xn2
        xn1 = plan.keep(sa, tag + ".xn1", "xn1", (M, Cc))
        st1 = plan.keep(sa, tag + ".st1", "st1", (M, 2), torch.float32)
        xm = plan.keep(sm, tag + ".xm", "xm", (M, Cc))
        xn2 = plan.keep(sm, tag + ".xn2", "xn2", (M, Cc))
        st2 = plan.keep(sm, tag + ".st2", "st2", (M, 2), torch.float32)
        if r.attn in (ATTN_FUSED_RC, ATTN_FUSED_SAVED):
            # LN1 + QKV + window attention + proj + residual + LN2 in ONE launch (csrc/wmsa_hg.hip / wmsa_block.hip); training also
            # writes what the backward needs: xn1, the attention output, the LayerNorm statistics and the window-major
            # log-sum-exp (and q / k / v where the backward reads them back).  The launch saves all of it or nothing: one half
            # that saves makes it save for both.
            ao = plan.keep(sa, tag + ".ao", "ao", (M, Cc))
            qkvw = plan.keep(sa, tag + ".qkvw", "qkvw", (M // 64, HEADS, 3, 64, Cc // HEADS)) if (plan.training and r.attn == ATTN_FUSED_SAVED) else None
            lsew = plan.keep(sa, tag + ".lsew", "lsew", (M // 64, HEADS, 64), torch.float32)
            if plan.training:
                ops.wmsa_block_fwd(x_in, r.wpk, xm, xn2, st1, st2, xn1, qkvw, lsew, ao, B, H, W, Cc, HEADS, ws, shift)
            else:
                ops.wmsa_block_fwd(x_in, r.wpk, xm, xn2, None, None, None, None, None, None, B, H, W, Cc, HEADS, ws, shift)
            return xm, xn2
        ops.layernorm_fwd(x_in, p[pre + "norm1.weight"], p[pre + "norm1.bias"], xn1, st1, M, Cc)
        if r.attn == ATTN_PADDED:
            Hp, Wp = r.pad
            Mp = B * Hp * Wp
            qkv = plan.keep(sa, tag + ".qkv", "qkv", (Mp, 3 * Cc))
            ops.gemm_nt([SegSpec(xn1, Cc, 0, 0, 0, 1, 0, H, W)], w[pre + "attn.qkv.weight"], qkv, Mp, 3 * Cc, Cc, spatial=(Hp, Wp),
                        bias=p[pre + "attn.qkv.bias"])
            lse = plan.keep(sa, tag + ".lse", "lse", (Mp, HEADS), torch.float32)
            aop = plan.keep(sa, tag + ".aop", "aop", (Mp, Cc))
            ops.window_attn_fwd(qkv, bias_t, aop, lse, B, Hp, Wp, Cc, HEADS, ws, 0)
            ops.gemm_nt([SegSpec(aop, Cc, 0, 0, 0, 1, 0, Hp, Wp)], w[pre + "attn.proj.weight"], xm, M, Cc, Cc, spatial=(H, W),
                        bias=p[pre + "attn.proj.bias"], resid=x_in)
        elif r.attn == ATTN_SHIFT_PAD:
            # every tensor on the unpadded grid: a pad key reads qkv.bias inside the kernel, a pad query is never computed
            ao = plan.keep(sa, tag + ".ao", "ao", (M, Cc))
            qkv = plan.keep(sa, tag + ".qkv", "qkv", (M, 3 * Cc))
            ops.gemm_nt([SegSpec(xn1)], w[pre + "attn.qkv.weight"], qkv, M, 3 * Cc, Cc, bias=p[pre + "attn.qkv.bias"])
            lse = plan.keep(sa, tag + ".lse", "lse", (M, HEADS), torch.float32)
            ops.window_attn_sp_fwd(qkv, p[pre + "attn.qkv.bias"], bias_t, ao, lse, B, H, W, Cc, HEADS, ws, shift)
            ops.gemm_nt([SegSpec(ao)], w[pre + "attn.proj.weight"], xm, M, Cc, Cc, bias=p[pre + "attn.proj.bias"], resid=x_in)
        else:
            ao = plan.keep(sa, tag + ".ao", "ao", (M, Cc))
            qkv = plan.keep(sa, tag + ".qkv", "qkv", (M, 3 * Cc))
            ops.gemm_nt([SegSpec(xn1)], w[pre + "attn.qkv.weight"], qkv, M, 3 * Cc, Cc, bias=p[pre + "attn.qkv.bias"])
            lse = plan.keep(sa, tag + ".lse", "lse", (M, HEADS), torch.float32)
            ops.window_attn_fwd(qkv, bias_t, ao, lse, B, H, W, Cc, HEADS, ws, shift)
            ops.gemm_nt([SegSpec(ao)], w[pre + "attn.proj.weight"], xm, M, Cc, Cc, bias=p[pre + "attn.proj.bias"], resid=x_in)
        ops.layernorm_fwd(xm, p[pre + "norm2.weight"], p[pre + "norm2.bias"], xn2, st2, M, Cc)
        return xm, xn2

    def _mlp_fwd(self, plan, P, tag, r: BlockRoute, xm, xn2):
        """xo = xm + MLP(xn2); returns xo."""
        p, w = self.params, P["w"]
        pre = E + tag + "."
        B, H, W, Cc, _, _ = r.geo
        M = B * H * W
        xo = plan.buf(tag + ".xo", (M, Cc))
        sm = plan.saves(tag + ".mlp")
        if r.mlp == MLP_FUSED:
            # fc1 + GELU + fc2 + residual in ONE launch (csrc/mlp.hip): the 4C-wide hidden activation leaves the CU only in training,
            # as GELU(h) for fc2's weight gradient (the backward recomputes h inside the dh GEMM, as below)
            # (r.mlp_bwd: the backward recomputes GELU(h) as well - no buffer, the inference form of the launch)
            ha = plan.buf(tag + ".ha", (M, 4 * Cc)) if sm and not r.mlp_bwd else None
            ops.mlp_fwd(xn2, w[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], w[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"],
                        xm, xo, ha, M, Cc)
        elif r.mlp in (MLP_LIN_RC, MLP_LIN_SAVED):
            ha = plan.keep(sm, tag + ".ha", "ha", (M, 4 * Cc))
            if r.mlp == MLP_LIN_RC:
                # only GELU(h) is written; backward recomputes h inside the dh GEMM
                ops.gemm_nt([SegSpec(xn2)], w[pre + "mlp.fc1.weight"], ha, M, 4 * Cc, Cc, bias=p[pre + "mlp.fc1.bias"], gelu_only=True)
            else:
                hp = plan.keep(sm, tag + ".hp", "hp", (M, 4 * Cc))
                ops.gemm_nt([SegSpec(xn2)], w[pre + "mlp.fc1.weight"], hp, M, 4 * Cc, Cc, bias=p[pre + "mlp.fc1.bias"], gelu_out=ha)
            ops.gemm_nt([SegSpec(ha)], w[pre + "mlp.fc2.weight"], xo, M, Cc, 4 * Cc, bias=p[pre + "mlp.fc2.bias"], resid=xm)
        else:
            if r.mlp == MLP_FOLD:
                # fc1 folded into the 2x2 convolution (csrc/convmlp.hip): composed weights, the convolution straight on xn2, a
                # correction on the last column / row (where the padded fc1 output is zero including its bias)
                cm = P["cmlp"][pre]
                ops.convmlp_compose(p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], p[pre + "mlp.conv1.weight"], p[pre + "mlp.conv1.bias"],
                                    cm["weff"], cm["weffT"], cm["beff"], cm["vtap"], Cc)
                src, wc, bc = xn2, cm["weff"], cm["beff"]
            else:
                src = plan.keep(sm, tag + ".u", "u", (M, Cc))
                ops.gemm_nt([SegSpec(xn2)], w[pre + "mlp.fc1.weight"], src, M, Cc, Cc, bias=p[pre + "mlp.fc1.bias"])
                wc, bc = w[pre + "mlp.conv1.weight"], p[pre + "mlp.conv1.bias"]
            cp = plan.keep(sm, tag + ".cp", "cp", (M, Cc))
            ca = plan.keep(sm, tag + ".ca", "ca", (M, Cc))
            segs = [SegSpec(src, Cc, 0, dy, dx, 1, 0, H, W) for (dy, dx) in TAPS2]
            ops.gemm_nt(segs, wc, cp, M, Cc, 4 * Cc, spatial=(H, W), bias=bc, gelu_out=ca)
            if r.mlp == MLP_FOLD:
                ops.convmlp_border_fix(cp, ca, cm["vtap"], B, H, W, Cc)
            ops.gemm_nt([SegSpec(ca)], w[pre + "mlp.fc2.weight"], xo, M, Cc, Cc, bias=p[pre + "mlp.fc2.bias"], resid=xm)
        return xo

    def _linear_bwd(self, P, name, dY, X, dX, M, N, K, *, bias=True, sq=False, wide=False, dgelu_aux=None, ldy=None, y_off=0,
                    resid=None, plan=None, need_dx=True):
        """Backward of one nn.Linear / 1x1 convolution `name` ([N][K] weight): dW (and dbias) += dY^T X by sodt_gemm_tn, then
        dX = dY W [* gelu'(dgelu_aux)] [+ resid] by sodt_gemm_nt; dY may be N columns at y_off of a wider buffer.  sq: try the
        square one-launch form first (csrc/linbwd.hip: both from one read of dY; ops.linear_bwd_sq returns False where the entry
        point refuses the layer, and the two launches run instead).  wide: the same for the 192 -> 576 layer (ops.linear_bwd_wide).  plan: its frozen parameters take no weight-gradient launch (a
        frozen weight AND bias leave the plain sodt_gemm_nt); need_dx False: nobody reads dX, only the parameter gradients run."""
        gw, gb, wT = self.g[name + ".weight"], self.g[name + ".bias"] if bias else None, P["wT"][name + ".weight"]
        wg = plan is None or plan.trainable(name + ".weight", *([name + ".bias"] if bias else []))
        if sq and wg and need_dx and ops.linear_bwd_sq(dY, X, wT, dX, gw, M, dbias=gb, dgelu_aux=dgelu_aux):
            return
        if wide and wg and need_dx and ops.linear_bwd_wide(dY, X, wT, dX, gw, M, dbias=gb):
            return
        if wg:
            ops.gemm_tn(dY, [SegSpec(X)], gw, M, N, K, dbias=gb, ldy=ldy, y_off=y_off)
        if need_dx:
            ops.gemm_nt([SegSpec(dY, N, y_off)], wT, dX, M, K, N, dgelu_aux=dgelu_aux, resid=resid)

    def _block_bwd(self, plan, P, tag, blk, dY, dX):
        """dY: gradient wrt the block output; writes the gradient wrt the block input into dX (where the input needs one)."""
        ops.set_tag(tag + ".bwd")
        r = plan.saved[tag]
        if not plan.unit(tag + ".mlp").runs_bwd:
            return
        dxm, dxn = self._mlp_bwd(plan, P, tag, r, dY)
        if plan.unit(tag + ".attn").runs_bwd:
            self._attn_bwd(plan, P, tag, r, dxm, dxn, dX)

    def _mlp_bwd(self, plan, P, tag, r: BlockRoute, dY):
        """MLP and LayerNorm-2 backward; returns (dxm: gradient wrt xm, dxn: scratch the attention backward goes on with).  Frozen
        parameters: a stand-alone weight-gradient launch whose every output is frozen is not issued; where the attention half has no
        backward (nothing trainable at or below it) the chain stops at the lowest trainable parameter of this half."""
        p, wT, g, b = self.params, P["wT"], self.g, plan.bufs
        pre = E + tag + "."
        B, H, W, Cc, _, _ = r.geo
        M = B * H * W
        xm, xn2 = b[tag + ".xm"], b[tag + ".xn2"]
        dxn = plan.scratch("dxn", (M, Cc))
        dxm = plan.scratch("dxm", (M, Cc))
        sq = self.use_fused_linbwd and r.sq_ok          # a backward-only switch: read live
        T = plan.trainable
        ln2 = plan.unit(tag + ".attn").runs_bwd or T(pre + "norm2.weight", pre + "norm2.bias")     # d(xn2) and the LayerNorm-2 backward
        fc1 = T(pre + "mlp.fc1.weight", pre + "mlp.fc1.bias")
        if r.mlp in (MLP_FUSED, MLP_LIN_RC, MLP_LIN_SAVED):
            dh = plan.scratch("dh", (M, 4 * Cc))
            fused = r.mlp_bwd and ops.mlp_bwd(xn2, dY, P["w"][pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], wT[pre + "mlp.fc2.weight"], dh,
                                              g[pre + "mlp.fc1.weight"], g[pre + "mlp.fc1.bias"], g[pre + "mlp.fc2.weight"],
                                              g[pre + "mlp.fc2.bias"], M)
            if r.mlp_bwd and not fused:
                raise RuntimeError(f"{tag}: sodt_mlp_bwd refused the block its route was recorded for (the forward kept no GELU(h))")
            ha = None if fused else b[tag + ".ha"]
            if fused:         # dh, dW1 / db1, dW2 / db2 are done: only dxn = dh fc1.weight is left
                if ln2:
                    ops.gemm_nt([SegSpec(dh, 4 * Cc, 0)], wT[pre + "mlp.fc1.weight"], dxn, M, Cc, 4 * Cc)
            elif r.mlp == MLP_LIN_SAVED:
                self._linear_bwd(P, pre + "mlp.fc2", dY, ha, dh, M, Cc, 4 * Cc, dgelu_aux=b[tag + ".hp"], plan=plan, need_dx=ln2 or fc1)
            else:       # dh = (dY fc2.weight) * gelu'(xn2 fc1.weight^T + b1): pre-activation recomputed in the first K half
                if T(pre + "mlp.fc2.weight", pre + "mlp.fc2.bias"):
                    ops.gemm_tn(dY, [SegSpec(ha)], g[pre + "mlp.fc2.weight"], M, Cc, 4 * Cc, dbias=g[pre + "mlp.fc2.bias"])
                if ln2 or fc1:
                    ops.gemm_nt([SegSpec(xn2), SegSpec(dY)], P["wcat"][pre + "mlp.fc1.weight"], dh, M, 4 * Cc, 2 * Cc,
                                bias=p[pre + "mlp.fc1.bias"], dgelu_rc=True)
            if not fused:
                self._linear_bwd(P, pre + "mlp.fc1", dh, xn2, dxn, M, 4 * Cc, Cc, plan=plan, need_dx=ln2)
        else:
            cp, ca = b[tag + ".cp"], b[tag + ".ca"]
            dc = plan.scratch("dc", (M, Cc))
            conv1 = T(pre + "mlp.conv1.weight", pre + "mlp.conv1.bias")
            self._linear_bwd(P, pre + "mlp.fc2", dY, ca, dc, M, Cc, Cc, sq=sq, dgelu_aux=cp, plan=plan, need_dx=ln2 or fc1 or conv1)
            bsegs = [SegSpec(dc, Cc, 0, -dy, -dx, 1, 0, H, W) for (dy, dx) in TAPS2]
            if r.mlp == MLP_FOLD:
                # d(Weff) = dc^T xn2(taps) (+ the column sums of dc), then the parameter gradients of fc1 / conv1 by the chain rule;
                # d(xn2) comes from ONE tap GEMM with the composed weights (no du, no du W1)
                cm = P["cmlp"][pre]
                if fc1 or conv1:
                    scr = plan.scratch("cmlp", (Cc * 4 * Cc + 4 * Cc,), torch.float32)
                    dweff, colsum, bs = scr[: Cc * 4 * Cc].view(Cc, 4 * Cc), scr[Cc * 4 * Cc: Cc * 4 * Cc + Cc], scr[Cc * 4 * Cc + Cc:].view(3, Cc)
                    ops.zero_(scr)
                    segs = [SegSpec(xn2, Cc, 0, dy, dx, 1, 0, H, W) for (dy, dx) in TAPS2]
                    ops.gemm_tn(dc, segs, dweff, M, Cc, 4 * Cc, spatial=(H, W), dbias=colsum)
                    ops.convmlp_border_sums(dc, bs, B, H, W, Cc)
                    ops.convmlp_decompose(dweff, colsum, bs, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], p[pre + "mlp.conv1.weight"],
                                          g[pre + "mlp.conv1.weight"], g[pre + "mlp.conv1.bias"], g[pre + "mlp.fc1.weight"], g[pre + "mlp.fc1.bias"], Cc)
                if ln2:
                    ops.gemm_nt(bsegs, cm["weffT"], dxn, M, Cc, 4 * Cc, spatial=(H, W))
            else:
                du = plan.scratch("du", (M, Cc))
                segs = [SegSpec(b[tag + ".u"], Cc, 0, dy, dx, 1, 0, H, W) for (dy, dx) in TAPS2]
                if conv1:
                    ops.gemm_tn(dc, segs, g[pre + "mlp.conv1.weight"], M, Cc, 4 * Cc, spatial=(H, W), dbias=g[pre + "mlp.conv1.bias"],
                                kperm=(Cc, 4))
                if ln2 or fc1:
                    ops.gemm_nt(bsegs, wT[pre + "mlp.conv1.weight"], du, M, Cc, 4 * Cc, spatial=(H, W))
                self._linear_bwd(P, pre + "mlp.fc1", du, xn2, dxn, M, Cc, Cc, plan=plan, need_dx=ln2)
        # dxn = d(xn2); the LayerNorm-2 backward adds the residual path's dY.  (Rounds 4-5 carried a GEMM with the LayerNorm backward
        # as its epilogue for the 192-column case: slower than these two launches, removed in round 6 - profiles/r04_lnfold_ab.md,
        # DESIGN.md section 5.)
        if ln2:
            ops.layernorm_bwd(dxn, xm, b[tag + ".st2"], p[pre + "norm2.weight"], dY, dxm, g[pre + "norm2.weight"], g[pre + "norm2.bias"], M, Cc)
        return dxm, dxn

    def _attn_bwd(self, plan, P, tag, r: BlockRoute, dxm, dxn, dX):
        """Attention and LayerNorm-1 backward: dX = d(x_in) from dxm = d(xm); dxn is scratch (the projection's input gradient, then
        d(xn1)).  The padded arm is the backward of an UNSHIFTED block whose resolution is not a multiple of its window (see
        _block_route): the projection's input gradient lands on the padded grid (zeros outside: the crop's adjoint), the attention
        backward runs on it, qkv.weight sees zero rows for the pad tokens while qkv.bias collects their gradient (their q / k / v
        ARE the bias), and the input gradient is read back cropped.  Frozen parameters as in _mlp_bwd: where the block's input needs
        no gradient the chain stops at the lowest trainable parameter."""
        p, wT, g, b = self.params, P["wT"], self.g, plan.bufs
        pre = E + tag + "."
        B, H, W, Cc, ws, shift = r.geo
        M = B * H * W
        xn1 = b[tag + ".xn1"]
        bias_t = P["bias_t"][pre + "attn.relative_position_bias_table"]
        L2 = 2 * ws - 1
        T = plan.trainable
        ln1 = plan.unit(tag + ".attn").any_dx or T(pre + "norm1.weight", pre + "norm1.bias")       # d(xn1) and the LayerNorm-1 backward
        qkvg = T(pre + "attn.qkv.weight", pre + "attn.qkv.bias")
        attn = ln1 or qkvg or T(pre + "attn.relative_position_bias_table")                        # the attention backward itself
        if r.attn == ATTN_PADDED:
            Hp, Wp = r.pad
            Mp = B * Hp * Wp
            aop = b[tag + ".aop"]
            if T(pre + "attn.proj.weight", pre + "attn.proj.bias"):
                ops.gemm_tn(dxm, [SegSpec(aop, Cc, 0, 0, 0, 1, 0, Hp, Wp)], g[pre + "attn.proj.weight"], M, Cc, Cc, spatial=(H, W),
                            dbias=g[pre + "attn.proj.bias"])
            if attn:
                daop = plan.scratch("daop", (Mp, Cc))
                ops.gemm_nt([SegSpec(dxm, Cc, 0, 0, 0, 1, 0, H, W)], wT[pre + "attn.proj.weight"], daop, Mp, Cc, Cc, spatial=(Hp, Wp))
                dqkv = plan.scratch("dqkvp", (Mp, 3 * Cc))
                dbt = plan.scratch("dbt", (HEADS, L2 * L2), torch.float32, zero=True)
                scratch = plan.scratch("attn_scratchp", (Mp * (Cc + HEADS),), torch.float32, zero=True) if r.zscratch else None
                ops.window_attn_bwd(b[tag + ".qkv"], bias_t, aop, daop, b[tag + ".lse"], dqkv, dbt, scratch, B, Hp, Wp, Cc, HEADS, ws, 0)
                # (always: the transposition also clears dbt, which the next block's attention backward adds into)
                ops.transpose_f32(dbt, g[pre + "attn.relative_position_bias_table"], HEADS, L2 * L2, accumulate=2)
                if qkvg:
                    ops.gemm_tn(dqkv, [SegSpec(xn1, Cc, 0, 0, 0, 1, 0, H, W)], g[pre + "attn.qkv.weight"], Mp, 3 * Cc, Cc,
                                spatial=(Hp, Wp), dbias=g[pre + "attn.qkv.bias"])
                if ln1:
                    ops.gemm_nt([SegSpec(dqkv, 3 * Cc, 0, 0, 0, 1, 0, Hp, Wp)], wT[pre + "attn.qkv.weight"], dxn, M, Cc, 3 * Cc, spatial=(H, W))
        else:
            ao, dao = b[tag + ".ao"], dxn
            self._linear_bwd(P, pre + "attn.proj", dxm, ao, dao, M, Cc, Cc, sq=self.use_fused_linbwd and r.sq_ok, plan=plan, need_dx=attn)
            if attn:
                dqkv = plan.scratch("dqkv", (M, 3 * Cc))
                dbt = plan.scratch("dbt", (HEADS, L2 * L2), torch.float32, zero=True)
                if r.attn == ATTN_FUSED_RC:
                    ops.wmsa_block_bwd(xn1, r.wpk, bias_t, dao, b[tag + ".lsew"], dqkv, dbt, B, H, W, Cc, HEADS, ws, shift)
                elif r.attn == ATTN_FUSED_SAVED:
                    ops.window_attn_bwd_wm(b[tag + ".qkvw"], bias_t, dao, b[tag + ".lsew"], dqkv, dbt, B, H, W, Cc, HEADS, ws, shift)
                elif r.attn == ATTN_SHIFT_PAD:
                    # the pad keys' k / v gradient belongs to qkv.bias (their k / v ARE the bias): added there by the kernel, beside the
                    # column sums of dqkv the linear backward below adds
                    ops.window_attn_sp_bwd(b[tag + ".qkv"], p[pre + "attn.qkv.bias"], bias_t, ao, dao, b[tag + ".lse"], dqkv,
                                           g[pre + "attn.qkv.bias"], dbt, B, H, W, Cc, HEADS, ws, shift)
                else:
                    scratch = plan.scratch("attn_scratch", (M * (Cc + HEADS),), torch.float32, zero=True) if r.zscratch else None
                    ops.window_attn_bwd(b[tag + ".qkv"], bias_t, ao, dao, b[tag + ".lse"], dqkv, dbt, scratch, B, H, W, Cc, HEADS, ws, shift)
                # (always: the transposition also clears dbt, which the next block's attention backward adds into)
                ops.transpose_f32(dbt, g[pre + "attn.relative_position_bias_table"], HEADS, L2 * L2, accumulate=2)
                self._linear_bwd(P, pre + "attn.qkv", dqkv, xn1, dxn, M, 3 * Cc, Cc, wide=self.use_wide_linbwd and r.wide_ok, plan=plan,
                                 need_dx=ln1)
        if ln1:
            ops.layernorm_bwd(dxn, r.x_in, b[tag + ".st1"], p[pre + "norm1.weight"], dxm, dX, g[pre + "norm1.weight"], g[pre + "norm1.bias"], M, Cc)

    # ------------------------------------------------------------------ PatchMerging
    def _merge_fwd(self, plan, P, tag, x, B, H, W, Cc):
        ops.set_tag(tag)
        p, w = self.params, P["w"]
        pre = E + tag + "."
        M2 = B * (H // 2) * (W // 2)
        sv = plan.saves(tag)
        z = plan.keep(sv, tag + ".z", "z", (M2, 2 * Cc))
        segs = [SegSpec(x, Cc, 0, dy, dx, 2, 0, H, W) for (dy, dx) in MERGE]
        ops.gemm_nt(segs, w[pre + "reduction.weight"], z, M2, 2 * Cc, 4 * Cc, spatial=(H // 2, W // 2))
        y = plan.buf(tag + ".y", (M2, 2 * Cc))
        st = plan.keep(sv, tag + ".st", "st", (M2, 2), torch.float32)
        ops.layernorm_fwd(z, p[pre + "norm.weight"], p[pre + "norm.bias"], y, st, M2, 2 * Cc)
        plan.saved[tag] = dict(x=x, geo=(B, H, W, Cc))
        return y

    def _merge_bwd(self, plan, P, tag, dY, dX):
        p, wT, g, b = self.params, P["wT"], self.g, plan.bufs
        pre = E + tag + "."
        sv = plan.saved[tag]
        B, H, W, Cc = sv["geo"]
        M2 = B * (H // 2) * (W // 2)
        dz = plan.buf(tag + ".dz", (M2, 2 * Cc))
        ops.layernorm_bwd(dY, b[tag + ".z"], b[tag + ".st"], p[pre + "norm.weight"], None, dz, g[pre + "norm.weight"],
                          g[pre + "norm.bias"], M2, 2 * Cc)
        segs = [SegSpec(sv["x"], Cc, 0, dy, dx, 2, 0, H, W) for (dy, dx) in MERGE]
        if plan.trainable(pre + "reduction.weight"):
            ops.gemm_tn(dz, segs, g[pre + "reduction.weight"], M2, 2 * Cc, 4 * Cc, spatial=(H // 2, W // 2))
        if not plan.unit(tag).any_dx:
            return
        for tap, (dy, dx) in enumerate(MERGE):   # the four taps tile the input grid exactly once
            ops.gemm_nt([SegSpec(dz, 2 * Cc, 0, 0, 0, 1, 0, H // 2, W // 2)], wT[pre + "reduction.weight"], dX, M2, Cc, 2 * Cc,
                        spatial=(H // 2, W // 2), w_off=tap * Cc * 2 * Cc, oscatter=(2, dy, dx, H, W))

    # ------------------------------------------------------------------ head units
    def _conv_fwd(self, plan, P, tag, pname, segs, spatial, M, K, Cout, k, out=None):
        """Conv2d(bias=False)+BN+SiLU (common.py:38-50) as GEMM (+f64 column stats) -> finalize -> normalise+SiLU.
        out: write the result into the first Cout columns of this wider [M][ld] buffer (a concat slice) instead of tag.y."""
        ops.set_tag(tag)
        p, w, bufs = self.params, P["w"], self.buffers
        y = plan.buf(tag + ".y", (M, Cout)) if out is None else out
        ldy = y.shape[-1]
        wname = pname + "conv.weight"
        sv = plan.saves(tag.split(".")[0])        # (tag: the head unit "h3", or one of its convolutions "h3.cv1")
        direct = bool(sv and not self.fused and self._direct3(plan, segs, K, Cout, k))
        if self.fused:
            ones = P["ones"].setdefault(Cout, torch.ones(Cout, device=self.dev))
            ops.gemm_nt(segs, w[wname], y, M, Cout, K, spatial=spatial, affine=(ones, p[pname + "conv.bias"]), ldc=ldy)
        elif plan.training:
            # (a unit that saves nothing still normalises with the batch statistics and moves the running ones: model.train())
            z = plan.keep(sv, tag + ".z", "z", (M, Cout))
            stats = plan.zbuf("f", tag + ".stats", (L.STATS_REPL, 2, Cout), torch.float64)   # zeroed with the pool (_forward_main)
            mr = plan.keep(sv, tag + ".mr", "mr", (2, Cout), torch.float32)
            if direct:
                # the 3x3 at 64 -> 64 channels of the stride-4 C3's Bottleneck: the direct kernel reads its input once (csrc/conv3.hip;
                # the nine-segment GEMM ran at 0.11-0.15 of its HBM roofline), the batch statistics come from the stored output
                H, W = spatial
                ops.conv3_c64_fwd(segs[4].t, w[wname], z, M // (H * W), H, W)
                ops.col_stats(z, stats, M, Cout)
            else:
                ops.gemm_nt(segs, w[wname], z, M, Cout, K, spatial=spatial, stats=stats)
            bn = self.model.get_submodule(pname + "bn")
            mom = self._bn_momentum(bn, pname + "bn")      # (common.py's 0.03 unless somebody moved it: bypass_bn)
            at = ops.recorded_count()
            if at is not None:
                plan.bn_marks.append([at, bn, pname + "bn", mom])
            count = M
            if self._sbn_on:
                # the statistics of every rank's rows: the sums are all-reduced between the launch that formed them and
                # sodt_bn_finalize, which divides by the total count (unbiased running variance included).  Issued here while
                # recording; a replay stops at this index for it (_forward).  A frozen unit's statistics are shared too.
                if at is not None:
                    plan.sbn_fwd.append((at, stats))
                self._sbn_fwd_collective(stats)
                count = M * self.ddp.world
            ops.bn_finalize(stats, mr, bufs[pname + "bn.running_mean"], bufs[pname + "bn.running_var"], count, Cout, 1e-3, mom)
            ops.bn_silu_fwd(z, mr, p[pname + "bn.weight"], p[pname + "bn.bias"], y, ldy, M, Cout)
        else:
            mr = plan.buf(tag + ".mr", (2, Cout), torch.float32)
            sc = plan.buf(tag + ".sc", (2, Cout), torch.float32)
            ops.bn_finalize(None, mr, bufs[pname + "bn.running_mean"], bufs[pname + "bn.running_var"], M, Cout, 1e-3, 0.03)
            ops.bn_affine(mr, p[pname + "bn.weight"], p[pname + "bn.bias"], sc[0], sc[1], Cout)
            ops.gemm_nt(segs, w[wname], y, M, Cout, K, spatial=spatial, affine=(sc[0], sc[1]), ldc=ldy)
        plan.saved[tag] = ConvRoute(segs, spatial, M, K, Cout, k, pname, direct)
        return y

    def _direct3(self, plan, segs, K, Cout, k):
        """a 3x3 Conv at 64 -> 64 channels on one dense bf16 tensor: sodt_conv3x3_c64_* (forward, input gradient, weight gradient)"""
        if not (self.use_direct_conv3 and k == 3 and Cout == 64 and K == 576 and plan.dt == torch.bfloat16 and len(segs) == 9):
            return False
        s0 = segs[4]
        return (s0.klen == 64 and s0.ld == 64 and s0.coff == 0 and s0.shr == 0 and s0.mul == 1 and s0.dy == 0 and s0.dx == 0
                and all(s_.t is s0.t for s_ in segs))

    def _conv_bwd(self, plan, tag, dy, lddy, dy_off, dz_out=None):
        """BN+SiLU backward and the conv weight gradient; returns dz (gradient at the conv output).  dz_out = (buffer, ld, column
        offset): dz is written as that column slice of a wider buffer (1x1 convolutions) and the buffer is returned."""
        ops.set_tag(tag + ".bwd")
        p, g, b = self.params, self.g, plan.bufs
        sv = plan.saved[tag]
        M, K, Cout, k, pname = sv.M, sv.K, sv.Cout, sv.k, sv.pname
        red = plan.zbuf("b", tag + ".red", (2, Cout), torch.float64)                          # zeroed with the pool (_backward_main)
        dz, lddz, dz_off = dz_out if dz_out is not None else (plan.buf(tag + ".dz", (M, Cout)), Cout, 0)
        ops.bn_silu_bwd_reduce(dy, lddy, b[tag + ".z"], b[tag + ".mr"], p[pname + "bn.weight"], p[pname + "bn.bias"], red, M, Cout,
                               dy_off=dy_off)
        if self._sbn_on:
            # the two means of dz run over every rank's rows: a copy of the sums is all-reduced (here while recording; a replay
            # stops at this index for it, _backward), dgamma / dbeta keep this rank's own sums for the gradient all-reduce
            red_all = plan.zbuf("b", tag + ".red_all", (2, Cout), torch.float64)
            at = ops.recorded_count()
            if at is not None:
                plan.sbn_bwd.append((at, red, red_all))
            self._sbn_bwd_collective(red, red_all)
            ops.bn_silu_bwd_apply_sync(dy, lddy, b[tag + ".z"], b[tag + ".mr"], p[pname + "bn.weight"], p[pname + "bn.bias"], red,
                                       red_all, M * self.ddp.world, dz, g[pname + "bn.weight"], g[pname + "bn.bias"], M, Cout,
                                       dy_off=dy_off, lddz=lddz, dz_off=dz_off)
        else:
            ops.bn_silu_bwd_apply(dy, lddy, b[tag + ".z"], b[tag + ".mr"], p[pname + "bn.weight"], p[pname + "bn.bias"], red, dz,
                                  g[pname + "bn.weight"], g[pname + "bn.bias"], M, Cout, dy_off=dy_off, lddz=lddz, dz_off=dz_off)
        cin = K // (k * k)
        if not plan.trainable(pname + "conv.weight"):
            pass
        elif sv.direct:
            assert dz_out is None
            H, W = sv.spatial
            scr = plan.buf("g.c64.scratch", (ops.conv3_c64_wgrad_scratch_floats(),), torch.float32)
            ops.conv3_c64_wgrad(dz, sv.segs[4].t, g[pname + "conv.weight"], None, scr, M // (H * W), H, W)
        else:
            ops.gemm_tn(dz, sv.segs, g[pname + "conv.weight"], M, Cout, K, spatial=sv.spatial,
                        kperm=(cin, k * k) if k > 1 else None, ldy=lddz, y_off=dz_off)
        return dz

    def _c3_fwd(self, plan, P, tag, pname, segs, spatial, M, c1, c2):
        c_ = c2 // 2
        H, W = spatial
        a1 = self._conv_fwd(plan, P, tag + ".cv1", pname + "cv1.", segs, spatial, M, c1, c_, 1)
        a2 = self._conv_fwd(plan, P, tag + ".m1", pname + "m.0.cv1.", [SegSpec(a1)], None, M, c_, c_, 1)
        s3 = [SegSpec(a2, c_, 0, dy, dx, 1, 0, H, W) for (dy, dx) in TAPS3]
        a3 = self._conv_fwd(plan, P, tag + ".m2", pname + "m.0.cv2.", s3, spatial, M, 9 * c_, c_, 3)
        b1 = self._conv_fwd(plan, P, tag + ".cv2", pname + "cv2.", segs, spatial, M, c1, c_, 1)
        out = self._conv_fwd(plan, P, tag + ".cv3", pname + "cv3.", [SegSpec(a3), SegSpec(b1)], None, M, 2 * c_, c2, 1)
        plan.saved[tag] = dict(M=M, c1=c1, c2=c2, spatial=spatial, pname=pname)
        return out

    def _c3_bwd(self, plan, P, tag, dout, ldd, d_off):
        """returns d(concatenated input) [M][c1], or None where no input of the unit needs a gradient."""
        wT = P["wT"]
        dx = plan.unit(tag).any_dx
        sv = plan.saved[tag]
        M, c1, c2, (H, W), pname = sv["M"], sv["c1"], sv["c2"], sv["spatial"], sv["pname"]
        c_ = c2 // 2
        dz3 = self._conv_bwd(plan, tag + ".cv3", dout, ldd, d_off)
        dcat = plan.buf(tag + ".dcat", (M, 2 * c_))
        ops.gemm_nt([SegSpec(dz3)], wT[pname + "cv3.conv.weight"], dcat, M, 2 * c_, c2)
        din = plan.buf(tag + ".din", (M, c1)) if dx else None
        # cv1 and cv2 read the same input: with their dz as the two halves of ONE [M][2 c_] buffer, d(input) = dz1 W1 + dz2 W2 is a
        # single GEMM against [W1^T | W2^T] (one write of din, one rounding) instead of a GEMM and a second one with a residual
        w12 = P["wT12"].get(pname) if dx else None
        dz12 = (plan.buf(tag + ".dz12", (M, 2 * c_)), 2 * c_) if w12 is not None else None
        dzb = self._conv_bwd(plan, tag + ".cv2", dcat, 2 * c_, c_, dz_out=dz12 + (c_,) if dz12 else None)
        if dx and w12 is None:
            ops.gemm_nt([SegSpec(dzb)], wT[pname + "cv2.conv.weight"], din, M, c1, c_)
        dza3 = self._conv_bwd(plan, tag + ".m2", dcat, 2 * c_, 0)
        da = plan.buf(tag + ".da", (M, c_))
        if plan.saved[tag + ".m2"].direct:
            ops.conv3_c64_fwd(dza3, wT[pname + "m.0.cv2.conv.weight"], da, M // (H * W), H, W, flip=True)
        else:
            segs = [SegSpec(dza3, c_, 0, -dy, -dx, 1, 0, H, W) for (dy, dx) in TAPS3]
            ops.gemm_nt(segs, wT[pname + "m.0.cv2.conv.weight"], da, M, c_, 9 * c_, spatial=(H, W))
        dza2 = self._conv_bwd(plan, tag + ".m1", da, c_, 0)
        ops.gemm_nt([SegSpec(dza2)], wT[pname + "m.0.cv1.conv.weight"], da, M, c_, c_)
        dza1 = self._conv_bwd(plan, tag + ".cv1", da, c_, 0, dz_out=dz12 + (0,) if dz12 else None)
        if w12 is not None:
            ops.gemm_nt([SegSpec(dza1)], w12, din, M, c1, 2 * c_)
        elif dx:
            ops.gemm_nt([SegSpec(dza1)], wT[pname + "cv1.conv.weight"], din, M, c1, c_, resid=din)
        return din

    # ------------------------------------------------------------------ SPP (common.py:129-140)
    def _spp_fwd(self, plan, P, tag, pname, segs, spatial, M, c1, c2, B):
        """cv1 (1x1 Conv+BN+SiLU) -> MaxPool 5 / 9 / 13 (stride 1, same padding: ONE 5x5 kernel in cascade, csrc/pool.hip) ->
        Concat -> cv2.  The concat never exists as a copy: cv1 and the pools write their slices of one [M][4 c_] buffer,
        which is cv2's single K-segment."""
        c_ = c1 // 2
        H, W = spatial
        cat = plan.buf(tag + ".cat", (M, 4 * c_))
        self._conv_fwd(plan, P, tag + ".cv1", pname + "cv1.", segs, spatial if any(s_.shr or s_.Hi for s_ in segs) else None, M, c1, c_, 1, out=cat)
        arg = plan.buf(tag + ".arg", (3, M, c_), torch.uint8) if plan.saves(tag) else None
        for i in range(3):                                   # m5, m9 = m5 o m5, m13 = m5 o m5 o m5 into the next slices
            ops.maxpool5_fwd(cat, cat, arg[i] if arg is not None else None, B, H, W, c_, ldx=4 * c_, ldy=4 * c_, x_off=i * c_,
                             y_off=(i + 1) * c_)
        out = self._conv_fwd(plan, P, tag + ".cv2", pname + "cv2.", [SegSpec(cat)], None, M, 4 * c_, c2, 1)
        plan.saved[tag] = dict(M=M, c1=c1, c2=c2, spatial=spatial, pname=pname, B=B)
        return out

    def _spp_bwd(self, plan, P, tag, dout, ldd, d_off):
        """returns d(input) [M][c1], or None where the input needs no gradient."""
        wT, b = P["wT"], plan.bufs
        sv = plan.saved[tag]
        M, c1, c2, (H, W), pname, B = sv["M"], sv["c1"], sv["c2"], sv["spatial"], sv["pname"], sv["B"]
        c_ = c1 // 2
        dz2 = self._conv_bwd(plan, tag + ".cv2", dout, ldd, d_off)
        dcat = plan.buf(tag + ".dcat", (M, 4 * c_))
        ops.gemm_nt([SegSpec(dz2)], wT[pname + "cv2.conv.weight"], dcat, M, 4 * c_, c2)
        for i in (2, 1, 0):                                  # d m13 -> m9 -> m5 -> a1, accumulated into the lower slice
            ops.maxpool5_bwd(dcat, b[tag + ".arg"][i], dcat, B, H, W, c_, lddy=4 * c_, lddx=4 * c_, dy_off=(i + 1) * c_, dx_off=i * c_,
                             accumulate=True)
        dz1 = self._conv_bwd(plan, tag + ".cv1", dcat, 4 * c_, 0)
        if not plan.unit(tag).any_dx:
            return None
        din = plan.buf(tag + ".din", (M, c1))
        ops.gemm_nt([SegSpec(dz1)], wT[pname + "cv1.conv.weight"], din, M, c1, c_)
        return din

    # ================================================================== super-resolution branch (model.py:284-287)
    def _sr_forward(self, plan: Plan):
        """output_sr = model_up(low-level, deep) on the tapped features: live launches (sr.SRBranch; its weights are re-laid out
        from the masters every call).  The taps are K-segment views of the head's buffers - an Upsample / Concat entry is index
        arithmetic here too."""
        from .sr import SRBranch
        B, t = plan.B, plan.H // 4               # (square: run() refuses sr with H != W)
        br = plan.sr
        if br is None:
            names = [n for n in self.params if n.startswith("model_up.")]
            br = plan.sr = SRBranch({n: self.params[n] for n in names}, plan.dt, {n: self.g[n] for n in names},
                                    dec="model_up.sr_decoder.", edsr="model_up.edsr.")
            br._prep_version = (self.params_version(), self._param_epoch)
        else:
            # re-lay the 82 SR tensors out only when a parameter may have changed: in-place writes through the Parameter objects
            # (version counters) or the fused optimizer / invalidate_params() (epoch) - not on every forward of an accumulation step
            ver = (self.params_version(), self._param_epoch)
            if getattr(br, "_prep_version", None) != ver:
                br.prepare()
                br._prep_version = ver
        low, deep = self._sr_segs(plan)
        return br.forward(low, deep, B, t, t)

    def _sr_segs(self, plan: Plan):
        """The branch's two inputs (low-level on the stride-4 grid, deep on the stride-8 grid) as K-segment views of the tapped
        features' buffers."""
        t = plan.H // 4
        def segs(parts, level):
            h = t >> level
            return [SegSpec(self._ref_buf(plan, ref), c, 0, 0, 0, 1, shr, h >> shr, h >> shr) for ref, c, shr in parts]
        return segs(self.head.sr_parts[0], 0), segs(self.head.sr_parts[1], 1)

    def _sr_backward(self, plan: Plan, dsr):
        """SR gradients: parameters into the flat buffer, inputs into plan.sr's dense buffers (zero when the SR output took no part
        in the loss); the recorded head backward adds them to the tapped features' gradients (_backward_main: sr_extra)."""
        br = plan.sr
        u = plan.unit("model_up")
        if not u.runs_bwd:
            return
        if dsr is None:
            for k in ("g.low", "g.x"):
                if k in br.bufs:
                    ops.zero_(br.bufs[k])
            return
        # the branch's frozen convolutions take no weight-gradient launch; taps that need no gradient take no input gradient
        br.trainable, br.need_dx = plan.trainable, u.any_dx
        br.backward(dsr)

    def _sr_extra(self, plan: Plan):
        """ref -> [(dense gradient buffer, ld, column offset, channels, shr)]: what the SR branch adds to d(feature)."""
        B, t = plan.B, plan.H // 4
        br = plan.sr
        low, deep = self.head.sr_parts
        c1 = sum(p.channels for p in low)
        c2 = sum(p.channels for p in deep)
        d_low = br._buf("g.low", (B * t * t, c1))
        d_x = br._buf("g.x", (B * (t // 2) ** 2, c2))
        extra: Dict[tuple, list] = {}
        for parts, buf, level in ((low, d_low, 0), (deep, d_x, 1)):
            coff = 0
            for ref, c, shr in parts:
                extra.setdefault(ref, []).append((buf, buf.shape[1], coff, c, shr, t >> level))
                coff += c
        return extra

    def _add_extra(self, plan: Plan, extra, ref, target):
        """target (buffer, ld, column offset) += the SR branch's gradient for feature `ref` (summed over the 2^shr x 2^shr children
        where the tap was an upsampled view)."""
        B = plan.B
        dst, ld, off = target
        for i, (buf, lds, coff, c, shr, H) in enumerate(extra.get(ref, ())):
            if shr == 0:
                ops.add_rows(dst, buf, B * H * H, c, ldd=ld, dcol=off, lds=lds, scol=coff)
            else:
                Hs = H >> shr
                tmp = plan.buf(f"sr.dup.{ref.kind}{ref.index}.{i}", (B * Hs * Hs, c))
                ops.gather_sum_rows(buf, lds, tmp, c, B, Hs, Hs, shr, c, d_off=coff)
                ops.add_rows(dst, tmp, B * Hs * Hs, c, ldd=ld, dcol=off)

    # ================================================================== backward
    def _backward(self, plan: Plan, x_rgb, x_ir, dpred, dsr=None):
        if self.fused or not plan.training:
            raise RuntimeError("backward needs a training-mode, un-fused model")
        P = self._prep_for(plan.dt)
        B, th, tw = plan.B, plan.H // 4, plan.W // 4
        T1 = B * th * tw
        fz = plan.fz
        fresh = self._claim_grads(None if fz is None else fz.frozen)
        if fresh:
            ops.zero_(self.flat_grad)
        if fz is not None and not fz.any_bwd:
            return                                   # everything frozen: no gradient to compute, nothing to reduce
        first = 0 if fz is None else fz.first_trainable_offset      # the frozen head of the buffer is zero on every rank
        if self.ddp is not None:
            self.ddp.begin_backward(self.flat_grad, fresh)
        # (1) Detect backward: live (dpred pointer changes)
        ud = plan.unit("detect")
        if ud.runs_bwd:
            cd = self.head.head_out[1]
            if plan.bwd_main is None:                    # decided once per plan: the recorded list holds Detect's GEMMs or it does not
                plan.det_fused = bool(self.use_fused_detect and ops.detect_fused_ok(cd, self.na, self.no, plan.dt))
            if plan.det_fused:
                # dX, dW and dbias from one read of dpred (csrc/detect.hip); g.dzd, the [T1][48] copy of dpred, does not exist here
                dyd = plan.buf("g.dyd", (T1, cd)) if ud.any_dx else None
                if dpred is None:                        # SR-only loss: a zero gradient, nothing for the parameters
                    if dyd is not None:
                        ops.zero_(dyd)
                elif ud.any_wgrad or dyd is not None:
                    wg, wn, bn = ud.any_wgrad, self.det_name + "m.0.weight", self.det_name + "m.0.bias"
                    hx = plan.bufs[self.head.by_row[self.head.head_out[0]].out_name]
                    if not ops.detect_bwd(dpred, hx, P["w"][wn], dyd, self.g[wn] if wg else None, self.g[bn] if wg else None,
                                          B, th * tw, self.na, self.no, cd, lddw=cd):
                        # refused (a dpred off its alignment): the three launches it replaces, live and with the same outputs
                        dzd = plan.buf("g.dzd", (T1, self.det_np))
                        ops.detect_unpermute(dpred, dzd, self.det_np, B, th * tw, self.na, self.no)
                        if wg:
                            ops.gemm_tn(dzd, [SegSpec(hx)], self.g[wn], T1, self.na * self.no, cd, ldy=self.det_np, lddw=cd, dbias=self.g[bn])
                        if dyd is not None:
                            ops.gemm_nt([SegSpec(dzd)], P["wT"][wn], dyd, T1, cd, self.det_np)
            else:
                dzd = plan.buf("g.dzd", (T1, self.det_np))
                if dpred is None:                            # SR-only loss
                    ops.zero_(dzd)
                else:
                    ops.detect_unpermute(dpred, dzd, self.det_np, B, th * tw, self.na, self.no)
        if self.sr:
            self._sr_backward(plan, dsr)             # live too: its input gradients land in plan.sr's buffers
        overlap = False
        if plan.bwd_main is None:
            with ops.Recorder() as rec:
                self._backward_main(plan, P)
            plan.bwd_main = rec.calls
        elif self.ddp is not None and self.ddp.world > 1 and ((self.ddp.sync and plan.bwd_marks) or plan.sbn_bwd):
            # replay in segments: at every mark one more bucket of the flat buffer is final and its all-reduce starts; with
            # synchronised BatchNorm the list also stops in front of every sodt_bn_silu_bwd_apply_sync for the sums of the other
            # ranks (no_sync() holds back the buckets, never those).  Both lists are in index order; merged, the buckets start
            # where they always did.
            overlap = bool(self.ddp.sync and plan.bwd_marks)
            stops = [(idx, 1, (lo, hi)) for idx, lo, hi in plan.bwd_marks] if overlap else []
            stops += [(idx, 0, (red, red_all)) for idx, red, red_all in plan.sbn_bwd]
            pos = 0
            for idx, bucket, what in sorted(stops, key=lambda s_: s_[:2]):
                ops.replay(plan.bwd_main, probes=self.probes_bwd, start=pos, end=idx)
                if bucket:
                    self.ddp.reduce_async(self.flat_grad[what[0]:what[1]])
                else:
                    self._sbn_bwd_collective(*what)
                pos = idx
            ops.replay(plan.bwd_main, probes=self.probes_bwd, start=pos)
        else:
            self._replay(plan, "bwd_main", plan.bwd_main, self.probes_bwd)
        if plan.unit("frontend").runs_bwd:
            self._frontend_bwd(plan, P, x_rgb, x_ir)
            if fz is not None:
                for lo, hi in fz.dirty_runs(0, self.fe_end):             # its frozen parameters: the one launch wrote all sixteen
                    ops.zero_(self.flat_grad[lo:hi])
        if self.ddp is not None:
            if overlap:
                self.ddp.finish(self.flat_grad[min(first, plan.bwd_marks[-1][1]): plan.bwd_marks[-1][1]])
            else:
                self.ddp.reduce(self.flat_grad[first:])

    def replay_encoder_backward(self, plan: Plan, x_rgb, x_ir):
        """Diagnostic / test hook: re-run the ENCODER part of the recorded backward (necks, stages 3..1, PatchMergings, patch
        embed, front end) from whatever the head-input gradient buffers `plan.enc_gin` hold now, accumulating into the flat
        gradient buffer.  The encoder has no cross-image coupling (LayerNorm, windows, per-image shifts), so a batch's encoder
        gradients are the sum of its images' - tests/test_fullsize_gpu.py checks the B = 8 training step that way.  Needs one
        ordinary backward on this plan first (it records the launches) and the activations of the latest forward."""
        if plan.bwd_main is None:
            raise RuntimeError("replay_encoder_backward: run one backward on this plan first")
        if plan.enc_bwd_start is None:
            off = [u.name for u in plan.fz.units.values() if not u.runs_bwd] if plan.fz is not None else []
            raise RuntimeError("replay_encoder_backward: the encoder's backward was not recorded on this plan: frozen parameters "
                               f"(requires_grad False) leave no backward for {', '.join(off[:4])}{' ...' if len(off) > 4 else ''}")
        ops.replay(plan.bwd_main, start=plan.enc_bwd_start)
        self._frontend_bwd(plan, self._prep_for(plan.dt), x_rgb, x_ir)

    def _frontend_bwd(self, plan: Plan, P, x_rgb, x_ir):
        # (3) front end: live
        B, H, W = plan.B, plan.H, plan.W
        fe = P["fe"]
        cb = self.model.image_encoder.chan_block
        ca_ws, ca_shift = int(cb.window_size), int(cb.shift_size)
        irs = x_ir.shape[1] * H * W
        gw, gb, gg, gbe, dx0 = self.g_fe_w, self.g_fe_b, self.g_fe_g, self.g_fe_be, plan.bufs["g.dx0"]
        if ca_ws == 1:
            ws = plan.buf("fe.ws", (ops.frontend_bwd_workspace_bytes(B, H, W) // 4,), torch.float32)
            ops.frontend_bwd(x_rgb, x_ir, irs, fe["w"], fe["b"], fe["g"], fe["be"], dx0, gw, gb, gg, gbe, B, H, W, ws=ws)
        else:
            de = plan.buf("fe.de", (B * (H // 4) * (W // 4), 192), torch.float32)
            ops.zero_(de)
            ops.cross_attn_ln_bwd(plan.bufs["fe.e"], fe["g"], dx0, de, gg, gbe, B, H, W, ca_ws, ca_shift)
            ops.patch_embed4_bwd(x_rgb, x_ir, irs, de, gw, gb, B, H, W)

    def _zero_frozen(self, plan: Plan, lo, hi):
        """Frozen parameters' slices in [lo, hi) of the flat buffer that a launch fusing dX with parameter gradients may have
        written (LayerNorm, BatchNorm, attention backwards; a GEMM whose weight is trainable and whose bias is not): back to zero,
        one memset per contiguous run (freeze.FreezeRecord.dirty_runs).  Nothing frozen: no launch."""
        if plan.fz is not None:
            for a, b_ in plan.fz.dirty_runs(lo, hi):
                ops.zero_(self.flat_grad[a:b_])

    def _mark(self, plan: Plan, lo, hi):
        """the gradients in [lo, hi) are final at this point of the recorded list: a data-parallel bucket (the buffer's frozen head
        is zero on every rank and is left out)"""
        self._zero_frozen(plan, lo, hi)
        lo = max(lo, 0 if plan.fz is None else plan.fz.first_trainable_offset)
        if lo < hi:
            plan.bwd_marks.append((ops.recorded_count(), lo, hi))

    def _head_bwd(self, plan: Plan, P, gout, extra):
        """The head units in reverse, the counterpart of _head_fwd.  gout: headgraph.Ref -> (buffer, ld, column offset) of the
        gradient at the last unit's output; returns it holding d(f0), d(f1), d(f2) under Ref("enc", j)."""
        B, th, tw = plan.B, plan.H // 4, plan.W // 4
        wT, U = P["wT"], plan.unit
        # ---- head units in reverse: every unit returns d(its concatenated input) [M][c1]; the gradient of an Upsample /
        #      Concat input is a column slice of it (nearest x2^shr upsample: summed over the 2^shr x 2^shr children).  A unit
        #      whose output needs no gradient is passed over; an input that needs none gets no slice (and no gather_sum_rows)
        for u in reversed(self.head.units):
            H, W = th >> u.level, tw >> u.level
            M = B * H * W
            tag = f"h{u.k}"
            ur = U(tag)
            if not ur.runs_bwd:
                continue
            dy, ld, off = gout.pop(u.ref)
            self._add_extra(plan, extra, u.ref, (dy, ld, off))
            if u.kind == "Conv":
                dz = self._conv_bwd(plan, tag, dy, ld, off)
                din = None
                if ur.any_dx:
                    din = plan.buf(tag + ".din", (M, u.c1))
                    w_ = wT[f"detect.{u.k}.conv.weight"]
                    if u.ksize == 1:
                        ops.gemm_nt([SegSpec(dz)], w_, din, M, u.c1, u.c2)
                    else:
                        segs = [SegSpec(dz, u.c2, 0, -dy_, -dx_, 1, 0, H, W) for (dy_, dx_) in TAPS3]
                        ops.gemm_nt(segs, w_, din, M, u.c1, 9 * u.c2, spatial=(H, W))
            elif u.kind == "C3":
                din = self._c3_bwd(plan, P, tag, dy, ld, off)
            else:
                din = self._spp_bwd(plan, P, tag, dy, ld, off)
            coff = 0
            for (ref, c, shr), src in zip(u.parts, self.unit_inputs[tag]):
                if not ur.needs_dx[src]:
                    pass
                elif shr == 0:
                    gout[ref] = (din, u.c1, coff)
                else:
                    Hs, Ws = H >> shr, W >> shr
                    dsrc = plan.buf(f"{tag}.dup{coff}", (B * Hs * Ws, c))
                    ops.gather_sum_rows(din, u.c1, dsrc, c, B, Hs, Ws, shr, c, d_off=coff)
                    gout[ref] = (dsrc, c, 0)
                coff += c
        for j in range(3):
            if Ref("enc", j) in gout:
                self._add_extra(plan, extra, Ref("enc", j), gout[Ref("enc", j)])
        return gout

    def _backward_main(self, plan: Plan, P):
        B, th, tw = plan.B, plan.H // 4, plan.W // 4
        wT, g, b = P["wT"], self.g, plan.bufs
        enc = self.model.image_encoder
        U, T = plan.unit, plan.trainable
        ops.zero_(plan.zpool("b"))                   # BN-backward reduction accumulators of every head conv
        T1, T2, T3 = B * th * tw, B * (th // 2) * (tw // 2), B * (th // 4) * (tw // 4)
        # ---- Detect
        hu = self.head.by_row[self.head.head_out[0]]
        cd = self.head.head_out[1]
        gout = {}                                                    # headgraph.Ref -> (buffer, ld, column offset)
        if U("detect").runs_bwd and plan.det_fused:
            if U("detect").any_dx:                                   # written by the live sodt_detect_bwd (_backward, step (1))
                gout[hu.ref] = (b["g.dyd"], cd, 0)
        elif U("detect").runs_bwd:
            dzd = b["g.dzd"]
            if U("detect").any_wgrad:
                ops.gemm_tn(dzd, [SegSpec(b[hu.out_name])], g[self.det_name + "m.0.weight"], T1, self.na * self.no, cd, ldy=self.det_np,
                            lddw=cd, dbias=g[self.det_name + "m.0.bias"])
            if U("detect").any_dx:
                dyd = plan.buf("g.dyd", (T1, cd))
                ops.gemm_nt([SegSpec(dzd)], wT[self.det_name + "m.0.weight"], dyd, T1, cd, self.det_np)
                gout[hu.ref] = (dyd, cd, 0)
        # ---- head units in reverse (the SR branch's input gradients join at their taps)
        extra = self._sr_extra(plan) if self.sr and U("model_up").runs_bwd and U("model_up").any_dx else {}
        gout = self._head_bwd(plan, P, gout, extra)
        (gf0, ld0, off0), (gf1, ld1, off1), (gf2, ld2, off2) = (gout.get(Ref("enc", j), (None, 0, 0)) for j in range(3))
        # where the head's backward ends and the encoder's begins, and the buffers the head left d(f0), d(f1), d(f2) in
        # (token-major rows, `ld` columns, the feature's columns at `off`): replay_encoder_backward re-runs the rest from there
        # (a trainable front end: every unit above it has a backward, the encoder's is recorded whole)
        if U("frontend").runs_bwd:
            plan.enc_bwd_start = ops.recorded_count()
            plan.enc_gin = [(gf0, ld0, off0, 256), (gf1, ld1, off1, 256), (gf2, ld2, off2, 512)]
        # ---- neck3 + stage 3
        d3a = d3b = None
        if U("neck3").runs_bwd:
            s3out = b["stage3.0.xo"]
            d3a = plan.buf("g.dA.768", (T3, 768))
            d3b = plan.buf("g.dB.768", (T3, 768))
            self._linear_bwd(P, E + "neck3", gf2, s3out, d3a, T3, 512, 768, bias=False, ldy=ld2, y_off=off2, plan=plan,
                             need_dx=U("neck3").any_dx)
            self._block_bwd(plan, P, "stage3.0", enc.stage3[0], d3a, d3b)
        # head, neck 3 and stage 3 gradients are final: first data-parallel bucket (ddp.GradReducer.reduce_async)
        self._mark(plan, self.ddp_split3, self.flat_grad.numel())
        # ---- pmerging2 -> d(stage2 out) ; + neck2
        cur = None
        if U("neck2").runs_bwd or U("pmerging2").runs_bwd:
            dA = plan.buf("g.dA.384", (T2, 384))
            dB = plan.buf("g.dB.384", (T2, 384))
            if U("pmerging2").runs_bwd:
                self._merge_bwd(plan, P, "pmerging2", d3b, dA)
            s2out = b["stage2.3.xo"]
            # (the neck and the PatchMerging read the same tensor: both leave an input gradient or neither does)
            if U("neck2").runs_bwd:
                self._linear_bwd(P, E + "neck2", gf1, s2out, dA, T2, 256, 384, bias=False, ldy=ld1, y_off=off1, resid=dA, plan=plan,
                                 need_dx=U("neck2").any_dx)
            cur, other = dA, dB
            for i in reversed(range(4)):
                self._block_bwd(plan, P, f"stage2.{i}", enc.stage2[i], cur, other)
                cur, other = other, cur
        # ---- pmerging1 -> d(stage1 out5) ; + neck1
        n1 = U("neck1").runs_bwd
        if n1 or U("pmerging1").runs_bwd:
            dA = plan.buf("g.dA.192", (T1, 192))
            dB = plan.buf("g.dB.192", (T1, 192))
            if U("pmerging1").runs_bwd:
                self._merge_bwd(plan, P, "pmerging1", cur, dA)
        if n1:
            o4, o5 = b["stage1.4.xo"], b["stage1.5.xo"]
            if T(E + "neck1.weight"):
                ops.gemm_tn(gf0, [SegSpec(o4), SegSpec(o5)], g[E + "neck1.weight"], T1, 256, 384, ldy=ld0, y_off=off0)
            df0 = SegSpec(gf0, 256, off0)
            if U("neck1").needs_dx["stage1.5.mlp"]:          # (then PatchMerging 1 has left its input gradient in dA)
                ops.gemm_nt([df0], wT[E + "neck1.weight"], dA, T1, 192, 256, w_off=192 * 256, resid=dA)        # d out5 += df0 @ Wn1[:,192:]
        # every gradient from PatchMerging 1 to the end of the flat buffer is final here: data-parallel runs start
        # their all-reduce now, under the stage-1 backward (ddp.GradReducer.reduce_async)
        self._mark(plan, self.ddp_split, self.ddp_split3)
        if U("stage1.5.mlp").runs_bwd:
            self._block_bwd(plan, P, "stage1.5", enc.stage1[5], dA, dB)
            if n1 and U("neck1").needs_dx["stage1.4.mlp"]:
                ops.gemm_nt([df0], wT[E + "neck1.weight"], dB, T1, 192, 256, resid=dB)                       # d out4 += df0 @ Wn1[:,:192]
            cur, other = dB, dA
            for i in reversed(range(5)):
                self._block_bwd(plan, P, f"stage1.{i}", enc.stage1[i], cur, other)
                cur, other = other, cur
            # ---- patch_embed 1x1 + pos_embed
            if U("embed").runs_bwd:
                if plan.saved["use_pos"] and T(E + "pos_embed"):
                    ops.batch_sum(cur, g[E + "pos_embed"], B, th * tw * 192)
                dx0 = plan.buf("g.dx0", (T1, 192)) if U("embed").any_dx else None
                self._linear_bwd(P, E + "patch_embed.proj", cur, b["x0"], dx0, T1, 192, 192, plan=plan, need_dx=U("embed").any_dx)
        self._zero_frozen(plan, self.fe_end, self.ddp_split)
