"""What a freeze list buys at the benchmark's shape (B = 8 @ 1024^2 bf16, ComputeLoss, FusedSGD + ModelEMA: bench.py's step), in one
process on ONE model whose requires_grad flags are switched between the configurations:

  none       nothing frozen
  encoder    everything under image_encoder (Train.py:328-333)
  stage2     the forward prefix through stage 2: front end, patch / pos embed, stage 1, PatchMerging 1, neck 1, stage 2

  python tools/mb_freeze.py [--rounds 5] [--steps 10] [--batch 8] [--size 1024]

Pass 1, memory: per configuration, with no plan cached, two steps; torch.cuda.max_memory_allocated over them and the bytes of the
plan's workspace.  Pass 2, time: the configurations alternate (tools/ab_norm.py's way: every round runs every arm, so drift of the
box lands on all of them), `--steps` steps per arm and round between two device synchronisations; ms per step, min and median over
the rounds, and the forward alone from HIP events around it inside the same steps.  Last, the eval plan's forward (model.eval(),
no_grad) for comparison with the forward of a frozen encoder.

The tool only sets requires_grad and reads public attributes, so the same file runs on a tree that ignores the flags: there
every arm is the unfrozen step, which is the baseline (profiles/r11_freeze.md).  bench.py is not touched and freezes nothing."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

E = "image_encoder."
STAGE2 = tuple(E + s for s in ("channel_embed_", "chan_block.", "patch_embed.", "pos_embed", "stage1.", "pmerging1.", "neck1.", "stage2."))
ARMS = {"none": lambda n: False, "encoder": lambda n: n.startswith(E), "stage2": lambda n: n.startswith(STAGE2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    B, S, dev, dt = a.batch, a.size, torch.device("cuda:0"), torch.bfloat16
    O = importlib.import_module(bench.PKG + ".optim")
    LS = importlib.import_module(bench.PKG + ".loss")
    model = bench.build_model(S, dev, dt)
    ema = O.ModelEMA(model)
    opt = O.FusedSGD(O.set_weight_decay(model), model=model, lr=0.01, momentum=0.937, nesterov=True, ema=ema)     # over ALL parameters
    model.hyp, model.gr, model.nc = dict(LS.DEFAULT_HYP), 1.0, 8
    compute_loss = LS.ComputeLoss(model)
    targets = LS.synthetic_targets(B, 32, 8, seed=0).to(dev)
    g = torch.Generator(device="cpu").manual_seed(2)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    ir = torch.rand(B, 3, S, S, generator=g).to(dev)
    eng = model._get_engine()
    fwd_ev = []

    def freeze(arm):
        for n, p in model.named_parameters():
            p.requires_grad_(not ARMS[arm](n))

    def step(timed=False):
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        pred, _ = model(x, ir, "RGB+IR")
        if timed:
            e1.record()
            fwd_ev.append((e0, e1))
        compute_loss(pred, targets)[0].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        ema.update(model)

    def plan_bytes():
        seen, tot = set(), 0
        for plan in eng.plans.values():
            for t in plan.bufs.values():
                st = t.untyped_storage()
                if st.data_ptr() not in seen:
                    seen.add(st.data_ptr())
                    tot += st.nbytes()
        return tot

    print(f"mb_freeze: B={B} @{S}^2 bf16, ComputeLoss + FusedSGD + ModelEMA; {a.rounds} rounds x {a.steps} steps per arm", flush=True)
    # ---- pass 1: memory, one configuration at a time with no plan cached
    mem = {}
    for arm in ARMS:
        freeze(arm)
        eng.plans.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        step()
        torch.cuda.synchronize()
        mem[arm] = dict(peak=torch.cuda.max_memory_allocated(), base=base, plan=plan_bytes())
        print(f"memory {arm:8s}: max_memory_allocated {mem[arm]['peak'] / 2 ** 30:7.2f} GiB ({base / 2 ** 30:.2f} GiB held before: "
              f"parameters, optimizer, EMA, inputs); plan workspace {mem[arm]['plan'] / 2 ** 30:7.2f} GiB", flush=True)
    # ---- pass 2: time, arms alternating
    eng.plans.clear()
    torch.cuda.empty_cache()
    for arm in ARMS:                                  # every plan recorded and replayed once before anything is timed
        freeze(arm)
        step()
        step()
    times = {arm: [] for arm in ARMS}
    fwd = {arm: [] for arm in ARMS}
    for _ in range(a.rounds):
        for arm in ARMS:
            freeze(arm)
            step()                                    # the switch itself (optimizer map rebuilt, .grad dropped) stays outside
            del fwd_ev[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(timed=True)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) * 1e3 / a.steps)
            fwd[arm].append(statistics.mean(s.elapsed_time(e) for s, e in fwd_ev))
    # ---- the eval plan's forward
    model.eval()
    ev = []
    with torch.no_grad():
        model(x, ir, "RGB+IR")
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                model(x, ir, "RGB+IR")
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) / a.steps)
    model.train()
    print("\n| configuration | step ms min | step ms median | img/s (median) | forward ms median | max_memory_allocated GiB | plan workspace GiB |")
    print("|---|---|---|---|---|---|---|")
    for arm in ARMS:
        med = statistics.median(times[arm])
        print(f"| {arm} | {min(times[arm]):.2f} | {med:.2f} | {B / med * 1e3:.1f} | {statistics.median(fwd[arm]):.2f} | "
              f"{mem[arm]['peak'] / 2 ** 30:.2f} | {mem[arm]['plan'] / 2 ** 30:.2f} |")
    print(f"| eval forward (decode included) | | | | {statistics.median(ev):.2f} (min {min(ev):.2f}) | | |")
    print("\nper round, ms per step: " + "; ".join(f"{arm} {[round(t, 2) for t in times[arm]]}" for arm in ARMS))
    fastest_none, slowest = min(times["none"]), {arm: max(times[arm]) for arm in ARMS if arm != "none"}
    print("every frozen run faster than every unfrozen run: "
          + ", ".join(f"{arm} {slowest[arm] < fastest_none} (slowest {slowest[arm]:.2f} vs fastest none {fastest_none:.2f})" for arm in slowest))
    print(json.dumps({"tool": "mb_freeze", "batch": B, "size": S, "rounds": a.rounds, "steps": a.steps,
                      "step_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
                      "fwd_ms": {k: [round(t, 3) for t in v] for k, v in fwd.items()}, "eval_fwd_ms": [round(t, 3) for t in ev],
                      "max_memory_allocated": {k: v["peak"] for k, v in mem.items()}, "plan_bytes": {k: v["plan"] for k, v in mem.items()}}))


if __name__ == "__main__":
    main()
