"""The row-streaming normalisation launches of one benchmark step (B = 8 @ 1024^2 bf16), launch by launch: sodt_bn_silu_fwd /
_bwd_reduce / _bwd_apply (csrc/head.hip, 12 Conv+BN+SiLU units = 36 launches) and sodt_layernorm_fwd / _bwd (csrc/norm.hip).  The
argument records are the engine's own (the recorded plan of a real step), so shapes, strides and buffers are the benchmark's.

  python tools/ab_norm.py --in-step 5                      table 1: every launch timed where it runs, inside the step (HIP events around
                                                           that one launch, mean of 5 steps), with shape, algorithmic bytes and GB/s.
                                                           SODT_LIB_PATH=<parent libsodt_hip.so> gives the same table for the parent.
  python tools/ab_norm.py --parent-lib PATH [--check]      table 2: the same records replayed alone, this tree's library against the
                                                           parent's (a second ctypes handle, one process), arms alternating, 5 rounds x
                                                           20 launches per arm; min / median per arm and GB/s against the best
                                                           ln_bwd_half_kernel (layernorm_bwd C = 192) launch of the same run.
  --lib NAME=PATH    further arms for table 2 (builds of csrc/head.hip with other -DBN_*_ROWS / -DBN_*_GRID values)
  --check            before timing: every bn_silu_fwd / _bwd_apply launch through the parent and through this tree's library on the
                     same inputs, outputs compared bit for bit; bn_silu_bwd_reduce sums by their largest relative difference.
  --only bn|ln       restrict table 2 to one family (the C = 192 reference launch always stays)
bench.py refuses SODT_LIB_PATH; this tool is the only place a second library is loaded.
"""
import argparse, collections, ctypes as C, importlib, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
L = importlib.import_module(bench.PKG + "._lib")
ES = 2
BN = ("sodt_bn_silu_fwd", "sodt_bn_silu_bwd_reduce", "sodt_bn_silu_bwd_apply")
LN = ("sodt_layernorm_fwd", "sodt_layernorm_bwd")


def shape_bytes(name, args):
    """(M, C, algorithmic bytes) of one launch: every operand crosses HBM once."""
    args = [getattr(v, "value", v) for v in args]
    if name == "sodt_bn_silu_fwd":
        M, Cc = args[6], args[7]
        return M, Cc, 2 * M * Cc * ES + 16 * Cc
    if name == "sodt_bn_silu_bwd_reduce":
        M, Cc = args[7], args[8]
        return M, Cc, 2 * M * Cc * ES + 32 * Cc
    if name == "sodt_bn_silu_bwd_apply":
        M, Cc = args[10], args[11]
        return M, Cc, 3 * M * Cc * ES + 40 * Cc
    if name == "sodt_layernorm_fwd":
        M, Cc = args[5], args[6]
        return M, Cc, M * (2 * Cc * ES + 8)
    M, Cc = args[8], args[9]
    return M, Cc, M * ((3 if args[4] else 2) + 1) * Cc * ES + M * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-step", type=int, default=0)
    ap.add_argument("--parent-lib")
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", choices=["bn", "ln"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    B, S, dev = 8, 1024, torch.device("cuda:0")
    model = bench.build_model(S, dev, torch.bfloat16)
    x = torch.rand(B, 3, S, S, device=dev); ir = torch.rand(B, 3, S, S, device=dev)

    def step():
        pred, _ = model(x, ir, "RGB+IR"); pred[0].float().square().mean().backward()
        for p in model.parameters():
            p.grad = None
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    eng = model._get_engine(); plan = eng.plans[(B, S, torch.bfloat16, True)]
    rows = []                                 # (which, index, fn, args, name, tag, M, C, bytes)
    for which, calls in (("fwd", plan.fwd_main), ("bwd", plan.bwd_main)):
        for i, (fn, args, name, tag) in enumerate(calls):
            if name in BN + LN:
                rows.append((which, i, fn, args, name, tag) + shape_bytes(name, args))
    print(f"library: {L.LIB_PATH}; {sum(r[4] in BN for r in rows)} BN+SiLU launches, {sum(r[4] in LN for r in rows)} LayerNorm launches per step", flush=True)

    if a.in_step:
        acc = collections.defaultdict(float)
        for which in ("fwd", "bwd"):
            evs = {r[1]: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for r in rows if r[0] == which}
            for _ in range(a.in_step):
                setattr(eng, "probes_" + which, evs)
                step(); torch.cuda.synchronize()
                setattr(eng, "probes_" + which, None)
                for i, (s, e) in evs.items():
                    acc[(which, i)] += s.elapsed_time(e) / a.in_step
        ref = max(r[8] / acc[(r[0], r[1])] / 1e6 for r in rows if r[4] == "sodt_layernorm_bwd" and r[7] == 192)
        print(f"\nIn-step time per launch, mean of {a.in_step} steps; reference = best layernorm_bwd C=192 (ln_bwd_half_kernel) launch: {ref:.0f} GB/s\n")
        print("| launch | tag | M | C | alg. MB | us | GB/s | of reference |\n|---|---|---|---|---|---|---|---|")
        tot = collections.defaultdict(float)
        for which, i, fn, args, name, tag, M, Cc, byt in rows:
            ms = acc[(which, i)]
            tot[name] += ms
            print(f"| {name[5:]} | {tag} | {M} | {Cc} | {byt / 1e6:.1f} | {ms * 1e3:.1f} | {byt / ms / 1e6:.0f} | {byt / ms / 1e6 / ref:.2f} |")
        print("\n" + "; ".join(f"{k[5:]} {v:.3f} ms/step" for k, v in tot.items()), flush=True)
        return

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    libs = collections.OrderedDict(new=None)
    for spec in ([f"parent={a.parent_lib}"] if a.parent_lib else []) + a.lib:
        k, path = spec.split("=", 1)
        lib = libs[k] = C.CDLL(path)
        for n in BN + LN:
            getattr(lib, n).argtypes = L.SIGNATURES[n]
            getattr(lib, n).restype = C.c_int

    def fn_of(arm, r):
        return r[2] if libs[arm] is None else getattr(libs[arm], r[4])

    if a.check and a.parent_lib:
        by_ptr = {t.data_ptr(): t for t in plan.bufs.values()}
        worst = 0.0
        for r in rows:
            name, args = r[4], r[3]
            if name not in BN:
                continue
            oi = {"sodt_bn_silu_fwd": 4, "sodt_bn_silu_bwd_reduce": 6, "sodt_bn_silu_bwd_apply": 7}[name]
            out = by_ptr.get(args[oi])
            if out is None:
                print(f"check {name[5:]} {r[5]}: output buffer not found among the plan's buffers, skipped")
                continue
            got = {}
            for arm in ("parent", "new"):
                out.zero_()
                assert fn_of(arm, r)(*args, st) == 0
                torch.cuda.synchronize()
                got[arm] = out.clone()
            if name == "sodt_bn_silu_bwd_reduce":
                d = float(((got["new"] - got["parent"]).abs() / got["parent"].abs().max().clamp_min(1e-300)).max())
                worst = max(worst, d)
                print(f"check {name[5:]} {r[5]} M={r[6]} C={r[7]}: max |diff| / max |sum| = {d:.2e}")
            else:
                same = torch.equal(got["new"].view(torch.int16), got["parent"].view(torch.int16))
                print(f"check {name[5:]} {r[5]} M={r[6]} C={r[7]}: identical bits: {same}")
                assert same
        print(f"check: every bn_silu_fwd / _bwd_apply output identical to the parent's; reduce sums within {worst:.2e}", flush=True)

    def timeit(fn, args):
        fn(*args, st); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn(*args, st)
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    fam = {"bn": BN, "ln": LN, None: BN + LN}[a.only]
    def keyf(r):                              # one timing per distinct (entry point, M, C, residual operand or row stride)
        name, args = r[4], r[3]
        return (name, r[6], r[7], bool(args[4]) if name == "sodt_layernorm_bwd" else args[5] if name == "sodt_bn_silu_fwd" else args[1] if name in BN else 0)
    count = collections.Counter(keyf(r) for r in rows)
    seen, work = set(), []
    for r in rows:
        key = keyf(r)
        if (r[4] in fam or (r[4] == "sodt_layernorm_bwd" and r[7] == 192)) and key not in seen:
            seen.add(key); work.append((key, r, count[key]))
    res = {}
    for key, r, n in work:
        res[key] = {arm: [] for arm in libs}
        for _ in range(a.rounds):
            for arm in libs:
                res[key][arm].append(timeit(fn_of(arm, r), r[3]))
    ref = max(r[8] / min(res[key]["new"]) / 1e6 for key, r, n in work if r[4] == "sodt_layernorm_bwd" and r[7] == 192)
    print(f"\nReplayed alone, {a.rounds} rounds x {a.iters} launches per arm, us per launch; reference rate (layernorm_bwd C=192, this run): {ref:.0f} GB/s\n")
    arms = list(libs)
    print("| launch | M | C | ld/res | per step | alg. MB | " + " | ".join(f"{k} min | {k} median" for k in arms) + " | new GB/s | of reference | new median < parent min |")
    print("|---|---|---|---|---|---|" + "---|---|" * len(arms) + "---|---|---|")
    saved = 0.0
    for key, r, n in work:
        v = res[key]
        med = statistics.median(v["new"])
        gate = (med < min(v["parent"])) if "parent" in v else None
        if "parent" in v:
            saved += n * (statistics.median(v["parent"]) - med)
        print(f"| {r[4][5:]} | {r[6]} | {r[7]} | {key[3]} | {n} | {r[8] / 1e6:.1f} | "
              + " | ".join(f"{min(v[k]) * 1e3:.1f} | {statistics.median(v[k]) * 1e3:.1f}" for k in arms)
              + f" | {r[8] / med / 1e6:.0f} | {r[8] / med / 1e6 / ref:.2f} | {gate} |")
    if "parent" in libs:
        print(f"\nparent median - new median, summed over the launches of one step: {saved:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
