"""A/B of sodt_linear_bwd_wide (csrc/linbwd.hip) against the two launches it replaces for attn.qkv, sodt_gemm_tn + sodt_gemm_nt with
the engine's arguments, at the stage-1 shape: M = 524288 (B = 8 @ 1024^2), N = 576, K = 192, bf16, the engine's 64 MiB scratch.

  python tools/ab_linbwd_wide.py [--parent-lib PATH] [--m 524288] [--rounds 5] [--iters 20] [--check] [--once wide|pair]
  python tools/ab_linbwd_wide.py --in-step 5

default:      the isolated launch, HIP events on the launch stream, same process; the arms alternate and the minimum / median /
              maximum of the rounds are printed.  Warm caches: this table does not rank, --in-step does.
--parent-lib: a libsodt_hip.so built from the parent commit; the pair is then ALSO timed through that library.
--check:      first compare the one launch with the pair at this shape: dX bit for bit, dW / dbias by their largest difference
              relative to the largest element.
--once:       launch one arm once and exit (for a counter pass under rocprofv3 --pmc FETCH_SIZE WRITE_SIZE, in a run of its own).
--in-step N:  the benchmark step (B = 8 @ 1024^2 bf16), HIP events around the attn.qkv backward launches of the six stage-1
              blocks where they run in the step (the engine's probe table), N steps per arm in ONE process: first with
              Engine.use_wide_linbwd on, then off (the plans are dropped and recorded again; the pair's kernels are the parent's,
              csrc/gemm*.hip being unchanged).  Per block: mean of the N steps, the pair's min-max spread over the steps, GB/s
              against the 1006 MB single-pass model and the fraction of the same run's best layernorm_bwd C = 192 launch.
"""
import argparse, collections, ctypes as C, importlib, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
L = importlib.import_module(bench.PKG + "._lib")
ops = importlib.import_module(bench.PKG + ".ops")
N, K = 576, 192


def model_bytes(M):
    return M * (N + 2 * K) * 2            # dY and X read once, dX written once


def isolated(a):
    dev, dt, M = torch.device("cuda:0"), torch.bfloat16, a.m
    g = torch.Generator(device="cpu").manual_seed(0)
    dY = torch.randn(M, N, generator=g).to(dt).to(dev)
    X = torch.randn(M, K, generator=g).to(dt).to(dev)
    wT = torch.randn(K, N, generator=g).to(dt).to(dev)
    dX = torch.empty(M, K, device=dev, dtype=dt)
    dW = torch.zeros(N, K, device=dev)
    db = torch.zeros(N, device=dev)
    ops.set_tn_scratch(torch.empty(16 << 20, dtype=torch.float32, device=dev))       # the engine's scratch
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def wide():
        assert ops.linear_bwd_wide(dY, X, wT, dX, dW, M, dbias=db)

    def pair():
        ops.gemm_tn(dY, [ops.SegSpec(X)], dW, M, N, K, dbias=db)
        ops.gemm_nt([ops.SegSpec(dY, N, 0)], wT, dX, M, K, N)

    arms = {"wide": wide, "pair": pair}
    if a.parent_lib:
        plib = C.CDLL(a.parent_lib)
        for n in ("sodt_gemm_tn", "sodt_gemm_nt"):
            getattr(plib, n).argtypes = L.SIGNATURES[n]
            getattr(plib, n).restype = C.c_int
        with ops.Recorder() as rec:                   # the very argument records the wrappers build, replayed through the parent
            pair()
        calls = [(getattr(plib, name), args) for (_, args, name, _) in rec.calls]

        def parent():
            for fn, args in calls:
                assert fn(*args, st) == 0
        arms["parent_pair"] = parent
    if a.check:
        out = {}
        for arm in ("wide", "pair"):
            dX.zero_(); dW.zero_(); db.zero_()
            arms[arm](); torch.cuda.synchronize()
            out[arm] = (dX.clone(), dW.clone(), db.clone())
        (x1, w1, b1), (x2, w2, b2) = out["wide"], out["pair"]
        print(f"check: dX identical bits: {torch.equal(x1.view(torch.int16), x2.view(torch.int16))}; "
              f"dW max |diff| / max |dW| = {float((w1 - w2).abs().max() / w2.abs().max()):.2e}; "
              f"dbias {float((b1 - b2).abs().max() / b2.abs().max()):.2e}", flush=True)
        dW.zero_(); db.zero_()
    if a.once:
        arms[a.once]()
        torch.cuda.synchronize()
        return

    def timeit(fn):
        fn(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].append(timeit(fn))
    print(f"M={M} N=576 K=192 bf16, {a.rounds} rounds x {a.iters} launches, ms per launch, warm caches (pair = gemm_tn + gemm_nt)")
    print("| arm | min | median | max |\n|---|---|---|---|")
    for k, v in res.items():
        print(f"| {k} | {min(v):.4f} | {statistics.median(v):.4f} | {max(v):.4f} |")
    t = statistics.median(res["wide"])
    print(f"wide: {model_bytes(M) / t / 1e6:.0f} GB/s of the {model_bytes(M) / 1e6:.0f} MB single-pass model", flush=True)


def struct_of(args):
    return getattr(args[0], "_obj", None)


def in_step(a):
    B, S, dev = 8, 1024, torch.device("cuda:0")
    model = bench.build_model(S, dev, torch.bfloat16)
    x = torch.rand(B, 3, S, S, device=dev); ir = torch.rand(B, 3, S, S, device=dev)
    M = B * (S // 4) ** 2

    def step():
        pred, _ = model(x, ir, "RGB+IR"); pred[0].float().square().mean().backward()
        for p in model.parameters():
            p.grad = None

    eng = model._get_engine()
    tables = {}
    for arm, on in (("wide", True), ("pair", False)):
        eng.use_wide_linbwd = on
        eng.plans.clear()                       # the recorded launch lists hold the other arm
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        plan = next(p for k, p in eng.plans.items() if k[3])
        groups, refs = collections.defaultdict(list), []        # block tag -> indices in bwd_main
        for i, (fn, args, name, tag) in enumerate(plan.bwd_main):
            g = struct_of(args)
            if name == "sodt_linear_bwd_wide":
                groups[tag].append(i)
            elif name in ("sodt_gemm_tn", "sodt_gemm_nt") and g is not None and g.M == M and tag.startswith("stage1.") and \
                    ((name == "sodt_gemm_tn" and (g.N, g.K) == (N, K)) or (name == "sodt_gemm_nt" and (g.N, g.K) == (K, N))):
                groups[tag].append(i)
            elif name == "sodt_layernorm_bwd":
                v = [getattr(q, "value", q) for q in args]
                if v[9] == 192:
                    refs.append((i, v[8] * ((3 if v[4] else 2) + 1) * 192 * 2 + v[8] * 8))
        want = 1 if on else 2
        assert len(groups) == 6 and all(len(v) == want for v in groups.values()), {k: len(v) for k, v in groups.items()}
        idx = [i for v in groups.values() for i in v] + [i for i, _ in refs]
        evs = {i: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for i in idx}
        per = collections.defaultdict(list)
        best_ref = 0.0
        for _ in range(a.in_step):
            eng.probes_bwd = evs
            step(); torch.cuda.synchronize()
            eng.probes_bwd = None
            for tag, ids in groups.items():
                per[tag].append(sum(evs[i][0].elapsed_time(evs[i][1]) for i in ids))
            best_ref = max(best_ref, max(byt / evs[i][0].elapsed_time(evs[i][1]) / 1e6 for i, byt in refs))
        tables[arm] = (dict(per), best_ref)
    eng.use_wide_linbwd = True
    (wide, refw), (pair, refp) = tables["wide"], tables["pair"]
    byt = model_bytes(M)
    print(f"library: {L.LIB_PATH}\nattn.qkv backward in the step, ms per block (events around the launches, reduce kernels included), "
          f"{a.in_step} steps per arm; best layernorm_bwd C=192 launch: {refw:.0f} GB/s (wide arm), {refp:.0f} GB/s (pair arm)\n")
    print("| block | pair mean | pair min | pair max | spread | wide mean | wide min | wide max | saved | keep | wide GB/s of 1006 MB | of reference |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    keep_all, tw, tp = True, 0.0, 0.0
    for tag in sorted(pair):
        p, w = pair[tag], wide[tag]
        pm, wm = statistics.mean(p), statistics.mean(w)
        spread = max(p) - min(p)
        keep = pm - wm > spread
        keep_all &= keep
        tw += wm; tp += pm
        print(f"| {tag} | {pm:.4f} | {min(p):.4f} | {max(p):.4f} | {spread:.4f} | {wm:.4f} | {min(w):.4f} | {max(w):.4f} | {pm - wm:+.4f} | "
              f"{'yes' if keep else 'NO'} | {byt / wm / 1e6:.0f} | {byt / wm / 1e6 / refw:.2f} |")
    print(f"\nsix blocks: pair {tp:.3f} ms, wide {tw:.3f} ms per step: {tp - tw:+.3f} ms; keep condition (saved > the pair's min-max spread "
          f"on every block): {'met' if keep_all else 'NOT met'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--m", type=int, default=524288)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--once", choices=("wide", "pair"))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--in-step", type=int, default=0)
    a = ap.parse_args()
    in_step(a) if a.in_step else isolated(a)


if __name__ == "__main__":
    main()
