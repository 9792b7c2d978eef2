"""The Detect level and the stride-4 C3's input gradient inside one benchmark step (B = 8 @ 1024^2 bf16), launch by launch.

  python tools/ab_detect.py --in-step 5

HIP events around each single launch where it runs in the step (tools/ab_norm.py --in-step does the same for the normalisation
launches), mean of N steps, with algorithmic bytes, GB/s and the fraction of the same run's best layernorm_bwd C = 192 launch.
The recorded launches (Detect's gemm_tn / gemm_nt where the engine still issues them, the h7 input-gradient GEMMs, the LayerNorm
reference) are probed through the engine's own probe table; the live ones (the Detect forward, detect_unpermute, detect_fwd,
detect_bwd) through a wrapper around the ops entry.  Run in a checkout of the parent commit it prints the parent's table.
"""
import argparse, collections, importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
ops = importlib.import_module(bench.PKG + ".ops")
ES = 2


def struct_of(args):
    return getattr(args[0], "_obj", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-step", type=int, default=5)
    a = ap.parse_args()
    B, S, dev = 8, 1024, torch.device("cuda:0")
    model = bench.build_model(S, dev, torch.bfloat16)
    x = torch.rand(B, 3, S, S, device=dev); ir = torch.rand(B, 3, S, S, device=dev)

    def step():
        pred, _ = model(x, ir, "RGB+IR"); pred[0].float().square().mean().backward()
        for p in model.parameters():
            p.grad = None

    # ---- live launches: events around the ops entry
    live, live_on = collections.defaultdict(list), [False]

    def wrap(name, label, pred=None):
        orig = getattr(ops, name, None)
        if orig is None:
            return
        def f(*args, **kw):
            if not live_on[0] or (pred is not None and not pred(args, kw)):
                return orig(*args, **kw)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); r = orig(*args, **kw); e.record()
            if r is not False:
                live[label].append((s, e))
            return r
        setattr(ops, name, f)
    wrap("gemm_nt", "Detect forward: gemm_nt DETECT", lambda args, kw: kw.get("detect") is not None)
    wrap("detect_unpermute", "detect_unpermute")
    wrap("detect_fwd", "detect_fwd")
    wrap("detect_bwd", "detect_bwd (+ reduce)")

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    eng = model._get_engine()
    plan = next(p for k, p in eng.plans.items() if k[3])
    T1 = B * (S // 4) ** 2
    na, no, cd, npad = eng.na, eng.no, eng.head.head_out[1], eng.det_np

    rows = []                                   # (index, label, bytes)
    refs = []
    for i, (fn, args, name, tag) in enumerate(plan.bwd_main):
        g = struct_of(args)
        if name == "sodt_gemm_tn" and g is not None and g.M == T1 and g.N == na * no and g.K == cd:
            rows.append((i, f"Detect dW/dbias: gemm_tn N={g.N} K={g.K}", T1 * (npad + cd) * ES))
        elif name == "sodt_gemm_nt" and g is not None and g.M == T1 and g.N == cd and g.K == npad:
            rows.append((i, f"Detect dX: gemm_nt N={g.N} K={g.K}", T1 * (npad + cd) * ES))
        elif name == "sodt_gemm_nt" and g is not None and tag.startswith("h7.cv") and g.M == T1 and g.N > 2 * g.K:
            resid = bool(g.flags & 2)
            rows.append((i, f"h7 din: gemm_nt N={g.N} K={g.K}{' +resid' if resid else ''} [{tag}]", T1 * (g.K + g.N * (2 if resid else 1)) * ES))
        elif name == "sodt_layernorm_bwd":
            v = [getattr(q, "value", q) for q in args]
            if v[9] == 192:
                refs.append((i, v[8] * ((3 if v[4] else 2) + 1) * 192 * ES + v[8] * 8))
    evs = {i: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for i, *_ in rows + refs}
    acc = collections.defaultdict(float)
    live_on[0] = True
    for _ in range(a.in_step):
        live.clear()
        eng.probes_bwd = evs
        step(); torch.cuda.synchronize()
        eng.probes_bwd = None
        for i, (s, e) in evs.items():
            acc[i] += s.elapsed_time(e) / a.in_step
        for label, pairs in live.items():
            acc[label] += sum(s.elapsed_time(e) for s, e in pairs) / a.in_step
    live_on[0] = False
    ref = max(byt / acc[i] / 1e6 for i, byt in refs)
    live_bytes = {"Detect forward: gemm_nt DETECT": T1 * (cd * ES + na * no * 4), "detect_fwd": T1 * (cd * ES + na * no * 4),
                  "detect_unpermute": T1 * (na * no * 4 + npad * ES), "detect_bwd (+ reduce)": T1 * (na * no * 4 + 2 * cd * ES)}
    print(f"library: {ops.L.LIB_PATH}\nIn-step time per launch, mean of {a.in_step} steps; reference = best layernorm_bwd C=192 launch: {ref:.0f} GB/s\n")
    print("| launch | alg. MB | us | GB/s | of reference |\n|---|---|---|---|---|")
    tot = 0.0
    table = [(lab, live_bytes[lab], acc[lab]) for lab in live_bytes if lab in acc] + [(lab, byt, acc[i]) for i, lab, byt in rows]
    for lab, byt, ms in table:
        tot += ms
        print(f"| {lab} | {byt / 1e6:.1f} | {ms * 1e3:.1f} | {byt / ms / 1e6:.0f} | {byt / ms / 1e6 / ref:.2f} |")
    print(f"\nsum of the rows: {tot:.3f} ms/step", flush=True)


if __name__ == "__main__":
    main()
