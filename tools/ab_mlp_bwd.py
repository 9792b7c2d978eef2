"""A/B of sodt_mlp_bwd (csrc/mlpbwd.hip) against the three launches it replaces in the stage-1 linear-MLP backward - sodt_gemm_tn
(dW2, db2), sodt_gemm_nt with SODT_EPI_BIAS | SODT_EPI_DGELU_RC (dh) and sodt_gemm_tn (dW1, db1) with the engine's arguments - at
the stage-1 shape: M = 524288 (B = 8 @ 1024^2), C = 192, hidden 768, bf16, the engine's 64 MiB scratch.

  python tools/ab_mlp_bwd.py [--m 524288] [--rounds 5] [--iters 20] [--check] [--once fused|three]
  python tools/ab_mlp_bwd.py --in-step 5

default:      the isolated launches, HIP events on the launch stream, same process; the arms alternate and the minimum / median /
              maximum of the rounds are printed.  Warm caches: this table does not rank, --in-step does.
--check:      first compare the one launch with the three at this shape: dh bit for bit, dW1 / db1 / dW2 / db2 by their largest
              difference relative to the largest element (the three launches read the forward's GELU(h), the one launch its own).
--once:       launch one arm once and exit (for a counter pass under rocprofv3 --pmc FETCH_SIZE, or WRITE_SIZE, each in a run of
              its own).
--in-step N:  the benchmark step (B = 8 @ 1024^2 bf16), HIP events around the launches of the three linear stage-1 blocks where
              they run in the step (the engine's probe tables), N steps per arm in ONE process: first with
              Engine.use_fused_mlp_bwd on, then off (the plans are dropped and recorded again; the three launches' kernels are the
              parent's, csrc/gemm*.hip being unchanged).  New arm: sodt_mlp_bwd (with its reduction) + sodt_mlp_fwd without the
              GELU(h) store; old arm: the three launches (with their reductions) + sodt_mlp_fwd with the store.  Per block: mean of
              the N steps, the old arm's min-max spread over the steps, GB/s against the single-pass byte model.
"""
import argparse, collections, ctypes as C, importlib, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
L = importlib.import_module(bench.PKG + "._lib")
ops = importlib.import_module(bench.PKG + ".ops")
Cc, H4 = 192, 768


def model_bytes(M, splits=32):
    """xn2 and dY read once, dh written once, the partial tiles of both weights written and read back"""
    return M * (2 * Cc + H4) * 2 + 2 * (2 * splits * H4 * Cc * 4)


def isolated(a):
    dev, dt, M = torch.device("cuda:0"), torch.bfloat16, a.m
    g = torch.Generator(device="cpu").manual_seed(0)
    xn = torch.randn(M, Cc, generator=g).to(dt).to(dev)
    dY = torch.randn(M, Cc, generator=g).to(dt).to(dev)
    w1 = (torch.randn(H4, Cc, generator=g) * Cc ** -0.5).to(dt).to(dev)
    w2T = (torch.randn(H4, Cc, generator=g) * Cc ** -0.5).to(dt).to(dev)
    b1 = (torch.randn(H4, generator=g) * 0.5).to(dev)
    wcat = torch.cat([w1, w2T], 1).contiguous()
    dh = torch.empty(M, H4, device=dev, dtype=dt)
    ha = torch.empty(M, H4, device=dev, dtype=dt)
    xo = torch.empty(M, Cc, device=dev, dtype=dt)
    dW1, dW2 = torch.zeros(H4, Cc, device=dev), torch.zeros(Cc, H4, device=dev)
    db1, db2 = torch.zeros(H4, device=dev), torch.zeros(Cc, device=dev)
    ops.set_tn_scratch(torch.empty(16 << 20, dtype=torch.float32, device=dev))       # the engine's scratch
    ops.mlp_fwd(xn, w1, b1, w2T.t().contiguous(), torch.zeros(Cc, device=dev), None, xo, ha, M, Cc)      # the forward's GELU(h)

    def fused():
        assert ops.mlp_bwd(xn, dY, w1, b1, w2T, dh, dW1, db1, dW2, db2, M)

    def three():
        ops.gemm_tn(dY, [ops.SegSpec(ha)], dW2, M, Cc, H4, dbias=db2)
        ops.gemm_nt([ops.SegSpec(xn), ops.SegSpec(dY)], wcat, dh, M, H4, 2 * Cc, bias=b1, dgelu_rc=True)
        ops.gemm_tn(dh, [ops.SegSpec(xn)], dW1, M, H4, Cc, dbias=db1)

    arms = {"fused": fused, "three": three}
    if a.check:
        out = {}
        for arm in ("fused", "three"):
            for t in (dh, dW1, dW2, db1, db2):
                t.zero_()
            arms[arm](); torch.cuda.synchronize()
            out[arm] = [t.clone() for t in (dh, dW1, db1, dW2, db2)]
        f, t = out["fused"], out["three"]
        rel = lambda u, v: float((u - v).abs().max() / v.abs().max())
        print(f"check: dh identical bits: {torch.equal(f[0].view(torch.int16), t[0].view(torch.int16))}; max |diff| / max |.|: "
              f"dW1 {rel(f[1], t[1]):.2e}, db1 {rel(f[2], t[2]):.2e}, dW2 {rel(f[3], t[3]):.2e}, db2 {rel(f[4], t[4]):.2e}", flush=True)
        for t_ in (dW1, dW2, db1, db2):
            t_.zero_()
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
    print(f"M={M} C=192 hidden=768 bf16, {a.rounds} rounds x {a.iters} launches, ms per arm, warm caches (three = gemm_tn + gemm_nt + gemm_tn)")
    print("| arm | min | median | max |\n|---|---|---|---|")
    for k, v in res.items():
        print(f"| {k} | {min(v):.4f} | {statistics.median(v):.4f} | {max(v):.4f} |")
    t = statistics.median(res["fused"])
    sp = ops.mlp_bwd_splits(M)
    print(f"fused: {model_bytes(M, sp) / t / 1e6:.0f} GB/s of the {model_bytes(M, sp) / 1e6:.0f} MB single-pass model", flush=True)


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
    for arm, on in (("fused", True), ("three", False)):
        eng.use_fused_mlp_bwd = on
        eng.plans.clear()                       # the recorded launch lists hold the other arm
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        plan = next(p for k, p in eng.plans.items() if k[3])
        bg, fg = collections.defaultdict(list), collections.defaultdict(list)        # block tag -> indices in bwd_main / fwd_main
        for i, (fn, args, name, tag) in enumerate(plan.fwd_main):
            if name == "sodt_mlp_fwd" and tag.startswith("stage1."):
                fg[tag].append(i)
        for i, (fn, args, name, tag) in enumerate(plan.bwd_main):
            g = struct_of(args)
            blk = tag[:-len(".bwd")] if tag.endswith(".bwd") else tag
            if blk not in fg:                   # (the conv-MLP blocks have a 192 x 768 weight gradient too)
                continue
            if name == "sodt_mlp_bwd":
                bg[blk].append(i)
            elif g is not None and g.M == M and tag.startswith("stage1."):
                if name == "sodt_gemm_tn" and (g.N, g.K) in ((Cc, H4), (H4, Cc)):
                    bg[blk].append(i)
                elif name == "sodt_gemm_nt" and (g.N, g.K) == (H4, 2 * Cc) and (g.flags & L.EPI_DGELU_RC):
                    bg[blk].append(i)
        want = 1 if on else 3
        assert len(bg) == 3 and all(len(v) == want for v in bg.values()), {k: len(v) for k, v in bg.items()}
        assert sorted(fg) == sorted(bg) and all(len(v) == 1 for v in fg.values()), dict(fg)
        ev = lambda ids: {i: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for i in ids}
        evb, evf = ev([i for v in bg.values() for i in v]), ev([i for v in fg.values() for i in v])
        per = collections.defaultdict(list)
        for _ in range(a.in_step):
            eng.probes_bwd, eng.probes_fwd = evb, evf
            step(); torch.cuda.synchronize()
            eng.probes_bwd = eng.probes_fwd = None
            for tag in bg:
                tb = sum(evb[i][0].elapsed_time(evb[i][1]) for i in bg[tag])
                tf = sum(evf[i][0].elapsed_time(evf[i][1]) for i in fg[tag])
                per[tag].append((tb + tf, tb, tf))
        tables[arm] = dict(per)
    eng.use_fused_mlp_bwd = True
    new, old = tables["fused"], tables["three"]
    byt = model_bytes(M, ops.mlp_bwd_splits(M))
    print(f"library: {L.LIB_PATH}\nstage-1 linear MLP in the step, ms per block (events around the launches, reduce kernels included; "
          f"bwd + fwd), {a.in_step} steps per arm\n")
    print("| block | old mean | old min | old max | spread | new mean | new min | new max | saved | keep | old bwd | new bwd | old fwd | new fwd | new bwd GB/s of model |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    keep_all, tn, to = True, 0.0, 0.0
    for tag in sorted(old):
        o, n = [v[0] for v in old[tag]], [v[0] for v in new[tag]]
        om, nm = statistics.mean(o), statistics.mean(n)
        spread = max(o) - min(o)
        keep = om - nm > spread
        keep_all &= keep
        tn += nm; to += om
        ob, nb = statistics.mean(v[1] for v in old[tag]), statistics.mean(v[1] for v in new[tag])
        of, nf = statistics.mean(v[2] for v in old[tag]), statistics.mean(v[2] for v in new[tag])
        print(f"| {tag} | {om:.4f} | {min(o):.4f} | {max(o):.4f} | {spread:.4f} | {nm:.4f} | {min(n):.4f} | {max(n):.4f} | {om - nm:+.4f} | "
              f"{'yes' if keep else 'NO'} | {ob:.4f} | {nb:.4f} | {of:.4f} | {nf:.4f} | {byt / nb / 1e6:.0f} |")
    print(f"\nthree blocks: old {to:.3f} ms, new {tn:.3f} ms per step: {to - tn:+.3f} ms; keep condition (saved > the old arm's min-max "
          f"spread on every block): {'met' if keep_all else 'NOT met'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=524288)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--once", choices=("fused", "three"))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--in-step", type=int, default=0)
    a = ap.parse_args()
    in_step(a) if a.in_step else isolated(a)


if __name__ == "__main__":
    main()
